#!/usr/bin/env python3
"""Time K23 (cgv_sasa_counts; csrc/sasa.hip) against a chunked tensor-op composition of the SAME definition on the same
GPU, at three shapes and two point counts:

    chignolin   166 atoms, 10 000 structures
    dipeptide    22 atoms, 100 000 structures
    protein    2000 atoms, 64 structures            each with P = 256 and P = 960 sphere points

    python tools/sasa_probe.py [--repeats 7] [--torch_repeats 2] [--out profiles/sasa.txt]

The structures are seeded: atoms uniform in a ball at 0.085 atoms / A^3 (the density of a folded protein with its
hydrogens), elements H 50 %, C 30 %, O 10 %, N 8 %, S 2 %, Bondi radii, probe 1.4 A.  Method: device tensors, one
warm-up pass of each form, then ``--repeats`` passes of the kernel and ``--torch_repeats`` of the tensor-op form (a pass
of which takes seconds), device events around a pass, nothing read back inside the window; median, min and max are
printed.  The kernel's pass is ``cgv_sasa_counts`` on all structures at once with per-atom counts, sums zeroed inside
the window.  The tensor-op pass builds, for a piece of at most 2^26 (point, occluder) pairs at a time, the points
``c_i + r_i u_k``, the squared distances in the operation order of ``sq_dist2``, the comparison with ``r_j^2``, the mask of
``j == i``, "any" over the occluders and the count -- the same per-atom counts, and they are compared with the kernel's
outside the window (eager fp32 tensor ops round every operation, so the two agree exactly; the number of differing
entries is printed).  The rate is the definition's S m P (m - 1) point-occluder tests over the time: what the tensor-op
form really performs, and what the kernel's pre-filter and early exits let it skip.  No GPU: the probe fails, it does not
fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("chignolin", 166, 10000), ("dipeptide", 22, 100000), ("protein", 2000, 64))
POINTS = (256, 960)
PIECE = 1 << 26
DENSITY = 0.085


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, ensemble, sasa
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--torch_repeats", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sasa_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = ["K23 (csrc/sasa.hip) against a chunked tensor-op composition of the same definition -- tools/sasa_probe.py",
             f"probe 1.4 A, Bondi radii, atoms uniform in a ball at {DENSITY} / A^3; median of {args.repeats} kernel passes and "
             f"{args.torch_repeats} tensor-op passes after one warm-up each, device events"]

    def timed(fn, repeats):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    for name, m, S in SHAPES:
        rng = np.random.default_rng(m)
        z = rng.choice([1, 6, 8, 7, 16], size=m, p=[0.5, 0.3, 0.1, 0.08, 0.02])
        radius = (3.0 * m / (4.0 * np.pi * DENSITY)) ** (1.0 / 3.0)
        v = rng.standard_normal((S, m, 3))
        v *= (radius * rng.random((S, m, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=2, keepdims=True)
        x = torch.from_numpy(v.astype(np.float32)).to(dev)
        r = sasa.inflated(sasa.radii_of(z, np.arange(m)), 1.4)
        cls, ids, _ = sasa.device_classes(sasa.polarity(z), r)
        C = int(ids.shape[0])
        d_sel, d_r, d_cls = (torch.from_numpy(a).to(dev) for a in (np.arange(m, dtype=np.int32), r, cls))
        d_r2 = d_r * d_r
        for P in POINTS:
            d_u = torch.from_numpy(sasa.sphere_points(P)).to(dev)
            counts = torch.zeros(S, m, dtype=torch.int32, device=dev)
            class_counts = torch.zeros(S, C, dtype=torch.int32, device=dev)
            sums = torch.zeros(2, m, dtype=torch.int64, device=dev)
            bad = torch.zeros(S, dtype=torch.int32, device=dev)
            ws = ensemble.workspace(int(lib.cgv_sasa_workspace_bytes(S, m, P)), dev)

            def kernel():
                sums.zero_()
                _lib.call("cgv_sasa_counts", _lib.ptr(x), _lib.ptr(d_sel), _lib.ptr(d_r), _lib.ptr(d_u), _lib.ptr(d_cls), S, m, m, P, C,
                          _lib.ptr(counts), _lib.ptr(class_counts), _lib.ptr(sums[0]), _lib.ptr(sums[1]), _lib.ptr(bad), _lib.ptr(ws),
                          ws.numel() * 8, _lib.stream_ptr())

            per_i = max(1, min(m, PIECE // (P * m)))                  # atoms i of a piece
            per_s = max(1, PIECE // (per_i * P * m)) if per_i == m else 1
            table = torch.zeros(S, m, dtype=torch.int32, device=dev)

            def tensor_ops():
                for s0 in range(0, S, per_s):
                    xs = x[s0:s0 + per_s]
                    for i0 in range(0, m, per_i):
                        ci, ri = xs[:, i0:i0 + per_i], d_r[i0:i0 + per_i]
                        a = ci.shape[1]
                        p = ci[:, :, None, :] + ri[None, :, None, None] * d_u[None, None, :, :]           # [c, a, P, 3]
                        dx = p[..., 0][..., None] - xs[:, None, None, :, 0]
                        d2 = dx * dx
                        dy = p[..., 1][..., None] - xs[:, None, None, :, 1]
                        d2 = d2 + dy * dy
                        dz = p[..., 2][..., None] - xs[:, None, None, :, 2]
                        buried = (d2 + dz * dz) < d_r2[None, None, None, :]                               # [c, a, P, m]
                        own = torch.arange(a, device=dev)
                        buried[:, own, :, i0 + own] = False
                        table[s0:s0 + per_s, i0:i0 + per_i] = (~buried.any(dim=3)).sum(dim=2)

            k_med, k_min, k_max = timed(kernel, args.repeats)
            t_med, t_min, t_max = timed(tensor_ops, args.torch_repeats)
            differ = int((counts != table).sum().item())
            tests = float(S) * m * P * (m - 1)
            exposed = float(counts.sum().item()) / (float(S) * m * P)
            lines += ["", f"{name}: m = {m}, {S} structures, P = {P}: {tests / 1e9:.2f} G point-occluder tests by the definition, "
                          f"{100 * exposed:.1f} % of the points exposed",
                      f"cgv_sasa_counts      {k_med:10.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {tests / k_med / 1e6:9.1f} G tests / s",
                      f"tensor-op form       {t_med:10.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   {tests / t_med / 1e6:9.1f} G tests / s   "
                      f"pieces of {per_s} structures x {per_i} atoms",
                      f"ratio torch / kernel {t_med / k_med:10.2f}   per-atom counts of the two forms that differ: {differ} of {S * m}"]
            print("\n".join(lines[-5:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
