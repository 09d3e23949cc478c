#!/usr/bin/env python3
"""Time K28 (cgv_lddt_counts; csrc/lddt.hip) against the obvious tensor-op formulation of the same predicate -- chunked
``torch.cdist`` of the models and of their references, the difference, five comparisons, masks and sums -- on the same
GPU, on a random-walk chain (1.5 A steps, noise of 1.5 A per coordinate) at three sizes and two pairings:

    m = 128, 512 (4 096 structures) and 2 048 (1 024 structures); all atoms selected
    paired   T = S: every structure has its own reference
    native   T = 1: one reference for all (the kernel keeps its distances in registers)

    python tools/lddt_probe.py [--repeats 7] [--out profiles/lddt.txt]

Method: device tensors, one warm-up pass of each form, then ``--repeats`` passes, device events around a pass, nothing read
back inside the window; the median and the spread are printed.  The kernel's pass is ``cgv_lddt_counts`` on all structures
at once (both gathers, then the pair kernel; its ``ref_index`` is a host array that the call copies), ``atom_counts`` zeroed
inside the window.  The tensor-op pass computes ``atom_counts [m, 6]`` only -- no per-structure counts -- in chunks sized
for 2^26 distances, so it does less.  A pair test is one unordered pair of one structure: ``S m (m - 1) / 2`` per pass.
The two tables are compared outside the window: ``cdist`` rounds differently from ``sqrtf(sq_dist2)``, so a few pairs on a
threshold may differ; the largest relative difference of an entry is printed, not asserted.  No GPU: the probe fails, it
does not fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 4096), (512, 4096), (2048, 1024))
R0, THRESHOLDS, TOL, RADIUS = 15.0, (0.5, 1.0, 2.0, 4.0), 0.4, 1.7


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, ensemble, lddt
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lddt_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    radius2 = float(lddt.cutoff2_of(R0))
    lines = ["K28 (csrc/lddt.hip) against chunked torch.cdist x 2 + compare + sum -- tools/lddt_probe.py",
             f"command: python tools/lddt_probe.py --repeats {args.repeats} --out profiles/lddt.txt",
             f"random-walk chain, 1.5 A steps, noise 1.5 A; R0 {R0} A, thresholds {THRESHOLDS}, radii {RADIUS} A, tolerance {TOL} A, pairs "
             f"at most 3 bonds apart excluded; median of {args.repeats} passes after one warm-up, device events"]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    for m, S in SHAPES:
        rng = np.random.default_rng(m)
        band = np.zeros((m, m), dtype=bool)
        for k in range(-3, 4):
            band |= np.eye(m, k=k, dtype=bool)
        d_excl = torch.from_numpy(ensemble.pack_mask(band).view(np.int32)).to(dev)
        allowed = torch.from_numpy(~band).to(dev)
        d_sel = torch.arange(m, dtype=torch.int32, device=dev)
        d_r = torch.full((m,), RADIUS, dtype=torch.float32, device=dev)
        c2 = float((np.float32(RADIUS) + np.float32(RADIUS) - np.float32(TOL)) ** 2)
        for name, T in (("paired", S), ("native", 1)):
            step = rng.normal(size=(T, m, 3))
            step *= 1.5 / np.linalg.norm(step, axis=2, keepdims=True)
            ref_h = np.cumsum(step, axis=1).astype(np.float32)
            index = np.arange(S, dtype=np.int32) % T
            ref = torch.from_numpy(ref_h).to(dev)
            x = (ref[torch.from_numpy(index).long().to(dev)] + 1.5 * torch.randn(S, m, 3, device=dev)).contiguous()
            struct = torch.zeros(S, 6, dtype=torch.int32, device=dev)
            atom = torch.zeros(m, 6, dtype=torch.int64, device=dev)
            bad = torch.zeros(S, dtype=torch.int32, device=dev)
            need = int(lib.cgv_lddt_workspace_bytes(S, T, m))
            ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)

            def kernel():
                atom.zero_()
                _lib.call("cgv_lddt_counts", _lib.ptr(x), _lib.ptr(ref), index.ctypes.data, _lib.ptr(d_sel), _lib.ptr(d_excl),
                          _lib.ptr(d_excl), _lib.ptr(d_r), S, T, m, m, radius2, *THRESHOLDS, TOL, _lib.ptr(struct), _lib.ptr(atom),
                          _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())

            chunk = max(1, min(S, (1 << 26) // (m * m)))
            table = torch.zeros(m, 6, dtype=torch.int64, device=dev)
            d_index = torch.from_numpy(index).long().to(dev)

            def tensor_ops():
                table.zero_()
                d0_one = torch.cdist(ref[:1], ref[:1]) if T == 1 else None
                for s0 in range(0, S, chunk):
                    p = x[s0:s0 + chunk]
                    d = torch.cdist(p, p)
                    d0 = d0_one if T == 1 else torch.cdist(ref[d_index[s0:s0 + chunk]], ref[d_index[s0:s0 + chunk]])
                    inc = (d0 < R0) & allowed
                    e = (d - d0).abs()
                    cols = [inc.expand_as(e).sum((0, 2))] + [(inc & (e < t)).sum((0, 2)) for t in THRESHOLDS]
                    cols.append(((d * d < c2) & allowed).sum((0, 2)))
                    table.add_(torch.stack(cols, dim=1))

            k_med, k_min, k_max = timed(kernel)
            t_med, t_min, t_max = timed(tensor_ops)
            rel = ((atom - table).abs().double() / table.clamp(min=1).double()).max().item()
            pairs = m * (m - 1) // 2
            tot = struct.long().sum(0).tolist()
            lines += ["", f"m = {m}, {S} structures, {name} (T = {T}): {pairs * S / 1e6:.1f} M pair tests; included {tot[0] / (pairs * S):.3f} of "
                          f"all pairs, preserved at 0.5 A {tot[1] / max(tot[0], 1):.3f}, clashes {tot[5] / (pairs * S):.4f}",
                      f"cgv_lddt_counts      {k_med:9.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {pairs * S / k_med / 1e6:.1f} G pair tests / s",
                      f"torch cdist form     {t_med:9.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   chunk {chunk} structures; atom table only",
                      f"ratio torch / kernel {t_med / k_med:9.2f}   largest relative difference of an entry of the two atom tables: {rel:.2e}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
