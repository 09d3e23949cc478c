#!/usr/bin/env python3
"""Time K25 (cgv_hbond_counts; csrc/hbond.hip) against a chunked tensor-op restatement of the SAME predicate on the same
GPU, at two shapes:

    chignolin   166 atoms, table 25 donor hydrogens x 35 acceptors, 100 000 structures
    protein    2000 atoms, table 200 x 360, 4 096 structures

    python tools/hbond_probe.py [--repeats 9] [--torch_repeats 3] [--out profiles/hbond.txt]

The structures are seeded and made on the device: atoms uniform in a ball at 0.085 atoms / A^3, every donor hydrogen 1 A
from its donor in a random direction; the donors are the first nH acceptors, and a pair whose acceptor is the donor itself
is excluded.  Cutoff 2.5 A, angle 120 degrees.  Method: one warm-up pass of each form, then ``--repeats`` passes of the
kernel and ``--torch_repeats`` of the tensor-op form, device events around a pass, nothing read back inside the window;
the passes rotate over ``COPIES`` independent copies of the structures (together larger than the 256 MB memory-side
cache), so no pass finds its input where the last one left it; median, min and max are printed.  The kernel's pass is
``cgv_hbond_counts`` on all structures at once, once with and once without ``bits``, the table zeroed inside the window.
The tensor-op pass forms, for a piece of at most 2^24 (structure, pair) entries at a time, u, v, d2, l2, dot and the three
comparisons in the operation order of the kernel, and sums the table and the per-structure counts -- it is compared with
the kernel's result outside the window (eager fp32 tensor ops round every operation, so the two agree exactly; the number
of differing entries is printed).  The rate is S nH nA pair tests over the time.  No GPU: the probe fails, it does not
fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("chignolin", 166, 25, 35, 100000), ("protein", 2000, 200, 360, 4096))
COPIES = 4
PIECE = 1 << 24
DENSITY = 0.085


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, hbonds
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--torch_repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hbond_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cutoff2, c2 = hbonds.cutoff2_of(2.5), hbonds.c2_of(120.0)
    lines = ["K25 (csrc/hbond.hip) against a chunked tensor-op restatement of the same predicate -- tools/hbond_probe.py",
             f"cutoff 2.5 A, angle 120 degrees, atoms uniform in a ball at {DENSITY} / A^3; median of {args.repeats} kernel passes and "
             f"{args.torch_repeats} tensor-op passes after one warm-up each, rotating over {COPIES} copies of the structures, device events"]

    def timed(fn, repeats):
        fn(0)
        torch.cuda.synchronize()
        ms = []
        for k in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(k + 1)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    for name, n, nH, nA, S in SHAPES:
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        radius = (3.0 * n / (4.0 * np.pi * DENSITY)) ** (1.0 / 3.0)
        don_h = np.arange(nH, dtype=np.int32)
        acc = np.arange(nH, nH + nA, dtype=np.int32)
        don_d = acc[:nH].copy()
        excl = acc[None, :] == don_d[:, None]
        xs = []
        for _ in range(COPIES):
            v = torch.randn(S, n, 3, device=dev, generator=gen)
            v = v * (radius * torch.rand(S, n, 1, device=dev, generator=gen) ** (1.0 / 3.0) / v.norm(dim=2, keepdim=True))
            w = torch.randn(S, nH, 3, device=dev, generator=gen)
            v[:, :nH] = v[:, nH:2 * nH] + w / w.norm(dim=2, keepdim=True)
            xs.append(v.contiguous())
        d_h, d_d, d_a = (torch.from_numpy(a).to(dev) for a in (don_h, don_d, acc))
        d_excl = torch.from_numpy(hbonds.pack_mask(excl).view(np.int64)).to(dev)
        d_allowed = torch.from_numpy(~excl).to(dev)
        W = (nA + 63) // 64
        table = torch.zeros(nH, nA, dtype=torch.int64, device=dev)
        per = torch.zeros(3, S, dtype=torch.int32, device=dev)
        bits = torch.zeros(S, nH, W, dtype=torch.int64, device=dev)
        need = int(lib.cgv_hbond_workspace_bytes(S, nH, nA))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)

        def kernel(k, with_bits=False):
            table.zero_()
            _lib.call("cgv_hbond_counts", _lib.ptr(xs[k % COPIES]), _lib.ptr(d_h), _lib.ptr(d_d), _lib.ptr(d_a), _lib.ptr(d_excl), None,
                      S, n, nH, nA, float(cutoff2), float(c2), _lib.ptr(table), _lib.ptr(per[0]), _lib.ptr(per[1]), _lib.ptr(per[2]),
                      _lib.ptr(bits) if with_bits else None, _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())

        piece = max(1, PIECE // (nH * nA))
        t_table = torch.zeros(nH, nA, dtype=torch.int64, device=dev)
        t_n = torch.zeros(S, dtype=torch.int32, device=dev)
        f_cut, f_c2 = float(cutoff2), float(c2)

        def tensor_ops(k):
            x = xs[k % COPIES]
            t_table.zero_()
            for s0 in range(0, S, piece):
                c = x[s0:s0 + piece]
                H, D, A = c[:, d_h.long()], c[:, d_d.long()], c[:, d_a.long()]
                u = D - H                                                     # [c, nH, 3]
                v = A[:, None, :, :] - H[:, :, None, :]                       # [c, nH, nA, 3]
                d2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
                l2 = ((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])[:, :, None]
                dot = (u[..., 0, None] * v[..., 0] + u[..., 1, None] * v[..., 1]) + u[..., 2, None] * v[..., 2]
                hit = (d2 < f_cut) & (dot < 0) & (dot * dot > (f_c2 * l2) * d2) & d_allowed[None]
                t_table.add_(hit.sum(dim=0))
                t_n[s0:s0 + piece] = hit.sum(dim=(1, 2))

        k_med, k_min, k_max = timed(kernel, args.repeats)
        b_med, b_min, b_max = timed(lambda k: kernel(k, True), args.repeats)
        t_med, t_min, t_max = timed(tensor_ops, args.torch_repeats)
        kernel(0)                                                             # both forms on the same copy
        tensor_ops(0)
        differ = int((table != t_table).sum().item()) + int((per[0] != t_n).sum().item())
        tests = float(S) * nH * nA
        bonded = float(table.sum().item()) / tests
        in_bytes = float(S) * n * 12
        lines += ["", f"{name}: {n} atoms, table {nH} x {nA}, {S} structures: {tests / 1e9:.3f} G pair tests, {100 * bonded:.2f} % bonded, "
                      f"{in_bytes / 1e6:.0f} MB of coordinates, {S * nH * W * 8 / 1e6:.0f} MB of bits",
                  f"cgv_hbond_counts            {k_med:10.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {tests / k_med / 1e6:9.1f} G tests / s   "
                  f"{in_bytes / k_med / 1e6:7.1f} GB / s of coordinates",
                  f"cgv_hbond_counts with bits  {b_med:10.3f} ms  (min {b_min:.3f}, max {b_max:.3f})   {tests / b_med / 1e6:9.1f} G tests / s",
                  f"tensor-op form              {t_med:10.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   {tests / t_med / 1e6:9.1f} G tests / s   "
                  f"pieces of {piece} structures",
                  f"ratio torch / kernel        {t_med / k_med:10.2f}   entries of the table and of n_hbonds that differ: {differ} of {nH * nA + S}"]
        print("\n".join(lines[-6:]), flush=True)
        xs = bits = ws = None
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
