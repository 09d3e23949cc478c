#!/usr/bin/env python3
"""Time K27's moments (cgv_pca_moments; csrc/pca.hip) against the same Gram matrix as torch's fp64 ``F.T @ F`` on a
materialised ``[S, d]`` feature tensor on the same GPU, at two shapes:

    chignolin   166 atoms, its 93 heavy atoms (d = 279),               100 000 structures
    protein     2 000 atoms, the backbone of 125 residues (d = 1 125),   4 096 structures
                (N, CA, C of every 16 atoms; clipped to cgv_pca_max_features())

    python tools/pca_probe.py [--repeats 9] [--out profiles/pca.txt]

The "aligned" structures are seeded and made on the device (a random base in a box at a protein's density plus 0.5 A of
noise; no superposition: K27 reads what K21 wrote, and K21 is not what is timed); the centre is the base.  Method: one
warm-up pass of each form, then ``--repeats`` passes, device events around a pass, nothing read back inside the window; the
passes rotate over ``COPIES`` independent copies of the structures, so no pass finds its input where the last one left it;
median, min and max are printed.  The kernel's pass is the two launches of ``cgv_pca_moments`` on all structures at once
(at 100 000 structures: one call, below the per-launch limit) into zeroed totals; the library form's pass gathers the
selected coordinates, widens them, subtracts the centre -- the ``[S, d]`` fp64 tensor the kernel never forms -- and
multiplies; its time is also given for the product alone on a tensor made beforehand.  The two Gram matrices are compared
outside the window.  Flops: 2 S d^2 for the whole matrix (what the library computes), 2 S 1024 P for the kernel's P upper
tile pairs; the fraction is of the vendor datasheet's 78.6 Tflop/s fp64 matrix peak.  No ratio is fixed in advance; if the
kernel is the slower one the output says so.  No GPU: the probe fails, it does not fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPIES = 4
PEAK = 78.6e12
VOLUME = 10.0                                             # A^3 per atom


def shapes(limit):
    heavy = list(range(93))                               # chignolin: 93 of 166 atoms are heavy; which ones does not matter here
    backbone = [16 * r + k for r in range(125) for k in range(3)][:limit // 3]
    return (("chignolin", 166, heavy, 100000), ("protein", 2000, backbone, 4096))


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, pca
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pca_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = ["K27 (csrc/pca.hip), cgv_pca_moments, against torch fp64 F.T @ F on a materialised [S, d] tensor -- tools/pca_probe.py",
             f"median of {args.repeats} passes after one warm-up each, rotating over {COPIES} copies of the structures, device events; "
             f"fractions of {PEAK / 1e12:.1f} Tflop/s"]

    def timed(fn):
        fn(0)
        torch.cuda.synchronize()
        ms = []
        for k in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(k + 1)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    for name, n, sel_list, S in shapes(pca.limits()["features"]):
        m = len(sel_list)
        d = 3 * m
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        side = (n * VOLUME) ** (1.0 / 3.0)
        base = side * torch.rand(n, 3, device=dev, generator=gen, dtype=torch.float64)
        ys = [(base[None].float() + 0.5 * torch.randn(S, n, 3, device=dev, generator=gen)).contiguous() for _ in range(COPIES)]
        sel = torch.tensor(sel_list, dtype=torch.int32, device=dev)
        sel64 = sel.long()
        bad = torch.zeros(S, dtype=torch.int32, device=dev)
        totals = pca.new_totals(d, dev)
        splits = int(lib.cgv_pca_moments_splits(S, d))
        ws = torch.empty(int(lib.cgv_pca_moments_workspace_bytes(S, d)) // 8, dtype=torch.float64, device=dev)
        gram = torch.empty(d, d, dtype=torch.float64, device=dev)

        def kernel(k):
            totals["cov"].zero_(), totals["sum"].zero_(), totals["n_good"].zero_()
            pca.moments_launch(ys[k % COPIES], sel, base, bad, totals, ws)

        def feats(k):
            return (ys[k % COPIES][:, sel64, :].double() - base[sel64][None]).reshape(S, d)

        def library(k):
            F = feats(k)
            torch.matmul(F.T, F, out=gram)

        made = [feats(k) for k in range(COPIES)]

        def product(k):
            F = made[k % COPIES]
            torch.matmul(F.T, F, out=gram)

        k_med, k_min, k_max = timed(kernel)
        l_med, l_min, l_max = timed(library)
        p_med, p_min, p_max = timed(product)
        kernel(0)
        library(0)
        differ = float((totals["cov"] - gram).abs().max() / gram.abs().max())
        tiles = (d + 31) // 32
        issued, whole = 2.0 * S * 1024 * tiles * (tiles + 1) / 2, 2.0 * S * d * d
        lines += ["", f"{name}: {n} atoms, m = {m} selected (d = {d}), {S} structures: {whole / 1e9:.1f} Gflop for the whole matrix, "
                      f"{issued / 1e9:.1f} Gflop issued by the kernel ({tiles * (tiles + 1) // 2} tile pairs x {splits} ranges), "
                      f"{S * n * 12 / 1e6:.0f} MB of coordinates, [S, d] fp64 would be {S * d * 8 / 1e6:.0f} MB",
                  f"cgv_pca_moments (two launches)          {k_med:10.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   "
                  f"{issued / k_med / 1e9:8.2f} Tflop/s issued = {issued / k_med / 1e-3 / PEAK:.3f} of the peak",
                  f"torch: gather, widen, subtract, F.T @ F {l_med:10.3f} ms  (min {l_min:.3f}, max {l_max:.3f})   "
                  f"{whole / l_med / 1e9:8.2f} Tflop/s = {whole / l_med / 1e-3 / PEAK:.3f} of the peak",
                  f"torch: F.T @ F alone on a made [S, d]   {p_med:10.3f} ms  (min {p_min:.3f}, max {p_max:.3f})   "
                  f"{whole / p_med / 1e9:8.2f} Tflop/s = {whole / p_med / 1e-3 / PEAK:.3f} of the peak",
                  f"ratio torch (with features) / kernel    {l_med / k_med:10.2f}   " +
                  ("K27 is SLOWER than the library product   " if k_med > l_med else "") +
                  f"largest |cov - F.T @ F| / largest |F.T @ F|: {differ:.2e}"]
        print("\n".join(lines[-6:]), flush=True)
        ys = made = None
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
