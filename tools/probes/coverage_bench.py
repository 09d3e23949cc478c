#!/usr/bin/env python3
"""Time K17 (cgv_superpose; csrc/superpose.hip) at chignolin size: 166 atoms, the heavy atoms of the capped 16-residue
peptide of ``internal_hist_bench.py`` (83; chignolin itself has 93 of its 166), 16 384 x 16 384 structures, against a batched torch
Kabsch (fp64 ``torch.linalg.svd`` of the 3 x 3 cross-covariances with the determinant correction) on the same GPU.

    python tools/probes/coverage_bench.py [--structures 16384] [--per-launch 4096] [--repeats 5] [--torch-rows 64]
                                          [--out profiles/coverage.txt]

The structures are a seeded random embedding with Gaussian displacements (the kernel's work does not depend on the
values).  Method: one warm-up pass, then ``--repeats`` passes of ``coverage.nearest``'s launch loop over the whole
rectangle (device tensors, running minima on the device, no read-back inside the window), device events around a pass;
the median is printed beside the 18 Sa Sb m flop of the nine cross-covariance sums (matrix pipe; the Jacobi epilogue on
the fp64 VALU is not counted).  The torch baseline is timed on ``--torch-rows`` rows against all columns (its
``[rows, Sb, 3, 3]`` intermediates do not fit for all rows at once) and scaled to the full rectangle."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def torch_kabsch_rows(A, B, m):
    """min over the columns of the superposed rmsd^2 of centred fp64 ``A [r,m,3]`` against ``B [S,m,3]``."""
    import torch
    M = torch.einsum("ikx,jky->ijxy", A, B)
    U, S, Vt = torch.linalg.svd(M)
    d = torch.where(torch.linalg.det(U) * torch.linalg.det(Vt) < 0, -1.0, 1.0)
    lam = S[..., 0] + S[..., 1] + d * S[..., 2]
    G = (A * A).sum((1, 2))[:, None] + (B * B).sum((1, 2))[None, :]
    return (torch.clamp(G - 2.0 * lam, min=0.0) / m).min(dim=1)


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, coverage
    from internal_hist_bench import peptide
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=16384)
    ap.add_argument("--per-launch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-rows", type=int, default=64)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "coverage.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("coverage_bench: no GPU; a time per pass cannot be measured here", file=sys.stderr)
        return 1
    z, _ = peptide("AAAAAAAGAAAAAAAG")
    z = np.array(z)
    n = len(z)
    sel = coverage.select_atoms(z, "heavy")
    m, S, P = len(sel), args.structures, args.per_launch
    rng = np.random.default_rng(0)
    x0 = np.cumsum(rng.standard_normal((n, 3)) * 0.9, axis=0)
    a = torch.from_numpy((x0[None] + 0.3 * rng.standard_normal((S, n, 3))).astype(np.float32)).cuda()
    b = torch.from_numpy((x0[None] + 0.3 * rng.standard_normal((S, n, 3))).astype(np.float32)).cuda()
    stab = torch.from_numpy(sel.astype(np.int32)).cuda()
    ws = torch.empty(int(_lib.load().cgv_superpose_workspace_bytes(min(P, S), min(P, S))) // 8 + 1, dtype=torch.float64, device="cuda")

    def one_pass():
        st = coverage.new_state(S, S, "cuda")
        for oa in range(0, S, P):
            for ob in range(0, S, P):
                coverage.superpose_launch(a[oa:oa + P], b[ob:ob + P], stab, st["row_min"][oa:oa + P], st["row_arg"][oa:oa + P],
                                          st["col_min"][ob:ob + P], st["col_arg"][ob:ob + P], oa, ob, workspace=ws)
        return st
    one_pass()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        st = one_pass()
        end.record()
        torch.cuda.synchronize()
        times.append(beg.elapsed_time(end))
    med = statistics.median(times)
    flop = 18.0 * S * S * m
    lines = [f"K17 (csrc/superpose.hip) at chignolin size -- tools/probes/coverage_bench.py",
             f"n = {n}, m = {m} heavy atoms, {S} x {S} structures = {S * S / 1e6:.1f} M pairs, {P} structures per launch "
             f"({((S + P - 1) // P) ** 2} calls per pass), workspace {ws.numel() * 8 / 1e6:.1f} MB",
             "",
             f"cgv_superpose     median {med:.1f} ms per pass (min {min(times):.1f}, max {max(times):.1f}, {args.repeats} passes)  |  "
             f"{S * S / med / 1e6:.2f} G pairs/s  |  18 Sa Sb m = {flop / 1e12:.2f} Tflop on the matrix pipe: {flop / med / 1e9:.2f} Tflop/s fp64"]
    # the torch baseline on a strip of rows, against the kernel's own minima
    r = min(args.torch_rows, S)
    A = a[:r, stab.long()].double()
    A = A - A.mean(1, keepdim=True)
    B = b[:, stab.long()].double()
    B = B - B.mean(1, keepdim=True)
    torch_kabsch_rows(A, B, m)
    torch.cuda.synchronize()
    tt = []
    for _ in range(3):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        got = torch_kabsch_rows(A, B, m)
        end.record()
        torch.cuda.synchronize()
        tt.append(beg.elapsed_time(end))
    tmed = statistics.median(tt)
    diff = float((got.values - st["row_min"][:r]).abs().max())
    same = int((got.indices.int() == st["row_arg"][:r]).sum())
    lines += [f"torch Kabsch      median {tmed:.1f} ms for {r} rows x {S} columns (fp64 einsum + torch.linalg.svd + det, min over the "
              f"columns) = {tmed * S / r:.0f} ms scaled to all rows  |  x{tmed * S / r / med:.0f} the kernel's pass",
              f"agreement         max |row_min^2 - torch| = {diff:.3e} A^2 on those rows, {same} of {r} nearest indices equal"]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
