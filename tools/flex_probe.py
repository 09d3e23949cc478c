#!/usr/bin/env python3
"""Time ``flexibility.mean_structure`` (K21, cgv_align_accumulate; csrc/align_mean.hip) against the obvious tensor-op
formulation -- a batched ``torch.linalg.svd`` Kabsch loop with the same start, stop rule and number of passes -- on the
same GPU, at three shapes:

    dipeptide   22 atoms, 10 heavy selected, 100 000 structures
    chignolin   175 atoms, 93 selected, 20 000 structures
    protein     2000 atoms, all selected, 2 000 structures

    python tools/flex_probe.py [--repeats 5] [--out profiles/flexibility.txt]

The structures are a seeded base plus 0.3 A noise, each randomly rotated and translated.  Method: device tensors, one
warm-up call of each form, then ``--repeats`` calls, wall clock around a synchronised call (both forms read one scalar per
pass, so both contain their host round trips); the median and the spread are printed.  Bytes streamed per second per pass:
a pass reads every structure once, ``S x n x 12`` bytes, over the time of a call divided by its passes.  The Kabsch form
works in fp64 on chunks of 2^22 coordinates, flips the last singular vector where the determinant is negative, and
computes mean, RMSF and RMSD -- what ``mean_structure`` returns.  The two results are compared outside the window and the
largest difference printed, not asserted.  No GPU: the probe fails, it does not fall back."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("dipeptide", 22, 10, 100000), ("chignolin", 175, 93, 20000), ("protein", 2000, 2000, 2000))


def kabsch_mean(x, sel, max_iter=10, tol=1e-4):
    """Generalised Procrustes with batched SVD; ``x [S,n,3]`` fp32 on the device, ``sel`` a LongTensor."""
    import torch
    S, n = x.shape[:2]
    chunk = max(1, (1 << 22) // (3 * n))

    def one_pass(target):
        b = target - target[sel].mean(0, keepdim=True)
        total, dev2, rmsd2 = torch.zeros_like(b), torch.zeros(n, dtype=torch.float64, device=x.device), []
        for s0 in range(0, S, chunk):
            a = x[s0:s0 + chunk].double()
            a = a - a[:, sel].mean(1, keepdim=True)
            u, _, vt = torch.linalg.svd(a[:, sel].transpose(1, 2) @ b[sel])
            d = torch.sign(torch.linalg.det(u @ vt))
            u = torch.cat([u[:, :, :2], u[:, :, 2:] * d[:, None, None]], 2)
            y = a @ (u @ vt)
            total += y.sum(0)
            diff = y - b
            dev2 += (diff * diff).sum(2).sum(0)
            rmsd2.append((diff[:, sel] ** 2).sum(2).mean(1))
        return total / S, dev2 / S, torch.cat(rmsd2), b

    target, passes = x[0].double(), 0
    for _ in range(max_iter):
        new, _, _, b = one_pass(target)
        move = float(torch.sqrt(((new - b)[sel] ** 2).sum(1).mean()))
        target, passes = new, passes + 1
        if move < tol:
            break
    mean, msf, rmsd2, b = one_pass(target)
    rmsf = torch.sqrt(torch.clamp(msf - ((mean - b) ** 2).sum(1), min=0.0))
    return mean.cpu().numpy(), rmsf.cpu().numpy(), torch.sqrt(rmsd2).cpu().numpy(), passes + 1


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import flexibility
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flex_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["K21 (csrc/align_mean.hip) mean_structure against a batched torch.linalg.svd Kabsch loop -- tools/flex_probe.py",
             f"0.3 A noise about a seeded base, median of {args.repeats} calls after one warm-up, wall clock around a synchronised call"]

    def timed(fn):
        out = fn()
        torch.cuda.synchronize()
        s = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            s.append(1e3 * (time.perf_counter() - t0))
        return out, statistics.median(s), min(s), max(s)

    for name, n, m, S in SHAPES:
        rng = np.random.default_rng(n)
        base = rng.uniform(0, (4.0 * n) ** (1.0 / 3.0) * 2.0, (n, 3))
        rot = np.linalg.qr(rng.standard_normal((S, 3, 3)))[0]
        rot = rot * np.sign(np.linalg.det(rot))[:, None, None]
        noisy = base[None] + 0.3 * rng.standard_normal((S, n, 3))
        x = torch.from_numpy((noisy @ rot + rng.uniform(-5, 5, (S, 1, 3))).astype(np.float32)).to(dev)
        sel = np.sort(rng.permutation(n)[:m])
        d_sel = torch.from_numpy(sel).to(dev)
        got, k_med, k_min, k_max = timed(lambda: flexibility.mean_structure(x, sel, structures_per_launch=1 << 16))
        (mean, rmsf, rmsd, passes), t_med, t_min, t_max = timed(lambda: kabsch_mean(x, d_sel))
        gb = S * n * 12 / 1e9
        lines += ["", f"{name}: n = {n}, m = {m}, {S} structures, {gb * 1e3:.1f} MB per pass; passes: kernel {got['iterations']}, Kabsch {passes}",
                  f"mean_structure       {k_med:9.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {gb * got['iterations'] / k_med * 1e3:8.1f} GB/s per pass",
                  f"torch svd Kabsch     {t_med:9.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   {gb * passes / t_med * 1e3:8.1f} GB/s per pass",
                  f"ratio torch / kernel {t_med / k_med:9.2f}   largest |rmsf difference| {np.abs(rmsf - got['rmsf']).max():.2e} A, "
                  f"|rmsd difference| {np.abs(rmsd - got['rmsd']).max():.2e} A"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
