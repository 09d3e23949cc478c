#!/usr/bin/env python3
"""Time K22 (cgv_kde_sums; csrc/kde.hip) against the obvious tensor-op formulation -- a chunked
``exp(-cdist^2)`` sum in torch -- on the same GPU, in the same process:

    N = 10^4 and 10^5 samples, M = 100^2 and 300^2 grid nodes, one 2-D plane, no periodic axis
    P = 8 planes of N = 10^4, M = 100^2, both axes periodic (the Ramachandran planes of a peptide)

    python tools/kde_probe.py [--repeats 7] [--out profiles/kde.txt]

The samples are seeded two-basin data in kernel units (a few kernel widths across), the points a regular grid over them.
Method: device tensors, one warm-up pass of each form, then ``--repeats`` passes, device events around a pass, nothing read
back inside the window; the median and the spread are printed.  The kernel's pass is both launches of ``cgv_kde_sums``
with the automatic split.  The tensor-op pass is ``torch.exp2(-torch.cdist(q, s) ** 2).sum(1)`` over chunks of points
sized for 2^27 distances, in fp32, without minimum image (so it does less on the periodic shape).  Terms per second are
N x M x P / time; the transcendental issue rate they are a fraction of is 256 CUs x 4 SIMDs x 8 lanes x 2.4 GHz =
19.7e12 / s (one v_exp_f32 per wave every 8 cycles).  The worst error of the kernel as a fraction of its derived bound
(tests/density_restatement.py) is measured at the first shape against an fp64 torch sum.  No GPU: the probe fails, it
does not fall back."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1, 10 ** 4, 100, False), (1, 10 ** 4, 300, False), (1, 10 ** 5, 100, False), (1, 10 ** 5, 300, False), (8, 10 ** 4, 100, True))
RATE = 256 * 4 * 8 * 2.4e9


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, density
    import density_restatement as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kde_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = ["K22 (csrc/kde.hip) against a chunked torch exp2(-cdist^2) sum -- tools/kde_probe.py",
             f"median of {args.repeats} passes after one warm-up, device events; transcendental issue rate {RATE / 1e12:.2f} T terms / s"]

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

    for P, N, G, periodic in SHAPES:
        rng = np.random.default_rng(N + G)
        M = G * G
        W = 12.0 if periodic else 0.0
        s = np.concatenate([rng.normal(0.0, 2.0, (P, N - N // 3, 2)), rng.normal(3.0, 1.2, (P, N // 3, 2))], axis=1)
        axis = np.linspace(-6.0, 6.0, G, endpoint=not periodic)
        q = np.broadcast_to(np.stack(np.meshgrid(axis, axis, indexing="ij"), -1).reshape(1, M, 2), (P, M, 2))
        if periodic:
            s = s - W * np.rint(s / W)
        d_s, d_q = torch.from_numpy(s.astype(np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        d_w = torch.full((P, 2), W, dtype=torch.float32, device=dev) if periodic else None
        splits = int(lib.cgv_kde_splits(P, N, M))
        ws = torch.empty(int(lib.cgv_kde_workspace_bytes(P, M, splits)) // 8, dtype=torch.float64, device=dev)
        out = {}

        def kernel():
            out["k"] = density.kde_sums(d_s, d_q, d_w, workspace=ws)[0]

        chunk = max(1, min(M, (1 << 27) // N))

        def tensor_ops():
            parts = []
            for p in range(P):
                parts.append(torch.cat([torch.exp2(-torch.cdist(d_q[p, m0:m0 + chunk], d_s[p]) ** 2).sum(1) for m0 in range(0, M, chunk)]))
            out["t"] = torch.stack(parts)

        k_med, k_min, k_max = timed(kernel)
        t_med, t_min, t_max = timed(tensor_ops)
        terms = float(P) * N * M
        lines += ["", f"P = {P}, N = {N}, M = {G} x {G}{', both axes periodic' if periodic else ''}: {terms / 1e9:.2f} G terms, {splits} sample ranges",
                  f"cgv_kde_sums         {k_med:9.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {terms / k_med / 1e9:.2f} T terms / s = "
                  f"{terms / (k_med * 1e-3) / RATE:.3f} of the transcendental issue rate",
                  f"torch exp2(-cdist^2) {t_med:9.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   chunk {chunk} points, fp32{', no minimum image' if periodic else ''}",
                  f"ratio torch / kernel {t_med / k_med:9.2f}"]
        if (P, N, G) == (1, 10 ** 4, 100):
            d64 = torch.cat([torch.exp2(-torch.cdist(d_q[0, m0:m0 + 2048].double(), d_s[0].double()) ** 2).sum(1) for m0 in range(0, M, 2048)])
            U = float(max(d_s.abs().max(), d_q.abs().max()))
            ratio = R.error_ratio(out["k"][0].cpu().numpy(), d64.cpu().numpy(), N, U)
            t_ratio = R.error_ratio(out["t"][0].double().cpu().numpy(), d64.cpu().numpy(), N, U)
            lines.append(f"worst error / bound against an fp64 sum (U = {U:.1f}, bound {R.relative_bound(U):.3g} relative): kernel {ratio:.3g}, "
                         f"torch fp32 form {t_ratio:.3g}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
