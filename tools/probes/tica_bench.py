#!/usr/bin/env python3
"""Time K16 (cgv_tica_moments, cgv_tica_project; csrc/tica.hip) at chignolin size: 166 atoms, the distance features of
the real backbone rule (``tica.backbone_atoms`` / ``tica.distance_pairs(sel, 2)``), T = 100 000 frames, lag = 100, and a
projection of S = 16 384 structures onto two components.

    python tools/probes/tica_bench.py [--frames 100000] [--lag 100] [--structures 16384] [--launches 20] [--repeats 5]
                                      [--cpu-frames 5000]

The molecule is the capped 16-residue peptide of ``internal_hist_bench.py`` (166 atoms, a bond graph that needs no
topology file); chignolin has 10 residues, so the backbone atoms of the first 10 residues are selected: 30 atoms, the
feature count of the real molecule (d = 416).  The frames are a seeded random embedding with Gaussian displacements (the
kernels' work does not depend on the values).  Method: 3 warm-up calls, then ``--repeats`` windows of ``--launches`` back-to-back calls each, device
events around a window, the totals zeroed once before it (the call adds).  Prints the median time per call beside the
flop count 6 N d^2 of the three products as the textbook counts them (the kernel uses the symmetry of two of them:
4 N d^2 are issued, plus the diagonal tiles' lower halves) and, for scale, the time of the numpy restatement's einsum
moments for ``--cpu-frames`` frames on this machine's CPU with the thread count numpy reports."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def windows(launch, zero, launches, repeats):
    import torch
    times = []
    for _ in range(repeats):
        zero()
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        for _ in range(launches):
            launch()
        end.record()
        torch.cuda.synchronize()
        times.append(beg.elapsed_time(end) * 1e3 / launches)
    return times


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, tica
    from internal_hist_bench import peptide
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--lag", type=int, default=100)
    ap.add_argument("--structures", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=5000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("tica_bench: no GPU; a time per call cannot be measured here", file=sys.stderr)
        return 1
    z, bonds = peptide("AAAAAAAGAAAAAAAG")
    z, bonds = np.array(z), np.array(bonds)
    n = len(z)
    sel = tica.backbone_atoms(z, bonds)[:30]                # N, CA, C of the first 10 residues
    pairs = tica.distance_pairs(sel, 2)
    d, T, lag, S = len(pairs), args.frames, args.lag, args.structures
    rng = np.random.default_rng(0)
    x0 = np.cumsum(rng.standard_normal((n, 3)) * 0.9, axis=0)
    xyz_h = (x0[None] + 0.1 * rng.standard_normal((T, n, 3))).astype(np.float32)
    xyz = torch.from_numpy(xyz_h).cuda()
    ptab = torch.from_numpy(pairs).cuda()
    totals = {k: torch.zeros((d,) if k.startswith("sum") else (d, d), dtype=torch.float64, device="cuda") for k in tica.MOMENT_KEYS}
    lib = _lib.load()
    splits = int(lib.cgv_tica_moments_splits(T, d, lag))
    ws = torch.empty(int(lib.cgv_tica_moments_workspace_bytes(T, d, lag)) // 8 + 1, dtype=torch.float64, device="cuda")

    def zero():
        for t in totals.values():
            t.zero_()
    for _ in range(3):
        tica.moments_launch(xyz, ptab, lag, totals, ws)
    torch.cuda.synchronize()
    times = windows(lambda: tica.moments_launch(xyz, ptab, lag, totals, ws), zero, args.launches, args.repeats)
    med, N = statistics.median(times), T - lag
    print(f"tica_moments  n {n}  sel {len(sel)}  d {d}  T {T}  lag {lag}  ranges {splits}  workspace {ws.numel() * 8 / 1e6:.1f} MB  |  "
          f"median {med:.1f} us/call (min {min(times):.1f}, max {max(times):.1f}, {args.repeats} windows of {args.launches})  |  "
          f"6 N d^2 = {6 * N * d * d / 1e9:.2f} Gflop: {6 * N * d * d / med / 1e6:.2f} Tflop/s fp64 (4 N d^2 issued: "
          f"{4 * N * d * d / med / 1e6:.2f} Tflop/s)", flush=True)
    # the projection
    model = tica.fit_from_moments({k: v.cpu().numpy() / args.launches for k, v in totals.items()} | {"n_frame_pairs": N}, lag, pairs=pairs)
    mean, W = torch.from_numpy(model.mean).cuda(), torch.from_numpy(model.W).cuda()
    k = int(W.shape[1])
    ics = torch.zeros(S, k, dtype=torch.float64, device="cuda")
    counts, outside = torch.zeros(50, 50, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    hist = (0, k - 1, 50, (-5.0, 5.0), (-5.0, 5.0), counts, outside)
    xs = xyz[:S].contiguous()
    for _ in range(3):
        tica.project_launch(xs, ptab, mean, W, ics, hist)
    torch.cuda.synchronize()
    times = windows(lambda: tica.project_launch(xs, ptab, mean, W, ics, hist), lambda: (counts.zero_(), outside.zero_()),
                    max(args.launches, 100), args.repeats)
    med = statistics.median(times)
    print(f"tica_project  S {xs.shape[0]}  d {d}  k {k}  bins 50 x 50  |  median {med:.1f} us/call (min {min(times):.1f}, "
          f"max {max(times):.1f})  |  {xs.shape[0] * d / med / 1e3:.2f} G features/s", flush=True)
    # the numpy restatement's moments on the CPU, for scale
    import tica_restatement as R
    Tc = min(args.cpu_frames, T)
    t0 = time.perf_counter()
    R.moments(xyz_h[:Tc], pairs, lag, "einsum")
    sec = time.perf_counter() - t0
    try:
        import threadpoolctl
        threads = max(p["num_threads"] for p in threadpoolctl.threadpool_info())
    except Exception:
        threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
    print(f"numpy restatement (einsum)  T {Tc}  d {d}  |  {sec * 1e3:.1f} ms on the CPU ({threads if threads else 'unknown'} threads; "
          f"einsum itself is one thread)  =  {sec / (Tc - lag) * 1e6:.2f} us per frame pair, {sec / (Tc - lag) * N * 1e3:.0f} ms "
          f"scaled to T {T}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
