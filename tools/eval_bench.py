#!/usr/bin/env python3
"""Time ``evaluate.sample_ensemble`` against the reference's call pattern on the same GPU and model.

    python tools/eval_bench.py [--out profiles/eval_ensemble.txt]

Batched path: ``sample_ensemble(frames, model, K, frames_per_launch=len(frames))`` -- one prior call, one decoder call on the
replicated bead graph, one metric launch, one read-back.  Baseline (scripts/sampling.py:252-333 on the device): per frame
one ``prior_net`` call, K single-frame ``model.decoder`` calls, every sample copied to the host, ``model(batch)``, and the
metric restated in torch with dense [n,n] matrices on the device (four per sample, as the reference builds them).  Both
are wall-clock between two device synchronisations (the paths end in host read-backs), median of ``--reps`` after one
warm-up; C-ABI calls per run are counted at ``_lib.call``."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import coarsegrainingvae_amd as cg                                    # noqa: E402
from coarsegrainingvae_amd import _lib, evaluate as ev                # noqa: E402

DEV = "cuda"
FILL = {2: 0.68, 3: 0.68, 4: 0.68, 5: 0.68}
CASES = [("dipeptide", 64, 32, 16), ("chignolin", 600, 8, 8), ("protein2000", 600, 1, 4)]


def reference_pattern(ds, model, K):
    out = []
    with torch.no_grad():
        for f in range(len(ds)):
            batch = cg.batch_to(cg.CG_collate([ds[f]]), DEV)
            z, cg_z, xyz, cg_xyz, nbr_list, CG_nbr_list, mapping, num_CGs = model.get_inputs(batch)
            mu, sigma = model.prior_net(cg_z, cg_xyz, CG_nbr_list)
            zs = z.cpu().numpy().astype(np.int64)
            elements = sorted(set(zs.tolist()))
            thr = ev.bond_thresholds(elements, 1.3, FILL).to(DEV)
            cls = torch.from_numpy(np.searchsorted(elements, zs)).to(DEV)
            heavy = torch.from_numpy(zs != 1).to(DEV)
            cut, cut_h = thr[cls[:, None], cls[None, :]], None

            def bonds(p, c):
                d = p[:, None, :] - p[None, :, :]
                b = (d.pow(2).sum(-1) <= c).long()
                b.fill_diagonal_(0)
                return b
            cut_h = cut[heavy][:, heavy]
            for _ in range(K):
                H = torch.randn_like(sigma).mul(sigma).add_(mu)
                dec = model.decoder(cg_xyz, CG_nbr_list, H, H, mapping, num_CGs)
                host = dec.cpu()                                       # sampling.py:280
                stats = []
                for pr, pg, c in ((xyz, dec, cut), (xyz[heavy], dec[heavy], cut_h)):
                    stats.append((bonds(pr, c) != bonds(pg, c)).sum())             # compare_graph
                    g_gen, g_ref = bonds(pg, c), bonds(pr, c)                        # count_valid_graphs builds them again
                    stats.append((g_ref - g_gen).sum().abs() / g_ref.sum())
                out.append((host, [float(s) for s in torch.stack([s.float() for s in stats]).cpu()]))
            model(batch)[5].cpu()
    return out


def timed(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    calls = [0]
    inner = _lib.call

    def counting(*a, **k):
        calls[0] += 1
        return inner(*a, **k)
    lines = ["workload frames x samples | batched ms (C-ABI calls) | reference call pattern ms (C-ABI calls) | ratio"]
    for workload, F, n_frames, K in CASES:
        w = cg.data.WORKLOADS[workload]
        ds = cg.CGDataset(cg.data.synthetic_frames(n_frames, w["n_atoms"], w["n_cgs"], w["box"], seed=5,
                                                   spatial_sort=(workload == "protein2000")))
        ds.generate_neighbor_list(w["atom_cutoff"], w["cg_cutoff"], device=DEV, undirected=True)
        model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], w["enc_nconv"], w["dec_nconv"], w["n_cgs"], seed=123).to(DEV)
        batched = lambda: ev.sample_ensemble(ds, model, K, frames_per_launch=n_frames, radii=FILL)
        baseline = lambda: reference_pattern(ds, model, K)
        t_b, t_r = timed(batched, args.reps), timed(baseline, args.reps)
        counts = []
        _lib.call = counting
        try:
            for fn in (batched, baseline):
                calls[0] = 0
                fn()
                counts.append(calls[0])
        finally:
            _lib.call = inner
        lines.append(f"{workload} {n_frames} x {K} (F = {F}) | {t_b:.2f} ({counts[0]}) | {t_r:.2f} ({counts[1]}) | {t_r / t_b:.2f}x")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
