#!/usr/bin/env python3
"""Time ``backmap.backmap`` on one GPU, on the shapes of ``profiles/eval_ensemble.txt``.

    python tools/backmap_bench.py [--out profiles/backmap.txt] [--only-check]

Per shape, wall clock between two device synchronisations (every path ends in a host read-back), median of ``--reps``
after one warm-up:
  backmap   ``backmap(model, beads, mapping, K, z=, bonds=, frames_per_launch=frames)``: bead graph, prior, decoder, K14,
            read-back
  (a)       ``evaluate.sample_ensemble(frames, model, K, graph_eval=True)`` on the same frames: it also needs the all-atom
            frames, runs ``model(batch)`` and K12
  (b)       the two metrics restated in torch with dense tensors on the same GPU on backmap's output (one ``[n,n]``
            distance matrix per sample, the topology as a dense matrix, one ``[K,K,n]`` tensor per frame), read back
  check     the K14 launch + read-back alone, on the same output
``--only-check`` runs nothing but K14 launches (for a ``rocprofv3 --kernel-trace --stats`` run of the kernel alone)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import coarsegrainingvae_amd as cg                                    # noqa: E402
from coarsegrainingvae_amd import backmap as bm, evaluate as ev       # noqa: E402

DEV = "cuda"
FILL = {2: 0.68, 3: 0.68, 4: 0.68, 5: 0.68}
CASES = [("dipeptide", 64, 32, 16), ("chignolin", 600, 8, 8), ("protein2000", 600, 1, 4)]


def dense_metrics(xyz, z, bonds):
    """xyz [T,K,n,3] device tensor -> counts [T,K,4], pair sums [T,K,K,2] on the host."""
    zs = np.asarray(z).astype(np.int64)
    elements = sorted(set(zs.tolist()))
    cls = torch.from_numpy(np.searchsorted(elements, zs)).to(DEV)
    cut = ev.bond_thresholds(elements, 1.3, FILL).to(DEV)[cls[:, None], cls[None, :]]
    heavy = torch.from_numpy(zs != 1).to(DEV)
    hh = heavy[:, None] & heavy[None, :]
    n = xyz.shape[2]
    topo = torch.zeros(n, n, dtype=torch.bool, device=DEV)
    b = torch.as_tensor(np.asarray(bonds)).to(DEV)
    topo[b[:, 0], b[:, 1]] = True
    topo = topo | topo.t()
    counts, sums = [], []
    for t in range(xyz.shape[0]):
        row = []
        for k in range(xyz.shape[1]):
            d = xyz[t, k][:, None, :] - xyz[t, k][None, :, :]
            got = d.pow(2).sum(-1) <= cut
            got.fill_diagonal_(False)
            miss, extra = topo & ~got, got & ~topo
            row.append(torch.stack([miss.sum(), extra.sum(), (miss & hh).sum(), (extra & hh).sum()]) // 2)
        counts.append(torch.stack(row))
        d2 = (xyz[t].double()[:, None] - xyz[t].double()[None, :]).pow(2).sum(-1)
        sums.append(torch.stack([d2.sum(-1), d2[..., heavy].sum(-1)], dim=-1))
    return torch.stack(counts).cpu(), torch.stack(sums).cpu()


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
    ap.add_argument("--only-check", action="store_true")
    args = ap.parse_args()
    lines = ["workload frames x samples | backmap ms | (a) sample_ensemble graph_eval ms | (b) dense torch metrics ms | "
             "K14 launch + read-back ms | backmap us per sample | (a) us per sample"]
    for workload, F, n_frames, K in CASES:
        w = cg.data.WORKLOADS[workload]
        ds = cg.CGDataset(cg.data.synthetic_frames(n_frames, w["n_atoms"], w["n_cgs"], w["box"], seed=5,
                                                   spatial_sort=(workload == "protein2000")))
        ds.generate_neighbor_list(w["atom_cutoff"], w["cg_cutoff"], device=DEV, undirected=True)
        model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], w["enc_nconv"], w["dec_nconv"], w["n_cgs"], seed=123).to(DEV)
        beads = torch.stack(ds.props["CG_nxyz"])[:, :, 1:].numpy().copy()
        mapping = ds.props["CG_mapping"][0]
        z = ds.props["nxyz"][0][:, 0].numpy().astype(np.int64)
        bonds = ds.props["bond_edge_list"][0].numpy()
        run = lambda: bm.backmap(model, beads, mapping, K, w["cg_cutoff"], z=z, bonds=bonds, radii=FILL, frames_per_launch=n_frames)
        out = run()
        gen = torch.from_numpy(out["xyz"]).to(DEV)
        plan = ev.QualityPlan(np.tile(z, n_frames), np.arange(n_frames + 1) * len(z), DEV, radii=FILL)
        blist = ev.BondList(bonds, plan)
        check = lambda: ev.read_back(list(ev.ensemble_check(gen.reshape(-1, 3), K, plan, blist)))
        if args.only_check:
            for _ in range(20):
                check()
            continue
        got = check()
        want = dense_metrics(gen, z, bonds)
        assert np.array_equal(got[0], want[0].numpy()) and np.allclose(got[1], want[1].numpy(), rtol=1e-10, atol=0)
        t_bm, t_chk = timed(run, args.reps), timed(check, args.reps)
        t_a = timed(lambda: ev.sample_ensemble(ds, model, K, frames_per_launch=n_frames, radii=FILL), args.reps)
        t_b = timed(lambda: dense_metrics(gen, z, bonds), args.reps)
        per = 1e3 / (n_frames * K)
        lines.append(f"{workload} {n_frames} x {K} (F = {F}) | {t_bm:.2f} | {t_a:.2f} | {t_b:.2f} | {t_chk:.3f} | "
                     f"{t_bm * per:.1f} | {t_a * per:.1f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
