#!/usr/bin/env python3
"""``run_baseline.py`` command-line surface of the reference (scripts/run_baseline.py:412-434): k-fold training and test
of the baseline models -- ``-model linear`` (linear backmap), ``equilinear`` (equivariant linear), ``mlp`` -- that the
paper's tables compare the CGVAE with.  Every flag keeps its name, type and default; ``-cutoff``, ``-kappa`` and ``--cross``
are parsed and unused, as in the reference (no neighbour list is built: no model reads one).  ``equimlp`` (``edgesetMLP``)
is not built and is refused.  Added flags: ``-traj file.npz`` (tools/traj_to_npz.py), ``--synthetic`` and ``-seed``.

    python -m coarsegrainingvae_amd.run_baseline -logdir out -device 0 -model equilinear -dataset dipeptide -N_cg 3 \
        -ndata 2000 -n_epochs 50 -n_splits 3 --synthetic

Per fold (run_baseline.py:243-392): the atom -> bead map from ``cgmap`` (``-cg_method newman | cgae | backbonepartition |
random``, or the file's own), one seeded random rotation per frame (get_diffpool_data(rotate=True)), Adam with
ReduceLROnPlateau(patience=10, factor=0.6, threshold=1e-4, min_lr=1e-7) on the validation ``loss_recon``, stop at
lr <= 1.5e-7; ``fold<i>/train_log.csv`` (the reference's columns), ``fold<i>/model.pt``; on the fold's test frames the
unaligned all-atom / heavy-atom RMSD (359-367) and, through the sample-quality kernel of ``evaluate`` (K12), the graph
differences and valid ratios (retrieve_recon_structures, 40-84).  ``cv_stats.csv`` has one row per fold with the reference's
columns; absent values (``train_tetra`` / ``test_tetra``: the tetrahedral term is parsed and never computed there either)
are empty cells.  A ``-traj`` file with elements that have no tabulated covalent radius gets the RMSD columns only, with a
message on stderr.  One JSON line on stdout carries the fold means and standard deviations.

Deliberately different: the folds.  They are contiguous k-fold blocks of the frames, as ``KFold(n_splits)`` gives without
shuffling, and a seeded 10 % OF THE FOLD'S OWN TRAINING INDICES serves for validation.  The reference draws
``train_test_split`` over ``range(len(train_index))`` -- over positions, not over the training indices -- which lets test
frames into training (run_baseline.py:248-252).  That is not reproduced.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import baseline, cgmap
from . import data as cgdata
from .run_ala import DATASET_SHAPES

MODELS = ("linear", "equilinear", "mlp")
TRAIN_LOG_COLUMNS = ["epoch", "lr", "train_recon", "val_recon", "train_graph", "val_graph"]
CV_STATS_COLUMNS = ["train_recon", "test_all_recon", "test_heavy_recon", "train_graph", "test_graph", "train_tetra", "test_tetra",
                    "all atom ged", "heavy atom ged", "all atom graph valid ratio", "heavy atom graph valid ratio"]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument("-logdir", type=str)
    p.add_argument("-model", type=str, default="equilinear")
    p.add_argument("-dataset", type=str, default="dipeptide")
    p.add_argument("-device", type=int)
    p.add_argument("-cutoff", type=float, default=2.5)
    p.add_argument("-batch_size", type=int, default=32)
    p.add_argument("-N_cg", type=int, default=3)
    p.add_argument("-width", type=int, default=1)
    p.add_argument("-depth", type=int, default=1)
    p.add_argument("-edgeorder", type=int, default=2)
    p.add_argument("-n_splits", type=int, default=3)
    p.add_argument("-n_epochs", type=int, default=50)
    p.add_argument("-ndata", type=int, default=2000)
    p.add_argument("-knbr", type=int, default=0)
    p.add_argument("-cg_method", type=str, default="newman")
    p.add_argument("-activation", type=str, default="ReLU")
    p.add_argument("-mapshuffle", type=float, default=0.0)
    p.add_argument("-lr", type=float, default=1e-3)
    p.add_argument("-gamma", type=float, default=0.0)
    p.add_argument("-kappa", type=float, default=0.0)
    p.add_argument("--tqdm_flag", action="store_true", default=False)
    p.add_argument("--cross", action="store_true", default=False)
    p.add_argument("-traj", type=str, default=None,
                   help="trajectory file from tools/traj_to_npz.py (xyz [T,n,3], z [n], bonds [Eb,2], optional mapping [n])")
    p.add_argument("--synthetic", action="store_true", default=False,
                   help="random-coordinate frames of the dataset's shape (no trajectories offline)")
    p.add_argument("-seed", type=int, default=123)
    return p


def kfold_indices(n_frames: int, n_splits: int):
    """[(train, test)] as ``sklearn.model_selection.KFold(n_splits)`` gives without shuffling: contiguous test blocks, the
    first ``n_frames % n_splits`` of them one frame longer."""
    n_frames, n_splits = int(n_frames), int(n_splits)
    if not 2 <= n_splits <= n_frames:
        raise ValueError(f"n_splits = {n_splits} for {n_frames} frames (need 2 <= n_splits <= frames)")
    sizes = np.full(n_splits, n_frames // n_splits, dtype=np.int64)
    sizes[: n_frames % n_splits] += 1
    idx, out, start = np.arange(n_frames), [], 0
    for size in sizes:
        out.append((np.concatenate([idx[:start], idx[start + size:]]), idx[start:start + size]))
        start += size
    return out


def fold_split(n_frames: int, n_splits: int, seed: int):
    """[(train, val, test)] index arrays: ``kfold_indices``, then a seeded ceil(10 %) of the fold's OWN training indices
    for validation (train_test_split(test_size=0.1) sizes).  No test frame is in train or val."""
    out = []
    for fold, (train, test) in enumerate(kfold_indices(n_frames, n_splits)):
        perm = np.random.default_rng([int(seed), 6, fold]).permutation(train)
        n_val = math.ceil(0.1 * len(train))
        out.append((np.sort(perm[n_val:]), np.sort(perm[:n_val]), test))
    return out


def load_frames(params, device):
    """(xyz float32 [T,n,3] rotated, z int64 [n], bonds [Eb,2], mapping int64 [n], mapping info or None)."""
    seed = int(params["seed"])
    if params.get("traj"):
        with np.load(params["traj"]) as f:
            need = {"xyz", "z", "bonds"}
            if not need.issubset(f.files):
                raise SystemExit(f"{params['traj']}: missing {sorted(need - set(f.files))} (see tools/traj_to_npz.py)")
            xyz, z, bonds = np.asarray(f["xyz"], dtype=np.float32), np.asarray(f["z"]).astype(np.int64), np.asarray(f["bonds"])
            file_mapping = f["mapping"] if "mapping" in f.files else None
    elif params["synthetic"]:
        if params["dataset"] not in DATASET_SHAPES:
            raise SystemExit(f"unknown -dataset {params['dataset']}; known shapes: {sorted(DATASET_SHAPES)}")
        n = DATASET_SHAPES[params["dataset"]]
        box = {"dipeptide": 6.0, "chignolin": 14.0, "pentapeptide": 11.0}[params["dataset"]]
        props = cgdata.synthetic_frames(params["ndata"], n, params["N_cg"], box, seed=0)
        xyz = torch.stack([t[:, 1:] for t in props["nxyz"]]).numpy()
        z = props["nxyz"][0][:, 0].numpy().astype(np.int64)                 # one molecule: the first frame's labels for all
        bonds, file_mapping = props["bond_edge_list"][0].numpy(), None
    else:
        raise SystemExit("pass -traj file.npz (a trajectory converted by tools/traj_to_npz.py) or --synthetic: the "
                         "reference's mdtraj ingestion is outside the hot path")
    xyz = xyz[: params["ndata"]]                                             # the map is chosen on the frames that are used
    mapping, info = cgmap.select_mapping(params["cg_method"], file_mapping, xyz, params["N_cg"], 0.25, device, z=z, bonds=bonds,
                                         mapshuffle=params["mapshuffle"], seed=seed)
    R = cgdata.random_rotation_matrices(xyz.shape[0], torch.Generator().manual_seed(seed))
    xyz = torch.bmm(torch.from_numpy(xyz), R.transpose(1, 2)).numpy()          # row vectors: x' = R x
    return xyz, z, bonds, np.asarray(mapping).astype(np.int64), info


def build_model(params, pooler, n_cgs, n_atoms):
    name = params["model"]
    if name == "equimlp":
        raise SystemExit("-model equimlp (edgesetMLP) is not built here; choose one of " + ", ".join(MODELS))
    if name not in MODELS:
        raise SystemExit(f"unknown -model {name}; choose one of " + ", ".join(MODELS))
    if name == "linear":
        return baseline.Baseline(pooler, n_cgs, n_atoms)
    if name == "equilinear":
        knn = params["knbr"] if params["knbr"] else n_cgs - 1                # run_baseline.py:199-200
        return baseline.EquiLinear(pooler, n_cgs, n_atoms, cross=params["cross"], knn=knn)
    return baseline.MLP(pooler, n_cgs, n_atoms, width=params["width"], depth=params["depth"], activation=params["activation"])


def _write_csv(path, columns, rows):
    with open(path, "w") as f:
        f.write(",".join(columns) + "\n")
        for r in rows:
            f.write(",".join("" if r.get(c) is None else str(r[c]) for c in columns) + "\n")


def _order(indices, epochs, rng):
    """int32 [epochs, len(indices)]: the indices in a fresh random order per epoch (DataLoader(shuffle=True))."""
    return rng.permuted(np.tile(np.asarray(indices, dtype=np.int32), (epochs, 1)), axis=1)


def reconstruct(model, frames, indices, batch_size):
    """(data [T',n,3], recon [T',n,3]) device tensors of the frames ``indices``, as the model's forward returns them."""
    data, recon = [], []
    with torch.no_grad():
        for s in range(0, len(indices), batch_size):
            xyz, out = model(frames[torch.as_tensor(indices[s:s + batch_size], device=frames.device)])
            data.append(xyz), recon.append(out)
    return torch.cat(data), torch.cat(recon)


def graph_quality(data, recon, z, radii):
    """(all_valid_ratio, heavy_valid_ratio, all_ged, heavy_ged) over the frames, one launch of the sample-quality kernel
    (retrieve_recon_structures: the one-sample evaluation ``reconstruction vs frame``, means over frames)."""
    from . import evaluate as ev
    T, n = int(data.shape[0]), int(data.shape[1])
    plan = ev.QualityPlan(np.tile(z, T), np.arange(T + 1) * n, data.device, radii=radii)
    raw = ev.sample_quality(data.reshape(T * n, 3), recon.reshape(T * n, 3), n_samples=1, plan=plan)
    counts, sums = ev.read_back([raw.counts, raw.sums])
    per_frame = [ev.assemble_sample_qualities(counts[f], sums[f], n, int(plan.n_heavy[f])) for f in range(T)]
    return tuple(float(v) for v in ev.assemble_reconstruction(per_frame))


def run(params) -> dict:
    from . import evaluate as ev
    if params["model"] not in MODELS:
        build_model(params, None, 0, 0)                                      # the refusals, before any work
    device = torch.device("cuda", int(params["device"] or 0))
    torch.cuda.set_device(device)
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    seed = int(params["seed"])
    xyz, z, bonds, mapping, map_info = load_frames(params, device)
    T, n = xyz.shape[0], xyz.shape[1]
    n_cgs = int(mapping.max()) + 1
    if params["N_cg"] and params["N_cg"] != n_cgs:
        raise SystemExit(f"-N_cg {params['N_cg']} but the mapping has {n_cgs} beads")
    edges = cgdata.get_high_order_edge(torch.as_tensor(bonds).long(), params["edgeorder"], n).numpy()
    frames = torch.from_numpy(xyz).to(device)
    present = sorted(set(z.tolist()))
    radii, graph_metrics = None, True
    if params["synthetic"] and not params.get("traj"):
        radii = {e: ev.COVALENT_RADII[6] for e in present if e not in ev.COVALENT_RADII}     # random labels, not chemistry
    else:
        try:
            ev.bond_radii(present)
        except KeyError as err:
            print(f"graph metrics skipped: {err.args[0]}", file=sys.stderr, flush=True)
            graph_metrics = False
    logdir = params["logdir"]
    if logdir:
        os.makedirs(logdir, exist_ok=True)
    bs, n_epochs, gamma = int(params["batch_size"]), int(params["n_epochs"]), float(params["gamma"])
    cv_rows, failed = [], False
    for fold, (train_idx, val_idx, test_idx) in enumerate(fold_split(T, params["n_splits"], seed)):
        split_dir = os.path.join(logdir, f"fold{fold}") if logdir else None
        if split_dir:
            os.makedirs(split_dir, exist_ok=True)
        torch.manual_seed(seed + fold)
        model = build_model(params, baseline.FixedPool(mapping, n_cgs), n_cgs, n).to(device)
        rng = np.random.default_rng([seed, 7, fold])
        train_order, val_order = _order(train_idx, max(n_epochs, 1), rng), _order(val_idx, 1, rng)
        spe = -(-len(train_idx) // bs)
        # the schedule of run_baseline.py:305-307 on a stand-in optimiser: only its learning rate is read
        knob = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=params["lr"])
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(knob, patience=10, factor=0.6, threshold=1e-4, min_lr=1e-7)
        log_rows, train_means = [], (float("nan"), float("nan"))
        for epoch in range(n_epochs):
            lr = knob.param_groups[0]["lr"]
            tr = baseline.fit(model, frames, train_order, bs, lr, gamma, edges=edges, first_step=epoch * spe, steps=spe)
            va = baseline.fit(model, frames, val_order, bs, lr, gamma, edges=edges, train=False)
            means = torch.cat([tr.mean(0), va.mean(0)]).tolist()              # one read per epoch
            train_means = (means[0], means[1])
            if np.isnan(means[0]):                                            # run_baseline.py:326-329
                print("NaN encountered, exiting...", file=sys.stderr, flush=True)
                failed = True
                break
            sched.step(means[2])
            if knob.param_groups[0]["lr"] <= 1.5e-7:                          # run_baseline.py:337-338
                break
            log_rows.append({"epoch": epoch, "lr": knob.param_groups[0]["lr"], "train_recon": means[0], "val_recon": means[2],
                             "train_graph": means[1], "val_graph": means[3]})
            if split_dir:
                _write_csv(os.path.join(split_dir, "train_log.csv"), TRAIN_LOG_COLUMNS, log_rows)
        if split_dir:
            if not log_rows:
                _write_csv(os.path.join(split_dir, "train_log.csv"), TRAIN_LOG_COLUMNS, log_rows)
            torch.save(model.state_dict(), os.path.join(split_dir, "model.pt"))
        test_log = baseline.fit(model, frames, _order(test_idx, 1, rng), bs, 0.0, gamma, edges=edges, train=False)
        data, recon = reconstruct(model, frames, test_idx, bs)
        d2 = (data - recon).pow(2).sum(-1)                                    # run_baseline.py:359-367
        heavy = torch.from_numpy(z != 1).to(device)
        row = {c: None for c in CV_STATS_COLUMNS}
        row.update({"train_recon": train_means[0], "train_graph": train_means[1], "test_graph": float(test_log[:, 1].mean()),
                    "test_all_recon": float(d2.mean().sqrt()),
                    "test_heavy_recon": float(d2[:, heavy].mean().sqrt()) if bool(heavy.any()) else float("nan")})
        if graph_metrics:
            all_valid, heavy_valid, all_ged, heavy_ged = graph_quality(data.contiguous(), recon.contiguous(), z, radii)
            row.update({"all atom ged": all_ged, "heavy atom ged": heavy_ged, "all atom graph valid ratio": all_valid,
                        "heavy atom graph valid ratio": heavy_valid})
        cv_rows.append(row)
        if logdir:
            _write_csv(os.path.join(logdir, "cv_stats.csv"), CV_STATS_COLUMNS, cv_rows)
        if failed:
            break

    def mean_std(col):
        vals = np.array([r[col] for r in cv_rows if r[col] is not None], dtype=np.float64)
        return {"mean": float(np.nanmean(vals)), "std": float(np.nanstd(vals))} if vals.size and not np.isnan(vals).all() else None
    summary = {"model": params["model"], "n_cgs": n_cgs, "n_atoms": int(n), "frames": int(T), "folds": len(cv_rows), "failed": failed,
               "all_rmsd": mean_std("test_all_recon"), "heavy_rmsd": mean_std("test_heavy_recon"),
               "all_ged": mean_std("all atom ged"), "heavy_ged": mean_std("heavy atom ged"),
               "all_valid_ratio": mean_std("all atom graph valid ratio"),
               "heavy_valid_ratio": mean_std("heavy atom graph valid ratio")}
    if map_info:
        summary["cg_mapping"] = {k: map_info[k] for k in ("method", "seconds", "attempts", "removals", "form", "seed") if k in map_info}
    return summary


def main(argv=None):
    params = vars(build_parser().parse_args(argv))
    print(json.dumps(run(params)))


if __name__ == "__main__":
    main(sys.argv[1:])
