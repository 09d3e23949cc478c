#!/usr/bin/env python3
"""``run_ala.py`` command-line surface of the reference (scripts/run_ala.py:417-482) on the
MI355X hot path.  Every flag keeps its name, type and default.  What is in scope here is the
training loop of one fold: model wiring (run_ala.py:184-209), Adam + ReduceLROnPlateau +
early stopping (211-215, 232-284) and the CSV log columns (228-229, 252-258).

Out of scope: trajectory download / mdtraj loading, the ``minimal`` / ``alpha`` mappings
(they need atom names), k-fold cross-validation.  On a ``-traj`` file without a ``mapping``, ``-cg_method cgae`` learns the
atom -> bead map on the device first and ``-cg_method newman`` partitions the bond graph there (cgmap.py, datasets.py:190-249,
277-312, 373-385); ``backbonepartition``, ``seqpartition`` and ``random`` are seeded.  Frames come either from ``--synthetic`` (uniform random
coordinates of the dataset's shape) or from ``-traj file.npz`` -- a trajectory
converted offline by ``tools/traj_to_npz.py`` (xyz [T,n,3] in Angstrom, z [n], bonds, optional
atom -> bead ``mapping``), which goes through the on-device ``build_dataset`` (datasets.py:459-506:
random rotation per frame, bead coordinates = scatter_mean, higher-order bond edges, batched
radius graphs).  Added flags: ``--synthetic``, ``-traj``, ``--no_hip_graph``; ``-device`` also
accepts ``cuda:N`` strings besides the reference's int.

    python -m coarsegrainingvae_amd.run_ala -logdir out -device 0 -dataset chignolin -n_cgs 6 \
        -batch_size 2 -ndata 64 -nepochs 3 -atom_cutoff 12.0 -cg_cutoff 25.0 -beta 0.05 -gamma 50.0 \
        -dec_nconv 9 -enc_nconv 2 -lr 0.0001 -n_basis 600 -n_rbf 10 --synthetic
Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1``;
each rank trains on its shard of every batch (frames are independent graphs).

After training (run_ala.py:286-408), on rank 0 and when the run did not fail, the test-time evaluation of
``evaluate.py``: reconstruction quality of the first ``-nevals`` training batches (a flag the reference parses and
never reads; here it caps the training frames evaluated, default 36 batches) and of the hold-out frames, the unaligned
all-atom / heavy-atom RMSD, and ``-n_ensemble`` samples per hold-out frame from the prior (``--graph_eval``: with the
bond-graph metrics; ``--reflectiontest``: on mirrored hold-out frames).  This driver trains ONE fold, so the hold-out
frames are its validation indices -- there is no separate k-fold test split -- and ``test_KL`` / ``test_graph`` are the
last epoch's validation terms.  Written to the log directory: ``cv_stats.csv`` (one row, the reference's columns,
absent values as empty cells; a ``-traj`` file with elements that have no tabulated covalent radius gets no
evaluation, with a message on stderr), ``test_all_rmsd*.txt`` / ``test_heavy_rmsd*.txt`` and ``samples.npz`` (sample, data,
bead and reconstruction coordinates; the reference's xyz movies need ase and are out of scope).  The JSON summary
carries the same numbers under ``"test_stats"``, with or without ``-logdir``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from datetime import date

import numpy as np
import torch

from . import cgmap, contacts, coverage, density, distributions, flexibility, tica
from . import data as cgdata
from .analyses import ANALYSES, BY_STEM
from .train import build_model, optim_dict
from .trainer import Trainer

# what the JSON summary's "cg_mapping" block shows of a mapping method's info: the learner's six keys, and for the
# partition methods whichever of theirs the info carries
CG_MAPPING_KEYS = {"cgae": ("method", "steps", "seconds", "attempts", "loss_recon", "loss_reg")}
CG_PARTITION_KEYS = ("method", "seconds", "removals", "launches", "form", "mapshuffle", "n_backbone", "seed")
DATASET_SHAPES = {"dipeptide": 22, "chignolin": 166, "pentapeptide": 94}   # atoms per frame


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(epilog="after the evaluation: --dist_eval compares the internal-coordinate distributions of the "
                                "hold-out frames with their prior samples and writes dist_stats.json (build_extras_parser)")
    p.add_argument("-logdir", type=str)
    p.add_argument("-device", type=str, default="0")        # reference: int CUDA ordinal (run_ala.py:421)
    p.add_argument("-n_cgs", type=int)
    p.add_argument("-lr", type=float, default=2e-4)
    p.add_argument("-dataset", type=str, default="dipeptide")
    p.add_argument("-n_basis", type=int, default=512)
    p.add_argument("-n_rbf", type=int, default=10)
    p.add_argument("-activation", type=str, default="swish")
    p.add_argument("-cg_method", type=str, default="minimal")
    p.add_argument("-atom_cutoff", type=float, default=4.0)
    p.add_argument("-optimizer", type=str, default="adam")
    p.add_argument("-cg_cutoff", type=float, default=4.0)
    p.add_argument("-enc_nconv", type=int, default=4)
    p.add_argument("-dec_nconv", type=int, default=4)
    p.add_argument("-batch_size", type=int, default=64)
    p.add_argument("-nepochs", type=int, default=2)
    p.add_argument("-ndata", type=int, default=200)
    p.add_argument("-nsamples", type=int, default=200)
    p.add_argument("-n_ensemble", type=int, default=16)
    p.add_argument("-nevals", type=int, default=36)
    p.add_argument("-edgeorder", type=int, default=2)
    p.add_argument("-auxcutoff", type=float, default=0.0)
    p.add_argument("-beta", type=float, default=0.001)
    p.add_argument("-gamma", type=float, default=0.01)
    p.add_argument("-eta", type=float, default=0.01)
    p.add_argument("-kappa", type=float, default=0.01)
    p.add_argument("-threshold", type=float, default=1e-3)
    p.add_argument("-nsplits", type=int, default=5)
    p.add_argument("-patience", type=int, default=5)
    p.add_argument("-factor", type=float, default=0.6)
    p.add_argument("-mapshuffle", type=float, default=0.0)
    p.add_argument("-cgae_reg_weight", type=float, default=0.25)
    p.add_argument("--dec_type", type=str, default="EquivariantDecoder")
    for flag in ("cross", "graph_eval", "shuffle", "cg_mp", "tqdm_flag", "det", "cg_radius_graph", "invariantdec",
                 "reflectiontest"):
        p.add_argument("--" + flag, action="store_true", default=False)
    p.add_argument("--no_hip_graph", action="store_true", default=False,
                   help="launch every kernel of every step eagerly instead of replaying one captured hipGraph per step")
    p.add_argument("--synthetic", action="store_true", default=False,
                   help="random-coordinate frames of the dataset's shape (no trajectories offline)")
    p.add_argument("-traj", type=str, default=None,
                   help="trajectory file from tools/traj_to_npz.py (xyz [T,n,3], z [n], bonds [Eb,2], optional mapping [n])")
    return p


def build_extras_parser() -> argparse.ArgumentParser:
    """Switches of analyses that run after the reference's evaluation.  They are kept apart from ``build_parser`` -- the
    reference's flag surface plus this build's run switches, which ``modelparams.json`` records -- and are parsed first
    by ``main``; what they do not know goes on to ``build_parser``."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--dist_eval", action="store_true", default=False,
                   help="after the evaluation, compare the internal-coordinate distributions of the hold-out frames with "
                        "their prior samples (distributions.compare): dist_stats.json in the log directory")
    p.add_argument("--tica_eval", action="store_true", default=False,
                   help="after the evaluation, fit TICA on the -traj file's frames in file order and compare the hold-out "
                        "samples with them in the plane of its two slowest components (tica.compare): tica_stats.json")
    p.add_argument("-tica_lag", type=int, default=100, help="lag of --tica_eval in frames of the file")
    p.add_argument("--cov_eval", action="store_true", default=False,
                   help="after the evaluation, coverage and precision of the hold-out frames' prior samples against those "
                        "frames by superposed heavy-atom RMSD (coverage.compare): cov_stats.json in the log directory")
    # absent from the parsed arguments unless given: without it they are what they were before the switch existed
    p.add_argument("--contact_eval", action="store_true", default=argparse.SUPPRESS,
                   help="after the evaluation, heavy-atom contact maps, native contacts and Rg of the hold-out frames' prior "
                        "samples against those frames (contacts.compare): contact_stats.json in the log directory")
    p.add_argument("--flex_eval", action="store_true", default=argparse.SUPPRESS,
                   help="after the evaluation, mean structure and per-atom fluctuation (RMSF) of the hold-out frames' prior "
                        "samples against those frames (flexibility.compare): flex_stats.json in the log directory")
    p.add_argument("--kde_eval", action="store_true", default=argparse.SUPPRESS,
                   help="after the evaluation, kernel density estimates of the hold-out frames and their prior samples in every "
                        "(phi, psi) plane (density.compare_torsions): kde_stats.json in the log directory")
    return p


def stored_params(params: dict) -> dict:
    """What ``modelparams.json`` records of the parameters: a switch of ``build_extras_parser`` that is off leaves the
    file as it was before the switch existed (its key, and the keys of its options, are left out)."""
    off = [k for a in ANALYSES if not params.get(a.stem + "_eval") for k in (a.stem + "_eval",) + a.options]
    return {k: v for k, v in params.items() if k not in off}


def annotate_job(task, job_name, n_cg):
    """scripts/utils.py:22-24."""
    return "{}_{}_{}_N{}".format(job_name, date.today().strftime("%m-%d"), task, n_cg)


def resolve_logdir(params):
    """Log-directory naming of run_ala.py:466-481."""
    task = "recon" if params["det"] else "sample"
    stem = params["cg_method"] + ("_invariantdec_" if params["invariantdec"] else "_") + task + \
        "_ndata{}".format(params["ndata"])
    name = annotate_job(stem, params["logdir"], params["n_cgs"])
    if params["cross"]:
        name += "_cross"
    if params["reflectiontest"]:
        name += "_reflectiontest"
    return name


class EarlyStopping:
    """scripts/utils.py:54-79."""

    def __init__(self, patience=5, min_delta=0):
        self.patience, self.min_delta, self.counter, self.best_loss, self.early_stop = patience, min_delta, 0, None, False

    def __call__(self, val_loss):
        if self.best_loss is None:
            self.best_loss = val_loss
        elif self.best_loss - val_loss > self.min_delta:
            self.best_loss, self.counter = val_loss, 0
        elif self.best_loss - val_loss < self.min_delta:
            self.counter += 1
            if self.counter >= self.patience:
                self.early_stop = True


def load_trajectory_dataset(params, device):
    """The non-synthetic branch of run_ala.py:124-181 for a file written by tools/traj_to_npz.py: frames (Angstrom),
    atomic numbers and the bond graph come from the file; the atom -> bead map is the file's ``mapping`` or, without
    one, what ``-cg_method`` says (cgmap.select_mapping): the map learned from the file's frames for ``cgae`` (under data
    parallel every rank learns the same map from the same seed), the Girvan-Newman partition of the file's bond graph for
    ``newman`` (with ``-mapshuffle``), the seeded ``backbonepartition`` / ``seqpartition`` / ``random``, and contiguous equal
    blocks of atoms for every other name (``minimal`` / ``alpha`` need atom names, which the file does not carry); then
    ``build_dataset`` on the device (datasets.py:459-506).  Returns (dataset, mapping, learner's info or None)."""
    with np.load(params["traj"]) as f:
        need = {"xyz", "z", "bonds"}
        if not need.issubset(f.files):
            raise SystemExit(f"{params['traj']}: missing {sorted(need - set(f.files))} (see tools/traj_to_npz.py)")
        xyz, z, bonds = f["xyz"], f["z"], f["bonds"]
        mapping = f["mapping"] if "mapping" in f.files else None
    # the learner sees the whole file (learn_map takes the trajectory, not the -ndata cut: datasets.py:190-197)
    mapping, map_info = cgmap.select_mapping(params["cg_method"], mapping, xyz, params["n_cgs"], params["cgae_reg_weight"], device,
                                             z=z, bonds=bonds, mapshuffle=params.get("mapshuffle", 0.0), seed=123)
    xyz = xyz[: params["ndata"]]
    n_cgs = int(mapping.max()) + 1
    if params["n_cgs"] and params["n_cgs"] != n_cgs:
        raise SystemExit(f"-n_cgs {params['n_cgs']} but the file's mapping has {n_cgs} beads")
    params["n_cgs"] = n_cgs
    gen = torch.Generator().manual_seed(123)
    dataset = cgdata.build_dataset(mapping, xyz, params["atom_cutoff"], params["cg_cutoff"], z, bonds,
                                   order=params["edgeorder"], rotate=True, generator=gen, device=device)
    return dataset, torch.as_tensor(mapping).long(), map_info


def _device(arg: str) -> torch.device:
    local = os.environ.get("LOCAL_RANK")
    if local is not None:
        return torch.device("cuda", int(local))
    return torch.device("cuda", int(arg)) if arg.isdigit() else torch.device(arg)


def _batches(dataset, indices, batch_size, rank, world, device, prepared=None):
    """Collate `batch_size` frames per step and give this rank its equal-size shard.  ``prepared()`` says whether
    a captured step exists: then the collated batch is handed over as is (the trainer loads it into the captured
    batch's buffers and replays); otherwise it gets its own graph bundle, with spare edge capacity so that it
    can become the captured batch."""
    if 0 < len(indices) < batch_size:                     # small validation split: one (world-divisible) batch
        indices, batch_size = indices[:len(indices) // world * world], len(indices) // world * world
    if not indices or batch_size <= 0:                    # fewer frames than ranks (or none): nothing to run
        return
    for start in range(0, len(indices) - batch_size + 1, max(batch_size, 1)):
        chunk = indices[start:start + batch_size]
        shard = chunk[rank::world] if world > 1 else chunk
        collated = cgdata.CG_collate([dataset[i] for i in shard])
        if prepared is not None and prepared():
            yield collated                                 # host tensors: checked on the host, copied in by the trainer
        else:
            yield cgdata.prepare_batch(collated, device, edge_slack=0.25 if prepared is not None else 0.0)


def write_cv_stats(path, stats):
    """cv_stats.csv (run_ala.py:404-405): one header line, one row; ``None`` is an empty cell."""
    from .evaluate import CV_STATS_COLUMNS
    with open(path, "w") as f:
        f.write(",".join(CV_STATS_COLUMNS) + "\n")
        f.write(",".join("" if stats.get(c) is None else str(stats[c]) for c in CV_STATS_COLUMNS) + "\n")


def evaluate_run(params, model, dataset, train_idx, val_idx, device, last_epoch, logdir):
    """run_ala.py:286-408 for one fold: reconstruction quality (train, capped by ``-nevals`` batches, and hold-out),
    unaligned RMSDs, ensemble sampling of the hold-out frames.  Returns the ``test_stats`` dict."""
    from . import evaluate as ev
    present = sorted({int(e) for t in dataset.props["nxyz"] for e in t[:, 0].tolist()})
    radii = None
    if params["synthetic"]:
        # synthetic frames carry random type labels 1..8, not chemistry: labels without a tabulated radius take carbon's
        radii = {e: ev.COVALENT_RADII[6] for e in present if e not in ev.COVALENT_RADII}
    else:
        try:
            ev.bond_radii(present)
        except KeyError as err:
            # a trajectory with elements outside the radius table: the bond-graph metrics are undefined for it -- say so
            # and leave the trained model (already saved) without an evaluation rather than fail the run
            print(f"evaluation skipped: {err.args[0]}", file=sys.stderr, flush=True)
            return None
    bs = max(int(params["batch_size"]), 1)

    def batches(idx, cap=None):
        starts = range(0, len(idx), bs)
        for start in (list(starts)[:cap] if cap is not None else starts):
            yield cgdata.CG_collate([dataset[i] for i in idx[start:start + bs]])

    def unaligned(true_xyz, recon_xyz, z):
        # run_ala.py:338-348 (frames of one molecule: the heavy filter is per atom of the concatenated frames)
        if not len(true_xyz):
            return None, None
        d2 = np.power(recon_xyz - true_xyz, 2).sum(-1)
        heavy = z != 1
        return float(np.sqrt(d2.mean())), (float(np.sqrt(d2[heavy].mean())) if heavy.any() else float("nan"))

    def z_of(idx, cap=None):
        idx = idx[:cap * bs] if cap is not None else idx
        return np.concatenate([dataset[i]["nxyz"][:, 0].numpy() for i in idx]) if idx else np.zeros(0)
    cap = max(int(params["nevals"]), 0)
    stats = {c: None for c in ev.CV_STATS_COLUMNS}
    tr = ev.reconstruction_quality(batches(train_idx, cap), model, reflection=False, radii=radii)
    stats["train_all_recon"], stats["train_heavy_recon"] = unaligned(tr[0], tr[1], z_of(train_idx, cap))
    if last_epoch:
        stats.update({"train_KL": last_epoch["train_KL"], "test_KL": last_epoch["val_KL"],
                      "train_graph": last_epoch["train_graph"], "test_graph": last_epoch["val_graph"]})
    samples = None
    if val_idx:
        te = ev.reconstruction_quality(batches(val_idx), model, reflection=params["reflectiontest"], radii=radii)
        stats["test_all_recon"], stats["test_heavy_recon"] = unaligned(te[0], te[1], z_of(val_idx))
        stats.update({"recon_all_valid_ratio": float(te[3]), "recon_heavy_valid_ratio": float(te[4]),
                      "recon_all_ged": float(te[5]), "recon_heavy_ged": float(te[6])})
        samples = ev.sample_ensemble([dataset[i] for i in val_idx], model, params["n_ensemble"],
                                     reflection=params["reflectiontest"], graph_eval=params["graph_eval"], radii=radii)
        if params["graph_eval"]:                                          # run_ala.py:370-385
            all_rmsds, heavy_rmsds, valid, valid_all, ged, ged_all = samples[4:]
            stats.update({"sample_heavy_valid_ratio": float(np.array(valid).mean()),
                          "sample_all_valid_ratio": float(np.array(valid_all).mean()),
                          "sample_all_rmsd": float(np.array(all_rmsds)[:, 0].mean()) if all_rmsds is not None else None,
                          "sample_heavy_rmsd": float(np.array(heavy_rmsds)[:, 1].mean()) if heavy_rmsds is not None else None,
                          "sample_heavy_ged": float(np.array(ged).mean()), "sample_all_ged": float(np.array(ged_all).mean())})
    if logdir:
        write_cv_stats(os.path.join(logdir, "cv_stats.csv"), stats)
        if stats["test_all_recon"] is not None:                          # run_ala.py:350-352
            for key, name in (("test_all_recon", "test_all_rmsd"), ("test_heavy_recon", "test_heavy_rmsd")):
                np.savetxt(os.path.join(logdir, "{}{:.4f}.txt".format(name, stats[key])), np.array([stats[key]]))
        if samples is not None and isinstance(samples[0], np.ndarray):
            np.savez_compressed(os.path.join(logdir, "samples.npz"), sample_xyzs=samples[0], data_xyzs=samples[1],
                                cg_xyzs=samples[2], recon_xyzs=samples[3], n_ensemble=params["n_ensemble"])
    for a in ANALYSES:
        if params.get(a.stem + "_eval"):
            head = (params,) if a.options else ()                         # an analysis with options reads them there
            stats[a.stem + "_stats"] = globals()[a.stem + "_eval"](*head, dataset, val_idx, samples, device, logdir)
    return stats


def _finish(a, full, logdir):
    """The full statistics of analysis ``a`` go to ``<stem>_stats.json`` in the log directory, their short form to the caller."""
    if logdir:
        with open(os.path.join(logdir, a.stem + "_stats.json"), "w") as f:
            json.dump(full, f)
    return a.module.summary_of(full)


def _hold_out_eval(stem, compare, dataset, val_idx, samples, logdir):
    """What ``--<stem>_eval`` does for every analysis of the hold-out frames against their prior samples (``samples``:
    ``evaluate.sample_ensemble``'s tuple): ``compare(ref, gen, z, bonds)`` gives the full statistics, or ``None`` after
    saying on stderr why it skipped.  Writes ``<stem>_stats.json``; returns the module's ``summary_of``, or ``None`` when
    there is nothing to compare (too few hold-out frames, or frames of different molecules)."""
    a = BY_STEM[stem]
    if samples is None or not isinstance(samples[0], np.ndarray) or len(val_idx) < a.min_frames:
        print(f"--{stem}_eval skipped: it needs at least {'two' if a.min_frames == 2 else 'four'} hold-out frames of one molecule",
              file=sys.stderr, flush=True)
        return None
    frame = dataset[val_idx[0]]
    z, n = frame["nxyz"][:, 0].numpy().astype(np.int64), int(frame["nxyz"].shape[0])
    full = compare(samples[1], samples[0].reshape(-1, n, 3), z, frame["bond_edge_list"].numpy() if a.needs_bonds else None)
    return None if full is None else _finish(a, full, logdir)


def dist_eval(dataset, val_idx, samples, device, logdir):
    """``--dist_eval``: over the internal coordinates of the molecule's bond graph (``distributions.compare``)."""
    return _hold_out_eval("dist", lambda ref, gen, z, bonds: distributions.compare(ref, gen, z, bonds, device=device),
                          dataset, val_idx, samples, logdir)


def cov_eval(dataset, val_idx, samples, device, logdir):
    """``--cov_eval``: by superposed heavy-atom RMSD (``coverage.compare``): does every hold-out frame have a sample near
    it, is every sample near a hold-out frame."""
    def compare(ref, gen, z, bonds):
        return coverage.compare(ref, gen, z, atoms="heavy" if (z != 1).any() else "all", device=device)
    return _hold_out_eval("cov", compare, dataset, val_idx, samples, logdir)


def contact_eval(dataset, val_idx, samples, device, logdir):
    """``--contact_eval``: by the contacts of their heavy atoms (``contacts.compare``): contact probability maps, native
    contacts, Rg.  The short form stays in the summary's ``"test_stats"``."""
    def compare(ref, gen, z, bonds):
        return contacts.compare(ref, gen, z, bonds, atoms="heavy" if (z != 1).sum() >= 2 else "all", device=device)
    return _hold_out_eval("contact", compare, dataset, val_idx, samples, logdir)


def flex_eval(dataset, val_idx, samples, device, logdir):
    """``--flex_eval``: by the fluctuation of their heavy atoms about each set's own mean structure
    (``flexibility.compare``); skipped also for fewer than three atoms.  The short form stays in ``"test_stats"``."""
    def compare(ref, gen, z, bonds):
        if z.shape[0] < 3:
            print("--flex_eval skipped: fewer than three atoms, no rotation to fit", file=sys.stderr, flush=True)
            return None
        return flexibility.compare(ref, gen, z, bonds, atoms="heavy" if (z != 1).sum() >= 3 else "all", device=device)
    return _hold_out_eval("flex", compare, dataset, val_idx, samples, logdir)


def kde_eval(dataset, val_idx, samples, device, logdir):
    """``--kde_eval``: as kernel density estimates in every (phi, psi) plane of the backbone (``density.compare_torsions``);
    skipped also for a molecule without a peptide backbone.  The short form stays in ``"test_stats"``."""
    def compare(ref, gen, z, bonds):
        if not distributions.peptide_backbone_torsions(z, bonds)[2]:
            print("--kde_eval skipped: the molecule has no peptide backbone, so no (phi, psi) plane", file=sys.stderr, flush=True)
            return None
        try:
            return density.compare_torsions(ref, gen, z, bonds, device=device)
        except ValueError as err:                                        # a torsion without spread, a kernel wider than period / 12
            print(f"--kde_eval skipped: {err}", file=sys.stderr, flush=True)
            return None
    return _hold_out_eval("kde", compare, dataset, val_idx, samples, logdir)


def tica_eval(params, dataset, val_idx, samples, device, logdir):
    """``--tica_eval``: TICA fitted on the frames of the ``-traj`` file IN FILE ORDER (the training order may be shuffled;
    a ``traj_starts`` key cuts the file into segments), the hold-out samples (``samples``: ``evaluate.sample_ensemble``'s
    tuple) compared with them.  Writes ``tica_stats.json``; returns ``tica.summary_of``, or ``None`` when there is
    nothing to compare: synthetic frames have no time order, the file is shorter than ``lag + 2`` frames, or the
    molecule has no peptide backbone."""
    lag = int(params.get("tica_lag", 100))
    if not params.get("traj"):
        print("--tica_eval skipped: synthetic frames have no time order (it needs -traj)", file=sys.stderr, flush=True)
        return None
    if samples is None or not isinstance(samples[0], np.ndarray):
        print("--tica_eval skipped: there are no hold-out samples", file=sys.stderr, flush=True)
        return None
    with np.load(params["traj"]) as f:
        xyz, z, bonds = np.asarray(f["xyz"], dtype=np.float32)[: params["ndata"]], f["z"], f["bonds"]
        starts = f["traj_starts"] if "traj_starts" in f.files else None
    if starts is not None:
        starts = np.asarray(starts)[np.asarray(starts) < xyz.shape[0]]
    if lag < 1 or xyz.shape[0] < lag + 2 or tica.backbone_atoms(z, bonds).shape[0] == 0:
        print(f"--tica_eval skipped: it needs a peptide backbone and at least lag + 2 = {lag + 2} frames in file order",
              file=sys.stderr, flush=True)
        return None
    full = tica.compare(tica.split_segments(xyz, starts), samples[0].reshape(-1, xyz.shape[1], 3), z, bonds, lag=lag, device=device)
    return _finish(BY_STEM["tica"], full, logdir)


def run(params) -> dict:
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    device = _device(str(params["device"]))
    torch.cuda.set_device(device)
    # the host side of a step is a few small tensor ops (collate, make_directed): on a many-core host torch's
    # default intra-op pool (one thread per core) turns each of them into a ~90 ms thread wake-up storm
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
        if params["batch_size"] % world:
            raise SystemExit("-batch_size must be divisible by the number of GPUs (equal-size shards)")
    if not params["synthetic"] and not params.get("traj"):
        raise SystemExit("pass -traj file.npz (a trajectory converted by tools/traj_to_npz.py) or --synthetic: the "
                         "reference's mdtraj / mdshare ingestion (datasets.py:170-187) is outside the hot path "
                         "(SURVEY.md 2.1 row 7)")
    seed = 123                                                          # run_ala.py:36-41
    torch.manual_seed(seed)
    np.random.seed(seed)
    beta = 0.0 if params["det"] else params["beta"]                      # run_ala.py:117-121
    map_info = None
    if params.get("traj"):
        dataset, mapping, map_info = load_trajectory_dataset(params, device)
    else:
        if params["dataset"] not in DATASET_SHAPES:
            raise SystemExit(f"unknown -dataset {params['dataset']}; known shapes: {sorted(DATASET_SHAPES)}")
        n_atoms = DATASET_SHAPES[params["dataset"]]
        box = {"dipeptide": 6.0, "chignolin": 14.0, "pentapeptide": 11.0}[params["dataset"]]
        dataset = cgdata.CGDataset(cgdata.synthetic_frames(params["ndata"], n_atoms, params["n_cgs"], box, seed=0))
        mapping = dataset.props["CG_mapping"][0]
    props = dataset.props
    # --cg_radius_graph has the reference's inverted sense: set => CG graph from bonds (run_ala.py:64-67)
    dataset.generate_neighbor_list(params["atom_cutoff"], None if params["cg_radius_graph"] else params["cg_cutoff"],
                                   device=device, undirected=True)
    n_train = int(0.9 * len(dataset))                                    # 10 % validation (run_ala.py:146-156)
    order = np.random.permutation(len(dataset)) if params["shuffle"] else np.arange(len(dataset))
    train_idx, val_idx = order[:n_train].tolist(), order[n_train:].tolist()

    model = build_model(params["n_basis"], params["n_rbf"], params["atom_cutoff"], params["cg_cutoff"],
                        params["enc_nconv"], params["dec_nconv"], params["n_cgs"], activation=params["activation"],
                        det=params["det"], invariantdec=params["invariantdec"], cg_mp=params["cg_mp"], seed=seed).to(device)
    if params["optimizer"] not in optim_dict:
        raise SystemExit("-optimizer must be one of " + ", ".join(optim_dict))
    trainer = Trainer(model, lr=params["lr"], beta=beta, gamma=params["gamma"], world_size=world, optimizer=params["optimizer"])
    use_graph = not params.get("no_hip_graph", False)                     # capture the step once, replay it on every batch
    min_lr, best, bad_epochs = 5e-8, None, 0                              # ReduceLROnPlateau(patience=2), run_ala.py:212-214
    early = EarlyStopping(patience=params["patience"])
    logdir = resolve_logdir(params) if params["logdir"] else None
    if rank == 0 and logdir:
        os.makedirs(logdir, exist_ok=True)
        with open(os.path.join(logdir, "modelparams.json"), "w") as f:
            json.dump({**stored_params(params), "mapping": torch.as_tensor(mapping).tolist()}, f, indent=4)
    log_rows, failed = [], False
    columns = ["epoch", "lr", "train_loss", "val_loss", "train_recon", "val_recon", "train_KL", "val_KL",
               "train_graph", "val_graph"]
    t_start = time.time()
    frames_seen = 0
    for epoch in range(params["nepochs"]):
        stats = {}
        for mode, idx in (("train", train_idx), ("val", val_idx)):
            tot, kls, recs, grs = [], [], [], []
            is_train = mode == "train"
            ready = (lambda t=is_train: trainer.has_graph(t)) if use_graph else None
            for batch in _batches(dataset, idx, params["batch_size"], rank, world, device, prepared=ready):
                if use_graph and trainer.arena is not None and not trainer.has_graph(is_train) and "_graph" in batch:
                    trainer.capture(batch, warmup=0, train=is_train)       # from the second step on: one graph per mode
                loss = trainer.step(batch, train=is_train).clone()         # (a replay refreshes the result tensors in place)
                kl, recon, graph = (t.clone() for t in trainer.last_terms)
                tot.append(loss), kls.append(kl), recs.append(recon), grs.append(graph)
                frames_seen += params["batch_size"] if mode == "train" else 0

            def mean(xs, keep=None):                       # one sync per epoch
                if not xs:
                    return float("nan")
                x = torch.stack(xs)
                if keep is not None:
                    x = x[keep]
                return float(x.mean()) if x.numel() else float("nan")
            # utils.py:145-148: a skipped batch (loss >= 200 gamma or NaN) contributes its KL but not its loss / recon /
            # graph terms to the epoch means
            keep = None
            if tot:
                lt = torch.stack(tot)
                keep = ~((lt >= 200.0 * params["gamma"]) | torch.isnan(lt))
            stats.update({f"{mode}_loss": mean(tot, keep), f"{mode}_KL": mean(kls), f"{mode}_recon": mean(recs, keep),
                          f"{mode}_graph": mean(grs, keep)})
        stats.update({"epoch": epoch, "lr": trainer.lr})
        log_rows.append(stats)
        if rank == 0:
            print(" ".join(f"{k}={stats[k]:.5g}" for k in columns), flush=True)
            if logdir:
                with open(os.path.join(logdir, "train_log.csv"), "w") as f:
                    f.write(",".join(columns) + "\n")
                    for r in log_rows:
                        f.write(",".join(str(r[c]) for c in columns) + "\n")
        val = stats["val_loss"]
        if not val_idx or len(val_idx) < world:
            # no validation frames (-ndata < 10, or fewer than ranks): not the reference's NaN failure (run_ala.py:278-281,
            # which means the model diverged) -- schedule and early stopping follow the training loss instead
            val = stats["train_loss"]
        elif np.isnan(stats["val_recon"]):                                # run_ala.py:278-281
            failed = True
            break
        # NB the reference feeds ReduceLROnPlateau / EarlyStopping the lowess-smoothed validation curve
        # (statsmodels, run_ala.py:259-275); statsmodels is not a dependency here and the control plane is outside the
        # hot path: the raw value is used.  LR-decay / stopping epochs can differ on noisy runs.
        if best is None or val < best * (1 - params["threshold"]):
            best, bad_epochs = val, 0
        else:
            bad_epochs += 1
            if bad_epochs > 2:
                trainer.lr = max(trainer.lr * params["factor"], min_lr)
                bad_epochs = 0
        if trainer.lr <= min_lr * 1.5:
            break
        early(val)
        if early.early_stop:
            break
    trainer.flush()                                                       # the last step's (deferred) parameter update
    elapsed = time.time() - t_start
    if rank == 0 and logdir:
        torch.save(model.state_dict(), os.path.join(logdir, "model.pt"))    # run_ala.py:355-357
        if failed:
            with open(os.path.join(logdir, "FAILED.txt"), "w") as f:
                print("TRAINING FAILED", file=f)
    test_stats = None
    if rank == 0 and not failed:                                          # the other ranks wait at the teardown below
        test_stats = evaluate_run(params, model, dataset, train_idx, val_idx, device, log_rows[-1] if log_rows else None, logdir)
    if world > 1:
        torch.distributed.destroy_process_group()
    top = {a.stem + "_stats": test_stats.pop(a.stem + "_stats", None) if test_stats else None
           for a in ANALYSES if a.top_level and params.get(a.stem + "_eval")}
    return {**top, "epochs": len(log_rows), "seconds": elapsed, "train_frames_per_s": frames_seen / max(elapsed, 1e-9),
            "final": log_rows[-1] if log_rows else None, "failed": failed, "skipped_steps": trainer.skipped_steps(),
            "graph_replays": trainer.replays, "test_stats": test_stats,
            **({"cg_mapping": {k: map_info[k] for k in CG_MAPPING_KEYS.get(map_info.get("method"), CG_PARTITION_KEYS)
                               if k in map_info}} if map_info else {})}


def main(argv=None):
    extras, rest = build_extras_parser().parse_known_args(argv)
    params = vars(build_parser().parse_args(rest))
    params.update(vars(extras))
    params["savemodel"] = True                                            # run_ala.py:464
    summary = run(params)
    if int(os.environ.get("RANK", "0")) == 0:
        print(json.dumps(summary))


if __name__ == "__main__":
    main(sys.argv[1:])
