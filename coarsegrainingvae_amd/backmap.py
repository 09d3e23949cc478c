#!/usr/bin/env python3
"""Backmapping: all-atom ensembles for a coarse-grained trajectory from a trained run, judged without a reference frame.

``evaluate.sample_ensemble`` needs the all-atom frame of every bead frame (``nxyz``, an atom neighbour list, the bonds) and
compares every sample with it.  A user who ran a CG simulation has bead coordinates only.  The decoder needs nothing
else: per chunk of frames this module builds the bead graph, calls ``model.prior_net`` ONCE, draws the latents of all
``frames x samples`` copies, calls ``model.decoder`` ONCE on the replicated bead graph (``evaluate.ensemble_batch``),
launches K14 (``cgv_ensemble_check``) ONCE and reads everything back ONCE.  No atom-level graph is built and
``model(batch)`` is never called.  What can still be asked of the samples:

  validity   does the sample have exactly the bond graph of the molecule's topology (K12's distance criterion
             ``(r_a + r_b) * 1.3``, tested against a bond list)?   needs ``z`` and ``bonds``
  diversity  the pairwise RMSD of the K samples of a frame -- the reference marks the place with
             ``# compute sample diversity`` (scripts/sampling.py:296) and computes nothing there

    python -m coarsegrainingvae_amd.backmap -model LOGDIR (-cg cg.npz | -traj atoms.npz) [-top top.npz] -n_samples K
        -out out.npz [-frames_per_launch M] [-seed S] [--pair_rmsd] [--require_valid all|heavy -max_rounds R]
        [--dist_stats [-ref atoms.npz]] [--tica_stats [-tica_lag 100] [-tica_bins 50]]
        [--cov_stats [-cov_thresholds 0.5 1.0 2.0] [-cov_atoms heavy]]
        [--contact_stats [-contact_cutoff 4.5] [-contact_atoms heavy|all] [-contact_exclude 3]
         [-contact_groups none|bead|residue]]
        [--flex_stats [-flex_atoms heavy|all] [-flex_groups none|bead|residue] [-flex_aligned aligned.npz]]
        [--kde_stats [-kde_plane torsion|tica] [-kde_grid 100] [-kde_bw scott|silverman|<float>]]

``-cg``: ``cg_xyz [T,N,3]`` in Angstrom.  ``-traj``: a ``tools/traj_to_npz.py`` file; its beads are the ``scatter_mean`` of
the atoms over the run's mapping (no rotation) -- the "coarse-grain, then backmap" round trip -- and its ``z`` / ``bonds``
are the topology unless ``-top`` (``z [n]``, ``bonds [Eb,2]``) is given.  The mapping comes from the run's
``modelparams.json``.  Output: ``xyz [T,K,n,3]``, ``cg_xyz``, ``mapping``, ``n_samples``, ``seed``, ``diversity_all`` /
``diversity_heavy [T]``, with a topology also ``valid_all`` / ``valid_heavy [T,K]`` and ``counts [T,K,4]`` (missing_all,
extra_all, missing_heavy, extra_heavy), with ``--pair_rmsd`` ``pair_rmsd_all`` / ``pair_rmsd_heavy [T,K,K]``, with
``--require_valid`` ``n_valid [T]``.  One JSON summary line goes to stdout.

``--dist_stats``: do the generated structures reproduce the distribution of all-atom data?  ``distributions.compare`` of
all ``T * K`` of them against the frames of ``-ref`` (a ``tools/traj_to_npz.py`` file with the topology's atom order;
default: the frames of ``-traj``): per-feature and per-(phi, psi) Jensen-Shannon divergences with their noise floor go to
``dist_stats.json`` next to ``-out``, their means into the summary line under ``"dist_stats"``.  Needs a topology.

``--tica_stats``: do they populate the slow, collective states of the simulation?  ``tica.compare``: TICA (lag
``-tica_lag`` frames) of the backbone distances is fitted on the frames of ``-ref`` (default: those of ``-traj``; a
``traj_starts`` key of the file cuts them into segments) taken as a time-ordered trajectory, the generated structures are
projected on its two slowest components and the maps compared over ``-tica_bins`` x ``-tica_bins`` bins.  Everything goes
to ``tica_stats.json`` next to ``-out``, the short form into the summary line under ``"tica_stats"``.  Needs a topology
with a peptide backbone and at least ``lag + 2`` reference frames.

``--cov_stats``: does every reference frame have a backmapped structure near it, and is every backmapped structure near
some reference frame?  ``coverage.compare``: superposed RMSD (K17) between all ``T * K`` structures and the frames of
``-ref`` (default: those of ``-traj``) over the ``-cov_atoms`` (``heavy`` or ``all``): COV-R / MAT-R, COV-P / MAT-P at the
``-cov_thresholds`` (Angstrom), with the even / odd floor of the reference, go to ``cov_stats.json`` next to ``-out``, the
short form into the summary line under ``"cov_stats"``.  Needs a topology (for the elements).

``--contact_stats``: do the backmapped structures pack as the reference does?  ``contacts.compare``: the contact
probability of every pair of ``-contact_atoms`` (``heavy`` or ``all``) closer than ``-contact_cutoff`` Angstrom and more
than ``-contact_exclude`` bonds apart (K20) -- or, with ``-contact_groups bead | residue``, of every pair of beads of the
run's mapping or of residues of a peptide -- over all ``T * K`` structures against the frames of ``-ref`` (default: those
of ``-traj``), the fraction of native contacts and the radius of gyration of every structure, with the even / odd floor of
the reference, go to ``contact_stats.json`` next to ``-out``, the short form into the summary line under
``"contact_stats"``.  Needs a topology.  These switches are absent from the parsed arguments unless given.

``--flex_stats``: do the backmapped structures move as much as the reference does?  ``flexibility.compare``: all ``T * K``
structures and the frames of ``-ref`` (default: those of ``-traj``) are each superposed about their own mean structure
over the ``-flex_atoms`` (``heavy`` or ``all``; K21) and the per-atom fluctuations (RMSF) -- or, with ``-flex_groups bead |
residue``, those of the beads of the run's mapping or of the residues of a peptide -- are compared, with the even / odd
floor of the reference: ``flex_stats.json`` next to ``-out``, the short form into the summary line under
``"flex_stats"``.  ``-flex_aligned file.npz`` also writes the backmapped structures in their mean's frame (``xyz``
[T*K,n,3]), the mean (``mean``), ``rmsf`` and the selection (``atoms``).  Needs a topology.  These switches, too, are
absent from the parsed arguments unless given.

``--kde_stats``: do the backmapped structures have the free-energy surface of the reference?  ``density.compare_torsions``
(``-kde_plane torsion``: every (phi, psi) plane of the backbone) or ``density.compare_tica`` (``tica``: the reference's
(IC1, IC2) plane at ``-tica_lag``): Gaussian kernel density estimates (K22) of all ``T * K`` structures and of the frames
of ``-ref`` on ``-kde_grid`` nodes per axis with bandwidth ``-kde_bw``, their Jensen-Shannon divergence, the RMS
difference of their free energies and the mean log density of the structures under the reference's estimate, with the
even / odd floor of the reference: ``kde_stats.json`` next to ``-out``, the short form into the summary line under
``"kde_stats"``.  Needs a topology with a peptide backbone and at least four reference frames.  Absent unless given.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Dict, Optional

import numpy as np
import torch

from . import contacts, coverage, density, distributions, flexibility, tica
from . import evaluate as ev
from .analyses import ANALYSES, BY_STEM
from .compare_cli import read_npz
from .train import build_model


# ----------------------------------------------------------------------------- a trained run
def read_params(logdir: str) -> dict:
    path = os.path.join(logdir, "modelparams.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: not a run directory of run_ala (-logdir)")
    with open(path) as f:
        params = json.load(f)
    if params.get("det"):
        raise ValueError(f"{logdir} is a --det run: it was trained without the prior's latent terms, there is no prior "
                         "to sample from")
    if "mapping" not in params:
        raise ValueError(f"{path} carries no atom -> bead mapping")
    return params


def load_run(logdir: str, device="cuda"):
    """``(model, params)`` of a run directory written by ``run_ala``: ``modelparams.json`` (the flags, plus the atom ->
    bead ``mapping``) and ``model.pt``, through ``train.build_model`` with ``strict=True``.  A ``--det`` run is refused."""
    params = read_params(logdir)
    model = build_model(params["n_basis"], params["n_rbf"], params["atom_cutoff"], params["cg_cutoff"], params["enc_nconv"],
                        params["dec_nconv"], params["n_cgs"], activation=params.get("activation", "swish"), det=False,
                        invariantdec=params.get("invariantdec", False), cg_mp=params.get("cg_mp", False), seed=None)
    state = torch.load(os.path.join(logdir, "model.pt"), map_location="cpu")
    model.load_state_dict(state, strict=True)
    return model.to(device), params


def check_topology(mapping, z=None, bonds=None) -> None:
    """A topology must describe the molecule the run was trained on: as many atoms as the mapping."""
    n = int(np.asarray(mapping).shape[0])
    if z is not None and int(np.asarray(z).shape[0]) != n:
        raise ValueError(f"the topology has {int(np.asarray(z).shape[0])} atoms, the run's mapping {n}")
    if bonds is not None and np.size(bonds) and int(np.asarray(bonds).max()) >= n:
        raise ValueError(f"the topology's bonds name atom {int(np.asarray(bonds).max())}, the run's mapping has {n} atoms")


def canonical_bonds(bonds) -> np.ndarray:
    """A bond list as K14 takes it: pairs ordered ``i < j``, sorted, every pair once (trajectory files list a bond in
    either orientation).  Self bonds stay and are refused by the launch's validation."""
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    b = np.where((b[:, 0] <= b[:, 1])[:, None], b, b[:, ::-1])
    return np.unique(b, axis=0) if b.shape[0] else b


# ----------------------------------------------------------------------------- the sampler
def _plan_for(z, sizes, device, scale, radii) -> ev.QualityPlan:
    fp = np.concatenate([[0], np.cumsum(sizes)])
    if z is None:
        # elements unknown: one class that bonds nothing and no heavy atoms (all-atom diversity only)
        return ev.QualityPlan(np.ones(int(fp[-1]), dtype=np.int64), fp, device, thresholds=np.zeros((1, 1), np.float32))
    return ev.QualityPlan(np.tile(np.asarray(z).astype(np.int64), len(sizes)), fp, device, scale, radii)


def backmap(model, cg_xyz, mapping, n_samples: int, cg_cutoff: float, *, z=None, bonds=None, eps=None,
            frames_per_launch: int = 8, cg_bonds=None, radii: Optional[Dict[int, float]] = None, scale: float = 1.3) -> dict:
    """``n_samples`` all-atom structures for every frame of the bead trajectory ``cg_xyz [T,N,3]`` (Angstrom) of one
    molecule with the atom -> bead ``mapping [n]``.  ``cg_cutoff``: the radius of the bead graph the model was trained
    with; ``cg_bonds [Ec,2]``: a fixed bead graph used instead (runs trained with ``--cg_radius_graph``:
    ``data._bond_cg_graph`` of the molecule's bonds).  ``eps [T * n_samples * N, F]``: the latents' noise in output
    order (frame, sample, bead) as for ``evaluate.sample_ensemble``; without it the device generator draws it
    (``ops.reparam_sample``; bracket with ``ops.get_sample_rng_state`` / ``set_sample_rng_state``; the generator advances
    per launch, so the same state reproduces the same structures for the same ``frames_per_launch``).

    Returns a dict of host arrays: ``xyz [T,K,n,3]`` float32, ``cg_xyz [T,N,3]``, ``pair_rmsd_all [T,K,K]``,
    ``diversity_all [T]`` (mean pairwise RMSD over ``k < l``; ``nan`` for one sample); with ``z`` (atomic numbers) also
    ``pair_rmsd_heavy`` / ``diversity_heavy``; with ``z`` and ``bonds [Eb,2]`` (``i < j``, unique) also ``counts [T,K,4]``,
    ``valid_all`` / ``valid_heavy [T,K]``.

    Per chunk of ``frames_per_launch`` frames: one batched bead radius graph (the function
    ``CGDataset.generate_neighbor_list`` uses: it reads the edge list back, its length being data dependent), one
    ``model.prior_net`` call, one ``model.decoder`` call, one K14 launch, one read-back of the results.  Runs under
    ``no_grad``; ``model.training`` is left as found."""
    from . import ops
    from .data import _batched_radius
    from .graph import BatchGraph
    K, M = int(n_samples), max(int(frames_per_launch), 1)
    cg = torch.as_tensor(np.asarray(cg_xyz.detach().cpu() if torch.is_tensor(cg_xyz) else cg_xyz), dtype=torch.float32)
    if cg.dim() != 3 or cg.shape[2] != 3:
        raise ValueError("cg_xyz must be [frames, beads, 3]")
    T, N = int(cg.shape[0]), int(cg.shape[1])
    mapping = torch.as_tensor(np.asarray(mapping.detach().cpu() if torch.is_tensor(mapping) else mapping)).long().reshape(-1)
    n = int(mapping.shape[0])
    if K < 1:
        raise ValueError("n_samples must be at least 1")
    if n == 0 or int(mapping.min()) < 0 or int(mapping.max()) >= N:
        raise ValueError(f"mapping must send every atom to one of the {N} beads")
    check_topology(mapping, z, bonds)
    if bonds is not None and z is None:
        raise ValueError("a bond list needs the atomic numbers z (the bond cutoffs are per element pair)")
    dev = ev.model_device(model)
    bead_id = torch.arange(N).float()[:, None]                 # column 0 as build_dataset writes it
    cg_nxyz = [torch.cat([bead_id, cg[t]], dim=1) for t in range(T)]
    atoms = torch.empty(n, 4)                                  # ensemble_batch reads its row count only
    fixed = torch.as_tensor(np.asarray(cg_bonds)).long().reshape(-1, 2) if cg_bonds is not None else None
    plans, out = {}, {"xyz": np.empty((T, K, n, 3), np.float32), "cg_xyz": cg.numpy().copy(),
                      "pair_rmsd_all": np.empty((T, K, K)), "diversity_all": np.empty(T)}
    if z is not None:
        out.update(pair_rmsd_heavy=np.empty((T, K, K)), diversity_heavy=np.empty(T))
    if bonds is not None:
        out.update(counts=np.empty((T, K, 4), np.int32), valid_all=np.empty((T, K), bool), valid_heavy=np.empty((T, K), bool))
    eps_at = 0
    was_training = model.training
    try:
        with torch.no_grad():
            ev.settle(model)
            for start in range(0, T, M):
                B = min(M, T - start)
                rows = cg_nxyz[start:start + B]
                nbrs = [fixed] * B if fixed is not None else _batched_radius(rows, cg_cutoff, dev, True)
                chunk = [{"CG_nxyz": rows[f], "nxyz": atoms, "CG_nbr_list": nbrs[f], "CG_mapping": mapping} for f in range(B)]
                rep = ev.ensemble_batch(chunk, K, dev)
                cg_rows = torch.cat(rows).to(dev)
                offs = torch.arange(B)[:, None] * N
                # the prior's bundle: bead graph and atom -> bead plan of the unreplicated chunk, an empty atom graph
                graph = BatchGraph(torch.zeros(B * n, 3, device=dev), cg_rows[:, 1:], (mapping[None, :] + offs).reshape(-1).to(dev),
                                   torch.zeros(0, 2, dtype=torch.int64, device=dev),
                                   torch.cat([nb + f * N for f, nb in enumerate(nbrs)]).to(dev))
                mu, sigma = model.prior_net(cg_rows[:, 0], graph.cg_xyz, graph.cg_nbrs, graph=graph)
                mu_r, sigma_r = mu[rep["src_bead"]], sigma[rep["src_bead"]]
                if eps is not None:
                    e = eps[eps_at:eps_at + mu_r.shape[0]].to(dev)
                    eps_at += mu_r.shape[0]
                    H = e.mul(sigma_r).add_(mu_r)
                else:
                    H = ops.reparam_sample(mu_r.contiguous(), sigma_r.contiguous())
                g_rep = rep["_graph"]
                gen = model.decoder(g_rep.cg_xyz, rep["CG_nbr_list"], H, H, rep["CG_mapping"], rep["num_CGs"], graph=g_rep)
                if B not in plans:                             # one molecule: the plan depends on the chunk's frame count only
                    plan = _plan_for(z, [n] * B, dev, scale, radii)
                    plans[B] = (plan, ev.BondList(bonds, plan) if bonds is not None else None)
                plan, bond_list = plans[B]
                raw = ev.ensemble_check(gen, K, plan, bond_list)
                gen_h, counts_h, sums_h = ev.read_back([gen, raw.counts, raw.pair_sums])
                out["xyz"][start:start + B] = gen_h.reshape(B, K, n, 3)
                for f in range(B):
                    chk = ev.assemble_ensemble_check(counts_h[f], sums_h[f], n, int(plan.n_heavy[f]))
                    t = start + f
                    out["pair_rmsd_all"][t], out["diversity_all"][t] = chk.pair_rmsd_all, chk.diversity_all
                    if z is not None:
                        out["pair_rmsd_heavy"][t], out["diversity_heavy"][t] = chk.pair_rmsd_heavy, chk.diversity_heavy
                    if bonds is not None:
                        out["counts"][t], out["valid_all"][t], out["valid_heavy"][t] = counts_h[f], chk.valid_all, chk.valid_heavy
    finally:
        model.train(was_training)
    out["n_samples"] = K
    return out


def backmap_valid(model, cg_xyz, mapping, n_samples: int, cg_cutoff: float, *, z, bonds, which: str = "all",
                  max_rounds: int = 4, **kw) -> dict:
    """``backmap`` that keeps valid samples only (``which``: the ``all``-atom or the ``heavy``-atom bond graph).  After
    the first draw, every frame with fewer than K valid samples gets K fresh draws per round, for at most ``max_rounds``
    rounds; valid samples are kept in draw order and a full frame is never drawn again.  A frame still short at the end
    is filled with the invalid draws of its last round and stays flagged in ``valid_*``.  The checks of the returned
    ensembles come from one final K14 pass over them.  Extra entries: ``n_valid [T]`` and ``n_valid_rounds [rounds,T]``
    (after the first draw and after every redraw).  One read-back per round and chunk, one for the final pass."""
    if which not in ("all", "heavy"):
        raise ValueError("which must be 'all' or 'heavy'")
    if kw.get("eps") is not None:
        raise ValueError("backmap_valid draws its own noise")
    K = int(n_samples)
    cg = np.asarray(cg_xyz.detach().cpu() if torch.is_tensor(cg_xyz) else cg_xyz, dtype=np.float32)
    first = backmap(model, cg, mapping, K, cg_cutoff, z=z, bonds=bonds, **kw)
    T, n = cg.shape[0], first["xyz"].shape[2]
    kept = [first["xyz"][t][first["valid_" + which][t]] for t in range(T)]      # valid samples, draw order
    spare = [first["xyz"][t][~first["valid_" + which][t]] for t in range(T)]    # the last round's invalid draws
    history = [np.array([min(len(k), K) for k in kept])]
    for _ in range(max(int(max_rounds), 0)):
        short = [t for t in range(T) if len(kept[t]) < K]
        if not short:
            break
        more = backmap(model, cg[short], mapping, K, cg_cutoff, z=z, bonds=bonds, **kw)
        for i, t in enumerate(short):
            ok = more["valid_" + which][i]
            kept[t] = np.concatenate([kept[t], more["xyz"][i][ok]])[:K]
            spare[t] = more["xyz"][i][~ok]
        history.append(np.array([min(len(k), K) for k in kept]))
    xyz = np.stack([np.concatenate([kept[t], spare[t][:K - len(kept[t])]]) if len(kept[t]) < K else kept[t] for t in range(T)])
    out = _check_only(model, xyz, cg, z, bonds, kw.get("frames_per_launch", 8), kw.get("radii"), kw.get("scale", 1.3))
    out.update(n_valid=history[-1], n_valid_rounds=np.stack(history), n_samples=K)
    return out


def _check_only(model, xyz, cg, z, bonds, frames_per_launch, radii, scale) -> dict:
    """K14 over finished ensembles ``xyz [T,K,n,3]``: the entries of ``backmap``'s result."""
    T, K, n = xyz.shape[:3]
    dev, M = ev.model_device(model), max(int(frames_per_launch), 1)
    out = {"xyz": xyz, "cg_xyz": cg.copy(), "pair_rmsd_all": np.empty((T, K, K)), "diversity_all": np.empty(T),
           "pair_rmsd_heavy": np.empty((T, K, K)), "diversity_heavy": np.empty(T), "counts": np.empty((T, K, 4), np.int32),
           "valid_all": np.empty((T, K), bool), "valid_heavy": np.empty((T, K), bool)}
    plans = {}
    for start in range(0, T, M):
        B = min(M, T - start)
        if B not in plans:
            plan = _plan_for(z, [n] * B, dev, scale, radii)
            plans[B] = (plan, ev.BondList(bonds, plan))
        plan, bond_list = plans[B]
        raw = ev.ensemble_check(torch.from_numpy(xyz[start:start + B].reshape(-1, 3)).to(dev), K, plan, bond_list)
        counts_h, sums_h = ev.read_back([raw.counts, raw.pair_sums])
        for f in range(B):
            chk, t = ev.assemble_ensemble_check(counts_h[f], sums_h[f], n, int(plan.n_heavy[f])), start + f
            out["pair_rmsd_all"][t], out["diversity_all"][t] = chk.pair_rmsd_all, chk.diversity_all
            out["pair_rmsd_heavy"][t], out["diversity_heavy"][t] = chk.pair_rmsd_heavy, chk.diversity_heavy
            out["counts"][t], out["valid_all"][t], out["valid_heavy"][t] = counts_h[f], chk.valid_all, chk.valid_heavy
    return out


# ----------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m coarsegrainingvae_amd.backmap", description="all-atom ensembles for a "
                                "coarse-grained trajectory from a trained run, with reference-free checks")
    p.add_argument("-model", type=str, required=True, help="run directory of run_ala (modelparams.json, model.pt)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("-cg", type=str, help=".npz with cg_xyz [T,N,3] in Angstrom")
    src.add_argument("-traj", type=str, help="tools/traj_to_npz.py file: coarse-grained with the run's mapping, then backmapped")
    p.add_argument("-top", type=str, default=None, help=".npz with z [n] and bonds [Eb,2] (default: those of -traj)")
    p.add_argument("-n_samples", type=int, required=True)
    p.add_argument("-out", type=str, required=True)
    p.add_argument("-frames_per_launch", type=int, default=8)
    p.add_argument("-seed", type=int, default=0, help="seed of the device sample generator")
    p.add_argument("-device", type=str, default="0")
    p.add_argument("--pair_rmsd", action="store_true", default=False, help="also write pair_rmsd_all / pair_rmsd_heavy [T,K,K]")
    p.add_argument("--require_valid", choices=("all", "heavy"), default=None,
                   help="keep valid samples only, redrawing short frames (needs a topology)")
    p.add_argument("-max_rounds", type=int, default=4, help="redraw rounds of --require_valid")
    p.add_argument("--dist_stats", action="store_true", default=False,
                   help="compare the internal-coordinate distributions of the output with -ref; writes dist_stats.json next to -out")
    p.add_argument("-ref", type=str, default=None, help="all-atom tools/traj_to_npz.py file, same atom order (default: the frames of -traj)")
    p.add_argument("--tica_stats", action="store_true", default=False,
                   help="compare the output with -ref in the plane of the reference's two slowest independent components; "
                        "writes tica_stats.json next to -out")
    p.add_argument("-tica_lag", type=int, default=100, help="lag of --tica_stats in frames of the reference")
    p.add_argument("-tica_bins", type=int, default=50, help="bins per component of --tica_stats")
    p.add_argument("--cov_stats", action="store_true", default=False,
                   help="coverage and precision of the output against -ref by superposed RMSD; writes cov_stats.json next to -out")
    p.add_argument("-cov_thresholds", type=float, nargs="+", default=[0.5, 1.0, 2.0], help="RMSD thresholds of --cov_stats in Angstrom")
    p.add_argument("-cov_atoms", choices=("heavy", "all"), default="heavy", help="atoms that --cov_stats superposes")
    # absent from the namespace unless given (CONTACT_DEFAULTS holds what they default to): a command line without them
    # parses to what it parsed to before they existed
    p.add_argument("--contact_stats", action="store_true", default=argparse.SUPPRESS,
                   help="contact probability maps, native contacts and Rg of the output against -ref; writes contact_stats.json next to -out")
    p.add_argument("-contact_cutoff", type=float, default=argparse.SUPPRESS, help="contact distance of --contact_stats in Angstrom (4.5)")
    p.add_argument("-contact_atoms", choices=("heavy", "all"), default=argparse.SUPPRESS, help="atoms that --contact_stats looks at (heavy)")
    p.add_argument("-contact_exclude", type=int, default=argparse.SUPPRESS,
                   help="pairs at most this many bonds apart are no contacts (3)")
    p.add_argument("-contact_groups", choices=("none", "bead", "residue"), default=argparse.SUPPRESS,
                   help="contacts between atoms (none), beads of the run's mapping, or residues of a peptide (none)")
    p.add_argument("--flex_stats", action="store_true", default=argparse.SUPPRESS,
                   help="mean structure and per-atom fluctuation (RMSF) of the output against -ref; writes flex_stats.json next to -out")
    p.add_argument("-flex_atoms", choices=("heavy", "all"), default=argparse.SUPPRESS,
                   help="atoms that --flex_stats superposes and reports (heavy)")
    p.add_argument("-flex_groups", choices=("none", "bead", "residue"), default=argparse.SUPPRESS,
                   help="a profile row per atom (none), per bead of the run's mapping, or per residue of a peptide (none)")
    p.add_argument("-flex_aligned", type=str, default=argparse.SUPPRESS,
                   help="with --flex_stats: also write the output structures in their mean's frame, and the mean, to this .npz")
    p.add_argument("--kde_stats", action="store_true", default=argparse.SUPPRESS,
                   help="kernel density estimates (free-energy surfaces) of the output against -ref in the backbone-torsion or "
                        "TICA plane; writes kde_stats.json next to -out")
    p.add_argument("-kde_plane", choices=("torsion", "tica"), default=argparse.SUPPRESS,
                   help="plane of --kde_stats: every (phi, psi) pair, or (IC1, IC2) with -tica_lag (torsion)")
    p.add_argument("-kde_grid", type=int, default=argparse.SUPPRESS, help="grid nodes per axis of --kde_stats (100)")
    p.add_argument("-kde_bw", type=kde_bandwidth, default=argparse.SUPPRESS,
                   help="bandwidth of --kde_stats: scott, silverman or a positive factor (scott)")
    return p


CONTACT_DEFAULTS = {"contact_stats": False, "contact_cutoff": 4.5, "contact_atoms": "heavy", "contact_exclude": 3,
                    "contact_groups": "none"}
FLEX_DEFAULTS = {"flex_stats": False, "flex_atoms": "heavy", "flex_groups": "none", "flex_aligned": None}
KDE_DEFAULTS = {"kde_stats": False, "kde_plane": "torsion", "kde_grid": 100, "kde_bw": "scott"}


def _option_group(args, defaults: dict) -> dict:
    """A switch and its options as parsed, with their defaults where they were not given (they are absent then)."""
    return {k: getattr(args, k, v) for k, v in defaults.items()}


def contact_args(args) -> dict:
    return _option_group(args, CONTACT_DEFAULTS)


def flex_args(args) -> dict:
    return _option_group(args, FLEX_DEFAULTS)


def kde_args(args) -> dict:
    return _option_group(args, KDE_DEFAULTS)


def kde_bandwidth(text: str):
    """``-kde_bw``: ``scott``, ``silverman`` or a positive number."""
    if text in ("scott", "silverman"):
        return text
    try:
        value = float(text)
    except ValueError:
        value = -1.0
    if not (value > 0 and np.isfinite(value)):
        raise argparse.ArgumentTypeError("scott, silverman or a positive number")
    return value


def read_inputs(args, params, device=None) -> dict:
    """The CLI's input files as ``cg_xyz``, ``z``, ``bonds`` (``None`` where absent), checked against the run's mapping.
    ``-traj`` frames are coarse-grained on ``device`` (``ops.scatter_mean`` over the mapping, no rotation)."""
    mapping = np.asarray(params["mapping"], dtype=np.int64)
    n, N = mapping.shape[0], int(mapping.max()) + 1
    z = bonds = ref_xyz = None
    on = [f"--{a.stem}_stats" for a in ANALYSES if getattr(args, a.stem + "_stats", False)]
    tica_stats, cov_stats = "--tica_stats" in on, "--cov_stats" in on
    contact, flex = contact_args(args), flex_args(args)
    if not flex["flex_stats"] and any(getattr(args, k, None) is not None for k in ("flex_atoms", "flex_groups", "flex_aligned")):
        raise SystemExit("-flex_atoms / -flex_groups / -flex_aligned are options of --flex_stats")
    kde = kde_args(args)
    if not kde["kde_stats"] and any(getattr(args, k, None) is not None for k in ("kde_plane", "kde_grid", "kde_bw")):
        raise SystemExit("-kde_plane / -kde_grid / -kde_bw are options of --kde_stats")
    kde_tica = kde["kde_stats"] and kde["kde_plane"] == "tica"
    need_ref, starts = bool(on), None
    if getattr(args, "ref", None) and not need_ref:
        raise SystemExit("-ref is the reference of " + " / ".join(f"--{a.stem}_stats" for a in ANALYSES))
    if args.cg:
        cg = np.asarray(read_npz(args.cg, ["cg_xyz"])["cg_xyz"], dtype=np.float32)
    else:
        f = read_npz(args.traj, ["xyz", "z", "bonds"])
        xyz, z, bonds, starts = np.asarray(f["xyz"], dtype=np.float32), f["z"], f["bonds"], f.get("traj_starts")
        if xyz.ndim != 3 or xyz.shape[1:] != (n, 3):
            raise SystemExit(f"{args.traj}: xyz is {xyz.shape}, the run's mapping has {n} atoms")
        from .ops import scatter_mean
        T = xyz.shape[0]
        ref_xyz = xyz if need_ref else None
        index = (torch.from_numpy(mapping).to(device)[None, :] + N * torch.arange(T, device=device)[:, None]).reshape(-1)
        cg = scatter_mean(torch.from_numpy(xyz).to(device).reshape(T * n, 3).contiguous(), index, dim=0,
                          dim_size=T * N).reshape(T, N, 3).cpu().numpy()
    if args.top:
        f = read_npz(args.top, ["z", "bonds"])
        z, bonds = f["z"], f["bonds"]
    if cg.ndim != 3 or cg.shape[1:] != (N, 3):
        raise SystemExit(f"cg_xyz is {cg.shape}, the run's mapping has {N} beads")
    try:
        check_topology(mapping, z, bonds)
    except ValueError as err:
        raise SystemExit(str(err))
    if bonds is not None:
        bonds = canonical_bonds(bonds)
    if args.require_valid and bonds is None:
        raise SystemExit("--require_valid needs a topology (-top, or the z / bonds of -traj)")
    if need_ref:
        switch = on[0]                                         # the first one asked for, in the table's order
        if bonds is None:
            raise SystemExit(f"{switch} needs a topology (-top, or the z / bonds of -traj)")
        if args.ref:
            f = read_npz(args.ref, ["xyz", "z"])
            ref_xyz, starts = np.asarray(f["xyz"], dtype=np.float32), f.get("traj_starts")
            if ref_xyz.ndim != 3 or ref_xyz.shape[1:] != (n, 3):
                raise SystemExit(f"{args.ref}: xyz is {ref_xyz.shape}, the topology has {n} atoms")
            if not np.array_equal(np.asarray(f["z"]).astype(np.int64).reshape(-1), np.asarray(z).astype(np.int64).reshape(-1)):
                raise SystemExit(f"{args.ref}: z differs from the topology's (the reference must list the same atoms in the same order)")
        if ref_xyz is None or ref_xyz.shape[0] < 2:
            raise SystemExit(f"{switch} needs reference frames: -ref file.npz (or -traj as the source), at least two")
        if tica_stats or kde_tica:
            if args.tica_lag < 1 or ref_xyz.shape[0] < args.tica_lag + 2:
                raise SystemExit(f"{'--tica_stats' if tica_stats else '--kde_stats -kde_plane tica'} needs 1 <= -tica_lag and at least lag + 2 reference frames: {ref_xyz.shape[0]} "
                                 f"frames, lag {args.tica_lag}")
            if tica.backbone_atoms(z, bonds).shape[0] == 0:
                raise SystemExit(f"{'--tica_stats' if tica_stats else '--kde_stats'}: the topology has no peptide backbone to take the distances from")
            try:
                tica.split_segments(ref_xyz, starts)
            except ValueError as err:
                raise SystemExit(f"{'--tica_stats' if tica_stats else '--kde_stats'}: {err}")
        if cov_stats:
            if not args.cov_thresholds or min(args.cov_thresholds) <= 0:
                raise SystemExit("--cov_stats: -cov_thresholds must be positive RMSDs in Angstrom")
            if coverage.select_atoms(z, args.cov_atoms).shape[0] == 0:
                raise SystemExit(f"--cov_stats: the topology has no {args.cov_atoms} atoms to superpose")
        if contact["contact_stats"]:
            if not contact["contact_cutoff"] > 0 or contact["contact_exclude"] < 0:
                raise SystemExit("--contact_stats: -contact_cutoff must be a positive distance in Angstrom, -contact_exclude >= 0")
            if coverage.select_atoms(z, contact["contact_atoms"]).shape[0] < 2:
                raise SystemExit(f"--contact_stats: the topology has fewer than two {contact['contact_atoms']} atoms")
            if contact["contact_groups"] == "residue":
                try:
                    contacts.groups_of(z, bonds, None, "residue")
                except ValueError as err:
                    raise SystemExit(f"--contact_stats: {err}")
        if flex["flex_stats"]:
            if coverage.select_atoms(z, flex["flex_atoms"]).shape[0] < 3:
                raise SystemExit(f"--flex_stats: the topology has fewer than three {flex['flex_atoms']} atoms: no rotation to fit")
            if flex["flex_groups"] == "residue":
                try:
                    contacts.groups_of(z, bonds, None, "residue")
                except ValueError as err:
                    raise SystemExit(f"--flex_stats: {err}")
        if kde["kde_stats"]:
            if kde["kde_grid"] < 2:
                raise SystemExit("--kde_stats: -kde_grid must be at least 2 nodes per axis")
            if ref_xyz.shape[0] < 4:
                raise SystemExit("--kde_stats needs at least four reference frames (its floor compares the even with the odd ones)")
            if kde["kde_plane"] == "torsion" and not distributions.peptide_backbone_torsions(z, bonds)[2]:
                raise SystemExit("--kde_stats: the topology has no peptide backbone, so no (phi, psi) plane")
    if params.get("cg_radius_graph") and bonds is None:
        raise SystemExit("the run was trained with --cg_radius_graph (bead graph from the bonds): pass a topology")
    return {"cg_xyz": cg, "z": z, "bonds": bonds, "mapping": mapping, **({"ref_xyz": ref_xyz} if need_ref else {}),
            **({"ref_starts": starts} if tica_stats or kde_tica else {})}


def _write_stats(out: str, stem: str, stats: dict) -> dict:
    """The full statistics of an analysis go to ``<stem>_stats.json`` next to ``-out``, their short form to the summary line."""
    with open(os.path.join(os.path.dirname(os.path.abspath(out)), stem + "_stats.json"), "w") as f:
        json.dump(stats, f)
    return BY_STEM[stem].module.summary_of(stats)


def run(args) -> dict:
    from . import ops
    from .data import _bond_cg_graph
    from .run_ala import _device
    params = read_params(args.model)
    device = _device(str(args.device))
    torch.cuda.set_device(device)
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    inp = read_inputs(args, params, device)
    model, params = load_run(args.model, device)
    mapping, z, bonds = inp["mapping"], inp["z"], inp["bonds"]
    radii = None
    if z is not None:
        try:
            ev.bond_radii(sorted(set(np.asarray(z).astype(np.int64).tolist())))
        except KeyError as err:
            if not params.get("synthetic"):
                raise SystemExit(err.args[0])
            # synthetic frames carry random type labels, not chemistry: as run_ala's evaluation, carbon's radius
            radii = {int(e): ev.COVALENT_RADII[6] for e in set(np.asarray(z).astype(np.int64).tolist()) if int(e) not in ev.COVALENT_RADII}
    cg_bonds = None
    if params.get("cg_radius_graph"):
        cg_bonds = _bond_cg_graph(torch.from_numpy(bonds), torch.from_numpy(mapping), mapping.shape[0], int(mapping.max()) + 1)
    ops.set_sample_rng_state(device, torch.tensor([ops.sample_seed(args.seed), 0, 0], dtype=torch.int64))
    kw = dict(z=z, bonds=bonds, frames_per_launch=args.frames_per_launch, cg_bonds=cg_bonds, radii=radii)
    torch.cuda.synchronize(device)
    t0 = time.time()
    if args.require_valid:
        res = backmap_valid(model, inp["cg_xyz"], mapping, args.n_samples, params["cg_cutoff"], which=args.require_valid,
                            max_rounds=args.max_rounds, **kw)
    else:
        res = backmap(model, inp["cg_xyz"], mapping, args.n_samples, params["cg_cutoff"], **kw)
    seconds = time.time() - t0
    keep = ["xyz", "cg_xyz", "valid_all", "valid_heavy", "counts", "diversity_all", "diversity_heavy", "n_valid"]
    if args.pair_rmsd:
        keep += ["pair_rmsd_all", "pair_rmsd_heavy"]
    arrays = {k: res[k] for k in keep if k in res}
    arrays.update(mapping=mapping, n_samples=np.int64(args.n_samples), seed=np.int64(args.seed))
    np.savez_compressed(args.out, **arrays)
    T, K = res["xyz"].shape[:2]
    dist = {}
    if args.dist_stats:
        stats = distributions.compare(inp["ref_xyz"], res["xyz"].reshape(T * K, -1, 3), z, bonds, device=device)
        dist["dist_stats"] = _write_stats(args.out, "dist", stats)
    if args.tica_stats:
        stats = tica.compare(tica.split_segments(inp["ref_xyz"], inp["ref_starts"]), res["xyz"].reshape(T * K, -1, 3), z, bonds,
                             lag=args.tica_lag, n_bins2=args.tica_bins, device=device)
        dist["tica_stats"] = _write_stats(args.out, "tica", stats)
    if args.cov_stats:
        stats = coverage.compare(inp["ref_xyz"], res["xyz"].reshape(T * K, -1, 3), z, thresholds=args.cov_thresholds,
                                 atoms=args.cov_atoms, device=device)
        dist["cov_stats"] = _write_stats(args.out, "cov", stats)
    contact = contact_args(args)
    if contact["contact_stats"]:
        stats = contacts.compare(inp["ref_xyz"], res["xyz"].reshape(T * K, -1, 3), z, bonds, atoms=contact["contact_atoms"],
                                 cutoff=contact["contact_cutoff"], exclude=contact["contact_exclude"],
                                 groups=None if contact["contact_groups"] == "none" else contact["contact_groups"],
                                 mapping=mapping, device=device)
        dist["contact_stats"] = _write_stats(args.out, "contact", stats)
    flex = flex_args(args)
    if flex["flex_stats"]:
        gen = res["xyz"].reshape(T * K, -1, 3)
        stats = flexibility.compare(inp["ref_xyz"], gen, z, bonds, atoms=flex["flex_atoms"],
                                    groups=None if flex["flex_groups"] == "none" else flex["flex_groups"], mapping=mapping,
                                    device=device)
        dist["flex_stats"] = _write_stats(args.out, "flex", stats)
        if flex["flex_aligned"]:
            sel = coverage.select_atoms(z, flex["flex_atoms"])
            own = flexibility.mean_structure(gen, sel, device=device)
            if own["mean"] is None:
                raise SystemExit("-flex_aligned: no output structure is finite, there is no mean to align to")
            np.savez_compressed(flex["flex_aligned"], xyz=flexibility.aligned(gen, own["mean"], sel, device=device), mean=own["mean"],
                                rmsf=own["rmsf"], atoms=sel.astype(np.int64))
    kde = kde_args(args)
    if kde["kde_stats"]:
        gen = res["xyz"].reshape(T * K, -1, 3)
        try:
            if kde["kde_plane"] == "torsion":
                stats = density.compare_torsions(inp["ref_xyz"], gen, z, bonds, n_grid=kde["kde_grid"], bandwidth=kde["kde_bw"], device=device)
            else:
                stats = density.compare_tica(tica.split_segments(inp["ref_xyz"], inp["ref_starts"]), gen, z, bonds, lag=args.tica_lag,
                                             n_grid=kde["kde_grid"], bandwidth=kde["kde_bw"], device=device)
        except ValueError as err:
            raise SystemExit(f"--kde_stats: {err}")
        dist["kde_stats"] = _write_stats(args.out, "kde", stats)

    def mean(key):
        if key not in res:
            return None
        v = np.asarray(res[key], dtype=np.float64)
        return float(np.nanmean(v)) if np.isfinite(v).any() else None
    return {"frames": int(T), "samples": int(T * K), "seconds": seconds, "samples_per_s": T * K / max(seconds, 1e-9),
            "valid_all_ratio": mean("valid_all"), "valid_heavy_ratio": mean("valid_heavy"),
            "diversity_all": mean("diversity_all"), "diversity_heavy": mean("diversity_heavy"), "out": args.out, **dist}


def main(argv=None):
    print(json.dumps(run(build_parser().parse_args(argv))))


if __name__ == "__main__":
    main(sys.argv[1:])
