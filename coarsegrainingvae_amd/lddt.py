"""How well every generated structure keeps the LOCAL geometry of the structure it should resemble, and whether its atoms
overlap: the local distance difference test (lDDT, Mariani et al. 2013) of every model structure against the reference
structure it is paired with, without superposition, per structure and per atom (or bead, or residue), and the steric
clashes of non-bonded atoms -- counted on the device for every pair and every structure (K28, ``cgv_lddt_counts``;
``csrc/lddt.hip``).

The other analyses compare the statistics of two SETS.  ``backmap -out`` writes K samples for each of T coarse-grained
frames, and for a test trajectory the all-atom frame every sample should resemble is known: this module scores each
sample against its own frame.  The superposed RMSD of ``evaluate`` is one scalar per sample, dominated by whatever loop
or terminus moves most; lDDT is local, needs no superposition and says which atoms are wrong.  Clashes -- two non-bonded
atoms closer than the sum of their radii less a tolerance -- pass every other analysis (``contacts`` counts them as
contacts).

Definition.  Over the selection ``sel [m]`` (default: the heavy atoms), for an unordered pair ``{i, j}``, ``i != j``, in
fp32 with every operation rounded on its own (``sqrtf`` correctly rounded):

    q0 = (dx*dx + dy*dy) + dz*dz  of ref_i - ref_j      q = the same of x_i - x_j          (csrc/sq_dist.h)
    included      iff  not excl_lddt  and  q0 < radius2            radius2 = fp32(R0) * fp32(R0), R0 = 15 by default
    e  = fabsf(sqrtf(q) - sqrtf(q0))                               one rounded subtraction
    preserved_k   iff  included and e < fp32(t_k)                  t = (0.5, 1, 2, 4) by default; four, ascending
    c  = (r_i + r_j) - fp32(tol)                                   tol = 0.4 by default; r: Bondi radii (``sasa.radii_of``)
    clash         iff  not excl_clash  and  c > 0  and  q < c * c

``excl_lddt``: the pairs of one group when group labels are given, else the pairs at most ``exclude`` bonds apart;
``excl_clash``: the pairs at most 3 bonds apart.  Every comparison is strict and false for a NaN.  The six quantities --
included, preserved at the four thresholds, clashes -- are counted per structure over the pairs ``i < j`` and per atom
over the pairs that contain it; a ``numpy.float32`` restatement reproduces every integer exactly, no floating-point
number leaves the device, and two calls give the same bits however the structures are cut into launches.  The lDDT of a
structure (an atom, a group) is the mean of its four preserved shares, computed on the host in fp64 from the integers.
A model structure with a non-finite selected coordinate, or scored against a reference that has one, is *bad*: its
per-structure values are ``-1`` and it enters no sum.

    python -m coarsegrainingvae_amd.lddt -gen samples.npz -ref traj.npz [-top top.npz] [-lddt_atoms heavy|all]
        [-lddt_groups none|bead|residue] [-lddt_radius 15] [-lddt_exclude 3] [-clash_tolerance 0.4] [-native FRAME]
        [-scores scores.npz] [-out lddt_stats.json]

``-gen``: the ``xyz [T, K, n, 3]`` that ``backmap -out`` writes, T the frames of ``-ref``: sample (t, k) is scored against
frame t.  With ``-native FRAME`` every structure of ``-gen`` (any shape) is scored against that one frame.  ``z`` and
``bonds`` (and ``mapping`` for ``-lddt_groups bead``) come from ``-top``, else from ``-ref``.  The full statistics of
``compare`` go to ``-out``, one JSON line with ``"lddt_stats": summary_of(...)`` to stdout; ``-scores`` takes the lDDT and
the clash count of every generated structure.
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .contacts import cutoff2_of, excluded_pairs
from .ensemble import check_sets, device_of, groups_of, read_back, scalar_block, select_atoms, structures
from .sasa import radii_of

QUANTITIES = ("included", "preserved_0", "preserved_1", "preserved_2", "preserved_3", "clashes")   # the six columns


def limits() -> Dict[str, int]:
    return ensemble.limits("lddt", ("structures", "references", "atoms"))


# ----------------------------------------------------------------------------- host: parameters, masks, pairing
def thresholds_of(thresholds) -> np.ndarray:
    """The four thresholds as the kernel takes them, fp32 ``[4]``; ``ValueError`` unless they are four finite lengths
    >= 0 in ascending order."""
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if t.shape[0] != 4:
        raise ValueError(f"four thresholds are needed, got {t.shape[0]}")
    t32 = t.astype(np.float32)
    if not np.isfinite(t32).all() or (t32 < 0).any():
        raise ValueError(f"a threshold must be a finite length >= 0, got {list(thresholds)}")
    if not (np.diff(t32) > 0).all():
        raise ValueError(f"the thresholds must be ascending, got {list(thresholds)}")
    return t32


def tolerance_of(tol: float) -> np.float32:
    t = np.float32(tol)
    if not np.isfinite(t) or t < 0:
        raise ValueError(f"the clash tolerance must be a finite length >= 0, got {tol}")
    return t


def same_group_pairs(labels) -> np.ndarray:
    """``[m, m]`` bool: True for ``i == j`` and for every pair of atoms with the same label."""
    g = np.asarray(labels).reshape(-1)
    return g[:, None] == g[None, :]


def default_ref_index(S: int, T: int) -> np.ndarray:
    """Which reference a model structure is scored against when the caller does not say: its own (``T == S``), the only
    one (``T == 1``), or ``s // (S // T)`` when ``T`` divides ``S`` -- the ``[T, K, ...]`` layout of ``backmap -out``
    flattened.  ``ValueError`` otherwise: it asks for ``ref_index``."""
    S, T = int(S), int(T)
    if T == S:
        return np.arange(S, dtype=np.int32)
    if T == 1:
        return np.zeros(S, dtype=np.int32)
    if T > 1 and S % T == 0:
        return (np.arange(S, dtype=np.int64) // (S // T)).astype(np.int32)
    raise ValueError(f"{S} structures cannot be paired with {T} references by their order: pass ref_index [S], the "
                     f"reference every structure is scored against")


def _square(mask, m: int, what: str) -> np.ndarray:
    a = np.asarray(mask)
    if a.dtype != np.bool_ or a.shape != (m, m):
        raise ValueError(f"{what} must be a bool array [{m}, {m}], got {a.dtype} {a.shape}")
    if not np.array_equal(a, a.T):
        raise ValueError(f"{what} must be symmetric")
    return a | np.eye(m, dtype=bool)


# ----------------------------------------------------------------------------- the launches
def count_pairs(xyz, ref_xyz, ref_index, sel, excl_lddt, excl_clash, radii, inclusion_radius: float = 15.0,
                thresholds=(0.5, 1, 2, 4), clash_tolerance: float = 0.4, structures_per_launch: int = 4096, device="cuda") -> dict:
    """The launches behind ``lddt_counts``, with every table the caller's own: ``sel [m]`` (unique atoms), the two
    SYMMETRIC bool masks ``[m, m]`` in the order of ``sel`` (the diagonal is added), ``radii [m]`` and ``ref_index [S]``.
    Returns the host arrays ``struct_counts [S,6]`` int64 (``-1`` for a bad structure), ``atom_counts [m,6]`` int64,
    ``bad [S]`` bool, ``n_good`` and the fp32 parameters the kernel took (``radius2``, ``t``, ``tol``)."""
    x, ref = structures(xyz), structures(ref_xyz)
    S, n, T = int(x.shape[0]), int(x.shape[1]), int(ref.shape[0])
    if int(ref.shape[1]) != n:
        raise ValueError(f"a model structure has {n} atoms, a reference structure {int(ref.shape[1])}")
    if S >= 2 ** 31:
        raise ValueError("fewer than 2^31 structures")
    radius2 = cutoff2_of(inclusion_radius)
    if not np.isfinite(radius2):
        raise ValueError(f"the inclusion radius must be a finite distance >= 0, got {inclusion_radius}")
    t, tol = thresholds_of(thresholds), tolerance_of(clash_tolerance)
    lim = limits()
    table = ensemble.selection(sel, n, purpose="score")
    m = int(table.shape[0])
    if m > lim["atoms"]:
        raise ValueError(f"the selection lists {m} atoms (the kernel holds {lim['atoms']})")
    ex_l, ex_c = _square(excl_lddt, m, "excl_lddt"), _square(excl_clash, m, "excl_clash")
    r32 = np.ascontiguousarray(np.asarray(radii, dtype=np.float32).reshape(-1))
    if r32.shape[0] != m or not np.isfinite(r32).all() or (r32 < 0).any():
        raise ValueError(f"radii must be {m} finite lengths >= 0")
    idx = np.asarray(ref_index).reshape(-1)
    if idx.shape[0] != S:
        raise ValueError(f"ref_index lists {idx.shape[0]} structures, there are {S}")
    idx = idx.astype(np.int64)
    if S and (idx.min() < 0 or idx.max() >= T):
        raise ValueError(f"ref_index names reference {int(idx.max() if idx.max() >= T else idx.min())}, there are {T}")
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(structures_per_launch, min(lim["structures"], lim["references"]), 32 * m)
    out = {"struct_counts": torch.zeros(S, 6, dtype=torch.int32, device=dev), "atom_counts": torch.zeros(m, 6, dtype=torch.int64, device=dev),
           "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if S:
        lib = _lib.load()
        d_sel = torch.from_numpy(table).to(dev)
        d_l, d_c = (torch.from_numpy(ensemble.pack_mask(e).view(np.int32)).to(dev) for e in (ex_l, ex_c))
        d_r = torch.from_numpy(r32).to(dev)
        k_most = min(M, S)
        need = int(lib.cgv_lddt_workspace_bytes(k_most, min(k_most, T), m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        named, d_ref = None, None
        for start, chunk in ensemble.chunks(x, M, dev):
            k = int(chunk.shape[0])
            uniq, local = np.unique(idx[start:start + k], return_inverse=True)     # only the references the chunk names
            if named is None or not np.array_equal(named, uniq):
                pick = torch.from_numpy(uniq).to(ref.device)
                named, d_ref = uniq, ref.index_select(0, pick).detach().to(dev, torch.float32).contiguous()
            local = np.ascontiguousarray(local.reshape(-1).astype(np.int32))
            _lib.call("cgv_lddt_counts", _lib.ptr(chunk), _lib.ptr(d_ref), local.ctypes.data, _lib.ptr(d_sel), _lib.ptr(d_l),
                      _lib.ptr(d_c), _lib.ptr(d_r), k, int(uniq.shape[0]), n, m, float(radius2), *(float(v) for v in t), float(tol),
                      _lib.ptr(out["struct_counts"][start:start + k]), _lib.ptr(out["atom_counts"]),
                      _lib.ptr(out["bad"][start:start + k]), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), tag="lddt_counts")
    sc, ac, bad = read_back([out["struct_counts"], out["atom_counts"], out["bad"]])
    return {"struct_counts": sc.astype(np.int64), "atom_counts": ac, "bad": bad.astype(bool), "n_good": int(S - int(bad.sum())),
            "radius2": radius2, "t": t, "tol": tol}


def lddt_counts(xyz, ref_xyz, z, bonds, ref_index=None, atoms="heavy", groups=None, exclude: int = 3, inclusion_radius: float = 15.0,
                thresholds=(0.5, 1, 2, 4), clash_tolerance: float = 0.4, radii=None, structures_per_launch: int = 4096,
                device="cuda") -> dict:
    """The lDDT and clash counts of the model structures ``xyz [S,n,3]`` against the reference structures
    ``ref_xyz [T,n,3]`` (host arrays, or tensors on any device -- a device tensor of models decides the device) of the
    molecule ``z [n]`` / ``bonds [Eb,2]`` over ``select_atoms(z, atoms)``.  ``ref_index [S]``: the reference of every
    structure (default: ``default_ref_index``).  ``groups``: a label for every atom of the molecule, ``[n]``
    (``ensemble.groups_of``); pairs of one group are then left out of the distance test, otherwise pairs at most
    ``exclude`` bonds apart are.  Clashes never count pairs at most 3 bonds apart.  ``radii``: ``{z: R}`` on top of the
    Bondi table (``sasa.radii_of``), or an array ``[m]`` for the selected atoms.  Host arrays:

      struct_counts [S,6] int64  per structure over the pairs i < j: included, preserved at the four thresholds, clashes
                                 (-1: bad structure)
      atom_counts [m,6] int64    the same per selected atom over the pairs that contain it, summed over the good structures
      bad [S] bool, n_good       structures that are not bad
      sel [m], ref_index [S]     the selection and the pairing used
      excl_lddt, excl_clash [m,m] bool, radii [m] fp32     the tables used
      inclusion_radius, thresholds, clash_tolerance, exclude, and radius2, t, tol: what the kernel took for them (fp32)

    The structures go through in launches of ``structures_per_launch``, each with only the references it names; the sums
    stay on the device; ONE read-back.  Everything that can be refused is a ``ValueError`` before any launch."""
    x, ref = structures(xyz), structures(ref_xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    if zz.shape[0] != n or int(ref.shape[1]) != n:
        raise ValueError(f"z lists {zz.shape[0]} atoms, the structures have {n} and {int(ref.shape[1])}")
    idx = default_ref_index(S, int(ref.shape[0])) if ref_index is None else np.asarray(ref_index).reshape(-1)
    sel = select_atoms(zz, atoms)
    table = ensemble.selection(sel, n, purpose="score")
    m = int(table.shape[0])
    if m > limits()["atoms"]:
        raise ValueError(f"the selection lists {m} atoms (the kernel holds {limits()['atoms']})")
    if groups is not None:
        g = np.asarray(groups).reshape(-1)
        if g.shape[0] != n:
            raise ValueError(f"groups lists {g.shape[0]} atoms, z has {n}")
        ex_l = same_group_pairs(g[table])
    else:
        ex_l = excluded_pairs(bonds, n, table, exclude)
    ex_c = excluded_pairs(bonds, n, table, 3)
    if radii is None or isinstance(radii, dict):
        r = radii_of(zz, table, radii).astype(np.float32)
    else:
        r = np.asarray(radii, dtype=np.float32).reshape(-1)
    res = count_pairs(x, ref, idx, table, ex_l, ex_c, r, inclusion_radius, thresholds, clash_tolerance, structures_per_launch, device)
    res.update(sel=table, ref_index=np.asarray(idx, dtype=np.int64), excl_lddt=ex_l, excl_clash=ex_c, radii=r,
               inclusion_radius=float(inclusion_radius), thresholds=[float(v) for v in thresholds],
               clash_tolerance=float(clash_tolerance), exclude=int(exclude))
    return res


# ----------------------------------------------------------------------------- host statistics
def _share(preserved: np.ndarray, included: np.ndarray) -> np.ndarray:
    """The mean of the four preserved shares ``[..., 4] / [...]`` in fp64; NaN where nothing is included."""
    inc = np.asarray(included, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inc > 0, np.asarray(preserved, dtype=np.float64).sum(-1) / (4.0 * inc), np.nan)


def scores(res: dict) -> dict:
    """Per structure, from the integers: ``lddt [S]`` fp64 (NaN for a bad structure and where no pair is included),
    ``n_clashes [S]`` int64 (-1: bad) and ``clashes_per_1000_atoms [S]`` fp64 (NaN: bad)."""
    sc = np.asarray(res["struct_counts"], dtype=np.int64).reshape(-1, 6)
    bad = np.asarray(res["bad"], dtype=bool)
    m = int(np.asarray(res["atom_counts"]).shape[0])
    lddt = np.where(bad, np.nan, _share(sc[:, 1:5], np.where(bad, 0, sc[:, 0])))
    n_clashes = np.where(bad, -1, sc[:, 5])
    return {"lddt": lddt, "n_clashes": n_clashes, "clashes_per_1000_atoms": np.where(bad, np.nan, 1000.0 * sc[:, 5] / max(m, 1))}


def profile(res: dict, groups=None) -> dict:
    """Per selected atom -- or, with ``groups`` (a label for every atom of the molecule, ``ensemble.groups_of``), per
    group, the integer counts of its atoms summed -- over the good structures: ``labels [P]`` (atom indices or group
    labels, ascending for groups), ``lddt [P]`` fp64 (NaN where nothing is included), ``included [P]`` and ``clashes [P]``
    int64 (clashing pairs that contain the atom; a pair inside a group counts twice there)."""
    ac = np.asarray(res["atom_counts"], dtype=np.int64).reshape(-1, 6)
    sel = np.asarray(res["sel"], dtype=np.int64).reshape(-1)
    labels = sel
    if groups is not None:
        g = np.asarray(groups).reshape(-1)
        if sel.shape[0] and int(sel.max()) >= g.shape[0]:
            raise ValueError(f"groups lists {g.shape[0]} atoms, the selection names atom {int(sel.max())}")
        labels, dense = np.unique(g[sel], return_inverse=True)
        summed = np.zeros((labels.shape[0], 6), dtype=np.int64)
        np.add.at(summed, dense.reshape(-1), ac)
        ac = summed
    return {"labels": labels, "lddt": _share(ac[:, 1:5], ac[:, 0]), "included": ac[:, 0], "clashes": ac[:, 5]}


def _opt(v):
    return None if v is None or not np.isfinite(v) else float(v)


def _moments3(v: np.ndarray) -> Optional[dict]:
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return {"mean": float(v.mean()), "std": float(v.std()), "min": float(v.min())} if v.size else None


def compare_from_counts(even: dict, odd: dict, gen: dict, neighbour: Optional[dict] = None, groups=None,
                        params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from results of ``lddt_counts`` -- the even reference frames and the odd ones, each
    against themselves, the generated structures against their references, and (``neighbour``) the odd frames against
    the even frame before them -- pure host.  ``groups``: a label for every atom of the molecule, for the profile.  Bad
    structures are in no denominator.  Keys: ``LDDT_STATS_KEYS``; see ``compare``."""
    sg = scores(gen)
    ok = np.isfinite(sg["lddt"])
    block = ensemble.hist(sg["lddt"][ok], 0.0, 1.0, 50)
    m3 = _moments3(sg["lddt"])
    prof = profile(gen, groups)
    order = [int(k) for k in np.argsort(np.where(np.isfinite(prof["lddt"]), prof["lddt"], np.inf), kind="stable")
             if np.isfinite(prof["lddt"][k])][:5]
    good = ~np.asarray(gen["bad"], dtype=bool)
    tot = np.asarray(gen["struct_counts"], dtype=np.int64).reshape(-1, 6)[good].sum(0)
    preserved = [float(tot[1 + k]) / float(tot[0]) if tot[0] > 0 else None for k in range(4)]

    def clashes(res):
        return np.asarray(res["struct_counts"], dtype=np.float64).reshape(-1, 6)[~np.asarray(res["bad"], dtype=bool), 5]
    ce, co, cg = clashes(even), clashes(odd), clashes(gen)
    cblock = None
    if ce.size + co.size and cg.size:                           # one bin per integer, up to the most clashes either set has
        top = int(max(np.concatenate([ce, co]).max(), cg.max()))
        cblock = scalar_block(ce, co, cg, -0.5, top + 0.5, top + 1)

    def per_atom(*rs):
        n_good = sum(r["n_good"] for r in rs)
        tab = sum(np.asarray(r["atom_counts"], dtype=np.int64).reshape(-1, 6)[:, 5] for r in rs)
        return None if n_good <= 0 else (tab / float(n_good)).tolist()
    return {**ensemble.set_sizes(even, odd, gen), "params": dict(params or {}), "n_atoms": int(np.asarray(gen["sel"]).shape[0]),
            "lddt": None if m3 is None else {**m3, "range": [0.0, 1.0], "hist": block},
            "lddt_profile": {"labels": [int(v) for v in prof["labels"]], "lddt": [_opt(v) for v in prof["lddt"]],
                             "included": [int(v) for v in prof["included"]], "clashes": [int(v) for v in prof["clashes"]]},
            "worst": [{"label": int(prof["labels"][k]), "lddt": float(prof["lddt"][k])} for k in order],
            "preserved": preserved, "clashes": cblock,
            "clashing_pairs_per_atom": {"labels": [int(v) for v in np.asarray(gen["sel"]).reshape(-1)], "ref": per_atom(even, odd),
                                        "gen": per_atom(gen)},
            "floor": {"lddt_neighbour": None if neighbour is None else _moments3(scores(neighbour)["lddt"]),
                      "clashes_jsd": cblock["floor"] if cblock else None}}


def compare(ref_xyz, gen_xyz, z, bonds, ref_index=None, atoms="heavy", groups=None, exclude: int = 3, inclusion_radius: float = 15.0,
            thresholds=(0.5, 1, 2, 4), clash_tolerance: float = 0.4, radii=None, mapping=None, structures_per_launch: int = 4096,
            device="cuda") -> dict:
    """Generated structures ``gen_xyz [S,n,3]`` against the reference frames ``ref_xyz [T,n,3]`` (at least two) they should
    resemble: ``[T*K,n,3]`` in the order of ``backmap -out`` flattened, or any ``S`` with ``ref_index [S]``
    (``default_ref_index``).  ``groups``: ``None`` (a profile per atom; the distance test leaves out pairs at most
    ``exclude`` bonds apart), ``"bead"`` (needs ``mapping``) or ``"residue"`` (``ensemble.groups_of``; the distance test
    leaves out the pairs of one group).  The reference's own clashes are counted from ``lddt_counts(ref, ref)``, its even
    and odd frames apart: what the halves differ by is the floor of ``clashes.jsd``, and their lDDT must be exactly 1.
    Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      params      atoms (the selection), groups, exclude, inclusion_radius, thresholds, clash_tolerance
      n_atoms     selected atoms
      lddt        {mean, std, min, range, hist ({counts [50], under, over})} of the per-structure score on [0, 1]; ``None``
                  when no structure has a score
      lddt_profile  {labels, lddt, included, clashes} per atom or group (``profile``; ``None`` for an empty denominator)
      worst       the five atoms or groups of lowest lDDT: {label, lddt}
      preserved   the four shares over all good structures (``None``: nothing included)
      clashes     {range, hist_ref, hist_gen, jsd, floor, mean_ref, std_ref, mean_gen, std_gen} of the clashes of a
                  structure, one bin per integer; ``None`` where a set has no good structure
      clashing_pairs_per_atom   {labels, ref, gen}: per selected atom the clashing pairs that contain it, per good structure
      floor       {lddt_neighbour: {mean, std, min} of every odd reference frame scored against the even frame before it --
                  what ordinary motion between consecutive frames already costs, and what every generated score is to be
                  read against --, clashes_jsd}
    """
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z, groups=groups)
    idx = default_ref_index(int(gen.shape[0]), int(ref.shape[0])) if ref_index is None else ref_index
    labels = None if groups is None else groups_of(z, bonds, mapping, groups)
    kw = dict(atoms=atoms, groups=labels, exclude=exclude, inclusion_radius=inclusion_radius, thresholds=thresholds,
              clash_tolerance=clash_tolerance, radii=radii, structures_per_launch=structures_per_launch, device=device)
    halves = ref[0::2], ref[1::2]
    even, odd = (lddt_counts(h, h, z, bonds, **kw) for h in halves)
    for half in (even, odd):
        own = scores(half)["lddt"]
        assert bool(np.all(own[np.isfinite(own)] == 1.0)), "a structure scored against itself must have an lDDT of exactly 1"
    got = lddt_counts(gen, ref, z, bonds, ref_index=idx, **kw)
    n_odd = int(halves[1].shape[0])
    neighbour = lddt_counts(halves[1], halves[0][:n_odd], z, bonds, ref_index=np.arange(n_odd), **kw)
    params = {"atoms": [int(i) for i in got["sel"]], "groups": groups, "exclude": int(exclude), "inclusion_radius": float(inclusion_radius),
              "thresholds": [float(v) for v in thresholds], "clash_tolerance": float(clash_tolerance)}
    return compare_from_counts(even, odd, got, neighbour=neighbour, groups=labels, params=params)


LDDT_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "n_atoms", "lddt", "lddt_profile", "worst", "preserved",
                   "clashes", "clashing_pairs_per_atom", "floor")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"lddt_stats"`` in its JSON summary line: no profile, no histograms."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_atoms", "worst", "preserved", "floor")}
    short["lddt"] = None if stats["lddt"] is None else {k: stats["lddt"][k] for k in ("mean", "std", "min")}
    short["clashes"] = ensemble.short_block(stats["clashes"])
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.lddt",
                                "lDDT and steric clashes of generated structures against the frames they should resemble",
                                top_help="npz with z and bonds (and mapping for -lddt_groups bead); default: those of -ref")
    p.add_argument("-lddt_atoms", choices=("heavy", "all"), default="heavy", help="the atoms scored (heavy)")
    p.add_argument("-lddt_groups", choices=("none", "bead", "residue"), default="none",
                   help="profile per atom, bead or residue; with groups the distance test leaves out pairs of one group (none)")
    p.add_argument("-lddt_radius", type=float, default=15.0, help="inclusion radius in the reference in Angstrom (15)")
    p.add_argument("-lddt_exclude", type=int, default=3, help="without groups: pairs at most this many bonds apart are left out (3)")
    p.add_argument("-clash_tolerance", type=float, default=0.4, help="overlap allowed before a pair clashes, in Angstrom (0.4)")
    p.add_argument("-native", type=int, default=None, metavar="FRAME", help="score every structure against this one frame of -ref")
    p.add_argument("-scores", default=None, help="npz that takes the lDDT and the clash count of every generated structure (not written)")
    return compare_cli.finish_parser(p, "lddt_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, ``ref_index``, ``groups``, ``mapping``, with
    everything that can be refused without a device refused here (``SystemExit``)."""
    if not (math.isfinite(args.lddt_radius) and args.lddt_radius >= 0):
        raise SystemExit("-lddt_radius must be a finite length >= 0 in Angstrom")
    if args.lddt_exclude < 0:
        raise SystemExit("-lddt_exclude must be >= 0")
    if not (math.isfinite(args.clash_tolerance) and args.clash_tolerance >= 0):
        raise SystemExit("-clash_tolerance must be a finite length >= 0 in Angstrom")
    groups = None if args.lddt_groups == "none" else args.lddt_groups
    need = ("z", "bonds", "mapping") if groups == "bead" else ("z", "bonds")
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args, need)
    shape = compare_cli.read_npz(args.gen, ["xyz"])["xyz"].shape       # read_sets flattens: the pairing needs [T, K]
    T, S = int(ref_xyz.shape[0]), int(gen_xyz.shape[0])
    if args.native is not None:
        if not 0 <= args.native < T:
            raise SystemExit(f"-native {args.native}: {args.ref} has frames 0 .. {T - 1}")
        ref_index = np.full(S, args.native, dtype=np.int32)
    elif len(shape) == 4 and int(shape[0]) == T:
        ref_index = default_ref_index(S, T)
    else:
        raise SystemExit(f"{args.gen}: xyz is {tuple(shape)}: paired scoring needs [T, K, n, 3] with T = {T}, the frames of "
                         f"{args.ref}; or pass -native FRAME to score every structure against one frame")
    bonds = np.asarray(top["bonds"])
    mapping = np.asarray(top["mapping"]) if groups == "bead" else None
    with compare_cli.refusing():
        m = int(select_atoms(z, args.lddt_atoms).shape[0])
        if m == 0:
            raise ValueError("the selection is empty (m = 0): no atoms to score")
        if m > limits()["atoms"]:
            raise ValueError(f"the selection lists {m} atoms (the kernel holds {limits()['atoms']})")
        if groups is not None:
            groups_of(z, bonds, mapping, groups)
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": bonds, "ref_index": ref_index, "groups": groups, "mapping": mapping}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    kw = dict(atoms=args.lddt_atoms, exclude=args.lddt_exclude, inclusion_radius=args.lddt_radius, clash_tolerance=args.clash_tolerance,
              device=args.device)
    with compare_cli.refusing():
        stats = compare(inp["ref_xyz"], inp["gen_xyz"], inp["z"], inp["bonds"], ref_index=inp["ref_index"], groups=inp["groups"],
                        mapping=inp["mapping"], **kw)
        if args.scores:
            labels = None if inp["groups"] is None else groups_of(inp["z"], inp["bonds"], inp["mapping"], inp["groups"])
            res = lddt_counts(inp["gen_xyz"], inp["ref_xyz"], inp["z"], inp["bonds"], ref_index=inp["ref_index"], groups=labels, **kw)
            sc = scores(res)
            np.savez(args.scores, lddt=sc["lddt"], n_clashes=sc["n_clashes"], bad=res["bad"], ref_index=res["ref_index"],
                     struct_counts=res["struct_counts"])
    compare_cli.finish("lddt", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
