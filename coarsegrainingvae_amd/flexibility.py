"""Does an ensemble move as much as the data does?  The mean structure of a set of structures and the fluctuation of
every atom about it (RMSF), computed on the device: every structure is superposed onto a target over a selection of atoms
and its aligned coordinates are accumulated (K21, ``cgv_align_accumulate``; ``csrc/align_mean.hip``).

Nothing in the reference superposes anything, and neither ``evaluate`` (the bond graph), ``distributions`` (bonds, angles,
torsions), ``tica`` (slow collective coordinates), ``coverage`` (whole-structure RMSD: it needs the largest eigenvalue of
the key matrix, never the rotation) nor ``contacts`` (packing) can tell a decoder whose samples collapse towards the mean
-- half as flexible as the simulation in its loops and side chains -- from one that moves as the data does.

``mean_structure`` is generalised Procrustes: superpose everything onto a target, average, make the average the new
target, until the target stops moving.  ``rmsf[i]`` is the root of the mean squared distance of atom ``i`` from its mean
position after superposition over the selection.  A structure with ANY non-finite coordinate is *bad*: it enters no sum,
its RMSD is NaN.

What the number does not mean: for an ensemble with several distinct states the mean structure is a chimera that no
structure resembles, and RMSF measures the spread BETWEEN the states as much as the motion inside them.  That spread is
still comparable between data and model -- the same chimera, the same spread, when the model populates the states as the
data does -- and ``coverage`` and ``tica`` are what tells the states apart.  RMSF also depends on the selection the
superposition is fitted on: compare profiles only for the same selection.

The host pieces shared with the other analyses (``selection``, ``groups_of``, ``scalar_block``, ...) live in ``ensemble``.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, ensemble, options
from .steploop import forced_form
from .coverage import rmsd_matrix
from .ensemble import check_sets, device_of, groups_of, read_back, scalar_block, select_atoms, structures

WORKSPACE_BYTES = 1 << 28              # structures_per_launch is lowered until the partial sums of a launch fit this


def limits() -> Dict[str, int]:
    return ensemble.limits("align")


def _form(n_atoms: int) -> int:
    """The form ``cgv_align_accumulate`` is asked for: option ``align_form`` (0 the library's rule, 1 a wave per
    structure, 2 a block per structure); forcing the wave form on a structure it does not hold is an error."""
    form = forced_form("align_form", lambda: int(options.get("align_form")))     # 0: the library applies its own rule
    if form not in (0, 1, 2):
        raise ValueError("option align_form must be 0 (rule), 1 (wave) or 2 (block)")
    if form == 1 and not _lib.load().cgv_align_wave_fits(int(n_atoms)):
        raise ValueError(f"option align_form = 1: a wave does not hold {n_atoms} atoms")
    return form


def new_state(n_atoms: int, device) -> Dict[str, torch.Tensor]:
    """Zeroed accumulators as ``cgv_align_accumulate`` merges into them."""
    return {"sum": torch.zeros(n_atoms, 3, dtype=torch.float64, device=device),
            "dev2": torch.zeros(n_atoms, dtype=torch.float64, device=device),
            "n_good": torch.zeros(1, dtype=torch.int32, device=device)}


def align_accumulate(xyz: torch.Tensor, sel: torch.Tensor, ref: torch.Tensor, sum: torch.Tensor, dev2: torch.Tensor,  # noqa: A002
                     n_good: torch.Tensor, rmsd2: torch.Tensor, bad: torch.Tensor, aligned: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None) -> None:
    """One ``cgv_align_accumulate`` call on device tensors: ``xyz [S,n,3]`` fp32, ``sel [m]`` int32, ``ref [n,3]`` fp64.
    ``sum [n,3]``, ``dev2 [n]`` (fp64) and ``n_good [1]`` (int32) are ADDED to; ``rmsd2 [S]`` fp64 (squared), ``bad [S]``
    int32 and ``aligned [S,n,3]`` fp32 (optional) are overwritten.  Shapes, dtypes and limits are checked before the
    launch; the CONTENTS of ``sel`` are the caller's to check (``mean_structure`` does)."""
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz must be [S, n, 3], got {tuple(xyz.shape)}")
    S, n, m = int(xyz.shape[0]), int(xyz.shape[1]), int(sel.numel())
    if xyz.dtype != torch.float32 or sel.dtype != torch.int32 or ref.dtype != torch.float64:
        raise ValueError("xyz must be float32, sel int32, ref float64")
    lim = limits()
    if n < 1 or n > lim["atoms"]:
        raise ValueError(f"{n} atoms per structure (the kernel holds 1..{lim['atoms']})")
    if S > lim["structures"]:
        raise ValueError(f"{S} structures (a launch holds {lim['structures']})")
    if sel.dim() != 1 or not 1 <= m <= n:
        raise ValueError(f"the selection must list 1..{n} atoms, it lists {m}")
    if tuple(ref.shape) != (n, 3):
        raise ValueError(f"ref must be [{n}, 3], got {tuple(ref.shape)}")
    for t, shape, dt, what in ((sum, (n, 3), torch.float64, "sum [n,3] float64"), (dev2, (n,), torch.float64, "dev2 [n] float64"),
                               (n_good, (1,), torch.int32, "n_good [1] int32"), (rmsd2, (S,), torch.float64, "rmsd2 [S] float64"),
                               (bad, (S,), torch.int32, "bad [S] int32")):
        if tuple(t.shape) != shape or t.dtype != dt:
            raise ValueError(f"{what}: got {t.dtype} {tuple(t.shape)}")
    if aligned is not None and (tuple(aligned.shape) != (S, n, 3) or aligned.dtype != torch.float32):
        raise ValueError("aligned must be [S, n, 3] float32")
    form = _form(n)
    if S == 0:
        return
    need = int(_lib.load().cgv_align_workspace_bytes(S, n, form))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = ensemble.workspace(need, xyz.device)
    _lib.call("cgv_align_accumulate", _lib.ptr(xyz), _lib.ptr(sel), _lib.ptr(ref), S, n, m, form, _lib.ptr(sum), _lib.ptr(dev2),
              _lib.ptr(n_good), _lib.ptr(rmsd2), _lib.ptr(bad), _lib.ptr(aligned), _lib.ptr(workspace),
              workspace.numel() * workspace.element_size(), _lib.stream_ptr(), tag="align_accumulate")


class _Passes:
    """The structures of one set on the device, cut into launches, and the buffers every pass reuses."""

    def __init__(self, xyz, sel, structures_per_launch, device):
        x = structures(xyz)
        self.S, self.n = int(x.shape[0]), int(x.shape[1])
        lim = limits()
        if self.n < 1 or self.n > lim["atoms"]:
            raise ValueError(f"{self.n} atoms per structure (the kernel holds 1..{lim['atoms']})")
        if self.S >= 2 ** 31:
            raise ValueError("n_good is int32: fewer than 2^31 structures")
        self.table = ensemble.selection(sel, self.n, purpose="superpose", at_least=3)
        self.form = _form(self.n)
        self.dev = device_of(x, device)
        if int(structures_per_launch) < 1:
            raise ValueError("structures_per_launch must be at least 1")
        self.M = max(1, min(int(structures_per_launch), lim["structures"]))
        lib = _lib.load()
        while self.M > 64 and int(lib.cgv_align_workspace_bytes(self.M, self.n, self.form)) > WORKSPACE_BYTES:
            self.M //= 2
        self.x = x.detach().to(self.dev, torch.float32).contiguous()
        self.sel = torch.from_numpy(self.table).to(self.dev)
        self.sel64 = self.sel.long()
        need = int(lib.cgv_align_workspace_bytes(min(self.M, max(self.S, 1)), self.n, self.form))
        self.ws = ensemble.workspace(need, self.dev)
        self.rmsd2 = torch.zeros(self.S, dtype=torch.float64, device=self.dev)
        self.bad = torch.zeros(self.S, dtype=torch.int32, device=self.dev)

    def run(self, target: torch.Tensor, aligned: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """One pass over all structures against ``target [n,3]`` fp64: the accumulators, on the device."""
        state = new_state(self.n, self.dev)
        for start in range(0, self.S, self.M):
            stop = min(start + self.M, self.S)
            align_accumulate(self.x[start:stop], self.sel, target, state["sum"], state["dev2"], state["n_good"],
                             self.rmsd2[start:stop], self.bad[start:stop], None if aligned is None else aligned[start:stop],
                             workspace=self.ws)
        return state

    def centred(self, target: torch.Tensor) -> torch.Tensor:
        return target - target[self.sel64].mean(0, keepdim=True)


def mean_structure(xyz, sel=None, max_iter: int = 10, tol: float = 1e-4, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Generalised Procrustes of the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device
    tensor decides the device) over the atoms ``sel [m]`` (at least three, no atom twice; default: all).

    The target starts as the first good structure.  One pass superposes every structure onto the target (both centred
    on the centroid of their selected atoms) and averages: the new target is ``sum / n_good``.  The passes stop when the
    target's root-mean-square move over the selection is below ``tol`` Angstrom, or after ``max_iter`` of them; one more
    pass is then made against the last mean, and it is what everything returned comes from.  Host arrays:

      mean        [n,3] fp64, the average of that last pass, its selected atoms' centroid at the origin
      rmsf        [n] fp64  sqrt(max(0, dev2 / n_good - |mean - target|^2)): about the mean, not about the target
      rmsd        [S] fp64 superposed RMSD over the selection to the target of the last pass (NaN: bad structure)
      bad         [S] bool;  n_good
      iterations  passes made, the last one included (rigid copies of one structure: 2)
      converged   whether the move fell below ``tol``;  last_move  the last move measured, Angstrom

    ``mean`` and ``rmsf`` are ``None`` when no structure is good.  The order of every addition is fixed: the same call
    gives the same bits.  ONE read-back at the end, and one scalar per pass (the move).  Limits (``limits()``) and bad
    arguments are refused before any launch."""
    if int(max_iter) < 1 or not float(tol) >= 0:
        raise ValueError("max_iter must be at least 1 and tol a number >= 0")
    p = _Passes(xyz, sel, structures_per_launch, device)
    S = p.S
    firsts = torch.nonzero(torch.isfinite(p.x.reshape(S, -1)).all(1)).reshape(-1)[:1].tolist() if S else []
    first = firsts[0] if firsts else -1
    if first < 0:
        return {"mean": None, "rmsf": None, "rmsd": np.full(S, np.nan), "bad": np.ones(S, dtype=bool), "n_good": 0,
                "iterations": 0, "converged": False, "last_move": None}
    target = p.x[first].double()
    passes, converged, move = 0, False, None
    for _ in range(int(max_iter)):
        state = p.run(target)
        new = state["sum"] / state["n_good"].double()
        d = (new - p.centred(target))[p.sel64]
        move = float(torch.sqrt((d * d).sum(1).mean()))       # the one scalar read of the pass
        passes, target = passes + 1, new
        if move < float(tol):
            converged = True
            break
    state = p.run(target)
    mean = state["sum"] / state["n_good"].double()
    shift = mean - p.centred(target)
    msf = torch.clamp(state["dev2"] / state["n_good"].double() - (shift * shift).sum(1), min=0.0)
    mean_h, msf_h, rmsd2, bad, good = read_back([mean, msf, p.rmsd2, p.bad, state["n_good"]])
    return {"mean": mean_h, "rmsf": np.sqrt(msf_h), "rmsd": np.sqrt(rmsd2), "bad": bad.astype(bool), "n_good": int(good[0]),
            "iterations": passes + 1, "converged": converged, "last_move": move}


def aligned(xyz, mean, sel=None, structures_per_launch: int = 4096, device="cuda") -> np.ndarray:
    """The structures ``xyz [S,n,3]`` superposed onto ``mean [n,3]`` over ``sel`` -- every atom rotated, in the frame in
    which the mean's selected atoms have their centroid at the origin -- as a host array ``[S,n,3]`` fp32 (NaN rows: bad
    structures).  One pass, one read-back."""
    p = _Passes(xyz, sel, structures_per_launch, device)
    target = torch.as_tensor(np.ascontiguousarray(np.asarray(mean, dtype=np.float64))).to(p.dev)
    if tuple(target.shape) != (p.n, 3):
        raise ValueError(f"mean must be [{p.n}, 3], got {tuple(target.shape)}")
    out = torch.empty(p.S, p.n, 3, dtype=torch.float32, device=p.dev)
    p.run(target, aligned=out)
    return read_back([out])[0]


# ----------------------------------------------------------------------------- host statistics
def group_rows(sel, labels=None):
    """``(rows, dense)``: what a row of a profile over the selection ``sel`` is -- without ``labels`` the atom indices
    (``dense`` is ``None``), with ``labels [m]`` (a group per selected atom) the labels in ascending order and, per
    selected atom, the row of its group."""
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    if labels is None:
        return [int(i) for i in sel], None
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    if lab.shape[0] != sel.shape[0]:
        raise ValueError(f"labels lists {lab.shape[0]} atoms, the selection {sel.shape[0]}")
    ids, dense = np.unique(lab, return_inverse=True)
    return [int(i) for i in ids], dense


def group_profile(rmsf, sel, labels=None):
    """``(rows, profile)``: without ``labels`` the RMSF of the selected atoms, rows = their indices; with ``labels [m]``
    (a group per selected atom) per group the root of the mean of its atoms' mean-square fluctuations, rows = the labels
    in ascending order (``group_rows``)."""
    rows, dense = group_rows(sel, labels)
    r = np.asarray(rmsf, dtype=np.float64)[np.asarray(sel, dtype=np.int64).reshape(-1)]
    if dense is None:
        return rows, r
    msf = np.bincount(dense, weights=r * r, minlength=len(rows)) / np.bincount(dense, minlength=len(rows))
    return rows, np.sqrt(msf)


def _profile_stats(a, b) -> dict:
    """Two profiles over the same rows: correlation (``None`` when one of them is constant), RMS difference, ratio of
    the means (``None`` when the first one's is zero)."""
    if a is None or b is None:
        return {"pearson": None, "profile_rmse": None, "ratio": None}
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    da, db = a - a.mean(), b - b.mean()
    norm = float(np.sqrt((da * da).sum() * (db * db).sum()))
    return {"pearson": float((da * db).sum() / norm) if norm > 0 else None,
            "profile_rmse": float(np.sqrt(np.mean((a - b) ** 2))),
            "ratio": float(b.mean() / a.mean()) if a.mean() > 0 else None}


def _mean_rmsd(a: dict, b: dict, sel, device) -> Optional[float]:
    if a["mean"] is None or b["mean"] is None:
        return None
    return float(rmsd_matrix(a["mean"][None].astype(np.float32), b["mean"][None].astype(np.float32), sel, device=device)[0, 0])


def compare(ref_xyz, gen_xyz, z, bonds, atoms="heavy", groups=None, mapping=None, n_bins: int = 20, max_iter: int = 10,
            tol: float = 1e-4, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) of the
    molecule ``z [n]`` / ``bonds [Eb,2]`` by their flexibility: each set is superposed about ITS OWN mean structure over
    ``select_atoms(z, atoms)`` (at least three atoms) and the RMSF profiles are compared.  ``groups``: ``None`` (a row per
    selected atom), ``"bead"`` (needs ``mapping``) or ``"residue"`` (``ensemble.groups_of``): a row per group, the root of
    the mean of its selected atoms' mean-square fluctuations.  The convention of ``distributions.compare`` and
    ``contacts.compare``: the even and the odd reference frames are also analysed apart, and what the two halves differ
    by is the ``floor`` every deviation is to be read against.  Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen   structures, and those left out as bad
      params        atoms (the selection), groups, n_bins, max_iter, tol
      labels        [P] the atom index or group label of a profile row
      rmsf_ref, rmsf_gen   [P] Angstrom (``None``: no good structure in the set)
      pearson, profile_rmse, ratio   correlation and RMS difference of the two profiles, mean RMSF of the generated set
                    over the reference's (below 1: the model moves less than the data)
      mean_rmsd     superposed RMSD between the two mean structures over the selection (``coverage.rmsd_matrix``)
      rmsd_to_mean  {range, hist_ref, hist_gen ({counts [n_bins], under, over}), jsd, floor, mean_ref, std_ref, mean_gen,
                    std_gen} of every structure's RMSD to its own set's mean, on [0, 1.2 x the reference's largest]
      floor         {pearson, profile_rmse, ratio, mean_rmsd} between the even and the odd reference frames
      convergence   {ref, gen, even, odd}: {iterations, converged, last_move} of each ``mean_structure``
      top_atoms     the ten rows of largest |rmsf_gen - rmsf_ref|: {label, rmsf_ref, rmsf_gen}
    """
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z, groups=groups)
    sel = select_atoms(z, atoms)
    ensemble.selection(sel, z.shape[0], purpose="superpose", at_least=3)
    glab = None if groups is None else groups_of(z, bonds, mapping, groups)[sel]
    kw = dict(sel=sel, max_iter=max_iter, tol=tol, structures_per_launch=structures_per_launch, device=device)
    runs = {"ref": mean_structure(ref, **kw), "gen": mean_structure(gen, **kw),
            "even": mean_structure(ref[0::2], **kw), "odd": mean_structure(ref[1::2], **kw)}
    params = {"atoms": [int(i) for i in sel], "groups": groups, "max_iter": int(max_iter), "tol": float(tol)}
    return compare_from_runs(runs, sel, glab, mean_rmsd=_mean_rmsd(runs["ref"], runs["gen"], sel, device),
                             floor_mean_rmsd=_mean_rmsd(runs["even"], runs["odd"], sel, device), n_bins=n_bins, params=params)


def compare_from_runs(runs: dict, sel, group_labels=None, mean_rmsd=None, floor_mean_rmsd=None, n_bins: int = 20,
                      params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from four results of ``mean_structure`` -- ``runs["ref"]`` (all reference frames),
    ``"gen"``, ``"even"`` and ``"odd"`` (the reference's halves), all over the selection ``sel`` -- pure host.
    ``group_labels [m]``: a group per selected atom (``None``: a row per atom); ``mean_rmsd`` / ``floor_mean_rmsd``: the
    superposed RMSD between the means of ref and gen / of even and odd, which ``compare`` takes from K17."""
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    labels = group_rows(sel, group_labels)[0]
    prof = {k: None if r["rmsf"] is None else group_profile(r["rmsf"], sel, group_labels)[1] for k, r in runs.items()}
    stats = _profile_stats(prof["ref"], prof["gen"])
    floor = dict(_profile_stats(prof["even"], prof["odd"]), mean_rmsd=floor_mean_rmsd)
    block, top = None, []
    r_ref, r_gen = np.asarray(runs["ref"]["rmsd"], dtype=np.float64), np.asarray(runs["gen"]["rmsd"], dtype=np.float64)
    fin = lambda v: v[np.isfinite(v)]
    if fin(r_ref).size and fin(r_gen).size:
        hi = 1.2 * float(fin(r_ref).max())
        block = scalar_block(fin(r_ref[0::2]), fin(r_ref[1::2]), fin(r_gen), 0.0, hi if hi > 0 else 1.0, n_bins)
    if prof["ref"] is not None and prof["gen"] is not None:
        dev = np.abs(prof["gen"] - prof["ref"])
        for k in np.argsort(-dev, kind="stable")[:10]:
            top.append({"label": labels[int(k)], "rmsf_ref": float(prof["ref"][k]), "rmsf_gen": float(prof["gen"][k])})
    listed = lambda v: None if v is None else [float(t) for t in v]
    return {"n_ref": int(r_ref.shape[0]), "n_gen": int(r_gen.shape[0]), "n_bad_ref": int(np.asarray(runs["ref"]["bad"]).sum()),
            "n_bad_gen": int(np.asarray(runs["gen"]["bad"]).sum()), "params": dict(params or {}, n_bins=int(n_bins)),
            "labels": labels, "rmsf_ref": listed(prof["ref"]), "rmsf_gen": listed(prof["gen"]), **stats,
            "mean_rmsd": mean_rmsd, "rmsd_to_mean": block, "floor": floor,
            "convergence": {k: {name: r[name] for name in ("iterations", "converged", "last_move")} for k, r in runs.items()},
            "top_atoms": top}


FLEX_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "labels", "rmsf_ref", "rmsf_gen", "pearson",
                   "profile_rmse", "ratio", "mean_rmsd", "rmsd_to_mean", "floor", "convergence", "top_atoms")


def summary_of(stats: dict) -> dict:
    """What the command-line tools put under ``"flex_stats"`` in their JSON summary line: no profiles, no histograms."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "pearson", "profile_rmse", "ratio", "mean_rmsd",
                                   "floor", "convergence")}
    short["rmsd_to_mean"] = ensemble.short_block(stats["rmsd_to_mean"], ("jsd", "floor") + ensemble.MOMENTS[1:])
    return short
