"""Does a generated ensemble populate the slow, collective states of the simulation?  Time-lagged independent component
analysis (TICA) of pairwise distances: moments and projections on the device (K16, ``cgv_tica_moments`` /
``cgv_tica_project``), the eigenproblem and the comparison in fp64 on the host.

The reference answers this offline in ``CoarseGrainingVAE/postanalysis.py:25-68``: pairwise backbone-atom distances with
``excluded_neighbors=2``, ``pyemma.coordinates.tica(lag=100)`` on the simulation, ``tica.transform`` of the generated
structures.  Here the atoms come from element and connectivity (``backbone_atoms``, the rule of
``distributions.peptide_backbone_torsions``), the features are computed on the fly from the coordinates (no
``[frames, d]`` tensor is stored), the two launches of ``cgv_tica_moments`` accumulate the five sums of a segment in fp64
on the matrix cores, and ``fit_from_moments`` solves the symmetrised (reversible) estimator with ``numpy.linalg.eigh``.

A feature is an fp32 distance, ``sqrt((dx*dx + dy*dy) + dz*dz)`` with every operation rounded, widened to fp64: a host
restatement in ``numpy.float32`` holds the same bits.  Non-finite coordinates are not filtered: they propagate into the
moments (and make the fit fail loudly), and count as ``outside`` in the projection's histogram.

The host pieces shared with the other analyses (``adjacency``, ``peptide_residues``, ``js_divergence``, ``read_back``)
live in ``ensemble``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ensemble
from .ensemble import adjacency, device_of, js_divergence, peptide_residues, read_back


# ----------------------------------------------------------------------------- features
def backbone_atoms(z, bonds) -> np.ndarray:
    """The N, CA and C atoms of every residue that ``distributions.peptide_backbone_torsions``' rule finds (a nitrogen, a
    non-amide carbon on it, an amide carbon on that: element and connectivity only), sorted.  Empty for a molecule
    without a peptide backbone: callers then need an explicit ``sel``."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    _, residues = peptide_residues(z, adjacency(z.shape[0], bonds))
    return np.array(sorted({a for r in residues for a in r}), dtype=np.int64)


def distance_pairs(sel, excluded_neighbors: int = 2) -> np.ndarray:
    """All ``(I, J)`` with ``I < J``, both in ``sel``, ``J > I + excluded_neighbors`` ON ATOM INDICES (not on positions in
    ``sel``), row-major over sorted ``sel``; int32 ``[d,2]``.  This is what pyemma's ``featurizer.pairs(sel,
    excluded_neighbors)`` does upstream, written from knowledge of that package: pyemma is not installed where this code
    is built and tested, so the equivalence cannot be pinned by a test here."""
    s = np.unique(np.asarray(sel, dtype=np.int64).reshape(-1))
    rows = [(int(i), int(j)) for a, i in enumerate(s) for j in s[a + 1:] if j > i + int(excluded_neighbors)]
    return np.array(rows, dtype=np.int32).reshape(-1, 2)


def limits() -> Dict[str, int]:
    return ensemble.limits("tica", ("features", "atoms", "bins2", "components"))


def _check_pairs(pairs, n_atoms: int) -> np.ndarray:
    """The pair table as the kernels take it; ``ValueError`` before any launch for a table the kernels would have to
    repair (an index outside ``[0, n_atoms)``) or cannot hold."""
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    lim = limits()
    if p.shape[0] == 0:
        raise ValueError("the pair table is empty: no features (pass an explicit sel)")
    if p.shape[0] > lim["features"]:
        raise ValueError(f"{p.shape[0]} distance features (the kernel holds {lim['features']}): pass a sparser sel")
    if n_atoms > lim["atoms"]:
        raise ValueError(f"{n_atoms} atoms per frame (the kernel holds {lim['atoms']})")
    if p.min() < 0 or p.max() >= n_atoms:
        raise ValueError(f"the pair table names atom {int(p.max() if p.max() >= n_atoms else p.min())}, a frame has {n_atoms} atoms")
    return p.astype(np.int32)


def frames(x) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"frames must be [T, n, 3], got {tuple(t.shape)}")
    return t


def split_segments(xyz, traj_starts=None) -> list:
    """The frames of a ``tools/traj_to_npz.py`` file as time-ordered segments: cut at ``traj_starts`` (int64, ascending,
    first 0) when the file has the key, one segment otherwise."""
    if traj_starts is None:
        return [xyz]
    s = np.asarray(traj_starts, dtype=np.int64).reshape(-1)
    if s.shape[0] == 0 or s[0] != 0 or (np.diff(s) <= 0).any() or s[-1] >= len(xyz):
        raise ValueError("traj_starts must be ascending frame indices, the first 0, all below the number of frames")
    ends = list(s[1:]) + [len(xyz)]
    return [xyz[int(a):int(b)] for a, b in zip(s, ends)]


# ----------------------------------------------------------------------------- moments
MOMENT_KEYS = ("sum_x", "sum_y", "cxx", "cyy", "cxy")


def moments_launch(xyz: torch.Tensor, pairs: torch.Tensor, lag: int, totals: Dict[str, torch.Tensor],
                   workspace: Optional[torch.Tensor] = None) -> int:
    """One ``cgv_tica_moments`` call: the sums of the segment ``xyz [T,n,3]`` (device, fp32) are ADDED to ``totals``
    (device, fp64: ``sum_x``, ``sum_y [d]``, ``cxx``, ``cyy``, ``cxy [d,d]``).  Returns the frame pairs it counted."""
    T, n, d = int(xyz.shape[0]), int(xyz.shape[1]), int(pairs.shape[0])
    if xyz.dtype != torch.float32 or pairs.dtype != torch.int32 or any(totals[k].dtype != torch.float64 for k in MOMENT_KEYS):
        raise ValueError("xyz must be float32, pairs int32, the totals float64")
    if tuple(totals["sum_x"].shape) != (d,) or tuple(totals["sum_y"].shape) != (d,) or any(
            tuple(totals[k].shape) != (d, d) for k in ("cxx", "cyy", "cxy")):
        raise ValueError("the totals do not have the shape of the pair table")
    need = int(_lib.load().cgv_tica_moments_workspace_bytes(T, d, int(lag)))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = ensemble.workspace(need, xyz.device)
    _lib.call("cgv_tica_moments", _lib.ptr(xyz), _lib.ptr(pairs), T, n, d, int(lag), *[_lib.ptr(totals[k]) for k in MOMENT_KEYS],
              _lib.ptr(workspace), workspace.numel() * workspace.element_size(), _lib.stream_ptr(), tag="tica_moments")
    return max(T - int(lag), 0)


def moments(trajs: Sequence, pairs, lag: int, frames_per_launch: int = 65536, device="cuda") -> dict:
    """The five sums of a TICA fit over the time-ordered segments ``trajs`` (a list of ``[T_i,n,3]`` host arrays or
    tensors): fp64 host arrays ``sum_x``, ``sum_y [d]``, ``cxx``, ``cyy``, ``cxy [d,d]`` and ``n_frame_pairs`` =
    ``sum(max(T_i - lag, 0))``.  A frame pair ``(t, t + lag)`` never crosses a segment boundary.  A segment with more
    than ``frames_per_launch`` pairs is fed as overlapping chunks ``[s, s + M + lag)``, so that every pair is counted
    exactly once.  The totals stay on the device in fp64 across the launches; ONE read-back."""
    lag, M = int(lag), max(int(frames_per_launch), 1)
    if lag < 1:
        raise ValueError("lag must be at least 1")
    segs = [frames(x) for x in trajs]
    if not segs:
        raise ValueError("no trajectory segments")
    n = int(segs[0].shape[1])
    if any(int(s.shape[1]) != n for s in segs):
        raise ValueError("the segments have different atom counts")
    table = _check_pairs(pairs, n)
    d = table.shape[0]
    cuda = [s for s in segs if s.is_cuda]
    dev = cuda[0].device if cuda else torch.device(device)
    ptab = torch.from_numpy(table).to(dev)
    totals = {k: torch.zeros((d,) if k.startswith("sum") else (d, d), dtype=torch.float64, device=dev) for k in MOMENT_KEYS}
    longest = max(min(int(s.shape[0]), M + lag) for s in segs)
    workspace = ensemble.workspace(_lib.load().cgv_tica_moments_workspace_bytes(longest, d, lag), dev)
    count = 0
    for seg in segs:
        N = int(seg.shape[0]) - lag
        for start in range(0, max(N, 0), M):
            m = min(M, N - start)
            chunk = seg[start:start + m + lag].detach().to(dev, torch.float32).contiguous()
            count += moments_launch(chunk, ptab, lag, totals, workspace)
    host = read_back([totals[k] for k in MOMENT_KEYS])
    return {**{k: np.array(v) for k, v in zip(MOMENT_KEYS, host)}, "n_frame_pairs": int(count)}


# ----------------------------------------------------------------------------- the fit (host, fp64)
@dataclass
class TicaModel:
    """A fitted TICA: ``pairs [d,2]`` int32, ``lag``, ``mean [d]``, ``W [d,k]`` (a structure's independent components are
    ``(f - mean) @ W``), ``eigenvalues [k]`` / ``timescales [k]`` (in frames) of the kept components, ``rank`` (directions
    of C0 kept), ``n_frame_pairs``."""
    pairs: np.ndarray
    lag: int
    mean: np.ndarray
    W: np.ndarray
    eigenvalues: np.ndarray
    timescales: np.ndarray
    rank: int
    n_frame_pairs: int

    def save(self, path: str) -> None:
        np.savez(path, pairs=self.pairs, lag=np.int64(self.lag), mean=self.mean, W=self.W, eigenvalues=self.eigenvalues,
                 timescales=self.timescales, rank=np.int64(self.rank), n_frame_pairs=np.int64(self.n_frame_pairs))

    @staticmethod
    def load(path: str) -> "TicaModel":
        with np.load(path, allow_pickle=False) as f:
            return TicaModel(f["pairs"].astype(np.int32), int(f["lag"]), f["mean"].astype(np.float64), f["W"].astype(np.float64),
                             f["eigenvalues"].astype(np.float64), f["timescales"].astype(np.float64), int(f["rank"]),
                             int(f["n_frame_pairs"]))


def fit_from_moments(m: dict, lag: int, dim: int = 2, epsilon: float = 1e-6, pairs=None) -> TicaModel:
    """The symmetrised (reversible) TICA estimator from the sums of ``moments``; pure host, fp64, no GPU.  With
    ``N = n_frame_pairs``:

      mu = (sum_x + sum_y) / 2N      C0 = (cxx + cyy) / 2N - mu mu^T      Ct = (cxy + cxy^T) / 2N - mu mu^T
      eigh(C0) = Q diag(l) Q^T, keep l_i > epsilon * l_max;  L = Q_keep diag(l_keep)^(-1/2)
      eigh(L^T Ct L), eigenvalues descending -> V;  W = L V[:, :dim]

    The cut-off is RELATIVE to the largest eigenvalue of C0: coordinates here are in Angstrom and pyemma's in nm, so its
    absolute ``epsilon`` would not carry over.  Each column of W has its entry of largest magnitude positive.
    ``timescales = -lag / ln|lambda|`` in frames.  There is no kinetic-map scaling: the components have unit variance on
    the data (``W^T C0 W = I``), not variance ``lambda^2``."""
    N = int(m["n_frame_pairs"])
    if N < 1:
        raise ValueError("no frame pairs: every segment is at most `lag` frames long")
    sx, sy = np.asarray(m["sum_x"], np.float64), np.asarray(m["sum_y"], np.float64)
    cxx, cyy, cxy = (np.asarray(m[k], np.float64) for k in ("cxx", "cyy", "cxy"))
    if not all(np.isfinite(a).all() for a in (sx, sy, cxx, cyy, cxy)):
        raise ValueError("the moments are not finite (a non-finite coordinate in the trajectory)")
    mu = (sx + sy) / (2.0 * N)
    c0 = (cxx + cyy) / (2.0 * N) - np.outer(mu, mu)
    ct = (cxy + cxy.T) / (2.0 * N) - np.outer(mu, mu)
    lam, Q = np.linalg.eigh(0.5 * (c0 + c0.T))
    keep = lam > float(epsilon) * lam.max()
    if lam.max() <= 0 or not keep.any():
        raise ValueError("the features do not vary: C0 has no positive eigenvalue")
    L = Q[:, keep] / np.sqrt(lam[keep])[None, :]
    ev, V = np.linalg.eigh(L.T @ ct @ L)
    order = np.argsort(-ev, kind="stable")
    ev, V = ev[order], V[:, order]
    k = min(int(dim), int(keep.sum()))
    W = L @ V[:, :k]
    big = np.abs(W).argmax(axis=0)
    W = W * np.where(W[big, np.arange(k)] < 0, -1.0, 1.0)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        ts = -float(lag) / np.log(np.abs(ev[:k]))
    d = mu.shape[0]
    table = np.zeros((d, 2), np.int32) if pairs is None else np.asarray(pairs, dtype=np.int32).reshape(d, 2)
    return TicaModel(table, int(lag), mu, np.ascontiguousarray(W), ev[:k].copy(), ts, int(keep.sum()), N)


def fit(trajs: Sequence, pairs, lag: int, dim: int = 2, epsilon: float = 1e-6, frames_per_launch: int = 65536,
        device="cuda") -> TicaModel:
    return fit_from_moments(moments(trajs, pairs, lag, frames_per_launch, device), lag, dim, epsilon, pairs=pairs)


# ----------------------------------------------------------------------------- projection
def project_launch(xyz: torch.Tensor, pairs: torch.Tensor, mean: torch.Tensor, W: torch.Tensor, ics: Optional[torch.Tensor],
                   hist=None) -> None:
    """One ``cgv_tica_project`` launch over ``xyz [S,n,3]`` (device, fp32).  ``ics [S,k]`` fp64 is written (or ``None``);
    ``hist = (comp_a, comp_b, n_bins2, (lo_a, hi_a), (lo_b, hi_b), counts [nb,nb] int32, outside [1] int32)`` is ADDED
    to (or ``None``)."""
    S, n, d, k = int(xyz.shape[0]), int(xyz.shape[1]), int(pairs.shape[0]), int(W.shape[1])
    if xyz.dtype != torch.float32 or pairs.dtype != torch.int32 or mean.dtype != torch.float64 or W.dtype != torch.float64:
        raise ValueError("xyz must be float32, pairs int32, mean and W float64")
    if tuple(mean.shape) != (d,) or int(W.shape[0]) != d or (ics is not None and (tuple(ics.shape) != (S, k) or ics.dtype != torch.float64)):
        raise ValueError("mean [d], W [d,k], ics [S,k] float64")
    _lib.call("cgv_tica_project", _lib.ptr(xyz), _lib.ptr(pairs), _lib.ptr(mean), _lib.ptr(W), S, n, d, k, _lib.ptr(ics),
              *ensemble.hist2_args(hist, k, limits()), _lib.stream_ptr(), tag="tica_project")


def project(xyz, model: TicaModel, structures_per_launch: int = 16384, device="cuda", hist=None, want_ics: bool = True):
    """The independent components ``[S,k]`` (host, fp64) of the structures ``xyz [S,n,3]``: one launch per
    ``structures_per_launch`` structures, ONE read-back.  ``hist = (comp_a, comp_b, n_bins2, (lo_a, hi_a), (lo_b, hi_b))``
    also gives the joint histogram of two components: the return value is then ``(ics, counts [nb,nb] int64, outside)``;
    with ``want_ics=False`` the components are neither stored nor read back (``ics`` is ``None``)."""
    x = frames(xyz)
    S, n, k = int(x.shape[0]), int(x.shape[1]), int(model.W.shape[1])
    table = _check_pairs(model.pairs, n)
    lim = limits()
    if not 1 <= k <= lim["components"]:
        raise ValueError(f"a launch projects onto 1..{lim['components']} components, the model has {k}")
    dev = device_of(x, device)
    acc = None if hist is None else ensemble.Hist2(hist, k, lim, dev)
    ptab = torch.from_numpy(table).to(dev)
    mean = torch.from_numpy(np.ascontiguousarray(model.mean, dtype=np.float64)).to(dev)
    W = torch.from_numpy(np.ascontiguousarray(model.W, dtype=np.float64)).to(dev)
    ics = torch.zeros(S, k, dtype=torch.float64, device=dev) if want_ics else None
    M = max(int(structures_per_launch), 1)
    for start, chunk in ensemble.chunks(x, M, dev):
        run = lambda h: project_launch(chunk, ptab, mean, W, ics[start:start + M] if want_ics else None, h)
        acc.launch(run) if acc else run(None)
    back = read_back(([ics] if want_ics else []) + (acc.totals() if acc else []))
    out_ics = np.array(back[0]) if want_ics else None
    if hist is None:
        return out_ics
    return out_ics, np.array(back[-2]), int(back[-1][0])


# ----------------------------------------------------------------------------- comparison
def compare(ref_trajs, gen_xyz, z, bonds, lag: int = 100, sel=None, excluded_neighbors: int = 2, n_bins2: int = 50,
            dim: int = 2, epsilon: float = 1e-6, frames_per_launch: int = 65536, structures_per_launch: int = 16384,
            device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against the time-ordered reference segments ``ref_trajs`` (a list of
    ``[T_i,n,3]``) in the plane of the reference's two slowest independent components.  TICA is fitted on the reference
    over the distances of ``distance_pairs(sel, excluded_neighbors)`` (``sel`` default: ``backbone_atoms(z, bonds)``);
    the histogram ranges are the reference's min / max of IC1 and IC2, widened by 5 % of the span on each side.
    Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_frame_pairs, d, lag, rank, n_bins2, sel, eigenvalues, timescales (frames), ranges [[lo, hi]] * 2
      jsd          Jensen-Shannon divergence (base 2) of the reference's and the generated (IC1, IC2) maps
      floor        the same between the even and the odd reference frames: what ``jsd`` is to be read against
      jsd_ic, floor_ic   [2] the same for the two marginals
      outside_gen  generated structures that fall outside the ranges (left out of the distributions); outside_ref
      counts       {ref, gen}: the maps [n_bins2][n_bins2] themselves

    A model of one component (rank 1) compares that component with itself: the map is its diagonal."""
    segs = [frames(x) for x in ref_trajs]
    z = np.asarray(z).astype(np.int64).reshape(-1)
    if sel is None:
        sel = backbone_atoms(z, bonds)
        if sel.shape[0] == 0:
            raise ValueError("the molecule has no peptide backbone: pass the atoms to use as sel")
    pairs = distance_pairs(sel, excluded_neighbors)
    model = fit(segs, pairs, lag, dim=dim, epsilon=epsilon, frames_per_launch=frames_per_launch, device=device)
    ref = torch.cat([s.detach().cpu() for s in segs]) if len(segs) > 1 else segs[0]
    kw = dict(structures_per_launch=structures_per_launch, device=device)
    ref_ics = project(ref, model, **kw)
    k = ref_ics.shape[1]
    ca, cb = 0, min(1, k - 1)
    ranges = []
    for c in (ca, cb):
        lo, hi = float(ref_ics[:, c].min()), float(ref_ics[:, c].max())
        pad = 0.05 * (hi - lo) if hi > lo else 0.5
        ranges.append((lo - pad, hi + pad))
    hist = (ca, cb, int(n_bins2), ranges[0], ranges[1])
    _, even, out_even = project(ref[0::2], model, hist=hist, want_ics=False, **kw)
    _, odd, out_odd = project(ref[1::2], model, hist=hist, want_ics=False, **kw)
    gen = frames(gen_xyz)
    _, gen_counts, out_gen = project(gen, model, hist=hist, want_ics=False, **kw)
    whole = even + odd
    return {"n_ref": int(ref.shape[0]), "n_gen": int(gen.shape[0]), "n_frame_pairs": model.n_frame_pairs, "d": int(pairs.shape[0]),
            "lag": int(lag), "rank": model.rank, "n_bins2": int(n_bins2), "sel": [int(a) for a in np.unique(sel)],
            "eigenvalues": model.eigenvalues.tolist(), "timescales": [float(t) if np.isfinite(t) else None for t in model.timescales],
            "ranges": [list(r) for r in ranges],
            "jsd": js_divergence(whole, gen_counts), "floor": js_divergence(even, odd),
            "jsd_ic": [js_divergence(whole.sum(1), gen_counts.sum(1)), js_divergence(whole.sum(0), gen_counts.sum(0))],
            "floor_ic": [js_divergence(even.sum(1), odd.sum(1)), js_divergence(even.sum(0), odd.sum(0))],
            "outside_gen": int(out_gen), "outside_ref": int(out_even + out_odd),
            "counts": {"ref": whole.tolist(), "gen": gen_counts.tolist()}}


TICA_STATS_KEYS = ("n_ref", "n_gen", "n_frame_pairs", "d", "lag", "rank", "n_bins2", "sel", "eigenvalues", "timescales", "ranges",
                   "jsd", "floor", "jsd_ic", "floor_ic", "outside_gen", "outside_ref", "counts")


def summary_of(stats: dict) -> dict:
    """What the command-line tools put under ``"tica_stats"`` in their JSON summary line."""
    return {k: stats[k] for k in ("jsd", "floor", "jsd_ic", "floor_ic", "outside_gen", "eigenvalues", "timescales", "rank", "d",
                                  "lag", "n_ref", "n_gen")}
