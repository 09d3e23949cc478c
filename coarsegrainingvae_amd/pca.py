"""In which directions do the atoms of an ensemble move TOGETHER?  Cartesian principal component analysis of the superposed
ensemble ("essential dynamics", Amadei, Linssen & Berendsen 1993; what ``gmx covar`` / ``gmx anaeig`` do): every structure
is superposed onto a target (K21, ``cgv_align_accumulate``), the ``3m x 3m`` covariance of the selected atoms' coordinates
is accumulated on the fp64 matrix cores (K27, ``cgv_pca_moments``; ``csrc/pca.hip``), the eigenproblem is solved in fp64 on
the host and structures are projected onto the modes on the device (``cgv_pca_project``).

``flexibility`` says how MUCH every atom moves.  A decoder can reproduce every per-atom RMSF and still move its atoms
independently where the simulation moves a hairpin as one hinge; RMSF, contact maps, DSSP and hydrogen bonds do not see
that difference, and ``tica`` is built on pairwise distances and needs time order, which a generated ensemble does not have.
Nothing in the reference computes a coordinate covariance.

Definition.  With ``y`` the structures superposed onto ``target`` over the selection ``sel [m]`` (in the frame in which the
target's selected atoms have their centroid at the origin), the feature of a structure is
``f[3a + c] = (double)y[sel[a], c] - centre[sel[a], c]`` with ``centre`` = the centred target (exact widening, one fp64
rounding: a numpy restatement holds the same bits), ``d = 3m``.  Over the N good structures (a structure with ANY non-finite
coordinate is bad and enters nothing) ``mu = sum f / N`` and ``C = sum f f^T / N - mu mu^T`` -- DIVIDED BY N, not N - 1, as
``gmx covar`` does.  ``eigh(C)``: eigenvalues descending (Angstrom^2) and clamped at 0, the modes orthonormal, each with its
entry of largest magnitude positive.  A structure's principal components are ``(f - mu) W``; ``cgv_pca_project`` is handed
``mu`` and subtracts it per feature (nothing is folded into an offset on the host).

What the numbers do not mean:
  * for an ensemble with several distinct states the leading modes are the directions that CONNECT the states, not the
    motion inside any of them, and the eigenvalues measure the populations' spread as much as flexibility;
  * the modes depend on the selection (compare only for the same one) and on the target everything is superposed onto --
    ``compare`` superposes all its sets onto ONE target, the reference's mean structure, for that reason;
  * after superposition the six rigid-body directions carry next to no variance: the last six eigenvalues are near zero and
    say nothing about the molecule, and RMSIP / overlap computed with ``dim`` close to ``d`` are dominated by them.

The host pieces shared with the other analyses live in ``ensemble``; the command line's front is ``compare_cli``.
"""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble, flexibility
from .ensemble import check_sets, js_divergence, read_back, select_atoms


def limits() -> Dict[str, int]:
    return ensemble.limits("pca", ("features", "atoms", "structures", "components", "bins2"))


# ----------------------------------------------------------------------------- checks that need no device
def _selection(sel, n_atoms: int) -> np.ndarray:
    """The selection as both kernels take it (K21 fits on it, K27 analyses it): at least three atoms, none twice, all in
    ``[0, n_atoms)``, and ``3m`` features within the limit."""
    table = ensemble.selection(sel, n_atoms, purpose="analyse", at_least=3)
    lim = limits()
    if 3 * table.shape[0] > lim["features"]:
        raise ValueError(f"{table.shape[0]} selected atoms are {3 * table.shape[0]} features (the kernel holds {lim['features']}): "
                         "pass a sparser selection (-pca_atoms backbone)")
    return table


def _check_dim(dim: int, d: int) -> int:
    k = limits()["components"]
    if not 1 <= int(dim) <= min(k, d):
        raise ValueError(f"dim must be in 1..{min(k, d)} (a launch projects onto at most {k} modes, there are {d} features), got {dim}")
    return int(dim)


def atoms_of(z, bonds, atoms="heavy") -> np.ndarray:
    """``select_atoms(z, atoms)``, and ``"backbone"``: the N, CA, C of every residue (``tica.backbone_atoms``)."""
    if isinstance(atoms, str) and atoms == "backbone":
        from .tica import backbone_atoms
        sel = backbone_atoms(z, bonds)
        if sel.shape[0] == 0:
            raise ValueError("the molecule has no peptide backbone: pass 'heavy', 'all' or an index array")
        return sel
    if isinstance(atoms, str) and atoms not in ("heavy", "all"):
        raise ValueError("atoms must be 'heavy', 'all', 'backbone' or an index array")
    return select_atoms(z, atoms)


def centred(target, sel) -> np.ndarray:
    """``target [n,3]`` in the frame K21 writes ``aligned`` in: its selected atoms' centroid at the origin (fp64)."""
    t = np.asarray(target, dtype=np.float64)
    return np.ascontiguousarray(t - t[np.asarray(sel, dtype=np.int64)].mean(0))


# ----------------------------------------------------------------------------- launches
def _check_chunk(y, sel, centre, bad):
    if y.dim() != 3 or y.shape[2] != 3:
        raise ValueError(f"y must be [S, n, 3], got {tuple(y.shape)}")
    S, n, m = int(y.shape[0]), int(y.shape[1]), int(sel.numel())
    if y.dtype != torch.float32 or sel.dtype != torch.int32 or centre.dtype != torch.float64 or bad.dtype != torch.int32:
        raise ValueError("y must be float32, sel and bad int32, centre float64")
    lim = limits()
    if n < 1 or n > lim["atoms"]:
        raise ValueError(f"{n} atoms per structure (the kernel holds 1..{lim['atoms']})")
    if S > lim["structures"]:
        raise ValueError(f"{S} structures (a launch holds {lim['structures']})")
    if sel.dim() != 1 or m < 1 or 3 * m > lim["features"]:
        raise ValueError(f"the selection lists {m} atoms: 1..{lim['features'] // 3} ({lim['features']} features) are held")
    if tuple(centre.shape) != (n, 3) or tuple(bad.shape) != (S,):
        raise ValueError(f"centre must be [{n}, 3] and bad [{S}], got {tuple(centre.shape)} and {tuple(bad.shape)}")
    return S, n, m


def new_totals(d: int, device) -> Dict[str, torch.Tensor]:
    """Zeroed accumulators as ``cgv_pca_moments`` adds to them."""
    return {"sum": torch.zeros(d, dtype=torch.float64, device=device), "cov": torch.zeros(d, d, dtype=torch.float64, device=device),
            "n_good": torch.zeros(1, dtype=torch.int32, device=device)}


def moments_launch(y: torch.Tensor, sel: torch.Tensor, centre: torch.Tensor, bad: torch.Tensor, totals: Dict[str, torch.Tensor],
                   workspace: Optional[torch.Tensor] = None) -> None:
    """One ``cgv_pca_moments`` call on device tensors: ``y [S,n,3]`` fp32 and ``bad [S]`` int32 as K21 wrote them, ``sel [m]``
    int32, ``centre [n,3]`` fp64.  ``totals`` (``new_totals``: ``sum [3m]``, ``cov [3m,3m]`` fp64, ``n_good [1]`` int32) are ADDED
    to.  Shapes, dtypes and limits are checked before the launch; the CONTENTS of ``sel`` are the caller's to check."""
    S, n, m = _check_chunk(y, sel, centre, bad)
    d = 3 * m
    for key, shape, dt in (("sum", (d,), torch.float64), ("cov", (d, d), torch.float64), ("n_good", (1,), torch.int32)):
        if tuple(totals[key].shape) != shape or totals[key].dtype != dt:
            raise ValueError(f"totals[{key!r}] must be {dt} {shape}, got {totals[key].dtype} {tuple(totals[key].shape)}")
    if S == 0:
        return
    need = int(_lib.load().cgv_pca_moments_workspace_bytes(S, d))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = ensemble.workspace(need, y.device)
    _lib.call("cgv_pca_moments", _lib.ptr(y), _lib.ptr(sel), _lib.ptr(centre), _lib.ptr(bad), S, n, m, _lib.ptr(totals["sum"]),
              _lib.ptr(totals["cov"]), _lib.ptr(totals["n_good"]), _lib.ptr(workspace), workspace.numel() * workspace.element_size(),
              _lib.stream_ptr(), tag="pca_moments")


def project_launch(y: torch.Tensor, sel: torch.Tensor, centre: torch.Tensor, bad: torch.Tensor, mean: torch.Tensor, W: torch.Tensor,
                   proj: Optional[torch.Tensor], hist=None) -> None:
    """One ``cgv_pca_project`` launch.  ``mean [3m]``, ``W [3m,k]`` fp64; ``proj [S,k]`` fp64 is overwritten (or ``None``);
    ``hist = (comp_a, comp_b, n_bins2, (lo_a, hi_a), (lo_b, hi_b), counts [nb,nb] int32, outside [1] int32)`` is ADDED to
    (or ``None``)."""
    S, n, m = _check_chunk(y, sel, centre, bad)
    d = 3 * m
    if mean.dtype != torch.float64 or W.dtype != torch.float64 or tuple(mean.shape) != (d,) or W.dim() != 2 or int(W.shape[0]) != d:
        raise ValueError(f"mean [{d}] and W [{d}, k] must be float64")
    k, lim = int(W.shape[1]), limits()
    if not 1 <= k <= lim["components"]:
        raise ValueError(f"a launch projects onto 1..{lim['components']} modes, W has {k}")
    if proj is not None and (tuple(proj.shape) != (S, k) or proj.dtype != torch.float64):
        raise ValueError(f"proj must be [{S}, {k}] float64")
    args = ensemble.hist2_args(hist, k, lim)
    if S == 0:
        return
    _lib.call("cgv_pca_project", _lib.ptr(y), _lib.ptr(sel), _lib.ptr(centre), _lib.ptr(bad), _lib.ptr(mean), _lib.ptr(W), S, n, m, k,
              _lib.ptr(proj), *args, _lib.stream_ptr(), tag="pca_project")


class _Chunks:
    """The structures of one set on the device, cut into launches: K21 superposes a chunk onto ``target`` into ONE reused
    ``[M,n,3]`` fp32 buffer (the aligned structures never exist for the whole set), and the caller's launch reads it."""

    def __init__(self, xyz, sel, target, structures_per_launch, device, recentre=True):
        x = ensemble.structures(xyz)
        table = _selection(sel, int(x.shape[1]))
        t = np.asarray(target, dtype=np.float64)
        if t.shape != (int(x.shape[1]), 3) or not np.isfinite(t).all():
            raise ValueError(f"target must be a finite [{int(x.shape[1])}, 3], got {t.shape}")
        self.p = p = flexibility._Passes(x, table, structures_per_launch, device)
        self.d = 3 * table.shape[0]
        lib = _lib.load()
        p.M = min(p.M, limits()["structures"])
        while p.M > 64 and p.M * p.n * 12 + int(lib.cgv_pca_moments_workspace_bytes(p.M, self.d)) > ensemble.WORKSPACE_BYTES:
            p.M //= 2
        # a model's target is centred already and is handed to both kernels as stored: the same bits as when it was fitted
        self.centre_host = centred(t, table) if recentre else np.ascontiguousarray(t)
        self.centre = torch.from_numpy(self.centre_host).to(p.dev)
        self.buf = torch.empty(min(p.M, max(p.S, 1)), p.n, 3, dtype=torch.float32, device=p.dev)
        self.state = flexibility.new_state(p.n, p.dev)

    def __iter__(self):
        p, st = self.p, self.state
        for start in range(0, p.S, p.M):
            stop = min(start + p.M, p.S)
            y = self.buf[:stop - start]
            flexibility.align_accumulate(p.x[start:stop], p.sel, self.centre, st["sum"], st["dev2"], st["n_good"], p.rmsd2[start:stop],
                                         p.bad[start:stop], y, workspace=p.ws)
            yield start, stop, y


def moments(xyz, target, sel=None, structures_per_launch: int = 4096, device="cuda") -> dict:
    """The sums a covariance needs, over the structures ``xyz [S,n,3]`` superposed onto ``target [n,3]`` over ``sel`` (at
    least three atoms, none twice; default: all).  Per chunk of ``structures_per_launch`` structures (lowered until the
    aligned chunk and the workspace fit ``ensemble.WORKSPACE_BYTES``): K21 superposes into a reused buffer, K27 adds the
    chunk's moments about ``centre`` = ``centred(target, sel)``.  The totals stay on the device; ONE read-back.  Host arrays:

      sum [d], cov [d,d] fp64, n_good      d = 3m; ``sum f`` and ``sum f f^T`` over the good structures
      bad [S] bool, rmsd [S]               K21's flags and superposed RMSD to the target (NaN: bad)
      mean_aligned [n,3]                   K21's ``sum / n_good`` (``None``: no good structure);  centre [n,3]
    """
    c = _Chunks(xyz, sel, target, structures_per_launch, device)
    p = c.p
    totals = new_totals(c.d, p.dev)
    ws = ensemble.workspace(int(_lib.load().cgv_pca_moments_workspace_bytes(min(p.M, max(p.S, 1)), c.d)), p.dev)
    for start, stop, y in c:
        moments_launch(y, p.sel, c.centre, p.bad[start:stop], totals, ws)
    s, cov, good, k21, rmsd2, bad = read_back([totals["sum"], totals["cov"], totals["n_good"], c.state["sum"], p.rmsd2, p.bad])
    n_good = int(good[0])
    return {"sum": np.array(s), "cov": np.array(cov), "n_good": n_good, "bad": bad.astype(bool), "rmsd": np.sqrt(rmsd2),
            "mean_aligned": k21 / n_good if n_good else None, "centre": c.centre_host}


# ----------------------------------------------------------------------------- the fit (host, fp64)
@dataclass
class PcaModel:
    """A fitted PCA: ``sel [m]`` int32, ``target [n,3]`` (what structures are superposed onto AND the point the features are
    taken about: its selected atoms' centroid is at the origin), ``mu [d]``, ``eigenvalues [d]`` (all of them, descending,
    Angstrom^2), ``W [d,dim]`` the kept modes (a structure's components are ``(f - mu) @ W``), ``total_variance`` (the trace),
    ``n_good``."""
    sel: np.ndarray
    target: np.ndarray
    mu: np.ndarray
    eigenvalues: np.ndarray
    W: np.ndarray
    total_variance: float
    n_good: int

    def save(self, path: str) -> None:
        np.savez(path, sel=self.sel, target=self.target, mu=self.mu, eigenvalues=self.eigenvalues, W=self.W,
                 total_variance=np.float64(self.total_variance), n_good=np.int64(self.n_good))

    @staticmethod
    def load(path: str) -> "PcaModel":
        with np.load(path, allow_pickle=False) as f:
            return PcaModel(f["sel"].astype(np.int32), f["target"].astype(np.float64), f["mu"].astype(np.float64),
                            f["eigenvalues"].astype(np.float64), f["W"].astype(np.float64), float(f["total_variance"]),
                            int(f["n_good"]))


def covariance_of(m: dict):
    """``(mu [d], C [d,d])`` of the sums of ``moments``: ``mu = sum / N``, ``C = cov / N - mu mu^T`` (divided by N, as
    ``gmx covar`` does), symmetrised.  ``ValueError`` for fewer than two good structures or non-finite sums."""
    N = int(m["n_good"])
    if N < 2:
        raise ValueError(f"{N} good structures: a covariance needs at least two")
    s, cov = np.asarray(m["sum"], np.float64), np.asarray(m["cov"], np.float64)
    if cov.ndim != 2 or cov.shape != (s.shape[0], s.shape[0]):
        raise ValueError(f"the moments do not fit together: sum {s.shape}, cov {cov.shape}")
    if not (np.isfinite(s).all() and np.isfinite(cov).all()):
        raise ValueError("the moments are not finite")
    mu = s / N
    C = cov / N - np.outer(mu, mu)
    return mu, 0.5 * (C + C.T)


def modes_of(C: np.ndarray):
    """``(eigenvalues [d], V [d,d])`` of a symmetric ``C``: ``numpy.linalg.eigh``, eigenvalues descending and clamped at 0,
    each column with its entry of largest magnitude positive (``tica.fit_from_moments``' convention)."""
    lam, V = np.linalg.eigh(C)
    order = np.argsort(-lam, kind="stable")
    lam, V = np.maximum(lam[order], 0.0), V[:, order]
    big = np.abs(V).argmax(axis=0)
    return lam, V * np.where(V[big, np.arange(V.shape[1])] < 0, -1.0, 1.0)[None, :]


def fit_from_moments(m: dict, sel, target, dim: int = 8) -> PcaModel:
    """The model from the sums of ``moments`` -- pure host, fp64, no GPU: ``covariance_of`` (divided by N), then
    ``modes_of``; the first ``dim <= d`` modes are kept.  ``target`` is stored as given: pass ``m["centre"]``, the centred
    target the sums were taken about."""
    mu, C = covariance_of(m)
    d = mu.shape[0]
    sel = np.asarray(sel, dtype=np.int32).reshape(-1)
    if 3 * sel.shape[0] != d:
        raise ValueError(f"the selection lists {sel.shape[0]} atoms, the moments have {d} features")
    if not 1 <= int(dim) <= d:
        raise ValueError(f"dim must be in 1..{d}, got {dim}")
    lam, V = modes_of(C)
    return PcaModel(sel, np.ascontiguousarray(np.asarray(target, dtype=np.float64)), mu, lam, np.ascontiguousarray(V[:, :int(dim)]),
                    float(lam.sum()), int(m["n_good"]))


def fit(xyz, sel=None, target=None, dim: int = 8, structures_per_launch: int = 4096, device="cuda") -> PcaModel:
    """PCA of the structures ``xyz [S,n,3]`` over ``sel`` (default: all atoms) superposed onto ``target [n,3]`` (default:
    ``flexibility.mean_structure(xyz, sel)["mean"]``); ``dim`` modes are kept, at most ``limits()["components"]``."""
    x = ensemble.structures(xyz)
    table = _selection(sel, int(x.shape[1]))
    _check_dim(dim, 3 * table.shape[0])
    kw = dict(structures_per_launch=structures_per_launch, device=device)
    if target is None:
        target = flexibility.mean_structure(x, table, **kw)["mean"]
        if target is None:
            raise ValueError("no structure is good: there is no mean structure to superpose onto")
    m = moments(x, target, table, **kw)
    return fit_from_moments(m, table, m["centre"], dim)


# ----------------------------------------------------------------------------- projection
def project(model: PcaModel, xyz, components=(0, 1), ranges=None, n_bins: int = 50, structures_per_launch: int = 4096,
            device="cuda") -> dict:
    """The principal components of the structures ``xyz [S,n,3]``: per chunk K21 superposes onto ``model.target``, then
    ``cgv_pca_project`` with ``centre = model.target`` and ``mean = model.mu`` forms ``(f - mu) W``.  ``ranges = ((lo_a, hi_a),
    (lo_b, hi_b))`` also bins ``components`` into an ``n_bins x n_bins`` map.  ONE read-back.  Host arrays: ``proj [S,dim]``
    fp64 (NaN rows: bad), ``hist2 [n_bins,n_bins]`` int64 and ``outside`` (``None`` without ``ranges``), ``bad [S]`` bool."""
    k = int(model.W.shape[1])
    c = _Chunks(xyz, model.sel, model.target, structures_per_launch, device, recentre=False)
    if model.W.shape[0] != c.d or model.mu.shape[0] != c.d:
        raise ValueError(f"the model has {model.W.shape[0]} features, its selection {c.d}")
    _check_dim(k, c.d)
    p, centre = c.p, c.centre
    mean = torch.from_numpy(np.ascontiguousarray(model.mu, dtype=np.float64)).to(p.dev)
    W = torch.from_numpy(np.ascontiguousarray(model.W, dtype=np.float64)).to(p.dev)
    proj = torch.empty(p.S, k, dtype=torch.float64, device=p.dev)
    acc = None
    if ranges is not None:
        acc = ensemble.Hist2((components[0], components[1], n_bins, ranges[0], ranges[1]), k, limits(), p.dev, bins_name="n_bins")
    for start, stop, y in c:
        run = lambda h: project_launch(y, p.sel, centre, p.bad[start:stop], mean, W, proj[start:stop], h)
        acc.launch(run) if acc else run(None)
    back = read_back([proj, p.bad] + (acc.totals() if acc else []))
    return {"proj": np.array(back[0]), "bad": back[1].astype(bool), "hist2": np.array(back[2]) if acc else None,
            "outside": int(back[3][0]) if acc else None}


# ----------------------------------------------------------------------------- host statistics
def dccm(C) -> np.ndarray:
    """The dynamic cross-correlation map ``[m,m]`` of a ``[3m,3m]`` covariance: the trace of the 3 x 3 block of atoms
    ``(i, j)`` over the roots of the two diagonal blocks' traces; a row of an atom with zero variance is 0."""
    C = np.asarray(C, dtype=np.float64)
    m = C.shape[0] // 3
    if C.ndim != 2 or C.shape != (3 * m, 3 * m):
        raise ValueError(f"C must be [3m, 3m], got {C.shape}")
    tr = np.einsum("iaja->ij", C.reshape(m, 3, m, 3))
    var = np.maximum(np.diag(tr), 0.0)
    norm = np.sqrt(np.outer(var, var))
    return np.divide(tr, norm, out=np.zeros_like(tr), where=norm > 0)


def rmsip(Wa, Wb) -> float:
    """Root-mean-square inner product of two sets of orthonormal modes ``[d,k]``: ``sqrt(sum_ij (a_i . b_j)^2 / k)``; 1 when
    they span the same space, 0 for orthogonal spaces."""
    Wa, Wb = np.asarray(Wa, dtype=np.float64), np.asarray(Wb, dtype=np.float64)
    if Wa.ndim != 2 or Wb.ndim != 2 or Wa.shape[0] != Wb.shape[0] or Wa.shape[1] < 1:
        raise ValueError(f"the mode sets must be [d, k] over the same features, got {Wa.shape} and {Wb.shape}")
    return float(np.sqrt(((Wa.T @ Wb) ** 2).sum() / Wa.shape[1]))


def covariance_overlap(la, Va, lb, Vb) -> Optional[float]:
    """Hess 2002: ``1 - sqrt(max(0, sum(la + lb) - 2 sum_ij sqrt(la_i lb_j) (va_i . vb_j)^2)) / sqrt(sum(la + lb))`` of two
    spectra (eigenvalues ``[k]``, modes ``[d,k]``): 1 for identical covariances.  ``None`` when both have no variance."""
    la, lb = np.maximum(np.asarray(la, np.float64), 0.0), np.maximum(np.asarray(lb, np.float64), 0.0)
    Va, Vb = np.asarray(Va, np.float64), np.asarray(Vb, np.float64)
    if Va.shape != (Va.shape[0], la.shape[0]) or Vb.shape != (Va.shape[0], lb.shape[0]):
        raise ValueError("eigenvalues [k] and modes [d, k] do not fit together")
    total = float(la.sum() + lb.sum())
    if total <= 0:
        return None
    cross = float((np.sqrt(np.outer(la, lb)) * (Va.T @ Vb) ** 2).sum())
    return float(1.0 - np.sqrt(max(0.0, total - 2.0 * cross)) / np.sqrt(total))


def variance_in_modes(model: PcaModel, C_other) -> np.ndarray:
    """``v_i^T C v_i / lambda_i`` for the kept modes of ``model``: how much of the variance the model's ensemble has along
    its mode ``i`` another ensemble (covariance ``C_other``) has along the same direction.  NaN where ``lambda_i`` is 0."""
    W = np.asarray(model.W, dtype=np.float64)
    lam = np.asarray(model.eigenvalues, dtype=np.float64)[:W.shape[1]]
    along = np.einsum("fi,fg,gi->i", W, np.asarray(C_other, dtype=np.float64), W)
    return np.divide(along, lam, out=np.full_like(along, np.nan), where=lam > 0)


def _pair_stats(a: dict, b: dict, dim: int) -> dict:
    """The four scalars that compare spectrum ``b`` with spectrum ``a`` (``{lam, V, C, dccm}``)."""
    tv_a, tv_b = float(a["lam"].sum()), float(b["lam"].sum())
    return {"rmsip": rmsip(a["V"][:, :dim], b["V"][:, :dim]), "covariance_overlap": covariance_overlap(a["lam"], a["V"], b["lam"], b["V"]),
            "total_variance_ratio": tv_b / tv_a if tv_a > 0 else None,
            "dccm_rmse": float(np.sqrt(np.mean((b["dccm"] - a["dccm"]) ** 2)))}


def compare_from_moments(moms: dict, sel, target, dim: int = 8, pc_map: Optional[dict] = None, params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from four results of ``moments`` -- ``moms["ref"]`` (all reference frames), ``"gen"``,
    ``"even"`` and ``"odd"`` (the reference's halves), all over ``sel`` and superposed onto the same ``target`` -- pure
    host.  ``pc_map``: ``{"range": [[lo, hi], [lo, hi]], "even", "odd", "gen": [n_bins,n_bins] counts}`` of (PC1, PC2) in
    the reference's modes, which ``compare`` takes from ``project``; ``None``: no map."""
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    spec = {}
    for key in ("ref", "gen", "even", "odd"):
        mu, C = covariance_of(moms[key])
        lam, V = modes_of(C)
        spec[key] = {"mu": mu, "C": C, "lam": lam, "V": V, "dccm": dccm(C)}
    d = spec["ref"]["lam"].shape[0]
    if 3 * sel.shape[0] != d or any(spec[k]["lam"].shape[0] != d for k in spec):
        raise ValueError("the four sets of moments and the selection do not have the same features")
    if not 1 <= int(dim) <= d:
        raise ValueError(f"dim must be in 1..{d}, got {dim}")
    dim = int(dim)
    ref, gen = spec["ref"], spec["gen"]
    model = PcaModel(sel.astype(np.int32), np.asarray(target, dtype=np.float64), ref["mu"], ref["lam"], np.ascontiguousarray(ref["V"][:, :dim]),
                     float(ref["lam"].sum()), int(moms["ref"]["n_good"]))
    share = lambda s: [float(v) for v in (s["lam"][:dim] / s["lam"].sum() if s["lam"].sum() > 0 else np.zeros(dim))]
    block = None
    if pc_map is not None:
        even, odd, g = (np.asarray(pc_map[k], dtype=np.int64) for k in ("even", "odd", "gen"))
        block = {"range": [[float(v) for v in r] for r in pc_map["range"]], "jsd": js_divergence(even + odd, g),
                 "floor": js_divergence(even, odd)}
    diff = np.abs(gen["dccm"] - ref["dccm"])
    iu = np.triu_indices(sel.shape[0], 1)
    top = [{"i": int(sel[iu[0][k]]), "j": int(sel[iu[1][k]]), "dccm_ref": float(ref["dccm"][iu[0][k], iu[1][k]]),
            "dccm_gen": float(gen["dccm"][iu[0][k], iu[1][k]])} for k in np.argsort(-diff[iu], kind="stable")[:10]]
    sizes = {"n_ref": int(np.asarray(moms["ref"]["bad"]).shape[0]), "n_gen": int(np.asarray(moms["gen"]["bad"]).shape[0]),
             "n_bad_ref": int(np.asarray(moms["ref"]["bad"], dtype=bool).sum()), "n_bad_gen": int(np.asarray(moms["gen"]["bad"], dtype=bool).sum())}
    out = {**sizes, "params": dict(params or {}, atoms=[int(i) for i in sel], dim=dim),
           "eigenvalues_ref": [float(v) for v in ref["lam"][:dim]], "eigenvalues_gen": [float(v) for v in gen["lam"][:dim]],
           "explained_ref": share(ref), "explained_gen": share(gen), **_pair_stats(ref, gen, dim),
           "variance_in_ref_modes": [float(v) if np.isfinite(v) else None for v in variance_in_modes(model, gen["C"])],
           "pc_map": block, "floor": _pair_stats(spec["even"], spec["odd"], dim), "top_pairs": top}
    return {k: out[k] for k in PCA_STATS_KEYS}


def _compare(ref_xyz, gen_xyz, z, bonds, atoms, dim, n_bins, structures_per_launch, device):
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z)
    sel = _selection(atoms_of(z, bonds, atoms), z.shape[0])
    dim = _check_dim(dim, 3 * sel.shape[0])
    if not 1 <= int(n_bins) <= limits()["bins2"]:
        raise ValueError(f"n_bins must be in 1..{limits()['bins2']}")
    kw = dict(structures_per_launch=structures_per_launch, device=device)
    target = flexibility.mean_structure(ref, sel, **kw)["mean"]
    if target is None:
        raise ValueError("no reference frame is good: there is no mean structure to superpose onto")
    sets = {"ref": ref, "gen": gen, "even": ref[0::2], "odd": ref[1::2]}
    moms = {k: moments(x, target, sel, **kw) for k, x in sets.items()}
    model = fit_from_moments(moms["ref"], sel, moms["ref"]["centre"], dim)
    ca, cb = 0, min(1, dim - 1)
    pr = project(model, ref, **kw)["proj"]
    ranges = []
    for c in (ca, cb):
        v = pr[np.isfinite(pr[:, c]), c]
        lo, hi = float(v.min()), float(v.max())
        pad = 0.2 * (hi - lo) if hi > lo else 0.5
        ranges.append((lo - pad, hi + pad))
    maps = {k: project(model, sets[k], components=(ca, cb), ranges=ranges, n_bins=n_bins, **kw)["hist2"] for k in ("even", "odd", "gen")}
    stats = compare_from_moments(moms, sel, model.target, dim, pc_map=dict(maps, range=ranges),
                                 params={"atoms_rule": atoms if isinstance(atoms, str) else "indices", "n_bins": int(n_bins)})
    return stats, model


def compare(ref_xyz, gen_xyz, z, bonds, atoms="heavy", dim: int = 8, n_bins: int = 50, structures_per_launch: int = 4096,
            device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) of the molecule
    ``z [n]`` / ``bonds [Eb,2]`` by their collective motion.  ALL FOUR sets -- reference, generated, the reference's even and
    odd frames -- are superposed onto the reference's mean structure over ``atoms_of(z, bonds, atoms)`` (``"heavy"``,
    ``"all"``, ``"backbone"`` or indices; at least three atoms), and each gets its own covariance about its own average.
    What the two halves of the reference differ by is the ``floor`` every deviation is to be read against.  Returns a dict
    that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen   structures, and those left out as bad
      params        atoms (the selection), atoms_rule, dim, n_bins
      eigenvalues_ref, eigenvalues_gen     [dim] Angstrom^2;  explained_ref, explained_gen  [dim] their share of the trace
      total_variance_ratio   trace of the generated covariance over the reference's (below 1: the model moves less)
      rmsip         root-mean-square inner product of the first ``dim`` modes of the two sets
      covariance_overlap     Hess' overlap of the two whole covariances
      variance_in_ref_modes  [dim] the generated variance along reference mode i over the reference's
      dccm_rmse     RMS difference of the two dynamic cross-correlation maps
      pc_map        {range, jsd, floor} of the (PC1, PC2) histograms in the REFERENCE's modes; range: the reference's
                    projections padded by 20 % of their span on each side
      floor         {rmsip, covariance_overlap, total_variance_ratio, dccm_rmse} between the even and the odd frames
      top_pairs     the ten atom pairs of largest |dccm_gen - dccm_ref|: {i, j, dccm_ref, dccm_gen}
    """
    return _compare(ref_xyz, gen_xyz, z, bonds, atoms, dim, n_bins, structures_per_launch, device)[0]


PCA_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "eigenvalues_ref", "eigenvalues_gen", "explained_ref",
                  "explained_gen", "total_variance_ratio", "rmsip", "covariance_overlap", "variance_in_ref_modes", "dccm_rmse",
                  "pc_map", "floor", "top_pairs")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"pca_stats"`` in its JSON summary line: no selection, no pair list."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "total_variance_ratio", "rmsip", "covariance_overlap",
                                   "dccm_rmse", "floor")}
    short["dim"] = stats["params"]["dim"]
    short["eigenvalues_ref"], short["eigenvalues_gen"] = stats["eigenvalues_ref"][:3], stats["eigenvalues_gen"][:3]
    short["pc_map"] = None if stats["pc_map"] is None else {k: stats["pc_map"][k] for k in ("jsd", "floor")}
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.pca", "essential dynamics (Cartesian PCA) of generated structures against a reference",
                                top_help="npz with z and bonds; default: those of -ref")
    p.add_argument("-pca_atoms", default="heavy", help="heavy | all | backbone: the atoms superposed on and analysed")
    p.add_argument("-pca_dim", type=int, default=8, help="modes kept and compared (at most 8)")
    p.add_argument("-pca_bins", type=int, default=50, help="bins per axis of the (PC1, PC2) map")
    p.add_argument("-model", default=None, help="npz that takes the reference's PcaModel (not written by default)")
    return compare_cli.finish_parser(p, "pca_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, with everything that can be refused without
    a device refused here (``SystemExit``)."""
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args)
    bonds = np.asarray(top["bonds"])
    with compare_cli.refusing():
        if args.pca_atoms not in ("heavy", "all", "backbone"):
            raise ValueError(f"-pca_atoms must be heavy, all or backbone, got {args.pca_atoms!r}")
        sel = _selection(atoms_of(z, bonds, args.pca_atoms), z.shape[0])
        _check_dim(args.pca_dim, 3 * sel.shape[0])
        if not 1 <= args.pca_bins <= limits()["bins2"]:
            raise ValueError(f"-pca_bins must be in 1..{limits()['bins2']}")
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": bonds}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    with compare_cli.refusing():
        stats, model = _compare(inp["ref_xyz"], inp["gen_xyz"], inp["z"], inp["bonds"], args.pca_atoms, args.pca_dim, args.pca_bins,
                                4096, args.device)
        if args.model:
            model.save(args.model)
    compare_cli.finish("pca", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
