"""Free-energy surfaces of ensembles: Gaussian kernel density estimates of 1-D and 2-D projections, their sums computed
on the device (K22, ``cgv_kde_sums``; ``csrc/kde.hip``).

The reference draws its central figure offline in ``CoarseGrainingVAE/plots.py:61-84`` (``kernel_density_plot``):
``scipy.stats.gaussian_kde`` of (phi, psi) of alanine dipeptide or (IC1, IC2) of chignolin on a 300 x 300 grid, shown as
``log(density + 1e-3)``.  Here the estimator is the same one -- scipy's definition of the bandwidth matrix, restated in
``Kde`` -- but the ``N x M`` exponentials run on the device, periodic axes (torsions) are handled by minimum image instead
of being cut at +-pi, and the numbers a figure would only show are returned: the divergence of two surfaces, the RMS
difference of their free energies, and the held-out log-likelihood of generated structures under the data's density, each
with the noise floor between the even and the odd reference frames.  No figure is drawn.

The host centres, whitens and scales the coordinates in fp64 (``_Frame``): with ``H = L L^T`` and ``c = sqrt(log2(e) / 2)``,
``u = c L^-1 (x - mean)`` turns ``exp(-(x - y)^T H^-1 (x - y) / 2)`` into ``exp2(-|u_x - u_y|^2)``, which is all the kernel
computes.  Centring is what keeps the fp32 coordinates small: data at 1000 +- 1 loses nothing.

The host pieces shared with the other analyses (``js_divergence``, ``read_back``, ``workspace``) live in ``ensemble``.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ensemble, options, tica
from .distributions import TORSION, InternalCoords, feature_values, peptide_backbone_torsions
from .ensemble import js_divergence, read_back

WORKSPACE_BYTES = 1 << 26              # the points of a launch are cut until the ranges' partial sums fit this
SCALE = math.sqrt(0.5 * math.log2(math.e))
MAX_WIDTH_FRACTION = 1.0 / 12.0        # of the period: beyond the nearest image a kernel is below exp(-18)


def limits() -> Dict[str, int]:
    return ensemble.limits("kde", ("planes", "samples", "points", "splits"))


# ----------------------------------------------------------------------------- the launch
def kde_sums(samples: torch.Tensor, points: torch.Tensor, period: Optional[torch.Tensor] = None,
             workspace: Optional[torch.Tensor] = None):
    """One ``cgv_kde_sums`` call on device tensors: ``samples [P,N,d]``, ``points [P,M,d]`` fp32 (already whitened and
    scaled), ``period [P,d]`` fp32 or ``None``.  Returns ``(sums [P,M] fp64, n_skipped [P] int32)`` on the device.  The
    number of sample ranges is option ``kde_splits`` (0: the library's rule)."""
    if samples.dim() != 3 or points.dim() != 3 or samples.shape[2] not in (1, 2) or points.shape[2] != samples.shape[2] or \
            points.shape[0] != samples.shape[0]:
        raise ValueError(f"samples must be [P, N, d] and points [P, M, d] with d in (1, 2), got {tuple(samples.shape)} and {tuple(points.shape)}")
    if samples.dtype != torch.float32 or points.dtype != torch.float32:
        raise ValueError("samples and points must be float32")
    P, N, d, M = int(samples.shape[0]), int(samples.shape[1]), int(samples.shape[2]), int(points.shape[1])
    if period is not None and (tuple(period.shape) != (P, d) or period.dtype != torch.float32):
        raise ValueError(f"period must be float32 [{P}, {d}]")
    lim = limits()
    if P > lim["planes"] or N > lim["samples"] or M > lim["points"] or P * M > 2 ** 30:
        raise ValueError(f"{P} planes, {N} samples, {M} points in one launch (the kernel holds {lim['planes']}, {lim['samples']}, "
                         f"{lim['points']}, planes x points <= 2^30)")
    splits = int(options.get("kde_splits"))
    if not 0 <= splits <= lim["splits"]:
        raise ValueError(f"option kde_splits must be 0 (rule) or 1..{lim['splits']}")
    lib = _lib.load()
    used = splits if splits else int(lib.cgv_kde_splits(P, N, M))
    need = int(lib.cgv_kde_workspace_bytes(P, M, used))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = ensemble.workspace(max(need, 8), samples.device)
    sums = torch.empty((P, M), dtype=torch.float64, device=samples.device)
    skipped = torch.zeros(P, dtype=torch.int32, device=samples.device)
    if P:
        _lib.call("cgv_kde_sums", _lib.ptr(samples) if N else None, _lib.ptr(points) if M else None, _lib.ptr(period), P, N, M, d,
                  splits, _lib.ptr(sums) if M else None, _lib.ptr(skipped), _lib.ptr(workspace),
                  workspace.numel() * workspace.element_size(), _lib.stream_ptr(), tag="kde_sums")
    return sums, skipped


# ----------------------------------------------------------------------------- bandwidths and whitening (host, fp64)
def _array(x, what: str, d: Optional[int] = None) -> np.ndarray:
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[1] not in (1, 2) or (d is not None and a.shape[1] != d):
        raise ValueError(f"{what} must be [rows, d] with d = {d if d is not None else '1 or 2'}, got {a.shape}")
    return np.ascontiguousarray(a)


def _period(period, d: int) -> np.ndarray:
    """``period`` as fp64 ``[d]``, 0 where the axis is not periodic (``None``: no axis is; a scalar: every axis)."""
    if period is None:
        return np.zeros(d)
    p = np.asarray(period, dtype=np.float64).reshape(-1)
    if p.shape[0] == 1:
        p = np.repeat(p, d)
    if p.shape[0] != d or not np.isfinite(p).all() or (p < 0).any():
        raise ValueError(f"period must hold {d} finite numbers >= 0 (0: the axis is not periodic)")
    return p


def bandwidth_factor(bandwidth, n: int, d: int) -> float:
    """scipy's ``gaussian_kde.factor``: Scott ``n^(-1/(d+4))``, Silverman ``(n (d+2) / 4)^(-1/(d+4))``, or a positive number."""
    if isinstance(bandwidth, str):
        if bandwidth == "scott":
            return float(n) ** (-1.0 / (d + 4))
        if bandwidth == "silverman":
            return (n * (d + 2) / 4.0) ** (-1.0 / (d + 4))
        raise ValueError("bandwidth must be 'scott', 'silverman' or a positive number")
    f = float(bandwidth)
    if not (math.isfinite(f) and f > 0):
        raise ValueError("bandwidth must be 'scott', 'silverman' or a positive number")
    return f


def bandwidth_matrix(data: np.ndarray, bandwidth="scott", period=None) -> np.ndarray:
    """``H [d,d]`` of the data ``[N,d]``.  No periodic axis: scipy's ``factor^2 cov(data, ddof=1)``.  Any periodic axis:
    diagonal, the width of an axis ``factor`` x its standard deviation (``ddof=1``), of a periodic one ``factor`` x its
    circular standard deviation ``sqrt(-2 ln R) period / (2 pi)``."""
    n, d = data.shape
    per = _period(period, d)
    if n < 2:
        raise ValueError("a bandwidth needs at least two samples")
    if not np.isfinite(data).all():
        raise ValueError("the data holds non-finite values")
    f = bandwidth_factor(bandwidth, n, d)
    if not (per > 0).any():
        return f * f * np.atleast_2d(np.cov(data, rowvar=False, ddof=1))
    w = np.zeros(d)
    for a in range(d):
        if per[a] > 0:
            ang = 2.0 * math.pi * data[:, a] / per[a]
            R = math.hypot(np.cos(ang).mean(), np.sin(ang).mean())
            w[a] = f * math.sqrt(max(-2.0 * math.log(R), 0.0)) * per[a] / (2.0 * math.pi) if R > 0 else math.inf
        else:
            w[a] = f * data[:, a].std(ddof=1)
    return np.diag(w * w)


class _Frame:
    """Centre, whitening and scale of one plane: ``to_kernel(x)`` gives the fp32 coordinates the kernel takes."""

    def __init__(self, H: np.ndarray, centre: np.ndarray, period: np.ndarray):
        d = H.shape[0]
        if not np.isfinite(H).all():
            raise ValueError("the bandwidth matrix is not finite (a periodic axis without a mean direction?)")
        if (period > 0).any() and np.abs(H - np.diag(np.diag(H))).max() > 0:
            raise ValueError("a plane with a periodic axis needs a diagonal bandwidth matrix")
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            L = None
        if L is None or not (np.diag(L) > 0).all() or not np.isfinite(np.linalg.inv(L)).all():
            raise ValueError("the bandwidth matrix is singular: the data has no spread along some direction")
        for a in range(d):
            if period[a] > 0 and L[a, a] > MAX_WIDTH_FRACTION * period[a]:
                raise ValueError(f"axis {a}: kernel width {L[a, a]:.4g} exceeds period / 12 = {period[a] / 12:.4g}: the minimum "
                                 "image is no longer the only one that counts")
        self.d, self.H, self.centre, self.period = d, H, centre, period
        self.A = SCALE * np.linalg.inv(L)                        # u = A (x - centre)
        self.det = float(np.prod(np.diag(L)) ** 2)
        diag = np.diag(self.A)
        self.kernel_period = np.where(period > 0, period * diag, 0.0).astype(np.float32)

    def to_kernel(self, x: np.ndarray) -> np.ndarray:
        y = x - self.centre[None, :]
        for a in range(self.d):
            if self.period[a] > 0:
                y[:, a] -= self.period[a] * np.rint(y[:, a] / self.period[a])
        return np.ascontiguousarray((y @ self.A.T).astype(np.float32))


def _centre(data: np.ndarray, period: np.ndarray) -> np.ndarray:
    c = data.mean(0)
    for a in range(data.shape[1]):
        if period[a] > 0:
            ang = 2.0 * math.pi * data[:, a] / period[a]
            c[a] = math.atan2(np.sin(ang).mean(), np.cos(ang).mean()) * period[a] / (2.0 * math.pi)
    return c


class Kde:
    """A Gaussian kernel density estimate of ``data [N,d]``, ``d`` 1 or 2 (a 1-D array is ``[N,1]``).

    ``bandwidth``: ``"scott"``, ``"silverman"`` or a number, scipy's ``factor``; ``H`` is ``bandwidth_matrix``.  Without
    periodic axes the estimate is ``scipy.stats.gaussian_kde(data.T, bw_method=bandwidth)``.  ``period``: ``None``, a
    number or one per axis, 0 for an axis that is not periodic; a periodic axis forces a diagonal ``H`` and its kernel
    width must not exceed ``period / 12`` (``ValueError``): at that width the nearest neglected image is at least six
    widths away and adds at most ``exp(-18)`` of a kernel's peak.  ``H=`` gives the matrix itself, for a second data
    set that is to be smoothed exactly as a first one.  ``ValueError``: fewer than two samples, non-finite data,
    ``d`` not 1 or 2, a singular ``H``."""

    def __init__(self, data, bandwidth="scott", period=None, H=None, device="cuda"):
        x = _array(data, "data")
        self.n, self.d = int(x.shape[0]), int(x.shape[1])
        self.period = _period(period, self.d)
        if self.n < 2:
            raise ValueError("a density estimate needs at least two samples")
        if not np.isfinite(x).all():
            raise ValueError("the data holds non-finite values")
        if H is None:
            H = bandwidth_matrix(x, bandwidth, self.period)
        H = np.asarray(H, dtype=np.float64).reshape(self.d, self.d)
        self.frame = _Frame(H, _centre(x, self.period), self.period)
        self.H, self.device = H, device
        self.samples = self.frame.to_kernel(x)
        self.norm = self.n * (2.0 * math.pi) ** (self.d / 2.0) * math.sqrt(self.frame.det)

    def evaluate(self, points) -> np.ndarray:
        """The density at ``points [M,d]``: fp64 ``[M]``."""
        return _evaluate_many([self], [points])[0]

    __call__ = evaluate

    def logpdf(self, points) -> np.ndarray:
        with np.errstate(divide="ignore"):
            return np.log(self.evaluate(points))

    def grid(self, ranges, n_grid: int = 100):
        """``(axes, density)``: ``axes[a]`` are ``n_grid`` nodes over ``ranges[a] = (lo, hi)`` -- both ends included,
        as the reference's ``mgrid``; on a periodic axis ``hi`` is left out, it is ``lo`` again -- and ``density`` has
        shape ``[n_grid] * d``, first axis first."""
        axes = grid_axes(ranges, n_grid, self.period)
        return axes, self.evaluate(grid_nodes(axes)).reshape((int(n_grid),) * self.d)


def grid_axes(ranges, n_grid: int, period) -> List[np.ndarray]:
    r = np.asarray(ranges, dtype=np.float64).reshape(-1, 2)
    if int(n_grid) < 2 or not np.isfinite(r).all() or (r[:, 0] >= r[:, 1]).any():
        raise ValueError("ranges must be finite (lo, hi) with lo < hi per axis, n_grid at least 2")
    per = _period(period, r.shape[0])
    return [np.linspace(lo, hi, int(n_grid), endpoint=not per[a] > 0) for a, (lo, hi) in enumerate(r)]


def grid_nodes(axes: Sequence[np.ndarray]) -> np.ndarray:
    return np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")], axis=1)


def _evaluate_many(kdes: Sequence[Kde], points_list: Sequence) -> List[np.ndarray]:
    """The densities of ``kdes[p]`` at ``points_list[p]``.  Planes of one ``d`` share launches: samples are padded to the
    longest plane with NaN rows (the kernel skips them) and points with zeros, the points are cut into chunks whose
    partial sums fit ``WORKSPACE_BYTES``; ONE read-back."""
    if len(kdes) != len(points_list):
        raise ValueError("one set of points per plane")
    pts = [_array(q, "points", k.d) for k, q in zip(kdes, points_list)]
    out: List[Optional[np.ndarray]] = [None] * len(kdes)
    lib, lim = _lib.load(), limits()
    pending = []
    for d in (1, 2):
        ids = [i for i, k in enumerate(kdes) if k.d == d]
        for at in range(0, len(ids), lim["planes"]):
            group = ids[at:at + lim["planes"]]
            dev = torch.device(kdes[group[0]].device)
            P, N, M = len(group), max(kdes[i].n for i in group), max(pts[i].shape[0] for i in group)
            S = np.full((P, N, d), np.nan, dtype=np.float32)
            Q = np.zeros((P, M, d), dtype=np.float32)
            W = np.zeros((P, d), dtype=np.float32)
            for row, i in enumerate(group):
                S[row, :kdes[i].n] = kdes[i].samples
                Q[row, :pts[i].shape[0]] = kdes[i].frame.to_kernel(pts[i].copy())
                W[row] = kdes[i].frame.kernel_period
            periodic = bool((W > 0).any())
            pack = torch.from_numpy(np.concatenate([S.reshape(-1), Q.reshape(-1), W.reshape(-1)])).to(dev)
            s_t, q_t = pack[:S.size].reshape(P, N, d), pack[S.size:S.size + Q.size].reshape(P, M, d)
            w_t = pack[S.size + Q.size:].reshape(P, d) if periodic else None
            forced = int(options.get("kde_splits"))
            step = max(M, 1)
            while step > 1024 and int(lib.cgv_kde_workspace_bytes(P, step, forced or int(lib.cgv_kde_splits(P, N, step)))) > WORKSPACE_BYTES:
                step = ((step + 1) // 2 + 1023) // 1024 * 1024
            parts = []
            for start in range(0, M, step):
                chunk = q_t[:, start:start + step].contiguous()
                parts.append(kde_sums(s_t, chunk, w_t)[0])
            sums = torch.cat(parts, dim=1) if parts else torch.zeros((P, 0), dtype=torch.float64, device=dev)
            pending.append((group, sums))
    back = read_back([s for _, s in pending]) if pending else []
    for (group, _), sums in zip(pending, back):
        for row, i in enumerate(group):
            out[i] = sums[row, :pts[i].shape[0]] / kdes[i].norm
    return out


def kde_many(list_of_data, list_of_points, bandwidth="scott", period=None, device="cuda") -> List[np.ndarray]:
    """``[Kde(data, bandwidth, period).evaluate(points) for data, points in zip(...)]`` with all planes of one ``d`` in
    ONE ``cgv_kde_sums`` launch per chunk of points (``period``: ``None``, or one entry per plane)."""
    periods = [None] * len(list_of_data) if period is None else list(period)
    if len(periods) != len(list_of_data) or len(list_of_points) != len(list_of_data):
        raise ValueError("one set of points (and one period, when given) per plane")
    return _evaluate_many([Kde(x, bandwidth, p, device=device) for x, p in zip(list_of_data, periods)], list_of_points)


# ----------------------------------------------------------------------------- host statistics
def free_energy(density, eps: float = 1e-3) -> np.ndarray:
    """``-log(density + eps)`` in kT: the reference plots ``log(density + 1e-3)``, the same surface upside down."""
    return -np.log(np.asarray(density, dtype=np.float64) + float(eps))


def _number(v) -> Optional[float]:
    return float(v) if v is not None and np.isfinite(v) else None


def _default_ranges(ref: np.ndarray, period: np.ndarray) -> List[List[float]]:
    out = []
    for a in range(ref.shape[1]):
        if period[a] > 0:
            out.append([-0.5 * period[a], 0.5 * period[a]])
        else:
            lo, hi = float(ref[:, a].min()), float(ref[:, a].max())
            pad = 0.05 * (hi - lo) if hi > lo else 0.5
            out.append([lo - pad, hi + pad])
    return out


def plane_stats(dens: Dict[str, np.ndarray], loglik_gen, loglik_floor, fe_window: float = 6.0, eps: float = 1e-3) -> dict:
    """The statistics of ``compare_planes`` from the four node densities ``dens["ref" | "gen" | "even" | "odd"]`` and the
    two mean log-likelihoods -- pure host."""
    f = {k: free_energy(v, eps) for k, v in dens.items()}
    near = f["ref"] <= f["ref"].min() + float(fe_window)
    rms = lambda a, b: float(np.sqrt(np.mean((a[near] - b[near]) ** 2)))
    return {"jsd": js_divergence(dens["ref"], dens["gen"]), "floor": js_divergence(dens["even"], dens["odd"]),
            "fe_rmse": rms(f["gen"], f["ref"]), "fe_floor": rms(f["even"], f["odd"]), "fe_nodes": int(near.sum()),
            "loglik_gen": _number(loglik_gen), "loglik_floor": _number(loglik_floor)}


def _compare_many(refs: Sequence[np.ndarray], gens: Sequence[np.ndarray], n_grid, bandwidth, periods, ranges_list, fe_window,
                  device) -> List[dict]:
    """``compare_planes`` of several planes at once: every estimate of all planes is one batched launch per chunk."""
    P = len(refs)
    for r, g in zip(refs, gens):
        if r.shape[0] < 4 or g.shape[0] < 2:
            raise ValueError("at least four reference rows (the floor compares the even with the odd ones) and two generated")
        if not np.isfinite(g).all():
            raise ValueError("the generated data holds non-finite values")
    whole = [Kde(r, bandwidth, per, device=device) for r, per in zip(refs, periods)]
    same = lambda x, p: Kde(x, period=periods[p], H=whole[p].H, device=device)
    gen = [same(g, p) for p, g in enumerate(gens)]
    even, odd = [same(r[0::2], p) for p, r in enumerate(refs)], [same(r[1::2], p) for p, r in enumerate(refs)]
    ranges = [rg if rg is not None else _default_ranges(r, k.period) for rg, r, k in zip(ranges_list, refs, whole)]
    axes = [grid_axes(rg, n_grid, k.period) for rg, k in zip(ranges, whole)]
    nodes = [grid_nodes(a) for a in axes]
    dens = {name: _evaluate_many(ks, nodes) for name, ks in (("ref", whole), ("gen", gen), ("even", even), ("odd", odd))}
    with np.errstate(divide="ignore"):
        ll_gen = [float(np.log(v).mean()) for v in _evaluate_many(whole, gens)]
        ll_floor = [float(np.log(v).mean()) for v in _evaluate_many(even, [r[1::2] for r in refs])]
    out = []
    for p in range(P):
        mine = {k: v[p] for k, v in dens.items()}
        shape = (int(n_grid),) * whole[p].d
        out.append({**plane_stats(mine, ll_gen[p], ll_floor[p], fe_window), "n_ref": int(refs[p].shape[0]), "n_gen": int(gens[p].shape[0]),
                    "n_grid": int(n_grid), "fe_window": float(fe_window), "bandwidth": whole[p].H.tolist(),
                    "period": whole[p].period.tolist(), "ranges": [[float(lo), float(hi)] for lo, hi in ranges[p]],
                    "density": {"ref": mine["ref"].reshape(shape).tolist(), "gen": mine["gen"].reshape(shape).tolist()}})
    return out


def compare_planes(ref, gen, n_grid: int = 100, bandwidth="scott", period=None, ranges=None, fe_window: float = 6.0,
                   device="cuda") -> dict:
    """Generated rows ``gen [Ng,d]`` against reference rows ``ref [Nr,d]`` of one projection, as smooth densities.  ONE
    bandwidth matrix, fitted on the whole reference, serves four estimates on one grid of ``n_grid`` nodes per axis:
    the reference, the generated rows, the even and the odd reference rows.  ``ranges`` default to the full period
    ``[-period / 2, period / 2)`` on a periodic axis and to the reference's min / max widened by 5 % of the span
    otherwise (as ``tica.compare``).  Returns a dict that ``json.dump`` takes:

      jsd, floor      ``distributions.js_divergence`` (base 2) of the node densities: generated against reference, and
                      even against odd reference rows -- what ``jsd`` is to be read against
      fe_rmse, fe_floor, fe_nodes   RMS difference of ``free_energy`` over the nodes within ``fe_window`` kT of the
                      reference's minimum (generated against reference; even against odd), and how many nodes that is
      loglik_gen      mean log density of the generated rows under the reference's estimate
      loglik_floor    mean log density of the odd reference rows under the even rows' estimate, same ``H``
                      (``None`` for a mean that is not finite: some row sits where the estimate underflows)
      n_ref, n_gen, n_grid, fe_window, bandwidth (``H``), period, ranges, density {ref, gen} ``[n_grid] * d``
    """
    r = _array(ref, "ref")
    g = _array(gen, "gen", r.shape[1])
    return _compare_many([r], [g], n_grid, bandwidth, [period], [ranges], fe_window, device)[0]


PLANE_STATS_KEYS = ("jsd", "floor", "fe_rmse", "fe_floor", "fe_nodes", "loglik_gen", "loglik_floor", "n_ref", "n_gen", "n_grid",
                    "fe_window", "bandwidth", "period", "ranges", "density")
_SHORT = ("jsd", "floor", "fe_rmse", "fe_floor", "fe_nodes", "loglik_gen", "loglik_floor")


def _means(planes: Sequence[dict]) -> dict:
    def mean(key):
        v = [p[key] for p in planes if p[key] is not None]
        return float(np.mean(v)) if v else None
    return {k: mean(k) for k in _SHORT if k != "fe_nodes"}


def torsion_pairs(z, bonds):
    """``(coords, rows)``: the backbone torsions of a peptide as a feature table of their own, and the (phi row, psi row)
    of every residue that has both (``distributions.peptide_backbone_torsions``)."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    phi, psi, pairs = peptide_backbone_torsions(z, bonds)
    if not pairs:
        raise ValueError("the molecule has no peptide backbone: no (phi, psi) pair to compare")
    feat = np.array(list(phi) + list(psi), dtype=np.int32).reshape(-1, 4)
    coords = InternalCoords(feat, np.full(feat.shape[0], TORSION, dtype=np.int32), np.zeros((0, 2), np.int32), int(z.shape[0]))
    return coords, [(a, len(phi) + b) for a, b in pairs]


def compare_torsions(ref_xyz, gen_xyz, z, bonds, n_grid: int = 100, bandwidth="scott", fe_window: float = 6.0,
                     structures_per_launch: int = 16384, device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` in every (phi, psi) plane
    of the peptide ``z [n]`` / ``bonds [Eb,2]``: the torsions come from ``distributions.feature_values``, both axes have
    period 2 pi, and every estimate of all planes is one batched launch.  Structures with an invalid torsion (a
    non-finite coordinate) are left out and counted.  Returns a dict that ``json.dump`` takes: ``plane`` (``"torsion"``),
    ``n_ref``, ``n_gen``, ``n_bad_ref``, ``n_bad_gen``, ``pairs`` (a ``compare_planes`` dict per residue, with the ``phi``
    and ``psi`` atoms) and ``mean`` (the means of jsd, floor, fe_rmse, fe_floor, loglik_gen, loglik_floor over the
    pairs).  ``ValueError``: no peptide backbone."""
    coords, rows = torsion_pairs(z, bonds)
    kw = dict(structures_per_launch=structures_per_launch, device=device)
    tr, tg = feature_values(ref_xyz, coords, **kw), feature_values(gen_xyz, coords, **kw)
    good_r, good_g = np.isfinite(tr).all(1), np.isfinite(tg).all(1)
    tr, tg = tr[good_r], tg[good_g]
    P = len(rows)
    per = [2.0 * math.pi, 2.0 * math.pi]
    planes = _compare_many([tr[:, list(r)] for r in rows], [tg[:, list(r)] for r in rows], n_grid, bandwidth, [per] * P, [None] * P,
                           fe_window, device)
    for plane, (a, b) in zip(planes, rows):
        plane["phi"], plane["psi"] = list(coords.atoms(a)), list(coords.atoms(b))
    return {"plane": "torsion", "n_ref": int(good_r.shape[0]), "n_gen": int(good_g.shape[0]), "n_bad_ref": int((~good_r).sum()),
            "n_bad_gen": int((~good_g).sum()), "pairs": planes, "mean": _means(planes)}


def compare_tica(ref_trajs, gen_xyz, z, bonds, lag: int = 100, n_grid: int = 100, bandwidth="scott", fe_window: float = 6.0,
                 sel=None, excluded_neighbors: int = 2, device="cuda") -> dict:
    """Generated structures against the time-ordered reference segments ``ref_trajs`` (a list of ``[T_i,n,3]``) in the
    plane of the reference's two slowest independent components (``tica.fit`` / ``tica.project`` as ``tica.compare``
    uses them), then ``compare_planes``.  The result carries ``plane`` (``"tica"``), ``lag``, ``eigenvalues`` and, like
    ``compare_torsions``, a one-entry ``pairs`` and ``mean``."""
    segs = [tica.frames(x) for x in ref_trajs]
    z = np.asarray(z).astype(np.int64).reshape(-1)
    if sel is None:
        sel = tica.backbone_atoms(z, bonds)
        if sel.shape[0] == 0:
            raise ValueError("the molecule has no peptide backbone: pass the atoms to use as sel")
    model = tica.fit(segs, tica.distance_pairs(sel, excluded_neighbors), lag, dim=2, device=device)
    ref = torch.cat([s.detach().cpu() for s in segs]) if len(segs) > 1 else segs[0]
    ics_ref, ics_gen = tica.project(ref, model, device=device), tica.project(tica.frames(gen_xyz), model, device=device)
    if ics_ref.shape[1] < 2:
        raise ValueError("the TICA model has one component: there is no (IC1, IC2) plane")
    good = np.isfinite(ics_gen[:, :2]).all(1)
    plane = compare_planes(ics_ref[:, :2], ics_gen[good, :2], n_grid=n_grid, bandwidth=bandwidth, fe_window=fe_window, device=device)
    return {"plane": "tica", "lag": int(lag), "eigenvalues": model.eigenvalues.tolist(), "n_ref": int(ics_ref.shape[0]),
            "n_gen": int(ics_gen.shape[0]), "n_bad_ref": 0, "n_bad_gen": int((~good).sum()), "pairs": [plane], "mean": _means([plane])}


KDE_STATS_KEYS = ("plane", "n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "pairs", "mean")


def summary_of(stats: dict) -> dict:
    """What the command-line tools put under ``"kde_stats"`` in their JSON summary line: no densities, no grids."""
    return {"plane": stats["plane"], "n_ref": stats["n_ref"], "n_gen": stats["n_gen"], "n_bad_ref": stats["n_bad_ref"],
            "n_bad_gen": stats["n_bad_gen"], "n_pairs": len(stats["pairs"]), "mean": stats["mean"],
            "pairs": [{k: p[k] for k in _SHORT} for p in stats["pairs"]]}
