"""Whether a generated ensemble SCATTERS like the data: the small-angle X-ray scattering profile I(q) of every structure and
of the ensemble, the observable that coarse-grained and disordered-protein ensembles are most often judged against, with the
real-space quantities that go with it -- the weighted P(r), Rg, Dmax, I(0).  The device produces exact integers only, a
weighted distance histogram PER STRUCTURE (K33, ``cgv_saxs_hist``; ``csrc/saxs_hist.hip``); every transcendental function
stays here, on the host, in fp64 -- the route of FoXS and CRYSOL-style codes.  ``pairdist`` (K29) cannot serve: it sums over
the ensemble, counts without weights, stops at 256 bins and leaves bonded neighbours out.

Forward model: point scatterers with contrast weights.

    w_i = Z_i + nH_i - rho0 * v_i          the default weight of a selected atom (``weights_of``); a caller may pass its own
      nH_i   the hydrogens bonded to atom i, folded into it when the selection holds no hydrogen (``heavy``); 0 for ``all``
      rho0   the solvent's electron density, 0.334 e / A^3 (water); 0 gives the in-vacuo curve
      v_i    the displaced volume ``DISPLACED_VOLUME[Z_i]`` (plus ``nH_i`` times hydrogen's when hydrogens are folded in)
    wq_i = rint(w_i * 16)                  fixed point (``quantise``); |wq_i| <= 32767, else ``ValueError``

The q-dependence of the atomic form factors is NOT modelled: every atom scatters as at q = 0, which is customary at small
angles, q up to about 0.3 / A, and overestimates the intensity beyond (by some 10 % at q = 0.5 / A for carbon).  An optional
``modulation(q)`` multiplies I(q) (default 1): a common Gaussian form-factor fall-off goes there.  No hydration shell.

Histogram, for structure ``s`` over EVERY pair ``i < j`` of the selection (scattering counts bonded neighbours too), in fp32
with every operation rounded on its own -- K29's bin rule unchanged (``pairdist``):

    rmax2 = fp32(r_max) * fp32(r_max)                  scale = fp32(float64(n_bins) / float64(fp32(r_max)))
    q = (dx*dx + dy*dy) + dz*dz  of x_i - x_j          in range  iff  q < rmax2  (strict)
    b = min(int(sqrtf(q) * scale), n_bins - 1)
    in range:  H_s[b] += wq_i * wq_j                   otherwise:  beyond_s += 1  (a count of pairs, whatever their weights)

``restate`` reproduces every integer in ``numpy.float32``; two calls give the same bits however the structures are cut into
launches.  A structure with a non-finite selected coordinate is *bad* and enters no sum.  From the integers, fp64:

    I_s(q) = modulation(q) * [sum_i wq_i^2 + 2 sum_b H_s[b] * sinc(q * r_b)] / 256         r_b = (b + 1/2) * r_max / n_bins
    P_s(r_b) = H_s[b] / 256 / width        Rg_s^2 = sum_b H_s[b] r_b^2 / (sum_i wq_i)^2 (``None`` when sum_i wq_i = 0)
    Dmax_s = the upper edge of the last non-zero bin                    I_s(0) = [sum_i wq_i^2 + 2 sum_b H_s[b]] / 256

The binning is the only approximation: ``|sinc'| <= 0.4362`` and ``|r - r_b| <= width / 2``, so a profile differs from the
Debye sum over the same weights by at most ``0.4362 * q * width * sum_{i<j} |wq_i wq_j| / 256``.  A structure with
``beyond_s != 0`` has an incomplete profile: it is counted, left out of the means, and ``compare`` refuses a reference that
has one.  The profile is analytic in q given ``H``: a model is evaluated AT an experiment's q values, nothing is interpolated.

    python -m coarsegrainingvae_amd.saxs -gen samples.npz -ref traj.npz [-top top.npz] [-saxs_atoms heavy|all]
        [-saxs_solvent 0.334] [-saxs_rmax R] [-saxs_bin 0.1] [-saxs_qmax 0.5] [-saxs_nq 101] [-saxs_exp curve.dat]
        [-saxs_units A|nm] [-profiles profiles.npz] [-out saxs_stats.json]

``z`` and ``bonds`` come from ``-top``, else from ``-ref``.  Without ``-saxs_rmax``, ``r_max`` is twice the largest distance
of a selected atom of the reference from its structure's centroid, rounded up to the next bin.  ``curve.dat`` is text with the
columns q, I, sigma and ``#`` comments, q in 1 / A (``-saxs_units nm``: in 1 / nm).  The full statistics of ``compare`` go to
``-out``, one JSON line with ``"saxs_stats": summary_of(...)`` to stdout.
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .contacts import cutoff2_of
from .ensemble import device_of, read_back, select_atoms, structures
from .pairdist import scale_of

RHO0 = 0.334                 # e / A^3: the electron density of water
FIXED = 16                   # the fixed point of a weight: wq = rint(w * 16); I and P(r) carry 1 / 256
MAX_WEIGHT = 32767           # |wq| at most: cgv_saxs_max_weight() (tests/test_saxs_cpu.py holds the two together)
SINC_SLOPE = 0.4362          # max |d sinc(x) / dx|, at x = 2.0816
# Displaced volumes in A^3 by atomic number.  Source: the Fraser-MacRae-Suzuki (J. Appl. Cryst. 11, 693, 1978) values that
# CRYSOL uses (Svergun, Barberato & Koch, J. Appl. Cryst. 28, 768, 1995), QUOTED FROM MEMORY -- no copy was at hand to
# confirm them; check them against the papers before relying on an absolute contrast.  No test depends on the values.
DISPLACED_VOLUME = {1: 5.15, 6: 16.44, 7: 2.49, 8: 9.13, 16: 19.86}


def limits() -> Dict[str, int]:
    return ensemble.limits("saxs", ("structures", "atoms", "bins", "weight"))


# ----------------------------------------------------------------------------- host: weights
def weights_of(z, bonds, sel, solvent: float = RHO0, fold_h: Optional[bool] = None) -> np.ndarray:
    """The contrast weights ``[m]`` fp64 of the selected atoms ``sel`` of the molecule ``z [n]`` / ``bonds [Eb,2]``:
    ``Z + nH - solvent * v``.  ``fold_h`` (default: when the selection holds no hydrogen): the hydrogens bonded to a selected
    atom and not selected themselves are folded into it -- their electron and their displaced volume.  ``solvent = 0`` gives
    electron counts and reads no volume; otherwise an element without an entry in ``DISPLACED_VOLUME`` is a ``ValueError``."""
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    n = zz.shape[0]
    s = ensemble.selection(sel, n, purpose="weigh").astype(np.int64)
    rho = float(solvent)
    if not (math.isfinite(rho) and rho >= 0):
        raise ValueError(f"solvent must be a finite electron density >= 0, got {solvent}")
    fold = bool((zz[s] != 1).all()) if fold_h is None else bool(fold_h)
    n_h = np.zeros(n, dtype=np.int64)
    if fold:
        inside = np.zeros(n, dtype=bool)
        inside[s] = True
        for a, nbrs in enumerate(ensemble.adjacency(n, bonds)):
            n_h[a] = sum(1 for b in nbrs if zz[b] == 1 and not inside[b])
    w = (zz[s] + n_h[s]).astype(np.float64)
    if rho > 0:
        needed = set(int(v) for v in zz[s]) | ({1} if n_h[s].any() else set())
        missing = sorted(needed - set(DISPLACED_VOLUME))
        if missing:
            raise ValueError(f"no displaced volume for Z = {missing}: pass weights, or solvent=0")
        vol = np.array([DISPLACED_VOLUME[int(v)] for v in zz[s]], dtype=np.float64) + n_h[s] * DISPLACED_VOLUME.get(1, 0.0)
        w = w - rho * vol
    return w


def quantise(weights) -> np.ndarray:
    """``rint(w * 16)`` as int32 ``[m]``; ``ValueError`` for a weight that is not finite or whose fixed point passes 32767."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if not np.isfinite(w).all():
        raise ValueError("a weight is not finite")
    wq = np.rint(w * FIXED)
    if wq.size and np.abs(wq).max() > MAX_WEIGHT:
        k = int(np.argmax(np.abs(wq)))
        raise ValueError(f"weight {k} = {w[k]:g} is out of range: |w| * {FIXED} must not pass {MAX_WEIGHT}")
    return np.ascontiguousarray(wq.astype(np.int32))


def _fixed(wq, m: int) -> np.ndarray:
    """The caller's fixed-point weights as int32 ``[m]``, in range."""
    a = np.asarray(wq).reshape(-1)
    if a.shape[0] != m or a.dtype.kind not in "iu":
        raise ValueError(f"wq must be {m} integers (quantise)")
    if a.size and np.abs(a.astype(np.int64)).max() > MAX_WEIGHT:
        raise ValueError(f"a fixed-point weight is out of range: |wq| must not pass {MAX_WEIGHT}")
    return np.ascontiguousarray(a.astype(np.int32))


def _tables(x, sel, wq, r_max, n_bins):
    """What ``saxs_hist`` and ``restate`` check alike, before a device is touched: ``(sel, wq, n_bins, scale, rmax2)``."""
    n = int(x.shape[1])
    scale, rmax2 = scale_of(r_max, n_bins if int(n_bins) >= 1 else 1), cutoff2_of(r_max)
    table = ensemble.selection(sel, n, purpose="weigh")
    w = _fixed(wq, int(table.shape[0]))
    lim = limits()
    if not 1 <= int(n_bins) <= lim["bins"]:
        raise ValueError(f"n_bins must be in 1..{lim['bins']}, got {n_bins}")
    if int(table.shape[0]) > lim["atoms"]:
        raise ValueError(f"the selection lists {table.shape[0]} atoms (the kernel holds {lim['atoms']})")
    return table, w, int(n_bins), scale_of(r_max, n_bins), rmax2


def _result(hist, beyond, bad, table, w, r_max, nb, scale, rmax2, into) -> dict:
    bad = np.asarray(bad).astype(bool)
    if into is not None:
        hist = np.concatenate([np.asarray(into["hist"], dtype=np.int64), hist])
        beyond = np.concatenate([np.asarray(into["beyond"], dtype=np.int64), beyond])
        bad = np.concatenate([np.asarray(into["bad"], dtype=bool), bad])
    w64 = w.astype(np.int64)
    return {"hist": hist, "beyond": beyond, "bad": bad, "n_good": int((~bad).sum()), "self_term": int((w64 * w64).sum()),
            "wq_sum": int(w64.sum()), "sel": table, "wq": w, "r_max": float(np.float32(r_max)), "n_bins": nb, "rmax2": rmax2, "scale": scale}


def _same_tables(into, table, w, r_max, nb) -> None:
    if into is not None and not (np.array_equal(into["sel"], table) and np.array_equal(into["wq"], w) and int(into["n_bins"]) == nb
                                 and float(into["r_max"]) == float(np.float32(r_max))):
        raise ValueError("into was made with another selection, other weights or other bins")


# ----------------------------------------------------------------------------- the launches
def saxs_hist(xyz, sel, wq, r_max: float, n_bins: int, into: Optional[dict] = None, chunk: int = 4096, device="cuda", split: int = 0) -> dict:
    """The weighted distance histogram of every structure of ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a
    device tensor decides the device) over the selection ``sel [m]`` (unique atoms) with the fixed-point weights ``wq [m]``
    (``quantise``).  Host arrays:

      hist [S, n_bins] int64     H_s[b]: the sum of wq_i * wq_j over the in-range pairs i < j of structure s; 0 for a bad one
      beyond [S] int64           the pairs at ``r_max`` or farther: a structure with one has an incomplete profile
      bad [S] bool, n_good       structures with a non-finite selected coordinate, and the number of the others
      self_term, wq_sum          sum_i wq_i^2 and sum_i wq_i (Python ints; the same for every structure)
      sel, wq, r_max (as fp32 holds it), n_bins, rmax2, scale (what the kernel took, fp32)

    The structures go through in launches of ``chunk`` (``ensemble.chunks``); the tables stay on the device; ONE read-back.
    ``into``: an earlier result with the same tables, whose rows come first -- a long ensemble may be fed in pieces, to the
    same integers as in one call.  ``split``: blocks per structure (0: the library decides; for tests and measurements, the
    result does not depend on it).  Everything that can be refused is a ``ValueError`` before any launch."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    table, w, nb, scale, rmax2 = _tables(x, sel, wq, r_max, n_bins)
    _same_tables(into, table, w, r_max, nb)
    lim = limits()
    if not 1 <= int(chunk) <= lim["structures"]:
        raise ValueError(f"chunk must be in 1..{lim['structures']}, got {chunk}")
    if int(split) < 0:
        raise ValueError("split must be >= 0")
    m = int(table.shape[0])
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(chunk, lim["structures"], 16 * m)
    out = {"hist": torch.zeros(S, nb, dtype=torch.int64, device=dev), "beyond": torch.zeros(S, dtype=torch.int64, device=dev),
           "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if S:
        lib = _lib.load()
        d_sel, d_wq = torch.from_numpy(table).to(dev), torch.from_numpy(w).to(dev)
        need = int(lib.cgv_saxs_workspace_bytes(min(M, S), m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        for start, part in ensemble.chunks(x, M, dev):
            k = int(part.shape[0])
            _lib.call("cgv_saxs_hist", _lib.ptr(part), _lib.ptr(d_sel), _lib.ptr(d_wq), k, n, m, nb, float(rmax2), float(scale), int(split),
                      _lib.ptr(out["hist"][start:start + k]), _lib.ptr(out["beyond"][start:start + k]), _lib.ptr(out["bad"][start:start + k]),
                      _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), tag="saxs_hist")
    hist, beyond, bad = read_back([out["hist"], out["beyond"], out["bad"]])
    return _result(hist, beyond, bad, table, w, r_max, nb, scale, rmax2, into)


def restate(xyz, sel, wq, r_max: float, n_bins: int, into: Optional[dict] = None) -> dict:
    """``saxs_hist`` restated in ``numpy.float32``, every operation rounded on its own -- all pairs of a structure at once,
    no tiles, no LDS -- to the same integers and the same keys.  Test infrastructure, and the definition in executable form."""
    x = np.asarray(xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else xyz, dtype=np.float32)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"structures must be [S, n, 3], got {x.shape}")
    table, w, nb, scale, rmax2 = _tables(x, sel, wq, r_max, n_bins)
    _same_tables(into, table, w, r_max, nb)
    S, m = x.shape[0], table.shape[0]
    i, j = np.triu_indices(m, 1)
    ww = w.astype(np.int64)[i] * w.astype(np.int64)[j]
    hist, beyond, bad = np.zeros((S, nb), dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=bool)
    for s in range(S):
        p = x[s, table]
        if not np.isfinite(p).all():
            bad[s] = True
            continue
        with np.errstate(over="ignore"):
            dx, dy, dz = p[i, 0] - p[j, 0], p[i, 1] - p[j, 1], p[i, 2] - p[j, 2]
            q = (dx * dx + dy * dy) + dz * dz
            inside = q < rmax2
            t = np.sqrt(q[inside]) * scale
        assert q.dtype == np.float32 and t.dtype == np.float32
        np.add.at(hist[s], np.minimum(t.astype(np.int64), nb - 1), ww[inside])
        beyond[s] = int((~inside).sum())
    return _result(hist, beyond, bad, table, w, r_max, nb, scale, rmax2, into)


# ----------------------------------------------------------------------------- host: from the integers, fp64
def centres(r_max: float, n_bins: int) -> np.ndarray:
    """``r_b = (b + 1/2) * r_max / n_bins``."""
    return (np.arange(int(n_bins), dtype=np.float64) + 0.5) * (float(r_max) / int(n_bins))


def _q(q) -> np.ndarray:
    qq = np.asarray(q, dtype=np.float64).reshape(-1)
    if not (np.isfinite(qq).all() and (qq >= 0).all()):
        raise ValueError("q must be finite and >= 0")
    return qq


def profile(hist, self_term, q, r_max: float, modulation: Optional[Callable] = None) -> np.ndarray:
    """``I(q) = modulation(q) * [self_term + 2 sum_b H[b] sinc(q r_b)] / 256`` for ``hist [n_bins]`` (``[n_q]``) or
    ``hist [S, n_bins]`` (``[S, n_q]``); ``hist`` may hold fp64 means of histograms.  ``q`` in 1 / A."""
    h = np.asarray(hist, dtype=np.float64)
    qq = _q(q)
    kernel = np.sinc(np.outer(centres(r_max, h.shape[-1]), qq) / np.pi)          # numpy's sinc is sin(pi x) / (pi x)
    out = (float(self_term) + 2.0 * (h @ kernel)) / float(FIXED * FIXED)
    if modulation is not None:
        out = out * np.asarray(modulation(qq), dtype=np.float64).reshape(-1)
    return out


def i_zero(hist, self_term) -> np.ndarray:
    """``I(0) = [self_term + 2 sum_b H[b]] / 256``: ``(sum_i wq_i)^2 / 256`` for a complete histogram."""
    return (float(self_term) + 2.0 * np.asarray(hist, dtype=np.float64).sum(-1)) / float(FIXED * FIXED)


def pr(hist, r_max: float) -> dict:
    """``{"r": bin centres, "p": H / 256 / width}``: the weighted pair-distance density; ``sum(p) * width`` is
    ``sum_{i<j} w_i w_j``."""
    h = np.asarray(hist, dtype=np.float64)
    width = float(r_max) / h.shape[-1]
    return {"r": centres(r_max, h.shape[-1]), "width": width, "p": h / float(FIXED * FIXED) / width}


def rg(hist, wq_sum, r_max: float):
    """The real-space radius of gyration ``sqrt(sum_b H[b] r_b^2) / |sum_i wq_i|`` per row of ``hist``; ``None`` when the
    weights sum to zero (it is not defined), NaN where mixed-sign weights leave a negative square."""
    if int(wq_sum) == 0:
        return None
    h = np.asarray(hist, dtype=np.float64)
    r2 = (h * centres(r_max, h.shape[-1]) ** 2).sum(-1) / float(int(wq_sum)) ** 2
    with np.errstate(invalid="ignore"):
        return np.sqrt(r2)


def dmax(hist, r_max: float) -> np.ndarray:
    """The upper edge of the last non-zero bin per row of ``hist``; 0 for an empty row."""
    h = np.asarray(hist)
    nb = h.shape[-1]
    filled = h != 0
    last = np.where(filled.any(-1), nb - np.argmax(filled[..., ::-1], axis=-1), 0)
    return last.astype(np.float64) * (float(r_max) / nb)


def _line(x, y, w=None):
    """Weighted least squares of ``y = a x + b`` along the last axis, from centred sums: ``(a, b)``."""
    w = np.ones_like(x) if w is None else w
    sw = w.sum(-1, keepdims=True)
    xm, ym = (w * x).sum(-1, keepdims=True) / sw, (w * y).sum(-1, keepdims=True) / sw
    a = (w * (x - xm) * (y - ym)).sum(-1) / (w * (x - xm) ** 2).sum(-1)
    return a, ym[..., 0] - a * xm[..., 0]


def guinier(q, I, q_max: Optional[float] = None) -> dict:
    """The Guinier fit ``ln I = ln I0 - Rg^2 q^2 / 3`` over the points with ``q <= q_max`` (all by default) of one profile:
    ``{"rg", "i0", "n_points"}``; ``rg`` is ``None`` where the slope is not negative.  At least two points with I > 0."""
    qq, ii = _q(q), np.asarray(I, dtype=np.float64).reshape(-1)
    if qq.shape != ii.shape:
        raise ValueError("q and I have different lengths")
    keep = (ii > 0) if q_max is None else (ii > 0) & (qq <= float(q_max))
    if int(keep.sum()) < 2 or np.ptp(qq[keep]) == 0:
        raise ValueError("a Guinier fit needs two points with I > 0 at different q")
    slope, icpt = _line(qq[keep] ** 2, np.log(ii[keep]))
    return {"rg": float(np.sqrt(-3.0 * slope)) if slope < 0 else None, "i0": float(np.exp(icpt)), "n_points": int(keep.sum())}


def fit(I_model, q_exp, I_exp, sigma, background: bool = False) -> dict:
    """Linear least squares of an experimental curve by a model evaluated AT the experimental q (``profile(hist, ..., q_exp,
    ...)``: nothing is interpolated): ``min sum ((scale * I_model + background - I_exp) / sigma)^2``.  ``I_model [n_q]`` or
    ``[S, n_q]`` (per structure).  Returns ``scale``, ``background`` (only with ``background=True``), ``chi2`` (reduced:
    divided by ``n_q`` less the fitted parameters; ``None`` when that is not positive) and ``n_points`` -- floats for one
    model, arrays ``[S]`` for many."""
    m = np.asarray(I_model, dtype=np.float64)
    qq, e, sg = _q(q_exp), np.asarray(I_exp, dtype=np.float64).reshape(-1), np.asarray(sigma, dtype=np.float64).reshape(-1)
    if not (m.shape[-1:] == qq.shape == e.shape == sg.shape) or m.ndim not in (1, 2):
        raise ValueError("the model, q, I and sigma must have one length")
    if not (np.isfinite(e).all() and np.isfinite(sg).all() and (sg > 0).all()):
        raise ValueError("I must be finite and sigma finite and > 0")
    w = np.broadcast_to(1.0 / (sg * sg), m.shape)
    eb = np.broadcast_to(e, m.shape)
    if background:
        c, k = _line(m, eb, w)
        resid = (c[..., None] * m + k[..., None] - e) / sg
    else:
        c = (w * m * eb).sum(-1) / (w * m * m).sum(-1)
        resid = (c[..., None] * m - e) / sg
    dof = qq.shape[0] - (2 if background else 1)
    chi2 = (resid * resid).sum(-1) / dof if dof > 0 else None
    one = (lambda v: None if v is None else float(v)) if m.ndim == 1 else (lambda v: v)
    res = {"scale": one(c), "chi2": one(chi2), "n_points": int(qq.shape[0])}
    if background:
        res["background"] = one(k)
    return res


def read_curve(path: str, units: str = "A") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(q, I, sigma)`` of a text file with the columns q, I, sigma (more are ignored), ``#`` comments and blank lines; q in
    1 / A, or with ``units = "nm"`` in 1 / nm and converted.  ``ValueError`` naming the line for anything else."""
    if units not in ("A", "nm"):
        raise ValueError("units must be 'A' or 'nm'")
    rows = []
    try:
        with open(path) as f:
            lines = f.readlines()
    except OSError as err:
        raise ValueError(f"{path}: {err.strerror}")
    for no, line in enumerate(lines, 1):
        text = line.split("#", 1)[0].strip()
        if not text:
            continue
        cells = text.replace(",", " ").split()
        try:
            row = [float(c) for c in cells[:3]]
        except ValueError:
            raise ValueError(f"{path}, line {no}: not a number")
        if len(row) < 3:
            raise ValueError(f"{path}, line {no}: three columns are needed (q, I, sigma)")
        if not all(math.isfinite(v) for v in row) or row[0] < 0 or row[2] <= 0:
            raise ValueError(f"{path}, line {no}: q must be >= 0, sigma > 0 and every number finite")
        rows.append(row)
    if len(rows) < 2:
        raise ValueError(f"{path}: fewer than two data lines")
    a = np.asarray(rows, dtype=np.float64)
    return a[:, 0] / (10.0 if units == "nm" else 1.0), a[:, 1], a[:, 2]


def default_r_max(ref_xyz, sel, bin_width: float = 0.1) -> Tuple[float, int]:
    """``(r_max, n_bins)`` that hold every pair of the reference: twice the largest distance of a selected atom from its
    structure's centroid (no pair is farther apart), rounded up to the next multiple of ``bin_width``."""
    if not (math.isfinite(bin_width) and bin_width > 0):
        raise ValueError("the bin width must be a finite length > 0")
    x = np.asarray(ref_xyz.detach().cpu().numpy() if torch.is_tensor(ref_xyz) else ref_xyz, dtype=np.float64)[:, np.asarray(sel, dtype=np.int64)]
    far = np.sqrt(((x - x.mean(1, keepdims=True)) ** 2).sum(-1))
    far = far[np.isfinite(far)]
    if not far.size:
        raise ValueError("the reference has no finite selected coordinate")
    n_bins = int(math.floor(2.0 * float(far.max()) * (1.0 + 1e-6) / bin_width)) + 1       # fp32 distances round: a hair more
    return n_bins * float(bin_width), n_bins


# ----------------------------------------------------------------------------- compare
def _complete(res: dict) -> np.ndarray:
    return ~np.asarray(res["bad"], dtype=bool) & (np.asarray(res["beyond"]) == 0)


def _mean_hist(*results) -> Optional[np.ndarray]:
    rows = np.concatenate([np.asarray(r["hist"], dtype=np.float64)[_complete(r)] for r in results])
    return rows.mean(0) if rows.shape[0] else None


def log_rms(a, b) -> Optional[float]:
    """The RMS of ``ln a - ln b`` over the points where both are positive: the relative difference of two profiles on a log-I
    scale.  ``None`` without such a point."""
    if a is None or b is None:
        return None
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    keep = (a > 0) & (b > 0)
    return float(np.sqrt(np.mean((np.log(a[keep]) - np.log(b[keep])) ** 2))) if keep.any() else None


def _opt_list(v):
    return None if v is None else [float(t) for t in v]


def refuse_beyond(even: dict, odd: dict, enough: Optional[float] = None) -> None:
    """``ValueError`` when a good reference structure has a pair at ``r_max`` or farther: its profile is incomplete."""
    cut = sum(int((~np.asarray(r["bad"], dtype=bool) & (np.asarray(r["beyond"]) != 0)).sum()) for r in (even, odd))
    if cut:
        hint = f"r_max = {enough:g} would do" if enough is not None else "pass a larger r_max (default_r_max gives one that would do)"
        raise ValueError(f"{cut} reference structures have pairs beyond r_max = {float(even['r_max']):g} A: their profiles are incomplete; {hint}")


def compare_from_hists(even: dict, odd: dict, gen: dict, q, modulation: Optional[Callable] = None, exp=None, params: Optional[dict] = None,
                       n_bins_rg: int = 50, enough: Optional[float] = None) -> dict:
    """The statistics of ``compare`` from three results of ``saxs_hist`` (or ``restate``) -- the even reference frames, the
    odd ones, the generated structures, with the same tables -- pure host.  ``exp``: ``(q_exp, I_exp, sigma)`` or ``None``.
    Keys: ``SAXS_STATS_KEYS``; see ``compare``."""
    for r in (odd, gen):
        _same_tables(r, even["sel"], even["wq"], even["r_max"], int(even["n_bins"]))
    refuse_beyond(even, odd, enough)
    qq, r_max, st, wsum = _q(q), float(even["r_max"]), int(even["self_term"]), int(even["wq_sum"])
    means = {"ref": _mean_hist(even, odd), "even": _mean_hist(even), "odd": _mean_hist(odd), "gen": _mean_hist(gen)}
    prof = {k: None if h is None else profile(h, st, qq, r_max, modulation) for k, h in means.items()}
    stats = {**ensemble.set_sizes(even, odd, gen), "n_beyond_gen": int((~np.asarray(gen["bad"], dtype=bool) & (np.asarray(gen["beyond"]) != 0)).sum()),
             "params": dict(params or {}), "n_atoms": int(np.asarray(even["sel"]).shape[0]), "q": qq.tolist(),
             "profile_ref": _opt_list(prof["ref"]), "profile_gen": _opt_list(prof["gen"]),
             "log_rms": log_rms(prof["gen"], prof["ref"]), "floor": log_rms(prof["even"], prof["odd"]),
             "i0_ref": None if means["ref"] is None else float(i_zero(means["ref"], st)),
             "i0_gen": None if means["gen"] is None else float(i_zero(means["gen"], st))}
    # per structure: Rg (its distribution against the reference's) and Dmax
    per = {}
    for name, r in (("even", even), ("odd", odd), ("gen", gen)):
        keep = _complete(r)
        radii = rg(np.asarray(r["hist"])[keep], wsum, r_max)
        per[name] = (None if radii is None else radii[np.isfinite(radii)], dmax(np.asarray(r["hist"])[keep], r_max))
    block = None
    if per["even"][0] is not None:
        ref_rg = np.concatenate([per["even"][0], per["odd"][0]])
        if ref_rg.size and per["gen"][0].size:
            lo, hi = float(ref_rg.min()), float(ref_rg.max())
            pad = 0.1 * (hi - lo) if hi > lo else 0.05 * max(abs(hi), 1.0)           # the reference's range, 20 % wider
            block = ensemble.scalar_block(per["even"][0], per["odd"][0], per["gen"][0], lo - pad, hi + pad, n_bins_rg)
    stats["rg"] = block
    ref_d, gen_d = np.concatenate([per["even"][1], per["odd"][1]]), per["gen"][1]
    stats["dmax"] = {"mean_ref": ensemble.moments(ref_d)[0], "max_ref": float(ref_d.max()) if ref_d.size else None,
                     "mean_gen": ensemble.moments(gen_d)[0], "max_gen": float(gen_d.max()) if gen_d.size else None}
    stats["exp"] = None
    if exp is not None:
        qe, ie, se = exp
        bg = bool((params or {}).get("background", False))
        at = lambda h: None if h is None else profile(h, st, qe, r_max, modulation)
        short = lambda f: None if f is None else {k: f[k] for k in ("scale", "chi2", "background") if k in f}
        one = {k: None if means[k] is None else fit(at(means[k]), qe, ie, se, bg) for k in ("ref", "gen")}
        keep = _complete(gen)
        each = fit(at(np.asarray(gen["hist"])[keep]), qe, ie, se, bg)["chi2"] if keep.any() else None
        dist = None
        if each is not None:
            where = np.flatnonzero(keep)
            dist = {"mean": float(each.mean()), "median": float(np.median(each)), "min": float(each.min()), "max": float(each.max()),
                    "best": int(where[int(np.argmin(each))]), "values": [float(v) for v in each]}
        stats["exp"] = {"n_points": int(np.asarray(qe).shape[0]), "ref": short(one["ref"]), "gen": short(one["gen"]), "structures": dist}
    return stats


def params_of(wq, r_max: float, n_bins: int, **more) -> dict:
    """What ``compare`` records of its inputs: the weights as floats, ``r_max`` as fp32 holds it, the bins, and ``more``."""
    return {"weights": [int(v) / float(FIXED) for v in np.asarray(wq).reshape(-1)], "r_max": float(np.float32(r_max)), "n_bins": int(n_bins),
            "bin_width": float(np.float32(r_max)) / int(n_bins), **more}


def q_grid(q_max: float = 0.5, n_q: int = 101) -> np.ndarray:
    if not (math.isfinite(q_max) and q_max > 0 and int(n_q) >= 2):
        raise ValueError("q_max must be a finite number > 0 and n_q at least 2")
    return np.linspace(0.0, float(q_max), int(n_q))


def compare(gen_xyz, ref_xyz, sel, wq, r_max: Optional[float] = None, bin_width: float = 0.1, q=None, modulation: Optional[Callable] = None,
            exp=None, background: bool = False, chunk: int = 4096, device="cuda") -> dict:
    """Generated structures ``gen_xyz [S,n,3]`` against the reference frames ``ref_xyz [T,n,3]`` (at least two) over the
    selection ``sel [m]`` with the fixed-point weights ``wq [m]``.  ``r_max``: ``default_r_max`` of the reference when
    ``None``, else rounded up to a multiple of ``bin_width``.  ``q``: the grid of the profiles (default ``q_grid()``).  The
    reference's even and odd frames are counted apart: what the halves differ by is the floor.  A reference structure with a
    pair beyond ``r_max`` is refused with the ``r_max`` that would do.  Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen, n_beyond_gen     structures, those left out as bad, and the generated ones left out of
                   every mean because a pair lies beyond r_max
      params       weights, r_max, n_bins, bin_width, background
      n_atoms, q, profile_ref, profile_gen                 the mean profiles of both ensembles on the q grid
      log_rms, floor    the RMS of ln I_gen - ln I_ref over the grid, and the same of the reference's even against odd frames
      i0_ref, i0_gen    I(0) of the mean profiles
      rg           ``ensemble.scalar_block`` of the real-space Rg per structure: histograms, JSD with its floor, means
                   (``None`` when the weights sum to zero)
      dmax         {mean_ref, max_ref, mean_gen, max_gen}
      exp          with an experimental curve: {n_points, ref, gen: {scale, chi2[, background]} of the mean profiles evaluated
                   at the curve's q, structures: {mean, median, min, max, best, values} of the per-structure chi2}
    """
    ref, gen = structures(ref_xyz), structures(gen_xyz)
    if int(ref.shape[0]) < 2:
        raise ValueError("at least two reference frames are needed (the floor compares the even with the odd ones)")
    if int(ref.shape[1]) != int(gen.shape[1]):
        raise ValueError(f"the frames have {int(ref.shape[1])} and {int(gen.shape[1])} atoms")
    table = ensemble.selection(sel, int(ref.shape[1]), purpose="weigh")
    enough, enough_bins = default_r_max(ref, table, bin_width)
    if r_max is None:
        r_max, n_bins = enough, enough_bins
    else:
        scale_of(r_max, 1)
        n_bins = max(int(math.ceil(float(r_max) / bin_width - 1e-9)), 1)
        r_max = n_bins * float(bin_width)
    lim = limits()
    if n_bins > lim["bins"]:
        raise ValueError(f"r_max = {r_max:g} A in bins of {bin_width:g} A is {n_bins} bins (the kernel holds {lim['bins']}): pass a wider bin")
    qq = q_grid() if q is None else _q(q)
    kw = dict(chunk=chunk, device=device)
    even, odd, got = (saxs_hist(s, table, wq, r_max, n_bins, **kw) for s in (ref[0::2], ref[1::2], gen))
    return compare_from_hists(even, odd, got, qq, modulation, exp, params_of(got["wq"], r_max, n_bins, background=bool(background)),
                              enough=enough)


SAXS_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_beyond_gen", "params", "n_atoms", "q", "profile_ref", "profile_gen",
                   "log_rms", "floor", "i0_ref", "i0_gen", "rg", "dmax", "exp")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"saxs_stats"`` in its JSON summary line: no profiles, no histograms, no weights."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_beyond_gen", "n_atoms", "log_rms", "floor", "i0_ref",
                                   "i0_gen", "dmax")}
    short["r_max"], short["n_bins"] = stats["params"].get("r_max"), stats["params"].get("n_bins")
    short["rg"] = ensemble.short_block(stats["rg"], ensemble.MOMENTS + ("floor",))
    short["exp"] = None
    if stats["exp"] is not None:
        e = stats["exp"]
        short["exp"] = {"n_points": e["n_points"], "ref": e["ref"], "gen": e["gen"],
                        "structures": None if e["structures"] is None else {k: e["structures"][k] for k in ("mean", "median", "min", "max", "best")}}
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.saxs",
                                "small-angle X-ray scattering profiles of generated structures against those of the reference frames",
                                top_help="npz with z and bonds; default: those of -ref")
    p.add_argument("-saxs_atoms", choices=("heavy", "all"), default="heavy", help="the scatterers; heavy folds the hydrogens in (heavy)")
    p.add_argument("-saxs_solvent", type=float, default=RHO0, help="the solvent's electron density in e / A^3; 0: in vacuo (0.334)")
    p.add_argument("-saxs_rmax", type=float, default=None, help="the largest distance binned, in Angstrom (from the reference)")
    p.add_argument("-saxs_bin", type=float, default=0.1, help="the bin width in Angstrom (0.1)")
    p.add_argument("-saxs_qmax", type=float, default=0.5, help="the q grid ends here, in 1 / Angstrom (0.5)")
    p.add_argument("-saxs_nq", type=int, default=101, help="points of the q grid from 0 (101)")
    p.add_argument("-saxs_exp", default=None, help="text file with the columns q, I, sigma: an experimental curve to fit")
    p.add_argument("-saxs_units", choices=("A", "nm"), default="A", help="the unit of -saxs_exp's q: 1 / A or 1 / nm (A)")
    p.add_argument("-saxs_background", action="store_true", help="fit a constant background with the scale")
    p.add_argument("-profiles", default=None, help="npz for q, both mean profiles and every generated structure's profile, Rg and Dmax")
    return compare_cli.finish_parser(p, "saxs_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``sel``, ``wq``, ``q``, ``exp``, with everything that can be
    refused without a device refused here (``SystemExit``)."""
    if not (math.isfinite(args.saxs_bin) and args.saxs_bin > 0):
        raise SystemExit("-saxs_bin must be a finite length > 0 in Angstrom")
    if args.saxs_rmax is not None and not (math.isfinite(args.saxs_rmax) and args.saxs_rmax > 0):
        raise SystemExit("-saxs_rmax must be a finite length > 0 in Angstrom")
    if not (math.isfinite(args.saxs_solvent) and args.saxs_solvent >= 0):
        raise SystemExit("-saxs_solvent must be a finite electron density >= 0")
    if not (math.isfinite(args.saxs_qmax) and args.saxs_qmax > 0) or args.saxs_nq < 2:
        raise SystemExit("-saxs_qmax must be > 0 and -saxs_nq at least 2")
    exp = None
    if args.saxs_exp is not None:
        with compare_cli.refusing("-saxs_exp: "):
            exp = read_curve(args.saxs_exp, args.saxs_units)
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args, ("z", "bonds"))
    with compare_cli.refusing():
        sel = select_atoms(z, args.saxs_atoms)
        if int(sel.shape[0]) == 0:
            raise ValueError("the selection is empty (m = 0): no atoms to weigh")
        wq = quantise(weights_of(z, np.asarray(top["bonds"]), sel, args.saxs_solvent))
        lim = limits()
        if int(sel.shape[0]) > lim["atoms"]:
            raise ValueError(f"the selection lists {sel.shape[0]} atoms (the kernel holds {lim['atoms']})")
        r_max, n_bins = default_r_max(ref_xyz, sel, args.saxs_bin) if args.saxs_rmax is None else \
            (args.saxs_rmax, int(math.ceil(args.saxs_rmax / args.saxs_bin - 1e-9)))
        if n_bins > lim["bins"]:
            raise ValueError(f"r_max = {r_max:g} A in bins of {args.saxs_bin:g} A is {n_bins} bins (the kernel holds {lim['bins']}): "
                             f"pass a wider -saxs_bin")
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "sel": sel, "wq": wq, "q": q_grid(args.saxs_qmax, args.saxs_nq), "exp": exp}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    with compare_cli.refusing():
        stats = compare(inp["gen_xyz"], inp["ref_xyz"], inp["sel"], inp["wq"], r_max=args.saxs_rmax, bin_width=args.saxs_bin, q=inp["q"],
                        exp=inp["exp"], background=args.saxs_background, device=args.device)
        if args.profiles:
            p = stats["params"]
            got = saxs_hist(inp["gen_xyz"], inp["sel"], inp["wq"], p["r_max"], p["n_bins"], device=args.device)
            radii = rg(got["hist"], got["wq_sum"], got["r_max"])
            np.savez(args.profiles, q=inp["q"], profile_ref=np.asarray(stats["profile_ref"], dtype=np.float64),
                     profile_gen=np.asarray(stats["profile_gen"] if stats["profile_gen"] is not None else [], dtype=np.float64),
                     profiles=profile(got["hist"], got["self_term"], inp["q"], got["r_max"]),
                     rg=np.full(got["hist"].shape[0], np.nan) if radii is None else radii, dmax=dmax(got["hist"], got["r_max"]),
                     beyond=got["beyond"], bad=got["bad"])
    compare_cli.finish("saxs", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
