"""Test-side restatement of the kernel density estimates (K22, csrc/kde.hip; coarsegrainingvae_amd/density.py) in plain
numpy fp64.  It lives in the tests only: nothing on the product path imports it, and it is no fallback for a missing kernel.

The estimator, written out on RAW coordinates (no whitening: that is the product's way of getting the same number):
  p(y) = sum_i exp(-(y - x_i)^T H^-1 (y - x_i) / 2) / (N (2 pi)^(d/2) sqrt(det H))
  H    = factor^2 cov(x, ddof=1), factor = N^(-1/(d+4)) (Scott), (N (d+2) / 4)^(-1/(d+4)) (Silverman) or a number;
         with a periodic axis H is diagonal, width_a = factor x std(ddof=1), on a periodic axis factor x the circular
         standard deviation sqrt(-2 ln R) period / (2 pi)
  on a periodic axis a difference is reduced to its minimum image, delta - period rint(delta / period).
``image_sum`` is the same with the 3^k nearest images summed explicitly instead.

``sums`` is what the KERNEL computes, on the coordinates the kernel is given: sum_i exp2(-|q - s_i|^2) with minimum image
in fp64; ``sums_fp32`` emulates the kernel's arithmetic (fp32 inputs, differences, squares and exponent, an fp64 sum).

The error bound of the kernel against ``sums`` (``relative_bound``), per point:
  U    the largest coordinate magnitude of the call, in the kernel's scaled units.  Rounding both coordinates of a
       difference to fp32 moves the exponent r = |delta|^2 by at most 4 sqrt(r) U 2^-24; the roundings of the squares and
       their sum by at most 3 r 2^-24; terms beyond r = 126 (exp2(-126) is fp32's smallest normal) are flushed to zero by
       v_exp_f32, so r <= 126 in every term that counts; d exp2(-r) / exp2(-r) = ln2 dr.
  c    v_exp_f32 is accurate to 1 ulp = 2 x 2^-24 relative ("AMD Instinct MI300 / CDNA3 Instruction Set Architecture",
       V_EXP_F32: "1ULP accuracy, denormals are flushed"); a stage adds at most 1024 non-negative fp32 terms one after
       the other, 1023 roundings of at most 2^-24 of the running (never decreasing) sum each; the fp64 additions of the
       stages and ranges are 2^-29 of that and are covered by one more unit.  c = 2 + 1023 + 1 = 1026.
  relative error <= ln2 (4 sqrt(126) U + 3 x 126) 2^-24 + c 2^-24
A point whose fp64 sum is below N 2^-126 -- all its terms may have been flushed -- is compared absolutely against that.
For the relative bound to hold right down to that floor, a sum at or above it must not have lost terms worth more than
the bound to the flush: the kernel computes every term as exp2(64 - r) and scales the fp64 sum by 2^-64, so what it
flushes is below 2^-190 per term, 2^-64 of the floor.  (The terms between r = 126 and 190 that this keeps carry an
exponent error of up to 3 x 190 x 2^-24 instead of 3 x 126 x 2^-24; they are at most the floor in total, and c covers it.)
"""
import math

import numpy as np

C_UNITS = 1026.0
R_FLUSH = 126.0
SCALE = math.sqrt(0.5 * math.log2(math.e))


def _rows(x):
    a = np.asarray(x, dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def _per(period, d):
    if period is None:
        return np.zeros(d)
    p = np.asarray(period, dtype=np.float64).reshape(-1)
    return np.repeat(p, d) if p.shape[0] == 1 else p


def factor(bandwidth, n, d):
    if bandwidth == "scott":
        return n ** (-1.0 / (d + 4))
    if bandwidth == "silverman":
        return (n * (d + 2) / 4.0) ** (-1.0 / (d + 4))
    return float(bandwidth)


def circular_std(x, period):
    ang = 2.0 * math.pi * np.asarray(x, dtype=np.float64) / period
    R = math.hypot(np.cos(ang).mean(), np.sin(ang).mean())
    return math.sqrt(-2.0 * math.log(R)) * period / (2.0 * math.pi)


def bandwidth_matrix(data, bandwidth="scott", period=None):
    x = _rows(data)
    n, d = x.shape
    per, f = _per(period, d), factor(bandwidth, x.shape[0], x.shape[1])
    if not (per > 0).any():
        return f * f * np.atleast_2d(np.cov(x.T, ddof=1))
    w = [f * (circular_std(x[:, a], per[a]) if per[a] > 0 else x[:, a].std(ddof=1)) for a in range(d)]
    return np.diag(np.square(w))


def _differences(points, data, per):
    """``[M, N, d]`` minimum-image differences."""
    delta = points[:, None, :] - data[None, :, :]
    for a in range(data.shape[1]):
        if per[a] > 0:
            delta[:, :, a] -= per[a] * np.rint(delta[:, :, a] / per[a])
    return delta


def normalisation(n, H):
    d = H.shape[0]
    return n * (2.0 * math.pi) ** (d / 2.0) * math.sqrt(np.linalg.det(H))


def evaluate(data, points, H, period=None, block=512):
    """The density of ``data [N,d]`` with bandwidth matrix ``H`` at ``points [M,d]``: fp64 ``[M]``."""
    x, q = _rows(data), _rows(points)
    per, Hinv = _per(period, x.shape[1]), np.linalg.inv(H)
    out = np.zeros(q.shape[0])
    for at in range(0, q.shape[0], block):
        delta = _differences(q[at:at + block], x, per)
        out[at:at + block] = np.exp(-0.5 * np.einsum("mna,ab,mnb->mn", delta, Hinv, delta)).sum(1)
    return out / normalisation(x.shape[0], H)


def image_sum(data, points, H, period):
    """``evaluate`` for a DIAGONAL ``H`` with the three nearest images of every periodic axis summed explicitly (the
    minimum image and its two neighbours) instead of the minimum image alone."""
    x, q = _rows(data), _rows(points)
    d = x.shape[1]
    per, Hinv = _per(period, d), np.linalg.inv(H)
    out = np.zeros(q.shape[0])
    delta = _differences(q, x, per)
    shifts = np.array(np.meshgrid(*[(-1, 0, 1) if per[a] > 0 else (0,) for a in range(d)], indexing="ij")).reshape(d, -1).T
    for k in shifts:
        moved = delta + (k * per)[None, None, :]
        out += np.exp(-0.5 * np.einsum("mna,ab,mnb->mn", moved, Hinv, moved)).sum(1)
    return out / normalisation(x.shape[0], H)


# ----------------------------------------------------------------------------- what the kernel computes
def sums(samples, points, period=None, block=256):
    """``sum_i exp2(-|q - s_i|^2)`` in fp64 of kernel-unit coordinates (``samples [N,d]``, ``points [M,d]``, any float
    type: widened exactly); non-finite samples are skipped, a non-finite point gives NaN."""
    s, q = _rows(samples), _rows(points)
    per = _per(period, s.shape[1])
    s = s[np.isfinite(s).all(1)]
    out = np.zeros(q.shape[0])
    good = np.isfinite(q).all(1)
    for at in range(0, q.shape[0], block):
        delta = _differences(np.where(good[at:at + block, None], q[at:at + block], 0.0), s, per)
        out[at:at + block] = np.exp2(-(delta * delta).sum(2)).sum(1)
    out[~good] = np.nan
    return out


def sums_fp32(samples, points, period=None):
    """The kernel's arithmetic emulated: fp32 inputs, differences, minimum image (``delta * (1 / period)``, ``rint``, one
    fused step emulated in fp64 and rounded once), squares and exponent ``64 - r``; terms beyond ``r - 64 = 126`` flushed;
    an fp64 sum, scaled by ``2^-64``."""
    f = np.float32
    s, q = _rows(samples).astype(f), _rows(points).astype(f)
    per = _per(period, s.shape[1]).astype(f)
    s = s[np.isfinite(s).all(1)]
    r = np.zeros((q.shape[0], s.shape[0]), dtype=f)
    for a in range(s.shape[1]):
        delta = q[:, None, a] - s[None, :, a]
        if per[a] > 0:
            k = np.rint(delta * (f(1.0) / per[a]))
            delta = (delta.astype(np.float64) - np.float64(per[a]) * k.astype(np.float64)).astype(f)
        r = r + delta * delta if a else delta * delta
    r = r - f(64.0)
    term = np.where(r > f(R_FLUSH), f(0), np.exp2(-r)).astype(np.float64)
    return term.sum(1) * 2.0 ** -64


def relative_bound(U):
    return (math.log(2.0) * (4.0 * math.sqrt(R_FLUSH) * float(U) + 3.0 * R_FLUSH) + C_UNITS) * 2.0 ** -24


def absolute_floor(n):
    return n * 2.0 ** -126


def error_ratio(got, want, n, U):
    """The worst error of ``got`` against the fp64 ``want`` as a fraction of what the bound allows: at most 1 passes.
    Points below the floor are compared absolutely against it; NaN must meet NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return math.inf
    ok = ~np.isnan(want)
    got, want = got[ok], want[ok]
    if got.size == 0:
        return 0.0
    floor = absolute_floor(max(n, 1))
    low = want < floor
    allowed = np.where(low, floor, relative_bound(U) * want)
    return float(np.max(np.abs(got - want) / allowed))


# ----------------------------------------------------------------------------- the statistics of compare_planes
def js_divergence(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    p, q = a / a.sum(), b / b.sum()
    m = 0.5 * (p + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = lambda u: np.where(u > 0, u * np.log2(u / m), 0.0).sum()
        return float(0.5 * (kl(p) + kl(q)))


def free_energy(density, eps=1e-3):
    return -np.log(np.asarray(density, dtype=np.float64) + eps)


def grid_nodes(ranges, n_grid, period):
    per = _per(period, len(ranges))
    axes = [np.linspace(lo, hi, n_grid, endpoint=not per[a] > 0) for a, (lo, hi) in enumerate(ranges)]
    return np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")], axis=1)


def default_ranges(ref, period):
    ref = _rows(ref)
    per, out = _per(period, ref.shape[1]), []
    for a in range(ref.shape[1]):
        if per[a] > 0:
            out.append((-0.5 * per[a], 0.5 * per[a]))
        else:
            lo, hi = ref[:, a].min(), ref[:, a].max()
            out.append((lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo)))
    return out


def compare_planes(ref, gen, n_grid=100, bandwidth="scott", period=None, ranges=None, fe_window=6.0):
    ref, gen = _rows(ref), _rows(gen)
    H = bandwidth_matrix(ref, bandwidth, period)
    ranges = default_ranges(ref, period) if ranges is None else ranges
    nodes = grid_nodes(ranges, n_grid, period)
    even, odd = ref[0::2], ref[1::2]
    dens = {k: evaluate(x, nodes, H, period) for k, x in (("ref", ref), ("gen", gen), ("even", even), ("odd", odd))}
    fe = {k: free_energy(v) for k, v in dens.items()}
    near = fe["ref"] <= fe["ref"].min() + fe_window
    rms = lambda a, b: float(np.sqrt(np.mean((a[near] - b[near]) ** 2)))
    with np.errstate(divide="ignore"):
        return {"jsd": js_divergence(dens["ref"], dens["gen"]), "floor": js_divergence(dens["even"], dens["odd"]),
                "fe_rmse": rms(fe["gen"], fe["ref"]), "fe_floor": rms(fe["even"], fe["odd"]), "fe_nodes": int(near.sum()),
                "loglik_gen": float(np.log(evaluate(ref, gen, H, period)).mean()),
                "loglik_floor": float(np.log(evaluate(even, odd, H, period)).mean()),
                "bandwidth": H, "ranges": ranges, "density": dens}


# ----------------------------------------------------------------------------- a synthetic peptide
def peptide(n_res=3):
    """``(z, bonds)`` of a capped backbone ACE-(GLY-like)_n-NME without hydrogens: CH3-C(=O)-[N-CA-C(=O)]_n-N-CH3.  Every
    residue has a phi and a psi."""
    z, bonds = [6, 6, 8], [(0, 1), (1, 2)]
    prev_c = 1
    for _ in range(n_res):
        n = len(z)
        z += [7, 6, 6, 8]                                    # N, CA, C, O
        bonds += [(prev_c, n), (n, n + 1), (n + 1, n + 2), (n + 2, n + 3)]
        prev_c = n + 2
    n = len(z)
    z += [7, 6]
    bonds += [(prev_c, n), (n, n + 1)]
    return np.array(z), np.array(bonds)


def place(prev3, length, angle, torsion):
    """The position of an atom bonded to ``prev3[2]`` at ``length``, with bond angle ``angle`` at ``prev3[2]`` and torsion
    ``torsion`` over (prev3[0], prev3[1], prev3[2], new) in the convention of ``internal_coords_restatement.value``."""
    a, b, c = prev3
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    d = np.array([-length * math.cos(angle), length * math.sin(angle) * math.cos(torsion), length * math.sin(angle) * math.sin(torsion)])
    return c + d[0] * bc + d[1] * m + d[2] * nrm


def peptide_structures(n_res, torsions):
    """``xyz [S, n, 3]`` float32 of ``peptide(n_res)`` whose backbone chain CH3-C-N-CA-C-...-N-CH3 has the torsions
    ``torsions [S, 3 n_res + 1]`` (omega_0, phi_1, psi_1, omega_1, ...) in chain order; carbonyl oxygens are placed
    trans to the chain.  Bond lengths 1.4 (1.2 to O), bond angles 115 degrees."""
    z, _ = peptide(n_res)
    chain = [0, 1] + [a for r in range(n_res) for a in (3 + 4 * r, 4 + 4 * r, 5 + 4 * r)] + [len(z) - 2, len(z) - 1]
    oxy = {1: 2, **{5 + 4 * r: 6 + 4 * r for r in range(n_res)}}
    ang = math.radians(115.0)
    out = np.zeros((len(torsions), len(z), 3))
    for s, tors in enumerate(np.asarray(torsions, dtype=np.float64)):
        x = out[s]
        x[chain[0]], x[chain[1]] = (0.0, 0.0, 0.0), (1.4, 0.0, 0.0)
        x[chain[2]] = (1.4 - 1.4 * math.cos(ang), 1.4 * math.sin(ang), 0.0)
        for k in range(3, len(chain)):
            x[chain[k]] = place([x[chain[k - 3]], x[chain[k - 2]], x[chain[k - 1]]], 1.4, ang, tors[k - 3])
        for c, o in oxy.items():
            k = chain.index(c)
            x[o] = place([x[chain[k + 1]], x[chain[k - 1]], x[c]], 1.2, math.radians(122.0), math.pi) if k >= 1 else x[o]
    return out.astype(np.float32)
