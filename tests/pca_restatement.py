"""Numpy restatement of K27 (csrc/pca.hip) and of the host statistics of ``coarsegrainingvae_amd.pca``, written from their
definitions and importing nothing of the package: features with the same bits, moments by a plain ascending loop, the
projection, DCCM, RMSIP and the covariance overlap."""
import numpy as np

from gram_restatement import bin_of, edge_distance, hist2      # noqa: F401  (the bin rule, shared with K16)


def features(y, sel, centre):
    """``f [S, 3m]``: ``(double)y[s, sel[a], c] - centre[sel[a], c]`` -- an exact widening and ONE fp64 rounding, the bits the
    kernel stages.  ``y`` is fp32 (rounded here if it is not)."""
    y32 = np.asarray(y, dtype=np.float32)
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    c = np.asarray(centre, dtype=np.float64)
    return (y32[:, sel, :].astype(np.float64) - c[sel][None]).reshape(y32.shape[0], 3 * sel.shape[0])


def moments(y, sel, centre, bad=None):
    """``sum [d]``, ``cov [d,d]``, ``n_good`` over the structures with ``bad == 0``, one structure after the other in
    ascending order; and ``abs_sum [d]`` / ``abs_cov [d,d]``, the sums of the absolute values of what was added (what the
    error bounds are made of)."""
    f = features(y, sel, centre)
    S, d = f.shape
    good = np.ones(S, dtype=bool) if bad is None else np.asarray(bad).reshape(-1) == 0
    out = {"sum": np.zeros(d), "cov": np.zeros((d, d)), "n_good": 0, "abs_sum": np.zeros(d), "abs_cov": np.zeros((d, d))}
    for s in range(S):
        if not good[s]:
            continue
        row = f[s]
        out["sum"] += row
        out["cov"] += np.outer(row, row)
        out["abs_sum"] += np.abs(row)
        out["abs_cov"] += np.abs(np.outer(row, row))
        out["n_good"] += 1
    return out


def moment_bounds(want):
    """``|d cov_ij| <= (N + 2) 2^-52 sum_s |f_si f_sj|`` (N additions in another order; the matrix core does not round the
    product, the restatement does: one more; one for the final addition to the totals) and ``|d sum_i| <= N 2^-52 sum_s
    |f_si|``."""
    N = want["n_good"]
    return {"cov": (N + 2) * 2.0 ** -52 * want["abs_cov"], "sum": N * 2.0 ** -52 * want["abs_sum"]}


def project(y, sel, centre, mean, W, bad=None):
    """``proj [S,k] = (f - mean) W`` (NaN rows: bad) and ``abs [S,k] = sum_f |(f - mean)_f W_fk|``; ``v = f - mean`` is one
    more fp64 rounding, the same on the device."""
    v = features(y, sel, centre) - np.asarray(mean, dtype=np.float64)[None]
    W = np.asarray(W, dtype=np.float64)
    good = np.ones(v.shape[0], dtype=bool) if bad is None else np.asarray(bad).reshape(-1) == 0
    v = np.where(good[:, None], v, 0.0)
    proj = np.zeros((v.shape[0], W.shape[1]))
    for f in range(v.shape[1]):                                # ascending features
        proj += v[:, f:f + 1] * W[f][None]
    proj[~good] = np.nan
    return proj, np.abs(v) @ np.abs(W)


def covariance(mom):
    """``(mu, C)``: ``mu = sum / N``, ``C = cov / N - mu mu^T`` -- divided by N."""
    N = mom["n_good"]
    mu = mom["sum"] / N
    return mu, mom["cov"] / N - np.outer(mu, mu)


def spectrum(C):
    """Eigenvalues descending (clamped at 0) and modes of a symmetric matrix; the signs are eigh's."""
    w, v = np.linalg.eigh(0.5 * (C + C.T))
    return np.maximum(w[::-1], 0.0), v[:, ::-1]


def dccm(C):
    m = C.shape[0] // 3
    out = np.zeros((m, m))
    for i in range(m):
        for j in range(m):
            num = sum(C[3 * i + c, 3 * j + c] for c in range(3))
            vi = sum(C[3 * i + c, 3 * i + c] for c in range(3))
            vj = sum(C[3 * j + c, 3 * j + c] for c in range(3))
            out[i, j] = num / np.sqrt(vi * vj) if vi > 0 and vj > 0 else 0.0
    return out


def rmsip(Wa, Wb):
    k = Wa.shape[1]
    return float(np.sqrt(sum(float(Wa[:, i] @ Wb[:, j]) ** 2 for i in range(k) for j in range(Wb.shape[1])) / k))


def covariance_overlap(la, Va, lb, Vb):
    total = float(np.sum(la) + np.sum(lb))
    cross = sum(np.sqrt(la[i] * lb[j]) * float(Va[:, i] @ Vb[:, j]) ** 2 for i in range(len(la)) for j in range(len(lb)))
    return 1.0 - np.sqrt(max(0.0, total - 2.0 * cross)) / np.sqrt(total)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def planted(rng, base, modes, amplitudes, S, noise=0.05):
    """``S`` fp32 structures: ``base [n,3]`` moved along the unit collective ``modes [k,n,3]`` with Gaussian amplitudes of
    standard deviation ``amplitudes [k]``, plus isotropic Gaussian ``noise``, each given a random proper rotation and a
    translation."""
    out = np.empty((S,) + base.shape, dtype=np.float32)
    for s in range(S):
        x = base + np.tensordot(rng.standard_normal(len(amplitudes)) * np.asarray(amplitudes), modes, 1)
        x = x + noise * rng.standard_normal(base.shape)
        out[s] = (x @ random_rotation(rng).T + rng.uniform(-5, 5, 3)).astype(np.float32)
    return out


def unit_modes(rng, k, n, against=None):
    """``k`` random orthonormal collective modes ``[k,n,3]``, orthogonal to the modes ``against`` too."""
    rows = [] if against is None else [a.reshape(-1) for a in against]
    keep = len(rows)
    for _ in range(k):
        v = rng.standard_normal(3 * n)
        for r in rows:
            v = v - (v @ r) * r
        rows.append(v / np.linalg.norm(v))
    return np.array(rows[keep:]).reshape(k, n, 3)
