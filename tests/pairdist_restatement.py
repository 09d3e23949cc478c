"""The definition of ``coarsegrainingvae_amd.pairdist`` restated in ``numpy.float32``, every operation rounded on its own --
whole ``[m, m]`` tables per structure, no tiles, no words, no LDS -- producing every output of ``cgv_pairdist_counts``; an
independent fp64 form; and the input generators of the pair-distance tests.  Test infrastructure, not a test."""
import numpy as np

F = np.float32


def chain(n, rng, step=1.5):
    """``[n, 3]`` float32: a random walk of ``step`` A steps."""
    d = rng.normal(size=(n, 3))
    d *= step / np.linalg.norm(d, axis=1, keepdims=True)
    return np.cumsum(d, axis=0).astype(F)


def chains(S, n, rng, step=1.5):
    return np.stack([chain(n, rng, step) for _ in range(S)])


def chain_bonds(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)


def band(m, depth):
    """``[m, m]`` bool: the pairs of a chain at most ``depth`` bonds apart, the diagonal included."""
    i = np.arange(m)
    return np.abs(i[:, None] - i[None, :]) <= depth


def n_pairs_of(C):
    return C * (C + 1) // 2


def pair_index(a, b, C):
    """The unordered class pair ``(lo <= hi)`` has the index ``lo * C - lo (lo - 1) / 2 + (hi - lo)``."""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo * C - lo * (lo - 1) // 2 + (hi - lo)


def rmax2_of(r_max):
    return F(r_max) * F(r_max)


def scale_of(r_max, n_bins):
    return F(np.float64(n_bins) / np.float64(F(r_max)))


def sq_dist2(a, b):
    """``(dx*dx + dy*dy) + dz*dz`` in fp32 of ``a [..., 3] - b [..., 3]`` (broadcast), every operation rounded on its own."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    return (xx + yy) + zz


def bins_of(x, r_max, n_bins):
    """Of ONE structure's selected atoms ``x [m, 3]``: ``(in_range [m, m] bool, b [m, m] int64)``."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = sq_dist2(x[:, None, :], x[None, :, :])
        in_range = q < rmax2_of(r_max)
        d = np.sqrt(q)
        t = d * scale_of(r_max, n_bins)
        assert q.dtype == F and d.dtype == F and t.dtype == F
        b = np.minimum(np.where(in_range, t, F(0)).astype(np.int64), n_bins - 1)      # truncation; only in-range entries are used
    return in_range, b


def pair_hist(xyz, sel, cls, C, excluded, r_max, n_bins):
    """Every output of ``cgv_pairdist_counts`` for the caller's tables: ``hist [P, n_bins]`` and ``beyond [P]`` int64,
    ``bad [S]`` bool; and ``n_pairs [P]``: the non-excluded pairs ``i < j`` of every class pair."""
    xyz = np.asarray(xyz, dtype=F)
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    cls = np.asarray(cls, dtype=np.int64).reshape(-1)
    m, S, P = sel.shape[0], xyz.shape[0], n_pairs_of(C)
    counted = np.triu(~(np.asarray(excluded, dtype=bool).reshape(m, m) | np.eye(m, dtype=bool)), 1)
    pc = pair_index(cls[:, None], cls[None, :], C)
    hist = np.zeros((P, n_bins), dtype=np.int64)
    beyond = np.zeros(P, dtype=np.int64)
    bad = np.zeros(S, dtype=bool)
    for s in range(S):
        x = xyz[s, sel]
        if not np.isfinite(x).all():
            bad[s] = True
            continue
        in_range, b = bins_of(x, r_max, n_bins)
        inside = counted & in_range
        np.add.at(hist, (pc[inside], b[inside]), 1)
        np.add.at(beyond, pc[counted & ~in_range], 1)
    return {"hist": hist, "beyond": beyond, "bad": bad, "n_pairs": np.bincount(pc[counted], minlength=P).astype(np.int64)}


def pair_hist64(x, cls, C, excluded, r_max, n_bins, skip=None):
    """An independent fp64 form of ONE structure ``x [m, 3]``: ``numpy.linalg.norm`` and ``floor(d * n_bins / r_max)``.
    ``skip [m, m]`` bool: pairs left out of every count."""
    x = np.asarray(x, dtype=np.float64)
    m, P = x.shape[0], n_pairs_of(C)
    d = np.linalg.norm(x[:, None] - x[None], axis=-1)
    counted = np.triu(~(np.asarray(excluded, dtype=bool) | np.eye(m, dtype=bool)), 1)
    if skip is not None:
        counted &= ~np.asarray(skip, dtype=bool)
    cls = np.asarray(cls, dtype=np.int64)
    pc = pair_index(cls[:, None], cls[None, :], C)
    inside = counted & (d < r_max)
    b = np.minimum(np.floor(np.where(inside, d, 0.0) * n_bins / r_max).astype(np.int64), n_bins - 1)
    hist = np.zeros((P, n_bins), dtype=np.int64)
    np.add.at(hist, (pc[inside], b[inside]), 1)
    return {"hist": hist, "beyond": np.bincount(pc[counted & (d >= r_max)], minlength=P).astype(np.int64)}


def near_tie(x, r_max, n_bins):
    """``[m, m]`` bool: the pairs whose fp64 ``d * n_bins / r_max`` lies within ``8 * 2^-24 * n_bins`` of an integer, or whose
    ``d`` lies within ``8 * 2^-24 * r_max`` of ``r_max`` -- where fp32 and fp64 may decide differently."""
    x = np.asarray(x, dtype=np.float64)
    d = np.linalg.norm(x[:, None] - x[None], axis=-1)
    t = d * n_bins / r_max
    eps = 8.0 * 2.0 ** -24
    return (np.abs(t - np.rint(t)) < eps * n_bins) | (np.abs(d - r_max) < eps * r_max)
