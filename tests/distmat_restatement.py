"""The definition of ``coarsegrainingvae_amd.distmat`` restated in ``numpy.float32`` / ``numpy.rint``, every operation rounded
on its own -- whole ``[m, m]`` tables per structure in a plain loop over the structures, no tiles, no words, no LDS --
producing every output of ``cgv_dist_moments``; an independent fp64 form; and the input generators of the distance-matrix
tests.  Nothing here is shared with ``distmat.py``.  Test infrastructure, not a test."""
import numpy as np

F = np.float32
U = 2.0 ** -24                         # the unit roundoff of fp32
SCALE = 2.0 ** 20
SCALE_DEV = 2.0 ** 12
MAX_RADIUS = 512.0


def cloud(S, n, rng, box=30.0):
    """``[S, n, 3]`` float32: uniform points in a box of ``box`` A."""
    return rng.uniform(0.0, box, size=(S, n, 3)).astype(F)


def sq_dist2(a, b):
    """``(dx*dx + dy*dy) + dz*dz`` in fp32 of ``a [..., 3] - b [..., 3]`` (broadcast), every operation rounded on its own."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    return (xx + yy) + zz


def is_bad(x):
    """Of ONE structure's selected atoms ``x [m, 3]``: a non-finite coordinate, or an atom more than 512 A from the centroid
    (fp64; the kernel sums the centroid in another order, so a structure within an fp64 rounding of 512 A may differ)."""
    if not np.isfinite(x).all():
        return True
    x64 = x.astype(np.float64)
    r2 = ((x64 - x64.mean(0)) ** 2).sum(1)
    return bool(not (r2 <= MAX_RADIUS * MAX_RADIUS).all())


def counted_of(m, mask=None):
    """``[m, m]`` bool: the pairs ``i < j`` that enter the sums."""
    left_out = np.eye(m, dtype=bool) if mask is None else (np.asarray(mask, dtype=bool).reshape(m, m) | np.eye(m, dtype=bool))
    return np.triu(~left_out, 1)


def terms(x, center):
    """Of ONE structure ``x [m, 3]`` against ``center [m, m]`` fp32: ``(d, e, f)`` fp32 ``[m, m]``."""
    q = sq_dist2(x[:, None, :], x[None, :, :])
    d = np.sqrt(q)
    e = d - center
    f = e * e
    assert q.dtype == F and d.dtype == F and e.dtype == F and f.dtype == F
    return d, e, f


def moments(xyz, sel, center=None, mask=None):
    """Every output of ``cgv_dist_moments`` over all structures: ``sum_e``, ``sum_e2 [m, m]`` and ``dev2 [S]`` int64,
    ``bad [S]`` bool, ``n_good``, ``n_pairs``."""
    xyz = np.asarray(xyz, dtype=F)
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    m, S = sel.shape[0], xyz.shape[0]
    ctr = np.zeros((m, m), F) if center is None else np.asarray(center, dtype=F).reshape(m, m)
    counted = counted_of(m, mask)
    a1, a2 = np.zeros((m, m), np.int64), np.zeros((m, m), np.int64)
    dev2, bad = np.zeros(S, np.int64), np.zeros(S, bool)
    for s in range(S):
        x = xyz[s, sel]
        if is_bad(x):
            bad[s] = True
            continue
        _, e, f = terms(x, ctr)
        ie = np.rint(e.astype(np.float64) * SCALE).astype(np.int64)
        i2 = np.rint(f.astype(np.float64) * SCALE).astype(np.int64)
        i12 = np.rint(f.astype(np.float64) * SCALE_DEV).astype(np.int64)
        a1 += np.where(counted, ie, 0)
        a2 += np.where(counted, i2, 0)
        dev2[s] = i12[counted].sum()
    return {"sum_e": a1 + a1.T, "sum_e2": a2 + a2.T, "dev2": dev2, "bad": bad, "n_good": int(S - bad.sum()), "n_pairs": int(counted.sum())}


def mean_std(xyz, sel, mask=None):
    """The two passes: ``(mean [m, m], std [m, m], drmsd [S], center [m, m] fp32)``; entries of pairs that do not count are 0
    (``drmsd``: NaN for a bad structure)."""
    first = moments(xyz, sel, None, mask)
    n = first["n_good"]
    ctr = (first["sum_e"].astype(np.float64) / SCALE / n).astype(F)
    second = moments(xyz, sel, ctr, mask)
    me = second["sum_e"].astype(np.float64) / SCALE / n
    var = np.maximum(second["sum_e2"].astype(np.float64) / SCALE / n - me * me, 0.0)
    dr = np.where(second["bad"], np.nan, np.sqrt(second["dev2"].astype(np.float64) / SCALE_DEV / second["n_pairs"]))
    return ctr.astype(np.float64) + me, np.sqrt(var), dr, ctr


def one_pass_std(xyz, sel, mask=None):
    """What the second pass is for: the standard deviation as ``sqrt(<d^2> - <d>^2)`` from the pass WITHOUT a centre."""
    first = moments(xyz, sel, None, mask)
    n = first["n_good"]
    me = first["sum_e"].astype(np.float64) / SCALE / n
    return np.sqrt(np.maximum(first["sum_e2"].astype(np.float64) / SCALE / n - me * me, 0.0))


def maps64(xyz, sel):
    """An independent fp64 form over the finite structures: ``(d [S, m, m], mean [m, m], std [m, m])`` with
    ``numpy.linalg.norm`` and ``numpy.std``."""
    x = np.asarray(xyz, dtype=np.float64)[:, np.asarray(sel)]
    d = np.linalg.norm(x[:, :, None, :] - x[:, None, :, :], axis=-1)
    return d, d.mean(0), d.std(0)


# ----------------------------------------------------------------------------- error bounds, from u = 2^-24 alone
def root_change(x, eta):
    """How far ``sqrt`` can move when its argument ``x >= 0`` moves by at most ``eta``: ``|sqrt(x') - sqrt(x)| =
    |x' - x| / (sqrt(x') + sqrt(x)) <= min(sqrt(eta), eta / sqrt(x))``."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.minimum(np.sqrt(eta), eta / np.sqrt(x))


def distance_bound(d_max):
    """``|d32 - d64| <= 4 u d``: one ``u`` per rounded operation of ``sq_dist2`` on the way to ``q`` (a difference, its
    square, two sums), halved by the root, plus the root's own."""
    return 4.0 * U * d_max


def mean_bound(d_max):
    """``|mean - mean64| <= 4 u d_max + 2^-21``: every term's distance error, and half a unit of the 2^-20 fixed point of
    ``sum_e`` per term (the mean of the terms' roundings is no larger than the largest)."""
    return distance_bound(d_max) + 2.0 ** -21


def std_bound(std64, d_max):
    """The two-pass standard deviation.  With ``a = 4 u d_max``: the fp32 deviations ``e`` differ from the fp64 ones by at most
    ``a`` each (``d - center`` is one more rounded difference, of at most ``u |e|``, inside the slack of ``a``: the count above
    is 3.5 u), and the standard deviation is a norm, so that of the fp32 deviations is within ``a`` of ``std64``.  On top of
    that the VARIANCE moves by ``eta``: ``u`` relative for the rounded square, on ``<e^2> <= (std64 + a)^2 + mu^2``; half a
    unit ``2^-21`` of the fixed point of ``sum_e2``; and ``(2 mu + 2^-21) 2^-21`` for the fixed point of ``sum_e`` in ``<e>^2``,
    where ``|<e>| <= mu = a + u d_max + 2^-20`` (the centre is the first pass's mean rounded to fp32).  So
    ``|std - std64| <= a + root_change(std64^2, eta)``."""
    a = distance_bound(d_max)
    mu = a + U * d_max + 2.0 ** -20
    eta = U * ((std64 + a) ** 2 + mu * mu) + 2.0 ** -21 + (2.0 * mu + 2.0 ** -21) * 2.0 ** -21
    return a + root_change(np.square(std64), eta)


def drmsd_bound(drmsd64, d_max):
    """The distance RMSD to a map held in fp32: an RMS over the pairs is a norm, so the distance errors move it by at most
    ``a = 4 u d_max``; its square then moves by ``u`` relative (the rounded square of every term) and by half a unit ``2^-13``
    of the 2^-12 fixed point of ``dev2``."""
    a = distance_bound(d_max)
    eta = U * (drmsd64 + a) ** 2 + 2.0 ** -13
    return a + root_change(np.square(drmsd64), eta)
