"""The definition of ``coarsegrainingvae_amd.lddt`` restated in ``numpy.float32``, every operation rounded on its own, in the
order the kernel's header gives -- whole ``[m, m]`` tables per structure, no tiles, no words, no caches -- producing every
output of ``cgv_lddt_counts``; and the input generators of the lDDT tests.  Test infrastructure, not a test."""
import numpy as np

F = np.float32


def chain(n, rng):
    """``[n, 3]`` float32: a random walk of 1.5 A steps."""
    step = rng.normal(size=(n, 3))
    step *= 1.5 / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, axis=0).astype(F)


def noisy(ref, S, sigma, rng):
    """``[S, n, 3]`` float32: the reference plus Gaussian noise of ``sigma`` per coordinate."""
    ref = np.asarray(ref, dtype=np.float64)
    return (ref[None] + rng.normal(0.0, sigma, (S,) + ref.shape)).astype(F)


def cloud_radius(n):
    """The inclusion radius of the random-cloud cases.  A walk of ``n`` steps of 1.5 A spans about ``1.5 sqrt(n)``: under the
    default 15 A every pair of a chain of up to some 60 atoms is included, and a case with everything counted proves
    nothing.  ``1.5 sqrt(n / 2)``, at most 15: from the chain's geometry alone."""
    return min(15.0, 1.5 * float(np.sqrt(n / 2.0)))


def chain_bonds(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)


def sq_dist2(a, b):
    """``(dx*dx + dy*dy) + dz*dz`` in fp32 of ``a [..., 3] - b [..., 3]`` (broadcast)."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def radius2_of(R0):
    return F(R0) * F(R0)


def pair_tests(x_rows, x_all, ref_rows, ref_all, r_rows, r_all, radius2, t, tol):
    """The raw tests (no masks) of the ordered pairs rows x all of one structure: ``included [R, m]``, ``preserved
    [4, R, m]`` and ``clash [R, m]`` bool."""
    with np.errstate(invalid="ignore", over="ignore"):
        q0 = sq_dist2(np.asarray(ref_rows)[:, None, :], np.asarray(ref_all)[None, :, :])
        q = sq_dist2(np.asarray(x_rows)[:, None, :], np.asarray(x_all)[None, :, :])
        included = q0 < F(radius2)
        e = np.abs(np.sqrt(q) - np.sqrt(q0))
        assert e.dtype == F
        preserved = np.stack([included & (e < F(tk)) for tk in t])
        c = (np.asarray(r_rows, dtype=F)[:, None] + np.asarray(r_all, dtype=F)[None, :]) - F(tol)
        clash = (c > 0) & (q < c * c)
    return included, preserved, clash


def lddt_counts(xyz, ref_xyz, ref_index, sel, excl_lddt, excl_clash, radii, R0=15.0, thresholds=(0.5, 1, 2, 4), tol=0.4):
    """Every output of ``cgv_lddt_counts`` for the caller's tables: ``struct_counts [S, 6]`` (``-1``: bad), ``atom_counts
    [m, 6]``, ``bad [S]``, and ``n_pairs``: the unordered pairs outside ``excl_lddt`` / ``excl_clash`` of a structure."""
    xyz, ref_xyz = np.asarray(xyz, dtype=F), np.asarray(ref_xyz, dtype=F)
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    m, S = sel.shape[0], xyz.shape[0]
    eye = np.eye(m, dtype=bool)
    ok_l, ok_c = ~(np.asarray(excl_lddt, dtype=bool) | eye), ~(np.asarray(excl_clash, dtype=bool) | eye)
    upper = np.triu(np.ones((m, m), dtype=bool), 1)
    radius2, t = radius2_of(R0), [F(v) for v in thresholds]
    struct = np.zeros((S, 6), dtype=np.int64)
    atom = np.zeros((m, 6), dtype=np.int64)
    bad = np.zeros(S, dtype=bool)
    for s in range(S):
        x, ref = xyz[s, sel], ref_xyz[int(ref_index[s]), sel]
        if not (np.isfinite(x).all() and np.isfinite(ref).all()):
            bad[s], struct[s] = True, -1
            continue
        included, preserved, clash = pair_tests(x, x, ref, ref, radii, radii, radius2, t, tol)
        tables = [included & ok_l] + [p & ok_l for p in preserved] + [clash & ok_c]
        for k, tab in enumerate(tables):
            struct[s, k] = int((tab & upper).sum())
            atom[:, k] += tab.sum(axis=1)
    return {"struct_counts": struct, "atom_counts": atom, "bad": bad,
            "n_pairs": (int((ok_l & upper).sum()), int((ok_c & upper).sum()))}


def atom_rows(rows, x, ref, sel, excl_lddt, excl_clash, radii, R0=15.0, thresholds=(0.5, 1, 2, 4), tol=0.4):
    """``atom_counts[rows]`` of ONE good structure, computed row-wise (``[len(rows), m]`` tables only)."""
    sel, rows = np.asarray(sel, dtype=np.int64).reshape(-1), np.asarray(rows, dtype=np.int64).reshape(-1)
    xs, rs, r = np.asarray(x, dtype=F)[sel], np.asarray(ref, dtype=F)[sel], np.asarray(radii, dtype=F)
    off = np.arange(sel.shape[0])[None, :] != rows[:, None]
    ok_l, ok_c = ~np.asarray(excl_lddt, dtype=bool)[rows] & off, ~np.asarray(excl_clash, dtype=bool)[rows] & off
    included, preserved, clash = pair_tests(xs[rows], xs, rs[rows], rs, r[rows], r, radius2_of(R0), [F(v) for v in thresholds], tol)
    tables = [included & ok_l] + [p & ok_l for p in preserved] + [clash & ok_c]
    return np.stack([tab.sum(axis=1) for tab in tables], axis=1).astype(np.int64)


def shares(w):
    """What the cloud guard looks at, from a restatement's numbers over its good structures: the included share of the
    pairs outside ``excl_lddt``, the preserved share at each threshold, the clash share of the pairs outside
    ``excl_clash``."""
    good = ~w["bad"]
    tot = w["struct_counts"][good].sum(axis=0).astype(np.float64)
    n = float(good.sum())
    return {"included": tot[0] / (n * w["n_pairs"][0]), "preserved": [tot[1 + k] / tot[0] for k in range(4)],
            "clash": tot[5] / (n * w["n_pairs"][1])}


def lddt64(x, ref, excluded, R0=15.0, thresholds=(0.5, 1, 2, 4)):
    """An independent fp64 lDDT of one structure: plain ``numpy.linalg.norm``."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.linalg.norm(x[:, None] - x[None], axis=-1)
    d0 = np.linalg.norm(ref[:, None] - ref[None], axis=-1)
    pairs = np.triu(~np.asarray(excluded, dtype=bool), 1) & (d0 < R0)
    kept = [(np.abs(d - d0)[pairs] < tk).sum() for tk in thresholds]
    return float(np.mean(kept) / pairs.sum()) if pairs.sum() else float("nan")


def near_tie(x, ref, R0=15.0, thresholds=(0.5, 1, 2, 4), eps=1e-4):
    """``[m, m]`` bool, symmetric: the pairs whose ``|d - d0|`` lies within ``eps`` of a threshold or whose ``d0`` lies
    within ``eps`` of ``R0`` (fp64) -- where fp32 and fp64 may decide differently."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.linalg.norm(x[:, None] - x[None], axis=-1)
    d0 = np.linalg.norm(ref[:, None] - ref[None], axis=-1)
    tie = np.abs(d0 - R0) < eps
    for tk in thresholds:
        tie |= np.abs(np.abs(d - d0) - tk) < eps
    return tie | tie.T
