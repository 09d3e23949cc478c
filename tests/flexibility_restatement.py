"""numpy fp64 restatement of K21 (csrc/align_mean.hip) and of ``flexibility.mean_structure``: the rotation comes from
``numpy.linalg.eigh`` of the same quaternion key matrix, generalised Procrustes follows the same start, stop rule and
formulas.  It also returns what a tolerance is derived from: the gap under the key matrix's top eigenvalue and its
Frobenius norm."""
import numpy as np


def key_matrix(M):
    """The symmetric 4 x 4 key matrix of the cross-covariance ``M[i, j] = sum_k a_k[i] b_k[j]`` (csrc/superpose_eig.h)."""
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = np.asarray(M, dtype=np.float64)
    return np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                     [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                     [zx - xz, xy + yx, -xx + yy - zz, yz + zy],
                     [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])


def rotation_of(q):
    q0, qx, qy, qz = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                     [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                     [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])


def rotation(M):
    """``(R, lambda, gap, |K|_F)``: the proper rotation with ``y = R a`` closest to ``b``, the top eigenvalue of the key
    matrix, its distance from the next one, and the key matrix's Frobenius norm."""
    K = key_matrix(M)
    w, v = np.linalg.eigh(K)
    return rotation_of(v[:, 3]), float(w[3]), float(w[3] - w[2]), float(np.linalg.norm(K))


def align_accumulate(xyz, sel, ref):
    """One pass of fp32 structures ``xyz [S,n,3]`` against ``ref [n,3]`` over ``sel``.  Returns a dict: ``sum [n,3]``,
    ``dev2 [n]``, ``n_good``, ``rmsd2 [S]`` (NaN: bad), ``bad [S]``, ``aligned [S,n,3]`` fp64 (NaN rows: bad), and per
    structure ``gap``, ``knorm`` (key matrix), ``g`` (G_a + G_b) and ``terms`` -- ``abs_sum [n]`` / ``abs_dev2 [n]``, the
    sums of the absolute values of what went into ``sum`` (largest component) and ``dev2``."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    S, n = x.shape[:2]
    m = sel.shape[0]
    b = np.asarray(ref, dtype=np.float64)
    b = b - b[sel].mean(0)
    gb = float((b[sel] ** 2).sum())
    out = {"sum": np.zeros((n, 3)), "dev2": np.zeros(n), "n_good": 0, "rmsd2": np.full(S, np.nan), "bad": np.zeros(S, dtype=bool),
           "aligned": np.full((S, n, 3), np.nan), "gap": np.full(S, np.nan), "knorm": np.full(S, np.nan), "g": np.full(S, np.nan),
           "abs_sum": np.zeros(n), "abs_dev2": np.zeros(n)}
    for s in range(S):
        if not np.isfinite(x[s]).all():
            out["bad"][s] = True
            continue
        a = x[s] - x[s][sel].mean(0)
        R, lam, gap, knorm = rotation(a[sel].T @ b[sel])
        y = a @ R.T
        ga = float((a[sel] ** 2).sum())
        out["rmsd2"][s] = max(0.0, ga + gb - 2.0 * lam) / m
        out["gap"][s], out["knorm"][s], out["g"][s] = gap, knorm, ga + gb
        out["aligned"][s] = y
        out["sum"] += y
        d2 = ((y - b) ** 2).sum(1)
        out["dev2"] += d2
        out["abs_sum"] += np.abs(y).max(1)
        out["abs_dev2"] += d2
        out["n_good"] += 1
    return out


def mean_structure(xyz, sel=None, max_iter=10, tol=1e-4):
    """``flexibility.mean_structure`` on the host; the same keys, plus ``passes``: the ``align_accumulate`` results of
    every pass, the last one included."""
    x = np.asarray(xyz, dtype=np.float32)
    S, n = x.shape[:2]
    sel = np.arange(n) if sel is None else np.asarray(sel, dtype=np.int64).reshape(-1)
    good = np.isfinite(x.reshape(S, -1)).all(1)
    if not good.any():
        return {"mean": None, "rmsf": None, "rmsd": np.full(S, np.nan), "bad": np.ones(S, dtype=bool), "n_good": 0, "iterations": 0,
                "converged": False, "last_move": None, "passes": []}
    target = x[int(np.flatnonzero(good)[0])].astype(np.float64)
    passes, converged, move = [], False, None
    for _ in range(int(max_iter)):
        res = align_accumulate(x, sel, target)
        passes.append(res)
        new = res["sum"] / res["n_good"]
        d = (new - (target - target[sel].mean(0)))[sel]
        move = float(np.sqrt((d * d).sum(1).mean()))
        target = new
        if move < tol:
            converged = True
            break
    res = align_accumulate(x, sel, target)
    passes.append(res)
    mean = res["sum"] / res["n_good"]
    shift = mean - (target - target[sel].mean(0))
    msf = np.maximum(res["dev2"] / res["n_good"] - (shift * shift).sum(1), 0.0)
    return {"mean": mean, "rmsf": np.sqrt(msf), "rmsd": np.sqrt(res["rmsd2"]), "bad": res["bad"], "n_good": res["n_good"],
            "iterations": len(passes), "converged": converged, "last_move": move, "passes": passes}


def group_profile(rmsf, sel, labels):
    """Per group (ascending label) the root of the mean of its selected atoms' mean-square fluctuations."""
    r = np.asarray(rmsf, dtype=np.float64)[np.asarray(sel, dtype=np.int64)]
    ids = sorted(set(int(v) for v in labels))
    return ids, np.array([np.sqrt(np.mean([r[k] ** 2 for k in range(len(r)) if int(labels[k]) == g])) for g in ids])


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def noisy_copies(rng, base, S, sigma):
    """``S`` copies of ``base [n,3]``, each with Gaussian noise of per-atom (or scalar) ``sigma`` added, then randomly
    rotated and translated; fp32."""
    base = np.asarray(base, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (base.shape[0],))
    out = np.empty((S,) + base.shape, dtype=np.float32)
    for s in range(S):
        y = base + rng.standard_normal(base.shape) * sigma[:, None]
        out[s] = (y @ random_rotation(rng).T + rng.uniform(-5, 5, 3)).astype(np.float32)
    return out
