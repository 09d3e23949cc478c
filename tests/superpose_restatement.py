"""Numpy restatement of K17 (csrc/superpose.hip): superposed RMSD by Kabsch's SVD with the determinant correction, and the
(value, lowest index) rule of the nearest-neighbour reductions.  Deliberately a different algorithm from the kernel's
(quaternion key matrix, Jacobi): the two agree only if both are right."""
import numpy as np

U = 2.0 ** -52


def centred(x, sel):
    """fp64 coordinates of the atoms ``sel`` of the structures ``x [S,n,3]`` minus their centroid, ``G [S]`` (the sum of
    their squares) and ``bad [S]`` (a non-finite selected coordinate; such a structure is returned as zeros)."""
    X = np.asarray(x)[:, np.asarray(sel, dtype=np.int64)].astype(np.float64)
    bad = ~np.isfinite(X).all(axis=(1, 2))
    X[bad] = 0.0
    X = X - X.mean(axis=1, keepdims=True)
    return X, (X * X).sum(axis=(1, 2)), bad


def rmsd2_matrix(a, b, sel=None):
    """``[Sa,Sb]`` squared RMSD after optimal superposition (proper rotations only) over ``sel``; NaN for a bad structure."""
    a, b = np.asarray(a), np.asarray(b)
    sel = np.arange(a.shape[1]) if sel is None else np.asarray(sel, dtype=np.int64)
    A, Ga, bad_a = centred(a, sel)
    B, Gb, bad_b = centred(b, sel)
    M = np.einsum("ikx,jky->ijxy", A, B)
    Um, S, Vt = np.linalg.svd(M)
    d = np.where(np.linalg.det(Um) * np.linalg.det(Vt) < 0, -1.0, 1.0)        # a reflection is not a superposition
    lam = S[..., 0] + S[..., 1] + d * S[..., 2]
    out = np.maximum(0.0, Ga[:, None] + Gb[None, :] - 2.0 * lam) / float(len(sel))
    out[bad_a, :] = np.nan
    out[:, bad_b] = np.nan
    return out


def rmsd2_pair(a, b, sel=None):
    return float(rmsd2_matrix(np.asarray(a)[None], np.asarray(b)[None], sel)[0, 0])


def bound_unit(a, b, sel=None):
    """``2^-52 (G_a[i] + G_b[j]) / m``: what the tests' bounds are multiples of."""
    a = np.asarray(a)
    sel = np.arange(a.shape[1]) if sel is None else np.asarray(sel, dtype=np.int64)
    Ga, Gb = centred(a, sel)[1], centred(b, sel)[1]
    return U * (Ga[:, None] + Gb[None, :]) / float(len(sel))


def min_rule(dense, axis, skip=None):
    """Minimum of ``dense [Sa,Sb]`` along ``axis`` (1: per row over the columns, 0: per column over the rows) and its
    index: NaN entries and the entries of the boolean ``skip`` never count, of equal values the lowest index wins, a line
    without a candidate is ``(+inf, -1)``."""
    D = np.array(dense, dtype=np.float64)
    out = np.isnan(D) if skip is None else (np.isnan(D) | np.asarray(skip, dtype=bool))
    D[out] = np.inf
    if axis == 0:
        D = D.T
    idx = D.argmin(axis=1)                                   # the first of equal minima
    val = D[np.arange(D.shape[0]), idx]
    return val, np.where(np.isinf(val), -1, idx).astype(np.int64)


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))                     # det +1


# a labelled tetrahedron with C2 symmetry only (chiral), centred, whose second moments are diagonal:
# sum x^2 = 8.5, sum y^2 = 4.78125, sum z^2 = 1, all mixed moments 0.  Its mirror image through x = 0 has
# M = diag(-8.5, 4.78125, 1): the best proper rotation reaches lambda = 8.5 + 4.78125 - 1 (the smallest moment is given
# up), so rmsd^2 = (2 * 14.28125 - 2 * 12.28125) / 4 = 4 * 1 / 4 = 1 exactly.
CHIRAL_TETRAHEDRON = np.array([[2.0, -0.375, -0.5], [-2.0, 0.375, -0.5], [0.5, 1.5, 0.5], [-0.5, -1.5, 0.5]])
CHIRAL_MIRROR_RMSD2 = 1.0
