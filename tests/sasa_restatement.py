"""The solvent-accessible surface of an ensemble restated in numpy.float32, operation for operation as
``csrc/sasa.hip`` defines it: the point ``c_i + r_i * u_k`` per component (the product an array operation of its own,
then the sum), the squared distance ``(dx*dx + dy*dy) + dz*dz`` with the operation order of ``csrc/sq_dist.h``, tested
with strict ``<`` against ``r_j * r_j``, every ``j != i`` by position.  No pre-filter and no early exit: every point is
tested against every other selected atom.  Also the exact cap count of two atoms on the z axis."""
import math

import numpy as np

BONDI = {1: 1.20, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.80, 16: 1.80, 17: 1.75}


def sphere_points(P):
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    rho = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1).astype(np.float32)


def inflated(R, probe=1.4):
    return np.asarray(R, dtype=np.float32) + np.float32(probe)


def bad_structures(xyz, sel):
    return ~np.isfinite(np.asarray(xyz, dtype=np.float32)[:, np.asarray(sel)]).all(axis=(1, 2))


def counts(xyz, sel, r, P):
    """``[S, m]`` int32: exposed points of every selected atom; the rows of a bad structure are -1.  ``r [m]`` fp32: the
    inflated radii."""
    x = np.asarray(xyz, dtype=np.float32)[:, np.asarray(sel)]
    r = np.asarray(r, dtype=np.float32)
    u = sphere_points(P)
    S, m = x.shape[0], x.shape[1]
    r2 = r * r
    out = np.zeros((S, m), dtype=np.int32)
    bad = bad_structures(xyz, sel)
    for s in range(S):
        if bad[s]:
            out[s] = -1
            continue
        c = x[s]
        for i in range(m):
            t = r[i] * u                                      # [P, 3], rounded
            p = c[i][None, :] + t                             # rounded
            dx, dy, dz = p[:, None, 0] - c[None, :, 0], p[:, None, 1] - c[None, :, 1], p[:, None, 2] - c[None, :, 2]
            buried = ((dx * dx + dy * dy) + dz * dz) < r2[None, :]          # [P, m]
            buried[:, i] = False
            out[s, i] = P - int(buried.any(axis=1).sum())
    return out


def sasa_counts(xyz, sel, r, P, cls, n_classes):
    """What ``sasa.sasa_counts`` returns from the device, from ``counts``."""
    cnt = counts(xyz, sel, r, P)
    bad = bad_structures(xyz, sel)
    good = cnt[~bad].astype(np.int64)
    cc = np.zeros((cnt.shape[0], n_classes), dtype=np.int64)
    for c in range(n_classes):
        cc[:, c] = cnt[:, np.asarray(cls) == c].sum(axis=1)
    cc[bad] = -1
    return {"counts": cnt, "class_counts": cc, "atom_sum": good.sum(axis=0), "atom_sumsq": (good * good).sum(axis=0),
            "n_good": int((~bad).sum()), "bad": bad}


# ----------------------------------------------------------------------------- two atoms on the z axis
def cap_threshold(d, r_i, r_j):
    """A point of atom i at height ``z`` (towards j) is inside j's sphere iff ``z > t``."""
    return (d * d + r_i * r_i - r_j * r_j) / (2.0 * d * r_i)


def cap_count(P, d, r_i, r_j, toward=1.0):
    """Exposed points of atom i when the only other atom j is at distance ``d`` along ``toward`` * z: ``#{k : toward z_k
    < t}``; ``P`` when the spheres do not overlap, ``0`` when i lies inside j.  fp64 on the fp32 radii and z_k."""
    d, r_i, r_j = float(d), float(r_i), float(r_j)
    if d >= r_i + r_j:
        return P
    if d + r_i <= r_j:
        return 0
    z = sphere_points(P)[:, 2].astype(np.float64)
    return int((toward * z < cap_threshold(d, r_i, r_j)).sum())


def near_tie(P, d, r_i, r_j, tol=1e-4):
    """Some z_k lies within ``tol`` of the threshold (or the spheres within ``tol`` of a tangency): fp32 rounding may
    decide the point."""
    d, r_i, r_j = float(d), float(r_i), float(r_j)
    if abs(d - (r_i + r_j)) < tol or abs(d + r_i - r_j) < tol:
        return True
    if d >= r_i + r_j or d + r_i <= r_j:
        return False
    z = sphere_points(P)[:, 2].astype(np.float64)
    return bool((np.abs(np.abs(z) - abs(cap_threshold(d, r_i, r_j))) < tol).any())
