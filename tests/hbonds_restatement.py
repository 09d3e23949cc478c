"""The hydrogen bonds of an ensemble restated in numpy.float32, operation for operation as ``csrc/hbond.hip`` defines
them: ``d2`` and ``l2`` with the operation order of ``csrc/sq_dist.h``, the dot product ``(ux*vx + uy*vy) + uz*vz`` of
``u = D - H`` and ``v = A - H``, every product and sum an array operation of its own, and the three strict tests
``d2 < cutoff2``, ``dot < 0``, ``dot*dot > (c2 * l2) * d2``.  The tables and masks are the caller's; every output of the
kernel is produced.  Also the same decision in fp64 with an ``arccos``, and a molecule with a wanted table."""
import math

import numpy as np

F = np.float32


def cutoff2_of(cutoff):
    c = F(cutoff)
    return F(c * c)


def c2_of(angle):
    return F(math.cos(math.radians(float(angle))) ** 2)


def sq_dist2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def terms(D, H, A):
    """``(d2, l2, dot)`` of fp32 positions ``[..., 3]`` that broadcast against each other."""
    D, H, A = (np.asarray(v, dtype=F) for v in (D, H, A))
    u, v = D - H, A - H
    dot = (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]
    return sq_dist2(A, H), sq_dist2(D, H), dot


def bonded(D, H, A, cutoff2, c2):
    with np.errstate(invalid="ignore", over="ignore"):
        d2, l2, dot = terms(D, H, A)
        return (d2 < F(cutoff2)) & (dot < F(0)) & (dot * dot > (F(c2) * l2) * d2)


def pack(mask):
    """Bool ``[..., nA]`` as uint64 ``[..., ceil(nA / 64)]``: bit ``a & 63`` of word ``a >> 6``, written out bit by bit."""
    mask = np.asarray(mask, dtype=bool)
    nA = mask.shape[-1]
    out = np.zeros(mask.shape[:-1] + ((nA + 63) // 64,), dtype=np.uint64)
    for a in range(nA):
        out[..., a >> 6] |= mask[..., a].astype(np.uint64) << np.uint64(a & 63)
    return out


def popcount(words):
    w = np.asarray(words, dtype=np.uint64)
    return np.unpackbits(np.ascontiguousarray(w).view(np.uint8).reshape(*w.shape, 8), axis=-1).sum(axis=(-1, -2)).astype(np.int64)


def bad_structures(xyz, don_h, don_d, acc):
    used = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1) for t in (don_h, don_d, acc)])
    return ~np.isfinite(np.asarray(xyz, dtype=F)[:, used]).all(axis=(1, 2))


def hbond_counts(xyz, don_h, don_d, acc, excluded, native=None, h_a_cutoff=2.5, angle=120.0):
    """Every output of ``cgv_hbond_counts`` from bool masks ``excluded`` / ``native`` ``[nH, nA]``: ``pair_counts``,
    ``n_hbonds``, ``n_native``, ``bad``, ``n_good``, ``bits`` and the bool table ``bonds [S, nH, nA]``."""
    x = np.asarray(xyz, dtype=F)
    don_h, don_d, acc = (np.asarray(t, dtype=np.int64).reshape(-1) for t in (don_h, don_d, acc))
    allowed = ~np.asarray(excluded, dtype=bool)
    H, D, A = x[:, don_h][:, :, None, :], x[:, don_d][:, :, None, :], x[:, acc][:, None, :, :]
    hit = bonded(D, H, A, cutoff2_of(h_a_cutoff), c2_of(angle)) & allowed[None]
    bad = bad_structures(x, don_h, don_d, acc)
    hit[bad] = False
    nat = np.zeros_like(allowed) if native is None else np.asarray(native, dtype=bool)
    n_hbonds = hit.sum(axis=(1, 2)).astype(np.int64)
    n_native = (hit & nat[None]).sum(axis=(1, 2)).astype(np.int64)
    n_hbonds[bad], n_native[bad] = -1, -1
    return {"pair_counts": hit.sum(axis=0).astype(np.int64), "n_hbonds": n_hbonds, "n_native": n_native, "bad": bad,
            "n_good": int((~bad).sum()), "bits": pack(hit), "bonds": hit}


# ----------------------------------------------------------------------------- the same decision in fp64
def geometry64(D, H, A):
    """``(distance H...A, angle D-H...A in degrees)`` in fp64 of the fp32 positions."""
    D, H, A = (np.asarray(v, dtype=F).astype(np.float64) for v in (D, H, A))
    u, v = D - H, A - H
    d, l = np.linalg.norm(v, axis=-1), np.linalg.norm(u, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cosine = np.clip((u * v).sum(-1) / (l * d), -1.0, 1.0)
    return d, np.degrees(np.arccos(cosine))


def bonded64(D, H, A, h_a_cutoff=2.5, angle=120.0):
    d, theta = geometry64(D, H, A)
    return (d < float(F(h_a_cutoff))) & (theta > float(angle))


def near_tie(D, H, A, h_a_cutoff=2.5, angle=120.0, tol_deg=1e-3, tol_len=1e-5):
    """fp64 puts the angle within ``tol_deg`` degrees of its threshold or the distance within ``tol_len`` Angstrom of its
    own: fp32 rounding may decide the pair."""
    d, theta = geometry64(D, H, A)
    return (np.abs(theta - float(angle)) < tol_deg) | (np.abs(d - float(F(h_a_cutoff))) < tol_len)


def triple(distance, theta_deg, l=1.0):
    """``(D, H, A)`` fp64 with H at the origin, D at ``l`` on -x, and A at ``distance`` from H at the angle ``theta_deg``
    to D (180: linear), in the xy plane."""
    t = math.radians(theta_deg)
    return (np.array([-l, 0.0, 0.0]), np.zeros(3), np.array([-distance * math.cos(t), distance * math.sin(t), 0.0]))


# ----------------------------------------------------------------------------- a molecule with a wanted table
DONORS, ACCEPTORS = (7,), (8,)            # the elements under which ``molecule`` has the wanted table


def molecule(nH, nA, n_excluded=0):
    """``(z, bonds)`` whose table is ``nH`` donor hydrogens x ``nA`` acceptors with ``donor_elements=DONORS`` and
    ``acceptor_elements=ACCEPTORS``: ``nH`` N-H pairs and ``nA`` oxygens, in the order hydrogens (atoms ``0 .. nH-1``),
    nitrogens, oxygens.  The first ``n_excluded`` nitrogens are bonded to an oxygen each (oxygen ``5 k mod nA`` to nitrogen
    ``k``): those pairs are excluded by the bond graph."""
    z = [1] * nH + [7] * nH + [8] * nA
    bonds = [(h, nH + h) for h in range(nH)] + [(nH + k, 2 * nH + (5 * k) % nA) for k in range(min(n_excluded, nH))]
    return np.array(z), np.array(bonds)


def cloud(z, bonds, S, sigma, rng, l=1.0):
    """``xyz [S, n, 3]`` fp32: heavy atoms from N(0, sigma), every hydrogen ``l`` away from its heavy atom in a random
    direction."""
    z, bonds = np.asarray(z), np.asarray(bonds)
    xyz = rng.normal(0.0, sigma, (S, z.shape[0], 3))
    for h, d in bonds.tolist():
        if z[h] != 1:
            continue
        v = rng.normal(0.0, 1.0, (S, 3))
        xyz[:, h] = xyz[:, d] + l * v / np.linalg.norm(v, axis=1, keepdims=True)
    return xyz.astype(F)
