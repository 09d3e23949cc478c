"""The three predicates of ``coarsegrainingvae_amd.stereo`` restated in ``numpy.float32``, every operation rounded on its own
-- whole tables per structure in a plain loop over the structures, no tiles, no words, no LDS -- producing every output of
``cgv_stereo_counts``; an independent fp64 form with its margins; and the input generators of the stereochemistry tests.
The comparisons of the crossing test are copied from the header comment of ``csrc/stereo.hip``.  Nothing here is shared with
``stereo.py``, and nothing on the product path imports this.  Test infrastructure, not a test."""
import numpy as np

F = np.float32
MAX_RING = 8
MARGIN = 1e-4                          # below this an fp64 outcome is marginal and left out of a comparison


# ----------------------------------------------------------------------------- fp32, every operation rounded on its own
def cross(u, v):
    """``(u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)`` of fp32 ``[..., 3]``: products first, then the difference."""
    ux, uy, uz, vx, vy, vz = u[..., 0], u[..., 1], u[..., 2], v[..., 0], v[..., 1], v[..., 2]
    a, b = uy * vz, uz * vy
    c, d = uz * vx, ux * vz
    e, f = ux * vy, uy * vx
    out = np.stack([a - b, c - d, e - f], axis=-1)
    assert out.dtype == F
    return out


def dot(u, v):
    """``(u.x*v.x + u.y*v.y) + u.z*v.z`` in fp32."""
    xx, yy, zz = u[..., 0] * v[..., 0], u[..., 1] * v[..., 1], u[..., 2] * v[..., 2]
    out = (xx + yy) + zz
    assert out.dtype == F
    return out


def centre_value(x, centres):
    """``V [C]`` fp32 of ONE structure ``x [n, 3]`` fp32 for ``centres [C, 4]`` = (c, a, b, d)."""
    c, a, b, d = (x[centres[:, k]] for k in range(4))
    return dot(a - c, cross(b - c, d - c))


def torsion_value(x, torsions):
    """``X [Q]`` fp32: cis when ``X > 0``."""
    i, j, k, l = (x[torsions[:, m]] for m in range(4))
    b1, b2, b3 = j - i, k - j, l - k
    return dot(cross(b1, b2), cross(b2, b3))


def crossed(p0, p1, g, v1, v2):
    """The segment ``(p0, p1)`` against the triangle ``(g, v1, v2)``, all fp32 ``[..., 3]`` (broadcast): bool."""
    d, tvec, e1, e2 = p1 - p0, p0 - g, v1 - g, v2 - g
    pv = cross(d, e2)
    det, up = dot(e1, pv), dot(tvec, pv)
    q = cross(tvec, e1)
    vp, tp = dot(d, q), dot(e2, q)
    wp = up + vp
    zero = F(0)
    pos = (det > zero) & (up >= zero) & (vp >= zero) & (wp <= det) & (tp >= zero) & (tp <= det)
    neg = (det < zero) & (up <= zero) & (vp <= zero) & (wp >= det) & (tp <= zero) & (tp >= det)
    return pos | neg


def ring_centre(v):
    """``g`` of the vertices ``v [k, 3]`` fp32: summed in table order, times ``fp32(1 / k)``."""
    g = v[0]
    for t in range(1, v.shape[0]):
        g = g + v[t]
    g = g * (F(1) / F(v.shape[0]))
    assert g.dtype == F
    return g


def pierced(x, ring, bonds):
    """``[B]`` bool of ONE structure: which bonds cross at least one triangle of the fan of ``ring`` (atom indices, no -1)."""
    v = x[np.asarray(ring)]
    k = v.shape[0]
    g = ring_centre(v)
    p0, p1 = x[bonds[:, 0]], x[bonds[:, 1]]
    hit = np.zeros(bonds.shape[0], dtype=bool)
    for t in range(k):
        hit |= crossed(p0, p1, g[None], v[t][None], v[(t + 1) % k][None])
    return hit


def named_atoms(tab):
    r = np.asarray(tab["rings"])
    return np.unique(np.concatenate([np.asarray(tab["centres"]).reshape(-1), np.asarray(tab["torsions"]).reshape(-1), r[r >= 0],
                                     np.asarray(tab["bonds"]).reshape(-1)]).astype(np.int64))


def counts(xyz, tab, want_sign=None, want_cis=None):
    """Every output of ``cgv_stereo_counts`` over all structures, tables in ATOM indices: ``neg``, ``flat [C]``, ``cis [Q]``,
    ``pierced [R, B]`` int64, ``counts [S, 3]`` int32, ``bad [S]`` bool, ``n_good``."""
    with np.errstate(all="ignore"):
        return _counts(np.asarray(xyz, dtype=F), tab, want_sign, want_cis)


def _counts(xyz, tab, want_sign, want_cis):
    centres, torsions, bonds = (np.asarray(tab[k], dtype=np.int64).reshape(-1, w) for k, w in (("centres", 4), ("torsions", 4), ("bonds", 2)))
    rings = [[int(a) for a in row if a >= 0] for row in np.asarray(tab["rings"]).reshape(-1, MAX_RING)]
    tested = np.asarray(tab["tested"], dtype=bool).reshape(len(rings), bonds.shape[0])
    S = xyz.shape[0]
    named = named_atoms(tab)
    neg, flat, cis = np.zeros(centres.shape[0], np.int64), np.zeros(centres.shape[0], np.int64), np.zeros(torsions.shape[0], np.int64)
    through = np.zeros(tested.shape, np.int64)
    per, bad = np.zeros((S, 3), np.int32), np.zeros(S, bool)
    for s in range(S):
        x = xyz[s]
        if not np.isfinite(x[named]).all():
            bad[s] = True
            continue
        if centres.shape[0]:
            V = centre_value(x, centres)
            ng, fl = V < F(0), V == F(0)
            neg += ng
            flat += fl
            if want_sign is not None:
                per[s, 0] = int((np.where(ng, -1, np.where(fl, 0, 1)) != np.asarray(want_sign)).sum())
        if torsions.shape[0]:
            c = torsion_value(x, torsions) > F(0)
            cis += c
            if want_cis is not None:
                per[s, 1] = int((c != (np.asarray(want_cis) != 0)).sum())
        if bonds.shape[0]:
            for r, ring in enumerate(rings):
                hit = pierced(x, ring, bonds) & tested[r]
                through[r] += hit
                per[s, 2] += int(hit.sum())
    return {"neg": neg, "flat": flat, "cis": cis, "pierced": through, "counts": per, "bad": bad, "n_good": int(S - bad.sum())}


# ----------------------------------------------------------------------------- fp64, written another way
def centre64(x, centres):
    """``(negative [C] bool, margin [C])``: the sign of the determinant of the three edge vectors (``numpy.linalg.det``) and
    ``|V| / (|a||b||d|)``."""
    x = np.asarray(x, dtype=np.float64)
    m = np.stack([x[centres[:, k]] - x[centres[:, 0]] for k in (1, 2, 3)], axis=1)
    V = np.linalg.det(m)
    return V < 0, np.abs(V) / np.prod(np.linalg.norm(m, axis=2), axis=1)


def torsion64(x, torsions):
    """``(cis [Q] bool, margin [Q])`` from the dihedral angle itself (``arctan2``): ``|omega| < 90 degrees`` and ``|cos omega|``."""
    x = np.asarray(x, dtype=np.float64)
    i, j, k, l = (x[torsions[:, m]] for m in range(4))
    b1, b2, b3 = j - i, k - j, l - k
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    m1 = np.cross(n1, b2 / np.linalg.norm(b2, axis=1, keepdims=True))
    omega = np.arctan2((m1 * n2).sum(1), (n1 * n2).sum(1))
    return np.abs(omega) < np.pi / 2, np.abs(np.cos(omega))


def crossed64(p0, p1, g, v1, v2):
    """``(crossed [N] bool, margin [N])`` for ``N`` segments against ``N`` triangles: the 3 x 3 system ``g + u (v1 - g) +
    v (v2 - g) = p0 + t (p1 - p0)`` solved by ``numpy.linalg.solve``; margin: the smallest of ``|u|, |v|, |1 - u - v|, |t|,
    |1 - t|`` (0 for a singular system)."""
    p0, p1, g, v1, v2 = (np.asarray(a, dtype=np.float64) for a in (p0, p1, g, v1, v2))
    A = np.stack([v1 - g, v2 - g, p0 - p1], axis=2)
    ok = np.abs(np.linalg.det(A)) > 1e-300
    sol = np.zeros(p0.shape)
    sol[ok] = np.linalg.solve(A[ok], (p0 - g)[ok][..., None])[..., 0]
    u, v, t = sol[:, 0], sol[:, 1], sol[:, 2]
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)
    margin = np.where(ok, np.min(np.abs(np.stack([u, v, 1 - u - v, t, 1 - t])), axis=0), 0.0)
    return inside, margin


# ----------------------------------------------------------------------------- inputs
def cloud(S, n, rng, box=30.0):
    """``[S, n, 3]`` float32: uniform points in a box of ``box`` A."""
    return rng.uniform(0.0, box, size=(S, n, 3)).astype(F)


def segments_and_triangles(N, rng, length=1.5, box=3.0):
    """``N`` random segments of ``length`` A and ``N`` random triangles in a box of ``box`` A, fp32: ``(p0, p1, g, v1, v2)``."""
    p0 = rng.uniform(0.0, box, size=(N, 3))
    d = rng.normal(size=(N, 3))
    p1 = p0 + length * d / np.linalg.norm(d, axis=1, keepdims=True)
    g, v1, v2 = (rng.uniform(0.0, box, size=(N, 3)) for _ in range(3))
    return tuple(a.astype(F) for a in (p0, p1, g, v1, v2))


def _distinct(rng, n, rows, width):
    if rows == 0:
        return np.zeros((0, width), np.int32)
    return np.stack([rng.choice(n, size=width, replace=False) for _ in range(rows)]).astype(np.int32)


def random_tables(rng, n, C, Q, R, B, share_tested=0.8):
    """Tables over ``n`` atoms with no chemistry in them: centres, torsions and bonds of distinct random atoms, rings of every
    size from 3 to 8 in turn, a random ``tested`` (NOT the rule of ``stereo.tables``: the kernel takes any mask)."""
    rings = np.full((R, MAX_RING), -1, np.int32)
    for r in range(R):
        k = 3 + r % 6
        rings[r, :k] = rng.choice(n, size=k, replace=False)
    return {"centres": _distinct(rng, n, C, 4), "torsions": _distinct(rng, n, Q, 4), "rings": rings, "bonds": _distinct(rng, n, B, 2),
            "tested": rng.uniform(size=(R, B)) < share_tested, "n_atoms": n}


def polygon(k, radius=1.4, centre=(0.0, 0.0, 0.0)):
    """A regular ``k``-gon in the plane ``z = centre.z``, ``[k, 3]`` fp32."""
    a = 2.0 * np.pi * np.arange(k) / k
    return (np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(k)], axis=1) + np.asarray(centre)).astype(F)


def one_ring(k, segments):
    """``k``-gon of atoms 0 .. k-1 about the origin in z = 0, then two atoms per segment: (tables, xyz [1, n, 3])."""
    ring = polygon(k)
    x = np.concatenate([ring, np.asarray(segments, dtype=F).reshape(-1, 3)])
    B = len(segments)
    rings = np.full((1, 8), -1, np.int32)
    rings[0, :k] = np.arange(k)
    bonds = (k + np.arange(2 * B).reshape(B, 2)).astype(np.int32)
    tab = {"centres": np.zeros((0, 4), np.int32), "torsions": np.zeros((0, 4), np.int32), "rings": rings, "bonds": bonds,
           "tested": np.ones((1, B), bool), "n_atoms": x.shape[0]}
    return tab, x[None]


HEXAGON_CASES = [(((0.2, 0.1, -1), (0.2, 0.1, 1)), True),            # through the ring, off its centre
                 (((0, 0, -1), (0, 0, 1)), True),                    # through g itself: a corner of all six triangles, counted once
                 (((0.5, 0, -1), (0.5, 0, 1)), True),                # through the fan edge from g to vertex 0: once
                 (((3, 0, -1), (3, 0, 1)), False),                   # outside
                 (((-1, 0.2, 0), (1, 0.2, 0)), False),               # coplanar: det == 0
                 (((0.2, 0.1, 2), (0.2, 0.1, 0.5)), False),          # stops short of the plane
                 (((0.2, 0.1, 1), (0.2, 0.1, 0)), True),             # ends exactly in the plane: inclusive
                 (((0.2, 0.1, 0), (0.2, 0.1, 1)), True)]             # begins exactly in it


# ACE - PHE - NME with all its hydrogens, and a chlorine molecule beside it (atoms 32, 33: a bond that belongs to nothing and
# can be threaded through the ring without moving anything else)
PHE_Z = np.array([6, 1, 1, 1, 6, 8,  7, 1, 6, 1, 6, 1, 1, 6, 6, 1, 6, 1, 6, 1, 6, 1, 6, 1, 6, 8,  7, 1, 6, 1, 1, 1,  17, 17])
PHE_BONDS = np.array([[0, 1], [0, 2], [0, 3], [0, 4], [4, 5], [4, 6], [6, 7], [6, 8], [8, 9], [8, 10], [10, 11], [10, 12], [10, 13], [13, 14],
                      [14, 15], [14, 16], [16, 17], [16, 18], [18, 19], [18, 20], [20, 21], [20, 22], [22, 23], [22, 13], [8, 24], [24, 25],
                      [24, 26], [26, 27], [26, 28], [28, 29], [28, 30], [28, 31], [32, 33]])
PHE = {"CA": 8, "HA": 9, "ring": [13, 14, 16, 18, 20, 22], "omega": [(0, 4, 6, 8), (8, 24, 26, 28)], "nme": [28, 29, 30, 31], "cl": (32, 33)}


def phe_base():
    """One conformation of the molecule above, ``[34, 3]`` fp64: the ring a regular hexagon about the origin in ``z = 0``."""
    x = np.zeros((34, 3))
    hexa = polygon(6).astype(np.float64)
    for t, a in enumerate(PHE["ring"]):
        x[a] = hexa[t]
    for a, h in ((14, 15), (16, 17), (18, 19), (20, 21), (22, 23)):
        x[h] = x[a] * (2.48 / 1.4)
    x[10], x[11], x[12] = (2.9, 0.0, 0.0), (3.2, -0.7, 0.7), (3.2, -0.6, -0.8)
    x[8], x[9], x[6], x[7] = (3.6, 1.2, 0.5), (3.2, 1.9, 1.2), (5.0, 1.0, 0.9), (5.5, 1.8, 1.2)
    x[4], x[5], x[0] = (5.8, -0.1, 0.6), (5.3, -1.2, 0.3), (7.3, 0.0, 0.8)
    x[1], x[2], x[3] = (7.7, 0.9, 0.4), (7.7, -0.8, 0.2), (7.5, -0.1, 1.9)
    x[24], x[25], x[26], x[27] = (3.4, 1.9, -0.8), (2.5, 2.7, -1.0), (4.4, 1.7, -1.8), (5.1, 1.0, -1.6)
    x[28], x[29], x[30], x[31] = (4.4, 2.4, -3.1), (5.4, 2.3, -3.5), (3.7, 1.8, -3.7), (4.1, 3.4, -3.0)
    x[32], x[33] = (0.0, 0.0, 6.0), (0.0, 0.0, 8.0)
    x[4], x[24] = x[[0, 5, 6]].mean(0), x[[8, 25, 26]].mean(0)      # the carbonyl carbons are planar: IN the plane of their neighbours
    return x


def phe_frames(S, rng, sigma=0.03):
    """``[S, 34, 3]`` fp32: the base conformation with Gaussian noise of ``sigma`` A on every coordinate."""
    return (phe_base()[None] + rng.normal(0.0, sigma, size=(S, 34, 3))).astype(F)


def invert_ca(x):
    """HA mirrored through the plane of (CA, N, CB): the hand of CA changes, nothing else does."""
    x = np.array(x, dtype=np.float64)
    c, n, cb, ha = x[8], x[6], x[10], x[9]
    normal = np.cross(n - c, cb - c)
    normal /= np.linalg.norm(normal)
    x[9] = ha - 2.0 * np.dot(ha - c, normal) * normal
    return x.astype(F)


def flip_omega(x):
    """The methyl group of NME turned by 180 degrees about the C - N bond of the second peptide bond: omega changes by 180."""
    x = np.array(x, dtype=np.float64)
    j, k = x[24], x[26]
    axis = (k - j) / np.linalg.norm(k - j)
    for a in PHE["nme"]:
        r = x[a] - k
        x[a] = k + 2.0 * np.dot(r, axis) * axis - r
    return x.astype(F)


def thread_ring(x):
    """The chlorine molecule put through the middle of the phenyl ring."""
    x = np.array(x, dtype=np.float64)
    x[32], x[33] = (0.1, 0.05, -1.0), (0.1, 0.05, 1.0)
    return x.astype(F)
