"""Test-side restatement of the internal-coordinate histograms (K15, csrc/internal_hist.hip) in plain numpy fp64, one
structure and one feature at a time, and the molecules its tests use.  It lives in the tests only: nothing on the product
path imports it, and it is no fallback for a missing kernel.

Formulas and bin rule are those of include/cgvae_hip.h, written out with scalar arithmetic:
  bond     |p0 - p1|                                    [lo, hi): under below lo, over at or above hi
  angle    atan2(|u x v|, u . v), u = p0 - p1, v = p2 - p1   [0, pi], pi in the last bin
  torsion  atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))   [-pi, pi) periodic, pi in bin 0
  bin = floor((x - lo) * n_bins / (hi - lo));  a feature that touches a non-finite coordinate is invalid.
Row layout: [under, n_bins bins, over, invalid].
"""
import math

import numpy as np

BOND, ANGLE, TORSION = 2, 3, 4


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def value(x, rec, kind):
    """The feature's value for ONE structure ``x [n,3]`` (any float type: widened to fp64), or ``None`` when one of its
    atoms has a non-finite coordinate."""
    p = [tuple(float(c) for c in x[int(rec[a])]) for a in range(kind)]
    if not all(math.isfinite(c) for q in p for c in q):
        return None
    if kind == BOND:
        d = _sub(p[0], p[1])
        return math.sqrt(_dot(d, d))
    if kind == ANGLE:
        u, v = _sub(p[0], p[1]), _sub(p[2], p[1])
        c = _cross(u, v)
        return math.atan2(math.sqrt(_dot(c, c)), _dot(u, v))
    b1, b2, b3 = _sub(p[1], p[0]), _sub(p[2], p[1]), _sub(p[3], p[2])
    c23, c12 = _cross(b2, b3), _cross(b1, b2)
    return math.atan2(math.sqrt(_dot(b2, b2)) * _dot(b1, c23), _dot(c12, c23))


def window(kind, bond_range):
    return {BOND: (float(bond_range[0]), float(bond_range[1])), ANGLE: (0.0, math.pi), TORSION: (-math.pi, math.pi)}[kind]


def position(val, kind, n_bins, bond_range):
    """``(x - lo) * n_bins / (hi - lo)`` before the floor: the distance to the next integer, in bin widths, is what the
    GPU test's acceptance rule looks at."""
    lo, hi = window(kind, bond_range)
    return (val - lo) * n_bins / (hi - lo)


def slot(val, kind, n_bins, bond_range):
    """Index into a feature's row ``[under, bins, over, invalid]``."""
    if val is None:
        return n_bins + 2
    lo, hi = window(kind, bond_range)
    b = math.floor(position(val, kind, n_bins, bond_range))
    if kind == TORSION:
        return 1 + (b if 0 <= b < n_bins else 0)
    if kind == ANGLE:
        return 1 + min(max(b, 0), n_bins - 1)
    if val < lo:
        return 0
    if val >= hi:
        return n_bins + 1
    return 1 + min(max(b, 0), n_bins - 1)


def values(xyz, feat, kind):
    """``[S][Nf]`` values (``None``: invalid) of the structures ``xyz [S,n,3]``."""
    feat, kind = np.asarray(feat).reshape(-1, 4), np.asarray(kind).reshape(-1)
    return [[value(x, feat[f], int(kind[f])) for f in range(len(kind))] for x in np.asarray(xyz)]


def restate_from(vals, kind, pairs, n_bins, n_bins2, bond_range):
    """``counts [Nf, n_bins + 3]`` and ``pair_counts [Np, n_bins2, n_bins2]`` (int64) from the rows of ``values``."""
    kind = np.asarray(kind).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    counts = np.zeros((len(kind), n_bins + 3), np.int64)
    pair_counts = np.zeros((len(pairs), n_bins2, n_bins2), np.int64)
    for row in vals:
        for f, v in enumerate(row):
            counts[f, slot(v, int(kind[f]), n_bins, bond_range)] += 1
        for p, (f, g) in enumerate(pairs):
            if row[f] is not None and row[g] is not None:
                pair_counts[p, slot(row[f], TORSION, n_bins2, bond_range) - 1, slot(row[g], TORSION, n_bins2, bond_range) - 1] += 1
    return counts, pair_counts


def restate(xyz, feat, kind, pairs, n_bins, n_bins2, bond_range):
    """``counts`` and ``pair_counts`` of ``xyz [S,n,3]``."""
    return restate_from(values(xyz, feat, kind), kind, pairs, n_bins, n_bins2, bond_range)


def well_conditioned(x, feat, kind, configs, edge=1e-9, min_sin=1e-3):
    """The acceptance rule of the GPU tests for ONE structure: every value at least ``edge`` of a bin width from every bin
    edge, for every ``(n_bins, n_bins2, bond_range)`` of ``configs`` it is histogrammed with (a torsion also with
    ``n_bins2``: it may be half of a pair), and every angle a torsion is built on (p0-p1-p2 and p1-p2-p3) with
    ``sin >= min_sin``.  Only then is "the same bin" a fair demand of two fp64 evaluations that may differ in their last
    bits (atan2, sqrt, the order of a sum)."""
    feat, kind = np.asarray(feat).reshape(-1, 4), np.asarray(kind).reshape(-1)
    for f in range(len(kind)):
        k = int(kind[f])
        v = value(x, feat[f], k)
        if v is None:
            return False
        for n_bins, n_bins2, bond_range in configs:
            for nb in ((n_bins, n_bins2) if k == TORSION else (n_bins,)):
                pos = position(v, k, nb, bond_range)
                if abs(pos - round(pos)) < edge:
                    return False
        if k == TORSION:
            for tri in (feat[f][:3], feat[f][1:]):
                if math.sin(value(x, tri, ANGLE)) < min_sin:
                    return False
    return True


# ----------------------------------------------------------------------------- molecules
# Alanine dipeptide ACE-ALA-NME, 22 atoms, written out by hand (the usual all-atom order):
#  0 H1   1 CH3  2 H2   3 H3   4 C    5 O        ACE
#  6 N    7 H    8 CA   9 HA  10 CB  11 HB1 12 HB2 13 HB3 14 C  15 O      ALA
# 16 N   17 H   18 C   19 H1  20 H2  21 H3       NME
ALA_Z = np.array([1, 6, 1, 1, 6, 8, 7, 1, 6, 1, 6, 1, 1, 1, 6, 8, 7, 1, 6, 1, 1, 1])
ALA_BONDS = np.array([(0, 1), (1, 2), (1, 3), (1, 4), (4, 5), (4, 6), (6, 7), (6, 8), (8, 9), (8, 10), (10, 11), (10, 12),
                      (10, 13), (8, 14), (14, 15), (14, 16), (16, 17), (16, 18), (18, 19), (18, 20), (18, 21)])
ALA_PHI, ALA_PSI = (4, 6, 8, 14), (6, 8, 14, 16)

# Capped glycine ACE-GLY-NME, 19 atoms: CA carries two hydrogens and no CB
#  0 H1   1 CH3  2 H2   3 H3   4 C    5 O        ACE
#  6 N    7 H    8 CA   9 HA2 10 HA3 11 C  12 O  GLY
# 13 N   14 H   15 C   16 H1  17 H2  18 H3       NME
GLY_Z = np.array([1, 6, 1, 1, 6, 8, 7, 1, 6, 1, 1, 6, 8, 7, 1, 6, 1, 1, 1])
GLY_BONDS = np.array([(0, 1), (1, 2), (1, 3), (1, 4), (4, 5), (4, 6), (6, 7), (6, 8), (8, 9), (8, 10), (8, 11), (11, 12),
                      (11, 13), (13, 14), (13, 15), (15, 16), (15, 17), (15, 18)])
GLY_PHI, GLY_PSI = (4, 6, 8, 11), (6, 8, 11, 13)


def embed(bonds, n, seed, length=1.4):
    """Coordinates ``[n,3]`` float64 for a tree-like bond graph without any chemistry: atom 0 at the origin, every other
    atom ``length`` away from its first lower-numbered neighbour in a seeded random direction, pushed to keep 1 A from
    the atoms placed before it.  Good enough for internal coordinates that are spread over their ranges."""
    rng = np.random.default_rng(seed)
    parent = {}
    for i, j in sorted((min(a, b), max(a, b)) for a, b in np.asarray(bonds).tolist()):
        parent.setdefault(j, i)
    x = np.zeros((n, 3))
    for j in range(1, n):
        for _ in range(200):
            d = rng.standard_normal(3)
            cand = x[parent[j]] + length * d / np.linalg.norm(d)
            if j == 1 or np.min(np.linalg.norm(x[:j] - cand, axis=1)) >= 1.0:
                break
        x[j] = cand
    return x


def branched_chain(n=70, seed=3):
    """A seeded branched chain of ``n`` carbons and hydrogens: atom j bonds to a random earlier atom of degree < 4.
    Returns ``(z [n], bonds [n-1,2])``."""
    rng = np.random.default_rng(seed)
    deg, bonds = np.zeros(n, int), []
    for j in range(1, n):
        lo = max(0, j - 6)                                   # mostly a chain, with short branches
        cand = [i for i in range(lo, j) if deg[i] < 4] or [i for i in range(j) if deg[i] < 4]
        i = int(rng.choice(cand))
        bonds.append((i, j))
        deg[i] += 1
        deg[j] += 1
    z = np.where(deg == 1, 1, 6)
    return z, np.array(bonds)


def draw_structures(x0, S, sigma, seed, feat, kind, configs):
    """``S`` structures ``x0 + sigma * N(0, 1)`` as float32, each kept only if ``well_conditioned`` says so in the fp64
    restatement.  Returns ``(xyz [S,n,3] float32, redrawn)``."""
    rng = np.random.default_rng(seed)
    out, redrawn = [], 0
    while len(out) < S:
        x = (x0 + sigma * rng.standard_normal(x0.shape)).astype(np.float32)
        if well_conditioned(x, feat, kind, configs):
            out.append(x)
        else:
            redrawn += 1
    return np.stack(out), redrawn
