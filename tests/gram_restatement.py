"""Numpy restatement of what the projections of K16 and K27 share (csrc/gram_dev.h): the bin rule of the two-component map,
written from its definition and importing nothing of the package."""
import numpy as np


def bin_of(v, lo, hi, nb):
    """The rule: for ``lo <= v < hi`` the bin ``floor((v - lo) * nb / (hi - lo))`` in fp64, clamped to ``[0, nb)``; -1
    otherwise (NaN included)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (v >= lo) & (v < hi)
        b = np.floor((np.where(inside, v, lo) - lo) * float(nb) / (hi - lo)).astype(np.int64)
    return np.where(inside, np.clip(b, 0, nb - 1), -1)


def edge_distance(v, lo, hi, nb):
    """How far ``v`` is from the nearest bin edge of ``[lo, hi)`` cut into ``nb`` bins (``lo`` and ``hi`` are edges)."""
    v = np.asarray(v, dtype=np.float64)
    edges = lo + (hi - lo) * np.arange(nb + 1) / nb
    return np.abs(v[:, None] - edges[None]).min(1)


def hist2(va, vb, ra, rb, nb):
    """``(counts [nb,nb], outside)`` of the pairs ``(va, vb)``: a pair with either value off its range or NaN is outside."""
    ia, ib = bin_of(va, ra[0], ra[1], nb), bin_of(vb, rb[0], rb[1], nb)
    ok = (ia >= 0) & (ib >= 0)
    counts = np.zeros((nb, nb), dtype=np.int64)
    np.add.at(counts, (ia[ok], ib[ok]), 1)
    return counts, int((~ok).sum())
