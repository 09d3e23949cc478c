"""Numpy restatement of K24 (csrc/cluster.hip): the neighbour graph from a dense matrix of squared RMSDs, on booleans, and
the GROMOS loop as a plain recount of every row in every iteration -- deliberately not the kernel's decrement scheme: the
two agree only if both are right."""
import numpy as np

import superpose_restatement as SR


def pack(dense, c2):
    """``adj [S,S]`` bool from ``dense [S,S]`` fp64: for ``p < q`` ``adj[p,q] = adj[q,p] = dense[p,q] <= c2`` (the upper
    triangle decides), ``adj[p,p] = dense[p,p]`` is not NaN; NaN compares false."""
    D = np.asarray(dense, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        upper = np.triu(D <= float(c2), 1)
    adj = upper | upper.T
    adj[np.diag_indices_from(adj)] = ~np.isnan(np.diag(D))
    return adj


def words(adj):
    """``[S, W]`` uint64 words of a boolean matrix, columns >= S zero: what the kernel's bit matrix must equal."""
    adj = np.asarray(adj, dtype=bool)
    S = adj.shape[0]
    W = (S + 63) // 64
    wide = np.zeros((S, 64 * W), dtype=np.uint8)
    wide[:, :S] = adj
    return np.packbits(wide.reshape(S, W, 64), axis=2, bitorder="little").view("<u8").reshape(S, W)


def gromos(adj, good=None):
    """``(label [S], centres [C], sizes [C])``: while a good structure is alive, the one with most alive neighbours (its
    own diagonal bit counts as a neighbour), lowest index on ties, becomes a centre; it (whatever its diagonal bit says)
    and its alive neighbours get the next label and leave."""
    adj = np.asarray(adj, dtype=bool)
    S = adj.shape[0]
    alive = np.diag(adj).copy() if good is None else np.asarray(good, dtype=bool).copy()
    label = np.full(S, -1, dtype=np.int32)
    centres, sizes = [], []
    for _ in range(S):
        if not alive.any():
            break
        count = np.where(alive, (adj & alive[None, :]).sum(axis=1), -1)      # recounted from nothing
        c = int(np.argmax(count))                                            # the first of equal maxima
        members = adj[c] & alive
        members[c] = True
        label[members] = len(centres)
        centres.append(c)
        sizes.append(int(members.sum()))
        alive &= ~members
    return label, np.array(centres, dtype=np.int32), np.array(sizes, dtype=np.int32)


def assign(dense, c2):
    """``(state [S], rmsd [S])`` from ``dense [S,C]`` squared RMSDs to the centres: the nearest centre by
    ``superpose_restatement.min_rule``, ``-1`` where the minimum is not ``<= c2``."""
    val, idx = SR.min_rule(dense, 1)
    return np.where(val <= float(c2), idx, -1).astype(np.int64), np.sqrt(val)
