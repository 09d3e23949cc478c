"""Contacts of an ensemble restated in numpy: the squared distance in float32 with the operation order of
``csrc/sq_dist.h: sq_dist2`` -- ``(dx*dx + dy*dy) + dz*dz``, every operation an array operation of its own, hence
individually rounded -- tested with strict ``<`` against ``float32(cutoff) * float32(cutoff)``; Rg in float64.  The
``*_loops`` functions say the same in plain Python loops over scalars and are what ``test_contacts_cpu.py`` checks the
array forms against."""
import numpy as np


def cutoff2(cutoff):
    c = np.float32(cutoff)
    return np.float32(c * c)


def sq_dist2(a, b):
    """float32 arrays [..., 3] -> (dx*dx + dy*dy) + dz*dz in float32."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def bad_structures(xyz, sel):
    return ~np.isfinite(np.asarray(xyz, dtype=np.float32)[:, sel]).all(axis=(1, 2))


def contact_tensor(xyz, sel, cutoff, excluded=None):
    """[S, m, m] bool: pair (i, j) of the selection is in contact in structure s.  The diagonal, excluded pairs and bad
    structures are False."""
    x = np.asarray(xyz, dtype=np.float32)[:, np.asarray(sel)]
    m = x.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        hit = sq_dist2(x[:, :, None, :], x[:, None, :, :]) < cutoff2(cutoff)
    block = np.eye(m, dtype=bool) if excluded is None else (np.asarray(excluded, dtype=bool) | np.eye(m, dtype=bool))
    hit &= ~block[None]
    hit[bad_structures(xyz, sel)] = False
    return hit


def rg2(xyz, sel):
    """[S] float64: mean squared distance of the selected atoms from their centroid; NaN for a bad structure."""
    x = np.asarray(xyz, dtype=np.float32)[:, np.asarray(sel)].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - x.mean(axis=1, keepdims=True)
        out = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).mean(axis=1)
    out[bad_structures(xyz, sel)] = np.nan
    return out


def _finish(hit, bad, native, rg):
    """From [S, P, P] bool to what ``contacts.contact_counts`` returns."""
    upper = np.triu(np.ones(hit.shape[1:], dtype=bool), 1)
    n_contacts = (hit & upper[None]).sum(axis=(1, 2)).astype(np.int64)
    nat = np.zeros_like(upper) if native is None else np.asarray(native, dtype=bool)
    n_native = (hit & (upper & nat)[None]).sum(axis=(1, 2)).astype(np.int64)
    n_contacts[bad], n_native[bad] = -1, -1
    return {"counts": hit.sum(axis=0).astype(np.int64), "n_good": int((~bad).sum()), "n_contacts": n_contacts,
            "n_native": n_native, "rg2": rg, "bad": bad}


def contact_counts(xyz, sel, cutoff, excluded=None, native=None):
    return _finish(contact_tensor(xyz, sel, cutoff, excluded), bad_structures(xyz, sel), native, rg2(xyz, sel))


def group_contact_counts(xyz, sel, groups, cutoff, excluded=None, native=None):
    """Groups (labels per selected atom; numbered in ascending label order) A != B are in contact in structure s iff ANY
    non-excluded pair of their atoms is."""
    hit = contact_tensor(xyz, sel, cutoff, excluded)
    ids, dense = np.unique(np.asarray(groups), return_inverse=True)
    G = ids.shape[0]
    member = dense[None, :] == np.arange(G)[:, None]                       # [G, m]
    ghit = np.zeros((hit.shape[0], G, G), dtype=bool)
    for a in range(G):
        for b in range(G):
            if a != b:
                ghit[:, a, b] = hit[:, member[a]][:, :, member[b]].any(axis=(1, 2))
    out = _finish(ghit, bad_structures(xyz, sel), native, rg2(xyz, sel))
    out["group_ids"] = ids
    return out


# ----------------------------------------------------------------------------- the same in loops over scalars
def contact_counts_loops(xyz, sel, cutoff, excluded=None, native=None):
    xyz = np.asarray(xyz, dtype=np.float32)
    S, m, f = xyz.shape[0], len(sel), np.float32
    c2 = f(f(cutoff) * f(cutoff))
    counts = np.zeros((m, m), dtype=np.int64)
    n_contacts, n_native = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    rg, bad = np.zeros(S, dtype=np.float64), np.zeros(S, dtype=bool)
    for s in range(S):
        pts = [xyz[s, a] for a in sel]
        if not all(np.isfinite(v) for p in pts for v in p):
            bad[s], n_contacts[s], n_native[s], rg[s] = True, -1, -1, np.nan
            continue
        cen = [sum(float(p[d]) for p in pts) / m for d in range(3)]
        rg[s] = sum(((float(p[0]) - cen[0]) ** 2 + (float(p[1]) - cen[1]) ** 2) + (float(p[2]) - cen[2]) ** 2 for p in pts) / m
        for i in range(m):
            for j in range(i + 1, m):
                if excluded is not None and excluded[i][j]:
                    continue
                dx, dy, dz = f(pts[i][0] - pts[j][0]), f(pts[i][1] - pts[j][1]), f(pts[i][2] - pts[j][2])
                if f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz)) < c2:
                    counts[i, j] += 1
                    counts[j, i] += 1
                    n_contacts[s] += 1
                    n_native[s] += 1 if native is not None and native[i][j] else 0
    return {"counts": counts, "n_good": int((~bad).sum()), "n_contacts": n_contacts, "n_native": n_native, "rg2": rg, "bad": bad}
