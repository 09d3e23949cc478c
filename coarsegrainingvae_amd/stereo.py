"""Whether a generated structure is the SAME MOLECULE as the data's, and a possible one: the hand of every stereocentre, the
cis / trans state of every bond that does not rotate (the peptide omega), and bonds threaded through rings -- the three
failures that backmapping tools check first because no energy minimisation repairs them -- counted on the device for every
structure of an ensemble (K31, ``cgv_stereo_counts``; ``csrc/stereo.hip``).

Every other analysis of a single structure here (``contacts``, ``lddt``, ``pairdist``, ``distmat``, ...) reads distances,
which a mirror image keeps: a structure with one inverted CA passes them all.  The decoder builds atoms from cross products,
so the hand is exactly what it can get wrong.

Definition.  From fp32 coordinates, every operation rounded on its own (no fused multiply-add, no square root, no division),
with ``x`` the cross product (products first, then the difference) and ``d`` the dot product ``(xx + yy) + zz``:

    centre (c, a, b, d)      V = d(a - c, x(b - c, d - c))                    negative: V < 0       flat: V == 0
    torsion (i, j, k, l)     X = d(x(j - i, k - j), x(k - j, l - k))          cis: X > 0, that is |omega| < 90 degrees
    ring v_0 .. v_{k-1} against a bond (p0, p1) none of whose atoms is in the ring:
        g = (((v_0 + v_1) + v_2) + ...) * fp32(1 / k); the ring is the fan of the k triangles (g, v_t, v_{t+1}); the bond
        pierces it when the segment crosses at least one of them (Moeller-Trumbore without the division, boundaries
        inclusive; the comparisons are written once, at the top of ``csrc/stereo.hip``)

A ``numpy.float32`` restatement reproduces every outcome, only integers leave the device, and two calls give the same bits
however the structures are cut into launches.  A structure with a non-finite coordinate among the atoms that the tables name
is *bad* and enters nothing.

    python -m coarsegrainingvae_amd.stereo -gen samples.npz -ref traj.npz [-top top.npz] [-stereo_atoms all|heavy]
        [-stereo_min_share 0.99] [-stereo_groups none|bead|residue] [-flags flags.npz] [-out stereo_stats.json]

``z`` and ``bonds`` (``mapping`` for ``-stereo_groups bead``) come from ``-top``, else from ``-ref``.  The expected hand of
every centre and state of every torsion are the reference frames' majority (``expected``).  The full statistics of
``compare`` go to ``-out``, ``counts [S, 3]`` and ``bad [S]`` of the generated structures to ``-flags``, one JSON line with
``"stereo_stats": summary_of(...)`` to stdout.
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .ensemble import adjacency, device_of, groups_of, pack_mask, peptide_residues, read_back, structures

MAX_RING = 8                           # atoms of a ring at the most: the width of the ring table (cgv_stereo_max_ring())
MIN_SHARE = 0.99                       # of the good reference frames a centre must be of one sign in
TOP = 5                                # the centres, torsions and (ring, bond) pairs named as the worst
KINDS = ("centres", "torsions", "rings")   # the columns of ``counts``


def limits() -> Dict[str, int]:
    return ensemble.limits("stereo", ("structures", "atoms", "centres", "torsions", "rings", "bonds", "ring"))


# ----------------------------------------------------------------------------- host: the tables from the bond graph
def colours(z, nbrs, live=None) -> np.ndarray:
    """Colour refinement (Weisfeiler-Lehman) to a fixed point: an atom's colour is its element, refined by the sorted
    colours of its neighbours until the number of classes stops growing.  ``[n]`` int64; atoms outside ``live`` get -1."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    n = z.shape[0]
    live = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    col = np.where(live, z, -1)
    classes = np.unique(col[live]).shape[0]
    while True:
        keys = [(int(col[a]), tuple(sorted(int(col[b]) for b in nbrs[a]))) if live[a] else None for a in range(n)]
        rank = {k: i for i, k in enumerate(sorted({k for k in keys if k is not None}))}
        col = np.array([rank[k] if k is not None else -1 for k in keys], dtype=np.int64)
        if len(rank) == classes:
            return col
        classes = len(rank)


def omega_torsions(z, nbrs) -> List[tuple]:
    """The peptide omega ``(CA, C, N, CA')`` of every amide bond, from element and connectivity by the rule of
    ``distributions.peptide_backbone_torsions`` (``ensemble.peptide_residues``): ``C`` an amide carbon, ``N`` a nitrogen on
    it, ``CA`` the residue's alpha carbon on ``C`` -- for a cap, the lowest carbon on ``C`` -- and ``CA'`` the alpha carbon
    on ``N``, for a cap the lowest carbon on ``N`` that is no amide carbon.  An amide nitrogen without a carbon of its own
    (a side-chain NH2) has no omega."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    is_amide, residues = peptide_residues(z, nbrs)
    ca_of_n, ca_of_c = {}, {}
    for N, CA, C in residues:
        ca_of_n.setdefault(N, CA)
        ca_of_c.setdefault(C, CA)
    out = []
    for C in range(z.shape[0]):
        if not is_amide[C]:
            continue
        for N in nbrs[C]:
            if z[N] != 7:
                continue
            before = [ca_of_c[C]] if C in ca_of_c and ca_of_c[C] != N else [a for a in nbrs[C] if z[a] == 6]
            own = ca_of_n.get(N)
            after = [own] if own is not None and own != C else [a for a in nbrs[N] if z[a] == 6 and a != C and not is_amide[a]]
            if before and after:
                out.append((int(before[0]), int(C), int(N), int(after[0])))
    return out


def small_rings(n: int, nbrs, max_ring: int = MAX_RING) -> List[List[int]]:
    """Every ring of at most ``max_ring`` atoms that is the shortest cycle through one of its bonds: a breadth-first search
    per bond with the bond taken out, deduplicated by atom set; vertices along the cycle, starting at the lowest atom and
    going towards its lower neighbour in the ring."""
    found = {}
    for i in range(n):
        for j in nbrs[i]:
            if j < i:
                continue
            parent, frontier, depth = {i: -1}, [i], 0
            while frontier and j not in parent and depth < max_ring - 1:
                nxt = []
                for a in frontier:
                    for b in nbrs[a]:
                        if b in parent or (a == i and b == j):
                            continue
                        parent[b] = a
                        nxt.append(b)
                frontier, depth = nxt, depth + 1
            if j not in parent:
                continue
            path, a = [], j
            while a != -1:
                path.append(a)
                a = parent[a]
            if len(path) < 3:
                continue
            k = path.index(min(path))
            path = path[k:] + path[:k]
            if path[-1] < path[1]:
                path = [path[0]] + path[1:][::-1]
            found.setdefault(tuple(sorted(path)), path)
    return [found[key] for key in sorted(found, key=lambda s: (found[s][0], found[s]))]


def tables(z, bonds, *, atoms: str = "all", torsions=None) -> dict:
    """The four tables of a molecule from its bond graph alone (``z [n]`` elements, ``bonds [nb, 2]``).  ``atoms="heavy"``
    takes the graph without its hydrogens (a heavy-atom topology).  Atom indices throughout:

      centres [C, 4] int32     (c, a, b, d): an atom of degree 4 whose four neighbours have pairwise different colours
                               (``colours``), with its three lowest-indexed neighbours.  A CH2 or CH3 is none.
      candidate [C] bool       ``atoms="heavy"`` only: a carbon or nitrogen of degree 3 with three different neighbour colours.
                               It is a stereocentre when its fourth neighbour is a hydrogen and planar when it has none;
                               ``expected`` tells them apart from the reference frames, no hybridisation is perceived
      torsions [Q, 4] int32    the peptide omegas (``omega_torsions``), then the caller's quadruples ``torsions``; n_omega
      rings [R, 8] int32       ``small_rings``, padded with -1
      bonds [B, 2] int32       every bond of the graph once, ``i < j``, sorted
      tested [R, B] bool       the pairs that are looked at: neither atom of the bond is in the ring
    """
    z = np.asarray(z).astype(np.int64).reshape(-1)
    n = z.shape[0]
    if atoms not in ("all", "heavy"):
        raise ValueError("atoms must be 'all' or 'heavy'")
    live = np.ones(n, dtype=bool) if atoms == "all" else z != 1
    nbrs = [[b for b in nb if live[b]] if live[a] else [] for a, nb in enumerate(adjacency(n, bonds))]
    col = colours(z, nbrs, live)
    centres, candidate = [], []
    for c in range(n):
        deg = len(nbrs[c])
        full = deg == 4
        if not (full or (atoms == "heavy" and deg == 3 and z[c] in (6, 7))):
            continue
        if len({int(col[b]) for b in nbrs[c]}) != deg:
            continue
        centres.append([c] + nbrs[c][:3])
        candidate.append(not full)
    tors = omega_torsions(z, nbrs)
    n_omega = len(tors)
    if torsions is not None:
        extra = np.asarray(torsions, dtype=np.int64).reshape(-1, 4)
        if extra.shape[0] and (extra.min() < 0 or extra.max() >= n):
            raise ValueError(f"torsions name atom {int(extra.max() if extra.max() >= n else extra.min())}, z has {n} atoms")
        tors += [tuple(int(v) for v in row) for row in extra]
    rings = small_rings(n, nbrs)
    ring_tab = np.full((len(rings), MAX_RING), -1, dtype=np.int32)
    for r, ring in enumerate(rings):
        ring_tab[r, :len(ring)] = ring
    pairs = np.array(sorted({(a, b) for a in range(n) for b in nbrs[a] if a < b}), dtype=np.int32).reshape(-1, 2)
    tested = np.ones((len(rings), pairs.shape[0]), dtype=bool)
    for r, ring in enumerate(rings):
        tested[r] = ~(np.isin(pairs[:, 0], ring) | np.isin(pairs[:, 1], ring))
    return {"centres": np.asarray(centres, dtype=np.int32).reshape(-1, 4), "candidate": np.asarray(candidate, dtype=bool),
            "torsions": np.asarray(tors, dtype=np.int32).reshape(-1, 4), "n_omega": n_omega, "rings": ring_tab, "bonds": pairs,
            "tested": tested, "n_atoms": n, "atoms": atoms}


def sizes(tab: dict):
    """``(C, Q, R, B)`` of a set of tables."""
    return tuple(int(np.asarray(tab[k]).shape[0]) for k in ("centres", "torsions", "rings", "bonds"))


def ring_sizes(rings) -> np.ndarray:
    r = np.asarray(rings).reshape(-1, MAX_RING)
    return (np.cumprod(r >= 0, axis=1)).sum(1).astype(np.int64)


def checked(tab: dict, n: int) -> dict:
    """The tables as the launch takes them (int32, contiguous), or ``ValueError``: a wrong shape, an atom outside ``[0, n)``,
    a ring of fewer than 3 atoms or with an entry after its first -1, a ``tested`` that is no bool ``[R, B]``."""
    out = {}
    for key, width in (("centres", 4), ("torsions", 4), ("rings", MAX_RING), ("bonds", 2)):
        a = np.asarray(tab[key])
        if a.ndim != 2 or a.shape[1] != width or a.dtype.kind not in "iu":
            raise ValueError(f"{key} must be an int array [., {width}], got {a.dtype} {a.shape}")
        a = a.astype(np.int64)
        named = a[a >= 0] if key == "rings" else a
        if named.size and (named.min() < 0 or named.max() >= n):
            raise ValueError(f"{key} name atom {int(named.max() if named.max() >= n else named.min())}, a structure has {n} atoms")
        out[key] = np.ascontiguousarray(a.astype(np.int32))
    k = ring_sizes(out["rings"])
    if ((out["rings"] >= 0).sum(1) != k).any() or (out["rings"] < -1).any():
        raise ValueError("a ring's atoms come first in its row, then -1")
    if (k < 3).any():
        raise ValueError("a ring has at least 3 atoms")
    C, Q, R, B = sizes(out)
    t = np.asarray(tab["tested"])
    if t.dtype != np.bool_ or t.shape != (R, B):
        raise ValueError(f"tested must be a bool array [{R}, {B}], got {t.dtype} {t.shape}")
    out["tested"], out["n_atoms"] = t, n
    return out


def _want(want, C: int, Q: int):
    """``(want_sign [C] int32 of -1 / +1 or None, want_cis [Q] int32 of 0 / 1 or None)`` from a caller's dict, checked."""
    if want is None:
        return None, None
    ws, wc = want.get("want_sign"), want.get("want_cis")
    if ws is not None:
        ws = np.asarray(ws).astype(np.int64).reshape(-1)
        if ws.shape[0] != C or not np.isin(ws, (-1, 1)).all():
            raise ValueError(f"want_sign must hold -1 or +1 for each of the {C} centres")
        ws = np.ascontiguousarray(ws.astype(np.int32))
    if wc is not None:
        wc = np.asarray(wc).astype(np.int64).reshape(-1)
        if wc.shape[0] != Q or not np.isin(wc, (0, 1)).all():
            raise ValueError(f"want_cis must hold 0 or 1 for each of the {Q} torsions")
        wc = np.ascontiguousarray(wc.astype(np.int32))
    return ws, wc


def _same_opt(a, b) -> bool:
    return (a is None) == (b is None) and (a is None or np.array_equal(a, b))


# ----------------------------------------------------------------------------- the launches
def counts(xyz, tab: dict, want: Optional[dict] = None, *, into: Optional[dict] = None, chunk: int = 4096, device="cuda") -> dict:
    """The three predicates over the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device tensor
    decides the device) for the tables ``tab`` (``tables``; atom indices) against ``want`` (``{"want_sign": [C] of -1 / +1,
    "want_cis": [Q] of 0 / 1}``, either may be missing or None; ``expected`` makes it).  Host arrays:

      neg, flat [C] int64        the good structures in which the centre is negative, flat
      cis [Q] int64              ... in which the torsion is cis
      pierced [R, B] int64       ... in which the bond goes through the ring
      counts [S, 3] int32        per structure: centres whose sign differs from want_sign (a flat one is wrong), torsions
                                 whose state differs from want_cis, pierced pairs; a counter without its ``want`` stays 0
      bad [S] bool, n_good       structures with a non-finite coordinate among the named atoms, and the number of the others
      tables, want_sign, want_cis     what was used

    The structures go through in launches of ``chunk`` (``ensemble.chunks``); the sums stay on the device; ONE read-back.
    ``into``: an earlier result with the same tables and ``want``; its sums are added and its ``counts`` / ``bad`` come
    first, so a long ensemble may be fed in pieces -- to the same integers as in one call.  Any of the tables may be empty.
    Everything that can be refused is a ``ValueError`` before any launch."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    t = checked(tab, n)
    C, Q, R, B = sizes(t)
    ws, wc = _want(want, C, Q)
    lim = limits()
    if not 1 <= int(chunk) <= lim["structures"]:
        raise ValueError(f"chunk must be in 1..{lim['structures']}, got {chunk}")
    for key, have in zip(("centres", "torsions", "rings", "bonds"), (C, Q, R, B)):
        if have > lim[key]:
            raise ValueError(f"the tables list {have} {key} (the kernel holds {lim[key]})")
    named = np.concatenate([t["centres"].reshape(-1), t["torsions"].reshape(-1), t["rings"][t["rings"] >= 0], t["bonds"].reshape(-1)])
    sel = np.unique(named).astype(np.int32)
    P = int(sel.shape[0])
    if P > lim["atoms"]:
        raise ValueError(f"the tables name {P} atoms (the kernel holds {lim['atoms']})")
    if into is not None:
        old = into["tables"]
        same = all(np.array_equal(old[k], t[k]) for k in ("centres", "torsions", "rings", "bonds", "tested")) and \
            _same_opt(into["want_sign"], ws) and _same_opt(into["want_cis"], wc)
        if not same:
            raise ValueError("into was counted with other tables or another want")
    place = lambda a: np.ascontiguousarray(np.where(a >= 0, np.searchsorted(sel, np.maximum(a, 0)), -1).astype(np.int32))
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(chunk, lim["structures"], 16 * max(P + R, 1))
    z64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=dev)
    out = {"neg": z64(C), "flat": z64(C), "cis": z64(Q), "pierced": torch.zeros(R, B, dtype=torch.int32, device=dev),
           "counts": torch.zeros(S, 3, dtype=torch.int32, device=dev), "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if S:
        lib = _lib.load()
        up = lambda a: None if a is None or a.size == 0 else torch.from_numpy(a).to(dev)
        d_sel, d_c, d_q, d_r, d_b = (up(a) for a in (sel, place(t["centres"]), place(t["torsions"]), place(t["rings"]), place(t["bonds"])))
        d_t = up(pack_mask(t["tested"]).view(np.int32)) if R and B else None
        d_ws, d_wc = up(ws), up(wc)
        need = int(lib.cgv_stereo_workspace_bytes(min(M, S), P, R))
        work = torch.empty(max((need + 15) // 16 * 4, 4), dtype=torch.float32, device=dev)
        for start, part in ensemble.chunks(x, M, dev):
            k = int(part.shape[0])
            _lib.call("cgv_stereo_counts", _lib.ptr(part), _lib.ptr(d_sel), _lib.ptr(d_c), _lib.ptr(d_q), _lib.ptr(d_r), _lib.ptr(d_b),
                      _lib.ptr(d_t), _lib.ptr(d_ws), _lib.ptr(d_wc), k, n, P, C, Q, R, B, _lib.ptr(out["neg"]), _lib.ptr(out["flat"]),
                      _lib.ptr(out["cis"]), _lib.ptr(out["pierced"]), _lib.ptr(out["counts"][start:start + k]),
                      _lib.ptr(out["bad"][start:start + k]), _lib.ptr(work), work.numel() * 4, _lib.stream_ptr(), tag="stereo")
    neg, flat, cis, pierced, cnt, bad = read_back([out[k] for k in ("neg", "flat", "cis", "pierced", "counts", "bad")])
    pierced, bad = pierced.astype(np.int64), bad.astype(bool)
    n_good = int(S - int(bad.sum()))
    if into is not None:
        neg, flat, cis, pierced = (a + np.asarray(into[k], dtype=np.int64) for a, k in ((neg, "neg"), (flat, "flat"), (cis, "cis"), (pierced, "pierced")))
        cnt = np.concatenate([np.asarray(into["counts"], dtype=np.int32).reshape(-1, 3), cnt])
        bad = np.concatenate([np.asarray(into["bad"], dtype=bool), bad])
        n_good += int(into["n_good"])
    return {"neg": neg, "flat": flat, "cis": cis, "pierced": pierced, "counts": cnt, "bad": bad, "n_good": n_good, "tables": t,
            "want_sign": ws, "want_cis": wc}


# ----------------------------------------------------------------------------- what the reference says is right
def expected_from_counts(rec: dict, tab: dict, min_share: float = MIN_SHARE) -> dict:
    """From the counts ``rec`` of the reference frames over ``tab`` (no ``want`` needed): the tables without the centres and
    candidates that are not of ONE sign in at least ``min_share`` of the good frames -- which removes the planar sp2 atoms
    of a heavy-atom topology, whose triple product is noise about 0, and any centre the data itself inverts -- and what is
    right for the rest.  Pure host.  ``{"tables", "want_sign" [C'] (the majority sign), "want_cis" [Q] (the majority
    state), "kept" [C] bool, "share" [C] (of the majority sign), "n_good"}``."""
    if not 0.5 < float(min_share) <= 1.0:
        raise ValueError("min_share must be in (0.5, 1]")
    n = int(rec["n_good"])
    if n < 1:
        raise ValueError("no good reference frame: nothing says what is right")
    neg, flat = np.asarray(rec["neg"], dtype=np.int64), np.asarray(rec["flat"], dtype=np.int64)
    pos = n - neg - flat
    share = np.maximum(neg, pos) / n
    kept = share >= float(min_share)
    out = dict(tab)
    out["centres"] = np.asarray(tab["centres"])[kept]
    out["candidate"] = np.asarray(tab.get("candidate", np.zeros(kept.shape[0], dtype=bool)))[kept]
    return {"tables": out, "want_sign": np.where(neg > pos, -1, 1)[kept].astype(np.int32),
            "want_cis": (2 * np.asarray(rec["cis"], dtype=np.int64) > n).astype(np.int32), "kept": kept, "share": share, "n_good": n}


def expected(ref_xyz, tab: dict, *, min_share: float = MIN_SHARE, chunk: int = 4096, device="cuda") -> dict:
    """ONE pass of the kernel over the reference frames, then ``expected_from_counts``."""
    if not 0.5 < float(min_share) <= 1.0:
        raise ValueError("min_share must be in (0.5, 1]")
    return expected_from_counts(counts(ref_xyz, tab, chunk=chunk, device=device), tab, min_share)


# ----------------------------------------------------------------------------- host statistics
def rates(rec: dict) -> dict:
    """Of one result of ``counts``, fp64 over its good structures: ``centres [C]`` the share in which the centre is wrong
    (against want_sign; flat is wrong), ``torsions [Q]`` in which the torsion is flipped (against want_cis), ``cis [Q]``,
    ``pierced [R, B]``; NaN without a good structure."""
    n = int(rec["n_good"])
    neg, flat, cis = (np.asarray(rec[k], dtype=np.float64) for k in ("neg", "flat", "cis"))
    ws, wc = rec["want_sign"], rec["want_cis"]
    wrong_c = np.zeros_like(neg) if ws is None else np.where(np.asarray(ws) > 0, neg + flat, n - neg)
    wrong_q = np.zeros_like(cis) if wc is None else np.where(np.asarray(wc) != 0, n - cis, cis)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"centres": wrong_c / n, "torsions": wrong_q / n, "cis": cis / n, "pierced": np.asarray(rec["pierced"], dtype=np.float64) / n}


def _valid(rec: dict) -> dict:
    """The share of good structures without an error of each kind, and without any."""
    good = ~np.asarray(rec["bad"], dtype=bool)
    c = np.asarray(rec["counts"]).reshape(-1, 3)[good]
    if c.shape[0] == 0:
        return {**{k: None for k in KINDS}, "all": None}
    return {**{k: float((c[:, i] == 0).mean()) for i, k in enumerate(KINDS)}, "all": float((c.sum(1) == 0).mean())}


def _errors(rec: dict) -> np.ndarray:
    good = ~np.asarray(rec["bad"], dtype=bool)
    return np.asarray(rec["counts"], dtype=np.int64).reshape(-1, 3)[good].sum(1)


def _sum(a: dict, b: dict) -> dict:
    """Two results over the same tables and want as one (the even and the odd reference frames)."""
    out = {k: np.asarray(a[k], dtype=np.int64) + np.asarray(b[k], dtype=np.int64) for k in ("neg", "flat", "cis", "pierced")}
    out.update(counts=np.concatenate([np.asarray(a["counts"]).reshape(-1, 3), np.asarray(b["counts"]).reshape(-1, 3)]),
               bad=np.concatenate([np.asarray(a["bad"], dtype=bool), np.asarray(b["bad"], dtype=bool)]),
               n_good=int(a["n_good"]) + int(b["n_good"]), want_sign=a["want_sign"], want_cis=a["want_cis"], tables=a["tables"])
    return out


def _top(score, make) -> list:
    order = np.argsort(-np.nan_to_num(score, nan=-1.0), kind="stable")[:TOP]
    return [make(int(k)) for k in order]


def _group_level(tab, rg, rr, labels) -> dict:
    """The three rates averaged over the items of every group: a centre belongs to its atom's group, a torsion to that of
    its second atom, a (ring, bond) pair to that of the ring's first atom."""
    labels = np.asarray(labels).reshape(-1)
    if labels.shape[0] != int(tab["n_atoms"]) or labels.dtype.kind not in "iu":
        raise ValueError(f"groups must be an int label for every atom of the molecule ({int(tab['n_atoms'])})")
    ids = np.unique(labels)
    per_ring = lambda r: np.where(tab["tested"].any(1), np.where(tab["tested"], r["pierced"], 0.0).sum(1), np.nan) if r["pierced"].size else np.zeros(0)
    items = {"centres": (labels[tab["centres"][:, 0]], rg["centres"], rr["centres"]),
             "torsions": (labels[tab["torsions"][:, 1]], rg["torsions"], rr["torsions"]),
             "rings": (labels[tab["rings"][:, 0]], per_ring(rg), per_ring(rr))}
    rows = []
    for g in ids:
        row = {"id": int(g)}
        for kind, (lab, gen, ref) in items.items():
            mine = lab == g
            row[kind] = {"n": int(mine.sum()), "gen": float(np.nanmean(gen[mine])) if mine.any() and np.isfinite(gen[mine]).any() else None,
                         "ref": float(np.nanmean(ref[mine])) if mine.any() and np.isfinite(ref[mine]).any() else None}
        row["gen"] = float(sum(row[k]["gen"] or 0.0 for k in KINDS))
        rows.append(row)
    score = np.array([r["gen"] for r in rows])
    return {"n_groups": int(ids.shape[0]), "ids": [int(v) for v in ids], "rows": rows, "worst": _top(score, lambda k: rows[k])}


def compare_from_counts(even: dict, odd: dict, gen: dict, groups=None, params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from three results of ``counts`` over the same tables and ``want`` -- the even reference
    frames, the odd ones and the generated structures.  Pure host.  ``groups [n]``: a label for every ATOM of the molecule.
    Keys: ``STEREO_STATS_KEYS``; see ``compare``."""
    tab = gen["tables"]
    if any(sizes(r["tables"]) != sizes(tab) for r in (even, odd)):
        raise ValueError("the three results have different tables")
    C, Q, R, B = sizes(tab)
    ref = _sum(even, odd)
    rg, rr = rates(gen), rates(ref)
    stats = {**ensemble.set_sizes(even, odd, gen), "params": dict(params or {}), "n_centres": C, "n_torsions": Q, "n_rings": R,
             "n_bonds": B, "n_tested": int(np.asarray(tab["tested"]).sum())}
    stats["valid"] = {"gen": _valid(gen), "ref": _valid(ref)}
    lst = lambda a: [None if not np.isfinite(v) else float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    stats["inversion_rate"] = {"gen": lst(rg["centres"]), "ref": lst(rr["centres"])}
    stats["cis_rate"] = {"gen": lst(rg["cis"]), "ref": lst(rr["cis"])}
    opt = lambda v: None if not np.isfinite(v) else float(v)
    stats["worst_centres"] = _top(rg["centres"], lambda k: {"centre": k, "atom": int(tab["centres"][k, 0]), "want": int(gen["want_sign"][k]) if gen["want_sign"] is not None else None,
                                                            "gen": opt(rg["centres"][k]), "ref": opt(rr["centres"][k])})
    stats["worst_torsions"] = _top(rg["torsions"], lambda k: {"torsion": k, "atoms": [int(v) for v in tab["torsions"][k]],
                                                              "want_cis": int(gen["want_cis"][k]) if gen["want_cis"] is not None else None,
                                                              "gen": opt(rg["torsions"][k]), "ref": opt(rr["torsions"][k])})
    flat_g, flat_r = rg["pierced"].reshape(-1), rr["pierced"].reshape(-1)
    stats["worst_pairs"] = _top(np.where(np.asarray(tab["tested"]).reshape(-1), flat_g, -1.0),
                                lambda k: {"ring": k // B, "bond": k % B, "ring_atoms": [int(v) for v in tab["rings"][k // B] if v >= 0],
                                           "bond_atoms": [int(v) for v in tab["bonds"][k % B]], "gen": opt(flat_g[k]), "ref": opt(flat_r[k])}) if R * B else []
    ee, eo, eg = _errors(even), _errors(odd), _errors(gen)
    top = int(max([int(v.max()) for v in (ee, eo, eg) if v.size] + [0]))
    stats["errors"] = ensemble.scalar_block(ee, eo, eg, -0.5, top + 0.5, top + 1)
    stats["groups"] = None
    if groups is not None:
        stats["groups"] = _group_level(tab, rg, rr, groups)
    return stats


def compare(gen_xyz, ref_xyz, z, bonds, *, atoms: str = "all", min_share: float = MIN_SHARE, groups=None, mapping=None, torsions=None,
            chunk: int = 4096, device="cuda", params: Optional[dict] = None, flags: Optional[dict] = None) -> dict:
    """Generated structures ``gen_xyz [S,n,3]`` against the reference frames ``ref_xyz [T,n,3]`` (at least two) of the
    molecule ``z``, ``bonds``: ``tables``, then ``expected`` from the reference, then the counts of the reference's even and
    odd frames and of the generated structures.  ``groups``: None, ``"bead"`` (``mapping``) or ``"residue"``.  Returns a
    dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      params, n_centres, n_torsions, n_rings, n_bonds, n_tested     the caller's ``params``; the tables' sizes after ``expected``
      valid             {gen, ref}: the share of good structures with no inverted centre (``centres``), no flipped torsion
                        (``torsions``), no pierced ring (``rings``), and none of the three (``all``)
      inversion_rate    {gen, ref}: per centre the share of good structures in which it has the wrong hand or is flat
      cis_rate          {gen, ref}: per torsion the share in which it is cis
      worst_centres, worst_torsions, worst_pairs     the five with the largest generated rate of errors, next to the reference's
      errors            ``ensemble.scalar_block`` of the errors per structure (the three counters summed): histograms, the
                        JSD to the reference's, its even / odd floor, moments
      groups            {n_groups, ids, rows, worst}: the rates averaged over every bead's or residue's items; else None

    ``flags``: a dict that receives ``counts [S, 3]`` and ``bad [S]`` of the generated structures (what ``-flags`` writes)."""
    ref, gen, z = ensemble.check_sets(ref_xyz, gen_xyz, z, groups=groups)
    tab = tables(z, bonds, atoms=atoms, torsions=torsions)
    if sum(sizes(tab)[:3]) == 0:
        raise ValueError("the topology has no stereocentre, no peptide bond and no ring: there is nothing to check")
    labels = None if groups is None else groups_of(z, bonds, mapping, groups)
    kw = dict(chunk=chunk, device=device)
    exp = expected(ref, tab, min_share=min_share, **kw)
    even, odd, got = (counts(s, exp["tables"], exp, **kw) for s in (ref[0::2], ref[1::2], gen))
    if flags is not None:
        flags.update(counts=got["counts"], bad=got["bad"])
    return compare_from_counts(even, odd, got, groups=labels, params=params)


STEREO_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "n_centres", "n_torsions", "n_rings", "n_bonds", "n_tested",
                     "valid", "inversion_rate", "cis_rate", "worst_centres", "worst_torsions", "worst_pairs", "errors", "groups")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"stereo_stats"`` in its JSON summary line: no per-item rates, no histograms, the
    single worst of each kind."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_centres", "n_torsions", "n_rings", "n_tested", "valid")}
    for k in ("worst_centres", "worst_torsions", "worst_pairs"):
        short[k] = stats[k][:1]
    short["errors"] = ensemble.short_block(stats["errors"], ensemble.MOMENTS + ("floor",))
    short["groups"] = None if stats["groups"] is None else {"n_groups": stats["groups"]["n_groups"], "worst": stats["groups"]["worst"][:1]}
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.stereo",
                                "inverted stereocentres, cis peptide bonds and pierced rings of generated structures against the reference frames",
                                top_help="npz with z and bonds (mapping for -stereo_groups bead); default: those of -ref")
    p.add_argument("-stereo_atoms", choices=("all", "heavy"), default="all", help="the bond graph: as it is, or without its hydrogens (all)")
    p.add_argument("-stereo_min_share", type=float, default=MIN_SHARE,
                   help="a centre is kept when it is of one sign in at least this share of the good reference frames (0.99)")
    p.add_argument("-stereo_groups", choices=("none", "bead", "residue"), default="none", help="also average the rates per bead or residue (none)")
    p.add_argument("-flags", default=None, help="npz that receives counts [S,3] and bad [S] of the generated structures (not written)")
    return compare_cli.finish_parser(p, "stereo_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, ``mapping``, ``tables``, with everything that
    can be refused without a device refused here (``SystemExit``), before the library is loaded."""
    if not 0.5 < args.stereo_min_share <= 1.0:
        raise SystemExit("-stereo_min_share must be in (0.5, 1]")
    need = ("z", "bonds") + (("mapping",) if args.stereo_groups == "bead" else ())
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args, need)
    with compare_cli.refusing():
        tab = tables(z, top["bonds"], atoms=args.stereo_atoms)
        if sum(sizes(tab)[:3]) == 0:
            raise ValueError("the topology has no stereocentre, no peptide bond and no ring: there is nothing to check")
        if args.stereo_groups != "none":
            groups_of(z, top["bonds"], top.get("mapping"), args.stereo_groups)
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": top["bonds"], "mapping": top.get("mapping"), "tables": tab}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    params = {"atoms": args.stereo_atoms, "min_share": float(args.stereo_min_share), "groups": args.stereo_groups}
    flags = {} if args.flags else None
    with compare_cli.refusing():
        stats = compare(inp["gen_xyz"], inp["ref_xyz"], inp["z"], inp["bonds"], atoms=args.stereo_atoms, min_share=args.stereo_min_share,
                        groups=None if args.stereo_groups == "none" else args.stereo_groups, mapping=inp["mapping"], device=args.device,
                        params=params, flags=flags)
    if args.flags:
        np.savez(args.flags, **flags)
    compare_cli.finish("stereo", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
