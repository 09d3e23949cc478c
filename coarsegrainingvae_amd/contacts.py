"""Which atoms (or beads, or residues) of an ensemble touch, how compact its structures are, and whether they have the
contacts the data has: contact probability maps, the fraction of native contacts Q and the radius of gyration Rg, counted
on the device for every pair and every structure (K20, ``cgv_contact_counts`` / ``cgv_contact_group_counts``;
``csrc/contact_map.hip``).

Nothing in the reference looks at non-bonded packing, and neither do ``evaluate`` (the bond graph), ``distributions``
(bonds, angles, torsions), ``tica`` (slow collective coordinates) or ``coverage`` (whole-structure RMSD): side chains of
different beads can pack wrongly, a hairpin can have the right (phi, psi) maps and the wrong strand pairing, an ensemble
can be too swollen or too collapsed, with every one of those clean.

A pair of selected atoms ``(i, j)``, ``i != j``, that is not excluded (bonded neighbours up to ``depth`` bonds:
``excluded_pairs``) is *in contact* in a structure iff ``(dx*dx + dy*dy) + dz*dz < cutoff2`` in fp32 with every operation
rounded on its own and ``cutoff2 = fp32(cutoff) * fp32(cutoff)`` -- so a host restatement in ``numpy.float32`` reproduces
every count exactly.  Two groups are in contact in a structure iff ANY non-excluded pair of their atoms is (this cannot
be derived from the atom counts: the "any" is taken per structure).  The result is a ``[m, m]`` (or ``[G, G]``) table of
integers -- no ``[S, m, m]`` tensor exists -- and four numbers per structure.  A structure with a non-finite selected
coordinate is *bad*: it is counted nowhere, its ``n_contacts`` and ``n_native`` are ``-1`` and its ``rg2`` is NaN.

The host pieces shared with the other analyses (``selection``, ``groups_of``, ``scalar_block``, ...) live in ``ensemble``.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, ensemble
from .ensemble import adjacency, check_sets, device_of, groups_of, read_back, scalar_block, select_atoms, structures

MAX_GROUPS = 4096                      # include/cgvae_hip.h: the group kernel's grid


def limits() -> Dict[str, int]:
    return ensemble.limits("contact")


def cutoff2_of(cutoff: float) -> np.float32:
    """The squared cutoff as the kernel takes it: the fp32 product of the fp32 cutoff."""
    c = np.float32(cutoff)
    if not np.isfinite(c) or c < 0:
        raise ValueError(f"the cutoff must be a finite distance >= 0, got {cutoff}")
    return np.float32(c * c)


# ----------------------------------------------------------------------------- host: masks and groups
def excluded_pairs(bonds, n_atoms: int, sel, depth: int = 3) -> np.ndarray:
    """``[m, m]`` bool over the selection ``sel``: True for ``i == j`` and for every pair at most ``depth`` bonds apart
    in the bond graph of all ``n_atoms`` atoms (paths may run through atoms outside the selection).  ``depth=3``
    excludes 1-2, 1-3 and 1-4 pairs, ``depth=0`` nothing but the diagonal.  Breadth-first search, host."""
    if int(depth) < 0:
        raise ValueError("depth must be >= 0")
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    if sel.shape[0] and (sel.min() < 0 or sel.max() >= n_atoms):
        raise ValueError(f"the selection names atom {int(sel.max() if sel.max() >= n_atoms else sel.min())}, the molecule has {n_atoms} atoms")
    nbrs = adjacency(int(n_atoms), bonds)
    where = {}
    for k, a in enumerate(sel.tolist()):
        where.setdefault(a, []).append(k)
    out = np.eye(sel.shape[0], dtype=bool)
    for k, a in enumerate(sel.tolist()):
        seen, frontier = {a}, [a]
        for _ in range(int(depth)):
            frontier = [c for b in frontier for c in nbrs[b] if c not in seen and not seen.add(c)]
            if not frontier:
                break
        for b in seen:
            out[k, where.get(b, [])] = True
    return out


# ----------------------------------------------------------------------------- the launches
def contact_counts(xyz, sel=None, cutoff: float = 4.5, excluded=None, native=None, groups=None,
                   structures_per_launch: int = 4096, device="cuda") -> dict:
    """Contacts of the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device tensor decides
    the device) over the atoms ``sel [m]`` (any order; default: all).  ``excluded [m,m]`` bool in the order of ``sel``
    (``excluded_pairs``; default: the diagonal).  Without ``groups`` the pairs are pairs of atoms; with ``groups [m]``
    (a label per selected atom) they are pairs of groups, numbered in ascending order of their labels (``group_ids``).
    ``native``: bool ``[m,m]`` (``[G,G]`` with groups), the pairs ``n_native`` counts.  Host arrays:

      counts      [m,m] or [G,G] int64, symmetric, zero diagonal: in how many good structures the pair is in contact
      n_good      structures that are not bad (the denominator of a probability)
      n_contacts  [S] int64 pairs in contact in structure s;  n_native [S] int64 those of them in ``native``
      rg2         [S] fp64 mean squared distance of the selected atoms from their centroid
      bad         [S] bool;  bad structures have n_contacts = n_native = -1 and rg2 = NaN
      group_ids   [G] the labels (only with ``groups``)

    The structures go through in launches of ``structures_per_launch``; the table is summed on the device in int64;
    ONE read-back.  Limits (``limits()``, total structures < 2^31, at most 4096 groups) are refused before any launch."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    lim = limits()
    if S >= 2 ** 31:
        raise ValueError("the counts are int32: fewer than 2^31 structures")
    c2 = cutoff2_of(cutoff)
    table = ensemble.selection(sel, n, purpose="count contacts of")
    m = int(table.shape[0])
    if m > lim["atoms"]:
        raise ValueError(f"the selection lists {m} atoms (the kernel holds {lim['atoms']})")
    excl = np.eye(m, dtype=bool) if excluded is None else (ensemble.square_mask(excluded, m, "excluded") | np.eye(m, dtype=bool))
    order, gstart, ids = None, None, None
    if groups is not None:
        g = np.asarray(groups, dtype=np.int64).reshape(-1)
        if g.shape[0] != m:
            raise ValueError(f"groups lists {g.shape[0]} atoms, the selection {m}")
        ids, dense = np.unique(g, return_inverse=True)
        if ids.shape[0] > MAX_GROUPS:
            raise ValueError(f"{ids.shape[0]} groups (the kernel holds {MAX_GROUPS})")
        order = np.argsort(dense, kind="stable")              # the groups become contiguous
        table, excl = np.ascontiguousarray(table[order]), excl[np.ix_(order, order)]
        gstart = np.concatenate([[0], np.cumsum(np.bincount(dense, minlength=ids.shape[0]))]).astype(np.int32)
    P = m if groups is None else int(ids.shape[0])
    nat = None if native is None else ensemble.square_mask(native, P, "native")
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(structures_per_launch, lim["structures"], 16 * m)
    total = torch.zeros(P, P, dtype=torch.int64, device=dev)
    part = torch.zeros(P, P, dtype=torch.int32, device=dev)
    per = {"n_contacts": torch.zeros(S, dtype=torch.int32, device=dev), "n_native": torch.zeros(S, dtype=torch.int32, device=dev),
           "rg2": torch.zeros(S, dtype=torch.float64, device=dev), "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if S:
        lib = _lib.load()
        d_sel = torch.from_numpy(table).to(dev)
        d_excl = torch.from_numpy(ensemble.pack_mask(excl).view(np.int32)).to(dev)
        d_nat = None if nat is None else torch.from_numpy(ensemble.pack_mask(nat).view(np.int32)).to(dev)
        d_gs = None if gstart is None else torch.from_numpy(gstart).to(dev)
        need = int(lib.cgv_contact_workspace_bytes(min(M, S), m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        for start, chunk in ensemble.chunks(x, M, dev):
            k = int(chunk.shape[0])
            if start:
                part.zero_()
            out = [_lib.ptr(per[key][start:start + k]) for key in ("n_contacts", "n_native", "rg2", "bad")]
            tail = [_lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()]
            if groups is None:
                _lib.call("cgv_contact_counts", _lib.ptr(chunk), _lib.ptr(d_sel), _lib.ptr(d_excl), _lib.ptr(d_nat), k, n, m,
                          float(c2), _lib.ptr(part), *out, *tail, tag="contact_counts")
            else:
                _lib.call("cgv_contact_group_counts", _lib.ptr(chunk), _lib.ptr(d_sel), _lib.ptr(d_gs), _lib.ptr(d_excl),
                          _lib.ptr(d_nat), k, n, m, P, float(c2), _lib.ptr(part), *out, *tail, tag="contact_group_counts")
            total += part
    counts, n_contacts, n_native, rg2, bad = read_back([total] + [per[k] for k in ("n_contacts", "n_native", "rg2", "bad")])
    res = {"counts": counts, "n_good": int(S - int(bad.sum())), "n_contacts": n_contacts.astype(np.int64),
           "n_native": n_native.astype(np.int64), "rg2": rg2, "bad": bad.astype(bool)}
    if groups is not None:
        res["group_ids"] = ids
    return res


# ----------------------------------------------------------------------------- host statistics
def _upper(allowed: np.ndarray) -> np.ndarray:
    return np.triu(np.asarray(allowed, dtype=bool), 1)


def probabilities(res: dict) -> Optional[np.ndarray]:
    """``counts / n_good`` (fp64), or ``None`` when no structure is good."""
    return None if res["n_good"] <= 0 else np.asarray(res["counts"], dtype=np.float64) / float(res["n_good"])


def native_set(even: dict, odd: dict, allowed, native_min: float = 0.5) -> np.ndarray:
    """The native pairs: allowed pairs whose contact probability in the reference (the integer sum of its even and odd
    frames) is at least ``native_min``.  Symmetric bool; all False when the reference has no good structure."""
    good = even["n_good"] + odd["n_good"]
    allowed = np.asarray(allowed, dtype=bool)
    if good <= 0:
        return np.zeros_like(allowed)
    counts = np.asarray(even["counts"], dtype=np.int64) + np.asarray(odd["counts"], dtype=np.int64)
    return (counts >= float(native_min) * good) & allowed & ~np.eye(allowed.shape[0], dtype=bool)


def _map_dev(p, q, upper):
    if p is None or q is None or not upper.any():
        return None, None
    d = (p - q)[upper]
    return float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())


def compare_from_counts(even: dict, odd: dict, gen: dict, allowed, native, labels=None, n_bins: int = 20,
                        params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from three results of ``contact_counts`` -- the even reference frames, the odd ones
    and the generated structures, all counted with the same selection, exclusions and ``native`` set -- pure host.
    ``allowed [P,P]`` bool: the pairs that count (not excluded); ``native [P,P]`` bool: the set ``n_native`` counted;
    ``labels [P]``: what a row of the maps is (an atom index, a group label), default ``0..P-1``.  Bad structures are in
    no denominator.  Keys: ``CONTACT_STATS_KEYS``; see ``compare``."""
    allowed = np.asarray(allowed, dtype=bool)
    P = allowed.shape[0]
    upper = _upper(allowed)
    labels = list(range(P)) if labels is None else [int(v) for v in labels]
    ref = {"counts": np.asarray(even["counts"], dtype=np.int64) + np.asarray(odd["counts"], dtype=np.int64),
           "n_good": even["n_good"] + odd["n_good"]}
    p_ref, p_gen, p_even, p_odd = probabilities(ref), probabilities(gen), probabilities(even), probabilities(odd)
    rmse, max_dev = _map_dev(p_ref, p_gen, upper)
    f_rmse, f_max = _map_dev(p_even, p_odd, upper)
    top = []
    if rmse is not None:
        ii, jj = np.nonzero(upper)
        dev = np.abs(p_ref - p_gen)[ii, jj]
        for k in np.argsort(-dev, kind="stable")[:10]:
            i, j = int(ii[k]), int(jj[k])
            top.append({"i": labels[i], "j": labels[j], "p_ref": float(p_ref[i, j]), "p_gen": float(p_gen[i, j])})
    n_native = int(_upper(np.asarray(native, dtype=bool) & allowed).sum())

    def good(res, key):
        return np.asarray(res[key])[~np.asarray(res["bad"], dtype=bool)]
    rg = [np.sqrt(good(r, "rg2").astype(np.float64)) for r in (even, odd, gen)]
    rg_ref = np.concatenate(rg[:2])
    rg_block = q_block = None
    if rg_ref.size and rg[2].size:
        lo, hi = float(rg_ref.min()), float(rg_ref.max())
        pad = 0.1 * (hi - lo) if hi > lo else 0.05 * max(abs(hi), 1.0)       # the reference's range, 20 % wider
        rg_block = scalar_block(rg[0], rg[1], rg[2], lo - pad, hi + pad, n_bins)
        if n_native > 0:
            q = [good(r, "n_native").astype(np.float64) / n_native for r in (even, odd, gen)]
            q_block = scalar_block(q[0], q[1], q[2], 0.0, 1.0, n_bins)
    return {**ensemble.set_sizes(even, odd, gen), "params": dict(params or {}, n_bins=int(n_bins)), "labels": labels,
            "p_ref": None if p_ref is None else p_ref.tolist(), "p_gen": None if p_gen is None else p_gen.tolist(),
            "map_rmse": rmse, "map_max_dev": max_dev,
            "floor": {"map_rmse": f_rmse, "map_max_dev": f_max, "q_jsd": q_block["floor"] if q_block else None,
                      "rg_jsd": rg_block["floor"] if rg_block else None},
            "top_pairs": top, "n_native": n_native, "q": q_block, "rg": rg_block}


def compare(ref_xyz, gen_xyz, z, bonds, atoms="heavy", cutoff: float = 4.5, exclude: int = 3, groups=None,
            native_min: float = 0.5, n_bins: int = 20, mapping=None, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) of the
    molecule ``z [n]`` / ``bonds [Eb,2]`` by their contacts over ``select_atoms(z, atoms)``: atoms closer than ``cutoff``
    Angstrom that are more than ``exclude`` bonds apart.  ``groups``: ``None`` (pairs of atoms), ``"bead"`` (needs
    ``mapping``) or ``"residue"`` (``groups_of``).  The convention of ``distributions.compare``: the generated
    structures, the even and the odd frames of the reference are counted apart, the reference is the integer sum of its
    halves, and what the halves differ by is the ``floor`` every deviation is to be read against.  The native set --
    pairs (of groups, when there are groups) whose reference probability is at least ``native_min`` -- needs the
    reference's table first, so the reference is counted once for its table and the three sets once with the native set.
    Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      params      atoms (the selection), cutoff, exclude, groups, native_min, n_bins
      labels      [P] the atom index or group label of a row of the maps
      p_ref, p_gen  [P][P] contact probabilities (``None``: no good structure in the set)
      map_rmse, map_max_dev   root mean square and largest |p_ref - p_gen| over the pairs that count
      floor       {map_rmse, map_max_dev, q_jsd, rg_jsd}: the same between the even and the odd reference frames
      top_pairs   the ten pairs of largest deviation: {i, j (labels), p_ref, p_gen}
      n_native    size of the native set
      q, rg       {range, hist_ref, hist_gen ({counts [n_bins], under, over}), jsd, floor, mean_ref, std_ref, mean_gen,
                  std_gen} of Q = n_native(s) / n_native on [0, 1] and of Rg (Angstrom) on the reference's range widened
                  by 20 %; ``None`` where a set has no good structure, ``q`` also when no pair is native
    """
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z, groups=groups)
    sel = select_atoms(z, atoms)
    excl = excluded_pairs(bonds, z.shape[0], sel, exclude)
    glab = None if groups is None else groups_of(z, bonds, mapping, groups)[sel]
    kw = dict(sel=sel, cutoff=cutoff, excluded=excl, groups=glab, structures_per_launch=structures_per_launch, device=device)
    even, odd = contact_counts(ref[0::2], **kw), contact_counts(ref[1::2], **kw)
    if glab is None:
        allowed, labels = ~excl, sel
    else:
        labels, dense = np.unique(glab, return_inverse=True)
        allowed = np.zeros((labels.shape[0],) * 2, dtype=bool)
        np.logical_or.at(allowed, (dense[:, None], dense[None, :]), ~excl)     # a pair of groups counts when a pair of its atoms does
        np.fill_diagonal(allowed, False)
    native = native_set(even, odd, allowed, native_min)
    if native.any():                                          # n_native of every structure needs the set
        even, odd = contact_counts(ref[0::2], native=native, **kw), contact_counts(ref[1::2], native=native, **kw)
    got = contact_counts(gen, native=native if native.any() else None, **kw)
    params = {"atoms": [int(i) for i in sel], "cutoff": float(cutoff), "exclude": int(exclude), "groups": groups,
              "native_min": float(native_min)}
    return compare_from_counts(even, odd, got, allowed, native, labels=labels, n_bins=n_bins, params=params)


CONTACT_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "labels", "p_ref", "p_gen", "map_rmse", "map_max_dev",
                      "floor", "top_pairs", "n_native", "q", "rg")


def summary_of(stats: dict) -> dict:
    """What the command-line tools put under ``"contact_stats"`` in their JSON summary line: no maps, no histograms."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "map_rmse", "map_max_dev", "floor", "n_native")}
    for k in ("q", "rg"):
        short[k] = ensemble.short_block(stats[k])
    return short
