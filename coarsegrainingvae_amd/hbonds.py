"""Which hydrogen bonds an ensemble has: for every pair (donor hydrogen, acceptor) of a molecule, in how many structures
it is hydrogen bonded, per structure the number of bonds and of NATIVE bonds, and on request every bond of every structure
as a bit -- counted on the device (K25, ``cgv_hbond_counts``; ``csrc/hbond.hip``) -- and whether generated structures keep
the bonds the data has.

None of the other analyses sees a hydrogen bond: ``contacts`` counts heavy-atom pairs within 4.5 Angstrom, and an ensemble
with every donor hydrogen turned away from its acceptor passes it, ``sasa``, ``flexibility`` and ``cluster`` untouched.
Hydrogens carry no weight in a bead position, so their placement is what a backmapping decoder gets wrong first.

Definition (Baker-Hubbard, intramolecular).  A *donor hydrogen* is an H (``z == 1``) bonded to exactly one heavy atom D with
``z[D]`` in ``donor_elements`` (default N, O).  An *acceptor* is an atom with ``z`` in ``acceptor_elements`` (default N, O).
The table has ``nH`` donor hydrogens and ``nA`` acceptors, ``W = ceil(nA / 64)``.  A pair (h, a) is *excluded* when A is D
itself, when A is bonded to D, or when the caller's own exclusion mask names it.  In a structure the pair is bonded iff it
is not excluded and, in fp32 with every operation rounded on its own,

    d2  = (dx*dx + dy*dy) + dz*dz  of A - H          (csrc/sq_dist.h)
    l2  = the same of D - H
    dot = (ux*vx + uy*vy) + uz*vz,  u = D - H, v = A - H
    d2 < cutoff2  and  dot < 0  and  dot*dot > (c2 * l2) * d2

with ``cutoff2 = fp32(h_a_cutoff) * fp32(h_a_cutoff)`` (default 2.5 Angstrom) and ``c2 = fp32(cos(angle)^2)``, computed in
fp64 and rounded once.  ``angle`` (default 120 degrees) is the least D-H...A angle and must lie in [90, 180): there
``cos(angle) <= 0`` and the last two tests are ``cos(D-H-A) < cos(angle)`` without a square root.  A ``numpy.float32``
restatement reproduces every integer exactly; no floating-point result leaves the device, and two calls give the same bits.
A structure with a non-finite coordinate among its D, H or A atoms is *bad*: its per-structure values are ``-1`` and it
enters no sum.

    python -m coarsegrainingvae_amd.hbonds -gen samples.npz -ref traj.npz [-top top.npz] [-hbond_cutoff 2.5]
        [-hbond_angle 120] [-hbond_native 0.5] [-bits bits.npz] [-out hbond_stats.json]

``-gen``: the ``xyz [T, K, n, 3]`` (or ``[S, n, 3]``) that ``backmap -out`` writes; ``-ref``: a trajectory file with
``xyz [T, n, 3]``; ``z`` and ``bonds`` come from ``-top``, else from ``-ref``.  The full statistics of ``compare`` go to
``-out``, one JSON line with ``"hbond_stats": summary_of(...)`` to stdout; ``-bits`` takes the bonds of every generated
structure (``bits [S, nH, W]`` uint64 with the tables).
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .contacts import cutoff2_of
from .ensemble import adjacency, check_sets, device_of, peptide_residues, read_back, scalar_block, structures


def limits() -> Dict[str, int]:
    return ensemble.limits("hbond", ("structures", "hydrogens", "acceptors"))


def c2_of(angle: float) -> np.float32:
    """``fp32(cos(angle)^2)`` of the least D-H...A angle in degrees, fp64 rounded once; ``ValueError`` outside [90, 180)."""
    a = float(angle)
    if not (math.isfinite(a) and 90.0 <= a < 180.0):
        raise ValueError(f"the angle must lie in [90, 180) degrees, got {angle}")
    return np.float32(math.cos(math.radians(a)) ** 2)


# ----------------------------------------------------------------------------- host: tables and masks
def donors_acceptors(z, bonds, donor_elements=(7, 8), acceptor_elements=(7, 8)):
    """``(don_h [nH], don_d [nH], acc [nA])`` int32, in ascending atom order: the hydrogens bonded to exactly one heavy
    atom, of a donor element, with that atom; the atoms of an acceptor element.  ``ValueError`` for a molecule without a
    donor hydrogen or without an acceptor."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    nbrs = adjacency(z.shape[0], bonds)
    donors, acceptors = {int(e) for e in donor_elements}, {int(e) for e in acceptor_elements}
    don_h, don_d = [], []
    for h in np.flatnonzero(z == 1).tolist():
        heavy = [b for b in nbrs[h] if z[b] != 1]
        if len(heavy) == 1 and int(z[heavy[0]]) in donors:
            don_h.append(h)
            don_d.append(heavy[0])
    acc = [a for a in range(z.shape[0]) if int(z[a]) in acceptors]
    if not don_h:
        raise ValueError("the molecule has no donor hydrogen: no H bonded to exactly one heavy atom of a donor element")
    if not acc:
        raise ValueError("the molecule has no acceptor: no atom of an acceptor element")
    return np.array(don_h, dtype=np.int32), np.array(don_d, dtype=np.int32), np.array(acc, dtype=np.int32)


def _bool_mask(mask, nH: int, nA: int, what: str) -> np.ndarray:
    """A bool ``[nH, nA]`` from a bool array of that shape or from pairs ``[(row, column), ...]`` of table positions."""
    a = np.asarray(mask)
    if a.dtype == np.bool_:
        if a.shape != (nH, nA):
            raise ValueError(f"{what} must be a bool array [{nH}, {nA}] or a list of (row, column), got {a.shape}")
        return a
    out = np.zeros((nH, nA), dtype=bool)
    p = a.astype(np.int64).reshape(-1, 2)
    if p.shape[0]:
        if p.min() < 0 or p[:, 0].max() >= nH or p[:, 1].max() >= nA:
            raise ValueError(f"{what} names a pair outside the [{nH}, {nA}] table")
        out[p[:, 0], p[:, 1]] = True
    return out


def pack_mask(mask, nH: Optional[int] = None, nA: Optional[int] = None) -> np.ndarray:
    """A mask over the table as the kernel takes it, uint64 ``[nH, W]``: bit ``a & 63`` of word ``a >> 6`` of row ``h``.
    ``mask``: bool ``[nH, nA]``, or pairs ``[(h, a), ...]`` of table positions with the table's ``nH`` and ``nA``."""
    a = np.asarray(mask)
    if a.dtype == np.bool_ and a.ndim == 2:
        nH, nA = a.shape
    elif nH is None or nA is None:
        raise ValueError("a list of pairs needs the table's nH and nA")
    m = _bool_mask(a, int(nH), int(nA), "the mask")
    W = (int(nA) + 63) // 64
    padded = np.zeros((int(nH), 64 * W), dtype=bool)
    padded[:, :int(nA)] = m
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    words = np.bitwise_or.reduce(np.where(padded.reshape(int(nH), W, 64), weights, np.uint64(0)), axis=-1)
    return np.ascontiguousarray(words.astype(np.uint64))


def unpack_mask(words, nA: int) -> np.ndarray:
    """The inverse of ``pack_mask`` on the last axis: bool ``[..., nA]`` from uint64 ``[..., W]``."""
    w = np.asarray(words, dtype=np.uint64)
    shifts = np.arange(64, dtype=np.uint64)
    flat = ((w[..., None] >> shifts) & np.uint64(1)).astype(bool).reshape(*w.shape[:-1], -1)
    return flat[..., :int(nA)]


def excluded_pairs(don_d, acc, bonds, extra=None) -> np.ndarray:
    """Bool ``[nH, nA]``: the acceptor is the donor itself or bonded to it, or ``extra`` (bool ``[nH, nA]`` or pairs of
    table positions) names the pair."""
    don_d = np.asarray(don_d, dtype=np.int64).reshape(-1)
    acc = np.asarray(acc, dtype=np.int64).reshape(-1)
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    n = int(max(don_d.max(initial=-1), acc.max(initial=-1), b.max(initial=-1))) + 1
    nbrs = adjacency(n, b)
    out = np.zeros((don_d.shape[0], acc.shape[0]), dtype=bool)
    for k, d in enumerate(don_d.tolist()):
        out[k] = (acc == d) | np.isin(acc, nbrs[d])
    if extra is not None:
        out |= _bool_mask(extra, out.shape[0], out.shape[1], "the extra exclusions")
    return out


def excluded_mask(don_d, acc, bonds, extra=None) -> np.ndarray:
    """``pack_mask(excluded_pairs(...))``: uint64 ``[nH, W]``."""
    return pack_mask(excluded_pairs(don_d, acc, bonds, extra))


# ----------------------------------------------------------------------------- the launches
def _dev_words(words: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(dev)


def hbond_counts(xyz, z, bonds, donor_elements=(7, 8), acceptor_elements=(7, 8), h_a_cutoff: float = 2.5, angle: float = 120.0,
                 excluded=None, native=None, per_pair: bool = False, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Hydrogen bonds of the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device tensor
    decides the device) of the molecule ``z [n]`` / ``bonds [Eb,2]``.  ``excluded``: the caller's own exclusions and
    ``native``: the pairs ``n_native`` counts, each a bool ``[nH,nA]`` or pairs of table positions.  Host arrays:

      pair_counts [nH,nA] int64  in how many good structures the pair is bonded
      n_hbonds [S] int64         bonds of structure s;  n_native [S] int64 those of them in ``native`` (-1: bad structure)
      bad [S] bool, n_good       structures that are not bad (the denominator of an occupancy)
      don_h, don_d [nH], acc [nA] int32   the tables (``donors_acceptors``)
      excluded [nH,nA] bool      the pairs that never count (``excluded_pairs``)
      h_a_cutoff, angle, cutoff2, c2     the parameters, and what the kernel took for them (fp32)
      bits [S,nH,W] uint64       with ``per_pair`` only: bit ``a & 63`` of word ``a >> 6`` is set iff (h, a) is bonded

    The structures go through in launches of ``structures_per_launch``; the sums stay on the device; ONE read-back.
    Refused with ``ValueError`` before any launch: a molecule with no donor hydrogen or no acceptor, an angle outside
    [90, 180), a cutoff that is not finite or is negative, a table beyond ``limits()``, ``z`` / ``bonds`` that do not match
    the frames."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    if zz.shape[0] != n:
        raise ValueError(f"z lists {zz.shape[0]} atoms, a structure has {n}")
    cutoff2, c2 = cutoff2_of(h_a_cutoff), c2_of(angle)
    if not np.isfinite(cutoff2):
        raise ValueError(f"the cutoff must be a finite distance >= 0, got {h_a_cutoff}")
    don_h, don_d, acc = donors_acceptors(zz, bonds, donor_elements, acceptor_elements)
    nH, nA = int(don_h.shape[0]), int(acc.shape[0])
    lim = limits()
    if nH > lim["hydrogens"] or nA > lim["acceptors"]:
        raise ValueError(f"the table is {nH} donor hydrogens x {nA} acceptors (the kernel holds {lim['hydrogens']} x {lim['acceptors']})")
    if S >= 2 ** 31:
        raise ValueError("fewer than 2^31 structures")
    excl = excluded_pairs(don_d, acc, bonds, excluded)
    nat = None if native is None else _bool_mask(native, nH, nA, "native")
    W = (nA + 63) // 64
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(structures_per_launch, lim["structures"], 16 * (2 * nH + nA))
    out = {"pair_counts": torch.zeros(nH, nA, dtype=torch.int64, device=dev), "n_hbonds": torch.zeros(S, dtype=torch.int32, device=dev),
           "n_native": torch.zeros(S, dtype=torch.int32, device=dev), "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if per_pair:
        out["bits"] = torch.zeros(S, nH, W, dtype=torch.int64, device=dev)
    if S:
        lib = _lib.load()
        d_h, d_d, d_a = (torch.from_numpy(a).to(dev) for a in (don_h, don_d, acc))
        d_excl = _dev_words(pack_mask(excl), dev)
        d_nat = None if nat is None else _dev_words(pack_mask(nat), dev)
        need = int(lib.cgv_hbond_workspace_bytes(min(M, S), nH, nA))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        for start, chunk in ensemble.chunks(x, M, dev):
            k = int(chunk.shape[0])
            _lib.call("cgv_hbond_counts", _lib.ptr(chunk), _lib.ptr(d_h), _lib.ptr(d_d), _lib.ptr(d_a), _lib.ptr(d_excl),
                      _lib.ptr(d_nat), k, n, nH, nA, float(cutoff2), float(c2), _lib.ptr(out["pair_counts"]),
                      _lib.ptr(out["n_hbonds"][start:start + k]), _lib.ptr(out["n_native"][start:start + k]),
                      _lib.ptr(out["bad"][start:start + k]), _lib.ptr(out["bits"][start:start + k]) if per_pair else None,
                      _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), tag="hbond_counts")
    keys = list(out)
    host = dict(zip(keys, read_back([out[k] for k in keys])))
    res = {"pair_counts": host["pair_counts"], "n_hbonds": host["n_hbonds"].astype(np.int64),
           "n_native": host["n_native"].astype(np.int64), "bad": host["bad"].astype(bool),
           "n_good": int(S - int(host["bad"].sum())), "don_h": don_h, "don_d": don_d, "acc": acc, "excluded": excl,
           "h_a_cutoff": float(h_a_cutoff), "angle": float(angle), "cutoff2": cutoff2, "c2": c2}
    if per_pair:
        res["bits"] = host["bits"].view(np.uint64)
    return res


# ----------------------------------------------------------------------------- host statistics
def occupancy(res: dict) -> Optional[np.ndarray]:
    """``pair_counts / n_good`` (fp64 ``[nH, nA]``), or ``None`` when no structure is good."""
    return None if res["n_good"] <= 0 else np.asarray(res["pair_counts"], dtype=np.float64) / float(res["n_good"])


def backbone_map(res: dict, z, bonds) -> Optional[np.ndarray]:
    """``[R, R]`` fp64: entry (i, j) is the occupancy of N-H(i)...O=C(j) between the residues of a peptide
    (``ensemble.peptide_residues``, numbered in the order of their N), summed over the hydrogens of N(i) and the carbonyl
    oxygens of C(j).  ``None`` when the molecule has no peptide backbone or the result no good structure."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    nbrs = adjacency(z.shape[0], bonds)
    _, found = peptide_residues(z, nbrs)
    residues, used = [], set()
    for triple in found:                                      # in the order of N, as ensemble.groups_of numbers them
        if not used & set(triple):
            residues.append(triple)
            used |= set(triple)
    occ = occupancy(res)
    if not residues or occ is None:
        return None
    don_d, acc = np.asarray(res["don_d"]), np.asarray(res["acc"])
    out = np.zeros((len(residues),) * 2, dtype=np.float64)
    for i, (N, _, _) in enumerate(residues):
        rows = np.flatnonzero(don_d == N)
        for j, (_, _, C) in enumerate(residues):
            oxy = [o for o in nbrs[C] if z[o] == 8 and len(nbrs[o]) == 1]
            cols = np.flatnonzero(np.isin(acc, oxy))
            out[i, j] = occ[np.ix_(rows, cols)].sum()
    return out


def native_pairs(even: dict, odd: dict, native_occupancy: float = 0.5) -> np.ndarray:
    """Bool ``[nH, nA]``: the pairs that are not excluded and whose occupancy over the whole reference (the integer sum of
    its even and odd frames) is at least ``native_occupancy``.  All False when the reference has no good structure."""
    good = even["n_good"] + odd["n_good"]
    allowed = ~np.asarray(even["excluded"], dtype=bool)
    if good <= 0:
        return np.zeros_like(allowed)
    counts = np.asarray(even["pair_counts"], dtype=np.int64) + np.asarray(odd["pair_counts"], dtype=np.int64)
    return (counts >= float(native_occupancy) * good) & allowed


def _dev(p, q, allowed):
    """RMSE and Pearson correlation of two occupancy tables over the pairs that count."""
    if p is None or q is None or not allowed.any():
        return None, None
    a, b = p[allowed], q[allowed]
    rmse = float(np.sqrt(np.mean((a - b) ** 2)))
    sa, sb = a.std(), b.std()
    return rmse, (float(np.mean((a - a.mean()) * (b - b.mean())) / (sa * sb)) if sa > 0 and sb > 0 else None)


def _kept(res_list, size: int) -> Optional[float]:
    vals = np.concatenate([np.asarray(r["n_native"], dtype=np.float64)[~np.asarray(r["bad"], dtype=bool)] for r in res_list])
    return float(vals.mean() / size) if size > 0 and vals.size else None


def compare_from_counts(even: dict, odd: dict, gen: dict, native=None, z=None, bonds=None, params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from three results of ``hbond_counts`` -- the even reference frames, the odd ones and
    the generated structures, all counted with the same tables, exclusions and ``native`` set (bool ``[nH, nA]``; default:
    none) -- pure host.  With ``z`` and ``bonds`` the backbone maps are added.  Bad structures are in no denominator.
    Keys: ``HBOND_STATS_KEYS``; see ``compare``."""
    don_h, don_d, acc = (np.asarray(gen[k]) for k in ("don_h", "don_d", "acc"))
    allowed = ~np.asarray(gen["excluded"], dtype=bool)
    nat = np.zeros_like(allowed) if native is None else (_bool_mask(native, *allowed.shape, "native") & allowed)
    ref = {**even, "pair_counts": np.asarray(even["pair_counts"], dtype=np.int64) + np.asarray(odd["pair_counts"], dtype=np.int64),
           "n_good": even["n_good"] + odd["n_good"]}
    p_ref, p_gen, p_even, p_odd = occupancy(ref), occupancy(gen), occupancy(even), occupancy(odd)
    rmse, pearson = _dev(p_ref, p_gen, allowed)
    f_rmse, f_pearson = _dev(p_even, p_odd, allowed)
    triple = lambda h, a: [int(don_d[h]), int(don_h[h]), int(acc[a])]
    zero = np.zeros(allowed.shape)
    o_ref, o_gen = (zero if p_ref is None else p_ref), (zero if p_gen is None else p_gen)
    pairs = [{"d": int(don_d[h]), "h": int(don_h[h]), "a": int(acc[a]), "occ_ref": None if p_ref is None else float(p_ref[h, a]),
              "occ_gen": None if p_gen is None else float(p_gen[h, a]), "native": bool(nat[h, a])}
             for h, a in zip(*np.nonzero(allowed & ((o_ref > 0) | (o_gen > 0))))]
    missing = spurious = None
    if p_gen is not None:
        missing = [triple(h, a) for h, a in zip(*np.nonzero(nat & (p_gen < 0.1)))]
        if p_ref is not None:
            spurious = [triple(h, a) for h, a in zip(*np.nonzero(allowed & ~nat & (p_gen >= 0.5) & (p_ref < 0.1)))]
    size = int(nat.sum())

    def good(res):
        return np.asarray(res["n_hbonds"], dtype=np.float64)[~np.asarray(res["bad"], dtype=bool)]
    ne, no, ng = good(even), good(odd), good(gen)
    block = None
    if ne.size + no.size and ng.size:                          # one bin per integer, up to the most bonds either set has
        top = int(max(np.concatenate([ne, no]).max(), ng.max()))
        block = scalar_block(ne, no, ng, -0.5, top + 0.5, top + 1)
    maps = {"backbone_ref": None, "backbone_gen": None}
    if z is not None and bonds is not None:
        for key, res in (("backbone_ref", ref), ("backbone_gen", gen)):
            m = backbone_map(res, z, bonds)
            maps[key] = None if m is None else m.tolist()
    return {**ensemble.set_sizes(even, odd, gen), "params": dict(params or {}), "n_donor_hydrogens": int(don_h.shape[0]), "n_acceptors": int(acc.shape[0]),
            "pairs": pairs, "occupancy_rmse": rmse, "occupancy_pearson": pearson,
            "floor": {"occupancy_rmse": f_rmse, "occupancy_pearson": f_pearson, "n_hbonds_jsd": block["floor"] if block else None},
            "n_native": size, "native": [triple(h, a) for h, a in zip(*np.nonzero(nat))],
            "kept_ref": _kept([even, odd], size), "kept_gen": _kept([gen], size), "missing": missing, "spurious": spurious,
            "n_hbonds": block, **maps}


def compare(ref_xyz, gen_xyz, z, bonds, donor_elements=(7, 8), acceptor_elements=(7, 8), h_a_cutoff: float = 2.5,
            angle: float = 120.0, excluded=None, native_occupancy: float = 0.5, structures_per_launch: int = 4096,
            device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) of the
    molecule ``z [n]`` / ``bonds [Eb,2]`` by their hydrogen bonds.  The convention of ``contacts.compare``: the generated
    structures, the even and the odd frames of the reference are counted apart, the reference is the integer sum of its
    halves, and what the halves differ by is the ``floor`` every deviation is to be read against.  The native set -- the
    pairs whose occupancy over the whole reference is at least ``native_occupancy`` -- needs the reference's table first,
    so the reference is counted once for its table and the three sets once with the native set.  Returns a dict that
    ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      params      h_a_cutoff, angle, native_occupancy, donor_elements, acceptor_elements
      n_donor_hydrogens, n_acceptors         the size of the table
      pairs       every pair bonded in a structure of either set: {d, h, a (atom indices), occ_ref, occ_gen, native}
      occupancy_rmse, occupancy_pearson      of generated against reference occupancy over the pairs that are not excluded
                  (``None``: a set without a good structure; the correlation also when a table is constant)
      floor       {occupancy_rmse, occupancy_pearson, n_hbonds_jsd}: the same between the even and the odd reference frames
      n_native, native   the size of the native set and its pairs as [D, H, A]
      kept_ref, kept_gen  the mean over the good structures of n_native(s) / n_native (``None`` without a native pair)
      missing     the native pairs with generated occupancy < 0.1, as [D, H, A]
      spurious    the pairs outside the native set with generated occupancy >= 0.5 and reference occupancy < 0.1
      n_hbonds    {range, hist_ref, hist_gen ({counts, under, over}), jsd, floor, mean_ref, std_ref, mean_gen, std_gen} of
                  the bonds of a structure, one bin per integer; ``None`` where a set has no good structure
      backbone_ref, backbone_gen   [R][R] occupancy of N-H(i)...O=C(j) (``backbone_map``); ``None`` without a peptide backbone
    """
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z)
    if not (math.isfinite(float(native_occupancy)) and 0.0 < float(native_occupancy) <= 1.0):
        raise ValueError(f"native_occupancy must lie in (0, 1], got {native_occupancy}")
    kw = dict(donor_elements=donor_elements, acceptor_elements=acceptor_elements, h_a_cutoff=h_a_cutoff, angle=angle,
              excluded=excluded, structures_per_launch=structures_per_launch, device=device)
    even, odd = hbond_counts(ref[0::2], z, bonds, **kw), hbond_counts(ref[1::2], z, bonds, **kw)
    native = native_pairs(even, odd, native_occupancy)
    if native.any():                                          # n_native of every structure needs the set
        even, odd = hbond_counts(ref[0::2], z, bonds, native=native, **kw), hbond_counts(ref[1::2], z, bonds, native=native, **kw)
    got = hbond_counts(gen, z, bonds, native=native if native.any() else None, **kw)
    params = {"h_a_cutoff": float(h_a_cutoff), "angle": float(angle), "native_occupancy": float(native_occupancy),
              "donor_elements": sorted(int(e) for e in donor_elements), "acceptor_elements": sorted(int(e) for e in acceptor_elements)}
    return compare_from_counts(even, odd, got, native=native, z=z, bonds=bonds, params=params)


HBOND_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "n_donor_hydrogens", "n_acceptors", "pairs",
                    "occupancy_rmse", "occupancy_pearson", "floor", "n_native", "native", "kept_ref", "kept_gen", "missing",
                    "spurious", "n_hbonds", "backbone_ref", "backbone_gen")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"hbond_stats"`` in its JSON summary line: no pair list, no maps, no histograms."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "occupancy_rmse", "occupancy_pearson", "floor",
                                   "n_native", "kept_ref", "kept_gen")}
    short["n_missing"] = None if stats["missing"] is None else len(stats["missing"])
    short["n_spurious"] = None if stats["spurious"] is None else len(stats["spurious"])
    short["n_hbonds"] = ensemble.short_block(stats["n_hbonds"])
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.hbonds", "hydrogen bonds of generated structures against a reference",
                                top_help="npz with z and bonds; default: those of -ref")
    p.add_argument("-hbond_cutoff", type=float, default=2.5, help="largest H...A distance in Angstrom (2.5)")
    p.add_argument("-hbond_angle", type=float, default=120.0, help="least D-H...A angle in degrees, in [90, 180) (120)")
    p.add_argument("-hbond_native", type=float, default=0.5, help="reference occupancy from which a pair is native, in (0, 1] (0.5)")
    p.add_argument("-bits", default=None, help="npz that takes the bonds of every generated structure as bits (not written)")
    return compare_cli.finish_parser(p, "hbond_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, with everything that can be refused without
    a device refused here (``SystemExit``)."""
    if not (math.isfinite(args.hbond_cutoff) and args.hbond_cutoff >= 0):
        raise SystemExit("-hbond_cutoff must be a finite length >= 0 in Angstrom")
    if not (math.isfinite(args.hbond_angle) and 90.0 <= args.hbond_angle < 180.0):
        raise SystemExit("-hbond_angle must lie in [90, 180) degrees")
    if not (math.isfinite(args.hbond_native) and 0.0 < args.hbond_native <= 1.0):
        raise SystemExit("-hbond_native must lie in (0, 1]")
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args)
    bonds = np.asarray(top["bonds"])
    with compare_cli.refusing():
        don_h, _, acc = donors_acceptors(z, bonds)
        lim = limits()
        if don_h.shape[0] > lim["hydrogens"] or acc.shape[0] > lim["acceptors"]:
            raise ValueError(f"the table is {don_h.shape[0]} donor hydrogens x {acc.shape[0]} acceptors "
                             f"(the kernel holds {lim['hydrogens']} x {lim['acceptors']})")
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": bonds}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    kw = dict(h_a_cutoff=args.hbond_cutoff, angle=args.hbond_angle, device=args.device)
    with compare_cli.refusing():
        stats = compare(inp["ref_xyz"], inp["gen_xyz"], inp["z"], inp["bonds"], native_occupancy=args.hbond_native, **kw)
        if args.bits:
            res = hbond_counts(inp["gen_xyz"], inp["z"], inp["bonds"], per_pair=True, **kw)
            np.savez(args.bits, bits=res["bits"], don_h=res["don_h"], don_d=res["don_d"], acc=res["acc"], bad=res["bad"])
    compare_cli.finish("hbond", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
