"""Which residues of an ensemble are helix, strand, turn or bend: the DSSP class (Kabsch & Sander 1983) of every residue of
every structure of a peptide, how often every residue is in every class, and per structure the residues of every class --
assigned on the device (K26, ``cgv_dssp_assign``; ``csrc/dssp.hip``) -- and whether generated structures keep the secondary
structure the data has.

``hbonds.backbone_map`` stops one step short: it reports N-H(i)...O=C(j) occupancies, not the per-residue strings every
MD paper reports.  An ensemble can keep most of its native hydrogen bonds and still have lost a strand register; only a
pattern analysis sees that.  DSSP needs backbone heavy atoms alone -- the amide hydrogen is virtual -- so it works on
heavy-atom molecules too.

Definition.  The residues are those of ``ensemble.peptide_residues`` in chain order (``backbone_table``): ``res [R,4]`` = N,
CA, C, O; ``prev [R,2]`` = the carbonyl C' bonded to N and its O' (``-1, -1``: no amide hydrogen, the residue never
donates); ``link [R]`` = 1 iff C(r) is bonded to N(r+1).  All of it in fp32 with every operation rounded on its own
(``sq`` and ``sq_dist2`` are ``(dx*dx + dy*dy) + dz*dz``, csrc/sq_dist.h), every test written so that a NaN fails it:

    virtual hydrogen   w = C' - O',  l = sqrtf(sq(w)),  H_k = N_k + w_k / l
    hb[i][j]           C=O of i accepts from N-H of j:  j has an H,  j != i,  j != i + 1,
                       sq_dist2(CA_i, CA_j) < fp32(81)  and  e < fp32(-0.5),
                       e = fp32(27.888) * (((1/rON + 1/rCH) - 1/rOH) - 1/rCN),  r = sqrtf(d2);
                       e = fp32(-9.9) when any of the four d2 < fp32(0.25)
    cont(a, b)         link[a .. b-1] are all 1
    turn_n(i)          hb[i][i+n] and cont(i, i+n),  n = 3, 4, 5
    bridge (i, j)      |i-j| >= 3, i+-1 and j+-1 exist, cont(i-1, i+1) and cont(j-1, j+1):
                       par(i,j)  = (hb[i-1][j] & hb[j][i+1]) | (hb[j-1][i] & hb[i][j+1])
                       anti(i,j) = (hb[i][j] & hb[j][i])     | (hb[i-1][j+1] & hb[j-1][i+1])
                       in a ladder when the same type also holds at (i+1, j+1) or (i-1, j-1) for par,
                       at (i+1, j-1) or (i-1, j+1) for anti
    bend(i)            cont(i-2, i+2), u = CA_i - CA_{i-2}, v = CA_{i+2} - CA_i:
                       uu > 0, vv > 0 and (dot <= 0 or dot*dot < (c2*uu)*vv),  c2 = fp32(cos(70 degrees)^2)

and the classes in the 1983 priority, each stage reading only finished earlier stages:

    H  i..i+3 where turn_4(i-1) & turn_4(i)
    E  not H, and has a bridge that is in a ladder
    B  not H, and has a bridge but none in a ladder
    G  i..i+2 where turn_3(i-1) & turn_3(i), and none of the three is H / E / B
    I  i..i+4 where turn_5(i-1) & turn_5(i), and none of the five is H / E / B / G
    T  still unassigned, and turn_n(i-k) for some n and 1 <= k < n
    S  still unassigned, and bend
    -  otherwise

A code is the index into ``CODES = "HBEGITS-"``; the reduced states are helix = H G I, strand = E B, and coil.  What differs
from mkdssp: ``e`` is not rounded to 0.001 kcal/mol; a residue may have any number of partners, not only its two best; ladders
are not joined across beta bulges; alpha helices are assigned before pi helices (as in 1983, not as mkdssp >= 2.1 does).  A
``numpy.float32`` restatement reproduces every integer exactly; no floating-point result leaves the device, and two calls
give the same bits.  A structure with a non-finite coordinate in any atom of the tables is *bad*: its ``n_class`` row is
``-1``, its codes are ``255`` and it enters no sum.

    python -m coarsegrainingvae_amd.dssp -gen samples.npz -ref traj.npz [-top top.npz] [-codes codes.npz] [-out dssp_stats.json]

``-gen``: the ``xyz [T, K, n, 3]`` (or ``[S, n, 3]``) that ``backmap -out`` writes; ``-ref``: a trajectory file with
``xyz [T, n, 3]``; ``z`` and ``bonds`` come from ``-top``, else from ``-ref``.  The full statistics of ``compare`` go to
``-out``, one JSON line with ``"dssp_stats": summary_of(...)`` to stdout; ``-codes`` takes the class of every residue of
every generated structure (``codes [S, R]`` uint8 with ``strings``, ``bad`` and the tables).
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .ensemble import adjacency, check_sets, device_of, peptide_residues, read_back, scalar_block, structures

CODES = "HBEGITS-"
BAD_CODE = 255                       # the code of every residue of a bad structure; ``strings`` writes it as "?"
STATES3 = "HE-"                      # the reduced states: helix, strand, coil
HELIX, STRAND, COIL = (0, 3, 4), (2, 1), (5, 6, 7)       # the codes of a reduced state


def limits() -> Dict[str, int]:
    return ensemble.limits("dssp", ("structures", "residues"))


# ----------------------------------------------------------------------------- host: tables
def backbone_table(z, bonds) -> Dict[str, np.ndarray]:
    """The tables of the kernel, int32: ``res [R,4]`` (N, CA, C, O), ``prev [R,2]`` (C', O' in front of N; ``-1, -1``:
    none, or N has three heavy neighbours as in proline) and ``link [R]`` (1 iff C(r) is bonded to N(r+1)).  The residues
    are those of ``ensemble.peptide_residues`` (a triple is dropped when one of its atoms is already used, the rule of
    ``ensemble.groups_of``), re-ordered into chain order: chains are walked from every residue whose N has no preceding
    residue, in the order of that N's atom index.  ``ValueError`` without a peptide backbone and for a cyclic one."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    nbrs = adjacency(z.shape[0], bonds)
    is_amide, found = peptide_residues(z, nbrs)
    residues, used = [], set()
    for triple in found:                                      # in the order of N, as ensemble.groups_of numbers them
        if not used & set(triple):
            residues.append(triple)
            used |= set(triple)
    if not residues:
        raise ValueError("the molecule has no peptide backbone: no N - CA - C' was found in the bond graph")
    of_n = {N: k for k, (N, _, _) in enumerate(residues)}
    nxt, before = [-1] * len(residues), [-1] * len(residues)
    for k, (N, _, C) in enumerate(residues):
        for a in nbrs[C]:
            if a != N and a in of_n and before[of_n[a]] < 0 and nxt[k] < 0:
                nxt[k], before[of_n[a]] = of_n[a], k
    order = []
    for k in range(len(residues)):                            # chain starts in ascending N: the residues are in that order
        if before[k] >= 0:
            continue                                          # reached from its chain's start
        while k >= 0:
            order.append(k)
            k = nxt[k]
    if len(order) != len(residues):
        raise ValueError("the peptide backbone is cyclic: a chain has no residue whose N is free")
    carbonyl = lambda c: [o for o in nbrs[c] if z[o] == 8 and len(nbrs[o]) == 1][0]
    res, prev, link = [], [], []
    for pos, k in enumerate(order):
        N, CA, C = residues[k]
        res.append([N, CA, C, carbonyl(C)])
        heavy = [a for a in nbrs[N] if z[a] != 1]
        amides = [c for c in nbrs[N] if c != CA and is_amide[c]]
        prev.append([amides[0], carbonyl(amides[0])] if amides and len(heavy) < 3 else [-1, -1])
        following = residues[order[pos + 1]][0] if pos + 1 < len(order) else -1
        link.append(1 if following in nbrs[C] else 0)
    return {"res": np.array(res, dtype=np.int32).reshape(-1, 4), "prev": np.array(prev, dtype=np.int32).reshape(-1, 2),
            "link": np.array(link, dtype=np.int32)}


# ----------------------------------------------------------------------------- the launches
def assign(xyz, z, bonds, codes: bool = False, hb_bits: bool = False, structures_per_launch: int = 4096, device="cuda") -> dict:
    """The secondary structure of the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device
    tensor decides the device) of the peptide ``z [n]`` / ``bonds [Eb,2]``.  Host arrays:

      class_counts [R,8] int64   in how many good structures residue r has class c (``CODES``)
      n_class [S,8] int64        the residues of every class in structure s (a row sums to R; -1: bad structure)
      bad [S] bool, n_good       structures that are not bad (the denominator of a propensity)
      res [R,4], prev [R,2], link [R] int32, R   the tables (``backbone_table``)
      codes [S,R] uint8          with ``codes`` only: the class of every residue (255: bad structure)
      hb_bits [S,R,W] uint64     with ``hb_bits`` only: bit ``j & 63`` of word ``j >> 6`` of row i is set iff C=O of i
                                 accepts from N-H of j; ``W = ceil(R / 64)``

    The structures go through in launches of ``structures_per_launch``; the sums stay on the device; ONE read-back.
    Refused with ``ValueError`` before any launch: a molecule without a peptide backbone or with a cyclic one, more residues
    than ``limits()``, ``z`` / ``bonds`` that do not match the frames."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    if zz.shape[0] != n:
        raise ValueError(f"z lists {zz.shape[0]} atoms, a structure has {n}")
    table = backbone_table(zz, bonds)
    R = int(table["res"].shape[0])
    lim = limits()
    if R > lim["residues"]:
        raise ValueError(f"the peptide has {R} residues (the kernel holds {lim['residues']})")
    if S >= 2 ** 31:
        raise ValueError("fewer than 2^31 structures")
    W = (R + 63) // 64
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(structures_per_launch, lim["structures"], 12 * n)
    out = {"class_counts": torch.zeros(R, 8, dtype=torch.int64, device=dev), "n_class": torch.zeros(S, 8, dtype=torch.int32, device=dev),
           "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if codes:
        out["codes"] = torch.zeros(S, R, dtype=torch.uint8, device=dev)
    if hb_bits:
        out["hb_bits"] = torch.zeros(S, R, W, dtype=torch.int64, device=dev)
    if S:
        d_res, d_prev, d_link = (torch.from_numpy(np.ascontiguousarray(table[k])).to(dev) for k in ("res", "prev", "link"))
        for start, chunk in ensemble.chunks(x, M, dev):
            k = int(chunk.shape[0])
            _lib.call("cgv_dssp_assign", _lib.ptr(chunk), _lib.ptr(d_res), _lib.ptr(d_prev), _lib.ptr(d_link), k, n, R,
                      _lib.ptr(out["class_counts"]), _lib.ptr(out["n_class"][start:start + k]), _lib.ptr(out["bad"][start:start + k]),
                      _lib.ptr(out["codes"][start:start + k]) if codes else None,
                      _lib.ptr(out["hb_bits"][start:start + k]) if hb_bits else None, _lib.stream_ptr(), tag="dssp_assign")
    keys = list(out)
    host = dict(zip(keys, read_back([out[k] for k in keys])))
    got = {"class_counts": host["class_counts"], "n_class": host["n_class"].astype(np.int64), "bad": host["bad"].astype(bool),
           "n_good": int(S - int(host["bad"].sum())), **table, "R": R}
    if codes:
        got["codes"] = host["codes"]
    if hb_bits:
        got["hb_bits"] = host["hb_bits"].view(np.uint64)
    return got


# ----------------------------------------------------------------------------- host statistics
def strings(codes) -> List[str]:
    """One string of ``CODES`` per structure from ``codes [S,R]``; a bad structure (255) is a row of ``?``."""
    letters = np.array(list(CODES) + ["?"])
    c = np.asarray(codes).astype(np.int64).reshape(-1, np.asarray(codes).shape[-1])
    return ["".join(row) for row in letters[np.where(c < len(CODES), c, len(CODES))]]


def propensity(res: dict) -> Optional[np.ndarray]:
    """``class_counts / n_good`` (fp64 ``[R,8]``), or ``None`` when no structure is good."""
    return None if res["n_good"] <= 0 else np.asarray(res["class_counts"], dtype=np.float64) / float(res["n_good"])


def reduce3(table: np.ndarray) -> np.ndarray:
    """``[..., 8]`` over the classes to ``[..., 3]`` over helix, strand, coil."""
    t = np.asarray(table)
    return np.stack([t[..., list(group)].sum(axis=-1) for group in (HELIX, STRAND, COIL)], axis=-1)


def _rmse(p, q) -> Optional[float]:
    return None if p is None or q is None else float(np.sqrt(np.mean((p - q) ** 2)))


def _agreement(res: dict, consensus: Optional[np.ndarray]) -> Optional[float]:
    """The mean over the good structures of the share of residues whose reduced state is the consensus'."""
    if consensus is None or res["n_good"] <= 0:
        return None
    c3 = reduce3(np.asarray(res["class_counts"], dtype=np.int64))
    return float(c3[np.arange(c3.shape[0]), consensus].sum() / (float(res["n_good"]) * c3.shape[0]))


def _fraction(res: dict, group) -> np.ndarray:
    good = ~np.asarray(res["bad"], dtype=bool)
    n = np.asarray(res["n_class"], dtype=np.float64)[good]
    return n[:, list(group)].sum(axis=1) / float(np.asarray(res["class_counts"]).shape[0])


def compare_from_counts(even: dict, odd: dict, gen: dict) -> dict:
    """The statistics of ``compare`` from three results of ``assign`` -- the even reference frames, the odd ones and the
    generated structures of one molecule -- pure host.  Bad structures are in no denominator.  Keys: ``DSSP_STATS_KEYS``;
    see ``compare``."""
    R = int(np.asarray(gen["class_counts"]).shape[0])
    ref = {**even, "class_counts": np.asarray(even["class_counts"], dtype=np.int64) + np.asarray(odd["class_counts"], dtype=np.int64),
           "n_good": even["n_good"] + odd["n_good"]}
    p_ref, p_gen, p_even, p_odd = propensity(ref), propensity(gen), propensity(even), propensity(odd)
    q_ref, q_gen = (None if p is None else reduce3(p) for p in (p_ref, p_gen))
    consensus = None if q_ref is None else np.argmax(reduce3(ref["class_counts"]), axis=1)      # a tie: helix, then strand
    lost = gained = None
    if q_ref is not None and q_gen is not None:
        lost = [[int(r), STATES3[k]] for r in range(R) for k in (0, 1) if q_ref[r, k] >= 0.5 and q_gen[r, k] < 0.1]
        gained = [[int(r), STATES3[k]] for r in range(R) for k in (0, 1) if q_gen[r, k] >= 0.5 and q_ref[r, k] < 0.1]
    blocks = {}
    for name, group in (("helix_fraction", HELIX), ("strand_fraction", STRAND)):
        fe, fo, fg = _fraction(even, group), _fraction(odd, group), _fraction(gen, group)
        blocks[name] = scalar_block(fe, fo, fg, -0.5 / R, (R + 0.5) / R, R + 1) if fe.size + fo.size and fg.size else None
    as_list = lambda a: None if a is None else a.tolist()
    return {**ensemble.set_sizes(even, odd, gen), "R": R, "codes": CODES, "states": STATES3,
            "propensity_ref": as_list(p_ref), "propensity_gen": as_list(p_gen), "propensity3_ref": as_list(q_ref),
            "propensity3_gen": as_list(q_gen), "propensity_rmse": _rmse(p_ref, p_gen),
            "floor": {"propensity_rmse": _rmse(p_even, p_odd),
                      "helix_fraction_jsd": blocks["helix_fraction"]["floor"] if blocks["helix_fraction"] else None,
                      "strand_fraction_jsd": blocks["strand_fraction"]["floor"] if blocks["strand_fraction"] else None},
            "consensus_ref": None if consensus is None else "".join(STATES3[k] for k in consensus),
            "agreement_ref": _agreement(ref, consensus), "agreement_gen": _agreement(gen, consensus),
            "lost": lost, "gained": gained, **blocks}


def compare(ref_xyz, gen_xyz, z, bonds, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) of the
    peptide ``z [n]`` / ``bonds [Eb,2]`` by their secondary structure.  The convention of ``contacts.compare``: the
    generated structures, the even and the odd frames of the reference are assigned apart, the reference is the integer
    sum of its halves, and what the halves differ by is the ``floor`` every deviation is to be read against.  Returns a
    dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      R, codes, states                       residues; the letters of the 8 classes and of the 3 reduced states
      propensity_ref, propensity_gen         [R][8]: the share of good structures in which residue r has class c
      propensity3_ref, propensity3_gen       [R][3]: the same over helix (H G I), strand (E B), coil
      propensity_rmse                        of generated against reference over the [R][8] entries (``None``: a set
                                             without a good structure)
      floor       {propensity_rmse, helix_fraction_jsd, strand_fraction_jsd}: the same between the even and the odd frames
      consensus_ref                          the reduced state most of the reference has, per residue, as a string of H E -
      agreement_ref, agreement_gen           the mean share of residues whose reduced state is the consensus'
      lost, gained                           [residue, "H" or "E"]: helix or strand propensity >= 0.5 in the reference and
                                             < 0.1 in the generated set (lost), or the other way round (gained)
      helix_fraction, strand_fraction        {range, hist_ref, hist_gen, jsd, floor, mean_ref, std_ref, mean_gen, std_gen} of
                                             the share of a structure's residues in the state, one bin per residue count
    """
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z)
    kw = dict(structures_per_launch=structures_per_launch, device=device)
    return compare_from_counts(assign(ref[0::2], z, bonds, **kw), assign(ref[1::2], z, bonds, **kw), assign(gen, z, bonds, **kw))


DSSP_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "R", "codes", "states", "propensity_ref", "propensity_gen",
                   "propensity3_ref", "propensity3_gen", "propensity_rmse", "floor", "consensus_ref", "agreement_ref",
                   "agreement_gen", "lost", "gained", "helix_fraction", "strand_fraction")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"dssp_stats"`` in its JSON summary line: no profiles, no histograms."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "R", "propensity_rmse", "floor", "consensus_ref",
                                   "agreement_ref", "agreement_gen")}
    short["n_lost"] = None if stats["lost"] is None else len(stats["lost"])
    short["n_gained"] = None if stats["gained"] is None else len(stats["gained"])
    short["helix_fraction"] = ensemble.short_block(stats["helix_fraction"])
    short["strand_fraction"] = ensemble.short_block(stats["strand_fraction"])
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.dssp", "secondary structure (DSSP) of generated structures against a reference",
                                top_help="npz with z and bonds; default: those of -ref")
    p.add_argument("-codes", default=None, help="npz that takes the class of every residue of every generated structure (not written)")
    return compare_cli.finish_parser(p, "dssp_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, with everything that can be refused without
    a device refused here (``SystemExit``)."""
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args)
    bonds = np.asarray(top["bonds"])
    with compare_cli.refusing():
        R = int(backbone_table(z, bonds)["res"].shape[0])
        if R > limits()["residues"]:
            raise ValueError(f"the peptide has {R} residues (the kernel holds {limits()['residues']})")
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": bonds}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    with compare_cli.refusing():
        stats = compare(inp["ref_xyz"], inp["gen_xyz"], inp["z"], inp["bonds"], device=args.device)
        if args.codes:
            res = assign(inp["gen_xyz"], inp["z"], inp["bonds"], codes=True, device=args.device)
            np.savez(args.codes, codes=res["codes"], strings=np.array(strings(res["codes"])), bad=res["bad"], res=res["res"],
                     prev=res["prev"], link=res["link"])
    compare_cli.finish("dssp", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
