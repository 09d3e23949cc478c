"""Whether a generated ensemble PACKS like the data: the distribution of the distances between pairs of atoms, by kind of
atom -- the radial / pair distribution P(r) that force matching and iterative Boltzmann inversion are judged by -- counted
on the device for every pair and every structure (K29, ``cgv_pairdist_counts``; ``csrc/pair_hist.hip``).

``distributions`` histograms the bonded terms only, ``contacts`` counts the pairs under ONE cutoff (the first bin of what is
here), ``tica`` computes backbone distances but no distribution, ``lddt`` compares a sample with its own frame.  A model
that puts non-bonded carbons at 3.4 A where the data has them at 3.9 A passes all of them; its P(r) does not.

Definition.  Over the selection ``sel [m]`` (default: the heavy atoms) with a class ``cls [m]`` in ``[0, C)`` for every
atom, for a pair ``i < j`` that the mask does not exclude (default: pairs at most ``exclude`` = 3 bonds apart), in fp32
with every operation rounded on its own (``sqrtf`` correctly rounded):

    rmax2 = fp32(r_max) * fp32(r_max)                  scale = fp32(float64(n_bins) / float64(fp32(r_max)))
    q = (dx*dx + dy*dy) + dz*dz  of x_i - x_j                                              (csrc/sq_dist.h)
    in range  iff  q < rmax2                           strict, false for a NaN
    b = min(int(sqrtf(q) * scale), n_bins - 1)         one rounded product, truncation, clamp

An in-range pair counts in ``hist[p][b]``, every other pair in ``beyond[p]``, ``p = pair_index(cls_i, cls_j, C)`` one of
the ``C (C + 1) / 2`` unordered class pairs.  A ``numpy.float32`` restatement reproduces every integer exactly, no
floating-point number leaves the device, and two calls give the same bits however the structures are cut into launches.
Every statistic -- P(r), its mean, the Jensen-Shannon divergence and the first Wasserstein distance between two sets -- is
host fp64 on those integers.  A structure with a non-finite selected coordinate is *bad* and enters no sum.

    python -m coarsegrainingvae_amd.pairdist -gen samples.npz -ref traj.npz [-top top.npz] [-pd_atoms heavy|all]
        [-pd_classes element|none|bead] [-pd_rmax 20] [-pd_bins 100] [-pd_exclude 3] [-out pairdist_stats.json]

``z`` and ``bonds`` (and ``mapping`` for ``-pd_classes bead``) come from ``-top``, else from ``-ref``.  The full statistics
of ``compare`` go to ``-out``, one JSON line with ``"pairdist_stats": summary_of(...)`` to stdout.
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .contacts import cutoff2_of, excluded_pairs
from .ensemble import check_sets, device_of, groups_of, js_divergence, pack_mask, read_back, select_atoms, structures

SYMBOLS = {1: "H", 6: "C", 7: "N", 8: "O", 9: "F", 15: "P", 16: "S", 17: "Cl"}     # names of the element classes; else "Z<z>"


def limits() -> Dict[str, int]:
    return ensemble.limits("pairdist", ("structures", "atoms", "classes", "bins"))


# ----------------------------------------------------------------------------- host: parameters, classes
def scale_of(r_max: float, n_bins: int) -> np.float32:
    """Bins per Angstrom as the kernel takes it: the fp64 quotient of ``n_bins`` and the fp32 ``r_max``, rounded to fp32.
    ``ValueError`` unless ``r_max`` is a finite distance > 0 (and the quotient a finite fp32)."""
    r = np.float32(r_max)
    if not np.isfinite(r) or r <= 0:
        raise ValueError(f"r_max must be a finite distance > 0, got {r_max}")
    with np.errstate(over="ignore"):
        scale, rmax2 = np.float32(np.float64(int(n_bins)) / np.float64(r)), cutoff2_of(r_max)
    if not np.isfinite(scale) or scale <= 0 or not np.isfinite(rmax2):
        raise ValueError(f"r_max = {r_max} leaves no finite bin width and square in fp32")
    return scale


def n_pairs_of(C: int) -> int:
    return int(C) * (int(C) + 1) // 2


def pair_index(a, b, C: int):
    """The index of the unordered class pair ``{a, b}`` among the ``C (C + 1) / 2``: ``lo * C - lo (lo - 1) / 2 + (hi - lo)``."""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo * int(C) - lo * (lo - 1) // 2 + (hi - lo)


def pair_names_of(class_names) -> List[str]:
    names = [str(v) for v in class_names]
    return [f"{names[a]}-{names[b]}" for a in range(len(names)) for b in range(a, len(names))]


def classes_of(z, sel, by="element") -> Tuple[np.ndarray, List[str]]:
    """``(cls [m] int32, class_names)`` for the selected atoms ``sel`` of the molecule ``z [n]``.  ``"element"``: the
    distinct elements of the selection in ascending Z; ``"none"``: one class; an int array ``[n]``: the caller's label for
    every atom of the molecule, densified in ascending order.  ``ValueError`` naming the classes when there are more than
    the kernel holds: pass ``"none"`` or coarser labels."""
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    s = np.asarray(sel, dtype=np.int64).reshape(-1)
    if isinstance(by, str):
        if by == "none":
            return np.zeros(s.shape[0], dtype=np.int32), ["all"]
        if by != "element":
            raise ValueError("classes must be 'element', 'none' or an int array with a label for every atom")
        values, dense = np.unique(zz[s], return_inverse=True)
        names = [SYMBOLS.get(int(v), f"Z{int(v)}") for v in values]
    else:
        labels = np.asarray(by).reshape(-1)
        if labels.shape[0] != zz.shape[0] or labels.dtype.kind not in "iu":
            raise ValueError(f"class labels must be an int array with one label for each of the {zz.shape[0]} atoms")
        values, dense = np.unique(labels[s], return_inverse=True)
        names = [str(int(v)) for v in values]
    most = limits()["classes"]
    if len(names) > most:
        raise ValueError(f"the selection has {len(names)} classes ({', '.join(names)}), the kernel holds {most}: pass "
                         f"classes='none' or coarser labels")
    return np.ascontiguousarray(dense.reshape(-1).astype(np.int32)), names


def _labels(classes, z, bonds, mapping):
    """``"bead"`` as the label array of ``ensemble.groups_of``; everything else as it is."""
    if isinstance(classes, str) and classes == "bead":
        return groups_of(z, bonds, mapping, "bead")
    return classes


def _square(mask, m: int) -> np.ndarray:
    return ensemble.square_mask(mask, m, "excluded") | np.eye(m, dtype=bool)


# ----------------------------------------------------------------------------- the launches
def count_pairs(xyz, sel, cls, n_classes: int, excluded, r_max: float = 20.0, n_bins: int = 100, structures_per_launch: int = 4096,
                device="cuda") -> dict:
    """The launches behind ``pair_hist``, with every table the caller's own: ``sel [m]`` (unique atoms), ``cls [m]`` in
    ``[0, n_classes)`` and the SYMMETRIC bool mask ``excluded [m, m]`` in the order of ``sel`` (the diagonal is added).
    Returns the host arrays ``hist [P, n_bins]`` and ``beyond [P]`` int64, ``bad [S]`` bool, ``n_good`` and the fp32
    ``rmax2`` / ``scale`` the kernel took."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    if S >= 2 ** 31:
        raise ValueError("fewer than 2^31 structures")
    lim = limits()
    C, nb = int(n_classes), int(n_bins)
    if not 1 <= C <= lim["classes"]:
        raise ValueError(f"n_classes must be in 1..{lim['classes']}, got {n_classes}")
    if not 1 <= nb <= lim["bins"]:
        raise ValueError(f"n_bins must be in 1..{lim['bins']}, got {n_bins}")
    scale, rmax2 = scale_of(r_max, nb), cutoff2_of(r_max)
    if not 1 <= int(structures_per_launch) <= lim["structures"]:
        raise ValueError(f"structures_per_launch must be in 1..{lim['structures']}, got {structures_per_launch}")
    table = ensemble.selection(sel, n, purpose="count")
    m = int(table.shape[0])
    if m > lim["atoms"]:
        raise ValueError(f"the selection lists {m} atoms (the kernel holds {lim['atoms']})")
    c32 = np.asarray(cls).reshape(-1)
    if c32.shape[0] != m or c32.dtype.kind not in "iu" or (c32 < 0).any() or (c32 >= C).any():
        raise ValueError(f"cls must be {m} integers in [0, {C})")
    c32 = np.ascontiguousarray(c32.astype(np.int32))
    ex = _square(excluded, m)
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(structures_per_launch, lim["structures"], 16 * m)
    P = n_pairs_of(C)
    out = {"hist": torch.zeros(P, nb, dtype=torch.int64, device=dev), "beyond": torch.zeros(P, dtype=torch.int64, device=dev),
           "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if S:
        lib = _lib.load()
        d_sel, d_cls = torch.from_numpy(table).to(dev), torch.from_numpy(c32).to(dev)
        d_ex = torch.from_numpy(pack_mask(ex).view(np.int32)).to(dev)
        need = int(lib.cgv_pairdist_workspace_bytes(min(M, S), m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        for start, chunk in ensemble.chunks(x, M, dev):
            k = int(chunk.shape[0])
            _lib.call("cgv_pairdist_counts", _lib.ptr(chunk), _lib.ptr(d_sel), _lib.ptr(d_cls), _lib.ptr(d_ex), k, n, m, C, nb,
                      float(rmax2), float(scale), _lib.ptr(out["hist"]), _lib.ptr(out["beyond"]), _lib.ptr(out["bad"][start:start + k]),
                      _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), tag="pairdist_counts")
    hist, beyond, bad = read_back([out["hist"], out["beyond"], out["bad"]])
    return {"hist": hist, "beyond": beyond, "bad": bad.astype(bool), "n_good": int(S - int(bad.sum())), "rmax2": rmax2, "scale": scale,
            "r_max": float(np.float32(r_max)), "n_bins": nb, "n_classes": C}


def pair_hist(xyz, z, bonds, atoms="heavy", classes="element", r_max: float = 20.0, n_bins: int = 100, exclude: int = 3,
              structures_per_launch: int = 4096, device="cuda") -> dict:
    """The pair-distance histograms of the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device
    tensor decides the device) of the molecule ``z [n]`` / ``bonds [Eb,2]`` over ``select_atoms(z, atoms)``, by class
    (``classes_of``: ``"element"``, ``"none"`` or a label for every atom), without the pairs at most ``exclude`` bonds
    apart.  Host arrays:

      hist [P, n_bins] int64     the in-range pairs i < j of the good structures by class pair (``pair_index``) and bin
      beyond [P] int64           the pairs at ``r_max`` or farther
      bad [S] bool, n_good       structures with a non-finite selected coordinate, and the number of the others
      sel [m], cls [m], class_names [C], pair_names [P], excluded [m, m] bool     the tables used
      rmax2, scale               what the kernel took (fp32); r_max (as fp32 holds it), n_bins, n_classes, exclude

    For every class pair ``hist[p].sum() + beyond[p] == n_good * (its non-excluded pairs i < j)``.  The structures go
    through in launches of ``structures_per_launch``; the sums stay on the device; ONE read-back.  Everything that can be
    refused is a ``ValueError`` before any launch."""
    x = structures(xyz)
    n = int(x.shape[1])
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    if zz.shape[0] != n:
        raise ValueError(f"z lists {zz.shape[0]} atoms, the structures have {n}")
    lim = limits()
    if not 1 <= int(n_bins) <= lim["bins"]:
        raise ValueError(f"n_bins must be in 1..{lim['bins']}, got {n_bins}")
    scale_of(r_max, n_bins)
    table = ensemble.selection(select_atoms(zz, atoms), n, purpose="count")
    m = int(table.shape[0])
    if m > lim["atoms"]:
        raise ValueError(f"the selection lists {m} atoms (the kernel holds {lim['atoms']})")
    cls, names = classes_of(zz, table, classes)
    ex = excluded_pairs(bonds, n, table, exclude)
    res = count_pairs(x, table, cls, len(names), ex, r_max, n_bins, structures_per_launch, device)
    res.update(sel=table, cls=cls, class_names=names, pair_names=pair_names_of(names), excluded=ex, exclude=int(exclude))
    return res


# ----------------------------------------------------------------------------- host statistics
def distribution(res: dict) -> dict:
    """From the integers, fp64: ``r [n_bins]`` (bin centres), ``width``, and per class pair (rows ``0 .. P-1``) and for all
    pairs together (key suffix ``_all``): ``p [P, n_bins]`` / ``p_all [n_bins]`` -- P(r) normalised over the in-range pairs,
    NaN where there are none --, ``mean`` / ``mean_all`` (the mean distance of the in-range pairs from the bin centres),
    ``beyond`` / ``beyond_all`` (the share of the counted pairs at ``r_max`` or farther) and ``n`` / ``n_all`` (in-range
    pairs)."""
    hist = np.asarray(res["hist"], dtype=np.int64)
    beyond = np.asarray(res["beyond"], dtype=np.int64).reshape(-1)
    nb = int(hist.shape[1])
    width = float(res["r_max"]) / nb
    r = (np.arange(nb, dtype=np.float64) + 0.5) * width

    def of(h, b):
        h = h.astype(np.float64)
        n_in = h.sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(n_in[..., None] > 0, h / n_in[..., None], np.nan)
            mean = np.where(n_in > 0, (h * r).sum(-1) / n_in, np.nan)
            share = np.where(n_in + b > 0, b / (n_in + b), np.nan)
        return p, mean, share
    p, mean, share = of(hist, beyond.astype(np.float64))
    p_all, mean_all, share_all = of(hist.sum(0), float(beyond.sum()))
    return {"r": r, "width": width, "p": p, "mean": mean, "beyond": share, "n": hist.sum(-1), "p_all": p_all, "mean_all": float(mean_all),
            "beyond_all": float(share_all), "n_all": int(hist.sum())}


def wasserstein1(counts_a, counts_b, width: float) -> Optional[float]:
    """The first Wasserstein distance of two histograms over the same bins of ``width``: the area between their cumulative
    distributions, from integer cumulative counts (exact until the one division).  ``None`` when either is empty."""
    a = [int(v) for v in np.asarray(counts_a).reshape(-1)]
    b = [int(v) for v in np.asarray(counts_b).reshape(-1)]
    if len(a) != len(b):
        raise ValueError("the histograms have different bins")
    na, nb = sum(a), sum(b)
    if na <= 0 or nb <= 0:
        return None
    ca = cb = area = 0
    for va, vb in zip(a, b):
        ca, cb = ca + va, cb + vb
        area += abs(ca * nb - cb * na)
    return float(width) * (area / (na * nb))


def _opt(v):
    return None if v is None or not np.isfinite(v) else float(v)


def _block(he, be, ho, bo, hg, bg, r, width) -> dict:
    """One class pair (or all pairs): the reference (even + odd) against the generated set."""
    hr, br = he + ho, int(be) + int(bo)
    n_r, n_g = int(hr.sum()), int(hg.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        pr = hr / float(n_r) if n_r else None
        pg = hg / float(n_g) if n_g else None
    worst = None
    if pr is not None and pg is not None:
        k = int(np.argmax(np.abs(pg - pr)))
        worst = {"value": float(pg[k] - pr[k]), "bin": k, "r": float(r[k])}
    return {"n_pairs_ref": n_r, "n_pairs_gen": n_g, "hist_ref": [int(v) for v in hr], "hist_gen": [int(v) for v in hg],
            "jsd": js_divergence(hr, hg), "floor": js_divergence(he, ho), "w1": wasserstein1(hr, hg, width),
            "w1_floor": wasserstein1(he, ho, width), "max_diff": worst,
            "mean_ref": None if pr is None else float((pr * r).sum()), "mean_gen": None if pg is None else float((pg * r).sum()),
            "beyond_ref": _opt(br / float(n_r + br)) if n_r + br else None, "beyond_gen": _opt(int(bg) / float(n_g + int(bg))) if n_g + int(bg) else None}


BLOCK_SHORT = ("jsd", "floor", "w1", "w1_floor", "max_diff", "mean_ref", "mean_gen", "beyond_ref", "beyond_gen")


def compare_from_counts(even: dict, odd: dict, gen: dict, params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from three results of ``pair_hist`` -- the even reference frames, the odd ones and the
    generated structures, counted with the same tables -- pure host.  Keys: ``PAIRDIST_STATS_KEYS``; see ``compare``."""
    hists = [np.asarray(w["hist"], dtype=np.int64) for w in (even, odd, gen)]
    if not (hists[0].shape == hists[1].shape == hists[2].shape) or len({float(w["r_max"]) for w in (even, odd, gen)}) != 1:
        raise ValueError("the three results have different bins or class pairs")
    beys = [np.asarray(w["beyond"], dtype=np.int64).reshape(-1) for w in (even, odd, gen)]
    nb = int(hists[0].shape[1])
    width = float(gen["r_max"]) / nb
    r = (np.arange(nb, dtype=np.float64) + 0.5) * width
    names = list(gen["pair_names"])
    pairs = {name: _block(hists[0][p], beys[0][p], hists[1][p], beys[1][p], hists[2][p], beys[2][p], r, width) for p, name in enumerate(names)}
    overall = _block(hists[0].sum(0), beys[0].sum(), hists[1].sum(0), beys[1].sum(), hists[2].sum(0), beys[2].sum(), r, width)
    return {**ensemble.set_sizes(even, odd, gen), "params": dict(params or {}), "n_atoms": int(np.asarray(gen["sel"]).shape[0]),
            "class_names": [str(v) for v in gen["class_names"]], "pair_names": names, "r": r.tolist(), "overall": overall, "pairs": pairs,
            "floor": {"jsd": overall["floor"], "w1": overall["w1_floor"]}}


def compare(ref_xyz, gen_xyz, z, bonds, atoms="heavy", classes="element", r_max: float = 20.0, n_bins: int = 100, exclude: int = 3,
            mapping=None, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Generated structures ``gen_xyz [S,n,3]`` against the reference frames ``ref_xyz [T,n,3]`` (at least two).  ``classes``:
    ``"element"``, ``"none"``, ``"bead"`` (needs ``mapping``) or a label for every atom.  The reference's even and odd frames
    are counted apart: what the halves differ by is the floor of every divergence.  Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      params       atoms (the selection), classes, r_max, n_bins, exclude, and rmax2 / scale as the kernel took them
      n_atoms, class_names, pair_names, r (bin centres in Angstrom)
      overall      all pairs together: {n_pairs_ref, n_pairs_gen (in-range pairs), hist_ref, hist_gen, jsd (base 2, of P(r)
                   normalised over the in-range pairs), floor (even against odd), w1 (first Wasserstein distance in
                   Angstrom, from the cumulative histograms), w1_floor, max_diff {value, bin, r}: the largest per-bin
                   difference gen - ref of P(r) and where it is, mean_ref, mean_gen, beyond_ref, beyond_gen: the share of
                   the counted pairs at r_max or farther}; ``None`` where a set has no in-range pair
      pairs        {pair name: the same block} for every class pair
      floor        {jsd, w1} of ``overall``
    """
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z)
    labels = _labels(classes, z, bonds, mapping)
    kw = dict(atoms=atoms, classes=labels, r_max=r_max, n_bins=n_bins, exclude=exclude, structures_per_launch=structures_per_launch,
              device=device)
    even, odd, got = (pair_hist(s, z, bonds, **kw) for s in (ref[0::2], ref[1::2], gen))
    params = {"atoms": [int(i) for i in got["sel"]], "classes": classes if isinstance(classes, str) else "labels", "r_max": got["r_max"],
              "n_bins": int(n_bins), "exclude": int(exclude), "rmax2": float(got["rmax2"]), "scale": float(got["scale"])}
    return compare_from_counts(even, odd, got, params=params)


PAIRDIST_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "n_atoms", "class_names", "pair_names", "r", "overall",
                       "pairs", "floor")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"pairdist_stats"`` in its JSON summary line: no histograms, no bin centres."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_atoms", "class_names", "pair_names", "floor")}
    short["overall"] = {k: stats["overall"][k] for k in BLOCK_SHORT}
    short["pairs"] = {name: {k: block[k] for k in ("jsd", "floor", "w1", "w1_floor")} for name, block in stats["pairs"].items()}
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.pairdist",
                                "pair-distance distributions P(r) of generated structures against those of the reference frames",
                                top_help="npz with z and bonds (and mapping for -pd_classes bead); default: those of -ref")
    p.add_argument("-pd_atoms", choices=("heavy", "all"), default="heavy", help="the atoms whose pairs are counted (heavy)")
    p.add_argument("-pd_classes", choices=("element", "none", "bead"), default="element",
                   help="one histogram per pair of elements, one for all pairs, or one per pair of beads (element)")
    p.add_argument("-pd_rmax", type=float, default=20.0, help="the largest distance binned, in Angstrom (20)")
    p.add_argument("-pd_bins", type=int, default=100, help="equal bins on [0, -pd_rmax) (100)")
    p.add_argument("-pd_exclude", type=int, default=3, help="pairs at most this many bonds apart are left out (3)")
    return compare_cli.finish_parser(p, "pairdist_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, ``classes``, ``mapping``, with everything that
    can be refused without a device refused here (``SystemExit``)."""
    if not (math.isfinite(args.pd_rmax) and args.pd_rmax > 0):
        raise SystemExit("-pd_rmax must be a finite length > 0 in Angstrom")
    if args.pd_exclude < 0:
        raise SystemExit("-pd_exclude must be >= 0")
    lim = limits()
    if not 1 <= args.pd_bins <= lim["bins"]:
        raise SystemExit(f"-pd_bins must be in 1..{lim['bins']}")
    need = ("z", "bonds", "mapping") if args.pd_classes == "bead" else ("z", "bonds")
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args, need)
    bonds = np.asarray(top["bonds"])
    mapping = np.asarray(top["mapping"]) if args.pd_classes == "bead" else None
    with compare_cli.refusing():
        scale_of(args.pd_rmax, args.pd_bins)
        sel = select_atoms(z, args.pd_atoms)
        m = int(sel.shape[0])
        if m == 0:
            raise ValueError("the selection is empty (m = 0): no atoms to count")
        if m > lim["atoms"]:
            raise ValueError(f"the selection lists {m} atoms (the kernel holds {lim['atoms']})")
        classes_of(z, sel, _labels(args.pd_classes, z, bonds, mapping))
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": bonds, "classes": args.pd_classes, "mapping": mapping}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    with compare_cli.refusing():
        stats = compare(inp["ref_xyz"], inp["gen_xyz"], inp["z"], inp["bonds"], atoms=args.pd_atoms, classes=inp["classes"],
                        r_max=args.pd_rmax, n_bins=args.pd_bins, exclude=args.pd_exclude, mapping=inp["mapping"], device=args.device)
    compare_cli.finish("pairdist", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
