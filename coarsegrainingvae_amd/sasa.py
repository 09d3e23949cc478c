"""Which atoms of an ensemble face the solvent: the solvent-accessible surface area (SASA, Shrake-Rupley) of every atom
of every structure, counted on the device (K23, ``cgv_sasa_counts``; ``csrc/sasa.hip``), and whether generated structures
expose what the data exposes.

None of the other analyses sees the surface: ``evaluate`` (the bond graph), ``distributions`` (internal coordinates),
``tica`` (slow modes), ``coverage`` (RMSD), ``contacts`` (pairs within a cutoff, Rg), ``flexibility`` (per-atom motion) and
``density`` (free-energy surfaces) are all clean for an ensemble that buries the polar groups the simulation exposes, or
turns a hydrophobic side chain out into the solvent.

The selected atoms are the molecule: the atoms probed and the only occluders.  Atom ``i`` has the inflated radius
``r_i = fp32(fp32(R_i) + fp32(probe))`` and ``P`` points ``c_i + r_i * u_k`` (per component, the product rounded, then the
sum) with ``u`` the golden-spiral points of ``sphere_points``.  A point is *buried* iff some selected position ``j != i``
has ``(dx*dx + dy*dy) + dz*dz < r_j * r_j`` for its difference to ``c_j`` -- fp32, every operation rounded on its own, as
``csrc/sq_dist.h`` -- and ``count[s, i]`` is the number of points that are not: an integer a ``numpy.float32`` restatement
reproduces exactly.  Areas are host fp64 arithmetic on these integers, ``4 pi r_i^2 count / P``: no floating-point result
leaves the device, and two calls give the same bits.  A structure with a non-finite selected coordinate is *bad*: its rows
are ``-1``, it is in no sum.  Lengths in Angstrom.

    python -m coarsegrainingvae_amd.sasa -gen samples.npz -ref traj.npz [-top top.npz] [-sasa_atoms all|heavy]
        [-sasa_probe 1.4] [-sasa_points 256] [-sasa_groups none|bead|residue] [-out sasa_stats.json]

``-gen``: the ``xyz [T, K, n, 3]`` (or ``[S, n, 3]``) that ``backmap -out`` writes; ``-ref``: a trajectory file with
``xyz [T, n, 3]``; ``z``, ``bonds`` and (for ``-sasa_groups bead``) ``mapping`` come from ``-top``, else from ``-ref``.
The full statistics of ``compare`` go to ``-out``, one JSON line with ``"sasa_stats": summary_of(...)`` to stdout.
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .ensemble import check_sets, device_of, groups_of, read_back, scalar_block, select_atoms, structures

BONDI_RADII = {1: 1.20, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.80, 16: 1.80, 17: 1.75}   # by atomic number (Bondi 1964)
POLARITY = ("apolar", "polar")         # what the labels of ``polarity`` mean


def limits() -> Dict[str, int]:
    return ensemble.limits("sasa", ("structures", "atoms", "points", "classes"))


def sphere_points(n_points: int) -> np.ndarray:
    """``u [P, 3]`` fp32: the golden spiral, built in fp64 and rounded once.  ``z_k = 1 - (2k + 1) / P`` (strictly
    descending), ``rho = sqrt(1 - z_k^2)``, ``phi = k pi (3 - sqrt 5)``, ``u_k = (rho cos phi, rho sin phi, z_k)``."""
    P = int(n_points)
    if P < 1:
        raise ValueError(f"at least one sphere point is needed, got {n_points}")
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    rho = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.ascontiguousarray(np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1).astype(np.float32))


def radii_of(z, sel, radii: Optional[dict] = None) -> np.ndarray:
    """The van der Waals radius of every selected atom, fp64 ``[m]``: ``BONDI_RADII`` by atomic number, the caller's
    ``radii = {z: R}`` first.  ``ValueError`` naming an element that is in neither, and for a radius that is no finite
    length >= 0."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    table = dict(BONDI_RADII)
    for key, value in (radii or {}).items():
        if not np.isfinite(value) or value < 0:
            raise ValueError(f"the radius of element {int(key)} must be a finite length >= 0, got {value}")
        table[int(key)] = float(value)
    picked = z[np.asarray(sel, dtype=np.int64).reshape(-1)]
    missing = sorted(set(picked.tolist()) - set(table))
    if missing:
        raise ValueError(f"no radius for the element with atomic number {missing[0]}: BONDI_RADII has "
                         f"{sorted(BONDI_RADII)}; pass radii={{{missing[0]}: R}}")
    return np.array([table[a] for a in picked.tolist()], dtype=np.float64)


def inflated(R, probe: float = 1.4) -> np.ndarray:
    """``r = fp32(fp32(R) + fp32(probe))``, what the kernel takes."""
    p = np.float32(probe)
    if not np.isfinite(p) or p < 0:
        raise ValueError(f"the probe radius must be a finite length >= 0, got {probe}")
    return np.ascontiguousarray(np.asarray(R, dtype=np.float32).reshape(-1) + p)


def device_classes(classes, r: np.ndarray):
    """The classes the device sums over: the distinct pairs (caller's label, inflated radius), in ascending order, so
    that the area of a class is one exact integer times ``4 pi r^2 / P``.  Returns ``(cls [m] int32, class_ids [C]
    int64: the label of a device class, class_r [C] fp32: its radius)``."""
    m = r.shape[0]
    lab = np.zeros(m, dtype=np.int64) if classes is None else np.asarray(classes).astype(np.int64).reshape(-1)
    if lab.shape[0] != m:
        raise ValueError(f"classes lists {lab.shape[0]} atoms, the selection {m}")
    pairs = np.stack([lab.astype(np.float64), r.astype(np.float64)], axis=1)
    uniq, cls = np.unique(pairs, axis=0, return_inverse=True)
    return np.ascontiguousarray(cls.reshape(-1).astype(np.int32)), uniq[:, 0].astype(np.int64), uniq[:, 1].astype(np.float32)


# ----------------------------------------------------------------------------- the launches
def sasa_counts(xyz, z, sel=None, probe: float = 1.4, n_points: int = 256, radii: Optional[dict] = None, classes=None,
                per_atom: bool = False, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Exposed sphere points of the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device
    tensor decides the device) of the molecule ``z [n]`` over the atoms ``sel [m]`` (any order; default: all) with the
    radii of ``radii_of`` inflated by ``probe``.  ``classes [m]``: a label per selected atom (default: one class).
    Host arrays:

      class_counts [S,C] int64   exposed points of structure s over the atoms of device class c (-1: bad structure)
      class_ids [C], class_r [C] the caller's label and the fp32 radius of a device class (``device_classes``)
      atom_sum, atom_sumsq [m] int64   sums of count and count^2 of an atom over the good structures
      n_good                     structures that are not bad (the denominator of a mean)
      bad [S] bool, r [m] fp32 the inflated radii, n_points
      counts [S,m] int32         with ``per_atom`` only: count[s, i] (-1: bad structure)

    The structures go through in launches of ``structures_per_launch``; the sums are kept on the device in int64; ONE
    read-back.  Everything ``ensemble.selection`` refuses, an unknown element and the limits (``limits()``) are refused
    before any launch."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    lim = limits()
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    if zz.shape[0] != n:
        raise ValueError(f"z lists {zz.shape[0]} atoms, a structure has {n}")
    table = ensemble.selection(sel, n, purpose="probe the surface of")
    m, P = int(table.shape[0]), int(n_points)
    if m > lim["atoms"]:
        raise ValueError(f"the selection lists {m} atoms (the kernel holds {lim['atoms']})")
    if not 1 <= P <= lim["points"]:
        raise ValueError(f"n_points must be 1 .. {lim['points']}, got {n_points}")
    r = inflated(radii_of(zz, table, radii), probe)
    cls, class_ids, class_r = device_classes(classes, r)
    C = int(class_ids.shape[0])
    if C > lim["classes"]:
        raise ValueError(f"{C} distinct (class, radius) pairs (the kernel holds {lim['classes']})")
    u = sphere_points(P)
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(structures_per_launch, lim["structures"], 16 * m + 4)
    out = {"class_counts": torch.zeros(S, C, dtype=torch.int32, device=dev), "bad": torch.zeros(S, dtype=torch.int32, device=dev),
           "atom_sum": torch.zeros(m, dtype=torch.int64, device=dev), "atom_sumsq": torch.zeros(m, dtype=torch.int64, device=dev)}
    if per_atom:
        out["counts"] = torch.zeros(S, m, dtype=torch.int32, device=dev)
    if S:
        lib = _lib.load()
        d_sel, d_r, d_u, d_cls = (torch.from_numpy(a).to(dev) for a in (table, r, u, cls))
        ws = ensemble.workspace(int(lib.cgv_sasa_workspace_bytes(min(M, S), m, P)), dev)
        for start, chunk in ensemble.chunks(x, M, dev):
            k = int(chunk.shape[0])
            _lib.call("cgv_sasa_counts", _lib.ptr(chunk), _lib.ptr(d_sel), _lib.ptr(d_r), _lib.ptr(d_u), _lib.ptr(d_cls), k, n, m, P, C,
                      _lib.ptr(out["counts"][start:start + k]) if per_atom else None, _lib.ptr(out["class_counts"][start:start + k]),
                      _lib.ptr(out["atom_sum"]), _lib.ptr(out["atom_sumsq"]), _lib.ptr(out["bad"][start:start + k]),
                      _lib.ptr(ws), ws.numel() * 8, _lib.stream_ptr(), tag="sasa_counts")
    keys = list(out)
    host = dict(zip(keys, read_back([out[k] for k in keys])))
    res = {"class_counts": host["class_counts"].astype(np.int64), "class_ids": class_ids, "class_r": class_r,
           "atom_sum": host["atom_sum"], "atom_sumsq": host["atom_sumsq"], "n_good": int(S - int(host["bad"].sum())),
           "bad": host["bad"].astype(bool), "r": r, "n_points": P}
    if per_atom:
        res["counts"] = host["counts"]
    return res


# ----------------------------------------------------------------------------- host statistics
def polarity(z) -> np.ndarray:
    """A label per atom, ``[n]`` int64: 0 (``POLARITY[0]``, apolar) for carbon and sulfur, 1 (polar) for everything else."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    return np.where((z == 6) | (z == 16), 0, 1).astype(np.int64)


def areas(res: dict) -> dict:
    """Areas in square Angstrom from a result of ``sasa_counts``, fp64 on its integers with ``r`` widened: an atom's area
    in a structure is ``4 pi r_i^2 count / P``.

      total [S]              the area of a structure (NaN: bad structure)
      labels [L], by_class [S, L]   the distinct caller labels, ascending, and the area of the atoms of each
      mean [m], std [m]      per atom over the good structures (NaN without one); std is the population's
    """
    P = float(res["n_points"])
    unit = 4.0 * math.pi * np.asarray(res["class_r"], dtype=np.float64) ** 2 / P            # [C] area of one point
    cc = np.asarray(res["class_counts"], dtype=np.float64)
    bad = np.asarray(res["bad"], dtype=bool)
    labels, dense = np.unique(np.asarray(res["class_ids"]), return_inverse=True)
    by_class = np.zeros((cc.shape[0], labels.shape[0]), dtype=np.float64)
    for c in range(cc.shape[1]):
        by_class[:, dense[c]] += cc[:, c] * unit[c]
    by_class[bad] = np.nan
    total = (cc * unit[None, :]).sum(axis=1)
    total[bad] = np.nan
    point = 4.0 * math.pi * np.asarray(res["r"], dtype=np.float64) ** 2 / P                 # [m]
    n = int(res["n_good"])
    if n > 0:
        mean = np.asarray(res["atom_sum"], dtype=np.float64) / n
        var = np.maximum(np.asarray(res["atom_sumsq"], dtype=np.float64) / n - mean * mean, 0.0)
        mean, std = point * mean, point * np.sqrt(var)
    else:
        mean = std = np.full(point.shape, np.nan)
    return {"total": total, "labels": labels, "by_class": by_class, "mean": mean, "std": std}


def _merged(a: dict, b: dict) -> dict:
    """The reference from its halves: integer sums."""
    return {**a, "atom_sum": a["atom_sum"] + b["atom_sum"], "atom_sumsq": a["atom_sumsq"] + b["atom_sumsq"],
            "n_good": a["n_good"] + b["n_good"], "class_counts": np.concatenate([a["class_counts"], b["class_counts"]]),
            "bad": np.concatenate([a["bad"], b["bad"]])}


def _profile(res: dict, dense, G: int):
    if res["n_good"] <= 0:
        return None
    mean = areas(res)["mean"]
    return mean if dense is None else np.bincount(dense, weights=mean, minlength=G)


def _dev(p, q):
    if p is None or q is None:
        return None, None
    d = p - q
    return float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())


def _scalars(res: dict) -> dict:
    """Per good structure: the total area, the area of the apolar atoms and its share (a structure without surface has
    no share and is left out of that one)."""
    a = areas(res)
    good = ~np.asarray(res["bad"], dtype=bool)
    total = a["total"][good]
    at = np.flatnonzero(a["labels"] == 0)
    apolar = a["by_class"][good][:, at[0]] if at.size else np.zeros_like(total)
    return {"total": total, "apolar": apolar, "apolar_fraction": apolar[total > 0] / total[total > 0]}


def compare_from_counts(even: dict, odd: dict, gen: dict, labels=None, groups=None, n_bins: int = 20,
                        params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from three results of ``sasa_counts`` -- the even reference frames, the odd ones
    and the generated structures, all counted over the same selection with ``classes = polarity(z)[sel]`` -- pure host.
    ``labels [m]``: what a selected atom is called (its index in the molecule; default ``0..m-1``); ``groups [m]``: a
    group label per selected atom, whose areas are then summed (beads, residues).  Bad structures are in no
    denominator.  Keys: ``SASA_STATS_KEYS``; see ``compare``."""
    m = int(np.asarray(gen["r"]).shape[0])
    dense, G = None, m
    rows = list(range(m)) if labels is None else [int(v) for v in labels]
    if groups is not None:
        g = np.asarray(groups, dtype=np.int64).reshape(-1)
        if g.shape[0] != m:
            raise ValueError(f"groups lists {g.shape[0]} atoms, the selection {m}")
        ids, dense = np.unique(g, return_inverse=True)
        dense, G, rows = dense.reshape(-1), int(ids.shape[0]), [int(v) for v in ids]
    ref = _merged(even, odd)
    p_ref, p_gen, p_even, p_odd = (_profile(r, dense, G) for r in (ref, gen, even, odd))
    rmse, max_dev = _dev(p_ref, p_gen)
    f_rmse, f_max = _dev(p_even, p_odd)
    top = []
    if rmse is not None:
        for k in np.argsort(-np.abs(p_ref - p_gen), kind="stable")[:10]:
            top.append({"i": rows[int(k)], "mean_ref": float(p_ref[k]), "mean_gen": float(p_gen[k])})
    se, so, sg = _scalars(even), _scalars(odd), _scalars(gen)
    blocks = {}
    for key in ("total", "apolar", "apolar_fraction"):
        both = np.concatenate([se[key], so[key]])
        blocks[key] = None
        if both.size and sg[key].size:
            lo, hi = float(both.min()), float(both.max())
            pad = 0.1 * (hi - lo) if hi > lo else 0.05 * max(abs(hi), 1.0)       # the reference's range, 20 % wider
            blocks[key] = scalar_block(se[key], so[key], sg[key], lo - pad, hi + pad, n_bins)
    floor = {"profile_rmse": f_rmse, "profile_max_dev": f_max}
    floor.update({key + "_jsd": blocks[key]["floor"] if blocks[key] else None for key in blocks})
    return {**ensemble.set_sizes(even, odd, gen), "params": dict(params or {}, n_bins=int(n_bins)), "labels": rows,
            "mean_ref": None if p_ref is None else p_ref.tolist(), "mean_gen": None if p_gen is None else p_gen.tolist(),
            "profile_rmse": rmse, "profile_max_dev": max_dev, "floor": floor, "top_atoms": top, **blocks}


def compare(ref_xyz, gen_xyz, z, bonds, atoms="all", probe: float = 1.4, n_points: int = 256, groups=None, mapping=None,
            n_bins: int = 20, radii: Optional[dict] = None, structures_per_launch: int = 4096, device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) of the
    molecule ``z [n]`` / ``bonds [Eb,2]`` by the solvent-accessible surface of ``select_atoms(z, atoms)``.  ``groups``:
    ``None`` (a profile over atoms), ``"bead"`` (needs ``mapping``) or ``"residue"`` (``groups_of``).  The convention of
    ``contacts.compare``: the generated structures, the even and the odd frames of the reference are counted apart, the
    reference is the integer sum of its halves, and what the halves differ by is the ``floor`` every deviation is to be
    read against.  Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      params      atoms (the selection), probe, n_points, groups, radii (of the selected elements), n_bins
      labels      [G] the atom index or group label of an entry of the profiles
      mean_ref, mean_gen  [G] mean area over the good structures, square Angstrom (``None``: no good structure)
      profile_rmse, profile_max_dev   root mean square and largest |mean_ref - mean_gen| over the profile
      floor       {profile_rmse, profile_max_dev, total_jsd, apolar_jsd, apolar_fraction_jsd}: the same between the even
                  and the odd reference frames
      top_atoms   the ten entries of largest deviation: {i (label), mean_ref, mean_gen}
      total, apolar, apolar_fraction   {range, hist_ref, hist_gen ({counts [n_bins], under, over}), jsd, floor, mean_ref,
                  std_ref, mean_gen, std_gen} of a structure's area, the area of its apolar atoms (``polarity``: C, S)
                  and their share, on the reference's range widened by 20 %; ``None`` where a set has no good structure
    """
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z, groups=groups)
    sel = select_atoms(z, atoms)
    glab = None if groups is None else groups_of(z, bonds, mapping, groups)[sel]
    kw = dict(sel=sel, probe=probe, n_points=n_points, radii=radii, classes=polarity(z)[sel],
              structures_per_launch=structures_per_launch, device=device)
    even, odd, got = sasa_counts(ref[0::2], z, **kw), sasa_counts(ref[1::2], z, **kw), sasa_counts(gen, z, **kw)
    used = {int(a): float(R) for a, R in zip(z[sel].tolist(), radii_of(z, sel, radii).tolist())}
    params = {"atoms": [int(i) for i in sel], "probe": float(probe), "n_points": int(n_points), "groups": groups,
              "radii": {str(a): used[a] for a in sorted(used)}}
    return compare_from_counts(even, odd, got, labels=sel, groups=glab, n_bins=n_bins, params=params)


SASA_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "labels", "mean_ref", "mean_gen", "profile_rmse",
                   "profile_max_dev", "floor", "top_atoms", "total", "apolar", "apolar_fraction")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"sasa_stats"`` in its JSON summary line: no profiles, no histograms."""
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "profile_rmse", "profile_max_dev", "floor")}
    for k in ("total", "apolar", "apolar_fraction"):
        short[k] = ensemble.short_block(stats[k])
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.sasa",
                                "solvent-accessible surface area of generated structures against a reference",
                                top_help="npz with z and bonds (and mapping); default: those of -ref")
    p.add_argument("-sasa_atoms", choices=("all", "heavy"), default="all", help="the atoms that make up the molecule (all)")
    p.add_argument("-sasa_probe", type=float, default=1.4, help="probe radius in Angstrom (1.4)")
    p.add_argument("-sasa_points", type=int, default=256, help="sphere points per atom (256)")
    p.add_argument("-sasa_groups", choices=("none", "bead", "residue"), default="none",
                   help="profile over atoms (none), beads of the mapping, or residues of a peptide (none)")
    return compare_cli.finish_parser(p, "sasa_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, ``mapping`` (``None`` where absent), with
    everything that can be refused without a device refused here (``SystemExit``)."""
    if not args.sasa_probe >= 0 or not math.isfinite(args.sasa_probe):
        raise SystemExit("-sasa_probe must be a finite length >= 0 in Angstrom")
    if args.sasa_points < 1:
        raise SystemExit("-sasa_points must be at least 1")
    ref_xyz, gen_xyz, z, top, ref = compare_cli.read_sets(args)
    mapping = top.get("mapping", ref.get("mapping"))
    groups = None if args.sasa_groups == "none" else args.sasa_groups
    sel = select_atoms(z, args.sasa_atoms)
    if sel.shape[0] == 0:
        raise SystemExit(f"the topology has no {args.sasa_atoms} atoms")
    with compare_cli.refusing():
        radii_of(z, sel)
    if groups is not None:
        with compare_cli.refusing(f"-sasa_groups {groups}: "):
            groups_of(z, top["bonds"], mapping, groups)
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": np.asarray(top["bonds"]), "mapping": mapping, "groups": groups}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    with compare_cli.refusing():
        stats = compare(inp["ref_xyz"], inp["gen_xyz"], inp["z"], inp["bonds"], atoms=args.sasa_atoms, probe=args.sasa_probe,
                        n_points=args.sasa_points, groups=inp["groups"], mapping=inp["mapping"], device=args.device)
    compare_cli.finish("sasa", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
