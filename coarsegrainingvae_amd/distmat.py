"""Whether a generated ensemble has the data's DISTANCES: the mean and the fluctuation of every inter-atomic distance over
an ensemble -- the ``[m, m]`` mean-distance map, its standard-deviation map, their difference between two ensembles (the
ens_dRMS by which disordered-protein ensembles are compared: Lazar et al. 2020, Protein Ensemble Database) and the
superposition-free distance RMSD of every structure to a target map -- summed on the device for every pair and every
structure (K30, ``cgv_dist_moments``; ``csrc/dist_moments.hip``).

``contacts`` reduces a distance to one bit against a cutoff, ``pairdist`` pools all pairs of a kind into one histogram,
``lddt`` scores one sample against one frame, ``flexibility`` and ``pca`` need a superposition, which is ill-defined for
exactly the flexible molecules people backmap.  What is here is invariant under rotation and reflection, needs no
alignment choice, and localises a discrepancy to a pair of atoms, beads or residues.

Definition.  Over the selection ``sel [m]``, for a good structure ``s`` and a pair ``i < j`` that the mask does not leave
out, with a centre table ``center [m, m]`` fp32 (zeros when there is none), in fp32 with every operation rounded on its own
(``sqrtf`` correctly rounded):

    q = (dx*dx + dy*dy) + dz*dz  of x_i - x_j          d = sqrt(q)       e = d - center[i][j]       f = e * e
    sum_e[i][j] += rint(e * 2^20)        sum_e2[i][j] += rint(f * 2^20)        dev2[s] += rint(f * 2^12)         (int64)

A ``numpy.float32`` / ``numpy.rint`` restatement reproduces every integer exactly, no floating-point number leaves the
device, and two calls give the same bits however the structures are cut into launches.  Every statistic is host fp64 on
those integers.  A structure with a non-finite selected coordinate, or with a selected atom more than 512 A from the
centroid of the selection, is *bad* and enters no sum; with that, and centres in [0, 1024] A, at most 2^22 good structures
go into one pair of tables (``sum_e2 <= 2^62``), and more are refused.

    python -m coarsegrainingvae_amd.distmat -gen samples.npz -ref traj.npz [-top top.npz] [-dm_atoms heavy|all]
        [-dm_exclude 0] [-dm_groups none|bead|residue] [-maps maps.npz] [-out distmat_stats.json]

``z`` (and ``bonds`` for ``-dm_exclude`` > 0 or ``-dm_groups residue``, ``mapping`` for ``-dm_groups bead``) come from
``-top``, else from ``-ref``.  The full statistics of ``compare`` go to ``-out``, the four maps to ``-maps``, one JSON line
with ``"distmat_stats": summary_of(...)`` to stdout.
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble
from .contacts import excluded_pairs
from .ensemble import device_of, groups_of, pack_mask, read_back, select_atoms, structures

SCALE = 2.0 ** 20                      # sum_e, sum_e2
SCALE_DEV = 2.0 ** 12                  # dev2
MAX_CENTER = 1024.0                    # the kernel takes a centre in [0, MAX_CENTER] as it is
TOP = 5                                # the pairs named as the worst


def limits() -> Dict[str, int]:
    return ensemble.limits("dist_moments", ("structures", "atoms", "total"))


# ----------------------------------------------------------------------------- host: tables
def _counted(mask, m: int) -> np.ndarray:
    """``[m, m]`` bool, symmetric, False on the diagonal: the pairs that enter the sums."""
    if mask is None:
        return ~np.eye(m, dtype=bool)
    return ~(ensemble.square_mask(mask, m, "mask") | np.eye(m, dtype=bool))


def _center(center, counted: np.ndarray) -> Optional[np.ndarray]:
    """The centre table as the kernel takes it (fp32, zero where no pair counts), or ``ValueError``."""
    if center is None:
        return None
    m = counted.shape[0]
    c = np.asarray(center)
    if c.shape != (m, m) or c.dtype.kind != "f":
        raise ValueError(f"center must be a float array [{m}, {m}], got {c.dtype} {c.shape}")
    c = np.where(counted, c, 0).astype(np.float32)
    if not np.isfinite(c).all() or (c < 0).any() or (c > MAX_CENTER).any():
        raise ValueError(f"center must hold distances in [0, {MAX_CENTER:g}] A at every pair that counts")
    if not np.array_equal(c, c.T):
        raise ValueError("center must be symmetric")
    return np.ascontiguousarray(c)


# ----------------------------------------------------------------------------- the launches
def moments(xyz, sel, *, center=None, mask=None, into: Optional[dict] = None, chunk: int = 4096, device="cuda") -> dict:
    """The sums of the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device tensor decides the
    device) over the selection ``sel [m]`` (unique atoms, ``m >= 2``), against ``center [m, m]`` (symmetric distances in
    [0, 1024] A; ``None``: zeros), without the pairs of the SYMMETRIC bool ``mask [m, m]`` (True: left out).  Host arrays:

      sum_e, sum_e2 [m, m] int64     the sums of rint(e * 2^20) and rint(f * 2^20) over the good structures, symmetric,
                                     zero on the diagonal and at a masked pair
      dev2 [S] int64                 per structure the sum of rint(f * 2^12) over the pairs i < j that count; 0 for a bad one
      bad [S] bool, n_good           structures left out, and the number of the others
      sel, counted [m, m] bool, n_pairs (counted pairs i < j), center (fp32, or None)     the tables used

    The structures go through in launches of ``chunk`` (``ensemble.chunks``); the sums stay on the device; ONE read-back.
    ``into``: an earlier result with the same tables; its sums are added and its ``dev2`` / ``bad`` come first, so a long
    ensemble may be fed in pieces -- to the same integers as in one call.  The tables hold ``limits()["total"]`` = 2^22
    good structures: a call that could pass that (``into["n_good"]`` plus ALL structures of this call) is refused.
    Everything that can be refused is a ``ValueError`` before any launch."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    lim = limits()
    if not 1 <= int(chunk) <= lim["structures"]:
        raise ValueError(f"chunk must be in 1..{lim['structures']}, got {chunk}")
    table = ensemble.selection(sel, n, purpose="measure")
    m = int(table.shape[0])
    if m < 2:
        raise ValueError(f"the selection lists {m} atom: a distance needs two")
    if m > lim["atoms"]:
        raise ValueError(f"the selection lists {m} atoms (the kernel holds {lim['atoms']})")
    counted = _counted(mask, m)
    c32 = _center(center, counted)
    before = 0
    if into is not None:
        before = int(into["n_good"])
        same = np.array_equal(into["sel"], table) and np.array_equal(into["counted"], counted) and \
            ((into["center"] is None) == (c32 is None)) and (c32 is None or np.array_equal(into["center"], c32))
        if not same:
            raise ValueError("into was summed over another selection, mask or centre")
    if before + S > lim["total"]:
        raise ValueError(f"{before} + {S} structures: one pair of tables holds {lim['total']} (the fixed-point budget)")
    dev = device_of(x, device)
    M = ensemble.structures_per_launch(chunk, lim["structures"], 16 * m)
    out = {"sum_e": torch.zeros(m, m, dtype=torch.int64, device=dev), "sum_e2": torch.zeros(m, m, dtype=torch.int64, device=dev),
           "dev2": torch.zeros(S, dtype=torch.int64, device=dev), "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if S:
        lib = _lib.load()
        d_sel = torch.from_numpy(table).to(dev)
        d_mask = None if mask is None else torch.from_numpy(pack_mask(~counted).view(np.int32)).to(dev)
        d_ctr = None if c32 is None else torch.from_numpy(c32).to(dev)
        need = int(lib.cgv_dist_moments_workspace_bytes(min(M, S), m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        for start, part in ensemble.chunks(x, M, dev):
            k = int(part.shape[0])
            _lib.call("cgv_dist_moments", _lib.ptr(part), _lib.ptr(d_sel), _lib.ptr(d_mask), _lib.ptr(d_ctr), k, n, m,
                      _lib.ptr(out["sum_e"]), _lib.ptr(out["sum_e2"]), _lib.ptr(out["dev2"][start:start + k]),
                      _lib.ptr(out["bad"][start:start + k]), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), tag="dist_moments")
    sum_e, sum_e2, dev2, bad = read_back([out["sum_e"], out["sum_e2"], out["dev2"], out["bad"]])
    bad = bad.astype(bool)
    n_good = int(S - int(bad.sum()))
    if into is not None:
        sum_e, sum_e2 = sum_e + np.asarray(into["sum_e"], dtype=np.int64), sum_e2 + np.asarray(into["sum_e2"], dtype=np.int64)
        dev2, bad = np.concatenate([np.asarray(into["dev2"], dtype=np.int64), dev2]), np.concatenate([np.asarray(into["bad"], dtype=bool), bad])
        n_good += before
    return {"sum_e": sum_e, "sum_e2": sum_e2, "dev2": dev2, "bad": bad, "n_good": n_good, "sel": table, "counted": counted,
            "n_pairs": int(np.triu(counted, 1).sum()), "center": c32}


# ----------------------------------------------------------------------------- host: maps from the integers
def first_mean(first: dict) -> np.ndarray:
    """The fp64 mean-distance map of a pass with NO centre: ``sum_e / 2^20 / n_good`` (0 where no pair counts)."""
    if first["center"] is not None:
        raise ValueError("the first pass has no centre")
    n = int(first["n_good"])
    if n == 0:
        return np.zeros(first["sum_e"].shape, dtype=np.float64)
    return np.asarray(first["sum_e"], dtype=np.float64) / SCALE / n


def maps_of(second: dict) -> dict:
    """From the pass against ``center = float32(first mean)``, fp64: ``mean = center + sum_e / 2^20 / n``, ``var = sum_e2 /
    2^20 / n - (sum_e / 2^20 / n)^2`` clipped at 0, ``std``; NaN where no pair counts or no structure is good, 0 on the
    diagonal.  ``drmsd [S]``: ``sqrt(dev2 / 2^12 / n_pairs)`` of every structure to the CENTRE, NaN for a bad one."""
    n, counted = int(second["n_good"]), np.asarray(second["counted"], dtype=bool)
    m = counted.shape[0]
    ctr = np.zeros((m, m)) if second["center"] is None else np.asarray(second["center"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        me = np.asarray(second["sum_e"], dtype=np.float64) / SCALE / n if n else np.full((m, m), np.nan)
        m2 = np.asarray(second["sum_e2"], dtype=np.float64) / SCALE / n if n else np.full((m, m), np.nan)
    mean = np.where(counted, ctr + me, np.nan)
    var = np.where(counted, np.maximum(m2 - me * me, 0.0), np.nan)
    np.fill_diagonal(mean, 0.0), np.fill_diagonal(var, 0.0)
    return {"mean": mean, "std": np.sqrt(var), "drmsd": drmsd_of(second)}


def drmsd_of(rec: dict) -> np.ndarray:
    """``sqrt(dev2 / 2^12 / n_pairs)`` per structure, NaN for a bad one (and for all when no pair counts)."""
    p = int(rec["n_pairs"])
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.sqrt(np.asarray(rec["dev2"], dtype=np.float64) / SCALE_DEV / p) if p else np.full(len(rec["dev2"]), np.nan)
    return np.where(np.asarray(rec["bad"], dtype=bool), np.nan, v)


def mean_std(xyz, sel, mask=None, chunk: int = 4096, device="cuda") -> dict:
    """The mean-distance map and the standard-deviation map of the structures ``xyz [S,n,3]`` over ``sel [m]``, fp64
    ``mean [m, m]`` and ``std [m, m]`` (NaN at a masked pair, 0 on the diagonal), and ``drmsd [S]``: every structure's
    distance RMSD to that mean map as fp32 holds it (NaN for a bad one).  Also ``bad``, ``n_good``, ``n_pairs``, ``sel``,
    ``counted`` and ``center`` (fp32: the map the second pass was centred on).

    TWO passes.  The first has no centre: ``mean = sum_e / 2^20 / n_good``.  The second has ``center = float32(mean)``:
    ``mean = center + sum_e / ...`` and ``var = sum_e2 / ... - (sum_e / ...)^2``, clipped at 0.  One pass would take the
    variance as ``<d^2> - <d>^2``: at a 50 A distance that subtracts two numbers near 2500 whose fixed-point and fp32
    errors are those of 2500, and a fluctuation of 0.01 A (a variance of 1e-4) is lost in them.  Against the centre the
    deviations themselves are squared, ``<e>`` is nearly 0, and the cancellation is gone."""
    first = moments(xyz, sel, mask=mask, chunk=chunk, device=device)
    ctr = np.where(first["counted"], first_mean(first), 0.0).astype(np.float32)
    second = moments(xyz, sel, center=ctr, mask=mask, chunk=chunk, device=device)
    return {**maps_of(second), **{k: second[k] for k in ("bad", "n_good", "n_pairs", "sel", "counted", "center")}}


def drmsd(xyz, sel, target, mask=None, chunk: int = 4096, device="cuda") -> np.ndarray:
    """The distance RMSD of every structure of ``xyz [S,n,3]`` to the map ``target [m, m]`` (symmetric, distances in
    [0, 1024] A, taken as fp32): ``sqrt(dev2 / 2^12 / n_pairs)`` over the pairs the mask leaves, fp64 ``[S]``, NaN for a bad
    structure.  No superposition: a reflected structure has distance RMSD 0."""
    return drmsd_of(moments(xyz, sel, center=np.asarray(target, dtype=np.float32), mask=mask, chunk=chunk, device=device))


# ----------------------------------------------------------------------------- host statistics
def _rms(a) -> Optional[float]:
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else None


def _pearson(a, b) -> Optional[float]:
    if a.size < 2 or not (np.ptp(a) > 0 and np.ptp(b) > 0):
        return None
    return float(np.corrcoef(a, b)[0, 1])


def _worst(diff, ref, gen, ii, jj, names) -> list:
    order = np.argsort(-np.abs(diff), kind="stable")[:TOP]
    return [{"i": int(ii[k]), "j": int(jj[k]), "a": int(names[ii[k]]), "b": int(names[jj[k]]), "ref": float(ref[k]), "gen": float(gen[k]),
             "diff": float(diff[k])} for k in order]


def _level(even, odd, ref, gen, keep, names) -> dict:
    """The statistics of one level (atoms, or groups) from four pairs of maps ``(mean, std)`` and the pairs ``keep [k, k]``
    that count: ``i < j`` of them, finite in all maps."""
    keep = np.triu(keep, 1)
    for mean, std in (even, odd, ref, gen):
        keep = keep & np.isfinite(mean) & np.isfinite(std)
    ii, jj = np.nonzero(keep)
    of = lambda maps: (maps[0][ii, jj], maps[1][ii, jj])
    (me, se), (mo, so), (mr, sr), (mg, sg) = of(even), of(odd), of(ref), of(gen)
    return {"n_pairs": int(ii.shape[0]), "ens_drms": _rms(mg - mr), "fluct_drms": _rms(sg - sr), "std_corr": _pearson(sr, sg),
            "floor": {"ens_drms": _rms(me - mo), "fluct_drms": _rms(se - so), "std_corr": _pearson(se, so)},
            "worst_mean": _worst(mg - mr, mr, mg, ii, jj, names), "worst_std": _worst(sg - sr, sr, sg, ii, jj, names)}


def group_maps(mean, std, counted, labels):
    """The maps averaged over the counted atom pairs of every pair of groups: ``(mean [G, G], std [G, G], ids [G])`` for the
    ``G`` distinct labels in ascending order; NaN on the diagonal and where two groups share no counted pair."""
    ids, dense = np.unique(np.asarray(labels).reshape(-1), return_inverse=True)
    G = ids.shape[0]
    onehot = np.zeros((G, dense.shape[0]))
    onehot[dense.reshape(-1), np.arange(dense.shape[0])] = 1.0
    ok = np.asarray(counted, dtype=bool) & np.isfinite(mean) & np.isfinite(std)
    cnt = onehot @ ok.astype(np.float64) @ onehot.T
    out = []
    for a in (mean, std):
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(cnt > 0, (onehot @ np.where(ok, a, 0.0) @ onehot.T) / cnt, np.nan)
        np.fill_diagonal(g, np.nan)
        out.append(g)
    return out[0], out[1], ids


def compare_from_moments(even: dict, odd: dict, ref: dict, gen: dict, gen_drmsd, groups=None, params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from four results of ``mean_std`` (or anything with their ``mean``, ``std``, ``drmsd``,
    ``bad``, ``counted``, ``sel``) -- the even reference frames, the odd ones, all of them and the generated structures, over
    the same tables -- and ``gen_drmsd [S]``, the generated structures' distance RMSD to the reference's centre.  Pure host.
    ``groups [m]``: a label for every selected atom.  Keys: ``DISTMAT_STATS_KEYS``; see ``compare``."""
    counted, sel = np.asarray(gen["counted"], dtype=bool), np.asarray(gen["sel"])
    m = counted.shape[0]
    if any(np.asarray(r["mean"]).shape != (m, m) for r in (even, odd, ref)):
        raise ValueError("the four results have different selections")
    maps = [(np.asarray(r["mean"], dtype=np.float64), np.asarray(r["std"], dtype=np.float64)) for r in (even, odd, ref, gen)]
    stats = {**ensemble.set_sizes(even, odd, gen), "params": dict(params or {}), "n_atoms": m}
    stats.update(_level(*maps, counted, sel))
    finite = lambda v: np.asarray(v, dtype=np.float64)[np.isfinite(np.asarray(v, dtype=np.float64))]
    re_, ro_, g_ = finite(even["drmsd_ref"]), finite(odd["drmsd_ref"]), finite(gen_drmsd)
    top = max([float(v.max()) for v in (re_, ro_, g_) if v.size] + [0.0])
    stats["drmsd"] = ensemble.scalar_block(re_, ro_, g_, 0.0, top if top > 0 else 1.0, 50)
    stats["groups"] = None
    if groups is not None:
        labels = np.asarray(groups).reshape(-1)
        if labels.shape[0] != m or labels.dtype.kind not in "iu":
            raise ValueError(f"groups must be an int label for each of the {m} selected atoms")
        gm = [group_maps(mean, std, counted, labels) for mean, std in maps]
        ids = gm[0][2]
        G = ids.shape[0]
        stats["groups"] = {"n_groups": int(G), "ids": [int(v) for v in ids],
                           **_level(*[(a, b) for a, b, _ in gm], ~np.eye(G, dtype=bool), ids)}
    return stats


def compare(gen_xyz, ref_xyz, sel, *, mask=None, groups=None, chunk: int = 4096, device="cuda", params: Optional[dict] = None,
            maps: Optional[dict] = None) -> dict:
    """Generated structures ``gen_xyz [S,n,3]`` against the reference frames ``ref_xyz [T,n,3]`` (at least two) over the
    selection ``sel [m]``, without the pairs of ``mask``.  The reference's even and odd frames are also summed apart: what the
    halves differ by is the floor of every number.  Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen     structures, and those left out as bad
      params, n_atoms, n_pairs               the caller's ``params``; selected atoms; pairs i < j that count
      ens_drms       sqrt(mean over those pairs of (mean_gen - mean_ref)^2), in Angstrom
      fluct_drms     the same of the standard-deviation maps
      std_corr       the Pearson correlation of the two standard-deviation maps (None when one is constant)
      floor          {ens_drms, fluct_drms, std_corr} of the even against the odd reference frames
      worst_mean     the five pairs with the largest |mean_gen - mean_ref|: {i, j (places in sel), a, b (atoms), ref, gen, diff}
      worst_std      the same for the standard deviations
      drmsd          ``ensemble.scalar_block`` of the distance RMSD to the REFERENCE mean map, of the reference structures
                     (even / odd) and of the generated ones: histograms, jsd, floor, moments
      groups         with ``groups [m]`` (a label for every selected atom): {n_groups, ids, and n_pairs .. worst_std as
                     above (i, j: places in ids; a, b: labels)} of the maps averaged over the counted atom pairs of every
                     pair of groups; else None

    ``maps``: a dict that receives ``mean_ref``, ``std_ref``, ``mean_gen``, ``std_gen`` (what ``-maps`` writes)."""
    gen, ref = structures(gen_xyz), structures(ref_xyz)
    if int(ref.shape[0]) < 2:
        raise ValueError("at least two reference frames are needed (the floor compares the even with the odd ones)")
    if int(gen.shape[1]) != int(ref.shape[1]):
        raise ValueError(f"the frames have {int(ref.shape[1])} and {int(gen.shape[1])} atoms")
    kw = dict(mask=mask, chunk=chunk, device=device)
    whole = mean_std(ref, sel, **kw)
    even, odd, got = (mean_std(s, sel, **kw) for s in (ref[0::2], ref[1::2], gen))
    even["drmsd_ref"], odd["drmsd_ref"] = whole["drmsd"][0::2], whole["drmsd"][1::2]
    gen_drmsd = drmsd(gen, sel, whole["center"], **kw)
    if maps is not None:
        maps.update(mean_ref=whole["mean"], std_ref=whole["std"], mean_gen=got["mean"], std_gen=got["std"], sel=whole["sel"])
    return compare_from_moments(even, odd, whole, got, gen_drmsd, groups=groups, params=params)


LEVEL_KEYS = ("n_pairs", "ens_drms", "fluct_drms", "std_corr", "floor", "worst_mean", "worst_std")
DISTMAT_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "n_atoms") + LEVEL_KEYS + ("drmsd", "groups")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"distmat_stats"`` in its JSON summary line: no histograms, the single worst pairs."""
    def level(b):
        return {**{k: b[k] for k in ("n_pairs", "ens_drms", "fluct_drms", "std_corr", "floor")},
                "worst_mean": b["worst_mean"][:1], "worst_std": b["worst_std"][:1]}
    short = {k: stats[k] for k in ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_atoms")}
    short.update(level(stats))
    short["drmsd"] = ensemble.short_block(stats["drmsd"], ensemble.MOMENTS + ("floor",))
    short["groups"] = None if stats["groups"] is None else {"n_groups": stats["groups"]["n_groups"], **level(stats["groups"])}
    return short


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.distmat",
                                "mean and fluctuation of every inter-atomic distance of generated structures against the reference frames",
                                top_help="npz with z (bonds for -dm_exclude > 0 and -dm_groups residue, mapping for -dm_groups bead); "
                                         "default: those of -ref")
    p.add_argument("-dm_atoms", choices=("heavy", "all"), default="heavy", help="the atoms whose distances are taken (heavy)")
    p.add_argument("-dm_exclude", type=int, default=0, help="pairs at most this many bonds apart are left out (0: none)")
    p.add_argument("-dm_groups", choices=("none", "bead", "residue"), default="none",
                   help="also compare the maps averaged over the atom pairs of every pair of beads or residues (none)")
    p.add_argument("-maps", default=None, help="npz that receives mean_ref, std_ref, mean_gen, std_gen [m,m] and sel (not written)")
    return compare_cli.finish_parser(p, "distmat_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``sel``, ``mask``, ``groups``, with everything that can be
    refused without a device refused here (``SystemExit``)."""
    if args.dm_exclude < 0:
        raise SystemExit("-dm_exclude must be >= 0")
    need = ["z"]
    if args.dm_exclude > 0 or args.dm_groups == "residue":
        need.append("bonds")
    if args.dm_groups == "bead":
        need.append("mapping")
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args, tuple(need))
    with compare_cli.refusing():
        sel = select_atoms(z, args.dm_atoms)
        m = int(sel.shape[0])
        if m < 2:
            raise ValueError(f"the selection lists {m} atoms: a distance needs two")
        if m > limits()["atoms"]:
            raise ValueError(f"the selection lists {m} atoms (the kernel holds {limits()['atoms']})")
        mask = excluded_pairs(top["bonds"], z.shape[0], sel, args.dm_exclude) if args.dm_exclude > 0 else None
        if mask is not None and not np.triu(~mask, 1).any():
            raise ValueError(f"-dm_exclude {args.dm_exclude} leaves no pair")
        groups = None
        if args.dm_groups != "none":
            groups = groups_of(z, top.get("bonds"), top.get("mapping"), args.dm_groups)[sel]
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "sel": sel, "mask": mask, "groups": groups}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    params = {"atoms": [int(i) for i in inp["sel"]], "exclude": int(args.dm_exclude), "groups": args.dm_groups}
    maps = {} if args.maps else None
    with compare_cli.refusing():
        stats = compare(inp["gen_xyz"], inp["ref_xyz"], inp["sel"], mask=inp["mask"], groups=inp["groups"], device=args.device,
                        params=params, maps=maps)
    if args.maps:
        np.savez(args.maps, **maps)
    compare_cli.finish("distmat", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
