"""Which conformational states an ensemble has, and how much weight a generated ensemble puts on each: clustering by
superposed RMSD (Daura et al., "GROMOS", the default of ``gmx cluster -method gromos``) on the device -- the pairwise
squared RMSDs of K17 (``cgv_superpose``) packed into a neighbour bit matrix and the greedy loop run over it by K24
(``cgv_cluster_pack``, ``cgv_cluster_gromos``; ``csrc/cluster.hip``).  No ``[S, S]`` fp64 tensor reaches the host.

None of the other analyses names states: ``coverage`` says whether something is near each frame, not whether the folded
and the misfolded basin are weighted 70 : 30; ``tica`` and ``density`` compare projections, in which two ensembles can
agree and still differ in the whole-structure states they visit.  Nothing in the reference computes this.

``c2 = float(cutoff) ** 2`` in fp64.  For structures ``p < q`` of a set, ``adj(p, q) = adj(q, p) = (d2(p, q) <= c2)`` with
``d2(p, q)`` what ``cgv_superpose`` writes for row ``p``, column ``q`` of the set against itself: only the upper triangle
decides, so the graph is symmetric.  ``adj(p, p) = 1`` iff ``p`` is good; a structure with a non-finite selected coordinate
is *bad*, has an empty row and column, label ``-1``, and is in no count.  The loop: ``alive`` starts as the good
structures; the centre is the alive structure with most alive neighbours (itself included), the lowest index on ties; it
and its alive neighbours become cluster ``k`` and leave; repeat until nothing is alive.  All of it is integer and ordered:
two calls give the same bits, whatever ``structures_per_launch`` is.  Lengths in Angstrom.

    python -m coarsegrainingvae_amd.cluster -gen samples.npz -ref traj.npz [-top top.npz] [-cluster_cutoff 1.0]
        [-cluster_atoms heavy|all] [-cluster_stride 1] [-labels labels.npz] [-out cluster_stats.json]

``-gen``: the ``xyz [T, K, n, 3]`` (or ``[S, n, 3]``) that ``backmap -out`` writes; ``-ref``: a trajectory file with
``xyz [T, n, 3]``; ``z`` comes from ``-top``, else from ``-ref``.  The states are the clusters of ``ref[::stride]``; every
reference frame and every generated structure is then assigned to the nearest centre within the cutoff.  The full
statistics of ``compare`` go to ``-out``, the states of all structures to ``-labels``, one JSON line with
``"cluster_stats": summary_of(...)`` to stdout.
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, compare_cli, coverage, ensemble
from .ensemble import check_sets, device_of, read_back, select_atoms, structures

MAX_CHUNK = 8192                       # structures_per_launch is capped here: one dense chunk is then at most 512 MiB


def limits() -> Dict[str, int]:
    return ensemble.limits("cluster", ("structures",))


def _c2(cutoff) -> float:
    c = float(cutoff)
    if not math.isfinite(c) or c < 0:
        raise ValueError(f"the cutoff must be a finite length >= 0, got {cutoff}")
    return c * c


def _chunk(structures_per_launch: int) -> int:
    return min((max(int(structures_per_launch), 1) + 63) // 64 * 64, MAX_CHUNK)


def _table(sel, n: int) -> np.ndarray:
    return ensemble.selection(sel, n, purpose="superpose", unique=False, max_atoms=coverage.limits()["atoms"])


# ----------------------------------------------------------------------------- the launches
def adjacency(xyz, sel=None, cutoff: float = 1.0, structures_per_launch: int = 4096, device="cuda") -> torch.Tensor:
    """The neighbour bit matrix ``bits [S, W]`` (device, int64 holding the 64 bits of a word; ``W = ceil(S / 64)``) of the
    structures ``xyz [S,n,3]`` over the atoms ``sel`` (default: all): bit ``q & 63`` of word ``q >> 6`` of row ``p`` is
    ``adj(p, q)``.  The set is cut into chunks of ``structures_per_launch`` rounded up to a multiple of 64; every pair of
    chunks ``oa <= ob`` is one ``cgv_superpose`` call with a dense output and one ``cgv_cluster_pack``, which also writes
    the mirrored words of the lower triangle.  The result does not depend on the chunk size."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    table = _table(sel, n)
    c2 = _c2(cutoff)
    lim = limits()["structures"]
    if S > lim:
        raise ValueError(f"{S} structures: the clustering kernel holds {lim}; take every k-th one (stride)")
    dev = device_of(x, device)
    W = (S + 63) // 64
    if S == 0:
        return torch.zeros(0, 0, dtype=torch.int64, device=dev)
    M = min(_chunk(structures_per_launch), (S + 63) // 64 * 64)
    lib = _lib.load()
    ws = ensemble.workspace(int(lib.cgv_cluster_workspace_bytes(S, M)), dev)
    bits = ws[:S * W].view(torch.int64).view(S, W)
    bits.zero_()
    room = ws[S * W:]
    xs = x.detach().to(dev, torch.float32).contiguous()
    stab = torch.from_numpy(table).to(dev)
    scratch = ensemble.workspace(int(lib.cgv_superpose_workspace_bytes(min(M, S), min(M, S))), dev)
    state = coverage.new_state(S, S, dev)                     # the launch merges minima nobody reads here
    for oa in range(0, S, M):
        ea = min(oa + M, S)
        for ob in range(oa, S, M):
            eb = min(ob + M, S)
            dense = room[:(ea - oa) * (eb - ob)].view(ea - oa, eb - ob)
            coverage.superpose_launch(xs[oa:ea], xs[ob:eb], stab, state["row_min"][oa:ea], state["row_arg"][oa:ea],
                                      state["col_min"][ob:eb], state["col_arg"][ob:eb], oa, ob, False, dense=dense,
                                      workspace=scratch)
            _lib.call("cgv_cluster_pack", _lib.ptr(dense), ea - oa, eb - ob, oa, ob, S, c2, _lib.ptr(bits), _lib.stream_ptr(),
                      tag="cluster_pack")
    return bits


def pack_mask(good, S: int) -> np.ndarray:
    """A boolean ``[S]`` as the ``[W]`` words the kernel takes (int64 holding the bits)."""
    g = np.zeros((S + 63) // 64 * 64, dtype=np.uint8)
    g[:S] = np.asarray(good, dtype=bool).reshape(-1)
    return np.packbits(g.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1).astype(np.uint64).view(np.int64)


def gromos(bits: torch.Tensor, S: int, good=None):
    """The clustering loop on a device bit matrix ``bits [S, W]`` (``adjacency``): one launch, one read-back.  ``good``: a
    boolean ``[S]``, the structures that take part (default: those with their diagonal bit).  Returns host arrays
    ``label [S]`` int32 (``-1``: not good), ``centres [C]``, ``sizes [C]`` int32 in the order the clusters were found."""
    S = int(S)
    lim = limits()["structures"]
    if S > lim:
        raise ValueError(f"{S} structures: the clustering kernel holds {lim}; take every k-th one (stride)")
    if S == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    W = (S + 63) // 64
    if tuple(bits.shape) != (S, W) or bits.dtype != torch.int64:
        raise ValueError(f"bits must be [{S}, {W}] int64, got {tuple(bits.shape)} {bits.dtype}")
    dev = bits.device
    d_good = None if good is None else torch.from_numpy(pack_mask(good, S)).to(dev)
    out = torch.empty(3 * S + 1, dtype=torch.int32, device=dev)
    _lib.call("cgv_cluster_gromos", _lib.ptr(bits), _lib.ptr(d_good), S, _lib.ptr(out[:S]), _lib.ptr(out[S:2 * S]),
              _lib.ptr(out[2 * S:3 * S]), _lib.ptr(out[3 * S:]), _lib.stream_ptr(), tag="cluster_gromos")
    host = read_back([out])[0]
    C = int(host[3 * S])
    return host[:S].copy(), host[S:S + C].copy(), host[2 * S:2 * S + C].copy()


def cluster(xyz, z, cutoff: float = 1.0, atoms="heavy", structures_per_launch: int = 4096, device="cuda") -> dict:
    """The clusters of the structures ``xyz [S,n,3]`` of the molecule ``z [n]`` by superposed RMSD over
    ``select_atoms(z, atoms)`` with the neighbour criterion ``rmsd <= cutoff``:

      label [S] int32     the cluster of a structure, ``-1`` for a bad one
      centres [C] int32   the centre of a cluster (an index into ``xyz``), in the order found
      sizes [C] int32     its number of members
      n_bad, cutoff, atoms (the selection used)

    ``ValueError`` before any launch for more structures than ``limits()`` (cluster every k-th frame: ``stride`` of
    ``compare``), a cutoff that is no finite length >= 0, and everything ``ensemble.selection`` refuses."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    if zz.shape[0] != n:
        raise ValueError(f"z lists {zz.shape[0]} atoms, a structure has {n}")
    _c2(cutoff)
    sel = select_atoms(zz, atoms)
    _table(sel, n)
    lim = limits()["structures"]
    if S > lim:
        raise ValueError(f"{S} structures: the clustering kernel holds {lim}; take every k-th one (stride)")
    bits = adjacency(x, sel, cutoff, structures_per_launch, device)
    label, centres, sizes = gromos(bits, S)
    return {"label": label, "centres": centres, "sizes": sizes, "n_bad": int((label < 0).sum()), "cutoff": float(cutoff),
            "atoms": [int(i) for i in sel]}


def assign(xyz, centre_xyz, sel=None, cutoff: float = 1.0, structures_per_launch: int = 4096, device="cuda"):
    """``(state [S] int64, rmsd [S] fp64)``: for every structure of ``xyz [S,n,3]`` the nearest of the centres
    ``centre_xyz [C,n,3]`` by superposed RMSD over ``sel`` (the lower index on equal distances) and the RMSD to it.  The
    squared minimum is tested with the same ``<= c2`` as the clustering; a structure with no centre within the cutoff is
    unassigned, ``state = -1`` (its ``rmsd`` is still that to the nearest centre).  A bad structure, or one without any
    good centre, has ``(-1, +inf)``.  Chunked as ``coverage.nearest``; one read-back."""
    a, c = structures(xyz), structures(centre_xyz)
    if int(a.shape[1]) != int(c.shape[1]):
        raise ValueError(f"the two sets have different atom counts (mismatched n): {int(a.shape[1])} and {int(c.shape[1])}")
    table = _table(sel, int(a.shape[1]))
    c2 = _c2(cutoff)
    sa, sc = int(a.shape[0]), int(c.shape[0])
    M = min(max(int(structures_per_launch), 1), coverage.limits()["structures"])
    dev = device_of(a, device)
    state = coverage.new_state(sa, sc, dev)
    if sa and sc:
        stab = torch.from_numpy(table).to(dev)
        xa, xc = a.detach().to(dev, torch.float32).contiguous(), c.detach().to(dev, torch.float32).contiguous()
        scratch = ensemble.workspace(int(_lib.load().cgv_superpose_workspace_bytes(min(M, sa), min(M, sc))), dev)
        for oa in range(0, sa, M):
            for ob in range(0, sc, M):
                ea, eb = min(oa + M, sa), min(ob + M, sc)
                coverage.superpose_launch(xa[oa:ea], xc[ob:eb], stab, state["row_min"][oa:ea], state["row_arg"][oa:ea],
                                          state["col_min"][ob:eb], state["col_arg"][ob:eb], oa, ob, False, workspace=scratch)
    row_min, row_arg = read_back([state["row_min"], state["row_arg"]])
    return np.where(row_min <= c2, row_arg, -1).astype(np.int64), np.sqrt(row_min)


# ----------------------------------------------------------------------------- host statistics
def _side(assigned, C: int):
    """Of one set: the good structures' states and RMSDs, populations ``[C]``, unassigned, bad."""
    state = np.asarray(assigned[0], dtype=np.int64).reshape(-1)
    rmsd = np.asarray(assigned[1], dtype=np.float64).reshape(-1)
    if state.shape != rmsd.shape:
        raise ValueError("a set's states and RMSDs have different lengths")
    if state.size and (state.min() < -1 or state.max() >= C):
        raise ValueError(f"a state outside -1 .. {C - 1}")
    good = np.isfinite(rmsd)
    s, r = state[good], rmsd[good]
    pop = np.bincount(s[s >= 0], minlength=C).astype(np.int64)
    return {"n": int(state.size), "n_bad": int(state.size - good.sum()), "state": s, "rmsd": r, "pop": pop,
            "unassigned": int((s < 0).sum())}


def _bins(side) -> np.ndarray:
    return np.concatenate([side["pop"], [side["unassigned"]]])


def _spread(side, C: int):
    hit = side["state"] >= 0
    total = np.bincount(side["state"][hit], weights=side["rmsd"][hit], minlength=C)
    return [float(total[k] / side["pop"][k]) if side["pop"][k] else None for k in range(C)]


def compare_from_labels(even, odd, gen, centres, sizes, min_population: float = 0.01, params: Optional[dict] = None) -> dict:
    """The statistics of ``compare`` from three results of ``assign`` -- ``(state, rmsd)`` of the even reference frames,
    the odd ones and the generated structures, all against the same ``C = len(centres)`` centres -- pure host.  A structure
    whose RMSD is not finite is bad and in no count.  Keys: ``CLUSTER_STATS_KEYS``; see ``compare``."""
    centres = [int(c) for c in np.asarray(centres).reshape(-1)]
    sizes = [int(c) for c in np.asarray(sizes).reshape(-1)]
    C = len(centres)
    if len(sizes) != C:
        raise ValueError(f"{C} centres, {len(sizes)} sizes")
    if not 0 <= float(min_population) <= 1:
        raise ValueError(f"min_population is a share of the reference, 0 .. 1, got {min_population}")
    e, o, g = _side(even, C), _side(odd, C), _side(gen, C)
    ref = {"n": e["n"] + o["n"], "n_bad": e["n_bad"] + o["n_bad"], "state": np.concatenate([e["state"], o["state"]]),
           "rmsd": np.concatenate([e["rmsd"], o["rmsd"]]), "pop": e["pop"] + o["pop"], "unassigned": e["unassigned"] + o["unassigned"]}
    good_ref, good_gen = ref["n"] - ref["n_bad"], g["n"] - g["n_bad"]
    assigned = int(ref["pop"].sum())
    order = np.argsort(-ref["pop"], kind="stable")
    held = np.cumsum(ref["pop"][order])
    states_90 = int(np.searchsorted(held, 0.9 * assigned, side="left") + 1) if assigned else 0
    missing = [int(k) for k in range(C) if good_ref and ref["pop"][k] >= float(min_population) * good_ref
               and ref["pop"][k] > 0 and g["pop"][k] == 0]
    top = []
    if good_ref and good_gen:
        p_ref, p_gen = ref["pop"] / good_ref, g["pop"] / good_gen
        for k in np.argsort(-np.abs(p_ref - p_gen), kind="stable")[:10]:
            top.append({"state": int(k), "centre": centres[int(k)], "p_ref": float(p_ref[k]), "p_gen": float(p_gen[k])})
    return {"n_ref": ref["n"], "n_gen": g["n"], "n_bad_ref": ref["n_bad"], "n_bad_gen": g["n_bad"],
            "params": dict(params or {}, min_population=float(min_population)), "n_clusters": C, "centres": centres,
            "sizes": sizes, "pop_ref": ref["pop"].tolist(), "pop_gen": g["pop"].tolist(), "unassigned_ref": ref["unassigned"],
            "unassigned_gen": g["unassigned"], "jsd": ensemble.js_divergence(_bins(ref), _bins(g)),
            "floor": ensemble.js_divergence(_bins(e), _bins(o)), "states_90": states_90, "missing_states": missing,
            "spread_ref": _spread(ref, C), "spread_gen": _spread(g, C), "top_states": top}


def _run(ref_xyz, gen_xyz, z, cutoff, atoms, stride, min_population, structures_per_launch, device):
    ref, gen, z = check_sets(ref_xyz, gen_xyz, z)
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1, got {stride}")
    if not 0 <= float(min_population) <= 1:
        raise ValueError(f"min_population is a share of the reference, 0 .. 1, got {min_population}")
    kw = dict(structures_per_launch=structures_per_launch, device=device)
    found = cluster(ref[::stride], z, cutoff, atoms, **kw)
    sel = np.asarray(found["atoms"], dtype=np.int64)
    frames = found["centres"].astype(np.int64) * stride
    centre_xyz = ref[torch.from_numpy(frames).to(ref.device)]
    even, odd, got = (assign(x, centre_xyz, sel, cutoff, **kw) for x in (ref[0::2], ref[1::2], gen))
    params = {"atoms": found["atoms"], "cutoff": float(cutoff), "stride": stride}
    stats = compare_from_labels(even, odd, got, frames, found["sizes"], min_population, params)
    ref_state = np.empty(int(ref.shape[0]), dtype=np.int64)
    ref_rmsd = np.empty(int(ref.shape[0]), dtype=np.float64)
    ref_state[0::2], ref_state[1::2], ref_rmsd[0::2], ref_rmsd[1::2] = even[0], odd[0], even[1], odd[1]
    labels = {"centres": frames, "sizes": found["sizes"], "cluster_label": found["label"], "ref_state": ref_state,
              "ref_rmsd": ref_rmsd, "gen_state": got[0], "gen_rmsd": got[1]}
    return stats, labels


def compare(ref_xyz, gen_xyz, z, cutoff: float = 1.0, atoms="heavy", stride: int = 1, min_population: float = 0.01,
            structures_per_launch: int = 4096, device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) of the
    molecule ``z [n]`` by the states of the reference: the clusters of ``ref[::stride]`` (``cluster``).  The even frames,
    the odd frames and the generated structures are each assigned to the nearest centre within the cutoff (``assign``),
    the reference is the sum of its halves, and what the halves differ by is the ``floor``.  Returns a dict that
    ``json.dump`` takes:

      n_ref, n_gen, n_bad_ref, n_bad_gen    structures, and those left out as bad (with no cluster at all: every one)
      params        atoms (the selection), cutoff, stride, min_population
      n_clusters, centres [C] (frame indices into ``ref_xyz``), sizes [C] (members among ``ref[::stride]``)
      pop_ref, pop_gen [C]   structures assigned to a state; unassigned_ref, unassigned_gen: good ones near no centre
      jsd           Jensen-Shannon divergence (base 2) of the two populations over C + 1 bins, unassigned being a bin;
                    ``None`` when a set has no good structure
      floor         the same between the even and the odd reference frames
      states_90     how many of the largest states hold 90 % of the assigned reference
      missing_states   states with at least ``min_population`` of the good reference and no generated structure
      spread_ref, spread_gen [C]   mean RMSD to the centre of the structures assigned to a state (``None``: none)
      top_states    the ten states of largest |p_ref - p_gen|: {state, centre, p_ref, p_gen}, p a share of the good ones
    """
    return _run(ref_xyz, gen_xyz, z, cutoff, atoms, stride, min_population, structures_per_launch, device)[0]


CLUSTER_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "n_clusters", "centres", "sizes", "pop_ref",
                      "pop_gen", "unassigned_ref", "unassigned_gen", "jsd", "floor", "states_90", "missing_states",
                      "spread_ref", "spread_gen", "top_states")
_LISTS = ("centres", "sizes", "pop_ref", "pop_gen", "spread_ref", "spread_gen")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"cluster_stats"`` in its JSON summary line: no per-cluster lists."""
    return {k: stats[k] for k in CLUSTER_STATS_KEYS if k not in _LISTS}


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.cluster",
                                "conformational states of a reference by RMSD clustering, and how generated structures populate them",
                                top_help="npz with z; default: that of -ref")
    p.add_argument("-cluster_cutoff", type=float, default=1.0, help="neighbour criterion: superposed RMSD in Angstrom (1.0)")
    p.add_argument("-cluster_atoms", choices=("heavy", "all"), default="heavy", help="the atoms superposed and compared (heavy)")
    p.add_argument("-cluster_stride", type=int, default=1, help="cluster every k-th reference frame (1)")
    p.add_argument("-labels", default=None, help="npz for the centres and the state of every frame and structure (not written)")
    return compare_cli.finish_parser(p, "cluster_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, with everything that can be refused without a device
    refused here (``SystemExit``)."""
    if not math.isfinite(args.cluster_cutoff) or args.cluster_cutoff < 0:
        raise SystemExit("-cluster_cutoff must be a finite length >= 0 in Angstrom")
    if args.cluster_stride < 1:
        raise SystemExit("-cluster_stride must be at least 1")
    ref_xyz, gen_xyz, z, _, _ = compare_cli.read_sets(args, need=("z",))
    if select_atoms(z, args.cluster_atoms).shape[0] == 0:
        raise SystemExit(f"the topology has no {args.cluster_atoms} atoms")
    lim = limits()["structures"]
    used = -(-ref_xyz.shape[0] // args.cluster_stride)
    if used > lim:
        raise SystemExit(f"{used} reference frames to cluster, the kernel holds {lim}: pass -cluster_stride "
                         f"{-(-ref_xyz.shape[0] // lim)} or more")
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    with compare_cli.refusing():
        stats, labels = _run(inp["ref_xyz"], inp["gen_xyz"], inp["z"], args.cluster_cutoff, args.cluster_atoms,
                             args.cluster_stride, 0.01, 4096, args.device)
    compare_cli.write_stats(stats, args.out)
    if args.labels:
        np.savez(args.labels, **labels)
    compare_cli.print_summary("cluster", summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
