"""Cases, inputs and the high-precision reference for the encoder message kernels (K2 / K4, csrc/equi_msg.hip and
csrc/equi_msg_grp.hip).  NOT a restatement: every formula comes from ``oracle.cgvae_oracle.equi_message_block`` (conv.py:505-563)
and, for the atom -> bead case, ``contractive_message_block`` (conv.py:703-733), run in float64 (the reference) or float32
(the yardstick of what fp32 arithmetic can give) on the block's own parameters.  No GPU needed.

Shared by tests/test_equi_message_cpu.py (the cases are what they claim; no GPU) and tests/test_equi_message_fp64.py
(``cg.EquiMessageBlock`` / ``cg.ContractiveMessageBlock`` on the device against this reference, one tensor at a time).

A graph has ``n_src`` gathered nodes and ``n_dst`` receivers (the same nodes except on the bipartite atom -> bead graph), a
directed edge list ``[E, 2]`` = (receiver, source) and the block's cutoff.  A RUN is (case, F, R, upstream arm, residual,
with_dv, msg_fwd_split, msg_bwd_split, msg_bwd_mfma, fwd_group, deferred); an option of -1 leaves the launcher's own rule in
force.  The table RUNS is the parametrisation of the GPU tests, and ``kernel_paths`` states -- by the launchers' own rules
(cgv_equi_msg_fwd, ops._grouped_forward_usable / graph.receiver_group_size, bwd_shape and equi_msg_bwd_impl) -- which
template instance a run reaches, so that the coverage of the table is checked without a GPU.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from oracle import cgvae_oracle as O

PREFIX = "b"
OUTS = ("ds", "dv")
ARMS = {"all": (0, 1), "ds": (0,), "dv": (1,)}       # the outputs in the loss; "dv": gs == nullptr with gv present
# filter slice k of [3F, .] carries m_0 v_j (k = 0, into dv), m_1 (k = 1, into ds), m_2 unit (k = 2, into dv): conv.py:519-525
ALIVE = {"all": {0, 1, 2}, "ds": {1}, "dv": {0, 2}}
EQUI_PARAMS = ("inv_message.inv_dense.0.weight", "inv_message.inv_dense.0.bias", "inv_message.inv_dense.1.weight",
               "inv_message.inv_dense.1.bias", "inv_message.dist_embed.block.1.weight", "inv_message.dist_embed.block.1.bias")
CONTRACTIVE_PARAMS = tuple(k.replace("inv_message.", "") for k in EQUI_PARAMS)
N_FILTERED = 4                # the last four parameters are [3F, ...]: compared a second time per slice [kF, (k+1)F)

# n_src / n_dst nodes at pos_src / pos_dst; named: {label: node} of the nodes a case is about; mapping: atom -> bead or None
Graph = namedtuple("Graph", "n_src n_dst pos_src pos_dst nbrs cutoff named mapping")
Run = namedtuple("Run", "case F R arm residual with_dv fwd_split bwd_split bwd_mfma fwd_group deferred")


def run(case, F, R, arm="all", residual=False, with_dv=True, fwd_split=-1, bwd_split=-1, bwd_mfma=-1, fwd_group=-1,
        deferred=False) -> Run:
    return Run(case, F, R, arm, residual, with_dv, fwd_split, bwd_split, bwd_mfma, fwd_group, deferred)


# ----------------------------------------------------------------------------------------------------------- graphs
def _shuffled(pairs, seed):
    nbrs = torch.tensor(pairs, dtype=torch.long).reshape(-1, 2)
    return nbrs[torch.randperm(nbrs.shape[0], generator=torch.Generator().manual_seed(seed))]


def _box(n, seed, box=4.0):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * box


def _same_nodes(n, xyz, nbrs, cutoff, named) -> Graph:
    return Graph(n, n, xyz, xyz, nbrs, cutoff, named, None)


def box_graph(n=23, box=4.0, nbr_cutoff=3.0, seed=4) -> Graph:
    """Random nodes in a ``box`` A cube, every pair within ``nbr_cutoff`` an edge in both directions; filter cutoff 6 A.
    3 n <= E < 16 n on n <= 64 nodes: the forward splits a receiver's row over four waves, the backward walks."""
    xyz = _box(n, seed, box)
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, nbr_cutoff, True))
    return _same_nodes(n, xyz, nbrs, 6.0, {})


LADDER = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129)        # outgoing degrees of nodes 0 .. 12 (source-sorted view)
SPLIT_HUBS = {13: 200, 14: 260}


def _out_segments(n, degrees, silent, seed):
    """Asymmetric list: source j sends exactly ``degrees[j]`` edges to the nodes outside ``silent`` and j itself, taken
    with stride 5 (coprime to the pool sizes used), so a degree beyond the pool repeats edges."""
    pairs = []
    for j, d in degrees.items():
        pool = [i for i in range(n) if i != j and i not in silent]
        assert len(pool) % 5 or d == 0
        pairs += [(pool[(13 * j + 5 * t) % len(pool)], j) for t in range(d)]
    return _shuffled(pairs, seed)


def segments_walk() -> Graph:
    """n = 70, E = 360 < 16 n: outgoing degrees 0, 1, 2, 3, 4, 5, 7, 8, 9 (around the 4-edge batches of the pipelined
    scalar-only walk), 63, 64, 65 (around its 64-edge warm-up blocks) and 129 (two block boundaries; 129 edges to 68
    receivers: the hub repeats edges).  Node 0 has no edge at all, nodes 13 .. 69 have incoming edges only."""
    n = 70
    nbrs = _out_segments(n, dict(enumerate(LADDER)), silent={0}, seed=5)
    return _same_nodes(n, _box(n, 70), nbrs, 9.5, {"isolated": 0, "only_in": 13, "hub129": 12})


def segments_split() -> Graph:
    """n = 16, E = 820 >= 48 n: the same ladder of outgoing degrees (slices of ceil(len / 4) edges per wave: empty slices,
    slices of 1, 2, 3 edges, a clamped last slice; tiles of 4 edges of the matrix-core kernel with 1, 2, 3 live rows) plus
    hubs of 200 and 260 edges.  Node 0 has no edge at all, node 15 incoming edges only; every multi-edge repeats."""
    n = 16
    nbrs = _out_segments(n, {**dict(enumerate(LADDER)), **SPLIT_HUBS}, silent={0}, seed=6)
    return _same_nodes(n, _box(n, 16), nbrs, 9.5, {"isolated": 0, "only_in": 15, "hub200": 13, "hub260": 14})


def geometry_graph(kind: str) -> Graph:
    """n = 9.  ``coincident-far``: nodes 0 and 1 coincide (distance sqrt(3e-8), unit vector 0: conv.py:25-29), node 8 lies
    50 A away and is joined to node 0 alone, by an edge beyond the 6 A cutoff in each direction (filter exactly 0: node 8
    receives nothing and sends nothing).  ``empty``: no edge at all."""
    n = 9
    xyz = _box(n, 9)
    if kind == "empty":
        return _same_nodes(n, xyz, torch.zeros(0, 2, dtype=torch.long), 6.0, {})
    xyz[1] = xyz[0]
    xyz[8] = xyz[0] + 50.0
    nbrs = torch.tensor([[0, 1], [1, 0], [0, 8], [8, 0], [2, 3], [3, 2], [4, 2]])
    return _same_nodes(n, xyz, nbrs, 6.0, {"coincident": 1, "far": 8})


CHUNK_GRAPHS = {"split-130": (130, 46, 13), "split-701": (701, 46, 13), "walk-1541": (1541, 0, 7)}


def chunk_graph(kind: str) -> Graph:
    """The smallest node counts that leave the minimum chunking of the backward (bwd_shape: ceil(n / 384) nodes per chunk,
    at least 1 on the split path and 4 on the walk path); source j sends ``lo + 5 j mod span`` edges to random other nodes.
    ``split-130``: 46 .. 58 edges per node, E >= 48 n; 130 chunks of one node, 136 partial sums: the reduction's second
    trip (its loop advances by 128 chunks) is partly valid.  ``split-701``: the same degrees; 351 chunks of two nodes, the
    last one holds node 700 alone, one padding chunk, third trip.  ``walk-1541``: 0 .. 6 edges per node (about 3),
    E < 48 n; 309 chunks of five nodes (wave w takes nodes w and w + 4 of a chunk), the last one holds one node."""
    n, lo, span = CHUNK_GRAPHS[kind]
    deg = torch.tensor([lo + (5 * j) % span for j in range(n)])
    src = torch.repeat_interleave(torch.arange(n), deg)
    hop = torch.randint(0, n - 1, (src.shape[0],), generator=torch.Generator().manual_seed(n))
    nbrs = torch.stack([(src + 1 + hop) % n, src], dim=1)
    nbrs = nbrs[torch.randperm(nbrs.shape[0], generator=torch.Generator().manual_seed(n + 1))]
    return _same_nodes(n, _box(n, n), nbrs, 9.5, {"last": n - 1})


def bipartite_graph() -> Graph:
    """37 atoms -> 5 beads (ContractiveMessageBlock: edge a = (mapping[a], a), every source has exactly one edge): beads of
    9, 1, 0, 20 and 7 atoms, the atoms not sorted by bead.  n_dst <= 64 and E >= 3 n_dst: the forward splits."""
    sizes = (9, 1, 0, 20, 7)
    mapping = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    mapping = mapping[torch.randperm(mapping.shape[0], generator=torch.Generator().manual_seed(37))]
    n = mapping.shape[0]
    nbrs = torch.stack([mapping, torch.arange(n)], dim=1)
    return Graph(n, len(sizes), _box(n, 37), _box(len(sizes), 5), nbrs, 9.5, {"empty_bead": 2, "single_bead": 1}, mapping)


def in_degrees(g: Graph):
    return torch.bincount(g.nbrs[:, 0], minlength=g.n_dst).tolist()


def out_degrees(g: Graph):
    return torch.bincount(g.nbrs[:, 1], minlength=g.n_src).tolist()


_GRAPHS = {}


def graph(name: str) -> Graph:
    if name not in _GRAPHS:
        kind, _, rest = name.partition(":")
        build = {"box": box_graph, "segments-walk": segments_walk, "segments-split": segments_split,
                 "bipartite": bipartite_graph}.get(kind)
        if build is not None:
            _GRAPHS[name] = build()
        elif kind == "geometry":
            _GRAPHS[name] = geometry_graph(rest)
        elif kind == "chunks":
            _GRAPHS[name] = chunk_graph(rest)
        else:
            raise KeyError(name)
    return _GRAPHS[name]


# ------------------------------------------------------------------------------------------------------------- runs
# all seven compiled n_rbf; odd widths (scalar-access instantiation), one channel, one 16-byte piece, 130 and 129 (two and
# one live channels in the second 128-channel tile), 132 (the matrix-core test's width), the model's 600 once
WIDTHS = [(1, 4), (7, 6), (4, 8), (130, 10), (129, 12), (132, 16), (34, 20), (600, 10)]
SEGMENT_CASES = ("segments-walk", "segments-split")
SEGMENT_SHAPES = [(8, 10), (7, 10), (130, 6), (132, 12)]
CHUNK_CASES = tuple("chunks:" + k for k in CHUNK_GRAPHS)

RUNS_WIDTHS = [run("box", F, R) for F, R in WIDTHS]
RUNS_SEGMENTS = [run(c, F, R) for c in SEGMENT_CASES for F, R in SEGMENT_SHAPES]
# (arm "all" without residual is the run of the same case in RUNS_WIDTHS / RUNS_SEGMENTS)
RUNS_ARMS = ([run(c, F, 10, arm, res) for c in ("box",) + SEGMENT_CASES for F in (8, 7)
              for arm, res in (("ds", False), ("dv", False), ("all", True))]
             + [run(c, 8, 10, arm, True) for c in ("box",) + SEGMENT_CASES for arm in ("ds", "dv")]
             + [run("segments-split", 8, 16, "ds"), run("segments-split", 8, 20, "ds")])     # n_rbf + 1 > 16: off the matrix cores
RUNS_NO_DV = ([run(c, F, 8, "ds", with_dv=False) for c in ("box", "segments-walk") for F in (8, 7)]
              + [run("segments-split", 8, 8, "ds", with_dv=False), run("box", 8, 8, "ds", True, with_dv=False)])
RUNS_GEOMETRY = ([run(c, 8, 8, "all", res) for c in ("geometry:coincident-far", "geometry:empty") for res in (False, True)]
                 + [run("geometry:coincident-far", 8, 8, arm) for arm in ("ds", "dv")])
RUNS_CHUNKS = ([run("chunks:split-130", 130, 10), run("chunks:split-130", 8, 8, "ds"), run("chunks:split-130", 8, 8, "ds", bwd_mfma=0),
                run("chunks:split-130", 8, 8, "dv")]
               + [run("chunks:split-701", 8, 10), run("chunks:split-701", 8, 10, "ds"), run("chunks:split-701", 8, 10, "ds", bwd_mfma=0),
                  run("chunks:split-701", 8, 10, "dv")]
               + [run("chunks:walk-1541", 130, 6), run("chunks:walk-1541", 8, 8), run("chunks:walk-1541", 8, 8, "ds"),
                  run("chunks:walk-1541", 8, 8, "dv")])
RUNS_BIPARTITE = [run("bipartite", 8, 10), run("bipartite", 8, 10, "all", True), run("bipartite", 7, 10), run("bipartite", 8, 10, "ds"),
                  run("bipartite", 8, 10, "dv"), run("bipartite", 130, 20)]
RUNS_DEFERRED = [run("segments-split", 8, 10, deferred=True), run("segments-split", 8, 10, "ds", deferred=True),
                 run("chunks:split-701", 8, 10, deferred=True), run("box", 132, 16, deferred=True), run("bipartite", 8, 10, deferred=True)]
# option pairs that only change the order of a sum: (a, b) differ in ONE launcher option
OPTION_PAIRS = [
    (run("segments-split", 8, 10, "ds", bwd_mfma=1), run("segments-split", 8, 10, "ds", bwd_mfma=0)),      # matrix cores / FMA walk
    (run("segments-split", 8, 16, "ds", bwd_mfma=1), run("segments-split", 8, 16, "ds", bwd_mfma=0)),      # n_rbf = 16: the same kernel
    (run("segments-split", 8, 10, fwd_group=0), run("segments-split", 8, 10, fwd_group=2)),
    (run("segments-split", 8, 10, fwd_group=2), run("segments-split", 8, 10, fwd_group=4)),
    (run("box", 8, 8, fwd_split=0), run("box", 8, 8, fwd_split=1)),
    (run("segments-walk", 8, 10, bwd_split=0), run("segments-walk", 8, 10, bwd_split=1)),
    (run("segments-split", 8, 10, bwd_split=0), run("segments-split", 8, 10, bwd_split=1)),
    (run("segments-walk", 7, 10, "ds", fwd_split=0), run("segments-walk", 7, 10, "ds", fwd_split=0, bwd_mfma=1)),   # odd F: the option is moot
]
RUNS_OPTIONS = [r for pair in OPTION_PAIRS for r in pair]
DETERMINISM_RUNS = [run("chunks:split-130", 8, 8, "ds"), run("chunks:split-701", 8, 10), run("chunks:walk-1541", 8, 8),
                    run("segments-split", 8, 10)]
RUNS = list(dict.fromkeys(RUNS_WIDTHS + RUNS_SEGMENTS + RUNS_ARMS + RUNS_NO_DV + RUNS_GEOMETRY + RUNS_CHUNKS + RUNS_BIPARTITE
                          + RUNS_DEFERRED + RUNS_OPTIONS))
OPTION_NAMES = {"fwd_split": "msg_fwd_split", "bwd_split": "msg_bwd_split", "bwd_mfma": "msg_bwd_mfma", "fwd_group": "fwd_group"}


def run_id(r: Run) -> str:
    opts = "".join(f"|{k}={getattr(r, k)}" for k in OPTION_NAMES if getattr(r, k) != -1)
    return (f"{r.case}|F{r.F}|R{r.R}|{r.arm}|{'residual' if r.residual else 'delta'}" + ("" if r.with_dv else "|no-dv") + opts
            + ("|deferred" if r.deferred else ""))


# ------------------------------------------------------------------------------------- the launchers' rules, restated
FWD_PATHS = tuple(f"fwd_dv{dv}_split{sp}_pair{pr}" for dv in (0, 1) for sp in (1, 4) for pr in (0, 1))
BWD_PATHS = tuple(f"bwd_gv{gv}_split{sp}_pair{pr}" for gv in (0, 1) for sp in (0, 1) for pr in (0, 1))
PATHS = FWD_PATHS + ("fwd_grp2", "fwd_grp4") + BWD_PATHS + ("bwd_mfma", "reduce", "reduce_jobs")

BWD_WAVES, BWD_MAX_CHUNKS, RED_TRIP = 4, 384, 16 * 8          # csrc/equi_msg.hip: BWD_WAVES, BWD_MAX_CHUNKS, RED_SLICES * CB
BwdShape = namedtuple("BwdShape", "split npc chunks cpx n_chunks")


def bwd_shape(n_src: int, n_edges: int, bwd_split: int = -1) -> BwdShape:
    """``bwd_shape`` of csrc/equi_msg.hip; ``n_chunks`` = 8 cpx partial sums reach the reduction (padding chunks included)."""
    split = n_edges >= 48 * max(n_src, 1)
    if bwd_split >= 0:
        split = bwd_split != 0
    npc = max(-(-n_src // BWD_MAX_CHUNKS), 1 if split else BWD_WAVES)
    chunks = -(-n_src // npc) if n_src > 0 else 1
    cpx = -(-chunks // 8)
    return BwdShape(split, npc, chunks, cpx, 8 * cpx)


def reduce_trips(n_chunks: int) -> int:
    """Trips of the reduction loop ``for (c0 = s; c0 < n_chunks; c0 += 128)`` taken by chunk slice s = 0."""
    return -(-n_chunks // RED_TRIP)


def group_size(n_dst: int, n_edges: int, fwd_group: int = -1) -> int:
    """graph.receiver_group_size: receivers per group of the shared-source forward, 0 = per-receiver walk."""
    if fwd_group >= 0:
        return fwd_group if fwd_group in (2, 4) else 0
    return 0 if (n_edges < 16 * max(n_dst, 1) or n_dst < 4) else 2


def kernel_paths(r: Run):
    """The template instances one forward + backward of the block launches (operands from torch's allocator: every
    alignment condition of the launchers holds, every compiled n_rbf is even, and the rows lie within 2 GiB)."""
    g = graph(r.case)
    E, F = g.nbrs.shape[0], r.F
    pair = int(F % 2 == 0)
    tiles = -(-F // 128)
    # forward: ops._EquiMessage.forward -> cgv_equi_msg_fwd_grouped | cgv_equi_msg_fwd
    rb = group_size(g.n_dst, E, r.fwd_group) if g.mapping is None else 0          # (only the atom plan gets groups)
    if r.with_dv and rb and E > 0 and pair:
        fwd = f"fwd_grp{rb}"
    else:
        split = E >= 16 * g.n_dst or (g.n_dst <= 64 and E >= 3 * g.n_dst)
        if r.fwd_split >= 0:
            split = r.fwd_split != 0
        fwd = f"fwd_dv{int(r.with_dv)}_split{4 if split else 1}_pair{pair}"
    # backward: equi_msg_bwd_impl
    has_gs, has_gv = 0 in ARMS[r.arm], r.with_dv and 1 in ARMS[r.arm]
    assert has_gs or has_gv
    sh = bwd_shape(g.n_src, E, r.bwd_split)
    mfma_pays = r.bwd_mfma == 1 or (r.bwd_mfma < 0 and (E >= 200 * max(g.n_src, 1) or 8 * sh.cpx * tiles <= 512))
    if not has_gv and has_gs and sh.split and r.R + 1 <= 16 and F % 4 == 0 and mfma_pays:
        bwd = "bwd_mfma"
    else:
        bwd = f"bwd_gv{int(has_gv)}_split{int(sh.split)}_pair{pair}"
    return {fwd, bwd, "reduce_jobs" if r.deferred else "reduce"}


def k_live(r: Run) -> int:
    """Live filter slices of the partial sums (``gv ? 3 : 1``)."""
    return 3 if (r.with_dv and 1 in ARMS[r.arm]) else 1


# --------------------------------------------------------------------------------------------- inputs and parameters
def param_names(g: Graph):
    return EQUI_PARAMS if g.mapping is None else CONTRACTIVE_PARAMS


def inputs(g: Graph, F: int, seed: int = 0):
    """Dense random s (sigma 1), v (sigma 0.5) on the sources, dense upstream weights u0, u1 on ds, dv and the receiver-shaped
    residual states H, V of the atom -> bead block (the other blocks' residual is the input state itself)."""
    gen = torch.Generator().manual_seed(5000 + seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    return dict(s=r(g.n_src, F), v=0.5 * r(g.n_src, F, 3), u0=r(g.n_dst, F), u1=r(g.n_dst, F, 3), H=r(g.n_dst, F),
                V=0.5 * r(g.n_dst, F, 3))


def block_params(names, F: int, R: int, seed: int = 0, bias_std: float = 0.1):
    """fp32 parameters of ``EquiMessageBlock(F, swish, R)`` / ``ContractiveMessageBlock`` under their state_dict names:
    Xavier-uniform weights as ``Dense`` draws them (modules.py:75-101), the (there zero) biases drawn too so that no bias
    path is fed zeros."""
    gen = torch.Generator().manual_seed(6000 + 7 * F + R + seed)
    shapes = {names[0]: (F, F), names[2]: (3 * F, F), names[4]: (3 * F, R)}
    P = {}
    for name in names:
        if name.endswith(".weight"):
            fo, fi = shapes[name]
            P[name] = (2.0 * torch.rand(fo, fi, generator=gen) - 1.0) * (6.0 / (fo + fi)) ** 0.5
        else:
            P[name] = torch.randn(shapes[name[:-4] + "weight"][0], generator=gen) * bias_std
    return P


# One channel: every filter slice is ONE number per basis function, a signed sum over all edges, and how far it cancels is
# the luck of the draw.  DRAW picks, per (case, F), a draw on which fp32 arithmetic can be judged (tests/test_equi_message_cpu.py
# holds every tensor of every run to REL).
DRAW = {}


def run_inputs(r: Run):
    g = graph(r.case)
    draw = DRAW.get((r.case, r.F), 0)
    return inputs(g, r.F, seed=g.n_src + r.F + draw), block_params(param_names(g), r.F, r.R, seed=draw)


# ------------------------------------------------------------------------------------------------------- reference
def in_names(g: Graph, residual: bool):
    return ("s", "v", "H", "V") if (g.mapping is not None and residual) else ("s", "v")


def run_reference(r: Run, dtype=torch.float64):
    """Forward + backward of ``sum_k (out_k * u_k).sum()`` over the outputs of ``r.arm`` in ``dtype``; with ``residual`` the
    outputs are the receivers' states plus the deltas (cgvae.py:287, 301-302).  {"out": 2, "gin": 2 or 4, "gpar": 6 tensors by
    name}; a gradient autograd leaves out is an exact zero.  (``with_dv`` = False is not a property of the reference: the
    device then skips the vector channel, its dv is compared with the residual / zero and only arm "ds" is run.)"""
    g = graph(r.case)
    inp, P = run_inputs(r)
    names = param_names(g)
    Pd = {PREFIX + "." + k: v.detach().to(dtype).requires_grad_(True) for k, v in P.items()}
    ins = {k: inp[k].detach().to(dtype).requires_grad_(True) for k in in_names(g, r.residual)}
    pos_s, pos_d = g.pos_src.to(dtype), g.pos_dst.to(dtype)
    r_e = pos_s[g.nbrs[:, 1]] - pos_d[g.nbrs[:, 0]]                       # cgvae.py:275 / 280
    if g.mapping is None:
        outs = O.equi_message_block(ins["s"], ins["v"], r_e, g.nbrs, Pd, PREFIX, O.swish, r.R, g.cutoff)
        res = (ins["s"], ins["v"])
    else:
        assert int(g.mapping.max()) + 1 == g.n_dst                        # (dim_size is inferred there)
        assert torch.equal(g.nbrs[:, 1], torch.arange(g.n_src)) and torch.equal(g.nbrs[:, 0], g.mapping)     # r_e is r_iI
        outs = O.contractive_message_block(ins["s"], ins["v"], r_e, g.mapping, Pd, PREFIX, O.swish, r.R, g.cutoff)
        res = (ins.get("H"), ins.get("V"))
    if r.residual:
        outs = [x + d for x, d in zip(res, outs)]
    loss = sum((outs[k] * inp[f"u{k}"].to(dtype)).sum() for k in ARMS[r.arm])
    if loss.requires_grad:
        loss.backward()
    grad = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(out={k: o.detach() for k, o in zip(OUTS, outs)}, gin={k: grad(t) for k, t in ins.items()},
                gpar={k: grad(Pd[PREFIX + "." + k]) for k in names})


def ref_key(r: Run):
    """What the reference depends on (no launcher option, not ``deferred``, not ``with_dv``)."""
    return (r.case, r.F, r.R, r.arm, bool(r.residual))


_REF = {}             # (ref_key, dtype) -> reference, computed once and left unchanged


def reference(r: Run, dtype=torch.float64):
    key = (ref_key(r), dtype)
    if key not in _REF:
        _REF[key] = run_reference(r, dtype)
    return _REF[key]


def short(name: str) -> str:
    return name.replace("inv_message.", "").replace(".block.1", "")


def compared(res, F: int, with_dv: bool = True):
    """The tensors of a result in the order they are compared: the outputs (dv only with the vector channel), the input
    gradients, the 6 parameter gradients, and the three slices [kF, (k+1)F) of each of the four filter tensors on their own."""
    items = [(k, res["out"][k]) for k in OUTS if with_dv or k == "ds"] + [("grad " + k, t) for k, t in res["gin"].items()]
    names = list(res["gpar"])
    for k in names:
        items.append(("grad " + short(k), res["gpar"][k]))
        if k in names[-N_FILTERED:]:
            items += [(f"grad {short(k)} slice {q}", res["gpar"][k][q * F:(q + 1) * F]) for q in range(3)]
    return items


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref| (the norm of tests/test_hip_parity.py)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30)) if ref.numel() else 0.0


def filter_slice_max(t: torch.Tensor, F: int):
    assert t.shape[0] == 3 * F
    return [float(t[k * F:(k + 1) * F].abs().max()) for k in range(3)]
