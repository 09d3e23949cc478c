"""Cases, inputs and the high-precision reference for the pseudo-vector message kernels (K3, csrc/pseudo_msg.hip).  NOT a
restatement: every formula comes from ``oracle.cgvae_oracle.equi_message_pseudo`` (conv.py:180-242), run in float64 (the
reference) or float32 (the yardstick of what fp32 arithmetic can give) on the block's own parameters.  No GPU needed.

Shared by tests/test_pseudo_message_cpu.py (the cases are what they claim; no GPU) and tests/test_pseudo_message_fp64.py
(``cg.EquiMessagePsuedo`` on the device against this reference, one tensor at a time).

A case is a bead graph (positions, directed edge list ``[E, 2]`` = (receiver, source), the block's cutoff) with a channel
count F and a radial basis R.  A RUN is (case, upstream arm, residual, option pseudo_fwd, deferred): the table RUNS is the
parametrisation of the GPU tests, and ``kernel_paths`` states -- by the launcher's own rule (cgv_pseudo_msg_fwd_rows /
pseudo_msg_bwd_impl) -- which kernels a run reaches, so that the coverage of the table is checked without a GPU.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict

import torch

from oracle import cgvae_oracle as O

PREFIX = "b"
OUTS = ("dh", "dhbar", "dv", "dvbar")
INS = ("s", "sbar", "v", "vbar")
PARAMS = ("inv_message.inv_dense.0.weight", "inv_message.inv_dense.0.bias", "inv_message.inv_dense.1.weight",
          "inv_message.inv_dense.1.bias", "inv_message.dist_embed.block.1.weight", "inv_message.dist_embed.block.1.bias")
FILTERED = PARAMS[2:]         # [9F, ...]: row block k = filter q_k (conv.py:199-217), compared a second time per block
# the outputs in the loss, and the filters q_k that then receive a gradient (conv.py:205-217: q0 carries dh, q1..q4 dv,
# q5..q8 dvbar; dhbar = v_i . vbar_j has no filter)
ARMS = {"all": (0, 1, 2, 3), "dh": (0,), "dhbar": (1,), "dv": (2,), "dvbar": (3,), "scalars": (0, 1), "vectors": (2, 3)}
ALIVE = {"all": set(range(9)), "dh": {0}, "dhbar": set(), "dv": {1, 2, 3, 4}, "dvbar": {5, 6, 7, 8}, "scalars": {0},
         "vectors": set(range(1, 9))}

Graph = namedtuple("Graph", "n xyz nbrs cutoff named")       # named: {label: node} of the nodes a case is about
Case = namedtuple("Case", "name graph F R")
Run = namedtuple("Run", "case arm residual variant deferred")


# ----------------------------------------------------------------------------------------------------------- graphs
def _shuffled(pairs, seed):
    nbrs = torch.tensor(pairs, dtype=torch.long).reshape(-1, 2)
    return nbrs[torch.randperm(nbrs.shape[0], generator=torch.Generator().manual_seed(seed))]


def _box(n, seed, box=4.0):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * box


def box_graph(n=23, box=4.0, nbr_cutoff=3.0, seed=4) -> Graph:
    """Random beads in a ``box`` A cube, every pair within ``nbr_cutoff`` an edge in both directions; filter cutoff 6 A."""
    xyz = _box(n, seed, box)
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, nbr_cutoff, True))
    return Graph(n, xyz, nbrs, 6.0, {})


def sparse_graph(n, seed=0) -> Graph:
    """About two incoming edges per node (1, 2 or 3): every node hears its successor on the ring, two in three a second
    node, one in seven a third.  Any two beads of the 4 A box are within the 9.5 A filter cutoff."""
    pairs = []
    for i in range(n):
        pairs.append((i, (i + 1) % n))
        if i % 3:
            pairs.append((i, (i + 2 + (7 * i) % max(n - 3, 1)) % n))
        if i % 7 == 0:
            pairs.append((i, (i + n // 2) % n))
    assert all(i != j for i, j in pairs)
    return Graph(n, _box(n, 100 + n), _shuffled(pairs, n), 9.5, {})


def _segments(n, degrees: Dict[int, int], silent, heavy=None, seed=0):
    """Asymmetric list: receiver r gets exactly ``degrees[r]`` incoming edges from the nodes outside ``silent`` and r
    itself, taken with stride 5 (coprime to the pool sizes used), so a degree beyond the pool repeats edges.  ``heavy`` =
    (receiver, source, count): that many of the receiver's edges come from ONE source (a long segment of the src-sorted
    view)."""
    pairs = []
    for r, d in degrees.items():
        pool = [j for j in range(n) if j != r and j not in silent]
        assert len(pool) % 5
        first = 0
        if heavy is not None and heavy[0] == r:
            pairs += [(r, heavy[1])] * heavy[2]
            first = heavy[2]
        pairs += [(r, pool[(13 * r + 5 * t) % len(pool)]) for t in range(first, d)]
    return _shuffled(pairs, seed)


GENERAL_DEGREES = {0: 0, 1: 1, 2: 2, 3: 3, 4: 7, 5: 8, 6: 9, 7: 16, 8: 17, 9: 130, 10: 257}
ONLY_OUT = 11                 # (like every node from 11 on) no incoming edge, but a source of others
DENSE_DEGREES = {0: 0, 1: 1, 2: 3, 3: 4, 4: 5, 5: 7, 6: 8, 7: 9, 8: 129, 9: 257}
HEAVY_SOURCE = 23


def segments_general() -> Graph:
    """n = 140, E = 450 < 16 n: incoming degrees 0, 1, 2, 3, 7, 8, 9, 16, 17 (around the 2- and 8-edge gather batches of
    pseudo_fwd_k / pseudo_bwd_recv_k), hubs of 130 and 257 edges (one and two boundaries of the 128-edge staged chunk; the
    second hub repeats edges), node 0 isolated, nodes 11.. with outgoing edges only."""
    n = 140
    nbrs = _segments(n, GENERAL_DEGREES, silent={0}, seed=3)
    return Graph(n, _box(n, 140), nbrs, 9.5, {"isolated": 0, "only_out": ONLY_OUT, "hub130": 9, "hub257": 10})


def segments_dense() -> Graph:
    """n = 24, E = 423 >= 16 n: incoming degrees 0, 1, 3, 4, 5, 7, 8, 9 (around the 4-edge batch and the 8-edge double batch
    of the dense walks: tail trips of every length), hubs of 129 and 257 edges (one and two 128-edge index chunks).  130
    of the larger hub's edges come from node 23: a 130-edge segment of the src-sorted view for pass B."""
    n = 24
    nbrs = _segments(n, DENSE_DEGREES, silent=set(), heavy=(9, HEAVY_SOURCE, 130), seed=4)
    return Graph(n, _box(n, 24), nbrs, 9.5, {"no_incoming": 0, "hub129": 8, "hub257": 9, "heavy_source": HEAVY_SOURCE})


def geometry_graph(kind: str) -> Graph:
    """n = 9.  ``coincident-far``: beads 0 and 1 coincide (distance sqrt(3e-8), unit vector 0: conv.py:25-29), bead 8 lies
    50 A away and is joined to bead 0 by an edge beyond the 6 A cutoff (its filter is exactly 0, the filter-free dhbar is
    not).  ``empty``: no edge at all."""
    n = 9
    xyz = _box(n, 9)
    if kind == "empty":
        return Graph(n, xyz, torch.zeros(0, 2, dtype=torch.long), 6.0, {})
    xyz[1] = xyz[0]
    xyz[8] = xyz[0] + 50.0
    nbrs = torch.tensor([[0, 1], [1, 0], [0, 8], [8, 0], [2, 3], [3, 2], [4, 2]])
    return Graph(n, xyz, nbrs, 6.0, {"coincident": 1, "far": 8})


def in_degrees(g: Graph):
    return torch.bincount(g.nbrs[:, 0], minlength=g.n).tolist()


def out_degrees(g: Graph):
    return torch.bincount(g.nbrs[:, 1], minlength=g.n).tolist()


# ------------------------------------------------------------------------------------------------------------ cases
WIDTHS = [(1, 4), (7, 6), (7, 10), (65, 8), (66, 16), (129, 10), (130, 6), (34, 20), (64, 12)]       # all 7 compiled n_rbf
CHUNKS = [(12, 64), (64, 8), (65, 8), (97, 8), (257, 8), (300, 8), (5, 320)]
DENSE_SHAPES = [(24, 10), (24, 20), (65, 10), (65, 20)]
_GRAPHS = {}


def _graph(key, build, *args):
    if key not in _GRAPHS:
        _GRAPHS[key] = build(*args)
    return _GRAPHS[key]


def case(name: str) -> Case:
    kind, _, rest = name.partition(":")
    nums = [int(x) for x in rest.split("-")] if rest and rest[0].isdigit() else []
    if kind == "width":
        return Case(name, _graph("box", box_graph), nums[0], nums[1])
    if kind == "chunk":
        return Case(name, _graph(("sparse", nums[0]), sparse_graph, nums[0]), nums[1], 8)
    if kind == "segments-general":
        return Case(name, _graph("general", segments_general), 24, 8)
    if kind == "segments-dense":
        return Case(name, _graph("dense", segments_dense), nums[0], nums[1])
    if kind == "geometry":
        return Case(name, _graph(("geometry", rest), geometry_graph, rest), 24, 8)
    raise KeyError(name)


WIDTH_CASES = [f"width:{F}-{R}" for F, R in WIDTHS]
CHUNK_CASES = [f"chunk:{n}-{F}" for n, F in CHUNKS]
DENSE_CASES = [f"segments-dense:{F}-{R}" for F, R in DENSE_SHAPES]
GEOMETRY_CASES = ["geometry:coincident-far", "geometry:empty"]
ARM_CASES = ["width:65-8", "segments-dense:24-10"]
DEFERRED_CASES = ["chunk:97-8", "segments-dense:24-10", "segments-dense:24-20"]
DENSE_VARIANTS = (0, 2, 4, 5)          # 0 the per-filter kernels; 2 staged pass B; 4 pseudo_bwd_src_k<8>; 5 the plain walk

RUNS_WIDTHS = [Run(c, "all", False, 0, False) for c in WIDTH_CASES]
RUNS_CHUNKS = [Run(c, "all", False, 0, False) for c in CHUNK_CASES]
RUNS_GENERAL = [Run("segments-general", "all", False, v, False) for v in range(7)]
RUNS_DENSE = [Run(c, "all", False, v, False) for c in DENSE_CASES for v in DENSE_VARIANTS]
# (arm "all" without residual is the run of the same case in RUNS_WIDTHS / RUNS_DENSE)
RUNS_ARMS = [Run(c, arm, res, 0, False) for c in ARM_CASES for arm in ARMS for res in (False, True) if res or arm != "all"]
RUNS_GEOMETRY = [Run(c, "all", res, 0, False) for c in GEOMETRY_CASES for res in (False, True)]
RUNS_DEFERRED = [Run(c, "all", False, 0, True) for c in DEFERRED_CASES]
RUNS = RUNS_WIDTHS + RUNS_CHUNKS + RUNS_GENERAL + RUNS_DENSE + RUNS_ARMS + RUNS_GEOMETRY + RUNS_DEFERRED


def run_id(run: Run) -> str:
    return (f"{run.case}|{run.arm}|{'residual' if run.residual else 'delta'}|fwd{run.variant}" + ("|deferred" if run.deferred else ""))


# --------------------------------------------------------------------------------------- the launcher's rule, restated
PATHS = ("fwd_wide", "fwd_narrow", "fwd_staged", "fwd_dense", "recv_wide", "recv_narrow", "recv_dense", "src_plain",
         "src_staged", "src_8", "src_dense", "reduce", "deferred_reduce")


def pseudo_chunks(n: int) -> int:
    """Source-node chunks of pass B (csrc/pseudo_msg.hip): one node per chunk up to 64 nodes, then max(24, n / 4) <= 64."""
    if n <= 64:
        return max(n, 1)
    return min(max(n // 4, 24), 64)


def kernel_paths(n: int, F: int, E: int, variant: int = 0, deferred: bool = False, all_upstream: bool = True):
    """The kernels one forward + backward of the block launches.  ``all_upstream``: what the LAUNCHER sees -- through
    ops._PseudoMessage always True on a dense graph (absent upstream gradients are handed over as zeros there)."""
    blocks = n * ((F + 63) // 64)
    dense = E >= 16 * n
    fwd = {1: "fwd_narrow", 2: "fwd_staged", 3: "fwd_staged", 4: "fwd_staged", 5: "fwd_wide", 6: "fwd_staged"}.get(variant)
    if fwd is None:
        fwd = "fwd_dense" if dense else ("fwd_wide" if blocks <= 256 else "fwd_narrow")
    if dense and all_upstream and variant == 0:
        bwd = {"recv_dense", "src_dense"}
    else:
        bwd = {"recv_wide" if blocks <= 256 else "recv_narrow",
               "src_8" if dense and variant == 4 else ("src_staged" if dense and variant != 5 else "src_plain")}
    return {fwd, "deferred_reduce" if deferred else "reduce"} | bwd


def run_paths(run: Run):
    c = case(run.case)
    return kernel_paths(c.graph.n, c.F, c.graph.nbrs.shape[0], run.variant, run.deferred)


# --------------------------------------------------------------------------------------------- inputs and parameters
def inputs(n: int, F: int, seed: int = 0):
    """Dense random s, sbar (sigma 1), v, vbar (sigma 0.3, distinct: the cross and sbar * vbar terms are products of the
    state, see decoder_loop_reference.dense_inputs) and dense upstream weights u0..u3 on dh, dhbar, dv, dvbar."""
    gen = torch.Generator().manual_seed(3000 + seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    return dict(s=r(n, F), sbar=r(n, F), v=0.3 * r(n, F, 3), vbar=0.3 * r(n, F, 3),
                u0=r(n, F), u1=r(n, F), u2=r(n, F, 3), u3=r(n, F, 3))


def block_params(F: int, R: int, seed: int = 0, bias_std: float = 0.1):
    """fp32 parameters of ``EquiMessagePsuedo(F, swish, R)`` under their state_dict names: Xavier-uniform weights as
    ``Dense`` draws them (modules.py:75-101), the (there zero) biases drawn too so that no bias path is fed zeros."""
    gen = torch.Generator().manual_seed(4000 + 7 * F + R + seed)
    shapes = {PARAMS[0]: (F, F), PARAMS[2]: (9 * F, F), PARAMS[4]: (9 * F, R)}
    P = {}
    for name in PARAMS:
        if name.endswith(".weight"):
            fo, fi = shapes[name]
            P[name] = (2.0 * torch.rand(fo, fi, generator=gen) - 1.0) * (6.0 / (fo + fi)) ** 0.5
        else:
            P[name] = torch.randn(shapes[name[:-4] + "weight"][0], generator=gen) * bias_std
    return P


# F = 1: every per-filter row block is ONE number, a signed sum over all 298 edges, and how far it cancels is the luck of
# the draw (over ten draws the fp32 oracle's own worst error ranged from 9e-7 to 1.2e-3 against fp64).  The draw used is
# one on which fp32 arithmetic can be judged: tests/test_pseudo_message_cpu.py holds every case to REL / 10.
DRAW = {"width:1-4": 5}


def case_inputs(c: Case):
    draw = DRAW.get(c.name, 0)
    return inputs(c.graph.n, c.F, seed=c.graph.n + c.F + draw), block_params(c.F, c.R, seed=draw)


# ------------------------------------------------------------------------------------------------------- reference
def run_reference(c: Case, inp, P, arm: str = "all", residual: bool = False, dtype=torch.float64):
    """Forward + backward of ``sum_k (out_k * u_k).sum()`` over the outputs of ``arm`` in ``dtype``; with ``residual`` the
    outputs are the inputs plus the deltas (cgvae.py:108-111).  {"out": 4, "gin": 4, "gpar": 6 tensors by name}; a
    gradient autograd leaves out is an exact zero."""
    g = c.graph
    Pd = {PREFIX + "." + k: v.detach().to(dtype).requires_grad_(True) for k, v in P.items()}
    ins = [inp[k].detach().to(dtype).requires_grad_(True) for k in INS]
    xyz = g.xyz.to(dtype)
    r_ij = xyz[g.nbrs[:, 1]] - xyz[g.nbrs[:, 0]]
    outs = O.equi_message_pseudo(*ins, r_ij, g.nbrs, Pd, PREFIX, O.swish, c.R, g.cutoff)
    if residual:
        outs = [x + d for x, d in zip(ins, outs)]
    loss = sum((outs[k] * inp[f"u{k}"].to(dtype)).sum() for k in ARMS[arm])
    if loss.requires_grad:
        loss.backward()
    grad = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(out={k: o.detach() for k, o in zip(OUTS, outs)}, gin={k: grad(t) for k, t in zip(INS, ins)},
                gpar={k: grad(Pd[PREFIX + "." + k]) for k in PARAMS})


_REF = {}             # (case, arm, residual, dtype) -> reference, computed once and left unchanged


def reference(case_name: str, arm: str = "all", residual: bool = False, dtype=torch.float64):
    key = (case_name, arm, bool(residual), dtype)
    if key not in _REF:
        c = case(case_name)
        inp, P = case_inputs(c)
        _REF[key] = run_reference(c, inp, P, arm, residual, dtype)
    return _REF[key]


def compared(res, F: int):
    """The tensors of a result in the order they are compared: 4 outputs, 4 input gradients, 6 parameter gradients, and the
    nine row blocks [kF, (k+1)F) of each of the four filter tensors on their own."""
    items = [(k, res["out"][k]) for k in OUTS] + [("grad " + k, res["gin"][k]) for k in INS]
    for k in PARAMS:
        short = k.replace("inv_message.", "").replace(".block.1", "")
        items.append(("grad " + short, res["gpar"][k]))
        if k in FILTERED:
            items += [(f"grad {short} q{q}", res["gpar"][k][q * F:(q + 1) * F]) for q in range(9)]
    return items


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref| (the norm of tests/test_hip_parity.py)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30)) if ref.numel() else 0.0


def filter_block_max(g: torch.Tensor, F: int):
    assert g.shape[0] == 9 * F
    return [float(g[k * F:(k + 1) * F].abs().max()) for k in range(9)]
