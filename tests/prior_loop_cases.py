"""Cases, inputs and the high-precision reference for the prior net's fused message-block loop (coarsegrainingvae_amd/prior_fused.py:
``prior_msg_fwd_k`` / ``prior_msg_bwd_k`` of csrc/decoder_layer.hip and the decoder layer's Dense kernels at N = K = F).
NOT a restatement: every formula comes from ``oracle.cgvae_oracle.equi_message_block`` (conv.py:505-563), looped with
``h += ds``, ``v += dv`` as CGprior.forward does (cgvae.py:391-392), run in float64 (the reference) or float32 (the
yardstick of what fp32 arithmetic can give) on the module's own parameters.  No GPU needed.

Shared by tests/test_prior_loop_cpu.py (the cases are what they claim; no GPU) and tests/test_prior_loop_fp64.py (the fused
loop, the per-block path and the forward kernel alone against this reference, one tensor at a time).

Two levels.  LOOP: ``CGprior.features(..., h0=h)`` from a dense random ``h`` and v = 0 (cgvae.py:388), loss
``(h_out * up).sum()``.  KERNEL: one ``cgv_prior_msg_fwd`` launch on dense random ``a1``, ``s`` and ``v``; its reference is the
same oracle function handed ``a1`` as the node state with an identity first Dense and an identity activation, so that
``inv_dense`` (conv.py:41-49) reduces to ``a1 W2^T + b2`` exactly and the message sums and the residual follow unchanged.

A case is (n, F, R, layers, graph, options, slack); ``kernel_path`` states -- by the launchers' own rules
(cgv_decoder_block_channels, the CGV_DL_QS boundary at 108 slices, F / 4 slices out of the message backward) -- which
instance of ``prior_msg_bwd_k`` / ``dec_dense_bwd_k`` a case reaches, so that the coverage of the table is checked without
a GPU.
"""
from __future__ import annotations

from collections import namedtuple

import torch

import decoder_loop_reference as D
from oracle import cgvae_oracle as O

PREFIX = "prior_net"
CUTOFF = 9.5
RBF_LIST = (4, 6, 8, 10, 12, 16, 20)            # CGV_RBF_LIST of csrc/cgv_common.h
MAX_EDGES = 240                                 # DL_MAX_EDGES of csrc/decoder_layer.hip: 16 nodes, every ordered pair
QS_BOUNDARY, MAX_SLICES = 108, 216              # CGV_DL_QS; the slice count cgv_prior_msg_bwd / cgv_decoder_dense_bwd accept
NAMES = ("W1", "b1", "W2", "b2", "Wd", "bd")    # prior_fused.layer_params order
FILTERED = ("W2", "b2", "Wd", "bd")             # [3F, .]: compared a second time per filter slice q_k = rows [kF, (k+1)F)
# The smallest share of max |dv| that each of the two terms of dv (m_0 v_j and m_2 unit_ij, conv.py:523-525) must reach
# wherever v_out is compared with v != 0: a term below it could be wrong without moving v_out past the tolerance scale.
SHARE = 0.1

Case = namedtuple("Case", "n F R layers graph options slack")
THIN = {"decoder_fat": 0}
COL0 = {"decoder_colsplit": 0, "decoder_nodesplit": 0}
COL3 = {"decoder_colsplit": 3, "decoder_nodesplit": 0}
CASES = {
    "chignolin-12-600": Case(12, 600, 10, 2, "dense", {}, 0.0),           # 75 slices into prior_msg_bwd_k, 150 into dense_bwd
    "chignolin-12-600-thin": Case(12, 600, 10, 2, "dense", THIN, 0.0),    # 150 slices: QS = 6 in prior_msg_bwd_k
    "chignolin-12-600-col0": Case(12, 600, 10, 2, "dense", COL0, 0.0),    # dense_bwd: one block per channel group
    "chignolin-12-600-col3": Case(12, 600, 10, 2, "dense", COL3, 0.0),    # ... three column parts
    "lane3-12-432-thin": Case(12, 432, 8, 2, "dense", THIN, 0.0),         # 108 slices: the last count on the 3-slice lane class
    "lane6-12-440-thin": Case(12, 440, 8, 2, "dense", THIN, 0.0),         # 110 slices: the first on the 6-slice lane class
    "odd8-8-436": Case(8, 436, 10, 2, "dense", {}, 0.0),                  # F % 8 == 4: 109 slices, QS = 6 with nothing set
    "widest-8-864-thin": Case(8, 864, 10, 2, "dense", THIN, 0.0),         # 216 slices: the cap
    "narrowest-5-16-R4": Case(5, 16, 4, 3, "dense", {}, 0.0),             # one column tile, smallest edge record
    "rbf6-6-32": Case(6, 32, 6, 2, "dense", {}, 0.0),
    "rbf12-8-64": Case(8, 64, 12, 2, "dense", {}, 0.0),
    "rbf16-7-48": Case(7, 48, 16, 2, "dense", {}, 0.0),
    "rbf20-7-200": Case(7, 200, 20, 2, "dense", {}, 0.0),                 # largest edge record
    "capacity-16-64": Case(16, 64, 10, 2, "dense", {}, 0.0),              # 16 nodes fully connected: 240 edges
    "pair-2-32": Case(2, 32, 8, 2, "pair", {}, 0.0),                      # two nodes, ONE directed edge
    "sparse-10-64": Case(10, 64, 8, 2, "sparse", {}, 0.0),                # a receiver without, receivers with one incoming edge
    "silent-source-9-64": Case(9, 64, 10, 2, "silent", {}, 0.0),          # a source without outgoing edge, an edge beyond the cutoff
    "deep-12-128": Case(12, 128, 10, 4, "dense", {}, 0.0),                # slices chained through four layers
    "single-12-128": Case(12, 128, 10, 1, "dense", {}, 0.0),              # base only: no slices ever reach prior_msg_bwd_k
    "single-12-128-slack": Case(12, 128, 10, 1, "dense", {}, 1.0),        # ... the same bits with capacity > E
    "sparse-10-64-single": Case(10, 64, 8, 1, "sparse", {}, 0.0),         # one layer: h_out[i] == h_in[i] bit for bit without incoming edge
    "slack-7-200": Case(7, 200, 20, 2, "dense", {}, 1.0),                 # capacity > E, NaN records past the last edge
}
# the forward kernel alone (dense a1, s, v): widest block count, 240 edges, empty rows, largest and smallest record, slack
KERNEL_CASES = ("chignolin-12-600", "capacity-16-64", "sparse-10-64", "rbf20-7-200", "narrowest-5-16-R4", "slack-7-200")
CHAIN_CASES = ("chignolin-12-600", "sparse-10-64")       # two launches, the second fed the first one's own s_out / v_out


# ----------------------------------------------------------------------------------------------------------- graphs
SILENT, FAR = 7, 8


def silent_source_graph(seed: int = 0):
    """n = 9.  Nodes 0 .. 6: random beads in a 4 A box, every ordered pair an edge.  Node 7 (``SILENT``) lies in the box
    and RECEIVES from each of them but sends nothing (no edge names it as a source).  Node 8 (``FAR``) lies 12 A beyond
    the box and is joined to node 0 alone, in both directions, by edges longer than the 9.5 A filter cutoff: their filter
    is exactly zero, so node 8 has edges but neither receives nor sends anything."""
    gen = torch.Generator().manual_seed(3000 + seed)
    xyz = torch.rand(9, 3, generator=gen) * 4.0
    xyz[FAR] = xyz[0] + torch.tensor([12.0, 3.0, 1.0])
    pairs = [(i, j) for i in range(7) for j in range(7) if i != j] + [(SILENT, j) for j in range(7)] + [(0, FAR), (FAR, 0)]
    nbrs = torch.tensor(pairs, dtype=torch.long)
    return xyz, nbrs[torch.randperm(nbrs.shape[0], generator=gen)]


def graph(case: Case, seed: int):
    """(xyz fp32 [n, 3], directed (receiver, source) list [E, 2]) of a case."""
    if case.graph in ("dense", "sparse"):
        return D.bead_graph(case.n, case.graph, seed=seed)
    if case.graph == "pair":                                 # EdgePlan.from_nbrs takes any directed list
        assert case.n == 2
        return torch.tensor([[0.3, 0.1, 0.2], [2.1, 1.4, 0.9]]), torch.tensor([[0, 1]], dtype=torch.long)
    if case.graph == "silent":
        assert case.n == 9
        return silent_source_graph(seed)
    raise ValueError(case.graph)


def in_degrees(nbrs, n):
    return torch.bincount(nbrs[:, 0], minlength=n).tolist()


def out_degrees(nbrs, n):
    return torch.bincount(nbrs[:, 1], minlength=n).tolist()


def capacity(case: Case, n_edges: int) -> int:
    """The plan's capacity argument: as graph.BatchGraph reserves it for edge_slack, 0 = exactly the edges."""
    return int(n_edges * (1.0 + case.slack)) + 64 if case.slack > 0 else 0


# ------------------------------------------------------------------------------------- the launchers' rules, restated
KernelPath = namedtuple("KernelPath", "msg_bwd_slices msg_bwd_qs dense_bwd_slices block_channels")


def block_channels(width: int, fat: int = 1) -> int:
    """cgv_decoder_block_channels: 8 when the width is a multiple of 8 and decoder_fat is on, else 4."""
    return 8 if width % 8 == 0 and fat != 0 else 4


def qs_class(n_slices: int) -> int:
    """CGV_DL_QS: slices per lane class of a slice sum, 3 up to 108 slices, else 6."""
    return 3 if n_slices <= QS_BOUNDARY else 6


def kernel_path(case: Case) -> KernelPath:
    """Slices handed to ``prior_msg_bwd_k`` by the layer above (= F / block channels, written by dense_bwd; 0 for a
    one-layer loop, whose only launch gets the dense upstream gradient: the launcher then takes QS = 3), its QS class, the
    slices into ``dec_dense_bwd_k`` (one per four-channel block of the message backward: F / 4) and the block width."""
    cb = block_channels(case.F, case.options.get("decoder_fat", 1))
    n_msg = case.F // cb if case.layers > 1 else 0
    return KernelPath(n_msg, qs_class(max(n_msg, 1)), case.F // 4, cb)


# --------------------------------------------------------------------------------------------- inputs and parameters
def layer_keys(layer: int, prefix: str = PREFIX):
    """Oracle names of the six tensors per layer, in ``prior_fused.layer_params`` order (W1 b1 W2 b2 Wd bd)."""
    return D.layer_keys(layer, prefix)[:6]


def params(F: int, R: int, layers: int, bias_std: float = 0.1):
    """fp32 parameters of the loop under the oracle's names: Xavier-uniform weights as ``Dense`` draws them
    (modules.py:75-101); the (there zero) biases are drawn too, so that no bias gradient is taken around zero."""
    gen = torch.Generator().manual_seed(7000 + 7 * F + R)
    P = {}
    for l in range(layers):
        kW1, kb1, kW2, kb2, kWd, kbd = layer_keys(l)
        for kw, kb, (fo, fi) in ((kW1, kb1, (F, F)), (kW2, kb2, (3 * F, F)), (kWd, kbd, (3 * F, R))):
            P[kw] = (2.0 * torch.rand(fo, fi, generator=gen) - 1.0) * (6.0 / (fo + fi)) ** 0.5
            P[kb] = torch.randn(fo, generator=gen) * bias_std
    return P


def inputs(n: int, F: int, seed: int):
    """Dense random h and upstream weight up of the loop; dense a1, s, v (sigma 0.5) of the forward kernel and a second
    a1 for the second launch of a chain."""
    gen = torch.Generator().manual_seed(8000 + seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    return dict(h=r(n, F), up=r(n, F), a1=r(n, F), s=r(n, F), v=0.5 * r(n, F, 3), a1b=r(n, F))


Setup = namedtuple("Setup", "case xyz nbrs inp P")
_SETUP = {}


def setup(name: str) -> Setup:
    """Graph, inputs and parameters of a case: functions of (n, F, R, layers, graph) alone, so the option and slack
    variants of a shape share them -- and the reference."""
    case = CASES[name]
    key = ref_key(name)
    if key not in _SETUP:
        xyz, nbrs = graph(case, seed=case.n + case.F)
        _SETUP[key] = (xyz, nbrs, inputs(case.n, case.F, seed=case.n + case.F), params(case.F, case.R, case.layers))
    return Setup(case, *_SETUP[key])


def ref_key(name: str):
    """What the reference depends on (no launcher option, no slack)."""
    c = CASES[name]
    return (c.n, c.F, c.R, c.layers, c.graph)


# ------------------------------------------------------------------------------------------------------- reference
def prior_loop(xyz, nbrs, h, v, P, n_layers, R, cutoff=CUTOFF, keep=None, prefix=PREFIX):
    """(h, v) after ``n_layers`` message blocks (cgvae.py:388-392 from the given state; dtype = that of the inputs and of
    ``P``).  ``keep``: a list that receives (h_l, v_l, phi_l) per layer: the state AFTER layer l and its node features
    ``inv_dense(h_{l-1})`` (conv.py:69), the ``phi`` the forward kernel stores for the backward."""
    r_ij = xyz[nbrs[:, 1]] - xyz[nbrs[:, 0]]
    for k in range(n_layers):
        blk = f"{prefix}.message_blocks.{k}"
        ds, dv = O.equi_message_block(h, v, r_ij, nbrs, P, blk, O.swish, R, cutoff)
        if keep is not None:
            phi = O.inv_dense(h, P, blk + ".inv_message.inv_dense", O.swish)
            keep.append((h + ds, v + dv, phi))
        h = h + ds
        v = v + dv
    return h, v


def run_loop_reference(name: str, dtype=torch.float64):
    """Forward + backward of ``(h_out * up).sum()`` in ``dtype``: {"h_out", "layers": [(h_l, v_l, phi_l)], "gh",
    "grads": {oracle key: gradient}}; a gradient autograd leaves out is an exact zero."""
    st = setup(name)
    c = st.case
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in st.P.items()}
    h = st.inp["h"].detach().to(dtype).requires_grad_(True)             # (detach: a new tensor object even when dtype is fp32)
    v0 = torch.zeros(c.n, c.F, 3, dtype=dtype)
    keep = []
    h_out, _ = prior_loop(st.xyz.to(dtype), st.nbrs, h, v0, P, c.layers, c.R, keep=keep)
    (h_out * st.inp["up"].to(dtype)).sum().backward()
    grad = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(h_out=h_out.detach(), layers=[tuple(t.detach() for t in lay) for lay in keep], gh=grad(h),
                grads={k: grad(P[k]) for l in range(c.layers) for k in layer_keys(l)})


def _identity(x):
    return x


def kernel_params(P, layer: int, F: int, dtype):
    """The layer's parameters with the first Dense replaced by the identity: with the identity activation
    ``O.inv_dense(a1, ...)`` is then ``a1 W2^T + b2`` with ``a1`` taken as given (x * 1 + 0 is exact in every format)."""
    kW1, kb1 = layer_keys(layer)[:2]
    Q = {k: v.to(dtype) for k, v in P.items()}
    Q[kW1], Q[kb1] = torch.eye(F, dtype=dtype), torch.zeros(F, dtype=dtype)
    return Q


def run_kernel_reference(name: str, dtype=torch.float64, n_launches: int = 1):
    """What ``n_launches`` chained ``cgv_prior_msg_fwd`` launches compute (layer l's parameters, launch 0 on a1 / s / v,
    launch 1 on a1b and launch 0's s_out / v_out): per launch {"phi", "s_out", "v_out", "dv_unit", "dv_vj"}; the last two
    are the two terms of dv on their own (the block with v = 0 gives the unit term alone)."""
    st = setup(name)
    c = st.case
    assert n_launches <= c.layers
    xyz = st.xyz.to(dtype)
    r_ij = xyz[st.nbrs[:, 1]] - xyz[st.nbrs[:, 0]]
    s, v = st.inp["s"].to(dtype), st.inp["v"].to(dtype)
    out = []
    for l, a1 in zip(range(n_launches), (st.inp["a1"].to(dtype), st.inp["a1b"].to(dtype))):
        Q = kernel_params(st.P, l, c.F, dtype)
        blk = f"{PREFIX}.message_blocks.{l}"
        phi = O.inv_dense(a1, Q, blk + ".inv_message.inv_dense", _identity)
        ds, dv = O.equi_message_block(a1, v, r_ij, st.nbrs, Q, blk, _identity, c.R, CUTOFF)
        _, dv_unit = O.equi_message_block(a1, torch.zeros_like(v), r_ij, st.nbrs, Q, blk, _identity, c.R, CUTOFF)
        s, v = s + ds, v + dv
        out.append(dict(phi=phi, s_out=s, v_out=v, dv_unit=dv_unit, dv_vj=dv - dv_unit))
    return out


_REF = {}             # (kind, ref_key, dtype) -> reference, computed once and left unchanged


def loop_reference(name: str, dtype=torch.float64):
    key = ("loop", ref_key(name), dtype)
    if key not in _REF:
        _REF[key] = run_loop_reference(name, dtype)
    return _REF[key]


def kernel_reference(name: str, dtype=torch.float64, n_launches: int = 1):
    key = ("kernel", n_launches, ref_key(name), dtype)
    if key not in _REF:
        _REF[key] = run_kernel_reference(name, dtype, n_launches)
    return _REF[key]


def compared(res, case: Case):
    """The tensors of a loop result in the order they are compared: h_out, grad h_in, the six parameter gradients of every
    layer, and the three filter slices of each [3F, .] tensor on their own."""
    F = case.F
    items = [("h_out", res["h_out"]), ("grad h_in", res["gh"])]
    for l in range(case.layers):
        for nm, key in zip(NAMES, layer_keys(l)):
            g = res["grads"][key]
            items.append((f"layer {l} grad {nm}", g))
            if nm in FILTERED:
                items += [(f"layer {l} grad {nm} q{k}", g[k * F:(k + 1) * F]) for k in range(3)]
    return items


def compared_kernel(res):
    """The tensors of a forward-kernel result: phi slice by slice, s_out, v_out (per launch of a chain)."""
    items = []
    for l, lay in enumerate(res):
        F = lay["s_out"].shape[1]
        items += [(f"launch {l} phi q{k}", lay["phi"][:, k * F:(k + 1) * F]) for k in range(3)]
        items += [(f"launch {l} s_out", lay["s_out"]), (f"launch {l} v_out", lay["v_out"])]
    return items


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref| (the norm of tests/test_hip_parity.py)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30)) if ref.numel() else 0.0
