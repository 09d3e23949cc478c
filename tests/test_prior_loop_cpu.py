"""The cases of tests/test_prior_loop_fp64.py are what they claim -- shown with the reference alone, no GPU.

Coverage of the table by the launchers' own rules (``prior_loop_cases.kernel_path``): every compiled n_rbf, both lane
classes of ``prior_msg_bwd_k``'s slice sum and the slice counts on either side of their boundary, the cap of 216 slices,
240 edges and one edge; the degree structure the sparse and silent-source graphs name; liveness, so that no comparison
passes trivially (the q1 rows of the filter tensors get a gradient in every layer, the q0 / q2 rows get exactly none, the
vector state is non-zero from layer 1 on and each of the two terms of dv carries at least ``SHARE`` of max |dv| wherever
v_out is compared); and the yardstick: the oracle loop in fp32 is within REL of its fp64 run on every compared tensor, so
the hard gate is reachable in fp32 arithmetic and cannot fail because of the inputs alone."""
import pytest
import torch
from torch.overrides import TorchFunctionMode

import prior_loop_cases as C
from oracle import cgvae_oracle as O

REL = 1e-4            # tests/test_hip_parity.py (BASELINE.json's criterion)
_KEYS = list(dict.fromkeys(C.ref_key(name) for name in C.CASES))
_BY_KEY = {}
for _name in C.CASES:
    _BY_KEY.setdefault(C.ref_key(_name), _name)
_IDS = [_BY_KEY[k] for k in _KEYS]


class _NoFloat32(TorchFunctionMode):
    """Records every torch call that returns a float32 tensor of one or more dimensions (tests/test_decoder_loop_cpu.py)."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            if torch.is_tensor(t) and t.dtype in (torch.float32, torch.float16, torch.bfloat16) and t.dim() >= 1:
                self.seen.append(getattr(func, "__name__", str(func)))
        return out


def test_table_covers_every_kernel_instance():
    paths = {name: C.kernel_path(c) for name, c in C.CASES.items()}
    assert sorted({c.R for c in C.CASES.values()}) == list(C.RBF_LIST)                    # every compiled n_rbf is run
    assert {p.msg_bwd_qs for p in paths.values()} == {3, 6}
    counts = {p.msg_bwd_slices for p in paths.values()}
    assert {0, 75, 108, 109, 110, 150, 216} <= counts and max(counts) == C.MAX_SLICES
    assert C.qs_class(108) == 3 and C.qs_class(109) == 6
    # the named rows
    assert paths["chignolin-12-600"] == C.KernelPath(75, 3, 150, 8)
    assert paths["chignolin-12-600-thin"] == C.KernelPath(150, 6, 150, 4)
    assert paths["chignolin-12-600-col0"] == paths["chignolin-12-600-col3"] == paths["chignolin-12-600"]
    assert paths["lane3-12-432-thin"] == C.KernelPath(108, 3, 108, 4)
    assert paths["lane6-12-440-thin"] == C.KernelPath(110, 6, 110, 4)
    odd = C.CASES["odd8-8-436"]
    assert odd.F % 8 == 4 and odd.options == {} and paths["odd8-8-436"] == C.KernelPath(109, 6, 109, 4)
    assert paths["widest-8-864-thin"] == C.KernelPath(216, 6, 216, 4)
    assert paths["single-12-128"].msg_bwd_slices == 0 and paths["deep-12-128"].msg_bwd_slices == 16
    assert paths["narrowest-5-16-R4"] == C.KernelPath(2, 3, 4, 8) and C.CASES["narrowest-5-16-R4"].layers == 3
    # both lane classes of dense_bwd's own slice sum (F / 4 slices) too
    assert {C.qs_class(p.dense_bwd_slices) for p in paths.values()} == {3, 6}
    # default options reach QS = 6 only through F % 8 == 4, F >= 436
    assert [n for n, c in C.CASES.items() if not c.options and paths[n].msg_bwd_qs == 6] == ["odd8-8-436"]
    assert C.kernel_path(C.Case(8, 432, 10, 2, "dense", {}, 0.0)).msg_bwd_qs == 3 == C.kernel_path(C.Case(8, 428, 10, 2, "dense", {}, 0.0)).msg_bwd_qs
    # what the launchers accept: n <= 16, F % 4 == 0, 16 <= F <= 864, at most 216 slices, 1 .. 240 edges
    for name, c in C.CASES.items():
        E = C.setup(name).nbrs.shape[0]
        assert 1 <= c.n <= 16 and c.F % 4 == 0 and 16 <= c.F <= 864 and 1 <= E <= C.MAX_EDGES, name
        assert paths[name].msg_bwd_slices <= C.MAX_SLICES and paths[name].dense_bwd_slices <= C.MAX_SLICES, name
    small = {c.R for c in C.CASES.values() if c.n <= 8 and c.F <= 64}
    assert {6, 12, 16} <= small
    assert all(name in C.CASES for name in C.KERNEL_CASES + C.CHAIN_CASES)
    assert all(C.CASES[name].layers >= 2 for name in C.CHAIN_CASES)


def test_edge_counts_and_slack():
    edges = {name: C.setup(name).nbrs.shape[0] for name in C.CASES}
    assert edges["capacity-16-64"] == 240 == C.MAX_EDGES and edges["pair-2-32"] == 1
    for name, c in C.CASES.items():
        if c.graph == "dense":
            assert edges[name] == c.n * (c.n - 1), name
    slack = [name for name, c in C.CASES.items() if c.slack > 0]
    assert sorted(slack) == ["single-12-128-slack", "slack-7-200"]
    for name in slack:
        assert edges[name] < C.capacity(C.CASES[name], edges[name])
    assert C.capacity(C.CASES["slack-7-200"], 42) == 148                   # staged records: 42 real + 106 NaN ones
    assert C.capacity(C.CASES["single-12-128-slack"], 132) > C.MAX_EDGES   # ... and a capacity the kernels clamp to 240
    assert C.ref_key("single-12-128-slack") == C.ref_key("single-12-128")
    assert C.ref_key("slack-7-200") == C.ref_key("rbf20-7-200")


def test_sparse_and_silent_source_graphs_have_the_structure_they_name():
    st = C.setup("sparse-10-64")
    n = st.case.n
    deg, out = C.in_degrees(st.nbrs, n), C.out_degrees(st.nbrs, n)
    assert deg[n - 1] == 0 == out[n - 1] and deg[n - 3] == deg[n - 2] == 1 and min(deg[:n - 3]) >= 2
    assert C.ref_key("sparse-10-64-single")[:3] == C.ref_key("sparse-10-64")[:3]

    st = C.setup("silent-source-9-64")
    n = st.case.n
    deg, out = C.in_degrees(st.nbrs, n), C.out_degrees(st.nbrs, n)
    assert out[C.SILENT] == 0 and deg[C.SILENT] == 7                       # receives from all of the cluster, sends nothing
    assert deg[C.FAR] == 1 == out[C.FAR]
    d = (st.xyz[st.nbrs[:, 0]] - st.xyz[st.nbrs[:, 1]]).norm(dim=1)
    beyond = d > C.CUTOFF
    assert int(beyond.sum()) == 2 and sorted(st.nbrs[beyond].tolist()) == [[0, C.FAR], [C.FAR, 0]]
    assert float(d[~beyond].max()) < 0.8 * C.CUTOFF
    assert not bool((st.nbrs[1:, 0] >= st.nbrs[:-1, 0]).all())              # not handed over sorted
    # the filter of the two long edges is exactly zero in the reference (envelope and basis both cut, modules.py:52-58, 148-172)
    dist = O.preprocess_r((st.xyz[st.nbrs[:, 1]] - st.xyz[st.nbrs[:, 0]]).double())[0]
    P = {k: v.double() for k, v in st.P.items()}
    w = O.distance_embed(dist, P, f"{C.PREFIX}.message_blocks.0.inv_message.dist_embed", st.case.R, C.CUTOFF)
    assert float(w[beyond].abs().max()) == 0.0 and float(w[~beyond].abs().min(dim=1).values.max()) > 0.0

    st = C.setup("pair-2-32")
    assert st.nbrs.tolist() == [[0, 1]] and C.in_degrees(st.nbrs, 2) == [1, 0] and C.out_degrees(st.nbrs, 2) == [0, 1]


def test_reference_stays_in_float64_and_is_the_oracle_prior_loop():
    st = C.setup("rbf6-6-32")
    c = st.case
    P = {k: v.double() for k, v in st.P.items()}
    with _NoFloat32() as watch:
        h, v = C.prior_loop(st.xyz.double(), st.nbrs, st.inp["h"].double(), torch.zeros(c.n, c.F, 3, dtype=torch.float64), P,
                            c.layers, c.R)
    assert h.dtype == torch.float64 and v.dtype == torch.float64
    assert watch.seen == [], f"float32 intermediates in the fp64 reference: {sorted(set(watch.seen))}"
    # in fp32, from an embedding lookup, the helper IS the message-block loop of O.prior_forward (cgvae.py:381-396): the
    # heads are replaced by the identity to read the state
    F = c.F
    Q = dict(st.P)
    Q[C.PREFIX + ".atom_embed.weight"] = torch.randn(100, F, generator=torch.Generator().manual_seed(1))
    eye, zero = torch.eye(F), torch.zeros(F)
    for head in ("mu", "sigma"):
        Q.update({f"{C.PREFIX}.{head}.0.weight": eye, f"{C.PREFIX}.{head}.0.bias": zero, f"{C.PREFIX}.{head}.2.weight": eye,
                  f"{C.PREFIX}.{head}.2.bias": zero})
    cg_z = torch.arange(c.n) % 5 + 1
    und = st.nbrs[st.nbrs[:, 1] > st.nbrs[:, 0]]
    directed, _ = O.make_directed(und)
    hp = O.Hyper(F, c.R, 5.0, C.CUTOFF, c.layers, 1, 6)
    mu, _ = O.prior_forward(cg_z, st.xyz, und, Q, hp)
    h32, _ = C.prior_loop(st.xyz, directed, Q[C.PREFIX + ".atom_embed.weight"][cg_z], torch.zeros(c.n, F, 3), Q, c.layers, c.R)
    assert torch.equal(mu, torch.tanh(h32))


@pytest.mark.parametrize("key", _KEYS, ids=_IDS)
def test_loop_reference_is_live_where_compared_and_exactly_zero_where_the_kernels_must_be(key):
    name = _BY_KEY[key]
    st = C.setup(name)
    c, F = st.case, st.case.F
    ref = C.loop_reference(name)
    assert all(t.dtype == torch.float64 and bool(torch.isfinite(t).all()) for _, t in C.compared(ref, c))
    for l in range(c.layers):
        keys = dict(zip(C.NAMES, C.layer_keys(l)))
        for nm in C.FILTERED:
            g = ref["grads"][keys[nm]]
            assert g.shape[0] == 3 * F
            assert float(g[F:2 * F].abs().max()) > 0.0, f"{name}: layer {l} grad {nm}: the q1 rows are dead"
            assert float(g[:F].abs().max()) == 0.0 and float(g[2 * F:].abs().max()) == 0.0, f"{name}: layer {l} grad {nm}: q0 / q2"
        for nm in ("W1", "b1"):
            assert float(ref["grads"][keys[nm]].abs().max()) > 0.0
        h_l, v_l, phi_l = ref["layers"][l]
        assert h_l.shape == (c.n, F) and v_l.shape == (c.n, F, 3) and phi_l.shape == (c.n, 3 * F)
        assert float(v_l.abs().max()) > 0.0, f"{name}: the vector state is zero after layer {l}"
    assert torch.equal(ref["layers"][-1][0], ref["h_out"])
    # nodes that receive nothing keep their state bit for bit; nodes that send nothing get the upstream weight alone
    deg, out = C.in_degrees(st.nbrs, c.n), C.out_degrees(st.nbrs, c.n)
    deaf = [i for i, d in enumerate(deg) if d == 0] + ([C.FAR] if c.graph == "silent" else [])
    silent = [j for j, d in enumerate(out) if d == 0] + ([C.FAR] if c.graph == "silent" else [])
    if c.graph in ("sparse", "silent", "pair"):
        assert deaf and silent
    for i in deaf:
        assert torch.equal(ref["h_out"][i], st.inp["h"][i].double()), (name, i)
        assert all(float(v_l[i].abs().max()) == 0.0 for _, v_l, _ in ref["layers"])
    for j in silent:
        assert torch.equal(ref["gh"][j], st.inp["up"][j].double()), (name, j)
    live = [j for j, d in enumerate(out) if d > 0 and j not in silent]
    assert float((ref["gh"][live] - st.inp["up"][live].double()).abs().min(dim=1).values.max()) > 0.0


@pytest.mark.parametrize("key", _KEYS, ids=_IDS)
def test_loop_inputs_are_well_conditioned_in_float32(key):
    """err_fp32_oracle <= REL on every compared tensor (per-slice comparisons included), and the fp32 oracle is exactly zero
    where the fp64 one is."""
    name = _BY_KEY[key]
    c = C.CASES[name]
    r64, r32 = C.loop_reference(name), C.loop_reference(name, torch.float32)
    worst = (0.0, "")
    for (what, a), (_, b) in zip(C.compared(r64, c), C.compared(r32, c)):
        assert b.dtype == torch.float32 and a.dtype == torch.float64
        if float(a.abs().max()) == 0.0:
            assert float(b.abs().max()) == 0.0, f"{what}: the fp32 oracle is non-zero where fp64 is exactly zero"
            continue
        worst = max(worst, (C.rel_err(b, a), what))
    print(f"{name} fp32 oracle WORST {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= REL, f"{name}: fp32 oracle off by {worst[0]:.3e} at {worst[1]}"


def _shares(lay):
    top = float((lay["dv_unit"] + lay["dv_vj"]).abs().max())
    return float(lay["dv_vj"].abs().max()) / top, float(lay["dv_unit"].abs().max()) / top


@pytest.mark.parametrize("name", sorted(set(C.KERNEL_CASES + C.CHAIN_CASES)))
def test_forward_kernel_inputs_keep_both_terms_of_dv_alive_and_are_well_conditioned(name):
    """Where v_out of ``prior_msg_fwd_k`` is compared, the v_j term (wave 0) and the unit term (wave 2) each reach
    ``SHARE`` of max |dv| -- in both launches of a chain, whose second one reads the first one's v_out; all three slices of
    phi are non-zero; the fp32 oracle is within REL of its fp64 run on every compared tensor."""
    n_launches = 2 if name in C.CHAIN_CASES else 1
    r64, r32 = C.kernel_reference(name, torch.float64, n_launches), C.kernel_reference(name, torch.float32, n_launches)
    st = C.setup(name)
    for l, lay in enumerate(r64):
        vj, unit = _shares(lay)
        print(f"{name} launch {l}: share of max |dv|: v_j term {vj:.3f} unit term {unit:.3f}")
        assert vj >= C.SHARE and unit >= C.SHARE, (name, l, vj, unit)
        assert all(t.dtype == torch.float64 for t in lay.values())
    assert C.rel_err(r64[0]["v_out"] - st.inp["v"].double(), r64[0]["dv_unit"] + r64[0]["dv_vj"]) <= 1e-14
    worst = (0.0, "")
    for (what, a), (_, b) in zip(C.compared_kernel(r64), C.compared_kernel(r32)):
        assert b.dtype == torch.float32 and float(a.abs().max()) > 0.0, what
        worst = max(worst, (C.rel_err(b, a), what))
    print(f"{name} fp32 oracle WORST {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= REL, f"{name}: fp32 oracle off by {worst[0]:.3e} at {worst[1]}"
    deg = C.in_degrees(st.nbrs, st.case.n)
    for i in [i for i, d in enumerate(deg) if d == 0]:                      # nothing arrives: the state passes through
        assert torch.equal(r64[0]["s_out"][i], st.inp["s"][i].double()) and torch.equal(r64[0]["v_out"][i], st.inp["v"][i].double())


def test_kernel_reference_takes_a1_as_given():
    """The identity first Dense: ``O.inv_dense`` returns ``a1 W2^T + b2`` on the drawn a1, whatever W1 and b1 are."""
    name = "rbf20-7-200"
    st = C.setup(name)
    lay = C.kernel_reference(name)[0]
    keys = dict(zip(C.NAMES, C.layer_keys(0)))
    want = st.inp["a1"].double() @ st.P[keys["W2"]].double().t() + st.P[keys["b2"]].double()
    assert C.rel_err(lay["phi"], want) <= 1e-14


@pytest.mark.parametrize("name", ["chignolin-12-600", "sparse-10-64", "deep-12-128"])
def test_loop_vector_state_carries_both_terms_from_layer_1_on(name):
    """In the loop v enters as zero (cgvae.py:388): layer 0's dv is the unit term alone, and from layer 1 on the v_j term
    reads what the layer below wrote.  Both terms then reach ``SHARE`` of that layer's max |dv|."""
    st = C.setup(name)
    c = st.case
    ref = C.loop_reference(name)
    P = {k: v.double() for k, v in st.P.items()}
    xyz = st.xyz.double()
    r_ij = xyz[st.nbrs[:, 1]] - xyz[st.nbrs[:, 0]]
    h, v = st.inp["h"].double(), torch.zeros(c.n, c.F, 3, dtype=torch.float64)
    for l in range(c.layers):
        blk = f"{C.PREFIX}.message_blocks.{l}"
        _, dv = O.equi_message_block(h, v, r_ij, st.nbrs, P, blk, O.swish, c.R, C.CUTOFF)
        _, dv_unit = O.equi_message_block(h, torch.zeros_like(v), r_ij, st.nbrs, P, blk, O.swish, c.R, C.CUTOFF)
        vj, unit = _shares(dict(dv_unit=dv_unit, dv_vj=dv - dv_unit))
        print(f"{name} layer {l}: share of max |dv|: v_j term {vj:.3f} unit term {unit:.3f}")
        assert (vj == 0.0) if l == 0 else (vj >= C.SHARE), (name, l, vj)
        assert unit >= C.SHARE
        h, v = ref["layers"][l][0], ref["layers"][l][1]
        assert C.rel_err(v, (ref["layers"][l - 1][1] if l else torch.zeros_like(v)) + dv) <= 1e-14
