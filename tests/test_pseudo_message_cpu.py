"""The cases of tests/test_pseudo_message_fp64.py are what they claim -- shown with the reference alone, no GPU.

Degree lists and the E-versus-16n side of every graph; which kernels of csrc/pseudo_msg.hip the run table reaches (by the
launcher's rule restated in ``pseudo_message_cases.kernel_paths``); that no term of the message is dead under the full
loss and exactly which are under each one-sided loss (a dead term would pass any comparison trivially); and that the
inputs are well conditioned: the oracle in fp32 is within REL / 10 of its fp64 run on every compared tensor."""
import pytest
import torch

import pseudo_message_cases as C

REL = 1e-4            # tests/test_hip_parity.py (BASELINE.json's criterion)


def test_width_graph_is_on_the_general_side_and_covers_every_rbf_count():
    g = C.case("width:65-8").graph
    assert g.n == 23 and 0 < g.nbrs.shape[0] < 16 * g.n
    assert min(C.in_degrees(g)) >= 1
    assert float((g.xyz[g.nbrs[:, 0]] - g.xyz[g.nbrs[:, 1]]).norm(dim=1).max()) <= 3.0 < g.cutoff
    assert sorted({R for _, R in C.WIDTHS}) == [4, 6, 8, 10, 12, 16, 20]
    assert [(F, R) for F, R in C.WIDTHS if (F * R) % 4] == [(7, 6), (7, 10), (129, 10)]             # filter rows not stageable
    assert [F for F, _ in C.WIDTHS if F % 64 == 1] == [1, 65, 129]                               # one live lane in the last block


@pytest.mark.parametrize("n,F", C.CHUNKS)
def test_sparse_graphs_have_about_two_incoming_edges(n, F):
    g = C.case(f"chunk:{n}-{F}").graph
    deg = C.in_degrees(g)
    assert g.n == n and set(deg) <= {1, 2, 3} and 1.5 <= sum(deg) / n <= 2.2
    assert g.nbrs.shape[0] < 16 * n and bool((g.nbrs[:, 0] != g.nbrs[:, 1]).all())


def test_chunking_and_launch_size_switch():
    chunks = {n: C.pseudo_chunks(n) for n, _ in C.CHUNKS}
    assert chunks == {12: 12, 64: 64, 65: 24, 97: 24, 257: 64, 300: 64, 5: 5}
    nodes_per_chunk = {n: -(-n // c) for n, c in chunks.items()}
    assert nodes_per_chunk[65] == 3 and nodes_per_chunk[97] == 5 and nodes_per_chunk[257] == 5 and nodes_per_chunk[300] == 5
    for n in (65, 97):                         # tail chunks without a node
        assert (chunks[n] - 1) * nodes_per_chunk[n] >= n
    blocks = {(n, F): n * ((F + 63) // 64) for n, F in C.CHUNKS}
    assert blocks[(12, 64)] == 12 and blocks[(64, 8)] == 64 and blocks[(5, 320)] == 25
    assert blocks[(257, 8)] > 256 and blocks[(300, 8)] > 256
    for n, F in C.CHUNKS:
        want = "fwd_narrow" if n > 256 else "fwd_wide"
        paths = C.kernel_paths(n, F, C.case(f"chunk:{n}-{F}").graph.nbrs.shape[0])
        assert want in paths and ("recv_narrow" if n > 256 else "recv_wide") in paths and "src_plain" in paths


def test_general_segment_graph_has_the_stated_degrees():
    g = C.case("segments-general").graph
    deg, out = C.in_degrees(g), C.out_degrees(g)
    assert g.n == 140 and g.nbrs.shape[0] == 450 < 16 * g.n
    assert [deg[k] for k in range(11)] == [0, 1, 2, 3, 7, 8, 9, 16, 17, 130, 257]
    assert deg[C.ONLY_OUT] == 0 and out[C.ONLY_OUT] > 0
    assert deg[0] == 0 and out[0] == 0                                    # isolated
    assert all(d == 0 for d in deg[11:])
    hub = g.nbrs[g.nbrs[:, 0] == 10]
    assert len({tuple(e) for e in hub.tolist()}) < hub.shape[0]           # duplicated edges
    assert bool((g.nbrs[:, 0] != g.nbrs[:, 1]).all())
    assert not bool((g.nbrs[1:, 0] >= g.nbrs[:-1, 0]).all())              # not handed over sorted


def test_dense_segment_graph_has_the_stated_degrees():
    g = C.case("segments-dense:24-10").graph
    deg, out = C.in_degrees(g), C.out_degrees(g)
    assert g.n == 24 and g.nbrs.shape[0] == 423 >= 16 * g.n
    assert [deg[k] for k in range(10)] == [0, 1, 3, 4, 5, 7, 8, 9, 129, 257]
    assert all(d == 0 for d in deg[10:])
    assert out[C.HEAVY_SOURCE] > 128                                      # pass B crosses a 128-edge index chunk too
    assert bool((g.nbrs[:, 0] != g.nbrs[:, 1]).all())
    for F, R in C.DENSE_SHAPES:
        assert C.case(f"segments-dense:{F}-{R}").graph is g


def test_geometry_graphs():
    g = C.case("geometry:coincident-far").graph
    assert g.n == 9 and torch.equal(g.xyz[0], g.xyz[1])
    d = (g.xyz[g.nbrs[:, 0]] - g.xyz[g.nbrs[:, 1]]).norm(dim=1)
    assert int((d == 0).sum()) == 2 and int((d > g.cutoff).sum()) == 2 and float(d.max()) > 50.0
    assert g.nbrs.shape[0] != 3                       # (torch.cross of the reference takes the FIRST axis of size 3)
    assert C.case("geometry:empty").graph.nbrs.shape == (0, 2)


def test_every_kernel_path_is_reached_by_the_run_table():
    reached = {}
    for run in C.RUNS:
        for p in C.run_paths(run):
            reached.setdefault(p, []).append(C.run_id(run))
    assert sorted(reached) == sorted(C.PATHS), sorted(set(C.PATHS) - set(reached))
    # the variants that stage 128-edge chunks run on the graph whose hubs cross one and two chunk boundaries
    general = {r.variant: C.run_paths(r) for r in C.RUNS_GENERAL}
    assert sorted(general) == list(range(7))
    assert [v for v, p in general.items() if "fwd_staged" in p] == [2, 3, 4, 6]
    dense = {r.variant: C.run_paths(r) for r in C.RUNS_DENSE if r.case == "segments-dense:65-20"}
    assert dense[0] >= {"fwd_dense", "recv_dense", "src_dense"} and "src_staged" in dense[2]
    assert "src_8" in dense[4] and "src_plain" in dense[5] and "fwd_wide" in dense[5]
    assert all("deferred_reduce" in C.run_paths(r) for r in C.RUNS_DEFERRED)
    assert len(C.RUNS) == len(set(C.RUNS))


@pytest.mark.parametrize("name", C.WIDTH_CASES + C.CHUNK_CASES + ["segments-general"] + C.DENSE_CASES + ["geometry:coincident-far"])
def test_every_term_is_live_under_the_full_loss(name):
    c = C.case(name)
    ref = C.reference(name)
    for key in (C.PARAMS[2], C.PARAMS[4]):
        blocks = C.filter_block_max(ref["gpar"][key], c.F)
        assert all(b > 0.0 for b in blocks), f"{name}: dead filter in {key}: {blocks}"
    for key in C.PARAMS:
        assert float(ref["gpar"][key].abs().max()) > 0.0, f"{name}: {key} has a zero gradient"
    for key in C.INS:
        assert float(ref["gin"][key].abs().max()) > 0.0
    assert all(t.dtype == torch.float64 for part in ref.values() for t in part.values())


@pytest.mark.parametrize("arm", [a for a in C.ARMS if a != "all"])
@pytest.mark.parametrize("name", C.ARM_CASES)
def test_one_sided_losses_keep_exactly_the_stated_filters_alive(name, arm):
    c = C.case(name)
    for residual in (False, True):
        ref = C.reference(name, arm, residual)
        for key in C.FILTERED:
            blocks = C.filter_block_max(ref["gpar"][key], c.F)
            for k in range(9):
                if k in C.ALIVE[arm]:
                    assert blocks[k] > 0.0, (name, arm, key, k)
                else:
                    assert blocks[k] == 0.0, (name, arm, key, k)
        node_mlp_alive = bool(C.ALIVE[arm])
        for key in C.PARAMS[:2]:
            assert (float(ref["gpar"][key].abs().max()) > 0.0) == node_mlp_alive
    # dhbar alone: no filter and no parameter is involved; the state still gets v_i . vbar_j's gradient
    if arm == "dhbar":
        ref = C.reference(name, arm, False)
        assert float(ref["gin"]["s"].abs().max()) == 0.0 and float(ref["gin"]["sbar"].abs().max()) == 0.0
        assert float(ref["gin"]["v"].abs().max()) > 0.0 and float(ref["gin"]["vbar"].abs().max()) > 0.0
        res = C.reference(name, arm, True)
        inp, _ = C.case_inputs(c)
        assert torch.equal(res["gin"]["sbar"], inp["u1"].double())           # straight through the residual


def test_isolated_nodes_and_the_empty_graph_give_exact_zeros():
    g = C.case("segments-general").graph
    ref = C.reference("segments-general")
    for k in C.OUTS:
        assert float(ref["out"][k][g.named["isolated"]].abs().max()) == 0.0
        assert float(ref["out"][k][g.named["only_out"]].abs().max()) == 0.0
    for k in C.INS:
        assert float(ref["gin"][k][g.named["isolated"]].abs().max()) == 0.0
    far = C.case("geometry:coincident-far").graph.named["far"]
    ref = C.reference("geometry:coincident-far")
    assert float(ref["out"]["dh"][far].abs().max()) == 0.0 and float(ref["out"]["dhbar"][far].abs().max()) > 0.0
    inp, _ = C.case_inputs(C.case("geometry:empty"))
    for residual in (False, True):
        ref = C.reference("geometry:empty", "all", residual)
        for k, x in zip(C.OUTS, C.INS):
            want = inp[x].double() if residual else torch.zeros_like(ref["out"][k])
            assert torch.equal(ref["out"][k], want)
        assert all(float(t.abs().max()) == 0.0 for t in ref["gpar"].values())


_KEYS = sorted({(r.case, r.arm, r.residual) for r in C.RUNS})


@pytest.mark.parametrize("name,arm,residual", _KEYS, ids=[f"{n}|{a}|{int(r)}" for n, a, r in _KEYS])
def test_inputs_are_well_conditioned_in_float32(name, arm, residual):
    """err_fp32_oracle <= REL / 10 on every compared tensor (per-filter row blocks included)."""
    c = C.case(name)
    r64, r32 = C.reference(name, arm, residual), C.reference(name, arm, residual, torch.float32)
    worst = (0.0, "")
    for (what, a), (_, b) in zip(C.compared(r64, c.F), C.compared(r32, c.F)):
        assert b.dtype == torch.float32 and a.dtype == torch.float64
        assert bool(torch.isfinite(a).all())
        if float(a.abs().max()) == 0.0:
            assert float(b.abs().max()) == 0.0, f"{what}: the fp32 oracle is non-zero where fp64 is exactly zero"
            continue
        worst = max(worst, (C.rel_err(b, a), what))
    assert worst[0] <= REL / 10, f"{name} {arm}: fp32 oracle off by {worst[0]:.3e} at {worst[1]}"
