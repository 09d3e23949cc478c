"""The cases of tests/test_equi_message_fp64.py are what they claim -- shown with the reference alone, no GPU.

Degree lists and the side of every graph against the launchers' thresholds (3 n / 16 n of the forward, 48 n of the
backward); nodes per chunk, chunks and partial sums of the three chunk cases by the restated ``bwd_shape``; which template
instances of csrc/equi_msg.hip and csrc/equi_msg_grp.hip the run table reaches (``equi_message_cases.kernel_paths``); that
the float64 reference is exactly zero where the GPU test demands exact zeros (a dead term elsewhere would pass any
comparison trivially: the live slices are checked to be live); and that the inputs are well conditioned: the oracle in fp32
is within REL of its fp64 run on every compared tensor, so the hard gate cannot fail because of the reference alone."""
import pytest
import torch

import equi_message_cases as C

REL = 1e-4            # tests/test_hip_parity.py (BASELINE.json's criterion)


def test_box_graph_splits_the_forward_and_walks_the_backward():
    g = C.graph("box")
    n, E = g.n_src, g.nbrs.shape[0]
    assert n == 23 == g.n_dst and n <= 64 and 3 * n <= E < 16 * n and E < 48 * n
    assert min(C.in_degrees(g)) >= 1 and C.in_degrees(g) == C.out_degrees(g)
    assert float((g.pos_src[g.nbrs[:, 0]] - g.pos_src[g.nbrs[:, 1]]).norm(dim=1).max()) <= 3.0 < g.cutoff
    assert sorted({R for _, R in C.WIDTHS}) == [4, 6, 8, 10, 12, 16, 20]                             # every compiled n_rbf
    assert [F for F, _ in C.WIDTHS if F % 2] == [1, 7, 129] and {1, 4, 130, 600} <= {F for F, _ in C.WIDTHS}
    assert [F for F, _ in C.WIDTHS if 0 < F % 128 <= 2] == [1, 130, 129]                             # last channel tile nearly empty
    assert [F for F, _ in C.WIDTHS].count(600) == 1 == [r.F for r in C.RUNS].count(600)


def test_walk_segment_graph_has_the_stated_degrees():
    g = C.graph("segments-walk")
    n, E = g.n_src, g.nbrs.shape[0]
    deg, out = C.in_degrees(g), C.out_degrees(g)
    assert n == 70 and E == 360 == sum(C.LADDER) and E < 16 * n and n > 64                        # forward and backward walk
    assert out[:13] == [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129] and all(d == 0 for d in out[13:])
    assert deg[g.named["only_in"]] > 0 and out[g.named["only_in"]] == 0
    assert deg[g.named["isolated"]] == 0 and out[g.named["isolated"]] == 0
    hub = g.nbrs[g.nbrs[:, 1] == g.named["hub129"]]
    assert hub.shape[0] == 129 and len({tuple(e) for e in hub.tolist()}) < 129                      # repeated edges
    for j in (9, 10, 11):
        seg = g.nbrs[g.nbrs[:, 1] == j]
        assert len({tuple(e) for e in seg.tolist()}) == seg.shape[0]                                 # 63 .. 65 distinct receivers
    assert bool((g.nbrs[:, 0] != g.nbrs[:, 1]).all())
    assert not bool((g.nbrs[1:, 1] >= g.nbrs[:-1, 1]).all())                                        # not handed over sorted


def test_split_segment_graph_has_the_stated_degrees():
    g = C.graph("segments-split")
    n, E = g.n_src, g.nbrs.shape[0]
    deg, out = C.in_degrees(g), C.out_degrees(g)
    assert n == 16 and E == 820 >= 48 * n and E < 200 * n
    assert out == [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129, 200, 260, 0]
    assert deg[g.named["isolated"]] == 0 and deg[g.named["only_in"]] > 0
    assert bool((g.nbrs[:, 0] != g.nbrs[:, 1]).all())
    # slices of ceil(len / 4) edges: segments of 1, 2, 3, 5 and 9 edges leave waves without an edge
    assert [d for d in out[:13] if 0 < d and 3 * -(-d // 4) >= d] == [1, 2, 3, 5, 9]
    sh = C.bwd_shape(n, E)
    assert sh.split and sh.npc == 1 and sh.n_chunks == 16 and 8 * sh.cpx <= 512                   # the matrix-core kernel pays by rule


def test_geometry_graphs():
    g = C.graph("geometry:coincident-far")
    assert g.n_src == 9 and torch.equal(g.pos_src[0], g.pos_src[1])
    d = (g.pos_src[g.nbrs[:, 0]] - g.pos_src[g.nbrs[:, 1]]).norm(dim=1)
    assert int((d == 0).sum()) == 2 and int((d > g.cutoff).sum()) == 2 and float(d.max()) > 50.0
    far = g.named["far"]
    touching = g.nbrs[(g.nbrs == far).any(dim=1)]
    assert sorted(touching.tolist()) == [[0, far], [far, 0]]
    assert C.graph("geometry:empty").nbrs.shape == (0, 2)


def test_chunk_graphs_leave_the_minimum_chunking():
    shapes = {}
    for name in C.CHUNK_CASES:
        g = C.graph(name)
        shapes[name] = (g, C.bwd_shape(g.n_src, g.nbrs.shape[0]))
        assert bool((g.nbrs[:, 0] != g.nbrs[:, 1]).all()) and int(g.nbrs.max()) == g.n_src - 1
    g, sh = shapes["chunks:split-130"]
    assert g.n_src == 130 and g.nbrs.shape[0] >= 48 * 130
    assert sh == C.BwdShape(True, 1, 130, 17, 136)
    assert C.reduce_trips(sh.n_chunks) == 2 and 0 < sh.n_chunks - C.RED_TRIP < C.RED_TRIP // 8      # second trip: 8 of 128 chunks valid
    g, sh = shapes["chunks:split-701"]
    assert g.n_src == 701 and g.nbrs.shape[0] >= 48 * 701
    assert sh == C.BwdShape(True, 2, 351, 44, 352)
    assert g.n_src - (sh.chunks - 1) * sh.npc == 1 and sh.n_chunks - sh.chunks == 1                # last chunk: one node; one padding chunk
    assert C.reduce_trips(sh.n_chunks) == 3
    g, sh = shapes["chunks:walk-1541"]
    E = g.nbrs.shape[0]
    assert g.n_src == 1541 and E < 48 * 1541 and 2.8 <= E / 1541 <= 3.2 and E < 16 * 1541
    assert sh == C.BwdShape(False, 5, 309, 39, 312)
    assert sh.npc > C.BWD_WAVES and g.n_src - (sh.chunks - 1) * sh.npc == 1 and C.reduce_trips(sh.n_chunks) == 3
    out = C.out_degrees(g)
    assert min(out) == 0 and max(out) == 6
    # the smallest sizes that do: one node fewer keeps the minimum nodes per chunk (701: the smallest with a one-node last chunk
    # AND a padding chunk beyond two trips)
    assert C.bwd_shape(384, 48 * 384).npc == 1 and C.bwd_shape(385, 48 * 385).npc == 2
    assert C.bwd_shape(1536, 0).npc == 4 and C.bwd_shape(1537, 0).npc == 5
    assert C.reduce_trips(C.bwd_shape(128, 48 * 128).n_chunks) == 1 and C.reduce_trips(C.bwd_shape(129, 48 * 129).n_chunks) == 2
    assert {r.F for r in C.RUNS if r.case.startswith("chunks:")} == {8, 130}


def test_bipartite_graph():
    g = C.graph("bipartite")
    assert (g.n_src, g.n_dst) == (37, 5) and g.nbrs.shape[0] == 37
    assert C.in_degrees(g) == [9, 1, 0, 20, 7] and C.out_degrees(g) == [1] * 37
    assert not bool((g.mapping[1:] >= g.mapping[:-1]).all())
    assert all("fwd_dv1_split4" in p for r in C.RUNS_BIPARTITE for p in C.kernel_paths(r) if p.startswith("fwd"))


def test_every_kernel_instance_is_reached_by_the_run_table():
    reached = {}
    for r in C.RUNS:
        for p in C.kernel_paths(r):
            reached.setdefault(p, []).append(C.run_id(r))
    assert sorted(reached) == sorted(C.PATHS), sorted(set(C.PATHS) - set(reached))
    assert len(C.PATHS) == 21 == len(set(C.PATHS))
    assert len(C.RUNS) == len(set(C.RUNS)) == len({C.run_id(r) for r in C.RUNS})
    paths = lambda *a, **k: C.kernel_paths(C.run(*a, **k))
    # n_rbf = 16 / 20 with a scalar-only upstream on a split graph stays off the matrix-core kernel; n_rbf = 10 takes it
    assert C.run("segments-split", 8, 16, "ds") in C.RUNS and "bwd_gv0_split1_pair1" in paths("segments-split", 8, 16, "ds")
    assert "bwd_mfma" in paths("segments-split", 8, 10, "ds") and "bwd_mfma" in paths("chunks:split-701", 8, 10, "ds")
    assert "bwd_gv0_split1_pair0" in paths("segments-split", 7, 10, "ds")                        # F % 4: off it too
    # arm "dv" (gs == nullptr) on both sides of the split and pair switches
    dv = {p for r in C.RUNS if r.arm == "dv" for p in C.kernel_paths(r) if p.startswith("bwd")}
    assert dv == {f"bwd_gv1_split{s}_pair{p}" for s in (0, 1) for p in (0, 1)}
    # the pipelined scalar-only walk (PAIR, no gv) on the graph built for its batches, and on the five-node chunks
    assert "bwd_gv0_split0_pair1" in paths("segments-walk", 8, 10, "ds") and "bwd_gv0_split0_pair1" in paths("chunks:walk-1541", 8, 8, "ds")
    # every chunk case under all three arms, one of them deferred, and in the determinism list
    for name in C.CHUNK_CASES:
        assert {r.arm for r in C.RUNS if r.case == name} == set(C.ARMS)
        assert any(r.case == name for r in C.DETERMINISM_RUNS)
    assert any(r.case.startswith("chunks:") for r in C.RUNS_DEFERRED)
    assert all("reduce_jobs" in C.kernel_paths(r) for r in C.RUNS_DEFERRED)
    assert {C.k_live(r) for r in C.RUNS_DEFERRED} == {1, 3}
    assert all(r.F % 4 == 0 for r in C.RUNS_DEFERRED)                      # (other widths pad their Dense operands outside the arena)
    assert all(r in C.RUNS for r in C.DETERMINISM_RUNS)
    assert any("hub260" in C.graph(r.case).named for r in C.DETERMINISM_RUNS)
    # the vector channel is skipped only under the scalar-only loss
    assert all(r.arm == "ds" for r in C.RUNS if not r.with_dv)


def test_option_pairs_differ_in_one_option_and_say_where_the_kernels_differ():
    same = []
    for a, b in C.OPTION_PAIRS:
        assert C.ref_key(a) == C.ref_key(b) and a.deferred == b.deferred and a.with_dv == b.with_dv
        assert sum(getattr(a, k) != getattr(b, k) for k in C.OPTION_NAMES) == 1
        same.append(C.kernel_paths(a) == C.kernel_paths(b))
    assert same == [False, True, False, False, False, False, False, True]
    a, b = C.OPTION_PAIRS[0]
    assert C.kernel_paths(a) - C.kernel_paths(b) == {"bwd_mfma"}
    a, b = C.OPTION_PAIRS[3]
    assert (C.kernel_paths(a) - C.kernel_paths(b), C.kernel_paths(b) - C.kernel_paths(a)) == ({"fwd_grp2"}, {"fwd_grp4"})


_KEYS = list(dict.fromkeys(C.ref_key(r) for r in C.RUNS))
_BY_KEY = {C.ref_key(r): r for r in C.RUNS}
_IDS = ["|".join(str(x) for x in k) for k in _KEYS]


@pytest.mark.parametrize("key", _KEYS, ids=_IDS)
def test_reference_is_exactly_zero_where_the_kernels_must_be_and_live_elsewhere(key):
    r = _BY_KEY[key]
    g = C.graph(r.case)
    ref = C.reference(r)
    assert all(t.dtype == torch.float64 and bool(torch.isfinite(t).all()) for part in ref.values() for t in part.values())
    names = list(ref["gpar"])
    E = g.nbrs.shape[0]
    for k in names[-C.N_FILTERED:]:                                       # absent arm: its filter slices get an exact zero
        peaks = C.filter_slice_max(ref["gpar"][k], r.F)
        for q in range(3):
            if q in C.ALIVE[r.arm] and E and r.case != "geometry:empty":
                assert peaks[q] > 0.0, (k, q)
            else:
                assert peaks[q] == 0.0, (k, q)
    if r.arm == "ds":
        assert float(ref["gin"]["v"].abs().max()) == 0.0
    if E == 0:
        inp, _ = C.run_inputs(r)
        for k, x in zip(C.OUTS, ("s", "v")):
            want = inp[x].double() if r.residual else torch.zeros_like(ref["out"][k])
            assert torch.equal(ref["out"][k], want)
        assert all(float(t.abs().max()) == 0.0 for t in ref["gpar"].values())
        return
    # sources without an outgoing edge: exact zero rows of the input gradients (through g_phi, g_v); with the residual the
    # upstream weight passes straight through instead
    silent = [j for j, d in enumerate(C.out_degrees(g)) if d == 0]
    deaf = [i for i, d in enumerate(C.in_degrees(g)) if d == 0]
    far = g.named.get("far")
    if far is not None:
        silent, deaf = silent + [far], deaf + [far]                       # its only edges lie beyond the cutoff
    own_residual = r.residual and g.mapping is None
    inp, _ = C.run_inputs(r)
    for j in silent:
        for k, u in (("s", "u0"), ("v", "u1")):
            want = inp[u][j].double() if own_residual and C.OUTS.index("ds" if k == "s" else "dv") in C.ARMS[r.arm] else 0.0 * inp[u][j].double()
            assert torch.equal(ref["gin"][k][j], want), (k, j)
    if not r.residual:
        for i in deaf:
            assert float(ref["out"]["ds"][i].abs().max()) == 0.0 and float(ref["out"]["dv"][i].abs().max()) == 0.0
    live = [j for j, d in enumerate(C.out_degrees(g)) if d > 0 and j != far]
    assert float(ref["gin"]["s"][live].abs().min(dim=1).values.max()) > 0.0


@pytest.mark.parametrize("key", _KEYS, ids=_IDS)
def test_inputs_are_well_conditioned_in_float32(key):
    """err_fp32_oracle <= REL on every compared tensor (per-slice comparisons included), and the fp32 oracle is exactly zero
    where the fp64 one is."""
    r = _BY_KEY[key]
    r64, r32 = C.reference(r), C.reference(r, torch.float32)
    worst = (0.0, "")
    for (what, a), (_, b) in zip(C.compared(r64, r.F), C.compared(r32, r.F)):
        assert b.dtype == torch.float32 and a.dtype == torch.float64
        if a.numel() == 0 or float(a.abs().max()) == 0.0:
            assert b.numel() == 0 or float(b.abs().max()) == 0.0, f"{what}: the fp32 oracle is non-zero where fp64 is exactly zero"
            continue
        worst = max(worst, (C.rel_err(b, a), what))
    assert worst[0] <= REL, f"{key}: fp32 oracle off by {worst[0]:.3e} at {worst[1]}"
