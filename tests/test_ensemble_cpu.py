"""What the ensemble analyses share (``ensemble``) and the table that drives their switches (``analyses``); no GPU.  The
refusals are matched against the literal messages of the three selection checks that ``ensemble.selection`` replaced."""
import re

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import backmap as bm, ensemble, run_ala
from coarsegrainingvae_amd.analyses import ANALYSES

# the three parameterisations in use: coverage (K17), contacts (K20), flexibility (K21)
COVERAGE = dict(purpose="superpose", unique=False, max_atoms=8)
CONTACTS = dict(purpose="count contacts of")
FLEXIBILITY = dict(purpose="superpose", at_least=3)


def _refused(message, sel, n_atoms, **how):
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        ensemble.selection(sel, n_atoms, **how)


@pytest.mark.parametrize("how", (COVERAGE, CONTACTS, FLEXIBILITY))
def test_selection_accepts_and_refuses_what_every_caller_does(how):
    assert ensemble.selection(None, 6, **how).tolist() == list(range(6))
    got = ensemble.selection([5, 0, 3], 6, **how)
    assert got.tolist() == [5, 0, 3] and got.dtype == np.int32 and got.flags["C_CONTIGUOUS"]
    _refused(f"the selection is empty (m = 0): no atoms to {how['purpose']}", [], 6, **how)
    _refused("the selection names atom -1, a structure has 6 atoms", [0, 2, -1], 6, **how)
    _refused("the selection names atom 6, a structure has 6 atoms", [0, 6, 2], 6, **how)


def test_selection_keeps_order_and_width():
    for how in (COVERAGE, CONTACTS):
        got = ensemble.selection([5, 0], 6, **how)
        assert got.tolist() == [5, 0] and got.dtype == np.int32


def test_selection_of_coverage_takes_a_repeat_and_has_its_two_limits():
    assert ensemble.selection([1, 1, 2], 6, **COVERAGE).tolist() == [1, 1, 2]
    assert ensemble.selection([0] * 6, 6, **COVERAGE).tolist() == [0] * 6
    _refused("the selection lists 7 atoms, a structure has 6", [0] * 7, 6, **COVERAGE)
    _refused("the selection lists 7 atoms, a structure has 6", [0] * 6 + [9], 6, **COVERAGE)     # before the index is looked at
    assert ensemble.selection(None, 8, **COVERAGE).shape == (8,)
    _refused("9 atoms per structure (the kernel holds 8)", None, 9, **COVERAGE)
    _refused("9 atoms per structure (the kernel holds 8)", [], 9, **COVERAGE)                    # before the selection is looked at


def test_selection_of_contacts_and_flexibility_refuses_a_repeat():
    for how in (CONTACTS, FLEXIBILITY):
        _refused("the selection names an atom twice", [1, 2, 1], 6, **how)
        _refused("the selection names atom 9, a structure has 6 atoms", [1, 9, 1], 6, **how)      # before the repeat
        # more entries than atoms: a repeat or a stray index, reported as that
        _refused("the selection names an atom twice", [0, 1, 2, 3, 4, 5, 0], 6, **how)
    assert ensemble.selection(None, 9, **CONTACTS).shape == (9,)                                 # no atom limit of its own


def test_selection_of_flexibility_needs_three_atoms():
    assert ensemble.selection([4, 1], 6, **CONTACTS).tolist() == [4, 1]
    assert ensemble.selection([4, 1, 0], 6, **FLEXIBILITY).tolist() == [4, 1, 0]
    _refused("the selection lists 2 atoms: a rotation needs at least 3", [4, 1], 6, **FLEXIBILITY)
    _refused("the selection lists 1 atoms: a rotation needs at least 3", [7], 6, **FLEXIBILITY)    # before the index is looked at
    _refused("the selection lists 2 atoms: a rotation needs at least 3", None, 2, **FLEXIBILITY)


def test_check_sets_refuses_in_the_order_of_the_compare_prologue():
    ref, gen, z = np.zeros((4, 5, 3), np.float32), np.zeros((6, 5, 3), np.float32), np.full(5, 6)
    r, g, zz = ensemble.check_sets(ref, gen, z, groups="bead")
    assert tuple(r.shape) == (4, 5, 3) and tuple(g.shape) == (6, 5, 3) and zz.dtype == np.int64 and zz.tolist() == [6] * 5
    two = "^" + re.escape("at least two reference frames are needed (the floor compares the even with the odd ones)") + "$"
    with pytest.raises(ValueError, match=two):
        ensemble.check_sets(ref[:1], gen, z)
    with pytest.raises(ValueError, match="^z lists 4 atoms, the frames have 5 and 5$"):
        ensemble.check_sets(ref, gen, z[:4])
    with pytest.raises(ValueError, match="^z lists 5 atoms, the frames have 5 and 7$"):
        ensemble.check_sets(ref, np.zeros((6, 7, 3), np.float32), z)
    with pytest.raises(ValueError, match="^groups must be None, 'bead' or 'residue'$"):
        ensemble.check_sets(ref, gen, z, groups="chain")
    # wrong in two ways: the earlier check speaks
    with pytest.raises(ValueError, match=re.escape("structures must be [S, n, 3], got (5, 3)")):
        ensemble.check_sets(ref[0], gen, z[:4])
    with pytest.raises(ValueError, match=two):
        ensemble.check_sets(ref[:1], gen, z[:4], groups="chain")
    with pytest.raises(ValueError, match="^z lists 4 atoms"):
        ensemble.check_sets(ref, gen, z[:4], groups="chain")
    # coverage's form: the generated set's width is not compared with z, and the message names the reference alone
    ensemble.check_sets(ref, np.zeros((6, 7, 3), np.float32), z, gen_width=False)
    with pytest.raises(ValueError, match="^z lists 4 atoms, a reference frame has 5$"):
        ensemble.check_sets(ref, gen, z[:4], gen_width=False)


def test_hist_moments_and_scalar_block_on_fixed_arrays():
    v = np.array([-0.5, 0.0, 0.24, 0.25, 0.99, 1.0, 1.0, 1.5, 2.0])
    assert ensemble.hist(v, 0.0, 1.0, 4) == {"counts": [2, 1, 0, 3], "under": 1, "over": 2}      # 1.0: the last bin, not over
    assert ensemble.hist(v, 1.0, 1.0, 3) == {"counts": [0, 0, 0], "under": 5, "over": 2}         # hi == lo: nothing is binned
    assert ensemble.hist(np.zeros(0), 0.0, 1.0, 2) == {"counts": [0, 0], "under": 0, "over": 0}
    assert ensemble.moments(np.zeros(0)) == (None, None)
    assert ensemble.moments(np.array([1.0, 3.0])) == (2.0, 1.0)
    even, odd, gen = np.array([0.1, 0.6]), np.array([0.1, 0.9]), np.array([0.1, 0.1, 0.6, 1.2])
    block = ensemble.scalar_block(even, odd, gen, 0.0, 1.0, 2)
    assert block["range"] == [0.0, 1.0]
    assert block["hist_ref"] == {"counts": [2, 2], "under": 0, "over": 0} and block["hist_gen"] == {"counts": [2, 1], "under": 0, "over": 1}
    assert block["floor"] == 0.0 and block["jsd"] == ensemble.js_divergence([2, 2], [2, 1]) and 0.0 < block["jsd"] < 1.0
    assert (block["mean_ref"], block["mean_gen"]) == (pytest.approx(0.425), pytest.approx(0.5))
    assert block["std_ref"] == pytest.approx(np.std([0.1, 0.6, 0.1, 0.9])) and block["std_gen"] == pytest.approx(np.std(gen))
    empty = ensemble.scalar_block(np.zeros(0), np.zeros(0), gen, 0.0, 1.0, 2)
    assert empty["mean_ref"] is None and empty["std_ref"] is None and empty["jsd"] is None and empty["floor"] is None


@pytest.mark.parametrize("S, M", ((0, 4), (3, 4), (4, 4), (9, 4)))                    # nothing, S < M, S = M, S = 2M + 1
def test_chunks_cover_the_set_in_order_as_contiguous_fp32(S, M):
    x = torch.arange(S * 5 * 3, dtype=torch.float64).reshape(5, S, 3).transpose(0, 1)         # float64 and not contiguous
    got = list(ensemble.chunks(x, M, "cpu"))
    assert [start for start, _ in got] == list(range(0, S, M)) and len(got) == -(-S // M)
    for start, chunk in got:
        assert chunk.dtype == torch.float32 and chunk.is_contiguous() and chunk.device.type == "cpu"
        assert tuple(chunk.shape) == (min(M, S - start), 5, 3) and not chunk.requires_grad
    if S:
        assert torch.equal(torch.cat([chunk for _, chunk in got]), x.to(torch.float32))
    grad = torch.zeros(3, 5, 3, requires_grad=True)
    assert not any(chunk.requires_grad for _, chunk in ensemble.chunks(grad, 2, "cpu"))


def test_structures_per_launch_is_the_rule_the_three_callers_wrote_out():
    assert ensemble.WORKSPACE_BYTES == 1 << 28
    m, nH, nA = 5000, 1500, 2000
    for per in (16 * m, 16 * m + 4, 16 * (2 * nH + nA)):                      # contacts, sasa, hbonds
        budget = (1 << 28) // per
        assert 64 < budget < 4096                                             # so that all three bounds are exercised
        for requested, limit in ((budget - 1, 1 << 20), (4096, 1 << 20), (4096, 100), (budget + 5, budget + 1), (0, 4096), (-3, 4096)):
            want = max(1, min(int(requested), limit, max(64, (1 << 28) // per)))
            assert ensemble.structures_per_launch(requested, limit, per) == want, (requested, limit, per)
    assert ensemble.structures_per_launch(3001, 1 << 20, 16 * m) == 3001      # below the budget: the request
    assert ensemble.structures_per_launch(1 << 30, 1 << 20, 16 * m) == (1 << 28) // (16 * m)   # above it: the budget
    assert ensemble.structures_per_launch(4096, 100, 16 * m) == 100           # above the limit
    assert ensemble.structures_per_launch(0, 4096, 16 * m) == 1
    assert ensemble.structures_per_launch(4096, 4096, 1 << 27) == 64          # the budget never asks for fewer than 64


def test_set_sizes_counts_structures_and_bad_ones():
    even, odd = {"bad": np.array([False, True, False])}, {"bad": np.array([0, 0], dtype=np.int32)}
    gen = {"bad": [True, True, False, False, True]}
    got = ensemble.set_sizes(even, odd, gen)
    assert got == {"n_ref": 5, "n_gen": 5, "n_bad_ref": 1, "n_bad_gen": 3} and list(got) == ["n_ref", "n_gen", "n_bad_ref", "n_bad_gen"]
    assert all(type(v) is int for v in got.values())
    empty = {"bad": np.zeros(0, dtype=bool)}
    assert ensemble.set_sizes(empty, empty, empty) == {"n_ref": 0, "n_gen": 0, "n_bad_ref": 0, "n_bad_gen": 0}


def test_short_block_keeps_the_moments():
    assert ensemble.MOMENTS == ("jsd", "mean_ref", "std_ref", "mean_gen", "std_gen")
    assert ensemble.short_block(None) is None and ensemble.short_block(None, ("jsd",)) is None
    block = ensemble.scalar_block(np.array([0.1, 0.6]), np.array([0.1, 0.9]), np.array([0.1, 0.1, 0.6, 1.2]), 0.0, 1.0, 2)
    short = ensemble.short_block(block)
    assert list(short) == list(ensemble.MOMENTS) and all(short[k] == block[k] for k in short)
    flex = ensemble.short_block(block, ("jsd", "floor") + ensemble.MOMENTS[1:])
    assert list(flex) == ["jsd", "floor", "mean_ref", "std_ref", "mean_gen", "std_gen"] and flex["floor"] == block["floor"]


def test_every_record_has_its_switch_in_both_command_lines():
    assert [a.stem for a in ANALYSES] == ["dist", "tica", "cov", "contact", "flex", "kde"]
    assert [a.min_frames for a in ANALYSES] == [2, 2, 2, 2, 2, 4] and [a.top_level for a in ANALYSES] == [True] * 3 + [False] * 3
    extras = {s for act in run_ala.build_extras_parser()._actions for s in act.option_strings}
    backmap = {s for act in bm.build_parser()._actions for s in act.option_strings}
    for a in ANALYSES:
        assert f"--{a.stem}_eval" in extras and f"--{a.stem}_stats" in backmap
        assert callable(a.module.summary_of) and callable(getattr(run_ala, a.stem + "_eval"))
        assert all("-" + k in extras for k in a.options)
    assert {s for s in extras if s.endswith("_eval")} == {f"--{a.stem}_eval" for a in ANALYSES}
    assert {s for s in backmap if s.endswith("_stats")} == {f"--{a.stem}_stats" for a in ANALYSES}


def test_stored_params_drops_exactly_the_keys_of_switched_off_records():
    base = vars(run_ala.build_parser().parse_args("-logdir x".split()))
    params = {**base, **vars(run_ala.build_extras_parser().parse_args([]))}
    assert run_ala.stored_params(params) == base                       # everything off: the file of before the switches existed
    for a in ANALYSES:
        on = run_ala.stored_params({**params, a.stem + "_eval": True})
        want = {a.stem + "_eval": True, **{k: params[k] for k in a.options}}
        assert on == {**base, **want}, a.stem
        assert ("tica_lag" in on) == (a.stem == "tica")
        off = run_ala.stored_params({**params, a.stem + "_eval": False})
        assert off == base, a.stem
    everything = run_ala.stored_params({**params, **{a.stem + "_eval": True for a in ANALYSES}})
    assert set(everything) - set(base) == {a.stem + "_eval" for a in ANALYSES} | {"tica_lag"}
