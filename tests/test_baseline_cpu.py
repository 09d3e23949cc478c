"""The baseline models without a GPU: the fp64 restatement against the reference's stored outputs, the fold split, the
command-line surface, the refusals, parameter names and the form rule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_restatement as R  # noqa: E402

from coarsegrainingvae_amd import _lib, baseline, run_baseline  # noqa: E402

STEP_Q = ("xyz_recon", "loss_recon", "loss_dist", "grad", "B_after1", "B_after10")


@pytest.mark.parametrize("name", R.STEP_FIXTURES)
def test_restatement_reproduces_the_reference_steps(golden, name):
    """fp64 restatement against the reference's fp32 outputs: within fp32 rounding of the sums involved (1e-5 relative to
    the largest entry is two orders above every stored deviation and far below any formula error), and equal to the
    deviation the generator stored."""
    f = golden(name)
    want = R.restate_step_fixture(f)
    for q in STEP_Q + (("partial_xyz_recon", "partial_loss_recon", "partial_loss_dist", "partial_grad") if "xyz_partial" in f else ()):
        dev = R.rel_dev(f[q], want[q])
        assert dev <= 1e-5, (q, dev)
        assert dev == pytest.approx(float(f["dev_" + q]), rel=1e-3, abs=1e-12), q


@pytest.mark.parametrize("name", R.MLP_FIXTURES)
def test_restatement_reproduces_the_reference_mlp(golden, name):
    f = golden(name)
    depth, last = int(f["depth"]), 2 * int(f["depth"]) + 2
    names = ("mlp.0", "mlp.2", f"mlp.{last}")
    weights = [f[f"p.{nm}.{w}"] for nm in names for w in ("weight", "bias")]
    want = R.step_outputs("mlp", weights, f["xyz"], f["mapping"], f["edges"], float(f["gamma"]), int(f["K"]), depth=depth)
    for q in ("xyz_recon", "loss_recon", "loss_dist", "grad_recon"):
        assert R.rel_dev(f[q], want[q]) <= 1e-5, q
    for (nm, w), g in zip([(nm, w) for nm in names for w in ("weight", "bias")], want["grads"]):
        assert R.rel_dev(f[f"g.{nm}.{w}"], g) <= 1e-5, (nm, w)           # mlp.2: the sum over the shared layer's uses
    if depth == 2:
        assert np.array_equal(f["p.mlp.2.weight"], f["p.mlp.4.weight"]) and np.array_equal(f["p.mlp.2.bias"], f["p.mlp.4.bias"])


def test_coincident_pair_and_empty_edge_list_in_the_restatement():
    xyz = torch.randn(2, 5, 3, dtype=torch.float64)
    recon = xyz.clone().requires_grad_(True)
    with torch.no_grad():
        recon[:, 1] = recon[:, 0]
    l_recon, l_dist = R.losses(recon, xyz, np.array([[0, 1], [2, 3]]))
    (l_recon + l_dist).backward()
    assert torch.isfinite(recon.grad).all() and float(l_dist.detach()) > 0
    assert float(R.losses(recon, xyz, np.zeros((0, 2), dtype=np.int64))[1]) == 0.0


@pytest.mark.parametrize("T,k", [(60, 2), (61, 3), (100, 3), (7, 7), (2000, 3)])
def test_fold_split(T, k):
    """Test-block sizes as sklearn's KFold (n // k, the first n % k one longer, contiguous, in order); validation = ceil(10 %)
    of the fold's own training indices; no test frame in train or val; every frame is tested exactly once."""
    folds = run_baseline.fold_split(T, k, seed=5)
    assert [len(te) for _, _, te in folds] == [T // k + (1 if i < T % k else 0) for i in range(k)]
    assert np.array_equal(np.concatenate([te for _, _, te in folds]), np.arange(T))
    for tr, va, te in folds:
        assert len(va) == int(np.ceil(0.1 * (T - len(te))))
        assert not set(te) & (set(tr) | set(va)) and not set(tr) & set(va)
        assert sorted(set(tr) | set(va) | set(te)) == list(range(T))
    again = run_baseline.fold_split(T, k, seed=5)
    assert all(np.array_equal(a, b) for f, g in zip(folds, again) for a, b in zip(f, g))


def test_cli_flag_surface():
    """scripts/run_baseline.py:412-434: name, type and default of every flag; plus -traj, --synthetic, -seed."""
    want = {"logdir": (str, None), "model": (str, "equilinear"), "dataset": (str, "dipeptide"), "device": (int, None),
            "cutoff": (float, 2.5), "batch_size": (int, 32), "N_cg": (int, 3), "width": (int, 1), "depth": (int, 1),
            "edgeorder": (int, 2), "n_splits": (int, 3), "n_epochs": (int, 50), "ndata": (int, 2000), "knbr": (int, 0),
            "cg_method": (str, "newman"), "activation": (str, "ReLU"), "mapshuffle": (float, 0.0), "lr": (float, 1e-3),
            "gamma": (float, 0.0), "kappa": (float, 0.0), "traj": (str, None), "seed": (int, 123)}
    switches = {"tqdm_flag", "cross", "synthetic"}
    actions = {a.dest: a for a in run_baseline.build_parser()._actions if a.dest != "help"}
    assert set(actions) == set(want) | switches
    for name, (typ, default) in want.items():
        a = actions[name]
        assert a.option_strings == ["-" + name] and a.type is typ and a.default == default, name
    for name in switches:
        a = actions[name]
        assert a.option_strings == ["--" + name] and a.default is False and a.nargs == 0, name
    assert run_baseline.CV_STATS_COLUMNS == ["train_recon", "test_all_recon", "test_heavy_recon", "train_graph", "test_graph",
                                            "train_tetra", "test_tetra", "all atom ged", "heavy atom ged",
                                            "all atom graph valid ratio", "heavy atom graph valid ratio"]
    assert run_baseline.TRAIN_LOG_COLUMNS == ["epoch", "lr", "train_recon", "val_recon", "train_graph", "val_graph"]


def test_equimlp_is_refused():
    params = vars(run_baseline.build_parser().parse_args("-model equimlp --synthetic".split()))
    with pytest.raises(SystemExit, match="equimlp"):
        run_baseline.run(params)


def test_empty_bead_is_refused():
    with pytest.raises(ValueError, match="empty"):
        baseline.FixedPool([0, 0, 2, 2], 3)
    pool = baseline.FixedPool([0, 0, 2, 1, 2], 3)
    assert pool.sizes.tolist() == [2, 1, 2]
    assert torch.allclose(pool.M_norm.sum(0), torch.ones(3)) and pool.M_norm[3, 1] == 1.0 and pool.M_norm[0, 0] == 0.5
    with pytest.raises(ValueError, match="knn"):
        baseline.EquiLinear(pool, 3, 5, False, 3)


def test_state_dict_names_and_reference_state():
    pool = baseline.FixedPool(np.arange(22) * 3 // 22, 3)
    assert list(baseline.Baseline(pool, 3, 22).state_dict()) == ["B"]
    assert tuple(baseline.Baseline(pool, 3, 22).B.shape) == (3, 22)
    eq = baseline.EquiLinear(pool, 3, 22, cross=False, knn=2)
    assert list(eq.state_dict()) == ["B"] and tuple(eq.B.shape) == (22, 6)
    mlp = baseline.MLP(pool, 3, 22, width=1, depth=2, activation="ReLU")
    keys = list(mlp.state_dict())
    assert keys == ["mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias",
                    "mlp.6.weight", "mlp.6.bias"]
    assert mlp.mlp[2] is mlp.mlp[4] and len(list(mlp.parameters())) == 6
    assert tuple(mlp.mlp[0].weight.shape) == (66, 9) and tuple(mlp.mlp[6].weight.shape) == (66, 66)
    # a reference state_dict: pooler.* keys dropped, the rest strict
    ref = {k: torch.randn_like(v) for k, v in mlp.state_dict().items()}
    ref["mlp.4.weight"], ref["mlp.4.bias"] = ref["mlp.2.weight"], ref["mlp.2.bias"]
    ref["pooler.atom_embed.weight"] = torch.zeros(100, 16)
    mlp.load_reference_state(ref)
    assert torch.equal(mlp.mlp[2].weight, ref["mlp.2.weight"]) and torch.equal(mlp.mlp[6].bias, ref["mlp.6.bias"])
    with pytest.raises(RuntimeError):
        mlp.load_reference_state({k: v for k, v in ref.items() if k != "mlp.0.bias"})
    eq.load_reference_state({"B": torch.ones(22, 6), "pooler.cg_network.0.weight": torch.zeros(16, 16)})
    assert torch.equal(eq.B.data, torch.ones(22, 6))
    with pytest.raises(RuntimeError):
        eq.load_reference_state({"B": torch.ones(22, 6), "extra": torch.zeros(1)})


def test_mlp_fixture_keys_are_the_modules_keys(golden):
    f = golden("g19_baseline_mlp_w1_d2_g05")
    pool = baseline.FixedPool(f["mapping"], int(f["K"]))
    mlp = baseline.MLP(pool, int(f["K"]), 22, width=1, depth=2)
    assert sorted(mlp.state_dict()) == [str(k) for k in f["state_keys"]]
    mlp.load_reference_state({str(k): torch.from_numpy(f["p." + str(k)]) for k in f["state_keys"]})


def test_form_rule_is_monotone():
    """cgv_baseline_resident_fits: once a size does not fit, no larger one does (in atoms, features and batch alike); the
    dipeptide and chignolin sizes of the issue fit."""
    fits = _lib.load().cgv_baseline_resident_fits
    assert fits(baseline.EQUILINEAR, 22, 6, 32) == 1 and fits(baseline.EQUILINEAR, 166, 30, 32) == 1
    assert fits(baseline.LINEAR, 22, 3, 32) == 1 and fits(baseline.EQUILINEAR, 300, 24, 16) == 1
    assert fits(baseline.EQUILINEAR, 300, 56, 16) == 0 and fits(0, 22, 3, 4) == 0 and fits(baseline.LINEAR, 0, 3, 4) == 0
    for kind in (baseline.LINEAR, baseline.EQUILINEAR):
        for axis in range(3):
            base = [64, 8, 8]
            seen_zero = False
            for v in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 4096, 16384, 65536):
                args = list(base)
                args[axis] = v
                ok = fits(kind, *args)
                assert not (seen_zero and ok), (kind, axis, v)
                seen_zero = seen_zero or not ok
            assert seen_zero, (kind, axis)
