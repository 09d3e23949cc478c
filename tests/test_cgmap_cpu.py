"""Host side of the coarse-graining map learner (``-cg_method cgae``, coarsegrainingvae_amd/cgmap.py): the fp64 restatement
against the reference's stored outputs, the mapping choice of the CLI, the retry rule, the frame-order table and the
noise generator's restatement.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgae_restatement as R  # noqa: E402

from coarsegrainingvae_amd import cgmap  # noqa: E402


@pytest.mark.parametrize("name", R.STEP_FIXTURES)
def test_restatement_reproduces_the_reference_step(golden, name):
    """The fixtures are the reference's fp32 outputs, so the restatement (fp64) can only agree with them to the rounding
    the reference accumulated.  Bound, from the fixture's dtype: every stored quantity is a chain of fp32 sums whose
    longest one runs over L = max(n_atoms, 3 B) terms (bead coordinates and their gradients sum over atoms, parameter
    gradients over the batch's 3 B coordinates); recursive summation of L terms is off by at most L eps relative to the
    sum of magnitudes (Higham, Accuracy and Stability, 4.2), taken here relative to the quantity's largest entry."""
    f = golden(name)
    assert f["M"].dtype == np.float32
    B, n, _ = f["X"].shape
    tol = max(n, 3 * B) * float(np.finfo(f["M"].dtype).eps)
    r = R.restate_fixture(f)
    for q in R.QUANTITIES + ("recon",):
        dev = R.rel_dev(f[q], r[q])
        print(f"{name} {q}: {dev:.3e} (bound {tol:.3e})")
        assert dev <= tol, (q, dev, tol)


def _frames(T=12, n=9):
    return np.random.default_rng(0).standard_normal((T, n, 3)).astype(np.float32)


def test_cgae_without_a_file_mapping_calls_the_learner(monkeypatch):
    calls = []

    def stub(xyz, n_cgs, reg_weight=None, device=None, **kw):
        calls.append((np.asarray(xyz).shape, n_cgs, reg_weight, device))
        return torch.tensor([2, 2, 2, 0, 0, 0, 1, 1, 1]), {"method": "cgae", "steps": 7}
    monkeypatch.setattr(cgmap, "learn_map", stub)
    mapping, info = cgmap.select_mapping("cgae", None, _frames(), 3, 0.4, "cuda:0")
    assert calls == [((12, 9, 3), 3, 0.4, "cuda:0")]
    assert mapping.tolist() == [2, 2, 2, 0, 0, 0, 1, 1, 1] and info["method"] == "cgae"


def test_cgae_with_a_file_mapping_uses_the_file(monkeypatch):
    monkeypatch.setattr(cgmap, "learn_map", lambda *a, **k: pytest.fail("the learner must not run"))
    file_mapping = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2])
    mapping, info = cgmap.select_mapping("cgae", file_mapping, _frames(), 3, 0.25, "cuda:0")
    assert mapping.tolist() == file_mapping.tolist() and info is None


def test_other_methods_keep_the_contiguous_blocks(monkeypatch):
    monkeypatch.setattr(cgmap, "learn_map", lambda *a, **k: pytest.fail("the learner must not run"))
    mapping, info = cgmap.select_mapping("minimal", None, _frames(T=4, n=22), 3, 0.25, "cuda:0")
    assert mapping.tolist() == ((np.arange(22) * 3) // 22).tolist() and info is None
    with pytest.raises(SystemExit):
        cgmap.select_mapping("minimal", None, _frames(), None, 0.25, "cuda:0")


def test_the_cli_module_routes_through_the_choice():
    from coarsegrainingvae_amd import run_ala
    assert run_ala.cgmap is cgmap
    params = vars(run_ala.build_parser().parse_args("-cg_method cgae -n_cgs 3".split()))
    assert params["cg_method"] == "cgae" and params["cgae_reg_weight"] == 0.25          # no new or changed flag


def _stub_learner(results, seeds):
    def learn_once(xyz, n_cgs, seed=None, **kw):
        seeds.append(seed)
        return torch.tensor(results[len(seeds) - 1]), {"method": "cgae", "steps": 5, "seconds": 1.0, "loss_recon": 0.1,
                                                       "loss_reg": 0.2, "attempts": 1, "form": "resident", "seed": seed}, None
    return learn_once


def test_retry_until_every_bead_is_used(monkeypatch):
    seeds = []
    results = [[0, 0, 0, 1, 1, 1], [2, 2, 2, 2, 2, 2], [0, 1, 2, 2, 1, 0], [0, 0, 0, 0, 0, 0]]
    monkeypatch.setattr(cgmap, "learn_once", _stub_learner(results, seeds))
    mapping, info = cgmap.learn_map(_frames(n=6), 3, seed=40)
    assert mapping.tolist() == results[2] and mapping.dtype == torch.long
    assert seeds == [40, 41, 42] and info["attempts"] == 3 and info["seed"] == 42 and info["seconds"] == 3.0


def test_retry_gives_up_after_the_cap(monkeypatch):
    seeds = []
    monkeypatch.setattr(cgmap, "learn_once", _stub_learner([[0, 0, 1, 1, 0, 0]] * 10, seeds))
    with pytest.raises(RuntimeError) as err:
        cgmap.learn_map(_frames(n=6), 3, seed=7)
    assert seeds == [7, 8, 9, 10, 11] and cgmap.MAX_ATTEMPTS == 5
    assert "6 atoms" in str(err.value) and "n_cgs = 3" in str(err.value)


@pytest.mark.parametrize("n_train,batch,epochs", [(180, 32, 7), (36, 32, 5), (64, 32, 3), (5, 8, 4)])
def test_frame_order_table(n_train, batch, epochs):
    order = cgmap.frame_order(n_train, batch, epochs, seed=3)
    assert order.dtype == np.int32 and order.shape == (epochs, n_train)
    for row in order:                                              # every epoch: a permutation of the training subset
        assert sorted(row.tolist()) == list(range(n_train))
    if n_train > 2:
        assert any(not np.array_equal(order[0], row) for row in order[1:])
    assert np.array_equal(order, cgmap.frame_order(n_train, batch, epochs, seed=3))
    spe = cgmap.steps_per_epoch(n_train, batch)
    assert spe == math.ceil(n_train / batch)
    sizes = [len(order[0, s * batch:(s + 1) * batch]) for s in range(spe)]
    assert sum(sizes) == n_train and all(s == batch for s in sizes[:-1])
    assert sizes[-1] == (n_train % batch or batch)                  # the partial last batch is there
    assert epochs * spe == order.shape[0] * cgmap.steps_per_epoch(order.shape[1], batch)    # what Learner derives from the table


def test_train_subset_and_initial_parameters():
    sub = cgmap.train_subset(1000, 5)
    assert len(sub) == 900 and len(set(sub.tolist())) == 900 and torch.equal(sub, cgmap.train_subset(1000, 5))
    assert len(cgmap.train_subset(200, 0)) == 180 and len(cgmap.train_subset(40, 0)) == 36
    assert not torch.equal(sub, cgmap.train_subset(1000, 6))
    torch.manual_seed(11)                                          # the reference's construction order (cgae.py:13-14)
    w, d = torch.randn(22, 3), torch.randn(3, 22)
    W, D = cgmap.initial_parameters(22, 3, 11)
    assert torch.equal(W, w) and torch.equal(D, d)


def test_noise_restatement_is_gumbel():
    """>= 10^6 draws: mean within 5 standard errors of the Euler-Mascheroni constant, variance within 5 standard errors
    of pi^2 / 6.  Standard errors of N independent draws: sqrt(var / N) for the mean; sqrt((mu4 - var^2) / N) for the
    variance, with the Gumbel's fourth central moment mu4 = (3 + 12/5) var^2 (excess kurtosis 12/5)."""
    n, K, steps = 1000, 6, 170
    g = np.stack([R.gumbel_noise(seed=99, step=s, n=n, K=K) for s in range(steps)]).astype(np.float64)
    N = g.size
    assert N >= 10 ** 6 and np.isfinite(g).all()
    var = math.pi ** 2 / 6
    se_mean, se_var = math.sqrt(var / N), math.sqrt((5.4 - 1.0) * var ** 2 / N)
    print(f"N {N}: mean {g.mean():.5f} (se {se_mean:.5f}), var {g.var():.5f} (se {se_var:.5f})")
    assert abs(g.mean() - 0.5772156649) < 5 * se_mean
    assert abs(g.var() - var) < 5 * se_var
    # stateless: a step's matrix depends on (seed, step) alone, and differs between steps, seeds and elements
    assert np.array_equal(R.gumbel_noise(99, 3, 50, 6), g[3, :50].astype(np.float32))
    assert not np.array_equal(R.gumbel_noise(98, 3, 50, 6), g[3, :50].astype(np.float32))
    assert len(np.unique(g[0])) > 0.99 * g[0].size
