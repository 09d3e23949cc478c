"""Essential dynamics on the device: K27 (csrc/pca.hip) against the numpy restatement (pca_restatement.py).  Every bound is
computed from the restatement's own numbers -- the magnitudes summed -- never from what the kernel returns; the measured
worst error / bound of every family is printed before it is asserted."""
import functools
import json

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import _lib, pca
import flexibility_restatement as FR
import pca_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -52
C_ROT = 32.0                                                  # tests/test_flexibility_gpu.py: the rotation's constant


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)      # a copy: the cached cases are read-only


def _moments(y, sel, centre, bad=None, chunk=None):
    """``pca.moments_launch`` over ``y`` in launches of ``chunk`` structures (default: one); host arrays."""
    S, d = y.shape[0], 3 * len(sel)
    bad = np.zeros(S, np.int32) if bad is None else bad
    yd, sd, cd, bd = _dev(y, np.float32), _dev(sel, np.int32), _dev(centre, np.float64), _dev(bad, np.int32)
    totals = pca.new_totals(d, DEV)
    step = chunk or max(S, 1)
    for s0 in range(0, max(S, 1), step):
        pca.moments_launch(yd[s0:s0 + step], sd, cd, bd[s0:s0 + step], totals)
    torch.cuda.synchronize()
    return {"sum": totals["sum"].cpu().numpy(), "cov": totals["cov"].cpu().numpy(), "n_good": int(totals["n_good"].cpu()[0])}


def _ratio(err, bound):
    """Worst error / bound; an element whose bound is 0 must be exact."""
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def _within(got, want, what, scale=1.0, extra=None):
    b = R.moment_bounds(want)
    bc, bs = scale * b["cov"] + (0 if extra is None else extra["cov"]), scale * b["sum"] + (0 if extra is None else extra["sum"])
    rc, rs = _ratio(np.abs(got["cov"] - want["cov"]), bc), _ratio(np.abs(got["sum"] - want["sum"]), bs)
    print(what, "worst error / bound: cov", rc, "sum", rs)
    assert got["n_good"] == want["n_good"], what
    assert np.array_equal(got["cov"], got["cov"].T), what            # exactly symmetric
    assert rc <= 1.0 and rs <= 1.0, (what, rc, rs)
    return rc, rs


@functools.lru_cache(maxsize=None)
def _case(m, S, seed=0):
    """Random fp32 "aligned" structures of n = m + 4 atoms in a 20 A box, a scattered and unordered selection of m of them,
    a centre within 1 A of the box's middle; and the restatement's moments."""
    rng = np.random.default_rng(1000 * m + S + 7919 * seed)
    n = m + 4
    y = rng.uniform(-10, 10, (S, n, 3)).astype(np.float32)
    sel = rng.permutation(n)[:m]
    centre = rng.uniform(-1, 1, (n, 3))
    want = R.moments(y, sel, centre)
    for v in (y, sel, centre, *want.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return y, sel, centre, want


def _one_range(d):
    """The structures of one range at ``d`` features, read from the library's rule: the largest count that is one range."""
    lib = _lib.load()
    per = next(S for S in range(1, 1 << 16) if lib.cgv_pca_moments_splits(S + 1, d) == 2)
    assert lib.cgv_pca_moments_splits(per, d) == 1 and lib.cgv_pca_moments_splits(2 * per, d) == 2 and per % 16 == 0
    return per


# ----------------------------------------------------------------------------- 1. the feature's bits
@pytest.mark.parametrize("m", [3, 11])
def test_one_hot_modes_return_the_features_bit_for_bit(m):
    """Exact on an MI355X: 0 of 9 x 37 and 33 x 37 values differ."""
    y, sel, centre, _ = _case(m, 37)
    d = 3 * m
    f = R.features(y, sel, centre)
    yd, sd, cd, bd = _dev(y, np.float32), _dev(sel, np.int32), _dev(centre, np.float64), _dev(np.zeros(37), np.int32)
    got = np.empty((37, d))
    for c0 in range(0, d, 8):                                     # 8 columns of the identity per launch
        W = np.eye(d)[:, c0:c0 + 8]
        proj = torch.empty(37, W.shape[1], dtype=torch.float64, device=DEV)
        pca.project_launch(yd, sd, cd, bd, _dev(np.zeros(d), np.float64), _dev(W, np.float64), proj)
        got[:, c0:c0 + 8] = proj.cpu().numpy()
    differ = int(((got + 0.0).view(np.int64) != (f + 0.0).view(np.int64)).sum())
    print("m", m, "feature values that differ:", differ, "of", f.size)
    assert differ == 0


# ----------------------------------------------------------------------------- 2. moments against the restatement
@pytest.mark.parametrize("m", [1, 10, 11, 21, 22, 43])            # d = 3, 30, 33, 63, 66, 129: one, two, three and five tiles
def test_moments_equal_the_restatement_within_the_summation_bound(m):
    """|d cov_ij| <= (N + 2) 2^-52 sum_s |f_si f_sj|, |d sum_i| <= N 2^-52 sum_s |f_si|.  Worst error / bound measured on an
    MI355X over the 54 cases: cov 0.25 (m 43, S 2: the one rounding of a product the matrix core does not make), 0.097 from
    S = 15 on and 0.016 at two ranges; sum 0.024 (m 43, two ranges; exact within one range, where both sides add in the same
    order)."""
    per = _one_range(3 * m)
    worst = (0.0, 0.0)
    for S in (1, 2, 15, 16, 17, per - 1, per, per + 1, 2 * per):
        y, sel, centre, want = _case(m, S)
        got = _moments(y, sel, centre)
        worst = tuple(max(a, b) for a, b in zip(worst, _within(got, want, f"m {m} S {S}")))
    print("m", m, "worst error / bound over S: cov", worst[0], "sum", worst[1])


# ----------------------------------------------------------------------------- 3. bad structures
def test_bad_structures_add_nothing():
    """Flagged rows (their y is NaN, as K21 writes it) in the middle of a stage, as a range's last row and as the last row.
    Worst error / bound measured on an MI355X: cov 0.011, sum 0.006."""
    m = 11
    per = _one_range(3 * m)
    S = per + 44
    y, sel, centre, _ = _case(m, S, seed=1)
    y = y.copy()
    bad = np.zeros(S, np.int32)
    bad[[5, 21, per - 1, per + 7, S - 1]] = 1
    y[bad == 1] = np.nan
    want = R.moments(np.where(np.isnan(y), 0, y), sel, centre, bad)
    assert want["n_good"] == S - 5
    got = _moments(y, sel, centre, bad)
    _within(got, want, "bad rows")
    assert np.isfinite(got["cov"]).all() and np.isfinite(got["sum"]).all()
    none = _moments(y, sel, centre, np.ones(S, np.int32))
    assert none["n_good"] == 0 and not none["cov"].any() and not none["sum"].any()
    assert not np.signbit(none["cov"]).any() and not np.signbit(none["sum"]).any()


# ----------------------------------------------------------------------------- 4. repeatability and chunks
def test_identical_calls_give_identical_bits_and_chunks_agree():
    """Measured on an MI355X, worst error / (twice the bound): cov 0.0056, sum 0.016 over chunks of 3, 16 and 4096."""
    m = 22
    y, sel, centre, want = _case(m, 700)
    a, b = _moments(y, sel, centre), _moments(y, sel, centre)
    assert a["cov"].tobytes() == b["cov"].tobytes() and a["sum"].tobytes() == b["sum"].tobytes() and a["n_good"] == b["n_good"] == 700
    for chunk in (3, 16, 4096):                                   # chunking changes the order: twice the bound
        _within(_moments(y, sel, centre, chunk=chunk), want, f"chunks of {chunk}", scale=2.0)
    nothing = _moments(y[:0], sel, centre)                       # S = 0 is a no-op
    assert nothing["n_good"] == 0 and not nothing["cov"].any() and not nothing["sum"].any()


# ----------------------------------------------------------------------------- 5. projection and histogram
@pytest.mark.parametrize("S", [1, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 2, 8])
def test_projection_and_histogram(k, S):
    """|d proj| <= (d + 2) 2^-52 sum_i |v_i W_ik| with v = f - mean (the restatement's bits).  The 16 x 16 map equals the
    restatement's over the structures farther from every bin edge than that bound; the rest may fall either side.
    Worst error / bound measured on an MI355X over the 12 cases: 0.011 (k 8, S 1000); no structure is near an edge."""
    m, nb = 43, 16                                                # d = 129: a lane sums up to three features
    d = 3 * m
    y, sel, centre, _ = _case(m, S, seed=2)
    rng = np.random.default_rng(10 * S + k)
    y = y.copy()
    bad = np.zeros(S, np.int32)
    if S > 2:
        bad[[1, S - 1]] = 1
        y[bad == 1] = np.nan
    W, mean = rng.standard_normal((d, k)) / np.sqrt(d), rng.uniform(-1, 1, d)
    want, mag = R.project(np.where(np.isnan(y), 0, y), sel, centre, mean, W, bad)
    bound = (d + 2) * U * mag
    ca, cb = 0, k - 1
    ra, rb = (-1.5 * 5.8, 1.5 * 5.8), (-1.2 * 5.8, 1.3 * 5.8)     # about 1.5 sigma of a projection: points fall off the map
    near = (R.edge_distance(np.nan_to_num(want[:, ca]), ra[0], ra[1], nb) <= bound[:, ca]) | \
           (R.edge_distance(np.nan_to_num(want[:, cb]), rb[0], rb[1], nb) <= bound[:, cb])
    near &= bad == 0
    assert near.sum() <= 0.01 * S, near.sum()                     # from the restatement, before the launch
    sure = ~near
    exp_counts, exp_out = R.hist2(want[sure, ca], want[sure, cb], ra, rb, nb)
    assert S < 100 or (exp_out > (bad != 0).sum() and exp_counts.sum() > 0.5 * S)   # the map is neither empty nor everything
    yd, sd, cd, bd = _dev(y, np.float32), _dev(sel, np.int32), _dev(centre, np.float64), _dev(bad, np.int32)
    proj = torch.full((S, k), 7.0, dtype=torch.float64, device=DEV)
    counts, outside = torch.zeros(nb, nb, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    pca.project_launch(yd, sd, cd, bd, _dev(mean, np.float64), _dev(W, np.float64), proj, (ca, cb, nb, ra, rb, counts, outside))
    got, counts, outside = proj.cpu().numpy(), counts.cpu().numpy().astype(np.int64), int(outside.cpu()[0])
    good = bad == 0
    assert np.isnan(got[~good]).all() and np.isfinite(got[good]).all()
    ratio = _ratio(np.abs(got[good] - want[good]), bound[good])
    print("k", k, "S", S, "worst error / bound: proj", ratio, "structures near an edge:", int(near.sum()))
    assert ratio <= 1.0
    assert counts.sum() + outside == S                            # every structure is counted once
    assert (counts - exp_counts >= 0).all() and outside - exp_out >= 0
    assert (counts - exp_counts).sum() + (outside - exp_out) == near.sum()


# ----------------------------------------------------------------------------- 6. through K21, end to end
@pytest.mark.parametrize("n", [12, 300])                          # the wave and the block form of K21
def test_moments_through_the_superposition(n):
    """``pca.moments`` against the restatement fed the host superposition's structures rounded to fp32.  On top of the
    summation bound: the two sides' aligned coordinates differ by K21's d y (tests/test_flexibility_gpu.py ``_bounds``:
    (C_ROT + m) 2^-52 |K|_F / gap |y| for the rotation, (m + 2) 2^-52 max|x| for the centring, 4 2^-52 |y| for the product)
    plus, where that moves a coordinate across a rounding boundary of fp32, the two half-ulps: delta = d y + 2^-23 |y_c|.
    It enters a feature once, so |d cov_ij| gains sum_s (|f_si| delta_sj + |f_sj| delta_si + delta_si delta_sj) and |d sum_i|
    gains sum_s delta_si.  Measured on an MI355X: the largest |d cov| is 4.4e-16 (n 12) and 1.8e-15 (n 300), 6.4e-10 and
    9.5e-10 of the bound -- no coordinate rounded the other way."""
    S = 40
    rng = np.random.default_rng(n)
    base = rng.uniform(0, 10, (n, 3))
    x = FR.noisy_copies(rng, base, S, 0.3)
    sel = rng.permutation(n)[:n - 5]
    m = len(sel)
    host = FR.align_accumulate(x, sel, base)
    centre = base - base[sel].mean(0)
    y32 = host["aligned"].astype(np.float32)
    want = R.moments(y32, sel, centre)
    ynorm = np.linalg.norm(host["aligned"], axis=2)                                          # [S, n]
    dy = ((C_ROT + m) * U * host["knorm"] / host["gap"] + 4 * U)[:, None] * ynorm + ((m + 2) * U * np.abs(x.astype(np.float64)).max((1, 2)))[:, None]
    delta = (dy[:, :, None] + 2.0 ** -23 * np.abs(host["aligned"]))[:, sel, :].reshape(S, 3 * m)
    f = np.abs(R.features(y32, sel, centre))
    extra = {"cov": f.T @ delta + delta.T @ f + delta.T @ delta, "sum": delta.sum(0)}
    got = pca.moments(x, base, sel, device=DEV)
    assert np.array_equal(got["centre"], centre) and not got["bad"].any() and got["n_good"] == S
    _within(got, want, f"through K21, n {n}", extra=extra)
    # without the fp32 term the sides still agree far inside it unless a coordinate rounded the other way
    print("n", n, "largest |d cov|", np.abs(got["cov"] - want["cov"]).max(), "against a bound of", (R.moment_bounds(want)["cov"] + extra["cov"]).max())
    assert np.abs(got["mean_aligned"] - host["sum"] / S).max() <= 1e-9
    assert np.abs(got["rmsd"] - np.sqrt(host["rmsd2"])).max() <= 1e-9


# ----------------------------------------------------------------------------- 7. planted motion
@functools.lru_cache(maxsize=None)
def _planted_sets():
    rng = np.random.default_rng(2024)
    n, S = 12, 400
    base = rng.uniform(0, 10, (n, 3))
    modes = R.unit_modes(rng, 2, n)
    other = R.unit_modes(rng, 2, n, against=modes)
    return {"ref": R.planted(rng, base, modes, (1.0, 0.5), S), "same": R.planted(rng, base, modes, (1.0, 0.5), S),
            "half": R.planted(rng, base, modes, (0.5, 0.25), S), "other": R.planted(rng, base, other, (1.0, 0.5), S)}


def _host_spectrum(x, target, sel):
    y = FR.align_accumulate(x, sel, target)["aligned"].astype(np.float32)
    mu, C = R.covariance(R.moments(y, sel, target - target[sel].mean(0)))
    lam, V = R.spectrum(C)
    return lam, V, C


def test_it_finds_planted_motion():
    """12 atoms in a 10 A box, 400 structures, two random unit collective modes with Gaussian amplitudes 1.0 and 0.5 A, 0.05 A
    of noise, a random proper rotation and translation each.  Measured on an MI355X (the host restatement gives the same
    figures to 1e-15): RMSIP(2) 0.9993 for an independent draw (floor 0.9991), 0.9987 for the half-amplitude ensemble, whose
    total variance is 0.287 of the reference's and 0.241 / 0.235 along its two modes; 0.069 for two other modes; (PC1, PC2)
    JSD 0.032 against a floor of 0.049 on 8 x 8 bins."""
    sets = _planted_sets()
    n = 12
    sel = np.arange(n)
    z, bonds = np.full(n, 6), np.zeros((0, 2), np.int64)
    # the restatement's verdicts first: the inputs, not the kernel, carry the margins
    target = FR.mean_structure(sets["ref"], sel)["mean"]
    lam, V, C = _host_spectrum(sets["ref"], target, sel)
    assert 0.6 < lam[0] < 1.0 and 0.15 < lam[1] < 0.3 and lam[2] < 0.01
    host = {k: _host_spectrum(sets[k], target, sel) for k in ("same", "half", "other")}
    assert R.rmsip(V[:, :2], host["same"][1][:, :2]) >= 0.995
    assert host["half"][0].sum() / lam.sum() < 0.45
    assert all(V[:, i] @ host["half"][2] @ V[:, i] / lam[i] < 0.45 for i in range(2))
    assert R.rmsip(V[:, :2], host["other"][1][:, :2]) < 0.4
    # the device
    same = pca.compare(sets["ref"], sets["same"], z, bonds, atoms="all", dim=2, n_bins=8, device=DEV)
    assert tuple(same) == pca.PCA_STATS_KEYS and json.loads(json.dumps(same)) == same
    # host and device stop refining the target once it moves less than 1e-4 A, so their targets agree to that order, and
    # to first order so do the statistics (all of order one here)
    assert same["rmsip"] >= 0.99 and same["eigenvalues_ref"] == pytest.approx(lam[:2], rel=1e-3)
    assert same["rmsip"] == pytest.approx(R.rmsip(V[:, :2], host["same"][1][:, :2]), abs=1e-3)
    assert same["covariance_overlap"] == pytest.approx(R.covariance_overlap(lam, V, host["same"][0], host["same"][1]), abs=1e-3)
    assert same["dccm_rmse"] == pytest.approx(float(np.sqrt(np.mean((R.dccm(host["same"][2]) - R.dccm(C)) ** 2))), abs=1e-3)
    floor = same["floor"]
    assert all(floor[key] is not None for key in ("rmsip", "covariance_overlap", "total_variance_ratio", "dccm_rmse")) and floor["rmsip"] >= 0.99
    assert same["pc_map"]["floor"] is not None and same["pc_map"]["floor"] > 0 and same["pc_map"]["jsd"] <= 3 * same["pc_map"]["floor"]
    assert (same["n_ref"], same["n_gen"], same["n_bad_ref"], same["n_bad_gen"]) == (400, 400, 0, 0)
    half = pca.compare(sets["ref"], sets["half"], z, bonds, atoms="all", dim=2, n_bins=8, device=DEV)
    assert half["total_variance_ratio"] < 0.5 and all(v < 0.5 for v in half["variance_in_ref_modes"]) and half["rmsip"] >= 0.99
    other = pca.compare(sets["ref"], sets["other"], z, bonds, atoms="all", dim=2, n_bins=8, device=DEV)
    assert other["rmsip"] < 0.5
    print("planted motion: rmsip same", same["rmsip"], "floor", floor["rmsip"], "half", half["rmsip"], "other", other["rmsip"],
          "variance ratio half", half["total_variance_ratio"], "in modes", half["variance_in_ref_modes"],
          "pc_map jsd", same["pc_map"]["jsd"], "floor", same["pc_map"]["floor"])


def test_fit_and_project_agree_with_the_host():
    """``fit`` with its default target, then ``project``: the components of the reference itself have the eigenvalues as
    their variances and no correlation, and a structure with a NaN is bad in both."""
    x = _planted_sets()["ref"].copy()
    x[7, 3, 1] = np.nan
    model = pca.fit(x, dim=3, device=DEV)
    assert model.n_good == 399 and model.W.shape == (36, 3) and model.eigenvalues.shape == (36,)
    out = pca.project(model, x, ranges=((-4, 4), (-2, 2)), n_bins=10, structures_per_launch=128, device=DEV)
    assert out["bad"].tolist() == [s == 7 for s in range(400)] and np.isnan(out["proj"][7]).all()
    p = out["proj"][~out["bad"]]
    np.testing.assert_allclose(p.mean(0), 0.0, atol=1e-9)
    np.testing.assert_allclose(p.T @ p / 399, np.diag(model.eigenvalues[:3]), atol=1e-9)
    assert out["hist2"].sum() + out["outside"] == 400 and out["outside"] >= 1 and out["hist2"].shape == (10, 10)
    want, _ = R.hist2(p[:, 0], p[:, 1], (-4, 4), (-2, 2), 10)
    assert np.abs(out["hist2"] - want).sum() <= 2                # a point on an edge may fall either side
    assert pca.project(model, x, device=DEV)["hist2"] is None


# ----------------------------------------------------------------------------- 8. limits and refusals through the wrapper
def test_bad_arguments_raise_before_a_launch():
    lim = pca.limits()
    S, n, m = 4, 6, 3
    y, sel, centre, bad = (torch.zeros(S, n, 3, device=DEV), torch.arange(m, dtype=torch.int32, device=DEV),
                           torch.zeros(n, 3, dtype=torch.float64, device=DEV), torch.zeros(S, dtype=torch.int32, device=DEV))
    totals = pca.new_totals(3 * m, DEV)

    def refused(match, y=y, sel=sel, centre=centre, bad=bad, totals=totals):
        with pytest.raises(ValueError, match=match):
            pca.moments_launch(y, sel, centre, bad, totals)
    over = lim["features"] // 3 + 1
    refused("features", y=torch.zeros(1, over, 3, device=DEV), sel=torch.arange(over, dtype=torch.int32, device=DEV),
            centre=torch.zeros(over, 3, dtype=torch.float64, device=DEV), bad=bad[:1])
    refused("a launch holds", y=torch.zeros(lim["structures"] + 1, 1, 3, device=DEV), sel=sel[:1],
            centre=torch.zeros(1, 3, dtype=torch.float64, device=DEV), bad=torch.zeros(lim["structures"] + 1, dtype=torch.int32, device=DEV))
    refused("float32", y=y.double())
    refused("int32", sel=sel.long())
    refused("float64", centre=centre.float())
    refused("int32", bad=bad.long())
    refused(r"\[S, n, 3\]", y=y[:, :, :2])
    refused("centre must be", centre=centre[:5])
    refused("centre must be", bad=bad[:3])
    refused("totals", totals=pca.new_totals(3 * m + 3, DEV))
    refused("totals", totals=dict(totals, n_good=totals["n_good"].long()))
    assert not totals["cov"].any() and not totals["sum"].any() and int(totals["n_good"][0]) == 0

    mean, proj = torch.zeros(3 * m, dtype=torch.float64, device=DEV), torch.zeros(S, 2, dtype=torch.float64, device=DEV)
    W = torch.zeros(3 * m, 2, dtype=torch.float64, device=DEV)
    counts, outside = torch.zeros(4, 4, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for match, kw in (("1..8 modes", dict(W=torch.zeros(3 * m, 9, dtype=torch.float64, device=DEV))), ("float64", dict(W=W.float())),
                      ("float64", dict(mean=mean[:5])), ("proj must be", dict(proj=proj[:3])),
                      ("n_bins2", dict(hist=(0, 1, lim["bins2"] + 1, (0, 1), (0, 1), counts, outside))),
                      ("components", dict(hist=(0, 2, 4, (0, 1), (0, 1), counts, outside))),
                      ("lo < hi", dict(hist=(0, 1, 4, (1, 1), (0, 1), counts, outside))),
                      ("int32", dict(hist=(0, 1, 4, (0, 1), (0, 1), counts.long(), outside)))):
        args = dict(mean=mean, W=W, proj=proj, hist=None)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            pca.project_launch(y, sel, centre, bad, args["mean"], args["W"], args["proj"], args["hist"])
    with pytest.raises(ValueError, match="target must be"):
        pca.moments(np.zeros((4, 6, 3), np.float32), np.zeros((5, 3)), device=DEV)


# ----------------------------------------------------------------------------- 9. the command line
def test_the_command_line_writes_its_statistics_and_the_model(tmp_path, capsys):
    sets = _planted_sets()
    n = 12
    np.savez(tmp_path / "ref.npz", xyz=sets["ref"], z=np.full(n, 6), bonds=np.zeros((0, 2), np.int64))
    np.savez(tmp_path / "gen.npz", xyz=sets["half"].reshape(100, 4, n, 3))
    out, model_path = tmp_path / "pca_stats.json", tmp_path / "model.npz"
    capsys.readouterr()
    stats = pca.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -pca_atoms all -pca_dim 2 -pca_bins 8 -model {model_path} "
                     f"-out {out} -device {DEV}".split())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["out"] == str(out) and line["pca_stats"] == json.loads(json.dumps(pca.summary_of(stats)))
    with open(out) as f:
        written = json.load(f)
    assert tuple(written) == pca.PCA_STATS_KEYS and written == json.loads(json.dumps(stats))
    assert written["total_variance_ratio"] < 0.5 and written["params"]["atoms_rule"] == "all" and written["n_gen"] == 400
    model = pca.PcaModel.load(str(model_path))
    assert model.W.shape == (36, 2) and model.sel.tolist() == list(range(n)) and model.n_good == 400
    assert model.eigenvalues[:2].tolist() == written["eigenvalues_ref"]
    proj = pca.project(model, sets["ref"][:50], device=DEV)
    assert proj["proj"].shape == (50, 2) and np.isfinite(proj["proj"]).all()
