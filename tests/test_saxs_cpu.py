"""SAXS profiles, host side: the numpy restatement against the fp64 Debye sum within the DERIVED binning bound, the fit, the
Guinier limit, the weights, the refusals, the command line's files and the library's symbols -- all without a device."""
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, build, saxs

F = np.float32
U = 2.0 ** -24                                                      # the unit roundoff of fp32


def _molecule(m, seed, positive=False):
    """``(xyz [2, m, 3] fp32, wq [m])``: random clouds about 20 A across; weights of both signs (a contrast: most positive,
    some negative) or all positive."""
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(size=(2, m, 3)) * 6.0).astype(F)
    w = rng.uniform(2.0, 9.0, m) if positive else rng.uniform(-3.0, 9.0, m)
    return xyz, saxs.quantise(w)


def _debye(x, wq, q):
    """The fp64 brute-force Debye sum over the same quantised weights: ``[sum wq_i^2 + 2 sum_{i<j} wq_i wq_j sinc(q r_ij)] / 256``."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(wq, dtype=np.float64)
    i, j = np.triu_indices(x.shape[0], 1)
    r = np.linalg.norm(x[i] - x[j], axis=1)
    return ((w * w).sum() + 2.0 * ((w[i] * w[j])[None, :] * np.sinc(np.outer(q, r) / np.pi)).sum(1)) / 256.0


# ----------------------------------------------------------------------------- the restatement against fp64 brute force
@pytest.mark.parametrize("m", [5, 40, 300])
def test_restate_and_profile_against_the_fp64_debye_sum_within_the_binning_bound(m):
    """|I_binned - I_Debye| <= 0.4362 * q * (w + 16 u r_max) * sum_{i<j} |wq_i wq_j| / 256: |sinc'| <= 0.4362, a pair's bin
    centre is at most w / 2 from its distance, and the fp32 chain (three differences, three squares, two sums, the square
    root, the product with a rounded scale: each at most u relative, 6 u on the bin coordinate) can move a pair that sits
    within 6 u r_max of a bin edge into the neighbouring bin, counted here as 8 u r_max per pair (twice in the bound as in
    the w term).  The fp64 sums themselves: 1e-12 relative of sum |wq_i wq_j|."""
    xyz, wq = _molecule(m, m)
    r_max, n_bins = 64.0, 640
    w = r_max / n_bins
    res = saxs.restate(xyz, np.arange(m), wq, r_max, n_bins)
    assert not res["bad"].any() and not res["beyond"].any() and res["hist"].shape == (2, n_bins)
    assert (res["hist"] < 0).any() and (res["hist"] > 0).any()                       # mixed-sign weights reach the cells
    q = np.linspace(0.0, 0.5, 26)
    got = saxs.profile(res["hist"], res["self_term"], q, res["r_max"])
    i, j = np.triu_indices(m, 1)
    A = float(np.abs(wq[i].astype(np.float64) * wq[j]).sum())
    worst = 0.0
    for s in range(2):
        bound = saxs.SINC_SLOPE * q * (w + 16 * U * r_max) * A / 256.0 + 1e-12 * A
        diff = np.abs(got[s] - _debye(xyz[s], wq, q))
        print(f"m = {m}, structure {s}: largest difference / bound = {np.max(diff[1:] / bound[1:]):.4f}")
        assert (diff <= bound).all()
        worst = max(worst, float(diff.max()))
    assert worst > 0                                                                # the binning is an approximation: it shows
    # the conservation identities, exact in integers
    assert res["self_term"] == int((wq.astype(np.int64) ** 2).sum()) and res["wq_sum"] == int(wq.sum())
    assert (res["self_term"] + 2 * res["hist"].sum(1) == res["wq_sum"] ** 2).all()
    assert np.array_equal(saxs.i_zero(res["hist"], res["self_term"]), np.full(2, res["wq_sum"] ** 2 / 256.0))
    assert np.allclose(got[:, 0], res["wq_sum"] ** 2 / 256.0, rtol=1e-14)


@pytest.mark.parametrize("m", [5, 40, 300])
@pytest.mark.parametrize("positive", [False, True])
def test_rg_against_the_brute_force_weighted_rg(m, positive):
    """Rg^2 = sum_{i<j} w_i w_j r_ij^2 / W^2 (W the sum of the weights) equals the weighted mean square distance from the
    weighted centroid, the form computed here.  |r_b^2 - r^2| = |r_b - r| (r_b + r) <= (w / 2 + 8 u r_max) * 2 r_max, so
    |Rg^2_binned - Rg^2| <= (w + 16 u r_max) * r_max * sum_{i<j} |w_i w_j| / W^2: within w * r_max, the issue's margin,
    whenever that last factor is below 1 -- it is at most 1 / 2 for weights of one sign, and asserted for the mixed ones."""
    xyz, wq = _molecule(m, 100 + m, positive)
    r_max, n_bins = 64.0, 640
    w = r_max / n_bins
    res = saxs.restate(xyz, np.arange(m), wq, r_max, n_bins)
    assert not res["beyond"].any()
    wf = wq.astype(np.float64)
    i, j = np.triu_indices(m, 1)
    factor = float(np.abs(wf[i] * wf[j]).sum()) / float(wf.sum()) ** 2
    assert factor < 1.0
    got = saxs.rg(res["hist"], res["wq_sum"], res["r_max"])
    for s in range(2):
        x = xyz[s].astype(np.float64)
        c = (wf[:, None] * x).sum(0) / wf.sum()
        want2 = float((wf * ((x - c) ** 2).sum(1)).sum() / wf.sum())
        print(f"m = {m}: Rg^2 {got[s] ** 2:.4f} against {want2:.4f}, margin {w * r_max:.2f}")
        assert abs(got[s] ** 2 - want2) <= (w + 16 * U * r_max) * r_max * factor + 1e-9 * want2
        assert abs(got[s] ** 2 - want2) <= w * r_max
    assert saxs.rg(res["hist"], 0, res["r_max"]) is None                             # weights that sum to zero: not defined
    d = saxs.dmax(res["hist"], res["r_max"])
    far = [np.linalg.norm(xyz[s][i].astype(np.float64) - xyz[s][j], axis=1).max() for s in range(2)]
    assert all(far[s] <= d[s] <= far[s] + w * (1 + 1e-6) for s in range(2))
    p = saxs.pr(res["hist"], res["r_max"])
    assert np.allclose(p["p"].sum(1) * p["width"], (wf[i] * wf[j]).sum() / 256.0, rtol=1e-12) and p["r"][0] == w / 2


def test_the_bin_rule_on_hand_placed_pairs():
    # r_max = 2, four bins of 0.5 (scale 2); weights 1, 2, -3 -> wq 16, 32, -48
    x = np.zeros((1, 3, 3), F)
    x[0, :, 0] = [0.0, 1.5, 2.0]
    wq = saxs.quantise([1.0, 2.0, -3.0])
    assert wq.tolist() == [16, 32, -48] and wq.dtype == np.int32
    res = saxs.restate(x, [0, 1, 2], wq, 2.0, 4)
    # d01 = 1.5 -> exactly 3: the UPPER bin; d12 = 0.5 -> exactly 1; d02 = 2.0 is exactly r_max: beyond, the test is strict
    assert res["hist"].tolist() == [[0, 32 * -48, 0, 16 * 32]] and res["beyond"].tolist() == [1] and res["bad"].tolist() == [False]
    x[0, 2, 0] = 0.0                                                 # two coincident atoms: bin 0
    res = saxs.restate(x, [0, 1, 2], wq, 2.0, 4)
    assert res["hist"].tolist() == [[16 * -48, 0, 0, 16 * 32 + 32 * -48]] and res["beyond"].tolist() == [0]
    x[0, 1, 1] = np.nan
    res = saxs.restate(x, [0, 2], [16, -48], 2.0, 1)                 # the NaN is outside the selection
    assert res["hist"].tolist() == [[-768]] and not res["bad"].any()
    res = saxs.restate(x, [0, 1, 2], wq, 2.0, 4)
    assert res["bad"].tolist() == [True] and not res["hist"].any() and res["n_good"] == 0
    more = saxs.restate(np.zeros((2, 3, 3), F), [0, 1, 2], wq, 2.0, 4, into=res)
    assert more["hist"].shape == (3, 4) and more["bad"].tolist() == [True, False, False] and more["n_good"] == 2
    with pytest.raises(ValueError, match="another selection"):
        saxs.restate(np.zeros((2, 3, 3), F), [0, 1, 2], wq, 2.0, 5, into=res)


# ----------------------------------------------------------------------------- fit, guinier
@pytest.mark.parametrize("background", [False, True])
def test_fit_gives_back_scale_and_background(background):
    xyz, wq = _molecule(40, 7, positive=True)
    res = saxs.restate(xyz, np.arange(40), wq, 64.0, 640)
    q = np.linspace(0.01, 0.45, 60)
    model = saxs.profile(res["hist"], res["self_term"], q, res["r_max"])
    c, k = 3.7e-4, (1.25 if background else 0.0)
    rng = np.random.default_rng(1)
    sigma = rng.uniform(0.01, 5.0, q.shape[0])                       # any sigma: an exact curve is fitted exactly
    one = saxs.fit(model[0], q, c * model[0] + k, sigma, background=background)
    assert one["scale"] == pytest.approx(c, rel=1e-11) and one["chi2"] < 1e-12 and one["n_points"] == 60
    if background:
        assert one["background"] == pytest.approx(k, rel=1e-9)
    else:
        assert "background" not in one
    both = saxs.fit(model, q, c * model[1] + k, sigma, background=background)
    assert both["scale"].shape == (2,) and both["chi2"][1] < 1e-12 and both["chi2"][0] > 1e-3     # the other structure does not fit
    with pytest.raises(ValueError, match="one length"):
        saxs.fit(model[0], q[:-1], model[0, :-1] * c, sigma)
    with pytest.raises(ValueError, match="sigma"):
        saxs.fit(model[0], q, model[0], np.zeros_like(q))


def test_the_guinier_rg_approaches_the_real_space_rg_as_the_window_shrinks():
    xyz, wq = _molecule(300, 3, positive=True)
    res = saxs.restate(xyz[:1], np.arange(300), wq, 64.0, 640)
    real = float(saxs.rg(res["hist"], res["wq_sum"], res["r_max"])[0])
    q = np.linspace(0.0, 0.2, 401)
    prof = saxs.profile(res["hist"][0], res["self_term"], q, res["r_max"])
    errors = []
    for limit in (1.3, 0.8, 0.4):                                    # q_max * Rg
        g = saxs.guinier(q, prof, q_max=limit / real)
        errors.append(abs(g["rg"] - real))
        assert g["n_points"] >= 10 and g["i0"] == pytest.approx(prof[0], rel=0.05)
    print("Guinier Rg errors:", errors, "real-space Rg", real)
    assert errors[0] > errors[1] > errors[2]
    with pytest.raises(ValueError, match="two points"):
        saxs.guinier(q[:1], prof[:1])


# ----------------------------------------------------------------------------- weights
def test_weights_of_folds_hydrogens_onto_their_heavy_atom():
    # methanol-like: C(0) H H H, O(4) H
    z = np.array([6, 1, 1, 1, 8, 1])
    bonds = np.array([[0, 1], [2, 0], [0, 3], [0, 4], [4, 5]])
    heavy = np.flatnonzero(z != 1)
    assert saxs.weights_of(z, bonds, heavy, solvent=0).tolist() == [9.0, 9.0]        # 6 + 3 and 8 + 1 electrons
    assert saxs.weights_of(z, bonds, np.arange(6), solvent=0).tolist() == [6.0, 1.0, 1.0, 1.0, 8.0, 1.0]
    assert saxs.weights_of(z, bonds, heavy, solvent=0, fold_h=False).tolist() == [6.0, 8.0]
    assert saxs.weights_of(z, bonds, [4, 0], solvent=0).tolist() == [9.0, 9.0] and saxs.weights_of(z, bonds, [0, 1], solvent=0, fold_h=True).tolist() == [8.0, 1.0]
    # in solvent: every weight drops by the density times a volume read from the ONE table, whatever its values
    v = saxs.DISPLACED_VOLUME
    w = saxs.weights_of(z, bonds, heavy, solvent=0.5)
    assert w.tolist() == [9.0 - 0.5 * (v[6] + 3 * v[1]), 9.0 - 0.5 * (v[8] + v[1])]
    assert saxs.weights_of(z, bonds, heavy).tolist() == saxs.weights_of(z, bonds, heavy, solvent=saxs.RHO0).tolist()
    with pytest.raises(ValueError, match="no displaced volume"):
        saxs.weights_of(np.array([6, 26]), np.zeros((0, 2), int), [0, 1])
    assert saxs.weights_of(np.array([6, 26]), np.zeros((0, 2), int), [0, 1], solvent=0).tolist() == [6.0, 26.0]
    with pytest.raises(ValueError, match="solvent"):
        saxs.weights_of(z, bonds, heavy, solvent=-1.0)


# ----------------------------------------------------------------------------- refusals
def test_every_value_error_comes_before_a_device_is_touched():
    n = 6
    xyz = np.zeros((4, n, 3), F)
    sel, wq = np.arange(n), np.full(n, 16, np.int32)
    lim = saxs.limits()
    with pytest.raises(ValueError, match="out of range"):
        saxs.quantise([1.0, 2048.0])
    with pytest.raises(ValueError, match="out of range"):
        saxs.quantise([-2047.97])
    assert saxs.quantise([2047.9, -2047.9]).tolist() == [32766, -32766]
    with pytest.raises(ValueError, match="not finite"):
        saxs.quantise([np.nan])
    for f in (saxs.saxs_hist, saxs.restate):
        def refused(match, x=xyz, s=sel, w=wq, r_max=10.0, n_bins=100, **kw):
            with pytest.raises(ValueError, match=match):
                f(x, s, w, r_max, n_bins, **kw)
        refused("out of range", w=np.array([16] * (n - 1) + [32768]))
        refused("out of range", w=np.array([16] * (n - 1) + [-32768]))
        refused("wq must be", w=wq[:-1])
        refused("wq must be", w=wq.astype(np.float64))
        refused("n_bins must be", n_bins=0)
        refused("n_bins must be", n_bins=lim["bins"] + 1)
        for r_max in (0.0, -1.0, float("nan"), float("inf")):
            refused("r_max", r_max=r_max)
        refused(r"\[S, n, 3\]", x=np.zeros((4, n), F))
        refused("twice", s=[0, 0, 1, 2, 3, 4])
        refused("selection is empty", s=[], w=[])
        big = lim["atoms"] + 1
        refused("the kernel holds", x=np.zeros((1, big, 3), F), s=np.arange(big), w=np.ones(big, np.int32))
    with pytest.raises(ValueError, match="chunk"):
        saxs.saxs_hist(xyz, sel, wq, 10.0, 100, chunk=lim["structures"] + 1)
    with pytest.raises(ValueError, match="chunk"):
        saxs.saxs_hist(xyz, sel, wq, 10.0, 100, chunk=0)
    with pytest.raises(ValueError, match="split"):
        saxs.saxs_hist(xyz, sel, wq, 10.0, 100, split=-1)
    with pytest.raises(ValueError, match="at least two reference frames"):
        saxs.compare(xyz, xyz[:1], sel, wq)
    with pytest.raises(ValueError, match="bins .the kernel holds"):
        saxs.compare(xyz, xyz, sel, wq, r_max=100.0, bin_width=0.01)
    with pytest.raises(RuntimeError, match="device"):               # everything before the launch went through
        saxs.saxs_hist(xyz, sel, wq, 10.0, 100, device="cpu")


def test_compare_refuses_a_reference_with_pairs_beyond_r_max_and_names_one_that_would_do():
    rng = np.random.default_rng(5)
    ref = (rng.normal(size=(6, 10, 3)) * 4.0).astype(F)
    sel, wq = np.arange(10), saxs.quantise(np.full(10, 6.0))
    enough, n_bins = saxs.default_r_max(ref, sel, 0.1)
    assert n_bins == round(enough / 0.1)
    ok = [saxs.restate(x, sel, wq, enough, n_bins) for x in (ref[0::2], ref[1::2], ref)]
    assert not any(r["beyond"].any() for r in ok)                    # the default holds every pair of the reference
    stats = saxs.compare_from_hists(*ok, saxs.q_grid(0.5, 11))
    assert tuple(stats) == saxs.SAXS_STATS_KEYS and stats["log_rms"] == pytest.approx(0.0, abs=1e-12) and stats["n_beyond_gen"] == 0
    assert json.loads(json.dumps(stats)) == stats and stats["rg"]["jsd"] == pytest.approx(0.0, abs=1e-12)
    json.dumps(saxs.summary_of(stats))
    short = [saxs.restate(x, sel, wq, 5.0, 50) for x in (ref[0::2], ref[1::2], ref)]
    assert any(r["beyond"].any() for r in short)
    with pytest.raises(ValueError, match=r"reference structures have pairs beyond r_max = 5 A.*larger r_max"):
        saxs.compare_from_hists(*short, saxs.q_grid())
    with pytest.raises(ValueError, match=f"r_max = {enough:g} would do"):
        saxs.compare_from_hists(*short, saxs.q_grid(), enough=enough)
    # a GENERATED structure beyond r_max is counted and left out, not refused
    wide = ref.copy()
    wide[1] *= 20.0
    stats = saxs.compare_from_hists(ok[0], ok[1], saxs.restate(wide, sel, wq, enough, n_bins), saxs.q_grid(0.5, 11))
    assert stats["n_beyond_gen"] == 1 and stats["n_bad_gen"] == 0


def _files(tmp_path, n=12):
    rng = np.random.default_rng(0)
    z = np.array([6, 1, 7, 8] * (n // 4))
    bonds = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    np.savez(tmp_path / "ref.npz", xyz=(rng.normal(size=(4, n, 3)) * 3).astype(F), z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=(rng.normal(size=(2, 3, n, 3)) * 3).astype(F))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}", n, z


def test_the_parser_read_inputs_and_the_curve_file(tmp_path):
    base, n, z = _files(tmp_path)
    args = saxs.parser().parse_args(base.split())
    assert (args.saxs_atoms, args.saxs_solvent, args.saxs_rmax, args.saxs_bin, args.saxs_qmax, args.saxs_nq, args.saxs_exp, args.saxs_units,
            args.profiles, args.out) == ("heavy", 0.334, None, 0.1, 0.5, 101, None, "A", None, "saxs_stats.json")
    inp = saxs.read_inputs(args)
    assert inp["gen_xyz"].shape == (6, n, 3) and inp["sel"].tolist() == np.flatnonzero(z != 1).tolist() and inp["exp"] is None
    assert inp["q"].shape == (101,) and inp["q"][0] == 0.0 and inp["q"][-1] == 0.5 and inp["wq"].dtype == np.int32
    vac = saxs.read_inputs(saxs.parser().parse_args((base + " -saxs_solvent 0 -saxs_atoms all").split()))
    assert vac["wq"].tolist() == (16 * z).tolist()
    # the curve: comments, blank lines, a fourth column; nm units convert to 1 / A
    curve = tmp_path / "curve.dat"
    curve.write_text("# q I sigma\n\n0.1 100.0 1.0\n0.2 50.0 0.5 9\n  3.0e-1, 25.0, 0.25  # tail\n")
    q, i, s = saxs.read_curve(str(curve))
    assert q.tolist() == [0.1, 0.2, 0.3] and i.tolist() == [100.0, 50.0, 25.0] and s.tolist() == [1.0, 0.5, 0.25]
    assert saxs.read_curve(str(curve), "nm")[0].tolist() == [0.1 / 10.0, 0.2 / 10.0, 0.3 / 10.0]
    inp = saxs.read_inputs(saxs.parser().parse_args((base + f" -saxs_exp {curve} -saxs_units nm").split()))
    assert inp["exp"][0].tolist() == [0.01, 0.02, 0.03]


def test_the_command_line_refuses_before_any_launch(tmp_path):
    base, n, z = _files(tmp_path)

    def refused(extra, match):
        with pytest.raises(SystemExit, match=match):
            saxs.read_inputs(saxs.parser().parse_args((base + " " + extra).split()))
    refused("-saxs_rmax 0", "-saxs_rmax")
    refused("-saxs_rmax nan", "-saxs_rmax")
    refused("-saxs_bin 0", "-saxs_bin")
    refused("-saxs_solvent -1", "-saxs_solvent")
    refused("-saxs_qmax 0", "-saxs_qmax")
    refused("-saxs_nq 1", "-saxs_nq")
    refused("-saxs_rmax 500 -saxs_bin 0.1", "5000 bins .the kernel holds 4096.*-saxs_bin")
    refused("-saxs_bin 0.0001", "bins .the kernel holds 4096")       # the default r_max, too many bins
    refused(f"-saxs_exp {tmp_path / 'none.dat'}", "-saxs_exp")
    for k, (text, match) in enumerate([("0.1 1.0\n0.2 2.0\n", "three columns"), ("0.1 1.0 x\n0.2 1 1\n", "not a number"),
                                       ("0.1 1.0 0.0\n0.2 1 1\n", "sigma > 0"), ("-0.1 1.0 1.0\n0.2 1 1\n", "q must be"),
                                       ("0.1 nan 1.0\n0.2 1 1\n", "finite"), ("# nothing\n0.1 1 1\n", "fewer than two")]):
        bad = tmp_path / f"bad{k}.dat"
        bad.write_text(text)
        refused(f"-saxs_exp {bad}", match)
    np.savez(tmp_path / "iron.npz", z=np.full(n, 26), bonds=np.zeros((0, 2), dtype=int))
    refused(f"-top {tmp_path / 'iron.npz'}", "no displaced volume")
    np.savez(tmp_path / "heavy.npz", z=np.full(n, 92), bonds=np.zeros((0, 2), dtype=int))
    assert saxs.read_inputs(saxs.parser().parse_args((base + f" -top {tmp_path / 'heavy.npz'} -saxs_solvent 0").split()))["wq"].tolist() == [92 * 16] * n
    np.savez(tmp_path / "hydrogen.npz", z=np.ones(n, dtype=int), bonds=np.zeros((0, 2), dtype=int))
    refused(f"-top {tmp_path / 'hydrogen.npz'}", "selection is empty")
    with pytest.raises(SystemExit):
        saxs.parser().parse_args((base + " -saxs_units pm").split())


# ----------------------------------------------------------------------------- library
NAMES = {"cgv_saxs_max_atoms", "cgv_saxs_max_structures", "cgv_saxs_max_bins", "cgv_saxs_max_weight", "cgv_saxs_row_tile", "cgv_saxs_col_tile",
         "cgv_saxs_small", "cgv_saxs_pack", "cgv_saxs_blocks", "cgv_saxs_workspace_bytes", "cgv_saxs_hist"}


def test_the_library_declares_binds_and_exports_the_scattering_kernel():
    assert NAMES <= set(_lib.header_symbols()) and NAMES <= set(_lib.PROTOTYPES)
    assert build.SOURCE_FLAGS["saxs_hist.hip"] == ["-ffp-contract=off"]
    lim = saxs.limits()
    assert lim == {"structures": lim["structures"], "atoms": 8192, "bins": 4096, "weight": saxs.MAX_WEIGHT} and lim["structures"] >= 65536
    assert lim["weight"] ** 2 < 2 ** 30 and lim["atoms"] * (lim["atoms"] - 1) // 2 < 2 ** 25          # the overflow bound of the header
    lib = _lib.load()
    assert lib.cgv_saxs_workspace_bytes(10, 5) >= 10 * 5 * 16 and lib.cgv_saxs_workspace_bytes(10, 5) % 16 == 0
    assert lib.cgv_saxs_workspace_bytes(10, lim["atoms"] + 1) == 0 and lib.cgv_saxs_workspace_bytes(lim["structures"] + 1, 5) == 0
    assert lib.cgv_saxs_workspace_bytes(-1, 5) == 0
    rt, ct, small = lib.cgv_saxs_row_tile(), lib.cgv_saxs_col_tile(), lib.cgv_saxs_small()
    assert rt == 64 and ct % 32 == 0 and small <= rt
    assert [lib.cgv_saxs_pack(22, nb) for nb in (1, 1024, 1025, 2048, 2049, 4096)] == [4, 4, 2, 2, 1, 1]
    assert all(p * nb * 8 <= 32 * 1024 for nb in (1, 1024, 1025, 2048, 2049, 4096) for p in [lib.cgv_saxs_pack(22, nb)])
    assert lib.cgv_saxs_blocks(1, small, 0) == 1 and lib.cgv_saxs_blocks(1, 193, 0) == 4 and lib.cgv_saxs_blocks(1, 193, 2) == 2
    assert lib.cgv_saxs_blocks(1, 193, 99) == 4 and lib.cgv_saxs_blocks(lim["structures"], 193, 0) == 1


def test_the_c_entry_refuses_with_its_reason():
    lib, lim = _lib.load(), saxs.limits()

    def call(S, m, n_bins=100, rmax2=400.0, scale=5.0, split=0):
        return lib.cgv_saxs_hist(None, None, None, S, 1 << 20, m, n_bins, rmax2, scale, split, None, None, None, None, 0, None)

    def refused(reason, *a, **kw):
        assert call(*a, **kw) == -1 and reason in lib.cgv_last_error_string(), lib.cgv_last_error_string()
    refused(b"cgv_saxs_max_atoms", 1, lim["atoms"] + 1)
    refused(b"cgv_saxs_max_structures", lim["structures"] + 1, 4)
    refused(b"cgv_saxs_max_bins", 1, 4, n_bins=lim["bins"] + 1)
    refused(b"cgv_saxs_max_bins", 1, 4, n_bins=0)
    refused(b"1 <= m", 1, 0)
    refused(b"rmax2", 1, 4, rmax2=float("nan"))
    refused(b"rmax2", 1, 4, rmax2=float("inf"))
    refused(b"scale", 1, 4, scale=0.0)
    refused(b"scale", 1, 4, scale=float("nan"))
    refused(b"split", 1, 4, split=-1)
    refused(b"null pointer", 1, 4)
    assert call(0, 4) == 0                                           # nothing to do
