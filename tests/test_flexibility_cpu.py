"""Mean structure and RMSF without a GPU: the numpy restatement on constructed cases, the host statistics of
``flexibility`` (group profiles, ``compare_from_runs``), the C ABI's declarations and refusals, and the command lines."""
import ctypes as C
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, backmap as bm, flexibility, run_ala
import flexibility_restatement as R


def _base(n, seed):
    return np.random.default_rng(seed).uniform(0, 10, (n, 3))


# ----------------------------------------------------------------------------- the restatement on constructed cases
def test_rigid_copies_have_no_fluctuation_and_a_mean_congruent_to_the_base():
    rng = np.random.default_rng(1)
    base = _base(17, 1)
    x = R.noisy_copies(rng, base, 40, 0.0)
    sel = rng.permutation(17)[:11]
    got = R.mean_structure(x, sel)
    assert got["iterations"] == 2 and got["converged"] and got["n_good"] == 40 and not got["bad"].any()
    # fp32 storage of coordinates up to 20 A moves an atom by up to 2^-24 x 20 x sqrt(3) = 2e-6 A
    assert got["rmsf"].max() < 1e-5 and got["rmsd"].max() < 1e-5
    d = lambda p: np.linalg.norm(p[:, None] - p[None], axis=-1)
    assert np.abs(d(got["mean"]) - d(base)).max() < 1e-5
    assert np.abs(got["mean"][sel].mean(0)).max() < 1e-12
    # a proper rotation: the signed volume of four atoms keeps its sign
    vol = lambda p: np.linalg.det(p[1:4] - p[0])
    assert vol(got["mean"]) * vol(base) > 0


def _fitted_msf(base, sigma):
    """First-order mean-square fluctuation of every atom after a least-squares rigid-body fit on all atoms: the noise
    passes through I - P, P the projector onto the six rigid-body modes (three translations, three infinitesimal
    rotations about the centroid) of the 3n coordinates."""
    n = base.shape[0]
    c = base - base.mean(0)
    modes = np.zeros((6, n, 3))
    for k in range(3):
        modes[k, :, k] = 1.0
        axis = np.zeros(3)
        axis[k] = 1.0
        modes[3 + k] = np.cross(axis, c)
    q = np.linalg.qr(modes.reshape(6, -1).T)[0]
    A = np.eye(3 * n) - q @ q.T
    cov = (A * np.repeat(sigma ** 2, 3)[None, :]) @ A.T
    return np.diag(cov).reshape(n, 3).sum(1)


def test_isotropic_noise_gives_sqrt3_sigma_per_atom_within_the_sampling_error():
    """Atom i gets Gaussian noise of sigma_i per component, S = 4000 structures.  S x msf_i / E[msf_i] is close to
    chi-squared with 3 S degrees of freedom: relative standard deviation sqrt(2 / (3 S)) = 0.0129 of msf_i, half of
    that, 0.0065, of rmsf_i; the bound is 5 of those, 0.032, plus 0.01 for what the first-order expectation leaves
    out (second order in sigma / extent: (0.3 / 4)^2 = 0.006).  E[msf_i] is 3 sigma_i^2 less what the fit of six
    rigid-body parameters on the 40 atoms absorbs and plus what it smears from the noisier atoms (_fitted_msf); without
    that correction the same bound holds with the correction's own size added, and the quietest atom shows why it is
    needed."""
    rng = np.random.default_rng(2)
    n, S = 40, 4000
    base, sigma = _base(n, 2), rng.uniform(0.05, 0.3, n)
    got = R.mean_structure(R.noisy_copies(rng, base, S, sigma))
    assert got["converged"] and 2 <= got["iterations"] <= 6
    sampling = 5 * 0.5 * np.sqrt(2.0 / (3 * S)) + 0.01
    expected = np.sqrt(_fitted_msf(base, sigma))
    rel = got["rmsf"] / expected - 1.0
    raw = got["rmsf"] / (np.sqrt(3.0) * sigma) - 1.0
    fit = np.abs(expected / (np.sqrt(3.0) * sigma) - 1.0)
    print("rmsf / expected - 1: min", rel.min(), "max", rel.max(), "; against sqrt(3) sigma:", raw.min(), raw.max(), "fit", fit.max())
    assert np.abs(rel).max() < sampling
    assert (np.abs(raw) < sampling + fit).all()
    assert np.corrcoef(got["rmsf"], sigma)[0, 1] > 0.99
    # uniform noise on many atoms: the fit takes 6 / (3 n) of the variance, 1 % of the RMSF at n = 100
    flat = R.mean_structure(R.noisy_copies(rng, _base(100, 7), 1500, 0.2))
    assert np.abs(flat["rmsf"] / (np.sqrt(3.0) * 0.2) - 1.0).max() < 5 * 0.5 * np.sqrt(2.0 / (3 * 1500)) + 0.01 + 0.03


def test_a_mirror_image_is_not_superposed():
    rng = np.random.default_rng(3)
    base = _base(12, 3)
    mirrored = (base * [1, 1, -1]) @ R.random_rotation(rng).T
    res = R.align_accumulate(np.stack([mirrored, base @ R.random_rotation(rng).T]).astype(np.float32), np.arange(12), base)
    assert res["rmsd2"][1] < 1e-10 and res["rmsd2"][0] > 1.0
    for s in range(2):
        Rm = R.rotation(np.eye(3))[0]
        assert abs(np.linalg.det(Rm) - 1.0) < 1e-12


def test_bad_structures_enter_nothing_in_the_restatement():
    rng = np.random.default_rng(4)
    x = R.noisy_copies(rng, _base(9, 4), 6, 0.2)
    x[0, 8, 1], x[3, 2, 0] = np.nan, np.inf
    got = R.mean_structure(x, [0, 1, 2, 3, 4])
    clean = R.mean_structure(x[[1, 2, 4, 5]], [0, 1, 2, 3, 4])
    assert got["bad"].tolist() == [True, False, False, True, False, False] and got["n_good"] == 4
    assert np.isnan(got["rmsd"][[0, 3]]).all() and np.array_equal(got["rmsd"][[1, 2, 4, 5]], clean["rmsd"])
    assert np.array_equal(got["mean"], clean["mean"]) and np.array_equal(got["rmsf"], clean["rmsf"])
    none = R.mean_structure(np.full((2, 4, 3), np.nan, np.float32))
    assert none["mean"] is None and none["n_good"] == 0 and none["iterations"] == 0


# ----------------------------------------------------------------------------- host statistics
def test_group_profiles_on_a_hand_made_grouping():
    rmsf = np.array([1.0, 9.0, 3.0, 4.0, 0.0, 2.0])
    sel = [5, 0, 2, 3]                                         # fluctuations 2, 1, 3, 4
    rows, prof = flexibility.group_profile(rmsf, sel)
    assert rows == sel and prof.tolist() == [2.0, 1.0, 3.0, 4.0]
    rows, prof = flexibility.group_profile(rmsf, sel, [7, 3, 7, 3])
    assert rows == [3, 7]
    assert np.allclose(prof, [np.sqrt((1.0 + 16.0) / 2), np.sqrt((4.0 + 9.0) / 2)], rtol=0, atol=1e-15)
    want = R.group_profile(rmsf, sel, [7, 3, 7, 3])
    assert want[0] == rows and np.allclose(want[1], prof, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="labels lists"):
        flexibility.group_profile(rmsf, sel, [1, 2])


def test_compare_from_runs_on_two_amplitudes():
    """The generated set has 0.6 times the reference's noise at every atom: the ratio of the mean RMSF is 0.6 within
    the sampling error (1200 and 900 structures: 5 sigma of the ratio of two means over 30 atoms is below 0.02; the
    fit's bias is the same fraction on both sides and cancels), and the profiles are proportional: pearson near 1."""
    rng = np.random.default_rng(5)
    n = 30
    base, sigma = _base(n, 5), rng.uniform(0.05, 0.3, n)
    ref, gen = R.noisy_copies(rng, base, 1200, sigma), R.noisy_copies(rng, base, 900, 0.6 * sigma)
    sel = np.arange(2, n)
    runs = {"ref": R.mean_structure(ref, sel), "gen": R.mean_structure(gen, sel), "even": R.mean_structure(ref[0::2], sel),
            "odd": R.mean_structure(ref[1::2], sel)}
    stats = flexibility.compare_from_runs(runs, sel, mean_rmsd=0.01, floor_mean_rmsd=0.02, n_bins=10, params={"atoms": sel.tolist()})
    assert set(stats) == set(flexibility.FLEX_STATS_KEYS) and json.loads(json.dumps(stats)) == stats
    assert stats["n_ref"] == 1200 and stats["n_gen"] == 900 and stats["n_bad_ref"] == stats["n_bad_gen"] == 0
    assert stats["labels"] == sel.tolist() and len(stats["rmsf_ref"]) == n - 2
    assert abs(stats["ratio"] - 0.6) < 0.02 and stats["pearson"] > 0.99
    assert abs(stats["floor"]["ratio"] - 1.0) < 0.03 and stats["floor"]["pearson"] > 0.99
    assert stats["floor"]["profile_rmse"] < stats["profile_rmse"] and stats["floor"]["mean_rmsd"] == 0.02
    assert stats["mean_rmsd"] == 0.01 and stats["params"]["n_bins"] == 10
    block = stats["rmsd_to_mean"]
    assert block["mean_gen"] < 0.7 * block["mean_ref"] and block["jsd"] > block["floor"] >= 0.0
    assert sum(block["hist_gen"]["counts"]) + block["hist_gen"]["over"] == 900 and block["range"][0] == 0.0
    assert len(stats["top_atoms"]) == 10
    worst = int(np.argmax(np.abs(np.array(stats["rmsf_gen"]) - np.array(stats["rmsf_ref"]))))
    assert stats["top_atoms"][0]["label"] == stats["labels"][worst]
    assert set(stats["convergence"]) == {"ref", "gen", "even", "odd"} and stats["convergence"]["ref"]["converged"]
    short = flexibility.summary_of(stats)
    assert "rmsf_ref" not in short and "labels" not in short and "hist_ref" not in short["rmsd_to_mean"]
    assert short["ratio"] == stats["ratio"] and short["floor"] == stats["floor"]
    # groups: rows per label
    grouped = flexibility.compare_from_runs(runs, sel, group_labels=np.arange(n - 2) // 7)
    assert grouped["labels"] == [0, 1, 2, 3] and len(grouped["rmsf_gen"]) == 4 and abs(grouped["ratio"] - 0.6) < 0.02
    # a set without a good structure
    empty = R.mean_structure(np.full((3, n, 3), np.nan, np.float32), sel)
    none = flexibility.compare_from_runs(dict(runs, gen=empty), sel)
    assert none["rmsf_gen"] is None and none["pearson"] is None and none["ratio"] is None and none["rmsd_to_mean"] is None
    assert none["n_bad_gen"] == 3 and none["top_atoms"] == [] and none["rmsf_ref"] is not None


# ----------------------------------------------------------------------------- refusals before any launch
def test_host_wrappers_refuse_bad_arguments_without_a_launch():
    x = np.zeros((4, 6, 3), np.float32)
    with pytest.raises(ValueError, match="names atom 6"):
        flexibility.mean_structure(x, [0, 1, 6])
    with pytest.raises(ValueError, match="m = 0"):
        flexibility.mean_structure(x, [])
    with pytest.raises(ValueError, match="at least 3"):
        flexibility.mean_structure(x, [0, 1])
    with pytest.raises(ValueError, match="twice"):
        flexibility.mean_structure(x, [1, 1, 2])
    with pytest.raises(ValueError, match=r"\[S, n, 3\]"):
        flexibility.mean_structure(x[0])
    with pytest.raises(ValueError, match="max_iter"):
        flexibility.mean_structure(x, max_iter=0)
    with pytest.raises(ValueError, match="atoms per structure"):
        flexibility.mean_structure(np.zeros((1, flexibility.limits()["atoms"] + 1, 3), np.float32))
    z, bonds = np.full(6, 6), [(0, 1)]
    with pytest.raises(ValueError, match="two reference frames"):
        flexibility.compare(x[:1], x, z, bonds)
    with pytest.raises(ValueError, match="groups must be"):
        flexibility.compare(x, x, z, bonds, groups="chain")
    with pytest.raises(ValueError, match="at least 3"):
        flexibility.compare(x, x, np.array([6, 6, 1, 1, 1, 1]), bonds)
    with pytest.raises(ValueError, match="need the coarse-graining mapping"):
        flexibility.compare(x, x, z, bonds, groups="bead")
    with pytest.raises(ValueError, match="need a peptide"):
        flexibility.compare(x, x, z, bonds, groups="residue")


def test_the_header_declares_the_entry_points_and_the_source_is_compiled_uncontracted():
    from coarsegrainingvae_amd import build, options
    names = ("cgv_align_accumulate", "cgv_align_workspace_bytes", "cgv_align_max_atoms", "cgv_align_max_structures",
             "cgv_align_wave_fits")
    declared = _lib.header_symbols()
    assert declared == sorted(_lib.PROTOTYPES)
    assert all(n in declared and n in _lib.PROTOTYPES for n in names)
    assert build.SOURCE_FLAGS["align_mean.hip"] == ["-ffp-contract=off"]
    assert len(_lib.PROTOTYPES["cgv_align_accumulate"][1]) == 16
    assert options.HOST["align_form"] == 0


def test_the_limits_are_refused_before_any_launch():
    lib, lim = _lib.load(), flexibility.limits()
    assert lim == {"structures": 1 << 20, "atoms": 4096}
    assert lib.cgv_align_wave_fits(256) == 1 and lib.cgv_align_wave_fits(257) == 0 and lib.cgv_align_wave_fits(0) == 0
    # ranges of at least 4 structures, 4 fp64 per atom and range
    assert lib.cgv_align_workspace_bytes(257, 22, 0) == 65 * 4 * 22 * 8 and lib.cgv_align_workspace_bytes(3, 300, 0) == 4 * 300 * 8
    assert lib.cgv_align_workspace_bytes(1 << 20, 22, 0) == 4096 * 4 * 22 * 8 and lib.cgv_align_workspace_bytes(1 << 20, 22, 2) == 512 * 4 * 22 * 8
    assert lib.cgv_align_workspace_bytes(lim["structures"] + 1, 22, 0) == 0 and lib.cgv_align_workspace_bytes(4, lim["atoms"] + 1, 0) == 0
    assert lib.cgv_align_workspace_bytes(4, 300, 1) == 0 and lib.cgv_align_workspace_bytes(4, 30, 3) == 0

    def call(S, n, m, form=0):
        return lib.cgv_align_accumulate(None, None, None, S, n, m, form, None, None, None, None, None, None, None, 0, None)
    assert call(-1, 5, 3) == -1 and call(lim["structures"] + 1, 5, 3) == -1 and call(4, lim["atoms"] + 1, 3) == -1
    assert call(4, 5, 0) == -1 and call(4, 5, 6) == -1 and call(4, 5, 3, 3) == -1 and call(4, 300, 3, 1) == -1
    assert call(4, 5, 3) == -1 and b"null" in lib.cgv_last_error_string()
    assert call(0, 5, 3) == 0                                              # no structures: nothing to do


# ----------------------------------------------------------------------------- command line
BASE = "-model D -cg c.npz -n_samples 4 -out o.npz"


def test_both_parsers_accept_the_switches_and_are_unchanged_without_them():
    p = bm.build_parser()
    off = p.parse_args(BASE.split())
    assert not any(k.startswith("flex") for k in vars(off))                 # what it parsed to before the switches existed
    assert bm.flex_args(off) == bm.FLEX_DEFAULTS == {"flex_stats": False, "flex_atoms": "heavy", "flex_groups": "none",
                                                     "flex_aligned": None}
    on = p.parse_args(f"{BASE} --flex_stats -flex_atoms all -flex_groups residue -flex_aligned a.npz".split())
    assert bm.flex_args(on) == {"flex_stats": True, "flex_atoms": "all", "flex_groups": "residue", "flex_aligned": "a.npz"}
    assert bm.flex_args(p.parse_args(f"{BASE} --flex_stats".split()))["flex_atoms"] == "heavy"
    for bad in ("-flex_atoms backbone", "-flex_groups chain"):
        with pytest.raises(SystemExit):
            p.parse_args(f"{BASE} --flex_stats {bad}".split())
    assert "flex_eval" not in vars(run_ala.build_extras_parser().parse_args([]))
    assert vars(run_ala.build_extras_parser().parse_args(["--flex_eval"]))["flex_eval"] is True
    assert not any("flex" in k for k in vars(run_ala.build_parser().parse_args("-logdir x".split())))
    got, rest = run_ala.build_extras_parser().parse_known_args("-logdir x --flex_eval -n_cgs 3".split())
    assert got.flex_eval and rest == ["-logdir", "x", "-n_cgs", "3"]
    params = vars(run_ala.build_parser().parse_args("-logdir x".split()))
    base = dict(params)
    params.update(vars(run_ala.build_extras_parser().parse_args([])))
    assert run_ala.stored_params(params) == base and run_ala.stored_params({**params, "flex_eval": False}) == base
    assert run_ala.stored_params({**params, "flex_eval": True}) == {**base, "flex_eval": True}


def test_flex_stats_inputs_are_checked(tmp_path):
    d = tmp_path / "run"
    d.mkdir()
    (d / "modelparams.json").write_text(json.dumps({"n_cgs": 2, "det": False, "mapping": [0] * 3 + [1] * 3}))
    params, p = bm.read_params(str(d)), bm.build_parser()
    cg, top, ref, hyd = tmp_path / "cg.npz", tmp_path / "top.npz", tmp_path / "ref.npz", tmp_path / "hyd.npz"
    z, bonds = np.array([6, 1, 7, 6, 1, 8]), np.stack([np.arange(5), np.arange(1, 6)], 1)
    np.savez(cg, cg_xyz=np.zeros((3, 2, 3), np.float32))
    np.savez(top, z=z, bonds=bonds)
    np.savez(ref, xyz=np.zeros((4, 6, 3), np.float32), z=z)
    np.savez(hyd, z=np.array([1, 1, 1, 1, 6, 6]), bonds=bonds)
    base = f"-model {d} -cg {cg} -n_samples 2 -out o"
    inp = bm.read_inputs(p.parse_args(f"{base} -top {top} --flex_stats -ref {ref}".split()), params)
    assert inp["ref_xyz"].shape == (4, 6, 3) and "ref_starts" not in inp
    inp = bm.read_inputs(p.parse_args(f"{base} -top {top} --flex_stats -flex_groups bead -ref {ref}".split()), params)
    assert inp["mapping"].tolist() == [0, 0, 0, 1, 1, 1]
    with pytest.raises(SystemExit, match="--flex_stats needs a topology"):
        bm.read_inputs(p.parse_args(f"{base} --flex_stats -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="reference frames"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --flex_stats".split()), params)
    with pytest.raises(SystemExit, match="no N - CA - C' backbone"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --flex_stats -flex_groups residue -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match=r"-ref is the reference of .*--contact_stats / --flex_stats"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="options of --flex_stats"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} -flex_aligned a.npz".split()), params)
    np.savez(ref, xyz=np.zeros((4, 6, 3), np.float32), z=np.array([1, 1, 1, 1, 6, 6]))
    with pytest.raises(SystemExit, match="fewer than three heavy atoms"):
        bm.read_inputs(p.parse_args(f"{base} -top {hyd} --flex_stats -ref {ref}".split()), params)
