"""Ensemble coverage without a GPU: the restatement against closed forms, the host metrics, the C ABI's declarations
and argument checks, the command-line switches."""
import ctypes
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, backmap as bm, coverage, ensemble, run_ala
import superpose_restatement as R


# ----------------------------------------------------------------------------- the restatement against closed forms
def test_a_rotated_and_translated_copy_superposes_to_zero():
    rng = np.random.default_rng(0)
    a = rng.uniform(0, 8, (9, 3))
    b = a @ R.random_rotation(rng).T + rng.uniform(-5, 5, 3)
    G = ((a - a.mean(0)) ** 2).sum()
    assert R.rmsd2_pair(a, b) <= 64 * R.U * 2 * G / 9
    sel = [7, 0, 3, 5]
    Gs = ((a[sel] - a[sel].mean(0)) ** 2).sum()
    assert R.rmsd2_pair(a, b, sel) <= 64 * R.U * 2 * Gs / 4
    assert R.rmsd2_pair(a, rng.uniform(0, 8, (9, 3))) > 0.1          # not vacuous


def test_the_mirror_image_of_a_chiral_tetrahedron_keeps_its_hand_computed_distance():
    rng = np.random.default_rng(1)
    a = R.CHIRAL_TETRAHEDRON
    assert np.abs(a.sum(0)).max() == 0 and np.abs(a.T @ a - np.diag([8.5, 4.78125, 1.0])).max() == 0
    mirror = a * np.array([-1.0, 1.0, 1.0])
    assert abs(R.rmsd2_pair(a, mirror) - R.CHIRAL_MIRROR_RMSD2) <= 1e-14
    moved = mirror @ R.random_rotation(rng).T + rng.uniform(-3, 3, 3)  # wherever the mirror image is put
    assert abs(R.rmsd2_pair(a, moved) - R.CHIRAL_MIRROR_RMSD2) <= 1e-13
    assert R.rmsd2_pair(a, a @ R.random_rotation(rng).T) <= 1e-13


def test_a_mirrored_planar_set_superposes_and_one_atom_is_zero():
    rng = np.random.default_rng(2)
    flat = np.concatenate([rng.uniform(0, 8, (7, 2)), np.zeros((7, 1))], axis=1)
    mirrored = flat * np.array([-1.0, 1.0, 1.0])                       # a half turn about y does the same
    G = ((flat - flat.mean(0)) ** 2).sum()
    assert R.rmsd2_pair(flat, mirrored) <= 64 * R.U * 2 * G / 7
    a, b = rng.uniform(0, 8, (5, 3)), rng.uniform(0, 8, (5, 3))
    assert R.rmsd2_pair(a, b, [3]) == 0.0 and R.bound_unit(a[None], b[None], [3])[0, 0] == 0.0


def test_the_min_rule_takes_the_lowest_index_and_skips_nan():
    D = np.array([[3.0, 1.0, 1.0, np.nan], [np.nan, np.nan, np.nan, np.nan], [0.5, 2.0, 0.5, 0.25]])
    v, i = R.min_rule(D, 1)
    assert v.tolist() == [1.0, np.inf, 0.25] and i.tolist() == [1, -1, 3]
    v, i = R.min_rule(D, 0)
    assert v.tolist() == [0.5, 1.0, 0.5, 0.25] and i.tolist() == [2, 0, 2, 2]
    v, i = R.min_rule(D[:, :3], 1, skip=np.eye(3, dtype=bool))
    assert v.tolist() == [1.0, np.inf, 0.5] and i.tolist() == [1, -1, 0]
    bad = np.random.default_rng(3).uniform(0, 8, (3, 4, 3))
    bad[1, 2, 0] = np.nan
    M = R.rmsd2_matrix(bad, bad, [0, 2])
    assert np.isnan(M[1]).all() and np.isnan(M[:, 1]).all() and np.isfinite(M[[0, 2]][:, [0, 2]]).all()
    assert np.isfinite(R.rmsd2_matrix(bad, bad, [0, 1, 3])).all()      # the NaN is outside the selection


# ----------------------------------------------------------------------------- metrics
def test_metrics_from_nearest_on_hand_made_minima():
    row = np.array([0.2, 0.6, 1.0, 3.0, np.inf])
    col = np.array([0.4, 0.4, 2.5, 0.1])
    m = coverage.metrics_from_nearest(row, col, (0.5, 1.0, 2.0))
    assert set(m) == set(coverage.METRIC_KEYS) and json.loads(json.dumps(m)) == m
    assert m["thresholds"] == [0.5, 1.0, 2.0]
    assert m["cov_r"] == [0.2, 0.6, 0.6]                               # the +inf frame is never covered
    assert m["mat_r_mean"] == pytest.approx(1.2) and m["mat_r_median"] == pytest.approx(0.8) and m["unmatched_r"] == 1
    assert m["cov_p"] == [0.75, 0.75, 0.75] and m["mat_p_mean"] == pytest.approx(0.85) and m["mat_p_median"] == pytest.approx(0.4)
    assert m["unmatched_p"] == 0
    none = coverage.metrics_from_nearest([np.inf, np.inf], [], (1.0,))
    assert none["cov_r"] == [0.0] and none["mat_r_mean"] is None and none["mat_r_median"] is None and none["unmatched_r"] == 2
    assert none["cov_p"] == [None] and none["mat_p_mean"] is None


def test_select_atoms():
    z = np.array([6, 1, 1, 7, 8, 1])
    assert coverage.select_atoms(z).tolist() == [0, 3, 4] and coverage.select_atoms(z, "all").tolist() == list(range(6))
    assert coverage.select_atoms(z, [4, 1]).tolist() == [4, 1]
    with pytest.raises(ValueError):
        coverage.select_atoms(z, "backbone")
    assert set(coverage.summary_of({k: None for k in coverage.COV_STATS_KEYS})) <= set(coverage.COV_STATS_KEYS)


# ----------------------------------------------------------------------------- the C ABI
def test_k17_is_declared_and_refuses_bad_arguments_before_touching_a_device():
    names = ["cgv_superpose", "cgv_superpose_workspace_bytes", "cgv_superpose_max_structures", "cgv_superpose_max_atoms"]
    declared = _lib.header_symbols()
    lib = _lib.load()
    for name in names:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
    lim = coverage.limits()
    assert lim["structures"] >= 16384 and lim["atoms"] >= 4096
    f = ctypes.c_void_p(None)
    call = lambda sa, sb, n, m, oa=0, ob=0: lib.cgv_superpose(f, f, f, sa, sb, n, m, oa, ob, 0, f, f, f, f, f, f, 0, f)
    assert call(4, 4, 5, 0) == -1 and b"m" in lib.cgv_last_error_string()
    assert call(4, 4, 5, 6) == -1
    assert call(-1, 4, 5, 2) == -1 and call(lim["structures"] + 1, 4, 5, 2) == -1
    assert call(4, 4, lim["atoms"] + 1, 2) == -1
    assert call(4, 4, 5, 2, -1, 0) == -1 and call(4, 4, 5, 2, 0, 2 ** 31 - 2) == -1
    assert call(4, 4, 5, 2) == -1 and b"null" in lib.cgv_last_error_string()
    assert call(0, 4, 5, 2) == 0 and call(4, 0, 5, 2) == 0              # an empty set: nothing to do
    # the workspace: centroid, G and the bad flag of every structure, one (value, index) partial per row and tile of 32
    # columns and per column and tile of 32 rows
    for sa, sb in ((1, 1), (32, 32), (33, 32), (40, 53), (4096, 4096)):
        ta, tb = (sa + 31) // 32, (sb + 31) // 32
        want = 36 * (sa + sb) + 12 * (tb * sa + ta * sb)
        got = lib.cgv_superpose_workspace_bytes(sa, sb)
        assert want <= got <= want + 8 and got % 8 == 0
    assert lib.cgv_superpose_workspace_bytes(lim["structures"] + 1, 4) == 0


def test_host_wrappers_refuse_bad_selections_without_a_launch():
    a, b = np.zeros((4, 6, 3), np.float32), np.zeros((5, 6, 3), np.float32)
    for call in (coverage.rmsd_matrix, coverage.nearest):
        with pytest.raises(ValueError, match="names atom 6"):
            call(a, b, [0, 6])
        with pytest.raises(ValueError, match="names atom -1"):
            call(a, b, [-1, 2])
        with pytest.raises(ValueError, match="m = 0"):
            call(a, b, [])
        with pytest.raises(ValueError, match="mismatched n"):
            call(a, np.zeros((5, 7, 3), np.float32))
        with pytest.raises(ValueError, match=r"\[S, n, 3\]"):
            call(a[0], b)
    with pytest.raises(ValueError, match="dense matrix is limited"):
        coverage.rmsd_matrix(np.zeros((4097, 1, 3), np.float32), np.zeros((4096, 1, 3), np.float32))
    as_coverage = dict(purpose="superpose", unique=False, max_atoms=coverage.limits()["atoms"])
    assert ensemble.selection(None, 6, **as_coverage).tolist() == list(range(6)) and ensemble.selection([5, 0], 6, **as_coverage).dtype == np.int32
    with pytest.raises(ValueError, match="two reference frames"):
        coverage.compare(a[:1], b, np.full(6, 6))


# ----------------------------------------------------------------------------- command line
def test_the_switches_exist_and_leave_every_other_default():
    p = bm.build_parser()
    off = vars(p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz".split()))
    assert off["cov_stats"] is False and off["cov_thresholds"] == [0.5, 1.0, 2.0] and off["cov_atoms"] == "heavy"
    rest = {k: v for k, v in off.items() if not k.startswith("cov_")}
    assert rest == {"model": "D", "cg": "c.npz", "traj": None, "top": None, "n_samples": 4, "out": "o.npz", "frames_per_launch": 8,
                    "seed": 0, "device": "0", "pair_rmsd": False, "require_valid": None, "max_rounds": 4, "dist_stats": False,
                    "ref": None, "tica_stats": False, "tica_lag": 100, "tica_bins": 50}
    on = p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz --cov_stats -cov_thresholds 0.25 1.5 -cov_atoms all".split())
    assert on.cov_stats is True and on.cov_thresholds == [0.25, 1.5] and on.cov_atoms == "all"
    extras = vars(run_ala.build_extras_parser().parse_args([]))
    assert extras == {"dist_eval": False, "tica_eval": False, "tica_lag": 100, "cov_eval": False}
    assert vars(run_ala.build_extras_parser().parse_args(["--cov_eval"]))["cov_eval"] is True
    # the reference's flag surface does not know the switch: it stays in the extras parser
    assert not any("cov" in k for k in vars(run_ala.build_parser().parse_args("-logdir x".split())))
    got, rest = run_ala.build_extras_parser().parse_known_args("-logdir x --cov_eval -n_cgs 3".split())
    assert got.cov_eval and rest == ["-logdir", "x", "-n_cgs", "3"]


def test_an_off_switch_adds_no_key_to_modelparams():
    params = vars(run_ala.build_parser().parse_args("-logdir x".split()))
    base = dict(params)
    params.update(vars(run_ala.build_extras_parser().parse_args([])))
    assert run_ala.stored_params(params) == base
    params.update(vars(run_ala.build_extras_parser().parse_args(["--cov_eval"])))
    assert run_ala.stored_params(params) == {**base, "cov_eval": True}


def test_cov_stats_inputs_are_checked(tmp_path):
    d = tmp_path / "run"
    d.mkdir()
    (d / "modelparams.json").write_text(json.dumps({"n_cgs": 2, "det": False, "mapping": [0] * 3 + [1] * 3}))
    params, p = bm.read_params(str(d)), bm.build_parser()
    cg, top, ref, hyd = tmp_path / "cg.npz", tmp_path / "top.npz", tmp_path / "ref.npz", tmp_path / "hyd.npz"
    z, bonds = np.array([6, 1, 7, 6, 1, 8]), np.stack([np.arange(5), np.arange(1, 6)], 1)
    np.savez(cg, cg_xyz=np.zeros((3, 2, 3), np.float32))
    np.savez(top, z=z, bonds=bonds)
    np.savez(ref, xyz=np.zeros((4, 6, 3), np.float32), z=z)
    np.savez(hyd, z=np.ones(6, int), bonds=bonds)
    base = f"-model {d} -cg {cg} -n_samples 2 -out o"
    inp = bm.read_inputs(p.parse_args(f"{base} -top {top} --cov_stats -ref {ref}".split()), params)
    assert inp["ref_xyz"].shape == (4, 6, 3) and "ref_starts" not in inp
    with pytest.raises(SystemExit, match="--cov_stats needs a topology"):
        bm.read_inputs(p.parse_args(f"{base} --cov_stats -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="reference frames"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --cov_stats".split()), params)
    with pytest.raises(SystemExit, match="positive"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --cov_stats -cov_thresholds 0 1 -ref {ref}".split()), params)
    np.savez(ref, xyz=np.zeros((4, 6, 3), np.float32), z=np.ones(6, int))
    with pytest.raises(SystemExit, match="no heavy atoms"):
        bm.read_inputs(p.parse_args(f"{base} -top {hyd} --cov_stats -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="-ref is the reference"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} -ref {ref}".split()), params)
