"""Essential dynamics, the part that needs no device: the fit from moments against numpy.cov + eigh, the sign rule, the
model file, the host statistics against their definitions (pca_restatement.py), the comparison on planted moments, every
refusal that comes before a launch, and that header, prototype table and library agree on the new names."""
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, pca
import dssp_restatement as DR
import pca_restatement as R


def _moments_of(F):
    """The sums ``pca.moments`` returns, of a feature matrix ``F [S,d]``."""
    return {"sum": F.sum(0), "cov": F.T @ F, "n_good": F.shape[0], "bad": np.zeros(F.shape[0], dtype=bool)}


def _features(seed, S=200, m=3, scales=None, mean=0.5):
    rng = np.random.default_rng(seed)
    d = 3 * m
    scales = np.linspace(0.3, 1.8, d) if scales is None else np.asarray(scales)
    q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    return (rng.standard_normal((S, d)) * scales) @ q.T + mean * rng.standard_normal(d)


# ----------------------------------------------------------------------------- the fit
def test_fit_from_moments_is_numpy_cov_divided_by_n_and_eigh():
    F = _features(1)
    model = pca.fit_from_moments(_moments_of(F), np.arange(3), np.zeros((3, 3)), dim=4)
    C = np.cov(F.T, bias=True)
    w, v = np.linalg.eigh(C)
    np.testing.assert_allclose(model.eigenvalues, w[::-1], rtol=1e-12)
    np.testing.assert_allclose(model.mu, F.mean(0), rtol=1e-12)
    np.testing.assert_allclose(model.total_variance, np.trace(C), rtol=1e-12)
    assert model.W.shape == (9, 4) and model.eigenvalues.shape == (9,) and model.n_good == 200
    for i in range(4):                                            # the same direction, whatever eigh's sign
        np.testing.assert_allclose(abs(model.W[:, i] @ v[:, ::-1][:, i]), 1.0, rtol=1e-12)
    np.testing.assert_allclose(model.W.T @ model.W, np.eye(4), atol=1e-12)
    mu, C2 = pca.covariance_of(_moments_of(F))
    np.testing.assert_allclose(C2, C, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(R.covariance(_moments_of(F))[1], C, rtol=1e-12, atol=1e-14)


def test_the_sign_rule_and_the_clamp():
    model = pca.fit_from_moments(_moments_of(_features(2)), np.arange(3), np.zeros((3, 3)), dim=9)
    big = np.abs(model.W).argmax(0)
    assert (model.W[big, np.arange(9)] > 0).all()
    flipped = pca.fit_from_moments(_moments_of(-_features(2)), np.arange(3), np.zeros((3, 3)), dim=9)
    np.testing.assert_allclose(flipped.W, model.W, atol=1e-9)    # f -> -f has the same covariance: the same signed modes
    # two identical structures: C is zero up to rounding, nothing negative comes out
    flat = pca.fit_from_moments(_moments_of(np.tile(_features(3)[:1], (2, 1))), np.arange(3), np.zeros((3, 3)), dim=2)
    assert (flat.eigenvalues >= 0).all() and flat.eigenvalues.max() < 1e-12
    lam, V = pca.modes_of(np.diag([1.0, -1e-18, 3.0]))
    assert lam.tolist() == [3.0, 1.0, 0.0] and np.allclose(np.abs(V), np.eye(3)[:, [2, 0, 1]])


def test_fit_from_moments_refuses_what_has_no_covariance():
    F = _features(4)
    ok = _moments_of(F)
    for bad, match in ((dict(ok, n_good=1), "at least two"), (dict(ok, n_good=0), "at least two"),
                       (dict(ok, sum=np.where(np.arange(9) == 2, np.nan, ok["sum"])), "not finite"),
                       (dict(ok, cov=ok["cov"] * np.inf), "not finite"), (dict(ok, cov=ok["cov"][:8, :8]), "do not fit")):
        with pytest.raises(ValueError, match=match):
            pca.fit_from_moments(bad, np.arange(3), np.zeros((3, 3)))
    with pytest.raises(ValueError, match="dim must be in 1..9"):
        pca.fit_from_moments(ok, np.arange(3), np.zeros((3, 3)), dim=10)
    with pytest.raises(ValueError, match="dim must be in 1..9"):
        pca.fit_from_moments(ok, np.arange(3), np.zeros((3, 3)), dim=0)
    with pytest.raises(ValueError, match="lists 4 atoms"):
        pca.fit_from_moments(ok, np.arange(4), np.zeros((4, 3)))


def test_the_model_file_round_trip(tmp_path):
    model = pca.fit_from_moments(_moments_of(_features(5)), np.array([4, 0, 2]), np.arange(15.0).reshape(5, 3), dim=3)
    model.save(str(tmp_path / "m.npz"))
    back = pca.PcaModel.load(str(tmp_path / "m.npz"))
    for name in ("sel", "target", "mu", "eigenvalues", "W"):
        a, b = getattr(model, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert back.total_variance == model.total_variance and back.n_good == model.n_good == 200
    assert back.sel.dtype == np.int32 and back.sel.tolist() == [4, 0, 2]
    with np.load(tmp_path / "m.npz", allow_pickle=False) as f:    # no pickle inside
        assert sorted(f.files) == ["W", "eigenvalues", "mu", "n_good", "sel", "target", "total_variance"]


# ----------------------------------------------------------------------------- host statistics
def test_rmsip_of_equal_rotated_and_orthogonal_spans():
    q = np.linalg.qr(np.random.default_rng(6).standard_normal((12, 12)))[0]
    A, B = q[:, :3], q[:, 3:6]
    assert pca.rmsip(A, A) == pytest.approx(1.0, abs=1e-14)
    g = np.linalg.qr(np.random.default_rng(7).standard_normal((3, 3)))[0]
    assert pca.rmsip(A, A @ g) == pytest.approx(1.0, abs=1e-14)   # another basis of the same span
    assert pca.rmsip(A, B) == pytest.approx(0.0, abs=1e-14)
    mixed = np.column_stack([q[:, 0], q[:, 3], q[:, 4]])
    assert pca.rmsip(A, mixed) == pytest.approx(np.sqrt(1.0 / 3.0), abs=1e-14)
    assert pca.rmsip(A, mixed) == pytest.approx(R.rmsip(A, mixed), abs=1e-14)
    with pytest.raises(ValueError, match="same features"):
        pca.rmsip(A, B[:5])


def test_covariance_overlap_identical_scaled_symmetric():
    Ca = np.cov(_features(8).T, bias=True)
    Cb = np.cov(_features(9).T, bias=True)
    (la, Va), (lb, Vb) = pca.modes_of(Ca), pca.modes_of(Cb)
    assert pca.covariance_overlap(la, Va, la, Va) == pytest.approx(1.0, abs=1e-7)
    scaled = pca.covariance_overlap(la, Va, 4.0 * la, Va)
    # sqrt(C) and 2 sqrt(C): |difference|_F^2 = tr C, over tr C + 4 tr C
    assert scaled == pytest.approx(1.0 - np.sqrt(1.0 / 5.0), abs=1e-12) and scaled < 1.0
    ab, ba = pca.covariance_overlap(la, Va, lb, Vb), pca.covariance_overlap(lb, Vb, la, Va)
    assert ab == pytest.approx(ba, abs=1e-13) and 0.0 <= ab < 1.0
    assert ab == pytest.approx(R.covariance_overlap(la, Va, lb, Vb), abs=1e-12)
    # against the matrix form: d^2 = |sqrt(A) - sqrt(B)|_F^2
    root = lambda l, V: (V * np.sqrt(l)) @ V.T
    dist = np.linalg.norm(root(la, Va) - root(lb, Vb))
    assert ab == pytest.approx(1.0 - dist / np.sqrt(la.sum() + lb.sum()), abs=1e-10)
    assert pca.covariance_overlap(np.zeros(9), Va, np.zeros(9), Vb) is None


def test_dccm_diagonal_opposite_atoms_and_zero_rows():
    rng = np.random.default_rng(10)
    S = 500
    a = rng.standard_normal((S, 3))
    F = np.concatenate([a, -2.0 * a, rng.standard_normal((S, 3)), np.zeros((S, 3))], axis=1)   # atom 1 moves against atom 0
    C = np.cov(F.T, bias=True)
    D = pca.dccm(C)
    assert D.shape == (4, 4) and np.allclose(np.diag(D)[:3], 1.0, atol=1e-14)
    assert D[0, 1] == pytest.approx(-1.0, abs=1e-14) and abs(D[0, 2]) < 0.2
    assert (D[3] == 0).all() and (D[:, 3] == 0).all()             # an atom that does not move
    np.testing.assert_allclose(D, R.dccm(C), atol=1e-14)
    np.testing.assert_allclose(D, D.T, atol=1e-15)
    with pytest.raises(ValueError, match=r"\[3m, 3m\]"):
        pca.dccm(np.zeros((4, 4)))


def test_variance_in_modes():
    F = _features(11)
    model = pca.fit_from_moments(_moments_of(F), np.arange(3), np.zeros((3, 3)), dim=3)
    C = np.cov(F.T, bias=True)
    np.testing.assert_allclose(pca.variance_in_modes(model, C), 1.0, rtol=1e-12)
    np.testing.assert_allclose(pca.variance_in_modes(model, 0.25 * C), 0.25, rtol=1e-12)


# ----------------------------------------------------------------------------- the comparison on planted moments
def _planted(seed, S, amplitude, other=False):
    """Features of m = 4 atoms moving along two planted directions (the first two axes, or axes 2 and 3) plus noise."""
    rng = np.random.default_rng(seed)
    F = 0.05 * rng.standard_normal((S, 12))
    F[:, 2 if other else 0] += amplitude * rng.standard_normal(S)
    F[:, 3 if other else 1] += 0.5 * amplitude * rng.standard_normal(S)
    return F


def test_compare_from_moments_on_planted_moments_and_json():
    ref, same, half, other = _planted(1, 4000, 1.0), _planted(2, 3000, 1.0), _planted(3, 3000, 0.5), _planted(4, 3000, 1.0, other=True)
    sel = np.array([5, 1, 7, 3])

    def run(gen, pc_map=None):
        moms = {"ref": _moments_of(ref), "gen": _moments_of(gen), "even": _moments_of(ref[0::2]), "odd": _moments_of(ref[1::2])}
        moms["gen"]["bad"] = np.array([False] * (gen.shape[0] - 1) + [True])
        return pca.compare_from_moments(moms, sel, np.zeros((8, 3)), dim=2, pc_map=pc_map, params={"n_bins": 4})
    maps = {"range": [(-3.0, 3.0), (-2.0, 2.0)], "even": np.eye(4, dtype=np.int64) * 5, "odd": np.eye(4, dtype=np.int64) * 5,
            "gen": np.ones((4, 4), dtype=np.int64)}
    good = run(same, maps)
    assert tuple(good) == pca.PCA_STATS_KEYS
    assert json.loads(json.dumps(good)) == good                   # plain lists, floats and None
    assert (good["n_ref"], good["n_gen"], good["n_bad_ref"], good["n_bad_gen"]) == (4000, 3000, 0, 1)
    assert good["params"] == {"n_bins": 4, "atoms": [5, 1, 7, 3], "dim": 2}
    assert good["rmsip"] > 0.999 and good["covariance_overlap"] > 0.95 and 0.9 < good["total_variance_ratio"] < 1.1
    assert all(0.9 < v < 1.1 for v in good["variance_in_ref_modes"]) and good["dccm_rmse"] < 0.05
    assert good["eigenvalues_ref"] == pytest.approx([1.0, 0.25], rel=0.1) and sum(good["explained_ref"]) > 0.95
    assert good["pc_map"]["range"] == [[-3.0, 3.0], [-2.0, 2.0]] and good["pc_map"]["floor"] == 0.0 and 0 < good["pc_map"]["jsd"] < 1
    assert set(good["floor"]) == {"rmsip", "covariance_overlap", "total_variance_ratio", "dccm_rmse"} and good["floor"]["rmsip"] > 0.999
    assert len(good["top_pairs"]) == 6 and {"i", "j", "dccm_ref", "dccm_gen"} == set(good["top_pairs"][0])   # m = 4: six pairs
    assert all(p["i"] in sel and p["j"] in sel for p in good["top_pairs"])
    weak = run(half)
    assert weak["rmsip"] > 0.99 and 0.2 < weak["total_variance_ratio"] < 0.3 and all(v < 0.3 for v in weak["variance_in_ref_modes"])
    assert weak["pc_map"] is None
    wrong = run(other)
    assert wrong["rmsip"] < 0.1 and wrong["covariance_overlap"] < 0.5 and wrong["variance_in_ref_modes"][0] < 0.01
    short = pca.summary_of(good)
    assert json.loads(json.dumps(short)) == short and short["pc_map"] == {"jsd": good["pc_map"]["jsd"], "floor": 0.0}
    assert short["dim"] == 2 and "top_pairs" not in short and pca.summary_of(weak)["pc_map"] is None
    with pytest.raises(ValueError, match="dim must be in 1..12"):
        pca.compare_from_moments({k: _moments_of(ref) for k in ("ref", "gen", "even", "odd")}, sel, np.zeros((8, 3)), dim=13)


# ----------------------------------------------------------------------------- refusals before any launch
def test_every_value_error_comes_before_a_device_is_touched():
    lim = pca.limits()
    assert lim["components"] == 8 and lim["features"] >= 1536 and lim["bins2"] >= 50
    z, bonds = DR.peptide(3, cap=True)
    n = len(z)
    xyz = np.zeros((4, n, 3), np.float32)
    with pytest.raises(ValueError, match="a rotation needs at least 3"):
        pca.fit(xyz, sel=[0, 1])
    with pytest.raises(ValueError, match="names an atom twice"):
        pca.fit(xyz, sel=[0, 1, 1])
    with pytest.raises(ValueError, match=f"names atom {n}"):
        pca.fit(xyz, sel=[0, 1, n])
    with pytest.raises(ValueError, match="dim must be in 1..8"):
        pca.fit(xyz, dim=9)
    with pytest.raises(ValueError, match="dim must be in 1..8"):
        pca.fit(xyz, dim=0)
    with pytest.raises(ValueError, match="dim must be in 1..8"):                # three atoms are nine features: 8 binds, not d
        pca.fit(xyz, sel=[0, 1, 2], dim=9)
    m_over = lim["features"] // 3 + 1
    with pytest.raises(ValueError, match=f"{3 * m_over} features .*-pca_atoms backbone"):
        pca.fit(np.zeros((2, m_over, 3), np.float32))
    with pytest.raises(ValueError, match=r"\[S, n, 3\]"):
        pca.fit(np.zeros((4, n), np.float32))
    with pytest.raises(ValueError, match="at least two reference frames"):
        pca.compare(xyz[:1], xyz, z, bonds)
    with pytest.raises(ValueError, match="z lists"):
        pca.compare(xyz, xyz[:, :n - 1], z, bonds)
    with pytest.raises(ValueError, match="'heavy', 'all', 'backbone'"):
        pca.compare(xyz, xyz, z, bonds, atoms="sidechain")
    with pytest.raises(ValueError, match="no peptide backbone"):
        pca.compare(xyz, xyz, np.full(n, 6), bonds, atoms="backbone")
    with pytest.raises(ValueError, match="dim must be in"):
        pca.compare(xyz, xyz, z, bonds, dim=9)
    with pytest.raises(ValueError, match="n_bins must be in"):
        pca.compare(xyz, xyz, z, bonds, n_bins=lim["bins2"] + 1)
    with pytest.raises(ValueError, match="a rotation needs at least 3"):
        pca.compare(xyz, xyz, z, bonds, atoms=[0, 1])
    assert pca.atoms_of(z, bonds, "backbone").shape[0] == 9 and (z[pca.atoms_of(z, bonds, "heavy")] != 1).all()


def _files(tmp_path):
    z, bonds = DR.peptide(3, cap=True)
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "ref.npz", xyz=rng.normal(0, 2, (4, len(z), 3)).astype(np.float32), z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=rng.normal(0, 2, (2, 3, len(z), 3)).astype(np.float32))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}", z, bonds


def test_the_parser_and_read_inputs(tmp_path):
    base, z, bonds = _files(tmp_path)
    args = pca.parser().parse_args(base.split())
    assert (args.pca_atoms, args.pca_dim, args.pca_bins, args.model, args.out, args.top, args.device) == \
        ("heavy", 8, 50, None, "pca_stats.json", None, "cuda")
    inp = pca.read_inputs(args)
    assert inp["ref_xyz"].shape == (4, len(z), 3) and inp["gen_xyz"].shape == (6, len(z), 3) and inp["z"].tolist() == z.tolist()
    args = pca.parser().parse_args((base + " -pca_atoms backbone -pca_dim 3 -pca_bins 20 -model m.npz -out x.json").split())
    assert (args.pca_atoms, args.pca_dim, args.pca_bins, args.model, args.out) == ("backbone", 3, 20, "m.npz", "x.json")
    pca.read_inputs(args)


def test_the_command_line_refuses_before_any_launch(tmp_path):
    base, z, bonds = _files(tmp_path)

    def refused(extra, match, line=base):
        with pytest.raises(SystemExit, match=match):
            pca.read_inputs(pca.parser().parse_args((line + " " + extra).split()))
    refused(f"-top {tmp_path / 'nothing.npz'}", "no such file")
    refused("", "no such file", line=f"-gen {tmp_path / 'nothing.npz'} -ref {tmp_path / 'ref.npz'}")
    np.savez(tmp_path / "bare.npz", xyz=np.zeros((4, len(z), 3), np.float32))
    refused("", "z / bonds", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'bare.npz'}")
    np.savez(tmp_path / "nokey.npz", z=z)
    refused(f"-top {tmp_path / 'nokey.npz'}", "missing")
    np.savez(tmp_path / "short.npz", xyz=np.zeros((1, len(z), 3), np.float32), z=z, bonds=bonds)
    refused("", "at least two", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'short.npz'}")
    refused("-pca_atoms sidechain", "-pca_atoms must be heavy, all or backbone")
    refused("-pca_dim 9", "dim must be in 1..8")
    refused("-pca_dim 0", "dim must be in 1..8")
    refused(f"-pca_bins {pca.limits()['bins2'] + 1}", "-pca_bins must be in")
    np.savez(tmp_path / "carbon.npz", z=np.full(len(z), 6), bonds=bonds)
    refused(f"-top {tmp_path / 'carbon.npz'} -pca_atoms backbone", "no peptide backbone")
    # a selection past the feature limit names the way out
    big = pca.limits()["features"] // 3 + 1
    np.savez(tmp_path / "big.npz", xyz=np.zeros((2, big, 3), np.float32), z=np.full(big, 6), bonds=np.zeros((0, 2), np.int64))
    refused("", "-pca_atoms backbone", line=f"-gen {tmp_path / 'big.npz'} -ref {tmp_path / 'big.npz'}")
    with pytest.raises(SystemExit):
        pca.parser().parse_args(["-gen", "a.npz"])                             # -ref is required


# ----------------------------------------------------------------------------- library
NAMES = {"cgv_pca_max_features", "cgv_pca_max_atoms", "cgv_pca_max_structures", "cgv_pca_max_components", "cgv_pca_max_bins2",
         "cgv_pca_moments_splits", "cgv_pca_moments_workspace_bytes", "cgv_pca_moments", "cgv_pca_project"}


def test_the_library_declares_binds_and_exports_the_pca_kernel():
    assert NAMES <= set(_lib.header_symbols()) and NAMES <= set(_lib.PROTOTYPES)
    assert {n for n in _lib.header_symbols() if n.startswith("cgv_pca_")} == NAMES
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    lim = pca.limits()
    assert lim["features"] >= 3 * 512 and lim["components"] == 8 and lim["structures"] >= 4096 and lim["atoms"] >= 4096


def test_the_split_rule_and_the_workspace():
    lib, lim = _lib.load(), pca.limits()
    assert lib.cgv_pca_moments_splits(0, 30) == 0 and lib.cgv_pca_moments_splits(100, 0) == 0
    assert lib.cgv_pca_moments_splits(1, 3) == 1 and lib.cgv_pca_moments_splits(256, 3) == 1 and lib.cgv_pca_moments_splits(257, 3) == 2
    # one tile pair: the rule allows 256 ranges, ceil(100000 / 256) = 391 structures each, whole stages make that 400
    assert lib.cgv_pca_moments_splits(100000, 3) == 250
    assert lib.cgv_pca_moments_splits(4096, 1536) == 1                         # 1176 tile pairs fill the device alone
    assert lib.cgv_pca_moments_splits(100, lim["features"] + 1) == 0 and lib.cgv_pca_moments_workspace_bytes(100, lim["features"] + 1) == 0
    for S, d in ((1, 3), (257, 33), (100000, 231), (4096, 1536), (lim["structures"], lim["features"])):
        dp = (d + 31) // 32 * 32
        assert lib.cgv_pca_moments_workspace_bytes(S, d) == lib.cgv_pca_moments_splits(S, d) * (dp * dp + dp + 1) * 8
    assert lib.cgv_pca_moments_workspace_bytes(lim["structures"], lim["features"]) <= 1 << 26


def test_the_c_entries_refuse_past_a_limit_with_their_reason():
    lib, lim = _lib.load(), pca.limits()

    def refused(reason, S=1, n=10, m=4):
        rc = lib.cgv_pca_moments(None, None, None, None, S, n, m, None, None, None, None, 0, None)
        assert rc == -1 and reason in lib.cgv_last_error_string(), lib.cgv_last_error_string()
    refused(b"cgv_pca_max_features", m=lim["features"] // 3 + 1)
    refused(b"cgv_pca_max_structures", S=lim["structures"] + 1)
    refused(b"cgv_pca_max_atoms", n=lim["atoms"] + 1)
    refused(b"null pointer")
    assert lib.cgv_pca_moments(None, None, None, None, 0, 10, 4, None, None, None, None, 0, None) == 0       # nothing to do

    def project(reason, S=1, m=4, k=2, nb=0):
        rc = lib.cgv_pca_project(None, None, None, None, None, None, S, 10, m, k, None, 0, 1, nb, 0.0, 1.0, 0.0, 1.0, None, None, None)
        assert rc == -1 and reason in lib.cgv_last_error_string(), lib.cgv_last_error_string()
    project(b"cgv_pca_max_components", k=lim["components"] + 1)
    project(b"cgv_pca_max_components", k=0)
    project(b"cgv_pca_max_features", m=lim["features"] // 3 + 1)
    project(b"cgv_pca_max_structures", S=lim["structures"] + 1)
    assert lib.cgv_pca_project(None, None, None, None, None, None, 0, 10, 4, 2, None, 0, 1, 0, 0.0, 1.0, 0.0, 1.0, None, None, None) == 0


# ----------------------------------------------------------------------------- the restatement against itself
def test_the_restatement_features_moments_projection_and_bins():
    rng = np.random.default_rng(12)
    y = rng.uniform(-8, 8, (9, 6, 3)).astype(np.float32)
    sel, centre = np.array([4, 0, 5]), rng.uniform(-8, 8, (6, 3))
    f = R.features(y, sel, centre)
    assert f.shape == (9, 9) and f[2, 3 * 1 + 2] == np.float64(y[2, 0, 2]) - centre[0, 2]
    bad = np.array([0, 0, 1, 0, 0, 0, 0, 0, 1])
    mom = R.moments(y, sel, centre, bad)
    keep = f[bad == 0]
    np.testing.assert_allclose(mom["cov"], keep.T @ keep, rtol=1e-13)
    np.testing.assert_allclose(mom["sum"], keep.sum(0), rtol=1e-13)
    assert mom["n_good"] == 7 and (mom["abs_cov"] >= np.abs(mom["cov"])).all()
    W = rng.standard_normal((9, 2))
    proj, mag = R.project(y, sel, centre, np.full(9, 0.25), W, bad)
    np.testing.assert_allclose(proj[bad == 0], (keep - 0.25) @ W, rtol=1e-12, atol=1e-13)
    assert np.isnan(proj[bad == 1]).all() and (mag[bad == 0] >= np.abs(proj[bad == 0])).all()
    assert R.bin_of(np.array([0.0, 0.999, 1.0, -1e-9, np.nan, 0.5]), 0.0, 1.0, 4).tolist() == [0, 3, -1, -1, -1, 2]
    counts, outside = R.hist2(np.array([0.1, 0.6, 2.0, np.nan]), np.array([0.9, 0.1, 0.5, 0.5]), (0, 1), (0, 1), 2)
    assert counts.tolist() == [[0, 1], [1, 0]] and outside == 2
    assert R.edge_distance(np.array([0.26, 0.5]), 0.0, 1.0, 4) == pytest.approx([0.01, 0.0])
