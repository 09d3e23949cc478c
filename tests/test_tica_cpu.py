"""TICA without a GPU: the pair tables, the backbone selection, the host fit on exact population moments, the
restatement's own moments, the C ABI's declarations and argument checks, the command line's input checks."""
import ctypes
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, backmap as bm, tica
import internal_coords_restatement as IR
import tica_restatement as R


# ----------------------------------------------------------------------------- features
def test_distance_pairs_exclude_neighbours_on_atom_indices():
    sel = [9, 0, 2, 3, 7]                                   # unsorted, with index gaps
    # sorted 0 2 3 7 9; J > I + 2 on ATOM indices: (0,2) is out although the two are adjacent in sel, (7,9) is out,
    # (0,3) is in although it is two positions along sel
    assert tica.distance_pairs(sel).tolist() == [[0, 3], [0, 7], [0, 9], [2, 7], [2, 9], [3, 7], [3, 9]]
    assert tica.distance_pairs(sel, 0).tolist() == [[0, 2], [0, 3], [0, 7], [0, 9], [2, 3], [2, 7], [2, 9], [3, 7], [3, 9], [7, 9]]
    assert tica.distance_pairs(sel, 6).tolist() == [[0, 7], [0, 9], [2, 9]]
    got = tica.distance_pairs(sel)
    assert got.dtype == np.int32 and got.shape == (7, 2)
    empty = tica.distance_pairs([4, 5, 6])
    assert empty.shape == (0, 2) and empty.dtype == np.int32
    assert tica.distance_pairs([], 0).shape == (0, 2)
    assert tica.distance_pairs([3, 3, 8]).tolist() == [[3, 8]]          # an atom listed twice is one atom


def test_backbone_atoms_of_the_dipeptide_and_of_a_hydrocarbon():
    got = tica.backbone_atoms(IR.ALA_Z, IR.ALA_BONDS)
    # phi = C' N CA C and psi = N CA C N': the residue is atoms 1..3 of phi
    assert got.tolist() == sorted(IR.ALA_PHI[1:]) and got.tolist() == sorted(IR.ALA_PSI[:3])
    assert [int(IR.ALA_Z[a]) for a in IR.ALA_PHI[1:]] == [7, 6, 6]
    perm = np.random.default_rng(0).permutation(22)
    z = np.empty(22, int)
    z[perm] = IR.ALA_Z
    assert tica.backbone_atoms(z, perm[IR.ALA_BONDS]).tolist() == sorted(perm[list(IR.ALA_PHI[1:])].tolist())
    zc, bc = IR.branched_chain(30, seed=1)
    none = tica.backbone_atoms(zc, bc)
    assert none.shape == (0,) and none.dtype == np.int64


# ----------------------------------------------------------------------------- the fit on exact population moments
def _ar1_moments(d=6, lag=5, N=1000, seed=3, duplicate=False):
    """Mixed AR(1) sources: x_t = m + A s_t, s_k with coefficient phi_k and variance sigma_k^2.  Population moments:
    C0 = A diag(sigma^2) A^T, C_tau = A diag(sigma^2 phi^lag) A^T.  A = orthogonal * diag(1..3) * orthogonal: cond 3."""
    rng = np.random.default_rng(seed)
    phi = np.array([0.99, 0.95, 0.9, 0.8, 0.6, 0.3])[:d]
    var = np.array([1.0, 0.5, 2.0, 0.7, 1.5, 0.9])[:d]
    u, _ = np.linalg.qr(rng.standard_normal((d, d)))
    v, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = u @ np.diag(np.linspace(1.0, 3.0, d)) @ v
    assert np.linalg.cond(A) <= 10
    m = rng.uniform(2.0, 9.0, d)
    if duplicate:                                            # feature d is a copy of feature 0: C0 loses one direction
        A, m = np.vstack([A, A[:1]]), np.append(m, m[0])
    c0, ct = A @ np.diag(var) @ A.T, A @ np.diag(var * phi ** lag) @ A.T
    mm = np.outer(m, m)
    mom = {"sum_x": N * m, "sum_y": N * m, "cxx": N * (c0 + mm), "cyy": N * (c0 + mm), "cxy": N * (ct + mm), "n_frame_pairs": N}
    return mom, c0, ct, phi ** lag, m


def test_fit_from_moments_recovers_the_ar1_eigenvalues_to_1e_9():
    lag = 5
    mom, c0, ct, want, m = _ar1_moments(lag=lag)
    model = tica.fit_from_moments(mom, lag, dim=6)
    err_ev = np.abs(model.eigenvalues - np.sort(want)[::-1]).max()
    err_c0 = np.abs(model.W.T @ c0 @ model.W - np.eye(6)).max()
    err_ct = np.abs(model.W.T @ ct @ model.W - np.diag(model.eigenvalues)).max()
    print("eigenvalues", err_ev, "W^T C0 W - I", err_c0, "W^T Ct W - diag", err_ct)
    assert err_ev <= 1e-9 and err_c0 <= 1e-9 and err_ct <= 1e-9
    assert np.abs(model.mean - m).max() <= 1e-12 and model.rank == 6 and model.n_frame_pairs == 1000 and model.lag == lag
    np.testing.assert_allclose(model.timescales, -lag / np.log(np.sort(want)[::-1]), rtol=1e-7)
    # the sign convention: every column's entry of largest magnitude is positive
    big = np.abs(model.W).argmax(0)
    assert (model.W[big, np.arange(6)] > 0).all()
    two = tica.fit_from_moments(mom, lag)                    # dim = 2: the two slowest, the same vectors
    assert two.W.shape == (6, 2) and np.abs(two.W - model.W[:, :2]).max() <= 1e-12
    # the restatement's own algebra agrees
    mean, W, ev, rank = R.fit(mom, lag, dim=6)
    assert rank == 6 and np.abs(ev - model.eigenvalues).max() <= 1e-9 and np.abs(W - model.W).max() <= 1e-7


def test_fit_drops_exactly_one_direction_of_a_duplicated_feature():
    mom, c0, ct, want, m = _ar1_moments(duplicate=True)
    model = tica.fit_from_moments(mom, 5, dim=7)
    assert model.rank == 6 and model.W.shape == (7, 6)
    assert np.abs(model.eigenvalues - np.sort(want)[::-1]).max() <= 1e-9
    with pytest.raises(ValueError, match="no frame pairs"):
        tica.fit_from_moments({**mom, "n_frame_pairs": 0}, 5)
    with pytest.raises(ValueError, match="not finite"):
        tica.fit_from_moments({**mom, "sum_x": mom["sum_x"] * np.nan}, 5)


def test_restated_moments_do_not_depend_on_the_order_of_the_sum():
    rng = np.random.default_rng(5)
    xyz = rng.uniform(0, 6, (40, 7, 3)).astype(np.float32)
    xyz[3, 2] = xyz[3, 5]                                    # a coincident pair: distance 0
    pairs = tica.distance_pairs(np.arange(7), 0)
    f = R.features(xyz, pairs)
    assert f.dtype == np.float32 and f.shape == (40, 21) and (f[3] == 0).sum() == 1
    want = np.sqrt(((xyz[:, pairs[:, 0]].astype(np.float64) - xyz[:, pairs[:, 1]]) ** 2).sum(-1))
    assert np.abs(f - want).max() <= 4 * 2.0 ** -24 * want.max()
    lag = 3
    a, b, c = (R.moments(xyz, pairs, lag, order) for order in ("forward", "reversed", "einsum"))
    N = 37
    assert a["n_frame_pairs"] == N
    for k in tica.MOMENT_KEYS:
        assert np.abs(a[k] - b[k]).max() <= N * 2.0 ** -52 * np.abs(a[k]).max(), k
        assert np.abs(a[k] - c[k]).max() <= N * 2.0 ** -52 * np.abs(a[k]).max(), k
    assert np.array_equal(a["cxx"], a["cxx"].T) and not np.array_equal(a["cxy"], a["cxy"].T)
    assert R.moments(xyz[:3], pairs, lag)["n_frame_pairs"] == 0 and not R.moments(xyz[:3], pairs, lag)["cxx"].any()


# ----------------------------------------------------------------------------- the C ABI
def test_k16_is_declared_and_refuses_bad_arguments_before_touching_a_device():
    names = ["cgv_tica_moments", "cgv_tica_project", "cgv_tica_max_features", "cgv_tica_max_atoms", "cgv_tica_max_bins2",
             "cgv_tica_max_components", "cgv_tica_moments_splits", "cgv_tica_moments_workspace_bytes"]
    declared = _lib.header_symbols()
    lib = _lib.load()
    for name in names:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
    lim = tica.limits()
    assert lim["features"] >= 1024 and lim["atoms"] >= 4096 and lim["bins2"] >= 50 and lim["components"] == 8
    f = ctypes.c_void_p(None)
    mom = lambda T, n, d, lag: lib.cgv_tica_moments(f, f, T, n, d, lag, f, f, f, f, f, f, 0, f)
    assert mom(10, 5, lim["features"] + 1, 1) == -1 and b"max_features" in lib.cgv_last_error_string()
    assert mom(10, 5, 4, 0) == -1 and b"lag" in lib.cgv_last_error_string()
    assert mom(10, lim["atoms"] + 1, 4, 1) == -1
    assert mom(0, 5, 4, 1) == 0 and mom(3, 5, 4, 3) == 0            # no frames / T <= lag: nothing to add
    proj = lambda S, d, k, nb, lo, hi, counts: lib.cgv_tica_project(f, f, f, f, S, 5, d, k, f, 0, 0, nb, lo, hi, 0.0, 1.0,
                                                                    counts, counts, f)
    one = ctypes.c_void_p(8)                                         # a non-NULL counts pointer; never dereferenced
    assert proj(4, lim["features"] + 1, 2, 10, 0.0, 1.0, f) == -1
    assert proj(4, 4, 9, 10, 0.0, 1.0, f) == -1 and b"max_components" in lib.cgv_last_error_string()
    assert proj(4, 4, 0, 10, 0.0, 1.0, f) == -1
    assert proj(4, 4, 2, lim["bins2"] + 1, 0.0, 1.0, one) == -1 and b"max_bins2" in lib.cgv_last_error_string()
    assert proj(4, 4, 2, 10, 1.0, 1.0, one) == -1 and proj(4, 4, 2, 10, 2.0, 1.0, one) == -1
    assert proj(0, 4, 2, 10, 0.0, 1.0, f) == 0                       # no structures: nothing to do
    # the helpers: positive, monotone in the frame count and the feature count
    last = 0
    for T in (2, 100, 5000, 200000):
        s, b = lib.cgv_tica_moments_splits(T, 10, 1), lib.cgv_tica_moments_workspace_bytes(T, 10, 1)
        assert s >= 1 and b >= s * 8 * (3 * 10 * 10 + 20) and b >= last
        last = b
    assert lib.cgv_tica_moments_splits(4000, 10, 1) > 1 and lib.cgv_tica_moments_splits(1, 10, 1) == 0
    last = 0
    for d in (1, 16, 17, 33, 400, lim["features"]):
        b = lib.cgv_tica_moments_workspace_bytes(600, d, 100)
        assert b >= 8 * (3 * d * d + 2 * d) and b >= last
        last = b
    assert lib.cgv_tica_moments_workspace_bytes(600, lim["features"] + 1, 100) == 0


def test_host_wrappers_refuse_bad_tables_without_a_launch():
    with pytest.raises(ValueError, match="names atom"):
        tica._check_pairs([[0, 7]], 7)
    with pytest.raises(ValueError, match="names atom"):
        tica._check_pairs([[-1, 3]], 7)
    with pytest.raises(ValueError, match="sparser sel"):
        tica._check_pairs(tica.distance_pairs(np.arange(80), 0), 80)
    with pytest.raises(ValueError, match="empty"):
        tica._check_pairs(np.zeros((0, 2)), 7)
    assert tica._check_pairs([[0, 6]], 7).dtype == np.int32
    x = np.zeros((10, 3, 3), np.float32)
    assert [s.shape[0] for s in tica.split_segments(x, [0, 4, 9])] == [4, 5, 1] and len(tica.split_segments(x)) == 1
    for bad in ([1, 4], [0, 4, 4], [0, 10], []):
        with pytest.raises(ValueError):
            tica.split_segments(x, bad)


# ----------------------------------------------------------------------------- model file, command line
def test_model_round_trips_through_npz(tmp_path):
    mom, *_ = _ar1_moments()
    pairs = tica.distance_pairs(np.arange(4), 0)
    model = tica.fit_from_moments(mom, 5, dim=3, pairs=pairs)
    model.save(str(tmp_path / "m.npz"))
    back = tica.TicaModel.load(str(tmp_path / "m.npz"))
    for k in ("pairs", "mean", "W", "eigenvalues", "timescales"):
        assert np.array_equal(getattr(back, k), getattr(model, k)) and getattr(back, k).dtype == getattr(model, k).dtype
    assert (back.lag, back.rank, back.n_frame_pairs) == (model.lag, model.rank, model.n_frame_pairs) == (5, 6, 1000)


def test_tica_stats_inputs_are_checked(tmp_path):
    d = tmp_path / "run"
    d.mkdir()
    n = len(IR.ALA_Z)
    (d / "modelparams.json").write_text(json.dumps({"n_cgs": 2, "det": False, "mapping": [0] * 11 + [1] * 11}))
    params, p = bm.read_params(str(d)), bm.build_parser()
    a = p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz".split())
    assert a.tica_stats is False and a.tica_lag == 100 and a.tica_bins == 50
    cg, top, ref, hc = tmp_path / "cg.npz", tmp_path / "top.npz", tmp_path / "ref.npz", tmp_path / "hc.npz"
    np.savez(cg, cg_xyz=np.zeros((3, 2, 3), np.float32))
    np.savez(top, z=IR.ALA_Z, bonds=IR.ALA_BONDS)
    np.savez(ref, xyz=np.zeros((12, n, 3), np.float32), z=IR.ALA_Z, bonds=IR.ALA_BONDS, traj_starts=np.array([0, 7]))
    base = f"-model {d} -cg {cg} -n_samples 2 -out o"
    inp = bm.read_inputs(p.parse_args(f"{base} -top {top} --tica_stats -tica_lag 10 -ref {ref}".split()), params)   # -ref alone with --tica_stats
    assert inp["ref_xyz"].shape == (12, n, 3) and inp["ref_starts"].tolist() == [0, 7]
    with pytest.raises(SystemExit, match="topology"):
        bm.read_inputs(p.parse_args(f"{base} --tica_stats -tica_lag 10 -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match=r"lag \+ 2"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --tica_stats -tica_lag 11 -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match=r"lag \+ 2"):                 # the default lag of 100
        bm.read_inputs(p.parse_args(f"{base} -top {top} --tica_stats -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="reference frames"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --tica_stats -tica_lag 10".split()), params)
    zc = np.full(n, 6)
    np.savez(hc, z=zc, bonds=np.stack([np.arange(n - 1), np.arange(1, n)], 1))
    np.savez(ref, xyz=np.zeros((12, n, 3), np.float32), z=zc)
    with pytest.raises(SystemExit, match="peptide backbone"):
        bm.read_inputs(p.parse_args(f"{base} -top {hc} --tica_stats -tica_lag 5 -ref {ref}".split()), params)
