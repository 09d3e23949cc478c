"""TICA on the device: K16 (csrc/tica.hip) against the numpy restatement -- feature bits, moments within the bound of a
reordered fp64 sum, projections, histograms count for count -- the host chunking, an end-to-end fit of a synthetic slow
process, and the backmap command line."""
import json

import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd import _lib, backmap as bm, tica
import internal_coords_restatement as IR
import tica_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -52


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _totals(d):
    return {k: torch.zeros((d,) if k.startswith("sum") else (d, d), dtype=torch.float64, device=DEV) for k in tica.MOMENT_KEYS}


def _frames(T, n, seed, box=8.0):
    return np.random.default_rng(seed).uniform(0, box, (T, n, 3)).astype(np.float32)


def _pairs(n, d, seed=0):
    """``d`` distinct pairs of ``n`` atoms (all pairs in order when ``d`` is their number)."""
    allp = tica.distance_pairs(np.arange(n), 0)
    assert d <= len(allp)
    return allp if d == len(allp) else allp[np.sort(np.random.default_rng(seed).permutation(len(allp))[:d])]


def _check_moments(got, want, N, what):
    """|delta| <= N 2^-52 |value| element-wise: every term is an exact product of non-negative fp32-valued doubles, only
    the order of the N additions differs (relative 2^-53 each; the bound carries a factor 2)."""
    worst = 0.0
    for k in tica.MOMENT_KEYS:
        g, w = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy(), want[k]
        assert g.shape == w.shape
        excess = np.abs(g - w) - N * U * np.abs(w)
        worst = max(worst, float((np.abs(g - w) / np.maximum(np.abs(w), 1e-300)).max()) if w.size else 0.0)
        assert (excess <= 0).all(), (what, k, float(excess.max()))
    print(what, "N", N, "max relative difference", worst, "bound", N * U)


# ----------------------------------------------------------------------------- feature bits
def test_features_through_one_hot_projection_are_the_restatements_bits():
    n, S = 7, 5
    xyz = _frames(S, n, 1, box=5.0)
    xyz[2, 4] = xyz[2, 1]                                   # a coincident pair of atoms
    pairs = _pairs(n, 21)
    want = R.features(xyz, pairs)
    assert want.dtype == np.float32 and (want[2] == 0).sum() == 1
    x, p, mean = _dev(xyz, torch.float32), _dev(pairs, torch.int32), torch.zeros(21, dtype=torch.float64, device=DEV)
    for first in (0, 8, 16):
        cols = list(range(first, min(first + 8, 21)))
        W = np.zeros((21, len(cols)))
        W[cols, np.arange(len(cols))] = 1.0
        ics = torch.full((S, len(cols)), -1.0, dtype=torch.float64, device=DEV)
        tica.project_launch(x, p, mean, _dev(W, torch.float64), ics)
        got = ics.cpu().numpy()
        assert np.array_equal(got, want[:, cols].astype(np.float64)), (first, np.abs(got - want[:, cols]).max())


# ----------------------------------------------------------------------------- moments
MOMENT_CASES = [(1, 2, 1), (10, 4, 1), (17, 8, 3), (33, 70, 3), (10, 6, 3), (33, 68, 1)]     # (d, T, lag): N = 1, 3, 5, 67, 3, 67


@pytest.mark.parametrize("d,T,lag", MOMENT_CASES)
def test_moments_equal_the_restatement_within_a_reordered_sum(d, T, lag):
    n = 9
    xyz, pairs = _frames(T, n, 10 * d + T), _pairs(n, d, seed=d)
    tot = _totals(d)
    assert tica.moments_launch(_dev(xyz, torch.float32), _dev(pairs, torch.int32), lag, tot) == T - lag
    want = R.moments(xyz, pairs, lag)
    _check_moments(tot, want, T - lag, f"d {d} T {T} lag {lag}")
    for k in ("cxx", "cyy"):
        assert torch.equal(tot[k], tot[k].T)                 # exactly symmetric
    assert want["cxx"].min() > 0                             # not vacuous


def test_a_segment_no_longer_than_the_lag_adds_nothing():
    xyz, pairs = _frames(5, 9, 2), _pairs(9, 10)
    for lag in (5, 9):
        tot = _totals(10)
        assert tica.moments_launch(_dev(xyz, torch.float32), _dev(pairs, torch.int32), lag, tot) == 0
        assert not any(bool(t.any()) for t in tot.values())


def test_moments_over_several_frame_ranges_add_and_repeat_bit_for_bit():
    lib = _lib.load()
    n, d, lag = 5, 10, 3
    T = 4000
    splits = int(lib.cgv_tica_moments_splits(T, d, lag))
    assert splits > 1                                        # the second launch sums more than one range
    xyz, pairs = _frames(T, n, 3), _pairs(n, d)
    x, p = _dev(xyz, torch.float32), _dev(pairs, torch.int32)
    a, b = _totals(d), _totals(d)
    tica.moments_launch(x, p, lag, a)
    tica.moments_launch(x, p, lag, b)
    for k in tica.MOMENT_KEYS:
        assert torch.equal(a[k], b[k]), k                    # the same bits on every run
    want = R.moments(xyz, pairs, lag, "einsum")
    _check_moments(a, want, T - lag, f"{splits} ranges")
    tica.moments_launch(x, p, lag, b)                        # a second call ADDS
    for k in tica.MOMENT_KEYS:
        assert torch.equal(b[k], a[k] + a[k]), k


def test_moments_at_chignolin_size():
    n, T, lag = 166, 600, 100
    sel = np.sort(np.random.default_rng(0).permutation(n)[:30])
    pairs = tica.distance_pairs(sel, 2)
    d = len(pairs)
    assert 380 <= d <= 435
    xyz = _frames(T, n, 4, box=14.0)
    tot = _totals(d)
    tica.moments_launch(_dev(xyz, torch.float32), _dev(pairs, torch.int32), lag, tot)
    _check_moments(tot, R.moments(xyz, pairs, lag, "einsum"), T - lag, f"chignolin-like d {d}")
    assert torch.equal(tot["cxx"], tot["cxx"].T) and torch.equal(tot["cyy"], tot["cyy"].T)


# ----------------------------------------------------------------------------- moments(): chunks and segments
def test_chunked_moments_count_every_frame_pair_once():
    T, lag, n = 50, 10, 6
    xyz, pairs = _frames(T, n, 7), _pairs(n, 15)
    want = R.moments(xyz, pairs, lag)
    for M in (7, 25, 50):                                    # chunks shorter and longer than the lag, and one chunk
        got = tica.moments([xyz], pairs, lag, frames_per_launch=M, device=DEV)
        assert got["n_frame_pairs"] == T - lag
        _check_moments(got, want, T - lag, f"frames_per_launch {M}")


def test_frame_pairs_do_not_cross_a_segment_boundary():
    lag, n = 4, 6
    a, b, c = _frames(30, n, 8), _frames(17, n, 9), _frames(3, n, 10)          # c is shorter than the lag: no pairs
    pairs = _pairs(n, 15)
    got = tica.moments([a, torch.from_numpy(b), c], pairs, lag, frames_per_launch=11, device=DEV)
    want = R.add(R.moments(a, pairs, lag), R.moments(b, pairs, lag))
    assert got["n_frame_pairs"] == 26 + 13 == want["n_frame_pairs"]
    _check_moments(got, want, 39, "two segments")
    joined = R.moments(np.concatenate([a, b]), pairs, lag)
    assert np.abs(joined["cxy"] - want["cxy"]).max() > 1e-6 * np.abs(want["cxy"]).max()   # the boundary pairs would show


def test_a_pair_table_with_an_atom_outside_the_frame_is_refused_before_any_launch():
    xyz = _frames(20, 6, 11)
    with pytest.raises(ValueError, match="names atom 6"):
        tica.moments([xyz], [[0, 3], [2, 6]], 2, device=DEV)
    model = tica.TicaModel(np.array([[0, 6]], np.int32), 2, np.zeros(1), np.ones((1, 1)), np.ones(1), np.ones(1), 1, 1)
    with pytest.raises(ValueError, match="names atom 6"):
        tica.project(xyz, model, device=DEV)
    with pytest.raises(ValueError, match="sparser sel"):
        tica.moments([_frames(4, 80, 12)], tica.distance_pairs(np.arange(80), 0), 2, device=DEV)


# ----------------------------------------------------------------------------- projection
@pytest.mark.parametrize("k,S", [(1, 1), (2, 1000), (8, 1000), (8, 1), (1, 1000), (2, 1)])
def test_projection_and_its_histogram(k, S):
    _projection_and_its_histogram(k, S, n=11, d=50)


@pytest.mark.parametrize("k", [1, 8])
def test_projection_where_a_lane_sums_three_features(k):
    """d = 130 of the 136 pairs of 17 atoms: the lanes' strided loop runs up to three times (at d = 50 never twice).  The
    bound d 2^-52 mass counts one rounding per product and per addition, so it holds for any d."""
    _projection_and_its_histogram(k, 65, n=17, d=130)


def _projection_and_its_histogram(k, S, n, d):
    nb = 12
    rng = np.random.default_rng(100 * k + S)
    xyz, pairs = _frames(S, n, 20 + k + S), _pairs(n, d, seed=2)
    mean, W = rng.uniform(2, 6, d), rng.standard_normal((d, k))
    want, mass = R.project(xyz, pairs, mean, W)
    x, p = _dev(xyz, torch.float32), _dev(pairs, torch.int32)
    mean_d, W_d = _dev(mean, torch.float64), _dev(W, torch.float64)
    ca, cb = 0, k - 1
    span = np.abs(want).max() + 1.0
    ra, rb = (-0.4 * span, 0.5 * span), (-0.3 * span, 0.45 * span)        # some structures fall outside
    counts = torch.zeros(nb, nb, dtype=torch.int32, device=DEV)
    outside = torch.zeros(1, dtype=torch.int32, device=DEV)
    ics = torch.zeros(S, k, dtype=torch.float64, device=DEV)
    tica.project_launch(x, p, mean_d, W_d, ics, (ca, cb, nb, ra, rb, counts, outside))
    got = ics.cpu().numpy()
    excess = np.abs(got - want) - d * U * mass
    print("k", k, "S", S, "max |delta| / bound", float((np.abs(got - want) / (d * U * mass)).max()))
    assert (excess <= 0).all()
    want_counts, want_out = R.bin2(got, ca, cb, nb, ra, rb)               # host binning of the RETURNED components
    assert np.array_equal(counts.cpu().numpy(), want_counts) and int(outside) == want_out
    assert int(counts.sum()) + int(outside) == S
    # the histogram alone gives the same counts, and a second launch adds
    only, only_out = torch.zeros_like(counts), torch.zeros_like(outside)
    tica.project_launch(x, p, mean_d, W_d, None, (ca, cb, nb, ra, rb, only, only_out))
    assert torch.equal(only, counts) and torch.equal(only_out, outside)
    tica.project_launch(x, p, mean_d, W_d, None, (ca, cb, nb, ra, rb, only, only_out))
    assert torch.equal(only, 2 * counts) and int(only_out) == 2 * want_out
    if S > 1:
        assert want_out > 0 and (want_counts > 0).sum() > 1               # not vacuous
        # the chunked host wrapper: the same components, the same counts
        model = tica.TicaModel(pairs, 1, mean, W, np.ones(k), np.ones(k), d, 1)
        h_ics, h_counts, h_out = tica.project(xyz, model, structures_per_launch=300, device=DEV, hist=(ca, cb, nb, ra, rb))
        assert np.array_equal(h_ics, got) and np.array_equal(h_counts, want_counts) and h_out == want_out
    bad = xyz.copy()
    bad[0, pairs[0, 0], 1] = np.nan                                        # a non-finite coordinate counts in outside
    nan_counts, nan_out = torch.zeros_like(counts), torch.zeros_like(outside)
    tica.project_launch(_dev(bad, torch.float32), p, mean_d, W_d, None, (ca, cb, nb, ra, rb, nan_counts, nan_out))
    assert int(nan_counts.sum()) + int(nan_out) == S and int(nan_out) >= 1


# ----------------------------------------------------------------------------- end to end: a slow hinge
def test_fit_finds_the_hinge_of_a_jittered_chain():
    """A 12-atom chain whose hinge angle follows an AR(1) path (phi = 0.995) between two wells, every atom with Gaussian
    jitter of 0.05 A; T = 4000, lag = 20, all 66 pair distances.  The device fit against the restatement's fit.

    Tolerance: the noise floor is the change of the RESTATEMENT's result when its moments are summed in reversed frame
    order -- measured: 4.1e-11 on the two leading eigenvalues (0.899, 0.628), 5.8e-10 on the leading component over the
    frames (unit variance); C0 keeps 24 of 66 directions, and the small kept ones amplify the moments' last bits --
    times 10, since the kernel's summation order differs from the restatement's by more than a reversal: the bounds are
    4.1e-10 and 5.8e-9.  (numpy's einsum order differs from the frame loop by 2.9e-11 and 2.6e-10.)  The floor is
    computed again on every run, from the restatement alone, and the bound taken from it."""
    T, lag = 4000, 20
    xyz, angle = R.hinge_chain(T, seed=0)
    pairs = tica.distance_pairs(np.arange(12), 0)
    assert len(pairs) == 66
    fwd, rev = R.moments(xyz, pairs, lag, "forward"), R.moments(xyz, pairs, lag, "reversed")
    mean_f, W_f, ev_f, rank_f = R.fit(fwd, lag)
    mean_r, W_r, ev_r, rank_r = R.fit(rev, lag)
    ic_f, ic_r = R.project(xyz, pairs, mean_f, W_f)[0], R.project(xyz, pairs, mean_r, W_r)[0]
    floor_ev = max(float(np.abs(ev_f - ev_r).max()), 2.0 ** -52)
    floor_ic = max(float(np.abs(ic_f[:, 0] - ic_r[:, 0]).max()), 2.0 ** -52)
    model = tica.fit([xyz], pairs, lag, device=DEV)
    ics = tica.project(xyz, model, device=DEV)
    d_ev, d_ic = float(np.abs(model.eigenvalues - ev_f).max()), float(np.abs(ics[:, 0] - ic_f[:, 0]).max())
    print("floor: eigenvalues", floor_ev, "IC1", floor_ic, "| device - restatement: eigenvalues", d_ev, "IC1", d_ic,
          "| eigenvalues", model.eigenvalues.tolist(), "rank", model.rank)
    assert model.rank == rank_f and model.W.shape == (66, 2) and ics.shape == (T, 2)
    assert d_ev <= 10 * floor_ev and d_ic <= 10 * floor_ic
    corr = [abs(float(np.corrcoef(ics[:, c], angle)[0, 1])) for c in (0, 1)]
    print("|corr| with the hinge angle", corr)
    assert corr[0] > corr[1] and corr[0] > 0.9
    assert abs(float(ics[:, 0].var()) - 1.0) < 0.05          # no kinetic-map scaling: unit variance on the data
    # compare: the trajectory against itself, and against the same frames with the hinge frozen in one well
    z, bonds = np.full(12, 6), np.stack([np.arange(11), np.arange(1, 12)], 1)
    same = tica.compare([xyz], xyz.copy(), z, bonds, lag=lag, sel=np.arange(12), excluded_neighbors=0, n_bins2=20, device=DEV)
    assert same["jsd"] == 0.0 and same["outside_gen"] == 0 and same["outside_ref"] == 0 and same["d"] == 66
    assert set(same) == set(tica.TICA_STATS_KEYS) and json.loads(json.dumps(same)) == same
    assert np.array(same["counts"]["ref"]).sum() == T and 0 < same["floor"] < 1 and same["jsd_ic"] == [0.0, 0.0]
    assert set(tica.summary_of(same)) <= set(tica.TICA_STATS_KEYS)
    frozen = R.hinge_chain(T, seed=0, frozen=True)[0]
    other = tica.compare([xyz], frozen, z, bonds, lag=lag, sel=np.arange(12), excluded_neighbors=0, n_bins2=20, device=DEV)
    print("floor", other["floor"], "frozen hinge jsd", other["jsd"], "outside", other["outside_gen"])
    assert other["jsd"] > other["floor"] and other["floor"] == same["floor"]
    with pytest.raises(ValueError, match="no peptide backbone"):
        tica.compare([xyz], xyz, z, bonds, lag=lag, device=DEV)


# ----------------------------------------------------------------------------- CLI
def test_backmap_cli_writes_tica_stats(tmp_path, capsys):
    """A fresh dipeptide-shaped run directory (the fixture pattern of test_backmap_gpu.py), the alanine dipeptide's
    topology, a random-walk reference of 40 frames: the file has the documented keys."""
    w = cg.data.WORKLOADS["dipeptide"]
    ds = cg.CGDataset(cg.data.synthetic_frames(3, w["n_atoms"], w["n_cgs"], w["box"], seed=11))
    model = cg.build_model(64, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], w["enc_nconv"], w["dec_nconv"], w["n_cgs"], seed=123)
    d = tmp_path / "run"
    d.mkdir()
    params = {"n_basis": 64, "n_rbf": w["n_rbf"], "atom_cutoff": w["atom_cutoff"], "cg_cutoff": w["cg_cutoff"],
              "enc_nconv": w["enc_nconv"], "dec_nconv": w["dec_nconv"], "n_cgs": w["n_cgs"], "activation": "swish", "det": False,
              "invariantdec": False, "cg_mp": False, "cg_radius_graph": False, "synthetic": True,
              "mapping": ds.props["CG_mapping"][0].tolist()}
    (d / "modelparams.json").write_text(json.dumps(params))
    torch.save(model.state_dict(), d / "model.pt")
    n = len(IR.ALA_Z)
    assert n == w["n_atoms"]
    rng = np.random.default_rng(0)
    ref = (rng.uniform(0, 6, (1, n, 3)) + np.cumsum(0.1 * rng.standard_normal((40, n, 3)), axis=0)).astype(np.float32)
    np.savez(tmp_path / "cg.npz", cg_xyz=torch.stack(ds.props["CG_nxyz"])[:, :, 1:].numpy())
    np.savez(tmp_path / "top.npz", z=IR.ALA_Z, bonds=IR.ALA_BONDS)
    np.savez(tmp_path / "ref.npz", xyz=ref, z=IR.ALA_Z, bonds=IR.ALA_BONDS, traj_starts=np.array([0, 22]))
    bm.main(f"-model {d} -cg {tmp_path / 'cg.npz'} -top {tmp_path / 'top.npz'} -n_samples 4 -out {tmp_path / 'out.npz'} "
            f"--tica_stats -tica_lag 5 -tica_bins 8 -ref {tmp_path / 'ref.npz'}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "dist_stats" not in line and set(line["tica_stats"]) == set(tica.summary_of({k: None for k in tica.TICA_STATS_KEYS}))
    stats = json.loads((tmp_path / "tica_stats.json").read_text())
    assert set(stats) == set(tica.TICA_STATS_KEYS)
    assert stats["n_ref"] == 40 and stats["n_gen"] == 12 and stats["lag"] == 5 and stats["n_bins2"] == 8
    assert stats["n_frame_pairs"] == (22 - 5) + (18 - 5)                   # two segments
    assert stats["sel"] == tica.backbone_atoms(IR.ALA_Z, IR.ALA_BONDS).tolist() and stats["d"] == len(tica.distance_pairs(stats["sel"]))
    assert np.array(stats["counts"]["gen"]).sum() + stats["outside_gen"] == 12 and np.array(stats["counts"]["ref"]).shape == (8, 8)
    assert not (tmp_path / "dist_stats.json").exists()
