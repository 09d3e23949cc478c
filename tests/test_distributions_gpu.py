"""Distribution statistics on the device: K15 (csrc/internal_hist.hip) against the fp64 restatement, integer for integer;
``distributions.compare`` end to end; the ``backmap`` CLI with ``--dist_stats``.

Equality with the restatement is a fair demand only of structures whose values are not within rounding of a bin edge:
``internal_coords_restatement.well_conditioned`` (1e-9 of a bin width from every edge, sin >= 1e-3 for the angles a
torsion is built on).  The seeds are fixed so that at most 1 structure in 100 is redrawn; the tests assert it."""
import functools
import json

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import _lib, backmap as bm, distributions as D
import internal_coords_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANGE = (0.5, 2.5)
NARROW = (1.3, 1.45)                      # most bonds of the jittered structures fall outside: under and over fill up
CONFIGS = ((7, 5, RANGE), (36, 36, RANGE), (36, 36, NARROW))
S_MAX = 257


def _launch(xyz, coords, n_bins, n_bins2, bond_range=RANGE, into=None):
    table = D._DeviceTable(coords, DEV)
    if into is None:
        into = (torch.zeros(coords.n_features, n_bins + 3, dtype=torch.int32, device=DEV),
                torch.zeros(coords.n_pairs, n_bins2, n_bins2, dtype=torch.int32, device=DEV))
    D.internal_hist(torch.as_tensor(xyz, dtype=torch.float32).to(DEV).contiguous(), table, n_bins, n_bins2, bond_range, *into)
    return into


def _equal(got, want):
    counts, pair_counts = got[0].cpu().numpy().astype(np.int64), got[1].cpu().numpy().astype(np.int64)
    print("features", counts.shape, "differing slots", int((counts != want[0]).sum()), "pairs", pair_counts.shape,
          "differing slots", int((pair_counts != want[1]).sum()))
    assert np.array_equal(counts, want[0]) and np.array_equal(pair_counts, want[1])


@functools.lru_cache(maxsize=None)
def _dipeptide():
    """The alanine dipeptide table with its (phi, psi) pair, ``S_MAX`` jittered structures that are well conditioned for
    every configuration the tests use, and their restated values -- computed once, never modified."""
    coords, rows = D.backbone_pairs(D.internal_coords(R.ALA_Z, R.ALA_BONDS), R.ALA_Z, R.ALA_BONDS)
    assert len(rows) == 1
    x0 = R.embed(R.ALA_BONDS, 22, seed=5)
    xyz, redrawn = R.draw_structures(x0, S_MAX, 0.1, 11, coords.feat, coords.kind, CONFIGS)
    print("dipeptide: redrawn", redrawn, "of", S_MAX)
    assert redrawn * 100 <= S_MAX
    xyz.setflags(write=False)
    return coords, xyz, R.values(xyz, coords.feat, coords.kind)


def _torsion_pairs(coords, count, seed):
    tors = np.nonzero(coords.kind == D.TORSION)[0]
    return np.random.default_rng(seed).choice(tors, (count, 2)).astype(np.int32)


# ----------------------------------------------------------------------------- K15 vs the restatement
@pytest.mark.parametrize("S", [1, 3, 70, 257])
@pytest.mark.parametrize("n_bins,n_bins2", [(7, 5), (36, 36)])
def test_kernel_equals_the_restatement(S, n_bins, n_bins2):
    coords, xyz, vals = _dipeptide()
    want = R.restate_from(vals[:S], coords.kind, coords.pairs, n_bins, n_bins2, RANGE)
    assert want[0].sum() == S * coords.n_features and want[1].sum() == S and not want[0][:, [0, -2, -1]].any()
    got = _launch(xyz[:S], coords, n_bins, n_bins2)
    _equal(got, want)
    again = _launch(xyz[:S], coords, n_bins, n_bins2)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])                      # the same bytes on every run


@pytest.mark.parametrize("n_bins2", [5, 36])
@pytest.mark.parametrize("which", ["none", "one_more_than_a_tile"])
def test_pair_tables_of_no_pair_and_of_more_than_a_tile(which, n_bins2):
    coords, xyz, vals = _dipeptide()
    tile = int(_lib.load().cgv_internal_hist_pair_tile(n_bins2))
    count = 0 if which == "none" else tile + 1
    c = coords.with_pairs(_torsion_pairs(coords, count, seed=n_bins2))
    assert c.n_pairs == count
    want = R.restate_from(vals[:70], c.kind, c.pairs, 36, n_bins2, RANGE)
    assert want[1].sum() == 70 * count
    _equal(_launch(xyz[:70], c, 36, n_bins2), want)


def test_a_table_without_one_kind_and_bonds_outside_the_range():
    coords, xyz, vals = _dipeptide()
    keep = np.nonzero(coords.kind != D.ANGLE)[0]
    c = D.InternalCoords(np.ascontiguousarray(coords.feat[keep]), np.ascontiguousarray(coords.kind[keep]),
                         np.searchsorted(keep, coords.pairs).astype(np.int32), 22)
    sub = [[row[f] for f in keep] for row in vals[:70]]
    _equal(_launch(xyz[:70], c, 36, 36), R.restate_from(sub, c.kind, c.pairs, 36, 36, RANGE))
    want = R.restate_from(vals[:70], coords.kind, coords.pairs, 36, 36, NARROW)
    bonds = coords.kind == D.BOND
    print("under", int(want[0][bonds, 0].sum()), "over", int(want[0][bonds, -2].sum()), "inside", int(want[0][bonds, 1:-2].sum()))
    assert want[0][bonds, 0].sum() > 70 and want[0][bonds, -2].sum() > 70 and want[0][bonds, 1:-2].sum() > 70
    assert not want[0][~bonds][:, [0, -2]].any()                                 # angles and torsions have no outside
    _equal(_launch(xyz[:70], coords, 36, 36, NARROW), want)


def test_a_table_of_more_than_one_feature_tile():
    z, bonds = R.branched_chain(70, seed=3)
    coords = D.internal_coords(z, bonds)
    tile = int(_lib.load().cgv_internal_hist_feature_tile(36))
    assert coords.n_features > tile and coords.n_features % tile                  # several tiles, the last one partial
    c = coords.with_pairs(_torsion_pairs(coords, 3, seed=1))
    xyz, redrawn = R.draw_structures(R.embed(bonds, 70, seed=2), 3, 0.1, 4, c.feat, c.kind, ((36, 36, RANGE),))
    assert redrawn == 0
    _equal(_launch(xyz, c, 36, 36), R.restate(xyz, c.feat, c.kind, c.pairs, 36, 36, RANGE))


def test_a_structure_with_a_nan_counts_as_invalid_and_in_no_pair():
    coords, xyz, _vals = _dipeptide()
    x = xyz[:3].copy()
    x[1, 8, 2] = np.nan                                                          # CA of the second structure
    want = R.restate(x, coords.feat, coords.kind, coords.pairs, 36, 36, RANGE)
    touches = np.array([8 in coords.atoms(f) for f in range(coords.n_features)])
    assert np.array_equal(want[0][:, -1], touches.astype(np.int64)) and touches.sum() > 10 and want[1].sum() == 2
    _equal(_launch(x, coords, 36, 36), want)
    x[1, 8, 2] = np.inf
    _equal(_launch(x, coords, 36, 36), want)


def test_two_launches_over_halves_add_up_to_one_launch():
    coords, xyz, vals = _dipeptide()
    whole = _launch(xyz, coords, 36, 36)
    halves = _launch(xyz[:128], coords, 36, 36)
    _launch(xyz[128:], coords, 36, 36, into=halves)
    assert torch.equal(halves[0], whole[0]) and torch.equal(halves[1], whole[1])
    # and through the host module, which adds the launches' int32 counts to int64 totals
    out = D.histograms(xyz, coords, 36, 36, RANGE, structures_per_launch=100)
    assert out["counts"].dtype == np.int64 and out["pair_counts"].dtype == np.int64
    _equal((torch.from_numpy(out["counts"]), torch.from_numpy(out["pair_counts"])),
           R.restate_from(vals, coords.kind, coords.pairs, 36, 36, RANGE))
    assert np.array_equal(out["counts"], whole[0].cpu().numpy())


def test_structures_too_large_to_stage_take_the_direct_path():
    n = D.limits()["staged_atoms"] + 1                                           # the smallest frame that selects it
    bonds = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    z = np.full(n, 6)
    coords = D.internal_coords(z, bonds)
    assert coords.n_features == (n - 1) + (n - 2) + (n - 3)
    c = coords.with_pairs(_torsion_pairs(coords, 3, seed=2))
    xyz, redrawn = R.draw_structures(R.embed(bonds, n, seed=6), 3, 0.1, 8, c.feat, c.kind, ((36, 5, RANGE),))
    assert redrawn == 0
    _equal(_launch(xyz, c, 36, 5), R.restate(xyz, c.feat, c.kind, c.pairs, 36, 5, RANGE))


def test_a_limit_exceeded_is_an_error_and_nothing_is_written():
    coords, xyz, _vals = _dipeptide()
    lim = D.limits()
    x = torch.from_numpy(xyz[:3].copy()).to(DEV)
    table = D._DeviceTable(coords, DEV)
    counts = torch.full((coords.n_features, 39), 7, dtype=torch.int32, device=DEV)
    pair_counts = torch.full((1, 36, 36), 7, dtype=torch.int32, device=DEV)

    def call(n_atoms=22, n_features=coords.n_features, n_pairs=1, n_bins=36, n_bins2=36):
        _lib.call("cgv_internal_hist", _lib.ptr(x), _lib.ptr(table.feat), _lib.ptr(table.kind), _lib.ptr(table.pairs), 3, n_atoms,
                  n_features, n_pairs, n_bins, n_bins2, 0.5, 2.5, _lib.ptr(counts), _lib.ptr(pair_counts), _lib.stream_ptr())
    for kw, match in ((dict(n_features=lim["features"] + 1), "max_features"), (dict(n_pairs=lim["pairs"] + 1), "max_pairs"),
                      (dict(n_bins=lim["bins"] + 1), "max_bins"), (dict(n_bins2=lim["bins2"] + 1), "max_bins2"),
                      (dict(n_atoms=lim["atoms"] + 1), "max_atoms"), (dict(n_bins=0), "max_bins")):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((pair_counts == 7).all())
    with pytest.raises(ValueError, match="features"):
        D.histograms(xyz[:3], D.InternalCoords(np.zeros((lim["features"] + 1, 4), np.int32), np.full(lim["features"] + 1, 2, np.int32),
                                               np.zeros((0, 2), np.int32), 22))
    with pytest.raises(ValueError, match="n_bins"):
        D.histograms(xyz[:3], coords, n_bins=lim["bins"] + 1)
    call()                                                                       # within the limits: it adds to what is there
    torch.cuda.synchronize()
    assert int(counts.sum()) == 7 * counts.numel() + 3 * coords.n_features


# ----------------------------------------------------------------------------- compare(), end to end
def _rotate_about_bond(xyz, a, b, moving, degrees):
    """``xyz [S,n,3]`` with the atoms ``moving`` rotated about the axis a -> b (Rodrigues), in fp64, rounded once."""
    x = xyz.astype(np.float64)
    k = x[:, b] - x[:, a]
    k /= np.linalg.norm(k, axis=1, keepdims=True)
    t = np.radians(degrees)
    v = x[:, moving] - x[:, b][:, None]
    kk = k[:, None]
    x[:, moving] = x[:, b][:, None] + v * np.cos(t) + np.cross(kk, v) * np.sin(t) + kk * (kk * v).sum(-1, keepdims=True) * (1 - np.cos(t))
    return x.astype(np.float32)


def test_compare_is_zero_on_itself_and_sees_a_rotated_torsion():
    rng = np.random.default_rng(21)
    ref = (R.embed(R.ALA_BONDS, 22, seed=5) + 0.05 * rng.standard_normal((200, 22, 3))).astype(np.float32)
    same = D.compare(ref, ref.copy(), R.ALA_Z, R.ALA_BONDS, structures_per_launch=64)
    assert set(same) == set(D.DIST_STATS_KEYS) and same["n_ref"] == 200 and same["n_gen"] == 200
    assert same["features"]["jsd"] == [0.0] * len(same["features"]["jsd"]) and same["pairs"]["jsd"] == [0.0]
    assert same["mean"] == {"all": {"bond": 0.0, "angle": 0.0, "torsion": 0.0}, "heavy": {"bond": 0.0, "angle": 0.0, "torsion": 0.0},
                            "pair": 0.0}
    assert same["counts"]["ref"] == same["counts"]["gen"] and np.sum(same["counts"]["ref"]) == 200 * len(same["features"]["kind"])
    floor = same["floor"]
    print("noise floor", floor)
    assert 0.0 < floor["all"]["torsion"] < 1.0 and 0.0 < floor["pair"] < 1.0 and 0.0 < floor["heavy"]["bond"] < 1.0
    json.dumps(same)
    # psi = N-CA-C-N' rotated by 90 degrees: everything beyond the CA-C bond turns about it
    moving = [15, 16, 17, 18, 19, 20, 21]
    gen = _rotate_about_bond(ref, 8, 14, moving, 90.0)
    out = D.compare(ref, gen, R.ALA_Z, R.ALA_BONDS)
    atoms = [tuple(a) for a in out["features"]["atoms"]]
    psi = atoms.index(R.ALA_PSI)
    assert out["pairs"]["psi"] == [psi] and atoms[out["pairs"]["phi"][0]] == R.ALA_PHI
    print("psi", out["features"]["jsd"][psi], "floor", out["features"]["floor"][psi], "pair", out["pairs"]["jsd"], out["pairs"]["floor"])
    assert out["features"]["jsd"][psi] > out["features"]["floor"][psi] and out["features"]["jsd"][psi] > 0.5
    assert out["pairs"]["jsd"][0] > out["pairs"]["floor"][0]
    assert out["mean"]["all"]["torsion"] > out["floor"]["all"]["torsion"]
    fixed = [f for f, a in enumerate(atoms) if not set(a) & set(moving)]          # bit-identical coordinates
    assert len(fixed) > 40 and all(out["features"]["jsd"][f] == 0.0 for f in fixed)
    assert out["features"]["floor"] == same["features"]["floor"]                  # the floor is the reference's own


# ----------------------------------------------------------------------------- the backmap CLI
def test_backmap_cli_writes_dist_stats_only_when_asked(tmp_path, capsys):
    import coarsegrainingvae_amd as cg
    from test_backmap_gpu import _setup, _write_run
    w, ds, model = _setup("dipeptide", 64, 6)
    d = _write_run(tmp_path, w, model, ds.props["CG_mapping"][0])
    fr = cg.data.synthetic_frames(6, 22, 3, 6.0, seed=4)
    z = fr["nxyz"][0][:, 0].numpy().astype(np.int64)
    np.savez(tmp_path / "traj.npz", xyz=torch.stack(fr["nxyz"])[:, :, 1:].numpy(), z=z, bonds=fr["bond_edge_list"][0].numpy())
    T, K = 6, 3
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    bm.main(f"-model {d} -traj {tmp_path / 'traj.npz'} -n_samples {K} -out {tmp_path / 'a' / 'out.npz'} --dist_stats".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(line["dist_stats"]) == {"mean", "floor", "n_ref", "n_gen"} and line["dist_stats"]["n_gen"] == T * K
    stats = json.loads((tmp_path / "a" / "dist_stats.json").read_text())
    assert set(stats) == set(D.DIST_STATS_KEYS) and stats["n_ref"] == T and stats["n_gen"] == T * K
    nf = len(stats["features"]["kind"])
    assert nf == D.internal_coords(z, fr["bond_edge_list"][0].numpy()).n_features > 0
    assert np.sum(stats["counts"]["gen"]) == T * K * nf and np.sum(stats["counts"]["ref"]) == T * nf
    assert line["dist_stats"]["mean"] == stats["mean"] and set(stats["mean"]) == {"all", "heavy", "pair"}
    assert set(stats["features"]) == {"atoms", "kind", "heavy", "jsd", "floor", "outside_ref", "outside_gen"}
    bm.main(f"-model {d} -traj {tmp_path / 'traj.npz'} -n_samples {K} -out {tmp_path / 'b' / 'out.npz'}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "dist_stats" not in line and not (tmp_path / "b" / "dist_stats.json").exists()
    with np.load(tmp_path / "a" / "out.npz") as fa, np.load(tmp_path / "b" / "out.npz") as fb:
        assert set(fa.files) == set(fb.files) and fa["xyz"].tobytes() == fb["xyz"].tobytes()


# ----------------------------------------------------------------------------- run_ala --dist_eval
def test_run_ala_dist_eval_writes_dist_stats_and_leaves_everything_else(tmp_path, capsys, monkeypatch):
    from coarsegrainingvae_amd import evaluate as ev, run_ala
    monkeypatch.chdir(tmp_path)
    base = ("-device 0 -dataset dipeptide -n_cgs 3 -batch_size 8 -ndata 40 -nepochs 1 -atom_cutoff 8.5 -cg_cutoff 9.5 -beta 0.05 "
            "-gamma 25.0 -dec_nconv 2 -enc_nconv 2 -lr 0.001 -n_basis 64 -n_rbf 8 -n_ensemble 2 --synthetic")
    out = {}
    for name, flag in (("with", " --dist_eval"), ("without", "")):
        run_ala.main(f"-logdir {name} {base}{flag}".split())
        out[name] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    d_with, d_without = next(tmp_path.glob("with_*_N3")), next(tmp_path.glob("without_*_N3"))
    stats = json.loads((d_with / "dist_stats.json").read_text())
    assert set(stats) == set(D.DIST_STATS_KEYS) and stats["n_ref"] == 4 and stats["n_gen"] == 8          # 4 hold-out frames, 2 samples
    assert out["with"]["dist_stats"] == D.summary_of(stats) and "dist_stats" not in out["with"]["test_stats"]
    assert "dist_stats" not in out["without"] and not (d_without / "dist_stats.json").exists()
    # cv_stats.csv keeps its columns (the values of two runs in one process differ: the device sample generator carries on)
    rows = [(d / "cv_stats.csv").read_text().splitlines() for d in (d_with, d_without)]
    assert rows[0][0] == rows[1][0] == ",".join(ev.CV_STATS_COLUMNS) and [len(r) for r in rows] == [2, 2]
    assert len(rows[0][1].split(",")) == len(rows[1][1].split(",")) == len(ev.CV_STATS_COLUMNS)
    assert sorted(p.name for p in d_with.iterdir() if not p.name.startswith("test_")) == \
        sorted([p.name for p in d_without.iterdir() if not p.name.startswith("test_")] + ["dist_stats.json"])
    stored = json.loads((d_without / "modelparams.json").read_text())
    assert "dist_eval" not in stored and json.loads((d_with / "modelparams.json").read_text())["dist_eval"] is True
