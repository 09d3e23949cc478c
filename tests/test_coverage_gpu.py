"""Ensemble coverage on the device: K17 (csrc/superpose.hip) against the SVD restatement within a measured bound, the
nearest-neighbour reductions exactly against the kernel's own dense output, chunking, bad structures, ``compare`` on a
constructed two-cluster case, and the backmap command line."""
import functools
import json

import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd import backmap as bm, coverage
import internal_coords_restatement as IR
import superpose_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [(1, 1), (15, 17), (33, 16), (64, 49)]
ATOMS = [(3, 1), (5, 2), (7, 3), (9, 5), (22, 22), (70, 67)]


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _case(sa, sb, n, m):
    """Structures uniform in an 8 A box and the selection: all atoms in order when m == n, otherwise m scattered atoms in
    a random (not ascending) order."""
    rng = np.random.default_rng(1000 * sa + 100 * sb + 10 * n + m)
    a = rng.uniform(0, 8, (sa, n, 3)).astype(np.float32)
    b = rng.uniform(0, 8, (sb, n, 3)).astype(np.float32)
    sel = np.arange(n) if m == n else rng.permutation(n)[:m]
    return a, b, sel


def _special():
    """Pairs (a_k, b_k), 12 atoms each: identical bit for bit, a rotated and translated copy, the mirror image of a chiral
    structure, collinear atoms (against a random structure), coplanar atoms (against their mirror image, moved), two
    coincident atoms (against a rotated copy).  The test looks at every pair of the 6 x 6, not only the diagonal."""
    rng = np.random.default_rng(7)
    base = rng.uniform(0, 8, (12, 3))
    line = base[0] + np.outer(rng.uniform(-4, 4, 12), rng.standard_normal(3))
    flat = np.concatenate([rng.uniform(0, 8, (12, 2)), np.full((12, 1), 3.0)], axis=1)
    twin = base.copy()
    twin[9] = twin[4]
    a = [base, base, base, line, flat, twin]
    b = [base.copy(), base @ R.random_rotation(rng).T + rng.uniform(-5, 5, 3), base * np.array([-1.0, 1.0, 1.0]),
         rng.uniform(0, 8, (12, 3)), flat * np.array([1.0, -1.0, 1.0]) + 2.0, twin @ R.random_rotation(rng).T]
    return np.array(a, np.float32), np.array(b, np.float32)


def _launch(a, b, sel, **kw):
    """One cgv_superpose call: the dense rmsd^2 and the squared minima, on the host."""
    sa, sb = len(a), len(b)
    state = coverage.new_state(sa, sb, DEV)
    dense = torch.full((sa, sb), -1.0, dtype=torch.float64, device=DEV)
    coverage.superpose_launch(_dev(a, torch.float32), _dev(b, torch.float32), _dev(sel, torch.int32), **state, dense=dense, **kw)
    return dense.cpu().numpy(), {k: v.cpu().numpy() for k, v in state.items()}


def _ratios(a, b, sel, rng):
    """|change of the restatement's rmsd^2| / (2^-52 (G_a + G_b) / m) under a random permutation of the atom order (the
    quantity does not change mathematically): the restatement's own rounding noise on these inputs."""
    one, two = R.rmsd2_matrix(a, b, sel), R.rmsd2_matrix(a, b, np.asarray(sel)[rng.permutation(len(sel))])
    unit = R.bound_unit(a, b, sel)
    assert (np.abs(one - two)[unit == 0] == 0).all()
    return (np.abs(one - two)[unit > 0] / unit[unit > 0]).ravel()


@functools.lru_cache(maxsize=None)
def _c():
    """The bound's constant: 10 x the worst ratio of ``_ratios`` over every case of the dense test and the special
    structures, measured on the CPU on each run."""
    rng = np.random.default_rng(99)
    worst = [_ratios(*_case(sa, sb, n, m), rng).max(initial=0.0) for sa, sb in SIZES for n, m in ATOMS]
    sa, sb = _special()
    worst.append(_ratios(sa, sb, np.arange(12), rng).max())
    floor = float(max(worst))
    print("restatement's noise floor under an atom permutation:", floor, "x 2^-52 (G_a + G_b) / m; c =", 10 * floor)
    return 10.0 * floor


def _check(got, a, b, sel, what):
    want, unit = R.rmsd2_matrix(a, b, sel), R.bound_unit(a, b, sel)
    assert got.shape == want.shape and np.isfinite(got).all() and (got >= 0).all()
    err = np.abs(got - want)
    ratio = float((err[unit > 0] / unit[unit > 0]).max(initial=0.0))
    print(what, "max |delta rmsd^2| / (2^-52 (G_a + G_b) / m) =", ratio, "bound c =", _c())
    assert (err <= _c() * unit).all(), (what, ratio, _c())


# ----------------------------------------------------------------------------- dense rmsd^2 against the restatement
@pytest.mark.parametrize("n,m", ATOMS)
@pytest.mark.parametrize("sa,sb", SIZES)
def test_dense_rmsd2_equals_the_restatement_within_its_own_noise(sa, sb, n, m):
    """|delta rmsd^2| <= c 2^-52 (G_a + G_b) / m.  c is 10 x the restatement's own worst change under a random permutation
    of the atom order over all these cases and the special structures (``_c``), which covers a different summation order
    and a different eigen-solver on the device.  The floor is computed again on every run, from the restatement alone.  When this
    was written the floor over the dense cases was 4.4 (Sa 64, Sb 49, n 70, m 67), so c = 44 unless the special structures
    raise it; a host emulation of the kernel's arithmetic (the same Jacobi text compiled for the CPU, sums in atom order)
    reached 3.5 on these cases.  The device's own worst ratio has not been measured: no GPU run could be made."""
    a, b, sel = _case(sa, sb, n, m)
    got, _ = _launch(a, b, sel)
    _check(got, a, b, sel, f"Sa {sa} Sb {sb} n {n} m {m}")
    if m == n:                                               # the default selection is every atom
        assert np.array_equal(coverage.rmsd_matrix(a, b, device=DEV), np.sqrt(got))
    else:
        assert np.array_equal(coverage.rmsd_matrix(a, b, sel, device=DEV), np.sqrt(got))


def test_special_structures_are_finite_and_within_the_same_bound():
    a, b = _special()
    sel = np.arange(12)
    got, _ = _launch(a, b, sel)
    _check(got, a, b, sel, "special structures")
    want = R.rmsd2_matrix(a, b, sel)
    unit = R.bound_unit(a, b, sel)
    assert got[0, 0] >= 0 and got[0, 0] <= _c() * unit[0, 0]             # identical bits: not NaN, zero within the bound
    assert got[1, 1] <= _c() * unit[1, 1] + want[1, 1]                   # a rigid copy
    assert want[2, 2] > 0.1 and got[2, 2] > 0.1                          # the mirror image of a chiral structure stays away
    # the hand-computed case: the tetrahedron's four atoms scattered among twelve
    tet, sel4 = np.zeros((2, 12, 3), np.float32), np.array([10, 1, 6, 3])
    tet[:] = np.random.default_rng(8).uniform(0, 8, (2, 12, 3))
    tet[0, sel4] = R.CHIRAL_TETRAHEDRON + 3.0
    tet[1, sel4] = R.CHIRAL_TETRAHEDRON * np.array([-1.0, 1.0, 1.0]) + 1.0
    got4, _ = _launch(tet[:1], tet[1:], sel4)
    _check(got4, tet[:1], tet[1:], sel4, "chiral tetrahedron")
    assert abs(got4[0, 0] - R.CHIRAL_MIRROR_RMSD2) <= _c() * R.bound_unit(tet[:1], tet[1:], sel4)[0, 0]


# ----------------------------------------------------------------------------- minima, exactly
def test_minima_equal_the_min_rule_on_the_kernels_own_dense_output():
    a, b, sel = _case(64, 49, 9, 5)
    b[2] = a[10]                                             # row 10 has its minimum (0 within rounding) in column 2 ...
    b[5] = b[2]                                              # ... and, with the same bits, in column 5
    a[1] = b[20]
    a[7] = a[1]                                              # column 20: rows 1 and 7
    dense, st = _launch(a, b, sel)
    assert np.array_equal(dense[:, 5], dense[:, 2]) and np.array_equal(dense[7], dense[1])
    assert st["row_arg"][10] == 2 and st["col_arg"][20] == 1               # the lower index of a tie wins
    for axis, vmin, arg in ((1, "row_min", "row_arg"), (0, "col_min", "col_arg")):
        v, i = R.min_rule(dense, axis)
        assert np.array_equal(st[vmin], v) and np.array_equal(st[arg], i), axis
    assert 5 not in st["row_arg"] and 7 not in st["col_arg"]
    # the chunk's offsets shift the indices, nothing else
    again, st2 = _launch(a, b, sel, off_a=100, off_b=1000)
    assert np.array_equal(again, dense)
    assert np.array_equal(st2["row_arg"], st["row_arg"] + 1000) and np.array_equal(st2["col_arg"], st["col_arg"] + 100)


# ----------------------------------------------------------------------------- chunking
def test_chunked_nearest_equals_the_single_launch_bit_for_bit():
    a, b, sel = _case(40, 53, 9, 5)
    b[20], b[44] = b[3], b[3]                                # ties across chunk boundaries
    one = coverage.nearest(a, b, sel, device=DEV)
    dense, st = _launch(a, b, sel)
    assert np.array_equal(one[0], np.sqrt(st["row_min"])) and np.array_equal(one[1], st["row_arg"])
    assert np.array_equal(one[2], np.sqrt(st["col_min"])) and np.array_equal(one[3], st["col_arg"])
    assert one[1].dtype == np.int64 and one[0].dtype == np.float64
    for per in (16, 7):
        got = coverage.nearest(a, b, sel, structures_per_launch=per, device=DEV)
        for x, y in zip(got, one):
            assert np.array_equal(x, y), per


def test_exclude_self_skips_the_diagonal():
    a, _, sel = _case(40, 1, 9, 5)
    a[30] = a[4]                                             # a twin: distance 0 off the diagonal
    dense = coverage.rmsd_matrix(a, a, sel, device=DEV)
    assert (np.diag(dense) <= 1e-6).all()
    for per in (4096, 16):
        rmin, rarg, cmin, carg = coverage.nearest(a, a, sel, exclude_self=True, structures_per_launch=per, device=DEV)
        assert (rarg != np.arange(40)).all() and (carg != np.arange(40)).all()
        v, i = R.min_rule(dense, 1, skip=np.eye(40, dtype=bool))
        assert np.array_equal(rmin, v) and np.array_equal(rarg, i)
        v, i = R.min_rule(dense, 0, skip=np.eye(40, dtype=bool))
        assert np.array_equal(cmin, v) and np.array_equal(carg, i)
        assert rarg[30] == 4 and rarg[4] == 30
    want = np.arange(40)
    want[30] = 4                                             # without the switch: itself, or its lower twin
    assert np.array_equal(coverage.nearest(a, a, sel, device=DEV)[1], want)


# ----------------------------------------------------------------------------- bad structures
def test_a_nan_inside_the_selection_is_a_nan_row_and_enters_no_minimum():
    a, b, sel = _case(33, 16, 9, 5)
    clean, st0 = _launch(a, b, sel)
    inside, outside = a.copy(), a.copy()
    inside[11, sel[2], 1] = np.nan
    outside[11, [k for k in range(9) if k not in sel][0], 1] = np.nan
    dense, st = _launch(inside, b, sel)
    assert np.isnan(dense[11]).all() and np.array_equal(np.delete(dense, 11, 0), np.delete(clean, 11, 0))
    assert st["row_min"][11] == np.inf and st["row_arg"][11] == -1
    v, i = R.min_rule(np.delete(clean, 11, 0), 0)
    assert np.array_equal(st["col_min"], v) and np.array_equal(st["col_arg"], np.where(i >= 11, i + 1, i))
    assert 11 not in st["col_arg"]
    same, st_out = _launch(outside, b, sel)
    assert np.array_equal(same, clean) and all(np.array_equal(st_out[k], st0[k]) for k in st0)
    # a bad column structure
    bb = b.copy()
    bb[3, sel[0], 2] = np.inf
    dense, st = _launch(a, bb, sel)
    assert np.isnan(dense[:, 3]).all() and st["col_min"][3] == np.inf and st["col_arg"][3] == -1 and 3 not in st["row_arg"]


# ----------------------------------------------------------------------------- determinism, validation
def test_two_identical_calls_give_identical_bits_and_bad_arguments_raise_before_a_launch():
    a, b, sel = _case(64, 49, 70, 67)
    d1, s1 = _launch(a, b, sel)
    d2, s2 = _launch(a, b, sel)
    assert d1.tobytes() == d2.tobytes() and all(s1[k].tobytes() == s2[k].tobytes() for k in s1)
    for call in (coverage.rmsd_matrix, coverage.nearest):
        with pytest.raises(ValueError):
            call(a, b, [0, 70], device=DEV)
        with pytest.raises(ValueError):
            call(a, b, [], device=DEV)
        with pytest.raises(ValueError):
            call(a, b[:, :69], device=DEV)
    x, y, s = _dev(a, torch.float32), _dev(b, torch.float32), _dev(sel, torch.int32)
    with pytest.raises(ValueError):
        coverage.superpose_launch(x, y, s[:0], **coverage.new_state(64, 49, DEV))
    with pytest.raises(ValueError):
        coverage.superpose_launch(x, y[:, :69].contiguous(), s, **coverage.new_state(64, 49, DEV))


# ----------------------------------------------------------------------------- compare
def test_compare_on_two_clusters():
    """The reference: 30 + 30 frames of noise 0.05 A around two random 10-atom shapes (several A apart after
    superposition), every frame randomly rotated and translated.  Samples near the first shape only cover half of the
    reference and are all near it; samples of both cover all of it."""
    rng = np.random.default_rng(5)
    shapes = rng.uniform(0, 8, (2, 10, 3))

    def draw(which):
        out = [(shapes[w] + 0.05 * rng.standard_normal((10, 3))) @ R.random_rotation(rng).T + rng.uniform(-9, 9, 3) for w in which]
        return np.array(out, np.float32)
    ref = draw([0, 1] * 30)
    z = np.array([6, 1, 7, 6, 1, 8, 6, 6, 1, 7])
    delta = 0.5                                              # noise: rmsd ~ 0.1; the two shapes: > 1
    assert R.rmsd2_pair(shapes[0], shapes[1], np.flatnonzero(z != 1)) > 1.0
    one = coverage.compare(ref, draw([0] * 25), z, thresholds=(delta,), device=DEV)
    assert set(one) == set(coverage.COV_STATS_KEYS) and json.loads(json.dumps(one)) == one
    assert one["atoms"] == [0, 2, 3, 5, 6, 7, 9] and one["n_ref"] == 60 and one["n_gen"] == 25
    assert one["cov_r"] == [0.5] and one["cov_p"] == [1.0] and one["unmatched_r"] == one["unmatched_p"] == 0
    assert one["mat_p_mean"] < 0.3 and one["mat_r_mean"] > 0.5
    assert sum(one["nearest_ref"]) == 25 and len(one["nearest_ref"]) == 60 and sum(one["nearest_ref"][1::2]) == 0
    assert one["floor"]["cov_r"] == [0.0] and one["floor"]["cov_p"] == [0.0]      # even frames are shape 0, odd frames shape 1
    both = coverage.compare(ref, draw([0, 1, 1, 0] * 6), z, thresholds=(delta,), device=DEV)
    assert both["cov_r"] == [1.0] and both["cov_p"] == [1.0] and sum(both["nearest_ref"]) == 24
    mixed = coverage.compare(draw([0, 0, 1, 1] * 15), draw([0]), z, thresholds=(delta, 50.0), atoms="all", device=DEV)
    assert mixed["floor"]["cov_r"] == [1.0, 1.0] and mixed["atoms"] == list(range(10)) and mixed["cov_r"] == [0.5, 1.0]


# ----------------------------------------------------------------------------- CLI
def test_backmap_cli_writes_cov_stats_and_nothing_without_the_switch(tmp_path, capsys):
    """A fresh dipeptide-shaped run directory (the fixture pattern of test_tica_gpu.py) and a random reference of 9
    frames: the file has the documented keys; without the switch the outputs are what they were."""
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
    ref = np.random.default_rng(0).uniform(0, 6, (9, n, 3)).astype(np.float32)
    np.savez(tmp_path / "cg.npz", cg_xyz=torch.stack(ds.props["CG_nxyz"])[:, :, 1:].numpy())
    np.savez(tmp_path / "top.npz", z=IR.ALA_Z, bonds=IR.ALA_BONDS)
    np.savez(tmp_path / "ref.npz", xyz=ref, z=IR.ALA_Z, bonds=IR.ALA_BONDS)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    base = f"-model {d} -cg {tmp_path / 'cg.npz'} -top {tmp_path / 'top.npz'} -n_samples 4"
    bm.main(f"{base} -out {tmp_path / 'a' / 'out.npz'} --cov_stats -cov_thresholds 1.0 4.0 -ref {tmp_path / 'ref.npz'}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "dist_stats" not in line and "tica_stats" not in line
    assert set(line["cov_stats"]) == set(coverage.summary_of({k: None for k in coverage.COV_STATS_KEYS}))
    stats = json.loads((tmp_path / "a" / "cov_stats.json").read_text())
    assert set(stats) == set(coverage.COV_STATS_KEYS) and line["cov_stats"] == coverage.summary_of(stats)
    assert stats["n_ref"] == 9 and stats["n_gen"] == 12 and stats["thresholds"] == [1.0, 4.0]
    assert stats["atoms"] == np.flatnonzero(np.asarray(IR.ALA_Z) != 1).tolist() and sum(stats["nearest_ref"]) == 12
    assert len(stats["cov_r"]) == 2 and stats["cov_r"][0] <= stats["cov_r"][1] and stats["mat_r_mean"] > 0
    assert set(stats["floor"]) == set(coverage.METRIC_KEYS)
    bm.main(f"{base} -out {tmp_path / 'b' / 'out.npz'}".split())
    line_b = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "cov_stats" not in line_b and set(line_b) == set(line) - {"cov_stats"}
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["out.npz"]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["cov_stats.json", "out.npz"]
    with np.load(tmp_path / "a" / "out.npz") as fa, np.load(tmp_path / "b" / "out.npz") as fb:
        assert set(fa.files) == set(fb.files) and fa["xyz"].tobytes() == fb["xyz"].tobytes()
