"""Host side of backmapping (no GPU): the dense restatement of the ensemble checks on a hand-built molecule, the pure
assembly of K14's outputs, bond-list validation, the CLI's parser and input validation, ``load_run``'s refusals."""
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, backmap as bm, evaluate as ev
import ensemble_check_restatement as R


def test_the_library_declares_and_exports_the_ensemble_check():
    for name in ("cgv_ensemble_check", "cgv_ensemble_check_max_samples", "cgv_ensemble_check_max_classes"):
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.cgv_ensemble_check_max_samples() >= 256
    assert lib.cgv_ensemble_check_max_classes() == lib.cgv_sample_quality_max_classes()


def test_hand_built_molecule_is_what_its_description_says():
    xyz, z, bonds, carbon = R.alkane()
    assert xyz.shape == (74, 3) and len(bonds) == 73 and (z == 6).sum() == 24 and np.all(bonds[:, 0] < bonds[:, 1])
    d = np.linalg.norm(xyz[:, None] - xyz[None], axis=-1)
    assert np.allclose(d[carbon[:-1], carbon[1:]], 1.5) and np.allclose(d[carbon[:-2], carbon[2:]], 2.45, atol=5e-3)
    ch = bonds[z[bonds[:, 1]] == 1]
    assert len(ch) == 50 and np.allclose(d[ch[:, 0], ch[:, 1]], 1.09)
    thr = ev.bond_thresholds([1, 6])
    assert abs(float(thr[1, 1]) ** 0.5 - 1.768) < 1e-5 and abs(float(thr[0, 0]) ** 0.5 - 0.598) < 1e-5


def test_restatement_gives_the_hand_computed_counts_on_every_case():
    names, gen, z, bonds, want = R.cases()
    K, n = gen.shape[:2]
    counts, sums = R.restate(gen.reshape(-1, 3), z, [0, n], K, bonds)
    for k, name in enumerate(names):
        assert counts[0, k].tolist() == want[k].tolist(), (name, counts[0, k].tolist())
    # the yardstick of the device tests holds valid and invalid samples of both graphs
    chk = ev.assemble_ensemble_check(counts[0].numpy(), sums[0].numpy(), n, int((z != 1).sum()))
    assert chk.valid_all.any() and (~chk.valid_all).any() and chk.valid_heavy.any() and (~chk.valid_heavy).any()
    assert (chk.valid_heavy & ~chk.valid_all).any()                 # the H-H contact: all-atom counts only
    # the threshold pair: exactly on it a bond, one ulp above it none
    at, above = names.index("at_thr"), names.index("above_thr")
    thr = np.float32(float(ev.bond_thresholds([1, 6])[1, 1]))
    c11, c12 = R.alkane()[3][11:13]
    sq = lambda x: np.float32(np.float32(np.float32(x[0] * x[0]) + np.float32(x[1] * x[1])) + np.float32(x[2] * x[2]))
    assert sq(gen[at, c12] - gen[at, c11]) == thr
    assert sq(gen[above, c12] - gen[above, c11]) == np.nextafter(thr, np.float32(np.inf), dtype=np.float32)
    # pair sums: symmetric, zero diagonal, and the stretched sample is 50 tail atoms x 0.25 A^2 from the valid one
    s = sums[0].numpy()
    assert np.array_equal(s, s.transpose(1, 0, 2)) and not s[np.arange(K), np.arange(K)].any()
    moved = n - R.alkane()[3][12]
    assert s[0, 1, 0] == pytest.approx(0.25 * moved, rel=1e-6)


def test_assemble_ensemble_check_on_literal_inputs():
    counts = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 2, 0, 1]])
    sums = np.zeros((3, 3, 2))
    sums[0, 1] = sums[1, 0] = (16.0, 2.0)
    sums[0, 2] = sums[2, 0] = (4.0, 8.0)
    sums[1, 2] = sums[2, 1] = (36.0, 18.0)
    chk = ev.assemble_ensemble_check(counts, sums, n_atoms=4, n_heavy=2)
    assert chk.valid_all.tolist() == [True, False, False] and chk.valid_heavy.tolist() == [True, True, False]
    assert chk.valid_all.dtype == bool and chk.missing_all.tolist() == [0, 1, 0] and chk.extra_all.tolist() == [0, 0, 2]
    assert chk.missing_heavy.tolist() == [0, 0, 0] and chk.extra_heavy.tolist() == [0, 0, 1]
    assert chk.pair_rmsd_all.tolist() == [[0, 2, 1], [2, 0, 3], [1, 3, 0]]
    assert chk.pair_rmsd_heavy.tolist() == [[0, 1, 2], [1, 0, 3], [2, 3, 0]]
    assert chk.diversity_all == 2.0 and chk.diversity_heavy == 2.0
    one = ev.assemble_ensemble_check(np.zeros((1, 4)), np.zeros((1, 1, 2)), 4, 2)
    assert np.isnan(one.diversity_all) and np.isnan(one.diversity_heavy) and one.valid_all.tolist() == [True]
    no_heavy = ev.assemble_ensemble_check(counts[:2], sums[:2, :2] * (1.0, 0.0), n_atoms=4, n_heavy=0)
    assert no_heavy.diversity_all == 2.0 and np.isnan(no_heavy.diversity_heavy)


def test_bond_list_validation():
    sizes = [4, 3]
    b, ptr = ev.validate_bonds([[0, 1], [1, 3]], [4, 4])
    assert b.tolist() == [[0, 1], [1, 3]] * 2 and ptr.tolist() == [0, 2, 4] and b.dtype == np.int32
    b, ptr = ev.validate_bonds(np.zeros((0, 2)), sizes)
    assert b.shape == (0, 2) and ptr.tolist() == [0, 0, 0]
    b, ptr = ev.validate_bonds([[0, 3], [0, 2]], sizes, bond_ptr=[0, 1, 2])
    assert ptr.tolist() == [0, 1, 2] and b.tolist() == [[0, 3], [0, 2]]
    for bad in ([[0, 1], [0, 1]], [[1, 0]], [[2, 2]], [[0, 4]], [[-1, 2]]):
        with pytest.raises(ValueError):
            ev.validate_bonds(bad, [4])
    with pytest.raises(ValueError):
        ev.validate_bonds([[0, 3]], sizes)                          # atom 3 is outside the 3-atom frame
    with pytest.raises(ValueError):
        ev.validate_bonds([[0, 3], [0, 1]], sizes, bond_ptr=[0, 1, 2, 2])
    # the same pair in two frames is no duplicate
    ev.validate_bonds([[0, 1], [0, 1]], sizes, bond_ptr=[0, 1, 2])
    assert bm.canonical_bonds([[3, 1], [1, 3], [0, 2]]).tolist() == [[0, 2], [1, 3]]


def _run_dir(tmp_path, **over):
    params = {"n_basis": 32, "n_rbf": 8, "atom_cutoff": 8.5, "cg_cutoff": 9.5, "enc_nconv": 2, "dec_nconv": 2, "n_cgs": 2,
              "activation": "swish", "det": False, "invariantdec": False, "cg_mp": False, "cg_radius_graph": False,
              "mapping": [0, 0, 0, 1, 1], **over}
    d = tmp_path / "run"
    d.mkdir()
    (d / "modelparams.json").write_text(json.dumps(params))
    return d


def test_parser_surface():
    p = bm.build_parser()
    a = p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz".split())
    assert (a.model, a.cg, a.traj, a.top, a.n_samples, a.out) == ("D", "c.npz", None, None, 4, "o.npz")
    assert (a.frames_per_launch, a.seed, a.pair_rmsd, a.require_valid, a.max_rounds) == (8, 0, False, None, 4)
    a = p.parse_args("-model D -traj t.npz -top top.npz -n_samples 2 -out o.npz -frames_per_launch 3 -seed 9 --pair_rmsd "
                     "--require_valid heavy -max_rounds 2".split())
    assert (a.traj, a.top, a.frames_per_launch, a.seed, a.pair_rmsd, a.require_valid, a.max_rounds) == \
        ("t.npz", "top.npz", 3, 9, True, "heavy", 2)
    for bad in ("-model D -n_samples 4 -out o.npz", "-model D -cg a -traj b -n_samples 4 -out o.npz",
                "-model D -cg a -n_samples 4 -out o.npz --require_valid some", "-cg a -n_samples 4 -out o.npz"):
        with pytest.raises(SystemExit):
            p.parse_args(bad.split())


def test_input_files_are_checked_against_the_run(tmp_path):
    d = _run_dir(tmp_path)
    params = bm.read_params(str(d))
    p = bm.build_parser()
    cg = tmp_path / "cg.npz"
    np.savez(cg, cg_xyz=np.zeros((3, 2, 3), np.float32))
    top = tmp_path / "top.npz"
    np.savez(top, z=np.array([6, 1, 1, 6, 1]), bonds=np.array([[1, 0], [0, 2], [0, 3], [3, 4]]))
    inp = bm.read_inputs(p.parse_args(f"-model {d} -cg {cg} -top {top} -n_samples 2 -out o".split()), params)
    assert inp["cg_xyz"].shape == (3, 2, 3) and inp["bonds"].tolist() == [[0, 1], [0, 2], [0, 3], [3, 4]]
    assert bm.read_inputs(p.parse_args(f"-model {d} -cg {cg} -n_samples 2 -out o".split()), params)["bonds"] is None
    with pytest.raises(SystemExit, match="topology"):                # nothing to be valid against
        bm.read_inputs(p.parse_args(f"-model {d} -cg {cg} -n_samples 2 -out o --require_valid all".split()), params)
    with pytest.raises(SystemExit, match="no such file"):
        bm.read_inputs(p.parse_args(f"-model {d} -cg {tmp_path / 'none.npz'} -n_samples 2 -out o".split()), params)
    with pytest.raises(SystemExit, match="missing"):
        bm.read_inputs(p.parse_args(f"-model {d} -cg {top} -n_samples 2 -out o".split()), params)
    wrong = tmp_path / "wrong.npz"
    np.savez(wrong, cg_xyz=np.zeros((3, 4, 3), np.float32))
    with pytest.raises(SystemExit, match="beads"):
        bm.read_inputs(p.parse_args(f"-model {d} -cg {wrong} -n_samples 2 -out o".split()), params)
    big = tmp_path / "big.npz"
    np.savez(big, z=np.array([6, 1, 1, 6, 1, 1]), bonds=np.array([[0, 1]]))
    with pytest.raises(SystemExit, match="6 atoms"):                 # a topology of another molecule
        bm.read_inputs(p.parse_args(f"-model {d} -cg {cg} -top {big} -n_samples 2 -out o".split()), params)
    with pytest.raises(ValueError, match="atoms"):
        bm.check_topology(params["mapping"], z=np.ones(6))


def test_load_run_refuses_a_det_run_and_a_directory_without_a_run(tmp_path):
    d = _run_dir(tmp_path, det=True)
    with pytest.raises(ValueError, match="no prior"):
        bm.load_run(str(d), device="cpu")
    with pytest.raises(FileNotFoundError):
        bm.load_run(str(tmp_path / "nowhere"), device="cpu")
