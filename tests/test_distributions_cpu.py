"""Distribution statistics without a GPU: the fp64 restatement of K15 on geometries with known answers, the feature tables
from the bond graph, the backbone torsions from elements and connectivity, the Jensen-Shannon divergence, and the C ABI's
declarations."""
import ctypes
import json
import math

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, backmap as bm, distributions as D
import internal_coords_restatement as R


# ----------------------------------------------------------------------------- the restatement on known geometries
def _four(deg):
    """Four hand-placed atoms: p1 at the origin, p2 = (0, 0, 1.5) (the central bond along +z), p0 = (1, 0, 0) and
    p3 = (cos a, sin a, 1.5).  By hand: b1 = (-1,0,0), b2 = (0,0,1.5), b3 = (cos a, sin a, 0); b2 x b3 = 1.5 (-sin a, cos a, 0),
    b1 x b2 = (0, 1.5, 0); y = |b2| b1 . (b2 x b3) = 2.25 sin a, x = (b1 x b2) . (b2 x b3) = 2.25 cos a: the torsion is +a.
    Looking along the central bond from p1 to p2, p3 is then rotated CLOCKWISE from p0 for a > 0 -- the IUPAC sign, which
    is mdtraj's."""
    a = math.radians(deg)
    return np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [math.cos(a), math.sin(a), 1.5]])


@pytest.mark.parametrize("deg", [60.0, -60.0, 180.0])
def test_restated_torsion_has_the_mdtraj_sign(deg):
    x = _four(deg)
    got = R.value(x, (0, 1, 2, 3), R.TORSION)
    if deg == 180.0:
        assert abs(got) == pytest.approx(math.pi, abs=1e-12)                    # +pi or -pi: one bin (below)
    else:
        assert got == pytest.approx(math.radians(deg), abs=1e-12)
        assert R.value(x, (3, 2, 1, 0), R.TORSION) == pytest.approx(got, abs=1e-12)    # read backwards: the same torsion
        assert R.value(x * [1, -1, 1], (0, 1, 2, 3), R.TORSION) == pytest.approx(-got, abs=1e-12)   # the mirror image


def test_restated_torsions_land_in_their_bins():
    # 36 bins of 10 degrees over [-180, 180): 65 -> bin 24, -55 -> bin 12 (half a bin off the edges at +-60)
    for deg, want_bin in ((65.0, 24), (-55.0, 12)):
        assert R.slot(R.value(_four(deg), (0, 1, 2, 3), R.TORSION), R.TORSION, 36, (0.5, 2.5)) == 1 + want_bin
    assert R.slot(R.value(_four(180.0), (0, 1, 2, 3), R.TORSION), R.TORSION, 36, (0.5, 2.5)) in (1, 36)
    assert R.slot(math.pi, R.TORSION, 36, (0.5, 2.5)) == 1                      # exactly pi: bin 0 (periodic)
    assert R.slot(-math.pi, R.TORSION, 36, (0.5, 2.5)) == 1
    assert R.slot(math.pi - 1e-9, R.TORSION, 36, (0.5, 2.5)) == 36              # just below pi: the last bin


def test_restated_right_angle_bond_and_their_bins():
    x = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [1.5, 0.0, 0.0]])
    assert R.value(x, (0, 1, 2, 0), R.ANGLE) == pytest.approx(math.pi / 2, abs=1e-15)
    assert R.value(x, (1, 3, 0, 0), R.BOND) == 1.5
    assert R.slot(math.pi / 2 + 1e-6, R.ANGLE, 36, (0.5, 2.5)) == 1 + 18 and R.slot(math.pi, R.ANGLE, 36, (0.5, 2.5)) == 36
    assert R.slot(0.0, R.ANGLE, 36, (0.5, 2.5)) == 1
    # bonds over [0.5, 2.5) in 20 bins of 0.1: 1.5 -> bin 10; under, over, the closed lower and open upper end
    assert R.slot(1.5 + 1e-9, R.BOND, 20, (0.5, 2.5)) == 1 + 10
    assert R.slot(0.5, R.BOND, 20, (0.5, 2.5)) == 1 and R.slot(0.4999, R.BOND, 20, (0.5, 2.5)) == 0
    assert R.slot(2.5, R.BOND, 20, (0.5, 2.5)) == 21 and R.slot(np.nextafter(2.5, 0), R.BOND, 20, (0.5, 2.5)) == 20
    bad = x.copy()
    bad[3, 1] = np.nan
    assert R.value(bad, (1, 3, 0, 0), R.BOND) is None and R.slot(None, R.BOND, 20, (0.5, 2.5)) == 22
    counts, pair_counts = R.restate(np.stack([x, bad]), [(1, 3, 0, 0), (0, 1, 2, 0)], [R.BOND, R.ANGLE], [], 20, 4, (0.5, 2.5))
    assert counts[0, 11] == 1 and counts[0, 22] == 1 and counts[1, 1 + 10] == 2 and counts.sum() == 4
    assert pair_counts.shape == (0, 4, 4)


# ----------------------------------------------------------------------------- feature tables
def _check_table(c, z, bonds):
    n = len(z)
    adj = np.zeros((n, n), bool)
    adj[bonds[:, 0], bonds[:, 1]] = adj[bonds[:, 1], bonds[:, 0]] = True
    deg = adj.sum(1)
    rows = [(int(k),) + c.atoms(f) for f, k in enumerate(c.kind)]
    assert len(set(rows)) == len(rows)
    nb = sum(1 for r in rows if r[0] == D.BOND)
    na = sum(1 for r in rows if r[0] == D.ANGLE)
    nt = sum(1 for r in rows if r[0] == D.TORSION)
    assert nb == len(bonds) and na == int((deg * (deg - 1) // 2).sum())
    assert nt == sum(int((deg[i] - 1) * (deg[j] - 1)) for i, j in bonds)            # acyclic: no i == l to leave out
    for r in rows:
        a = r[1:]
        assert all(adj[a[t], a[t + 1]] for t in range(len(a) - 1)) and len(set(a)) == len(a)
        if r[0] == D.BOND:
            assert a[0] < a[1]
        elif r[0] == D.ANGLE:
            assert a[0] < a[2]
        else:
            assert a[1] < a[2]
    assert c.feat.dtype == np.int32 and c.kind.dtype == np.int32 and c.feat.shape == (len(rows), 4) and c.n_atoms == n
    return nb, na, nt


def test_internal_coords_and_backbone_torsions_of_alanine_dipeptide():
    c = D.internal_coords(R.ALA_Z, R.ALA_BONDS)
    # torsions by hand, (deg - 1)(deg - 1) per bond: CH3-C 6, C-N 4, N-CA 6, CA-CB 9, CA-C 6, C-N 4, N-CH3 6
    assert _check_table(c, R.ALA_Z, R.ALA_BONDS) == (21, 36, 41)
    heavy = D.internal_coords(R.ALA_Z, R.ALA_BONDS, "heavy")
    assert all(R.ALA_Z[a] != 1 for f in range(heavy.n_features) for a in heavy.atoms(f))
    assert [int((heavy.kind == k).sum()) for k in (2, 3, 4)] == [9, 11, 10]
    assert {(int(k),) + heavy.atoms(f) for f, k in enumerate(heavy.kind)} <= {(int(k),) + c.atoms(f) for f, k in enumerate(c.kind)}
    phi, psi, pairs = D.peptide_backbone_torsions(R.ALA_Z, R.ALA_BONDS)
    assert phi == [R.ALA_PHI] and psi == [R.ALA_PSI] and pairs == [(0, 0)]
    with_pairs, rows = D.backbone_pairs(c, R.ALA_Z, R.ALA_BONDS)
    assert len(rows) == 1 and c.atoms(rows[0][0]) == R.ALA_PHI and c.atoms(rows[0][1]) == R.ALA_PSI
    assert with_pairs.pairs.tolist() == [list(rows[0])] and with_pairs.pairs.dtype == np.int32
    # bonds in either orientation and listed twice: the same table
    again = D.internal_coords(R.ALA_Z, np.concatenate([R.ALA_BONDS[:, ::-1], R.ALA_BONDS[:5]]))
    assert np.array_equal(again.feat, c.feat) and np.array_equal(again.kind, c.kind)
    with pytest.raises(ValueError):
        D.internal_coords(R.ALA_Z, R.ALA_BONDS, "backbone")


def test_backbone_torsions_of_capped_glycine_and_of_a_relabelled_molecule():
    c = D.internal_coords(R.GLY_Z, R.GLY_BONDS)
    assert _check_table(c, R.GLY_Z, R.GLY_BONDS)[0] == 18
    phi, psi, pairs = D.peptide_backbone_torsions(R.GLY_Z, R.GLY_BONDS)
    assert phi == [R.GLY_PHI] and psi == [R.GLY_PSI] and pairs == [(0, 0)]
    # atom order is no input: a permuted alanine dipeptide gives the permuted torsions
    perm = np.random.default_rng(0).permutation(22)                 # new index of old atom a: perm[a]
    z = np.empty(22, int)
    z[perm] = R.ALA_Z
    phi, psi, pairs = D.peptide_backbone_torsions(z, perm[R.ALA_BONDS])
    assert phi == [tuple(perm[list(R.ALA_PHI)])] and psi == [tuple(perm[list(R.ALA_PSI)])] and pairs == [(0, 0)]
    coords, rows = D.backbone_pairs(D.internal_coords(z, perm[R.ALA_BONDS]), z, perm[R.ALA_BONDS])
    assert len(rows) == 1 and coords.atoms(rows[0][0]) in (phi[0], phi[0][::-1])


def test_backbone_torsions_of_a_hydrocarbon_are_empty():
    z, bonds = R.branched_chain(30, seed=1)
    assert D.peptide_backbone_torsions(z, bonds) == ([], [], [])
    coords, rows = D.backbone_pairs(D.internal_coords(z, bonds), z, bonds)
    assert rows == [] and coords.pairs.shape == (0, 2)
    _check_table(coords, z, bonds)


# ----------------------------------------------------------------------------- JSD
def test_js_divergence_properties():
    a = np.array([5, 0, 3, 2, 0, 0])
    b = np.array([0, 4, 0, 0, 7, 0])
    c = np.array([1, 1, 6, 0, 2, 0])
    assert D.js_divergence(a, a) == 0.0 and D.js_divergence(a, 3 * a) == 0.0
    assert D.js_divergence(a, b) == pytest.approx(1.0, abs=1e-15)
    assert D.js_divergence(a, c) == D.js_divergence(c, a) and 0.0 < D.js_divergence(a, c) < 1.0
    # by hand: p = (1/2, 1/2), q = (1, 0): m = (3/4, 1/4); JSD = (1/2)[(1/2)log2(2/3) + (1/2)log2(2)] + (1/2) log2(4/3)
    want = 0.5 * (0.5 * math.log2(2 / 3) + 0.5 * math.log2(2)) + 0.5 * math.log2(4 / 3)
    assert D.js_divergence([1, 1], [2, 0]) == pytest.approx(want, abs=1e-15)
    assert D.js_divergence(np.zeros(6, int), a) is None and D.js_divergence(a, np.zeros(6, int)) is None
    assert D.js_divergence(np.zeros((3, 3), int), np.zeros((3, 3), int)) is None
    assert D.js_divergence(np.eye(3, dtype=int), np.eye(3, dtype=int)) == 0.0                   # a pair's 2-D map
    with pytest.raises(ValueError):
        D.js_divergence(a, a[:5])
    row = np.array([7, 1, 2, 3, 9, 4])                                                          # under, 3 bins, over, invalid
    assert D.outside(row) == {"under": 7, "over": 9, "invalid": 4} and row[1:-2].tolist() == [1, 2, 3]


# ----------------------------------------------------------------------------- the C ABI
def test_k15_is_declared_in_the_header_and_the_prototypes_and_its_limits_are_sane():
    names = ["cgv_internal_hist", "cgv_internal_hist_max_features", "cgv_internal_hist_max_pairs", "cgv_internal_hist_max_bins",
             "cgv_internal_hist_max_bins2", "cgv_internal_hist_max_atoms", "cgv_internal_hist_max_staged_atoms",
             "cgv_internal_hist_feature_tile", "cgv_internal_hist_pair_tile"]
    declared = _lib.header_symbols()
    lib = _lib.load()
    for name in names:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
    lim = D.limits()
    assert lim["features"] >= 4096 and lim["pairs"] >= 256 and lim["bins"] >= 360 and lim["bins2"] >= 36
    assert 166 <= lim["staged_atoms"] < lim["atoms"]
    for nb in (1, 7, 36, lim["bins"]):
        assert 1 <= lib.cgv_internal_hist_feature_tile(nb) <= 256
    for nb2 in (1, 5, 36, lim["bins2"]):
        assert lib.cgv_internal_hist_pair_tile(nb2) >= 1
    assert lib.cgv_internal_hist_feature_tile(lim["bins"] + 1) == 0 and lib.cgv_internal_hist_pair_tile(lim["bins2"] + 1) == 0
    # argument errors are reported before any device work (no GPU needed)
    f = ctypes.c_void_p(None)
    assert lib.cgv_internal_hist(f, f, f, f, 1, 1, lim["features"] + 1, 0, 36, 36, 0.5, 2.5, f, f, f) == -1
    assert b"max_features" in lib.cgv_last_error_string()
    assert lib.cgv_internal_hist(f, f, f, f, 1, 1, 1, 0, 36, 36, 2.5, 0.5, f, f, f) == -1
    assert lib.cgv_internal_hist(f, f, f, f, 0, 22, 5, 0, 36, 36, 0.5, 2.5, f, f, f) == 0          # no structures: nothing to do


# ----------------------------------------------------------------------------- the backmap CLI's input checks
def test_dist_stats_reference_is_checked_against_the_topology(tmp_path):
    d = tmp_path / "run"
    d.mkdir()
    (d / "modelparams.json").write_text(json.dumps({"n_cgs": 2, "det": False, "mapping": [0, 0, 0, 1, 1]}))
    params, p = bm.read_params(str(d)), bm.build_parser()
    a = p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz".split())
    assert a.dist_stats is False and a.ref is None
    cg, top, ref = tmp_path / "cg.npz", tmp_path / "top.npz", tmp_path / "ref.npz"
    z, bonds = np.array([6, 1, 1, 6, 1]), np.array([[1, 0], [0, 2], [0, 3], [3, 4]])
    np.savez(cg, cg_xyz=np.zeros((3, 2, 3), np.float32))
    np.savez(top, z=z, bonds=bonds)
    np.savez(ref, xyz=np.zeros((4, 5, 3), np.float32), z=z, bonds=bonds)
    base = f"-model {d} -cg {cg} -n_samples 2 -out o"
    inp = bm.read_inputs(p.parse_args(f"{base} -top {top} --dist_stats -ref {ref}".split()), params)
    assert inp["ref_xyz"].shape == (4, 5, 3) and inp["ref_xyz"].dtype == np.float32
    assert "ref_xyz" not in bm.read_inputs(p.parse_args(f"{base} -top {top}".split()), params)
    with pytest.raises(SystemExit, match="topology"):
        bm.read_inputs(p.parse_args(f"{base} --dist_stats -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="reference frames"):        # bead coordinates alone carry no reference
        bm.read_inputs(p.parse_args(f"{base} -top {top} --dist_stats".split()), params)
    with pytest.raises(SystemExit, match="--dist_stats"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} -ref {ref}".split()), params)
    other = tmp_path / "other.npz"
    np.savez(other, xyz=np.zeros((4, 5, 3), np.float32), z=np.array([6, 1, 1, 7, 1]), bonds=bonds)
    with pytest.raises(SystemExit, match="z differs"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --dist_stats -ref {other}".split()), params)
    np.savez(other, xyz=np.zeros((4, 6, 3), np.float32), z=np.array([6, 1, 1, 6, 1, 1]), bonds=bonds)
    with pytest.raises(SystemExit, match="5 atoms"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --dist_stats -ref {other}".split()), params)
