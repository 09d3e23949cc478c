"""Hydrogen bonds on the device: K25 (csrc/hbond.hip) against the numpy restatement.  A pair is bonded by three strict
comparisons of fp32 values that both sides round identically: every comparison here is integer EQUALITY, on every output of
the kernel, ``bits`` included."""
import functools
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, hbonds
import density_restatement as DR
import hbonds_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUTPUTS = ("pair_counts", "n_hbonds", "n_native", "bad", "bits")
ELEMENTS = dict(donor_elements=R.DONORS, acceptor_elements=R.ACCEPTORS)


def _tables(z, bonds, elements=ELEMENTS, excluded=None):
    don_h, don_d, acc = hbonds.donors_acceptors(z, bonds, **elements)
    return don_h, don_d, acc, hbonds.excluded_pairs(don_d, acc, bonds, excluded)


def _want(xyz, z, bonds, elements=ELEMENTS, excluded=None, native=None, h_a_cutoff=2.5, angle=120.0):
    don_h, don_d, acc, excl = _tables(z, bonds, elements, excluded)
    want = R.hbond_counts(xyz, don_h, don_d, acc, excl, native, h_a_cutoff, angle)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want


def _same(got, want, what=""):
    assert got["n_good"] == want["n_good"], what
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _check(xyz, z, bonds, elements=ELEMENTS, want=None, what="", excluded=None, native=None, h_a_cutoff=2.5, angle=120.0, **kw):
    got = hbonds.hbond_counts(xyz, z, bonds, excluded=excluded, native=native, h_a_cutoff=h_a_cutoff, angle=angle, per_pair=True,
                              device=DEV, **elements, **kw)
    _same(got, _want(xyz, z, bonds, elements, excluded, native, h_a_cutoff, angle) if want is None else want, what)
    return got


def _fraction(want, excl):
    """Bonded pairs over the pairs that count, over the good structures."""
    return want["bonds"].sum() / float(max(want["n_good"], 1) * (~excl).sum())


@functools.lru_cache(maxsize=None)
def _cloud(nH, nA, S, sigma=1.0, n_excluded=5, seed=0):
    """A molecule with an ``nH x nA`` table in ``S`` random structures, and the restatement's result.  The spread is
    chosen so that the restatement bonds between 2 % and 60 % of the pairs that count: a case with no bond, or with
    nothing but bonds, proves nothing."""
    z, bonds = R.molecule(nH, nA, n_excluded=n_excluded)
    xyz = R.cloud(z, bonds, S, sigma, np.random.default_rng(1000 * nH + 10 * nA + S + seed))
    want = _want(xyz, z, bonds)
    excl = _tables(z, bonds)[3]
    assert 0.02 <= _fraction(want, excl) <= 0.60, (nH, nA, S, _fraction(want, excl))
    return xyz, z, bonds, want


def _single(D, H, A):
    """One N-H donor and one O acceptor: z, bonds, and a structure ``[1, 3, 3]`` in the order H, N, O."""
    return np.array([[H, D, A]], dtype=np.float32)


Z1, B1 = R.molecule(1, 1)


# ----------------------------------------------------------------------------- one pair
def test_one_donor_one_acceptor_one_structure():
    for distance, theta, bonded in ((1.9, 180.0, 1), (2.6, 180.0, 0), (1.9, 110.0, 0), (1.9, 130.0, 1)):
        got = _check(_single(*R.triple(distance, theta)), Z1, B1, what=(distance, theta))
        assert got["pair_counts"].tolist() == [[bonded]] and got["n_hbonds"].tolist() == [bonded]
        assert got["bits"].tolist() == [[[bonded]]] and got["n_native"].tolist() == [0]
    for angle, theta, bonded in ((90.0, 91.0, 1), (90.0, 89.0, 0), (179.9, 179.0, 0), (179.9, 179.99, 1)):
        got = _check(_single(*R.triple(1.9, theta)), Z1, B1, angle=angle, what=(angle, theta))
        assert got["n_hbonds"].tolist() == [bonded]


@pytest.mark.parametrize("shift", [0.0, 500.0])
def test_a_pair_within_two_ulps_of_the_distance_threshold(shift):
    """A linear triple with H...A at the cutoff along each axis, the acceptor's coordinate moved by -2 .. +2 ulps."""
    xyz = []
    for axis in range(3):
        for ulps in range(-2, 3):
            H = np.full(3, shift, dtype=np.float32)
            D, A = H.copy(), H.copy()
            D[axis] -= np.float32(1.0)
            A[axis] += np.float32(2.5)
            for _ in range(abs(ulps)):
                A[axis] = np.nextafter(A[axis], np.float32(np.inf if ulps > 0 else -np.inf))
            xyz.append([H, D, A])
    xyz = np.array(xyz, dtype=np.float32)
    got = _check(xyz, Z1, B1, what=shift)
    assert 0 < got["n_hbonds"].sum() < len(xyz)                # the sweep crosses the threshold


@pytest.mark.parametrize("angle", [120.0, 135.0])
def test_a_triple_swept_across_the_angle_threshold_in_one_ulp_steps(angle):
    D, H, A = (v.astype(np.float32) for v in R.triple(2.0, angle))
    xyz = []
    y = A[1]
    for _ in range(40):
        y = np.nextafter(y, np.float32(-np.inf))
    for _ in range(81):
        xyz.append([H, D, np.array([A[0], y, A[2]], dtype=np.float32)])
        y = np.nextafter(y, np.float32(np.inf))
    xyz = np.array(xyz, dtype=np.float32)
    got = _check(xyz, Z1, B1, angle=angle, what=angle)
    assert 0 < got["n_hbonds"].sum() < len(xyz)                # the sweep crosses the threshold


# ----------------------------------------------------------------------------- random clouds
def test_a_one_by_one_table_in_three_structures():
    xyz = R.cloud(Z1, B1, 3, 1.5, np.random.default_rng(10))
    want = _want(xyz, Z1, B1)
    assert want["n_hbonds"].sum() == 1                         # one structure of three is bonded: 33 %
    _check(xyz, Z1, B1, want=want)


@pytest.mark.parametrize("nH,nA", [(31, 63), (32, 64), (33, 65), (65, 129)])
def test_random_clouds_around_the_tile_sizes(nH, nA):
    xyz, z, bonds, want = _cloud(nH, nA, 3)
    _check(xyz, z, bonds, want=want, what=(nH, nA))


def test_the_kernels_own_row_tile_and_chunk_boundaries():
    lib = _lib.load()
    rows, chunk = int(lib.cgv_hbond_row_tile()), int(lib.cgv_hbond_chunk())
    for nH, S in ((rows - 1, chunk + 1), (rows, chunk), (rows + 1, chunk - 1), (2 * rows + 1, 2 * chunk + 1)):
        xyz, z, bonds, want = _cloud(nH, 66, S)
        _check(xyz, z, bonds, want=want, what=(nH, S))


def test_more_structures_than_slices_times_chunk_and_cuts_of_the_structure_axis():
    S = 1100                                                   # no multiple of the chunk; several chunks per slice
    xyz, z, bonds, want = _cloud(8, 8, S, n_excluded=3)
    first = _check(xyz, z, bonds, want=want)
    again = _check(xyz, z, bonds, want=want)                   # two calls give identical arrays
    for k in OUTPUTS:
        assert np.array_equal(first[k], again[k]), k
    _check(xyz, z, bonds, want=want, structures_per_launch=7, what="launches of 7")
    few = xyz[:37]
    want_few = _want(few, z, bonds)
    for per in (37, 7, 1):
        _check(few, z, bonds, want=want_few, structures_per_launch=per, what=per)


# ----------------------------------------------------------------------------- bad structures
def test_structures_with_a_nan_in_a_table_atom_are_bad_and_the_rest_unchanged():
    xyz, z, bonds, clean = _cloud(33, 65, 9)
    don_h, don_d, acc, _ = _tables(z, bonds)
    broken = np.array(xyz)
    broken[0, don_d[5], 0] = np.nan
    broken[4, don_h[32], 1] = np.inf
    broken[8, acc[64], 2] = -np.inf
    got = _check(broken, z, bonds, what="NaN")
    assert got["bad"].tolist() == [True, False, False, False, True, False, False, False, True] and got["n_good"] == 6
    assert (got["n_hbonds"][[0, 4, 8]] == -1).all() and (got["n_native"][[0, 4, 8]] == -1).all() and not got["bits"][[0, 4, 8]].any()
    keep = [1, 2, 3, 5, 6, 7]
    assert np.array_equal(got["bits"][keep], clean["bits"][keep]) and np.array_equal(got["n_hbonds"][keep], clean["n_hbonds"][keep])
    assert np.array_equal(got["pair_counts"], clean["bonds"][keep].sum(axis=0))


def test_a_nan_in_an_atom_of_no_table_is_not_bad():
    z, bonds = R.molecule(9, 20, n_excluded=2)
    z, bonds = np.concatenate([z, [6, 1]]), np.concatenate([bonds, [[len(z), len(z) + 1]]])       # a C-H nobody asks about
    xyz = R.cloud(z, bonds, 4, 1.0, np.random.default_rng(5))
    xyz[1, -2] = np.nan
    xyz[2, -1] = np.inf
    got = _check(xyz, z, bonds)
    assert not got["bad"].any() and got["n_good"] == 4 and got["pair_counts"].sum() > 0


# ----------------------------------------------------------------------------- masks
def test_native_counts_are_the_popcount_of_bits_and_native():
    xyz, z, bonds, want = _cloud(33, 65, 9)
    rng = np.random.default_rng(2)
    native = rng.random((33, 65)) < 0.5
    got = _check(xyz, z, bonds, native=native)
    assert np.array_equal(got["n_native"], R.popcount(got["bits"] & hbonds.pack_mask(native)[None]).sum(axis=1))
    assert 0 < got["n_native"].sum() < got["n_hbonds"].sum()
    pairs = [(int(h), int(a)) for h, a in np.argwhere(native)]
    _check(xyz, z, bonds, native=pairs, want=_want(xyz, z, bonds, native=native), what="native as a list of pairs")
    none = _check(xyz, z, bonds, want=want)
    assert not none["n_native"].any()


def test_an_exclusion_removes_a_pair_that_would_bond():
    xyz, z, bonds, want = _cloud(33, 65, 9)
    h, a = (int(v) for v in np.argwhere(want["pair_counts"] == want["pair_counts"].max())[0])
    assert want["pair_counts"][h, a] > 0
    got = _check(xyz, z, bonds, excluded=[(h, a)])
    assert got["pair_counts"][h, a] == 0 and not ((got["bits"][:, h, a >> 6] >> np.uint64(a & 63)) & np.uint64(1)).any()
    assert got["n_hbonds"].sum() == want["n_hbonds"].sum() - want["pair_counts"][h, a]
    assert got["excluded"][h, a] and got["excluded"].sum() == 6


def test_bits_past_the_last_acceptor_are_zero():
    xyz, z, bonds, _ = _cloud(33, 65, 9)
    got = hbonds.hbond_counts(xyz, z, bonds, per_pair=True, device=DEV, **ELEMENTS)
    assert got["bits"].shape == (9, 33, 2) and not (got["bits"][:, :, 1] >> np.uint64(1)).any()
    assert got["bits"][:, :, 1].any()                          # acceptor 64 is bonded somewhere


# ----------------------------------------------------------------------------- limits
def test_tables_at_the_limits():
    lim = hbonds.limits()
    for nH, nA, sigma in ((lim["hydrogens"], 3, 4.0), (3, lim["acceptors"], 4.0)):
        z, bonds = R.molecule(nH, nA, n_excluded=2)
        xyz = R.cloud(z, bonds, 1, sigma, np.random.default_rng(nH))
        got = _check(xyz, z, bonds, what=(nH, nA))
        assert got["pair_counts"].sum() > 0
    for nH, nA in ((lim["hydrogens"] + 1, 3), (3, lim["acceptors"] + 1)):
        z, bonds = R.molecule(nH, nA)
        with pytest.raises(ValueError, match="the kernel holds"):
            hbonds.hbond_counts(np.zeros((1, z.shape[0], 3), np.float32), z, bonds, device=DEV, **ELEMENTS)


# ----------------------------------------------------------------------------- end to end on a peptide
CLOSED = [180.0, -131.8, -64.2, 180.0, -86.7, 64.8, 180.0, 43.4, 7.6, 180.0]         # a gamma turn: N-H of residue 3 to O=C of residue 1
OPEN = [180.0] * 10                                                                # the extended chain


def _peptide(torsion_sets):
    """The three-residue peptide of ``density_restatement`` with an amide hydrogen on every N (1.0 Angstrom along the
    bisector that points away from its two neighbours): ``(z, bonds, xyz [S, n, 3])``."""
    z, bonds = DR.peptide(3)
    x = DR.peptide_structures(3, np.radians(torsion_sets)).astype(np.float64)
    nbrs = hbonds.adjacency(len(z), bonds)
    zs, bs, hs = z.tolist(), bonds.tolist(), []
    for N in np.flatnonzero(z == 7).tolist():
        a, b = nbrs[N]
        u, v = x[:, a] - x[:, N], x[:, b] - x[:, N]
        w = -(u / np.linalg.norm(u, axis=1, keepdims=True) + v / np.linalg.norm(v, axis=1, keepdims=True))
        hs.append(x[:, N] + w / np.linalg.norm(w, axis=1, keepdims=True))
        bs.append([N, len(zs)])
        zs.append(1)
    return np.array(zs), np.array(bs), np.concatenate([x, np.stack(hs, axis=1)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ensembles():
    rng = np.random.default_rng(11)
    jitter = lambda t, S: np.asarray(t)[None, :] + rng.normal(0.0, 1.0, (S, 10))         # a degree of noise
    z, bonds, closed = _peptide(jitter(CLOSED, 12))
    _, _, opened = _peptide(jitter(OPEN, 10))
    return z, bonds, closed, opened


def test_a_peptide_that_loses_its_backbone_hydrogen_bond(tmp_path, capsys):
    z, bonds, closed, opened = _ensembles()
    don_h, don_d, acc, excl = _tables(z, bonds, {})
    want_closed, want_open = _want(closed, z, bonds, {}), _want(opened, z, bonds, {})
    D, H, A = 11, 19, 6                                        # N of residue 3, its H, the carbonyl O of residue 1
    h, a = int(np.flatnonzero(don_h == H)[0]), int(np.flatnonzero(acc == A)[0])
    assert don_d[h] == D and z[D] == 7 and z[A] == 8
    assert want_closed["pair_counts"][h, a] == 12 and want_open["n_hbonds"].sum() == 0       # the restatement says which is which
    _check(closed, z, bonds, {}, want=want_closed)
    _check(opened, z, bonds, {}, want=want_open)
    stats = hbonds.compare(closed, opened, z, bonds, device=DEV)
    assert set(stats) == set(hbonds.HBOND_STATS_KEYS)
    assert [D, H, A] in stats["native"] and [D, H, A] in stats["missing"] and stats["spurious"] == []
    assert stats["kept_ref"] == 1.0 and stats["kept_gen"] < 1.0 and stats["occupancy_rmse"] > 0
    ref_map, gen_map = np.array(stats["backbone_ref"]), np.array(stats["backbone_gen"])
    assert ref_map.shape == (3, 3) and ref_map[2, 0] == 1.0 and ref_map.sum() == 1.0 and gen_map.shape == (3, 3) and not gen_map.any()
    same = hbonds.compare(closed, closed, z, bonds, device=DEV)
    assert same["occupancy_rmse"] == 0.0 and same["kept_ref"] == same["kept_gen"] and same["missing"] == []
    assert same["occupancy_pearson"] == pytest.approx(1.0)
    # the command line on the same files
    np.savez(tmp_path / "ref.npz", xyz=closed, z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=opened.reshape(5, 2, -1, 3))
    out, bits = tmp_path / "stats.json", tmp_path / "bits.npz"
    capsys.readouterr()
    hbonds.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -out {out} -bits {bits} -device {DEV}".split())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["out"] == str(out) and line["hbond_stats"] == json.loads(json.dumps(hbonds.summary_of(stats)))
    with open(out) as f:
        written = json.load(f)
    assert set(written) == set(hbonds.HBOND_STATS_KEYS) and written["missing"] == stats["missing"]
    with np.load(bits) as f:
        assert np.array_equal(f["bits"], want_open["bits"]) and f["don_h"].tolist() == don_h.tolist()
