"""Hydrogen bonds, host side: the tables and masks of ``hbonds``, the numpy restatement of the predicate against
hand-placed triples and against an fp64 ``arccos``, the statistics of ``compare_from_counts`` on hand-made integer tables,
the command line's refusals and every ``ValueError`` -- all without a device."""
import json
import math

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, hbonds
import hbonds_restatement as R

# alanine dipeptide, ACE-ALA-NME: CH3 (0; H 1-3), C (4) = O (5), N (6) - H (7), CA (8; H 9), CB (10; H 11-13), C (14) = O (15),
# N (16) - H (17), CH3 (18; H 19-21)
ALA_Z = np.array([6, 1, 1, 1, 6, 8, 7, 1, 6, 1, 6, 1, 1, 1, 6, 8, 7, 1, 6, 1, 1, 1])
ALA_BONDS = np.array([(0, 1), (0, 2), (0, 3), (0, 4), (4, 5), (4, 6), (6, 7), (6, 8), (8, 9), (8, 10), (10, 11), (10, 12), (10, 13),
                      (8, 14), (14, 15), (14, 16), (16, 17), (16, 18), (18, 19), (18, 20), (18, 21)])


# ----------------------------------------------------------------------------- tables
def test_donors_and_acceptors_of_alanine_dipeptide():
    don_h, don_d, acc = hbonds.donors_acceptors(ALA_Z, ALA_BONDS)
    assert don_h.tolist() == [7, 17] and don_d.tolist() == [6, 16] and acc.tolist() == [5, 6, 15, 16]
    assert all(a.dtype == np.int32 for a in (don_h, don_d, acc))
    excl = hbonds.excluded_pairs(don_d, acc, ALA_BONDS)
    assert excl.tolist() == [[False, True, False, False], [False, False, False, True]]       # A is D itself
    _, _, oxy = hbonds.donors_acceptors(ALA_Z, ALA_BONDS, acceptor_elements=(8,))
    assert oxy.tolist() == [5, 15]


def test_a_hydroxyl_hydrogen_is_a_donor_and_a_c_h_is_not():
    z, bonds = np.array([6, 1, 1, 1, 8, 1]), np.array([(0, 1), (0, 2), (0, 3), (0, 4), (4, 5)])         # methanol
    don_h, don_d, acc = hbonds.donors_acceptors(z, bonds)
    assert don_h.tolist() == [5] and don_d.tolist() == [4] and acc.tolist() == [4]
    assert hbonds.excluded_pairs(don_d, acc, bonds).all()
    with pytest.raises(ValueError, match="no donor hydrogen"):
        hbonds.donors_acceptors(z, bonds, donor_elements=(7,))
    with pytest.raises(ValueError, match="no acceptor"):
        hbonds.donors_acceptors(z, bonds, acceptor_elements=(7,))
    bridging = hbonds.donors_acceptors(np.array([8, 1, 8, 1]), np.array([(0, 1), (1, 2), (2, 3)]))    # H 1 has two heavy neighbours
    assert bridging[0].tolist() == [3]


def test_a_hydrocarbon_is_refused():
    z, bonds = np.array([6, 1, 1, 1, 6, 1, 1, 1]), np.array([(0, 1), (0, 2), (0, 3), (0, 4), (4, 5), (4, 6), (4, 7)])
    with pytest.raises(ValueError, match="no donor hydrogen"):
        hbonds.donors_acceptors(z, bonds)
    with pytest.raises(ValueError, match="no donor hydrogen"):
        hbonds.hbond_counts(np.zeros((2, 8, 3), np.float32), z, bonds)


def test_the_acceptor_bonded_to_the_donor_is_excluded():
    z, bonds = np.array([1, 7, 8, 8]), np.array([(0, 1), (1, 2)])                  # H-N-O and a lone O
    don_h, don_d, acc = hbonds.donors_acceptors(z, bonds)
    assert acc.tolist() == [1, 2, 3]
    assert hbonds.excluded_pairs(don_d, acc, bonds).tolist() == [[True, True, False]]
    assert hbonds.excluded_pairs(don_d, acc, bonds, extra=[(0, 2)]).tolist() == [[True, True, True]]
    assert hbonds.excluded_pairs(don_d, acc, bonds, extra=np.array([[False, False, True]])).all()
    with pytest.raises(ValueError, match="outside"):
        hbonds.excluded_pairs(don_d, acc, bonds, extra=[(0, 3)])
    assert hbonds.excluded_mask(don_d, acc, bonds).tolist() == [[3]]


@pytest.mark.parametrize("nA", [1, 64, 65])
def test_pack_mask_word_and_bit_positions(nA):
    W = (nA + 63) // 64
    pairs = [(0, 0), (1, nA - 1), (2, nA // 2)]
    words = hbonds.pack_mask(pairs, nH=3, nA=nA)
    assert words.dtype == np.uint64 and words.shape == (3, W)
    want = np.zeros((3, W), dtype=np.uint64)
    for h, a in pairs:
        want[h, a >> 6] |= np.uint64(1) << np.uint64(a & 63)
    assert np.array_equal(words, want)
    mask = np.zeros((3, nA), dtype=bool)
    for h, a in pairs:
        mask[h, a] = True
    assert np.array_equal(hbonds.pack_mask(mask), want) and np.array_equal(R.pack(mask), want)
    assert np.array_equal(hbonds.unpack_mask(words, nA), mask)
    full = hbonds.pack_mask(np.ones((2, nA), dtype=bool))
    assert int(full[0, -1]) == (1 << (nA - 64 * (W - 1))) - 1                 # bits past nA are zero
    if nA == 65:
        assert words[1].tolist() == [0, 1] and full[0].tolist() == [2 ** 64 - 1, 1]
    with pytest.raises(ValueError, match="nH and nA"):
        hbonds.pack_mask(pairs)


# ----------------------------------------------------------------------------- the predicate
def _one(distance, theta, cutoff=2.5, angle=120.0):
    D, H, A = R.triple(distance, theta)
    return bool(R.bonded(D, H, A, R.cutoff2_of(cutoff), R.c2_of(angle)))


def test_the_restatement_on_hand_placed_triples():
    assert _one(1.9, 180.0) and not _one(2.6, 180.0)
    assert not _one(1.9, 110.0) and _one(1.9, 130.0)
    assert _one(2.49, 121.0) and not _one(2.51, 179.0) and not _one(2.49, 119.0)
    assert _one(1.9, 91.0, angle=90.0) and not _one(1.9, 89.0, angle=90.0)            # dot < 0 decides at 90 degrees
    just_under = math.nextafter(180.0, 0.0)
    assert not _one(1.9, 170.0, angle=just_under) and not _one(1.9, 179.0, angle=179.9) and _one(1.9, 179.99, angle=179.9)
    assert abs(float(hbonds.c2_of(120.0)) - 0.25) < 1e-7
    assert hbonds.c2_of(120.0) == R.c2_of(120.0) and hbonds.c2_of(90.0) == R.c2_of(90.0) and 0 <= float(hbonds.c2_of(90.0)) < 1e-30
    assert float(hbonds.c2_of(just_under)) <= 1.0
    assert hbonds.cutoff2_of(2.5) == R.cutoff2_of(2.5) == np.float32(6.25)
    nan = np.array([np.nan, 0.0, 0.0])
    D, H, A = R.triple(1.9, 180.0)
    assert not R.bonded(nan, H, A, 6.25, 0.25) and not R.bonded(D, nan, A, 6.25, 0.25) and not R.bonded(D, H, nan, 6.25, 0.25)


def test_the_square_root_free_form_against_an_fp64_arccos():
    rng = np.random.default_rng(7)
    n = 10 ** 4
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    D = rng.normal(0.0, 5.0, (n, 3))
    H = D + rng.uniform(0.9, 1.1, (n, 1)) * unit(rng.normal(size=(n, 3)))
    A = H + rng.uniform(1.5, 3.5, (n, 1)) * unit(rng.normal(size=(n, 3)))
    D, H, A = (v.astype(np.float32) for v in (D, H, A))
    for angle in (120.0, 90.0, 150.0):
        got = R.bonded(D, H, A, R.cutoff2_of(2.5), R.c2_of(angle))
        want = R.bonded64(D, H, A, 2.5, angle)
        tie = R.near_tie(D, H, A, 2.5, angle)
        assert 0.02 * n < want.sum() < 0.6 * n                                # the draw has both kinds
        assert not ((got != want) & ~tie).any()
        assert tie.sum() < 0.01 * n


def test_the_restatement_produces_every_output():
    z, bonds = R.molecule(3, 70, n_excluded=2)
    don_h, don_d, acc = hbonds.donors_acceptors(z, bonds, R.DONORS, R.ACCEPTORS)
    assert don_h.tolist() == [0, 1, 2] and don_d.tolist() == [3, 4, 5] and acc.tolist() == list(range(6, 76))
    excl = hbonds.excluded_pairs(don_d, acc, bonds)
    assert excl.sum() == 2 and excl[0, 0] and excl[1, 5]
    xyz = R.cloud(z, bonds, 5, 1.5, np.random.default_rng(3))
    xyz[2, 7, 1] = np.inf
    native = np.zeros_like(excl)
    native[:, ::2] = True
    w = R.hbond_counts(xyz, don_h, don_d, acc, excl, native)
    assert w["bad"].tolist() == [False, False, True, False, False] and w["n_good"] == 4
    assert w["n_hbonds"][2] == -1 and w["n_native"][2] == -1 and not w["bits"][2].any()
    assert w["bits"].shape == (5, 3, 2) and w["pair_counts"].sum() == w["n_hbonds"][~w["bad"]].sum() > 0
    assert np.array_equal(R.popcount(w["bits"]).sum(axis=1), np.where(w["bad"], 0, w["n_hbonds"]))
    assert np.array_equal(R.popcount(w["bits"] & R.pack(native)[None]).sum(axis=1), np.where(w["bad"], 0, w["n_native"]))
    assert not (w["bonds"] & excl[None]).any()


# ----------------------------------------------------------------------------- statistics
def _result(pair_counts, n_hbonds, n_native=None, bad=None):
    """A result of ``hbond_counts`` over a 2 x 3 table: hydrogens 10, 11 on donors 0, 1; acceptors 1, 2, 3 (pair (1, 0):
    A is D)."""
    n_hbonds = np.asarray(n_hbonds, dtype=np.int64)
    bad = np.zeros(n_hbonds.shape[0], dtype=bool) if bad is None else np.asarray(bad, dtype=bool)
    excl = np.array([[False, False, False], [True, False, False]])
    return {"pair_counts": np.asarray(pair_counts, dtype=np.int64), "n_hbonds": n_hbonds,
            "n_native": np.zeros_like(n_hbonds) if n_native is None else np.asarray(n_native, dtype=np.int64), "bad": bad,
            "n_good": int((~bad).sum()), "don_h": np.array([10, 11], np.int32), "don_d": np.array([0, 1], np.int32),
            "acc": np.array([1, 2, 3], np.int32), "excluded": excl}


def test_occupancy_and_the_native_set_at_its_boundary():
    even, odd = _result([[2, 1, 0], [0, 0, 1]], [1, 2, 1]), _result([[1, 0, 0], [0, 0, 2]], [2, 0, 1])
    assert np.array_equal(hbonds.occupancy(even), np.array([[2, 1, 0], [0, 0, 1]]) / 3.0)
    assert hbonds.occupancy(_result(np.zeros((2, 3)), [-1], bad=[True])) is None
    # over the reference: 3/6, 1/6, 0, -, 0, 3/6: at native_occupancy = 0.5 a pair with exactly half is native
    assert hbonds.native_pairs(even, odd, 0.5).tolist() == [[True, False, False], [False, False, True]]
    assert not hbonds.native_pairs(even, odd, 0.51).any()
    assert hbonds.native_pairs(even, odd, 1.0 / 6.0).tolist() == [[True, True, False], [False, False, True]]
    both = _result([[3, 0, 0], [3, 0, 0]], [2, 2, 2])
    assert hbonds.native_pairs(both, both, 0.5).tolist() == [[True, False, False], [False, False, False]]   # excluded: never native


def test_compare_from_counts_kept_missing_and_spurious():
    native = np.array([[True, False, False], [False, False, True]])
    even = _result([[2, 0, 0], [0, 0, 2]], [2, 2], n_native=[2, 2])
    odd = _result([[2, 0, 0], [0, 0, 1]], [2, 1], n_native=[2, 1])
    gen = _result([[4, 0, 0], [0, 3, 0]], [2, 2, 1, 2, -1], n_native=[1, 1, 1, 1, -1], bad=[0, 0, 0, 0, 1])
    stats = hbonds.compare_from_counts(even, odd, gen, native=native, params={"angle": 120.0})
    assert set(stats) == set(hbonds.HBOND_STATS_KEYS)
    assert (stats["n_ref"], stats["n_gen"], stats["n_bad_ref"], stats["n_bad_gen"]) == (4, 5, 0, 1)
    assert stats["n_native"] == 2 and stats["native"] == [[0, 10, 1], [1, 11, 3]]
    assert stats["kept_ref"] == pytest.approx((2 + 2 + 2 + 1) / 4 / 2) and stats["kept_gen"] == pytest.approx(0.5)
    assert stats["missing"] == [[1, 11, 3]]                   # native, generated occupancy 0 < 0.1
    assert stats["spurious"] == [[1, 11, 2]]                  # not native, generated 0.75 >= 0.5, reference 0 < 0.1
    occ = {(p["d"], p["h"], p["a"]): (p["occ_ref"], p["occ_gen"], p["native"]) for p in stats["pairs"]}
    assert occ == {(0, 10, 1): (1.0, 1.0, True), (1, 11, 2): (0.0, 0.75, False), (1, 11, 3): (0.75, 0.0, True)}
    ref, got = np.array([1.0, 0, 0, 0, 0.75]), np.array([1.0, 0, 0, 0.75, 0])    # the five pairs that are not excluded
    assert stats["occupancy_rmse"] == pytest.approx(np.sqrt(np.mean((ref - got) ** 2)))
    assert stats["occupancy_pearson"] == pytest.approx(np.corrcoef(ref, got)[0, 1])
    assert stats["floor"]["occupancy_rmse"] == pytest.approx(np.sqrt(0.25 / 5))
    assert stats["n_hbonds"]["mean_ref"] == pytest.approx(1.75) and stats["n_hbonds"]["mean_gen"] == pytest.approx(1.75)
    assert stats["n_hbonds"]["hist_gen"]["counts"] == [0, 1, 3] and stats["n_hbonds"]["hist_ref"]["counts"] == [0, 1, 3]
    assert stats["backbone_ref"] is None and stats["backbone_gen"] is None
    assert stats["params"] == {"angle": 120.0}
    json.dumps(stats)
    short = hbonds.summary_of(stats)
    assert set(short) == {"n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "occupancy_rmse", "occupancy_pearson", "floor", "n_native",
                          "kept_ref", "kept_gen", "n_missing", "n_spurious", "n_hbonds"}
    assert short["n_missing"] == 1 and short["n_spurious"] == 1 and set(short["n_hbonds"]) == {"jsd", "mean_ref", "std_ref", "mean_gen", "std_gen"}


def test_identical_halves_have_a_zero_floor_and_an_empty_set_gives_none():
    half = _result([[2, 1, 0], [0, 0, 1]], [1, 2, 1], n_native=[1, 1, 0])
    native = np.array([[True, False, False], [False, False, False]])
    stats = hbonds.compare_from_counts(half, half, half, native=native)
    assert stats["floor"]["occupancy_rmse"] == 0.0 and stats["occupancy_rmse"] == 0.0
    assert stats["floor"]["occupancy_pearson"] == pytest.approx(1.0) and stats["floor"]["n_hbonds_jsd"] == 0.0
    assert stats["kept_ref"] == stats["kept_gen"] == pytest.approx(2.0 / 3.0) and stats["missing"] == [] and stats["spurious"] == []
    none = hbonds.compare_from_counts(half, half, half)
    assert none["n_native"] == 0 and none["kept_ref"] is None and none["kept_gen"] is None and none["missing"] == []
    flat = _result(np.zeros((2, 3)), [0, 0])
    assert hbonds.compare_from_counts(flat, flat, flat)["floor"]["occupancy_pearson"] is None       # a constant table
    empty = _result(np.zeros((2, 3)), [-1, -1], n_native=[-1, -1], bad=[True, True])
    stats = hbonds.compare_from_counts(half, half, empty, native=native)
    assert stats["occupancy_rmse"] is None and stats["n_hbonds"] is None and stats["kept_gen"] is None and stats["missing"] is None
    assert hbonds.summary_of(stats)["n_hbonds"] is None and hbonds.summary_of(stats)["n_missing"] is None


def test_the_backbone_map_of_alanine_dipeptide():
    don_h, don_d, acc = hbonds.donors_acceptors(ALA_Z, ALA_BONDS)
    res = {"pair_counts": np.array([[0, 0, 3, 0], [1, 0, 0, 0]]), "n_good": 4, "don_h": don_h, "don_d": don_d, "acc": acc}
    m = hbonds.backbone_map(res, ALA_Z, ALA_BONDS)
    assert m.shape == (1, 1) and m[0, 0] == 0.75                # one residue: N 6 - CA 8 - C 14; N-H 7 ... O 15
    assert hbonds.backbone_map(res, np.array([1, 8, 1]), np.array([(0, 1), (1, 2)])) is None


# ----------------------------------------------------------------------------- refusals before any launch
def test_every_value_error_comes_before_a_device_is_touched():
    xyz = np.zeros((3, 22, 3), np.float32)

    def refused(match, frames=xyz, z=ALA_Z, bonds=ALA_BONDS, **kw):
        with pytest.raises(ValueError, match=match):
            hbonds.hbond_counts(frames, z, bonds, **kw)
    for angle in (89.9, 180.0, 200.0, float("nan"), -120.0):
        refused(r"\[90, 180\)", angle=angle)
    for cutoff in (-1.0, float("inf"), float("nan")):
        refused("cutoff", h_a_cutoff=cutoff)
    refused("z lists 21 atoms", z=ALA_Z[:21])
    refused("bonds name atom", bonds=np.array([(0, 22)]))
    refused(r"\[S, n, 3\]", frames=np.zeros((3, 22), np.float32))
    refused("no acceptor", acceptor_elements=(16,))
    refused("no donor hydrogen", donor_elements=(16,))
    refused(r"native must be a bool array \[2, 4\]", native=np.zeros((2, 5), dtype=bool))
    refused("outside", excluded=[(2, 0)])
    lim = hbonds.limits()
    z, bonds = R.molecule(lim["hydrogens"] + 1, 2)
    refused("the kernel holds", frames=np.zeros((1, z.shape[0], 3), np.float32), z=z, bonds=bonds,
            donor_elements=R.DONORS, acceptor_elements=R.ACCEPTORS)
    z, bonds = R.molecule(2, lim["acceptors"] + 1)
    refused("the kernel holds", frames=np.zeros((1, z.shape[0], 3), np.float32), z=z, bonds=bonds,
            donor_elements=R.DONORS, acceptor_elements=R.ACCEPTORS)
    with pytest.raises(ValueError, match="at least two reference frames"):
        hbonds.compare(xyz[:1], xyz, ALA_Z, ALA_BONDS)
    with pytest.raises(ValueError, match="z lists"):
        hbonds.compare(xyz, xyz[:, :21], ALA_Z, ALA_BONDS)
    with pytest.raises(ValueError, match="native_occupancy"):
        hbonds.compare(xyz, xyz, ALA_Z, ALA_BONDS, native_occupancy=0.0)


# ----------------------------------------------------------------------------- command line
def _files(tmp_path, n_ref=4):
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "ref.npz", xyz=rng.normal(0, 2, (n_ref, 22, 3)).astype(np.float32), z=ALA_Z, bonds=ALA_BONDS)
    np.savez(tmp_path / "gen.npz", xyz=rng.normal(0, 2, (2, 3, 22, 3)).astype(np.float32))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}"


def test_the_parser_and_read_inputs(tmp_path):
    base = _files(tmp_path)
    args = hbonds.parser().parse_args(base.split())
    assert (args.hbond_cutoff, args.hbond_angle, args.hbond_native, args.bits, args.out, args.top) == \
        (2.5, 120.0, 0.5, None, "hbond_stats.json", None)
    inp = hbonds.read_inputs(args)
    assert inp["ref_xyz"].shape == (4, 22, 3) and inp["gen_xyz"].shape == (6, 22, 3) and inp["z"].tolist() == ALA_Z.tolist()
    args = hbonds.parser().parse_args((base + " -hbond_cutoff 3 -hbond_angle 135 -hbond_native 0.3 -bits b.npz -out x.json").split())
    assert (args.hbond_cutoff, args.hbond_angle, args.hbond_native, args.bits, args.out) == (3.0, 135.0, 0.3, "b.npz", "x.json")
    np.savez(tmp_path / "top.npz", z=ALA_Z, bonds=ALA_BONDS[:8])
    inp = hbonds.read_inputs(hbonds.parser().parse_args((base + f" -top {tmp_path / 'top.npz'}").split()))
    assert inp["bonds"].tolist() == ALA_BONDS[:8].tolist()


def test_the_command_line_refuses_before_any_launch(tmp_path):
    base = _files(tmp_path)

    def refused(extra, match):
        with pytest.raises(SystemExit, match=match):
            hbonds.read_inputs(hbonds.parser().parse_args((base + " " + extra).split()))
    refused("-hbond_cutoff -1", "-hbond_cutoff")
    refused("-hbond_angle 80", "-hbond_angle")
    refused("-hbond_angle 180", "-hbond_angle")
    refused("-hbond_native 0", "-hbond_native")
    refused("-hbond_native 1.5", "-hbond_native")
    refused(f"-top {tmp_path / 'nothing.npz'}", "no such file")
    np.savez(tmp_path / "other.npz", z=[6, 6], bonds=[[0, 1]])
    refused(f"-top {tmp_path / 'other.npz'}", "the topology has 2 atoms")
    np.savez(tmp_path / "carbon.npz", z=np.where(ALA_Z == 1, 1, 6), bonds=ALA_BONDS)
    refused(f"-top {tmp_path / 'carbon.npz'}", "no donor hydrogen")
    np.savez(tmp_path / "bare.npz", xyz=np.zeros((4, 22, 3), np.float32))
    with pytest.raises(SystemExit, match="z / bonds"):
        hbonds.read_inputs(hbonds.parser().parse_args(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'bare.npz'}".split()))
    np.savez(tmp_path / "short.npz", xyz=np.zeros((1, 22, 3), np.float32), z=ALA_Z, bonds=ALA_BONDS)
    with pytest.raises(SystemExit, match="at least two"):
        hbonds.read_inputs(hbonds.parser().parse_args(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'short.npz'}".split()))
    np.savez(tmp_path / "wide.npz", xyz=np.zeros((3, 23, 3), np.float32))
    with pytest.raises(SystemExit, match="wide.npz: xyz is"):
        hbonds.read_inputs(hbonds.parser().parse_args(f"-gen {tmp_path / 'wide.npz'} -ref {tmp_path / 'ref.npz'}".split()))
    with pytest.raises(SystemExit):
        hbonds.parser().parse_args(["-gen", "a.npz"])                          # -ref is required


# ----------------------------------------------------------------------------- library
def test_the_library_declares_binds_and_exports_the_hydrogen_bond_kernel():
    names = {"cgv_hbond_max_structures", "cgv_hbond_max_hydrogens", "cgv_hbond_max_acceptors", "cgv_hbond_row_tile",
             "cgv_hbond_chunk", "cgv_hbond_workspace_bytes", "cgv_hbond_counts"}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.PROTOTYPES)
    lim = hbonds.limits()
    assert lim["hydrogens"] >= 4096 and lim["acceptors"] >= 4096 and lim["structures"] >= 4096
    lib = _lib.load()
    assert lib.cgv_hbond_workspace_bytes(10, 3, 5) >= 10 * (3 + 3 + 5) * 16
    assert lib.cgv_hbond_workspace_bytes(10, lim["hydrogens"] + 1, 5) == 0 and lib.cgv_hbond_workspace_bytes(10, 3, lim["acceptors"] + 1) == 0
    assert lib.cgv_hbond_row_tile() >= 1 and lib.cgv_hbond_chunk() >= 1


def test_the_c_entry_refuses_a_table_past_a_limit_with_its_reason():
    lib, lim = _lib.load(), hbonds.limits()
    nulls = [None] * 6

    def refused(S, nH, nA, cutoff2, c2, reason):
        rc = lib.cgv_hbond_counts(*nulls, S, 10, nH, nA, cutoff2, c2, None, None, None, None, None, None, 0, None)
        assert rc == -1 and reason in lib.cgv_last_error_string(), lib.cgv_last_error_string()
    refused(1, lim["hydrogens"] + 1, 4, 6.25, 0.25, b"cgv_hbond_max_hydrogens")
    refused(1, 4, lim["acceptors"] + 1, 6.25, 0.25, b"cgv_hbond_max_acceptors")
    refused(lim["structures"] + 1, 4, 4, 6.25, 0.25, b"cgv_hbond_max_structures")
    refused(1, 0, 4, 6.25, 0.25, b"at least one")
    refused(1, 4, 4, float("nan"), 0.25, b"cutoff2")
    refused(1, 4, 4, 6.25, 1.5, b"c2")
    refused(1, 4, 4, 6.25, 0.25, b"null pointer")
    assert lib.cgv_hbond_counts(*nulls, 0, 10, 4, 4, 6.25, 0.25, None, None, None, None, None, None, 0, None) == 0   # nothing to do
