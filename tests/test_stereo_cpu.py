"""Stereochemistry without a device: the numpy.float32 restatement of K31 (csrc/stereo.hip) against an independent fp64
form, hand-built cases of the three predicates, ``stereo.tables`` / ``expected_from_counts`` on small molecules, the host
statistics on hand-made integers, and the command line's refusals."""
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, build, stereo
import stereo_restatement as R

F = np.float32
NAMES = {"cgv_stereo_counts", "cgv_stereo_workspace_bytes", "cgv_stereo_max_structures", "cgv_stereo_max_atoms", "cgv_stereo_max_centres",
         "cgv_stereo_max_torsions", "cgv_stereo_max_rings", "cgv_stereo_max_bonds", "cgv_stereo_max_ring", "cgv_stereo_item_tile",
         "cgv_stereo_row_tile", "cgv_stereo_col_tile", "cgv_stereo_chunk"}
MAX_MARGINAL = 0.01                    # the share of items the fp64 margins may leave out; measured 4e-4 at the most: reaching it means a bug


# ----------------------------------------------------------------------------- 1. fp32 against fp64
def test_centres_and_torsions_follow_the_fp64_form_outside_near_ties():
    rng = np.random.default_rng(0)
    n, items = 40, 2000
    quads = R._distinct(rng, n, items, 4).astype(np.int64)
    left_c = left_q = total = 0
    for x in R.cloud(25, n, rng):
        neg64, mc = R.centre64(x, quads)
        V = R.centre_value(x, quads)
        keep = mc >= R.MARGIN
        assert np.array_equal((V < 0)[keep], neg64[keep]) and not (V == 0)[keep].any()
        cis64, mq = R.torsion64(x, quads)
        keep_q = mq >= R.MARGIN
        assert np.array_equal((R.torsion_value(x, quads) > 0)[keep_q], cis64[keep_q])
        left_c, left_q, total = left_c + int((~keep).sum()), left_q + int((~keep_q).sum()), total + items
    print(f"marginal: {left_c} of {total} centres, {left_q} of {total} torsions")
    assert left_c <= MAX_MARGINAL * total and left_q <= MAX_MARGINAL * total


def test_the_crossing_test_follows_the_fp64_form_outside_near_ties():
    N = 200000
    p0, p1, g, v1, v2 = R.segments_and_triangles(N, np.random.default_rng(1))
    got = R.crossed(p0, p1, g, v1, v2)
    want, margin = R.crossed64(p0, p1, g, v1, v2)
    keep = margin >= R.MARGIN
    print(f"marginal: {int((~keep).sum())} of {N} pairs; crossing: {want.mean():.4f}; differing among the kept: {int((got != want)[keep].sum())}")
    assert np.array_equal(got[keep], want[keep])
    assert (~keep).sum() <= MAX_MARGINAL * N and 0.03 < want.mean() < 0.2


# ----------------------------------------------------------------------------- 2. hand-built cases
def test_a_mirror_image_flips_every_centre_and_nothing_else():
    rng = np.random.default_rng(2)
    n = 30
    xyz = R.cloud(6, n, rng, box=5.0)
    tab = R.random_tables(rng, n, 40, 40, 12, 50)
    a = R.counts(xyz, tab)
    b = R.counts(xyz * np.array([1, 1, -1], F), tab)
    assert not a["flat"].any() and np.array_equal(b["neg"], 6 - a["neg"]) and a["neg"].sum() > 0
    assert np.array_equal(a["cis"], b["cis"]) and np.array_equal(a["pierced"], b["pierced"]) and a["pierced"].sum() > 0 and a["cis"].sum() > 0
    want = np.where(2 * a["neg"] > 6, -1, 1)
    ca, cb = R.counts(xyz, tab, want_sign=want)["counts"], R.counts(xyz * np.array([1, 1, -1], F), tab, want_sign=want)["counts"]
    assert np.array_equal(ca[:, 0] + cb[:, 0], np.full(6, 40))       # every centre is wrong in exactly one of the two


def test_a_hexagon_and_the_segments_that_do_and_do_not_cross_it():
    tab, xyz = R.one_ring(6, [seg for seg, _ in R.HEXAGON_CASES])
    got = R.counts(xyz, tab)
    assert got["pierced"][0].tolist() == [int(hit) for _, hit in R.HEXAGON_CASES]
    assert got["counts"][0].tolist() == [0, 0, sum(hit for _, hit in R.HEXAGON_CASES)]
    tab["tested"][0, 0] = False                                      # a pair that is not looked at is not counted
    assert R.counts(xyz, tab)["pierced"][0, 0] == 0


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7, 8])
def test_rings_of_every_size(k):
    tab, xyz = R.one_ring(k, [((0.1, 0.05, -1), (0.1, 0.05, 1)), ((0.3, 0, -1), (0.3, 0, 1)), ((2, 2, -1), (2, 2, 1))])
    assert R.counts(xyz, tab)["pierced"][0].tolist() == [1, 1, 0]    # inside; through the fan edge g - v_0: once; outside
    tilted = xyz @ np.array([[1, 0, 0], [0, 0.6, -0.8], [0, 0.8, 0.6]], F).T + F(3)
    assert R.counts(tilted, tab)["pierced"][0, 0] == 1 and R.counts(tilted, tab)["pierced"][0, 2] == 0


def test_a_bad_structure_enters_nothing_and_unnamed_atoms_are_not_looked_at():
    rng = np.random.default_rng(3)
    xyz = R.cloud(4, 20, rng, box=4.0)
    tab = R.random_tables(rng, 19, 5, 5, 3, 9)                       # atom 19 is named by nothing
    xyz[1, 3, 0], xyz[2, 19, 1] = np.nan, np.inf
    assert 3 in R.named_atoms(tab)
    got = R.counts(xyz, tab, want_sign=np.ones(5), want_cis=np.zeros(5))
    assert got["bad"].tolist() == [False, True, False, False] and not got["counts"][1].any() and got["n_good"] == 3
    clean = R.counts(xyz[[0, 2, 3]], tab)
    assert all(np.array_equal(got[k], clean[k]) for k in ("neg", "flat", "cis", "pierced"))


# ----------------------------------------------------------------------------- 3. tables
def _alanine_dipeptide():
    z = np.array([6, 1, 1, 1, 6, 8, 7, 1, 6, 1, 6, 1, 1, 1, 6, 8, 7, 1, 6, 1, 1, 1])
    bonds = [[0, 1], [0, 2], [0, 3], [0, 4], [4, 5], [4, 6], [6, 7], [6, 8], [8, 9], [8, 10], [10, 11], [10, 12], [10, 13], [8, 14], [14, 15],
             [14, 16], [16, 17], [16, 18], [18, 19], [18, 20], [18, 21]]
    return z, np.array(bonds)


def test_tables_of_alanine_dipeptide():
    z, bonds = _alanine_dipeptide()
    tab = stereo.tables(z, bonds)
    assert tab["centres"].tolist() == [[8, 6, 9, 10]] and tab["candidate"].tolist() == [False]
    assert tab["torsions"].tolist() == [[0, 4, 6, 8], [8, 14, 16, 18]] and tab["n_omega"] == 2
    assert tab["rings"].shape == (0, 8) and tab["bonds"].shape == (21, 2) and tab["tested"].shape == (0, 21)
    assert stereo.sizes(tab) == (1, 2, 0, 21)
    more = stereo.tables(z, bonds, torsions=[[4, 6, 8, 14]])
    assert more["torsions"].tolist()[2] == [4, 6, 8, 14] and more["n_omega"] == 2
    with pytest.raises(ValueError, match="name atom"):
        stereo.tables(z, bonds, torsions=[[4, 6, 8, 22]])
    with pytest.raises(ValueError, match="atoms must be"):
        stereo.tables(z, bonds, atoms="backbone")


def test_tables_of_the_phenylalanine_molecule_a_ch2_and_a_ch3_are_no_centres():
    tab = stereo.tables(R.PHE_Z, R.PHE_BONDS)
    assert tab["centres"].tolist() == [[8, 6, 9, 10]]                # CA; not the CH2 (10), not the CH3s (0, 28)
    assert [tuple(t) for t in tab["torsions"].tolist()] == R.PHE["omega"]
    assert [[a for a in row if a >= 0] for row in tab["rings"].tolist()] == [R.PHE["ring"]]
    assert tab["bonds"].shape == (33, 2) and (tab["bonds"][:, 0] < tab["bonds"][:, 1]).all()
    ring = set(R.PHE["ring"])
    assert tab["tested"][0].tolist() == [not (a in ring or b in ring) for a, b in tab["bonds"].tolist()]
    assert tab["tested"][0].sum() == 33 - 6 - 5 - 1                  # without the ring's bonds, its five C - H and CB - CG


def _heavy_fragment():
    """Heavy atoms of proline (N 0, CA 1, C 2, O 3, CB 4, CG 5, CD 6), tryptophan's indole hung on atom 7 (CB) and a benzene."""
    z = [7, 6, 6, 8, 6, 6, 6] + [6] + [6, 6, 7, 6, 6, 6, 6, 6, 6] + [6] * 6
    pro = [[0, 1], [1, 2], [2, 3], [1, 4], [4, 5], [5, 6], [6, 0]]
    # indole: CG 8, CD1 9, NE1 10, CE2 11, CD2 12 (five) and CD2 12, CE2 11, CZ2 13, CH2 14, CZ3 15, CE3 16 (six), fused at 11 - 12
    trp = [[7, 8], [8, 9], [9, 10], [10, 11], [11, 12], [12, 8], [11, 13], [13, 14], [14, 15], [15, 16], [16, 12]]
    phe = [[17 + t, 17 + (t + 1) % 6] for t in range(6)]
    return np.array(z), np.array(pro + trp + phe)


def test_rings_of_proline_tryptophan_and_benzene():
    z, bonds = _heavy_fragment()
    rings = stereo.small_rings(z.shape[0], stereo.adjacency(z.shape[0], bonds))
    assert sorted(len(r) for r in rings) == [5, 5, 6, 6]             # no 9-ring around the indole
    assert sorted(sorted(r) for r in rings) == [[0, 1, 4, 5, 6], [8, 9, 10, 11, 12], [11, 12, 13, 14, 15, 16], [17, 18, 19, 20, 21, 22]]
    for r in rings:                                                  # consecutive vertices are bonded: the order is along the cycle
        have = {tuple(sorted(b)) for b in bonds.tolist()}
        assert all(tuple(sorted((r[t], r[(t + 1) % len(r)]))) in have for t in range(len(r))) and r[0] == min(r)
    tab = stereo.tables(z, bonds, atoms="heavy")
    assert stereo.ring_sizes(tab["rings"]).tolist() == [5, 5, 6, 6]
    big = np.array([[t, (t + 1) % 9] for t in range(9)])             # a 9-ring is too large, an 8-ring is not
    assert stereo.small_rings(9, stereo.adjacency(9, big)) == []
    assert [len(r) for r in stereo.small_rings(8, stereo.adjacency(8, big[:7].tolist() + [[7, 0]]))] == [8]


def test_expected_drops_the_planar_candidates_of_a_heavy_atom_topology():
    tab = stereo.tables(R.PHE_Z, R.PHE_BONDS, atoms="heavy")
    cand = {int(c[0]): bool(f) for c, f in zip(tab["centres"], tab["candidate"])}
    assert cand == {4: True, 8: True, 24: True}                      # CA and the two carbonyl carbons; CG's ortho carbons are alike
    rng = np.random.default_rng(4)
    frames = R.phe_frames(200, rng, sigma=0.05)                      # its carbonyl carbons lie in the plane of their neighbours, up to the noise
    rec = R.counts(frames, tab)
    exp = stereo.expected_from_counts(rec, tab)
    assert exp["tables"]["centres"][:, 0].tolist() == [8] and exp["want_sign"].shape == (1,) and exp["kept"].sum() == 1
    assert exp["share"][exp["kept"]].tolist() == [1.0] and (exp["share"][~exp["kept"]] < 0.9).all()
    full = R.counts(frames, stereo.tables(R.PHE_Z, R.PHE_BONDS))     # the all-atom centre (8; 6, 9, 10) has its own sign
    assert full["neg"][0] in (0, 200) and exp["want_cis"].tolist() == [0, 0]
    with pytest.raises(ValueError, match="min_share"):
        stereo.expected_from_counts(rec, tab, min_share=0.5)
    with pytest.raises(ValueError, match="no good reference frame"):
        stereo.expected_from_counts({**rec, "n_good": 0}, tab)


def test_the_three_edits_of_the_phenylalanine_frames_change_exactly_what_they_name():
    tab = stereo.tables(R.PHE_Z, R.PHE_BONDS)
    frames = R.phe_frames(8, np.random.default_rng(5))
    base = R.counts(frames, tab)
    want = stereo.expected_from_counts(base, tab)
    assert want["kept"].all() and not base["pierced"].any()
    edited = frames.copy()
    edited[1], edited[3], edited[5] = R.invert_ca(frames[1]), R.flip_omega(frames[3]), R.thread_ring(frames[5])
    edited[6] = R.thread_ring(R.flip_omega(R.invert_ca(frames[6])))
    got = R.counts(edited, tab, want["want_sign"], want["want_cis"])
    assert got["counts"].tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]]
    b = [tuple(p) for p in tab["bonds"].tolist()].index(R.PHE["cl"])
    assert got["pierced"][0, b] == 2 and got["pierced"].sum() == 2


# ----------------------------------------------------------------------------- 4. host statistics on hand-made integers
def _rec(tab, neg, flat, cis, pierced, counts, bad, ws, wc):
    bad = np.asarray(bad, bool)
    return {"neg": np.asarray(neg, np.int64), "flat": np.asarray(flat, np.int64), "cis": np.asarray(cis, np.int64),
            "pierced": np.asarray(pierced, np.int64), "counts": np.asarray(counts, np.int32).reshape(-1, 3), "bad": bad,
            "n_good": int((~bad).sum()), "tables": tab, "want_sign": np.asarray(ws, np.int32), "want_cis": np.asarray(wc, np.int32)}


def _hand_made():
    tab = {"centres": np.array([[1, 0, 2, 3], [5, 4, 6, 7]], np.int32), "torsions": np.array([[0, 1, 5, 6]], np.int32),
           "rings": np.array([[0, 1, 2, -1, -1, -1, -1, -1]], np.int32), "bonds": np.array([[4, 5], [6, 7], [0, 1]], np.int32),
           "tested": np.array([[True, True, False]]), "n_atoms": 8}
    ws, wc = [1, -1], [0]
    even = _rec(tab, [0, 2], [0, 0], [0], [[0, 0, 0]], [[0, 0, 0], [0, 0, 0]], [False, False], ws, wc)
    odd = _rec(tab, [0, 1], [0, 0], [1], [[0, 0, 0]], [[0, 1, 0], [0, 0, 0]], [False, True], ws, wc)
    gen = _rec(tab, [2, 4], [1, 0], [1], [[0, 3, 0]], [[1, 0, 1], [1, 0, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0]], [0, 0, 0, 0, 1], ws, wc)
    return tab, even, odd, gen


def test_compare_from_counts_summary_of_and_the_key_set():
    tab, even, odd, gen = _hand_made()
    st = stereo.compare_from_counts(even, odd, gen, groups=[0, 0, 0, 0, 1, 1, 1, 1], params={"atoms": "all"})
    assert tuple(st) == stereo.STEREO_STATS_KEYS and json.loads(json.dumps(st)) == st
    assert (st["n_ref"], st["n_gen"], st["n_bad_ref"], st["n_bad_gen"]) == (4, 5, 1, 1)
    assert (st["n_centres"], st["n_torsions"], st["n_rings"], st["n_bonds"], st["n_tested"]) == (2, 1, 1, 3, 2)
    assert st["valid"]["gen"] == {"centres": 0.25, "torsions": 0.75, "rings": 0.25, "all": 0.25}
    assert st["valid"]["ref"] == {"centres": 1.0, "torsions": pytest.approx(2 / 3), "rings": 1.0, "all": pytest.approx(2 / 3)}
    assert st["inversion_rate"] == {"gen": [0.75, 0.0], "ref": [0.0, 0.0]}       # centre 0 wants +: 2 negative + 1 flat of 4; centre 1 wants -
    assert st["cis_rate"] == {"gen": [0.25], "ref": [pytest.approx(1 / 3)]}
    assert st["worst_centres"][0] == {"centre": 0, "atom": 1, "want": 1, "gen": 0.75, "ref": 0.0} and len(st["worst_centres"]) == 2
    assert st["worst_torsions"][0]["atoms"] == [0, 1, 5, 6] and st["worst_torsions"][0]["gen"] == 0.25
    assert st["worst_pairs"][0] == {"ring": 0, "bond": 1, "ring_atoms": [0, 1, 2], "bond_atoms": [6, 7], "gen": 0.75, "ref": 0.0}
    assert st["worst_pairs"][-1]["bond"] == 2                        # the pair that is not tested comes last
    assert st["errors"]["hist_gen"]["counts"] == [1, 0, 2, 1] and st["errors"]["hist_ref"]["counts"] == [2, 1, 0, 0]
    assert 0 < st["errors"]["jsd"] < 1 and st["errors"]["floor"] == 1.0 and st["errors"]["mean_gen"] == 1.75
    g = st["groups"]
    assert g["n_groups"] == 2 and g["ids"] == [0, 1] and g["rows"][0]["centres"] == {"n": 1, "gen": 0.75, "ref": 0.0}
    assert g["rows"][1]["centres"]["gen"] == 0.0 and g["rows"][0]["rings"]["gen"] == 0.75 and g["worst"][0]["id"] == 0
    short = stereo.summary_of(st)
    assert set(short) == {"n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_centres", "n_torsions", "n_rings", "n_tested", "valid",
                          "worst_centres", "worst_torsions", "worst_pairs", "errors", "groups"}
    assert len(short["worst_pairs"]) == 1 and "hist_ref" not in short["errors"] and short["groups"]["n_groups"] == 2
    assert stereo.compare_from_counts(even, odd, gen)["groups"] is None
    with pytest.raises(ValueError, match="label for every atom"):
        stereo.compare_from_counts(even, odd, gen, groups=[0, 1])


def test_tables_are_checked_before_anything_else():
    tab, _, _, _ = _hand_made()
    assert stereo.checked(tab, 8)["rings"].dtype == np.int32 and stereo.ring_sizes(tab["rings"]).tolist() == [3]
    for key, bad_value, match in (("centres", np.array([[1, 0, 2, 8]]), "name atom"), ("bonds", np.array([[0, 1, 2]]), r"\[., 2\]"),
                                  ("rings", np.array([[0, 1, -1, 2, -1, -1, -1, -1]]), "then -1"),
                                  ("rings", np.array([[0, 1, -1, -1, -1, -1, -1, -1]]), "at least 3"),
                                  ("tested", np.ones((1, 2), bool), "tested must be"), ("torsions", np.zeros((1, 4)), "int array")):
        with pytest.raises(ValueError, match=match):
            stereo.checked({**tab, key: bad_value}, 8)
    with pytest.raises(ValueError, match="want_sign"):
        stereo._want({"want_sign": [1, 0]}, 2, 1)
    with pytest.raises(ValueError, match="want_cis"):
        stereo._want({"want_cis": [2]}, 2, 1)
    assert stereo._want({"want_sign": [1, -1]}, 2, 1)[1] is None


# ----------------------------------------------------------------------------- 5. the command line
def _files(tmp_path, z=R.PHE_Z, bonds=R.PHE_BONDS, **extra):
    rng = np.random.default_rng(6)
    keys = {} if bonds is None else {"bonds": bonds}
    np.savez(tmp_path / "ref.npz", xyz=R.cloud(4, len(z), rng), z=z, **keys, **extra)
    np.savez(tmp_path / "gen.npz", xyz=R.cloud(3, len(z), rng))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}"


def test_the_parser_and_read_inputs(tmp_path):
    base = _files(tmp_path, mapping=np.arange(34) // 6)
    args = stereo.parser().parse_args(base.split())
    assert (args.stereo_atoms, args.stereo_min_share, args.stereo_groups, args.flags, args.out, args.device) == \
        ("all", 0.99, "none", None, "stereo_stats.json", "cuda")
    inp = stereo.read_inputs(args)
    assert stereo.sizes(inp["tables"]) == (1, 2, 1, 33) and inp["ref_xyz"].shape == (4, 34, 3) and inp["gen_xyz"].shape == (3, 34, 3)
    inp = stereo.read_inputs(stereo.parser().parse_args((base + " -stereo_atoms heavy -stereo_groups bead").split()))
    assert stereo.sizes(inp["tables"])[3] == 17 and inp["mapping"].shape == (34,)
    with pytest.raises(SystemExit):
        stereo.parser().parse_args((base + " -stereo_groups atom").split())


def test_every_refusal_of_the_command_line_comes_before_the_library_is_loaded(tmp_path, monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    base = _files(tmp_path, bonds=None)                              # z alone

    def refused(extra, match, line=None):
        with pytest.raises(SystemExit, match=match):
            stereo.main(((line or base) + " " + extra).split())
    refused("", "missing z / bonds")
    np.savez(tmp_path / "top.npz", z=R.PHE_Z, bonds=R.PHE_BONDS)
    with_top = base + f" -top {tmp_path / 'top.npz'}"
    refused("-stereo_groups bead", "missing", line=with_top)
    refused("-stereo_min_share 0.4", "-stereo_min_share", line=with_top)
    refused("-stereo_groups residue", "not connected", line=with_top)            # the chlorine molecule belongs to no residue
    np.savez(tmp_path / "nokeys.npz", xyz=np.zeros((4, 34, 3), F))
    refused("", "missing z", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'nokeys.npz'}")
    np.savez(tmp_path / "ethane.npz", z=np.array([6, 6, 1, 1, 1, 1, 1, 1]), bonds=np.array([[0, 1], [0, 2], [0, 3], [0, 4], [1, 5], [1, 6], [1, 7]]))
    np.savez(tmp_path / "ref8.npz", xyz=np.zeros((4, 8, 3), F))
    np.savez(tmp_path / "gen8.npz", xyz=np.zeros((2, 8, 3), F))
    refused("", "nothing to check", line=f"-gen {tmp_path / 'gen8.npz'} -ref {tmp_path / 'ref8.npz'} -top {tmp_path / 'ethane.npz'}")
    refused("", "the topology has 8 atoms", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref8.npz'} -top {tmp_path / 'ethane.npz'}")
    refused("", "the topology has 34 atoms", line=f"-gen {tmp_path / 'gen8.npz'} -ref {tmp_path / 'ref.npz'} -top {tmp_path / 'top.npz'}")
    np.savez(tmp_path / "one.npz", xyz=np.zeros((1, 34, 3), F))
    refused("", "at least two reference frames", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'one.npz'} -top {tmp_path / 'top.npz'}")
    refused("", "no such file", line=f"-gen {tmp_path / 'absent.npz'} -ref {tmp_path / 'ref.npz'} -top {tmp_path / 'top.npz'}")
    with pytest.raises(ValueError, match="nothing to check"):        # compare itself, on host arrays, before any launch
        stereo.compare(np.zeros((2, 8, 3), F), np.zeros((4, 8, 3), F), np.array([6, 6, 1, 1, 1, 1, 1, 1]),
                       np.array([[0, 1], [0, 2], [0, 3], [0, 4], [1, 5], [1, 6], [1, 7]]), device="cpu")


# ----------------------------------------------------------------------------- the library
def test_the_library_declares_binds_and_exports_the_stereo_kernel():
    assert NAMES <= set(_lib.header_symbols()) and NAMES <= set(_lib.PROTOTYPES)
    assert build.SOURCE_FLAGS["stereo.hip"] == ["-ffp-contract=off"] and len(_lib.PROTOTYPES["cgv_stereo_counts"][1]) == 25
    lib = _lib.load()
    assert (lib.cgv_stereo_item_tile(), lib.cgv_stereo_row_tile(), lib.cgv_stereo_col_tile(), lib.cgv_stereo_chunk()) == (256, 16, 64, 8)
    assert lib.cgv_stereo_max_ring() == stereo.MAX_RING == R.MAX_RING == 8
    assert stereo.limits() == {"structures": 2 ** 20, "atoms": 32768, "centres": 65536, "torsions": 65536, "rings": 2048, "bonds": 32768, "ring": 8}
    assert lib.cgv_stereo_workspace_bytes(10, 5, 2) == 10 * 7 * 16 and lib.cgv_stereo_workspace_bytes(1, 32769, 0) == 0
    assert lib.cgv_stereo_workspace_bytes(2 ** 20 + 1, 2, 0) == 0 and lib.cgv_stereo_workspace_bytes(1, 2, 2049) == 0


def test_the_c_entry_refuses_with_its_reason():
    lib = _lib.load()

    def call(S=1, n=8, P=4, C=1, Q=1, R=1, B=1):
        rc = lib.cgv_stereo_counts(*([None] * 9), S, n, P, C, Q, R, B, *([None] * 6), None, 0, None)
        return rc, lib.cgv_last_error_string().decode()
    for kw, why in ((dict(S=2 ** 20 + 1), "max_structures"), (dict(n=40000, P=32769), "max_atoms"), (dict(P=9), "n_sel <= n_atoms"),
                    (dict(C=65537), "max_centres"), (dict(Q=65537), "max_torsions"), (dict(R=2049), "max_rings"), (dict(B=32769), "max_bonds"),
                    (dict(P=0), "at least one selected atom"), (dict(S=-1), "bad size"), (dict(C=-1), "bad size"), (dict(), "null pointer")):
        rc, msg = call(**kw)
        assert rc != 0 and why in msg and "cgv_stereo_counts" in msg, (kw, msg)
    assert call(S=0)[0] == 0                                         # no structures: nothing to do
