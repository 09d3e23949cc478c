"""lDDT and clashes, host side: the numpy restatement against an independent fp64 lDDT and against known values, the masks,
the pairing defaults, the statistics on hand-made integer tables, the command line's refusals and the library's -- all
without a device."""
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, build, contacts, ensemble, lddt
import density_restatement as DR
import lddt_restatement as R

CARBON = 1.7                                                     # Bondi


def _chain_case(n, S, sigma, seed):
    rng = np.random.default_rng(seed)
    ref = R.chain(n, rng)
    return ref, R.noisy(ref, S, sigma, rng), contacts.excluded_pairs(R.chain_bonds(n), n, np.arange(n), 3)


def _score(w, s=0):
    sc = w["struct_counts"][s]
    return sc[1:5].sum() / (4.0 * sc[0])


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n", [31, 129])
def test_the_restatement_against_an_independent_fp64_lddt(n):
    ref, xyz, excl = _chain_case(n, 4, 1.5, n)
    pairs = int(np.triu(~excl, 1).sum())
    dropped = 0
    for s in range(xyz.shape[0]):
        tie = R.near_tie(xyz[s], ref)
        dropped += int(np.triu(tie & ~excl, 1).sum())
        mask = excl | tie
        w = R.lddt_counts(xyz[s:s + 1], ref[None], [0], np.arange(n), mask, mask, np.full(n, CARBON))
        assert 0 < w["struct_counts"][0, 1] < w["struct_counts"][0, 4] <= w["struct_counts"][0, 0]
        assert _score(w) == pytest.approx(R.lddt64(xyz[s], ref, mask), abs=1e-12)
    print(f"n = {n}: the tie filter drops {dropped} of {pairs * xyz.shape[0]} pairs")
    assert dropped <= 0.01 * pairs * xyz.shape[0]


@pytest.mark.parametrize("n", [8, 31, 63, 65, 129, 257])
def test_the_chain_cloud_stays_inside_the_guard_bands(n):
    ref, xyz, excl = _chain_case(n, 12, 1.5, n)
    w = R.lddt_counts(xyz, ref[None], [0] * 12, np.arange(n), excl, excl, np.full(n, CARBON), R0=R.cloud_radius(n))
    sh = R.shares(w)
    print(n, sh)
    assert 0.30 <= sh["included"] <= 0.95 and all(0.05 <= p <= 0.95 for p in sh["preserved"]) and 0.01 <= sh["clash"] <= 0.50, sh
    assert np.array_equal(w["atom_counts"].sum(0), 2 * w["struct_counts"].sum(0))


def test_known_values():
    ref, _, excl = _chain_case(40, 1, 0.0, 5)
    sel, r = np.arange(40), np.full(40, CARBON)
    same = R.lddt_counts(ref[None], ref[None], [0], sel, excl, excl, r)
    assert _score(same) == 1.0 and same["struct_counts"][0, 0] > 0
    a, b, c = 0.7, -1.1, 0.4                                       # a rigid motion: Rz(a) Ry(b) Rx(c) x + t
    rot = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @
           np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]]) @
           np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]]))
    moved = (ref.astype(np.float64) @ rot.T + np.array([3.0, -20.0, 11.0])).astype(np.float32)
    mask = excl | R.near_tie(moved, ref)
    assert np.triu(mask & ~excl, 1).sum() <= 0.01 * np.triu(~excl, 1).sum()
    w = R.lddt_counts(moved[None], ref[None], [0], sel, mask, mask, r)
    assert _score(w) == 1.0 and w["struct_counts"][0, 0] > 0
    none = np.eye(2, dtype=bool)
    two = lambda d0, d: R.lddt_counts(np.array([[[0, 0, 0], [d, 0, 0]]], np.float32), np.array([[[0, 0, 0], [d0, 0, 0]]], np.float32),
                                      [0], [0, 1], none, none, [CARBON, CARBON])
    w = two(10.0, 10.75)
    assert w["struct_counts"][0].tolist() == [1, 0, 1, 1, 1, 0] and _score(w) == 0.75
    assert w["atom_counts"].tolist() == [[1, 0, 1, 1, 1, 0]] * 2
    assert two(15.1, 15.1)["struct_counts"][0].tolist() == [0] * 6                # beyond the inclusion radius: counts nowhere
    assert two(2.0, 2.9)["struct_counts"][0].tolist() == [1, 0, 1, 1, 1, 1]       # 2.9 < 1.7 + 1.7 - 0.4
    assert two(2.0, 3.0)["struct_counts"][0, 5] == 0                              # strict
    nan = R.lddt_counts(np.full((1, 2, 3), np.nan, np.float32), np.zeros((1, 2, 3), np.float32), [0], [0, 1], none, none, [1.7, 1.7])
    assert nan["bad"].tolist() == [True] and nan["struct_counts"][0].tolist() == [-1] * 6 and not nan["atom_counts"].any()


# ----------------------------------------------------------------------------- masks and pairing
def test_the_masks_of_both_kinds():
    z, bonds = DR.peptide(3)
    n = z.shape[0]
    labels = lddt.groups_of(z, bonds, None, "residue")
    assert sorted(set(labels.tolist())) == [0, 1, 2]
    xyz = np.zeros((2, n, 3), np.float32)
    with pytest.raises(RuntimeError, match="device"):              # everything before the launch went through
        lddt.lddt_counts(xyz, xyz, z, bonds, groups=labels, device="cpu")
    same = lddt.same_group_pairs(labels)
    assert same.diagonal().all() and np.array_equal(same, same.T) and same.sum() == sum(int((labels == g).sum()) ** 2 for g in range(3))
    by_bonds = contacts.excluded_pairs(bonds, n, np.arange(n), 2)
    assert by_bonds[0, 3] and not by_bonds[0, 4] and by_bonds.diagonal().all()  # CH3 - C - N is two bonds, CA three
    packed = ensemble.pack_mask(by_bonds)
    assert packed.dtype == np.uint32 and packed.shape == (n, 1)
    assert packed.tolist() == [[sum(1 << int(j) for j in np.flatnonzero(row))] for row in by_bonds]     # n <= 32: one word a row
    wide = np.zeros((3, 65), dtype=bool)
    wide[0, 0] = wide[1, 31] = wide[1, 32] = wide[2, 64] = True
    assert ensemble.pack_mask(wide).tolist() == [[1, 0, 0], [1 << 31, 1, 0], [0, 0, 1]]


def test_the_ref_index_defaults_and_the_refusal():
    assert lddt.default_ref_index(4, 4).tolist() == [0, 1, 2, 3]
    assert lddt.default_ref_index(5, 1).tolist() == [0] * 5
    assert lddt.default_ref_index(6, 3).tolist() == [0, 0, 1, 1, 2, 2]
    assert lddt.default_ref_index(0, 1).shape == (0,)
    for S, T in ((5, 2), (3, 6), (4, 0)):
        with pytest.raises(ValueError, match="pass ref_index"):
            lddt.default_ref_index(S, T)


def test_every_value_error_comes_before_a_device_is_touched():
    z, bonds = DR.peptide(2)
    n = z.shape[0]
    xyz = np.zeros((4, n, 3), np.float32)

    def refused(match, x=xyz, ref=xyz, zz=z, **kw):
        with pytest.raises(ValueError, match=match):
            lddt.lddt_counts(x, ref, zz, bonds, **kw)
    refused("pass ref_index", ref=xyz[:3])
    refused("ref_index names reference", ref_index=[0, 1, 2, 4])
    refused("ref_index lists 3", ref_index=[0, 1, 2])
    refused("z lists", zz=z[:-1])
    refused(r"\[S, n, 3\]", x=np.zeros((4, n), np.float32))
    refused("ascending", thresholds=(0.5, 2, 1, 4))
    refused("four thresholds", thresholds=(0.5, 1, 2))
    refused("threshold must be", thresholds=(-0.5, 1, 2, 4))
    refused("threshold must be", thresholds=(0.5, 1, 2, float("inf")))
    refused("tolerance", clash_tolerance=float("nan"))
    refused("tolerance", clash_tolerance=-0.1)
    for radius in (-1.0, float("inf"), float("nan")):
        refused("finite distance", inclusion_radius=radius)
    refused("depth", exclude=-1)
    refused("groups lists", groups=np.zeros(n - 1, dtype=int))
    refused("radii must be", radii=np.ones(n - 1))
    refused("radii must be", radii=np.full(n, np.nan))
    refused("no radius for the element", zz=np.where(z == 8, 99, z))
    refused("atoms must be", atoms="light")
    refused("selection is empty", zz=np.ones(n, dtype=int))
    big = lddt.limits()["atoms"] + 1
    with pytest.raises(ValueError, match="the kernel holds"):
        lddt.lddt_counts(np.zeros((1, big, 3), np.float32), np.zeros((1, big, 3), np.float32), np.full(big, 6), np.zeros((0, 2), int))
    with pytest.raises(ValueError, match="symmetric"):
        lddt.count_pairs(xyz, xyz, np.arange(4), np.arange(n), np.triu(np.ones((n, n), bool)), np.eye(n, dtype=bool), np.ones(n))
    with pytest.raises(ValueError, match="at least two reference frames"):
        lddt.compare(xyz[:1], xyz, z, bonds)
    with pytest.raises(ValueError, match="groups must be"):
        lddt.compare(xyz, xyz, z, bonds, groups="chain")


# ----------------------------------------------------------------------------- statistics on hand-made tables
def _result(struct, atom, bad=None, sel=(0, 2, 3)):
    struct = np.asarray(struct, dtype=np.int64).reshape(-1, 6)
    bad = np.zeros(struct.shape[0], dtype=bool) if bad is None else np.asarray(bad, dtype=bool)
    return {"struct_counts": struct, "atom_counts": np.asarray(atom, dtype=np.int64).reshape(-1, 6), "bad": bad,
            "n_good": int((~bad).sum()), "sel": np.asarray(sel, dtype=np.int32)}


def test_scores_and_profile_on_hand_made_tables():
    res = _result([[4, 1, 2, 3, 4, 2], [0, 0, 0, 0, 0, 0], [-1] * 6], [[8, 2, 4, 6, 8, 1], [0, 0, 0, 0, 0, 3], [4, 4, 4, 4, 4, 0]],
                  bad=[0, 0, 1])
    sc = lddt.scores(res)
    assert sc["lddt"][0] == (1 + 2 + 3 + 4) / 16.0 and np.isnan(sc["lddt"][1]) and np.isnan(sc["lddt"][2])
    assert sc["n_clashes"].tolist() == [2, 0, -1]
    assert sc["clashes_per_1000_atoms"][0] == pytest.approx(2000.0 / 3) and np.isnan(sc["clashes_per_1000_atoms"][2])
    per_atom = lddt.profile(res)
    assert per_atom["labels"].tolist() == [0, 2, 3] and per_atom["lddt"][0] == 20 / 32.0 and np.isnan(per_atom["lddt"][1])
    assert per_atom["lddt"][2] == 1.0 and per_atom["clashes"].tolist() == [1, 3, 0]
    grouped = lddt.profile(res, groups=np.array([7, 9, 7, 5]))      # atoms 0 and 2 are group 7, atom 3 is group 5
    assert grouped["labels"].tolist() == [5, 7] and grouped["included"].tolist() == [4, 8] and grouped["clashes"].tolist() == [0, 4]
    assert grouped["lddt"].tolist() == [1.0, 20 / 32.0]
    with pytest.raises(ValueError, match="groups lists"):
        lddt.profile(res, groups=np.array([0, 1]))


def test_compare_from_counts_keys_json_and_bad_structures():
    ref = _result([[4, 4, 4, 4, 4, 0], [4, 4, 4, 4, 4, 1]], [[8, 8, 8, 8, 8, 1], [4, 4, 4, 4, 4, 1], [4, 4, 4, 4, 4, 0]])
    gen = _result([[4, 0, 2, 4, 4, 3], [4, 4, 4, 4, 4, 0], [-1] * 6], [[8, 4, 6, 8, 8, 3], [4, 0, 2, 4, 4, 3], [4, 4, 4, 4, 4, 0]],
                  bad=[0, 0, 1])
    near = _result([[4, 2, 4, 4, 4, 0]], np.zeros((3, 6)))
    stats = lddt.compare_from_counts(ref, ref, gen, neighbour=near, params={"exclude": 3})
    assert tuple(stats) == lddt.LDDT_STATS_KEYS
    assert (stats["n_ref"], stats["n_gen"], stats["n_bad_ref"], stats["n_bad_gen"], stats["n_atoms"]) == (4, 3, 0, 1, 3)
    assert stats["lddt"]["mean"] == pytest.approx((10 / 16.0 + 1.0) / 2) and stats["lddt"]["min"] == 10 / 16.0
    assert sum(stats["lddt"]["hist"]["counts"]) == 2 and len(stats["lddt"]["hist"]["counts"]) == 50
    assert stats["preserved"] == [4 / 8.0, 6 / 8.0, 1.0, 1.0]
    assert stats["worst"][0] == {"label": 2, "lddt": 10 / 16.0} and [w["label"] for w in stats["worst"]] == [2, 0, 3]
    assert stats["lddt_profile"]["labels"] == [0, 2, 3] and stats["lddt_profile"]["clashes"] == [3, 3, 0]
    assert stats["clashes"]["mean_gen"] == 1.5 and stats["clashes"]["mean_ref"] == 0.5 and stats["clashes"]["floor"] == 0.0
    assert stats["clashes"]["hist_gen"]["counts"] == [1, 0, 0, 1] and stats["clashes"]["jsd"] > 0
    assert stats["clashing_pairs_per_atom"] == {"labels": [0, 2, 3], "ref": [0.5, 0.5, 0.0], "gen": [1.5, 1.5, 0.0]}
    assert stats["floor"]["lddt_neighbour"] == {"mean": 14 / 16.0, "std": 0.0, "min": 14 / 16.0} and stats["floor"]["clashes_jsd"] == 0.0
    assert json.loads(json.dumps(stats)) == stats
    short = lddt.summary_of(stats)
    assert set(short) == {"n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_atoms", "worst", "preserved", "floor", "lddt", "clashes"}
    assert set(short["lddt"]) == {"mean", "std", "min"} and set(short["clashes"]) == {"jsd", "mean_ref", "std_ref", "mean_gen", "std_gen"}
    grouped = lddt.compare_from_counts(ref, ref, gen, groups=np.array([7, 9, 7, 5]))
    assert grouped["lddt_profile"]["labels"] == [5, 7] and grouped["worst"][0]["label"] == 7 and grouped["floor"]["lddt_neighbour"] is None
    empty = _result([[-1] * 6], np.zeros((3, 6)), bad=[1])
    none = lddt.compare_from_counts(ref, ref, empty)
    assert none["lddt"] is None and none["clashes"] is None and none["preserved"] == [None] * 4 and none["worst"] == []
    assert none["lddt_profile"]["lddt"] == [None] * 3 and none["clashing_pairs_per_atom"]["gen"] is None
    json.dumps(none)
    assert lddt.summary_of(none)["lddt"] is None


# ----------------------------------------------------------------------------- command line
def _files(tmp_path, gen_shape=(4, 3)):
    z, bonds = DR.peptide(2)
    n = z.shape[0]
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "ref.npz", xyz=rng.normal(0, 3, (4, n, 3)).astype(np.float32), z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=rng.normal(0, 3, (*gen_shape, n, 3)).astype(np.float32))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}", n


def test_the_parser_and_read_inputs(tmp_path):
    base, n = _files(tmp_path)
    args = lddt.parser().parse_args(base.split())
    assert (args.lddt_atoms, args.lddt_groups, args.lddt_radius, args.lddt_exclude, args.clash_tolerance, args.native, args.scores,
            args.out) == ("heavy", "none", 15.0, 3, 0.4, None, None, "lddt_stats.json")
    inp = lddt.read_inputs(args)
    assert inp["gen_xyz"].shape == (12, n, 3) and inp["ref_index"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3] and inp["groups"] is None
    inp = lddt.read_inputs(lddt.parser().parse_args((base + " -native 2 -lddt_groups residue").split()))
    assert inp["ref_index"].tolist() == [2] * 12 and inp["groups"] == "residue"
    base, n = _files(tmp_path, gen_shape=(5,))
    assert lddt.read_inputs(lddt.parser().parse_args((base + " -native 0").split()))["ref_index"].tolist() == [0] * 5


def test_the_command_line_refuses_before_any_launch(tmp_path):
    base, n = _files(tmp_path)

    def refused(extra, match, line=None):
        with pytest.raises(SystemExit, match=match):
            lddt.read_inputs(lddt.parser().parse_args(((line or base) + " " + extra).split()))
    refused("-lddt_radius -1", "-lddt_radius")
    refused("-lddt_radius nan", "-lddt_radius")
    refused("-lddt_exclude -1", "-lddt_exclude")
    refused("-clash_tolerance -0.1", "-clash_tolerance")
    refused("-native 4", "-native 4")
    refused("-native -1", "-native -1")
    refused("-lddt_groups bead", "mapping")
    refused(f"-top {tmp_path / 'nothing.npz'}", "no such file")
    np.savez(tmp_path / "hydrogen.npz", z=np.ones(n, dtype=int), bonds=np.zeros((0, 2), dtype=int))
    refused(f"-top {tmp_path / 'hydrogen.npz'}", "selection is empty")
    np.savez(tmp_path / "carbon.npz", z=np.full(n, 6), bonds=np.zeros((0, 2), dtype=int))
    refused(f"-top {tmp_path / 'carbon.npz'} -lddt_groups residue", "need a peptide")
    flat, _ = _files(tmp_path, gen_shape=(12,))
    refused("", r"paired scoring needs \[T, K, n, 3\] with T = 4", line=flat)
    other, _ = _files(tmp_path, gen_shape=(3, 4))
    refused("", "paired scoring needs", line=other)
    with pytest.raises(SystemExit):
        lddt.parser().parse_args((base + " -lddt_atoms light").split())


# ----------------------------------------------------------------------------- library
NAMES = {"cgv_lddt_max_atoms", "cgv_lddt_max_structures", "cgv_lddt_max_references", "cgv_lddt_row_tile", "cgv_lddt_col_tile",
         "cgv_lddt_chunk", "cgv_lddt_workspace_bytes", "cgv_lddt_counts"}


def test_the_library_declares_binds_and_exports_the_lddt_kernel():
    assert NAMES <= set(_lib.header_symbols()) and NAMES <= set(_lib.PROTOTYPES)
    assert build.SOURCE_FLAGS["lddt.hip"] == ["-ffp-contract=off"]
    lim = lddt.limits()
    assert lim["atoms"] >= 2048 and lim["structures"] >= 4096 and lim["references"] >= 4096
    lib = _lib.load()
    assert lib.cgv_lddt_workspace_bytes(10, 3, 5) >= (10 + 3) * 5 * 16 and lib.cgv_lddt_workspace_bytes(10, 3, 5) % 16 == 0
    assert lib.cgv_lddt_workspace_bytes(10, 3, lim["atoms"] + 1) == 0 and lib.cgv_lddt_workspace_bytes(lim["structures"] + 1, 3, 5) == 0
    assert lib.cgv_lddt_workspace_bytes(10, lim["references"] + 1, 5) == 0 and lib.cgv_lddt_workspace_bytes(-1, 3, 5) == 0
    assert lib.cgv_lddt_row_tile() >= 1 and lib.cgv_lddt_col_tile() >= 32 and lib.cgv_lddt_chunk() >= 1


def test_the_c_entry_refuses_with_its_reason():
    lib, lim = _lib.load(), lddt.limits()
    index = np.array([0, 1, 5], dtype=np.int32)

    def call(S, T, m, radius2=225.0, t=(0.5, 1.0, 2.0, 4.0), tol=0.4, ref_index=None, rest=None):
        return lib.cgv_lddt_counts(rest, rest, ref_index, rest, rest, rest, rest, S, T, 1 << 20, m, radius2, *t, tol, rest, rest, rest, rest, 0, None)

    def refused(reason, *a, **kw):
        assert call(*a, **kw) == -1 and reason in lib.cgv_last_error_string(), lib.cgv_last_error_string()
    refused(b"cgv_lddt_max_atoms", 1, 1, lim["atoms"] + 1)
    refused(b"cgv_lddt_max_structures", lim["structures"] + 1, 1, 4)
    refused(b"cgv_lddt_max_references", 1, lim["references"] + 1, 4)
    refused(b"1 <= m", 1, 1, 0)
    refused(b"radius2", 1, 1, 4, radius2=float("nan"))
    refused(b"radius2", 1, 1, 4, radius2=-1.0)
    refused(b"threshold must be", 1, 1, 4, t=(0.5, 1.0, 2.0, float("inf")))
    refused(b"ascending", 1, 1, 4, t=(0.5, 2.0, 1.0, 4.0))
    refused(b"tolerance", 1, 1, 4, tol=float("nan"))
    refused(b"null pointer", 1, 1, 4)
    refused(b"at least one reference", 1, 0, 4)
    # every device pointer is a dummy that is never used: ref_index is a host array and is checked first
    dummy = index.ctypes.data
    refused(b"ref_index outside", 3, 5, 4, ref_index=dummy, rest=dummy)
    assert call(0, 0, 4) == 0                                        # nothing to do
