"""Secondary structure, host side: the tables of ``dssp.backbone_table``, the numpy restatement of the assignment against
its own fp64 form and on built helices and sheets, the statistics of ``compare_from_counts`` on hand-made counts, every
refusal that needs no device, and the library's symbols."""
import math

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, dssp
import dssp_restatement as R


def _assign(z, bonds, xyz):
    t = dssp.backbone_table(z, bonds)
    x = np.asarray(xyz, dtype=np.float32)
    return R.assign(x[None] if x.ndim == 2 else x, t["res"], t["prev"], t["link"]), t


# ----------------------------------------------------------------------------- tables
def test_the_table_of_a_capped_peptide():
    z, bonds = R.peptide(3, cap=True)                          # CH3 C O | N CA C O x 3 | N CH3
    t = dssp.backbone_table(z, bonds)
    assert t["res"].tolist() == [[3, 4, 5, 6], [7, 8, 9, 10], [11, 12, 13, 14]]
    assert t["prev"].tolist() == [[1, 2], [5, 6], [9, 10]]     # the acetyl counts, although it is no residue
    assert t["link"].tolist() == [1, 1, 0]
    assert all(t[k].dtype == np.int32 for k in ("res", "prev", "link"))
    z, bonds = R.peptide(3)                                    # no caps: the last C has no N and is no amide carbon
    t = dssp.backbone_table(z, bonds)
    assert t["res"].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]] and t["prev"].tolist() == [[-1, -1], [2, 3]] and t["link"].tolist() == [1, 0]


def test_a_nitrogen_with_three_heavy_neighbours_never_donates():
    z, bonds = R.peptide(3, cap=True)
    z, bonds = np.concatenate([z, [6, 1]]), np.concatenate([bonds, [[7, len(z)], [11, len(z) + 1]]])   # a CD on N of residue 1; an H on N of 2
    t = dssp.backbone_table(z, bonds)
    assert t["prev"].tolist() == [[1, 2], [-1, -1], [9, 10]] and t["link"].tolist() == [1, 1, 0]


def test_two_chains_and_residues_listed_against_the_chain():
    z1, b1 = R.peptide(3, cap=True)
    z, bonds = np.concatenate([z1, z1]), np.concatenate([b1, b1 + len(z1)])
    t = dssp.backbone_table(z, bonds)
    assert t["res"][:, 0].tolist() == [3, 7, 11, 20, 24, 28] and t["link"].tolist() == [1, 1, 0, 1, 1, 0]
    assert t["prev"][3].tolist() == [18, 19]
    flip = np.arange(len(z1))[::-1]                            # atom k becomes atom n - 1 - k: the N of the last residue comes first
    t = dssp.backbone_table(z1[::-1], flip[b1])
    assert t["res"].tolist() == [[flip[a] for a in row] for row in [[3, 4, 5, 6], [7, 8, 9, 10], [11, 12, 13, 14]]]
    assert t["prev"].tolist() == [[flip[1], flip[2]], [flip[5], flip[6]], [flip[9], flip[10]]] and t["link"].tolist() == [1, 1, 0]


def test_a_cyclic_backbone_and_a_molecule_without_one_are_refused():
    z, bonds = R.peptide(4)
    ring = np.concatenate([bonds, [[14, 0]]])                  # the last C to the first N
    with pytest.raises(ValueError, match="cyclic"):
        dssp.backbone_table(z, ring)
    with pytest.raises(ValueError, match="no peptide backbone"):
        dssp.backbone_table(np.array([6, 6, 8, 1]), np.array([(0, 1), (1, 2), (2, 3)]))
    with pytest.raises(ValueError, match="no peptide backbone"):
        dssp.assign(np.zeros((2, 4, 3), np.float32), np.array([6, 6, 8, 1]), np.array([(0, 1), (1, 2), (2, 3)]))


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n_res,S,seed", [(10, 400, 0), (40, 40, 1), (129, 6, 2)])
def test_fp32_and_fp64_disagree_on_near_ties_only(n_res, S, seed):
    z, bonds, xyz = R.random_chains(n_res, S, seed)
    got, t = _assign(z, bonds, xyz)
    want = R.hbonds64(xyz, t["res"], t["prev"])
    tie = R.near_tie(xyz, t["res"], t["prev"])
    assert tie.mean() <= 0.01                                  # the seeds are chosen so: else the next line says little
    assert not ((got["hb"] != want) & ~tie).any()
    assert 0.01 <= got["hb"].sum() / got["inside"].sum() <= 0.5


@pytest.mark.parametrize("kind,letter", [(R.ALPHA, "H"), (R.HELIX_310, "G"), (R.PI_HELIX, "I")])
def test_ideal_helices(kind, letter):
    # 14 residues either way (without caps the last C is no amide carbon and its residue none): every bond i -> i + n is
    # there, every residue from 1 is covered by a start a >= 1, and the last start is 13 - n, which reaches residue 12
    for cap, n_res in ((True, 14), (False, 15)):
        z, bonds = R.peptide(n_res, cap)
        got, t = _assign(z, bonds, R.ideal(kind, n_res, cap))
        assert R.strings(got["codes"]) == ["-" + letter * 12 + "-"], (cap, R.strings(got["codes"]))
        n = {"G": 3, "H": 4, "I": 5}[letter]
        assert got["parts"]["turn"][n - 3, 0, :14 - n].all()      # every i -> i + n bond of the helix
        assert got["n_class"].sum() == 14 and got["class_counts"].sum() == 14 and not got["bad"].any()


def test_a_two_strand_sheet_and_an_isolated_bridge():
    for pose, want, ladder in (("anti", "--EEE---EEE-", "ladder_anti"), ("par", "-EEEE--EEEE-", "ladder_par")):
        z, bonds, xyz = R.two_strands(pose)
        got, t = _assign(z, bonds, xyz)
        assert t["link"].tolist() == [1] * 5 + [0] + [1] * 5 + [0]
        assert R.strings(got["codes"]) == [want] and got["parts"][ladder].any()
        other = "ladder_par" if ladder == "ladder_anti" else "ladder_anti"
        assert not got["parts"][other].any()
    got, _ = _assign(*R.two_strands("bridge"))
    assert R.strings(got["codes"]) == ["----B---B---"]
    assert got["parts"]["anti"].sum() == 2 and not got["parts"]["ladder_anti"].any() and not got["parts"]["par"].any()


def test_the_restatement_marks_bad_structures_and_packs_bits():
    z, bonds, xyz = R.random_chains(70, 4, 3)
    xyz = np.array(xyz)
    xyz[1, 4, 0] = np.nan                                      # the CA of the first residue
    xyz[2, 2, 1] = np.inf                                      # the acetyl's O: a prev atom
    got, t = _assign(z, bonds, xyz)
    assert got["bad"].tolist() == [False, True, True, False] and got["n_good"] == 2
    assert (got["n_class"][[1, 2]] == -1).all() and (got["codes"][[1, 2]] == 255).all() and not got["hb_bits"][[1, 2]].any()
    assert got["hb_bits"].shape == (4, 70, 2) and not (got["hb_bits"][:, :, 1] >> np.uint64(6)).any()
    assert (got["n_class"][[0, 3]].sum(axis=1) == 70).all() and got["class_counts"].sum() == 140
    assert R.strings(got["codes"])[1] == "?" * 70 == dssp.strings(got["codes"])[1]
    assert dssp.strings(got["codes"]) == R.strings(got["codes"])


# ----------------------------------------------------------------------------- host statistics
def _result(codes):
    """A result of ``assign`` from rows of class letters; a row of ``?`` is a bad structure."""
    c = np.array([[255 if ch == "?" else dssp.CODES.index(ch) for ch in row] for row in codes], dtype=np.uint8)
    bad = (c == 255).all(axis=1)
    n_class = np.stack([(c == k).sum(axis=1) for k in range(8)], axis=1).astype(np.int64)
    n_class[bad] = -1
    return {"class_counts": np.stack([(c[~bad] == k).sum(axis=0) for k in range(8)], axis=1).astype(np.int64), "n_class": n_class,
            "bad": bad, "n_good": int((~bad).sum()), "codes": c}


def test_propensity_reduce3_and_strings():
    res = _result(["HHE-", "HGB-", "????", "TIES"])
    p = dssp.propensity(res)
    assert p.shape == (4, 8) and p[0].tolist() == [2 / 3, 0, 0, 0, 0, 1 / 3, 0, 0] and np.allclose(p.sum(axis=1), 1.0)
    assert dssp.reduce3(p)[1].tolist() == pytest.approx([1.0, 0.0, 0.0]) and dssp.reduce3(p)[2].tolist() == pytest.approx([0.0, 1.0, 0.0])
    assert dssp.strings(res["codes"]) == ["HHE-", "HGB-", "????", "TIES"]
    assert dssp.propensity(_result(["????"])) is None


def test_compare_from_counts_on_hand_made_counts():
    even, odd = _result(["HHHHEE--", "HHHHEE--", "????????"]), _result(["HHHHEE--", "GGG-EE-S"])
    gen = _result(["HHHH----", "HHHH---T", "-HHH-B--", "HHHH----"])
    stats = dssp.compare_from_counts(even, odd, gen)
    assert set(stats) == set(dssp.DSSP_STATS_KEYS)
    assert (stats["n_ref"], stats["n_gen"], stats["n_bad_ref"], stats["n_bad_gen"], stats["R"]) == (5, 4, 1, 0, 8)
    assert stats["consensus_ref"] == "HHHHEE--"
    assert stats["agreement_ref"] == pytest.approx((8 + 8 + 8 + 7) / 32.0) and stats["agreement_gen"] == pytest.approx((6 + 6 + 6 + 6) / 32.0)       # B counts as strand
    assert stats["lost"] == [[4, "E"]] and stats["gained"] == []           # residue 5 keeps a quarter of its strand: not lost
    p_ref, p_gen = np.array(stats["propensity_ref"]), np.array(stats["propensity_gen"])
    assert p_ref.shape == (8, 8) and p_ref[0].tolist() == [0.75, 0, 0, 0.25, 0, 0, 0, 0] and p_gen[5, 1] == 0.25
    assert np.array(stats["propensity3_ref"])[0].tolist() == [1.0, 0.0, 0.0]
    assert stats["propensity_rmse"] == pytest.approx(math.sqrt(np.mean((p_ref - p_gen) ** 2)))
    assert stats["floor"]["propensity_rmse"] == pytest.approx(math.sqrt(np.mean((dssp.propensity(even) - dssp.propensity(odd)) ** 2)))
    assert stats["helix_fraction"]["mean_ref"] == pytest.approx((0.5 * 3 + 3 / 8) / 4) and stats["helix_fraction"]["mean_gen"] == pytest.approx(15 / 32)
    assert stats["helix_fraction"]["hist_ref"]["counts"] == [0, 0, 0, 1, 3, 0, 0, 0, 0] and stats["strand_fraction"]["hist_gen"]["counts"][:2] == [3, 1]
    same = dssp.compare_from_counts(gen, gen, gen)
    assert same["propensity_rmse"] == 0.0 and same["floor"]["propensity_rmse"] == 0.0 and same["lost"] == same["gained"] == []
    assert same["helix_fraction"]["jsd"] == 0.0 and same["agreement_ref"] == same["agreement_gen"]
    swapped = dssp.compare_from_counts(gen, gen, even)
    assert swapped["gained"] == [[4, "E"]] and swapped["lost"] == []        # residue 5 has a quarter of strand in the reference
    short = dssp.summary_of(stats)
    assert set(short) == {"n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "R", "propensity_rmse", "floor", "consensus_ref", "agreement_ref",
                          "agreement_gen", "n_lost", "n_gained", "helix_fraction", "strand_fraction"}
    assert short["n_lost"] == 1 and short["n_gained"] == 0 and set(short["helix_fraction"]) == {"jsd", "mean_ref", "std_ref", "mean_gen", "std_gen"}
    empty = _result(["????????"])
    none = dssp.compare_from_counts(even, odd, empty)
    assert none["propensity_rmse"] is None and none["lost"] is None and none["agreement_gen"] is None and none["helix_fraction"] is None
    assert none["agreement_ref"] is not None and dssp.summary_of(none)["n_lost"] is None


# ----------------------------------------------------------------------------- refusals before any launch
def test_every_value_error_comes_before_a_device_is_touched():
    z, bonds = R.peptide(3, cap=True)
    xyz = np.zeros((4, len(z), 3), np.float32)

    def refused(match, frames=xyz, z=z, bonds=bonds):
        with pytest.raises(ValueError, match=match):
            dssp.assign(frames, z, bonds)
    refused("z lists 16 atoms", z=z[:16])
    refused("bonds name atom", bonds=np.array([(0, 17)]))
    refused(r"\[S, n, 3\]", frames=np.zeros((4, len(z)), np.float32))
    refused("no peptide backbone", bonds=bonds[:3])
    lim = dssp.limits()
    big_z, big_bonds = R.peptide(lim["residues"] + 1, cap=True)
    refused("the kernel holds", frames=np.zeros((1, len(big_z), 3), np.float32), z=big_z, bonds=big_bonds)
    with pytest.raises(ValueError, match="at least two reference frames"):
        dssp.compare(xyz[:1], xyz, z, bonds)
    with pytest.raises(ValueError, match="z lists"):
        dssp.compare(xyz, xyz[:, :16], z, bonds)


def _files(tmp_path):
    z, bonds = R.peptide(3, cap=True)
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "ref.npz", xyz=rng.normal(0, 2, (4, len(z), 3)).astype(np.float32), z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=rng.normal(0, 2, (2, 3, len(z), 3)).astype(np.float32))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}", z, bonds


def test_the_parser_and_read_inputs(tmp_path):
    base, z, bonds = _files(tmp_path)
    args = dssp.parser().parse_args(base.split())
    assert (args.codes, args.out, args.top, args.device) == (None, "dssp_stats.json", None, "cuda")
    inp = dssp.read_inputs(args)
    assert inp["ref_xyz"].shape == (4, 17, 3) and inp["gen_xyz"].shape == (6, 17, 3) and inp["z"].tolist() == z.tolist()
    args = dssp.parser().parse_args((base + " -codes c.npz -out x.json").split())
    assert (args.codes, args.out) == ("c.npz", "x.json")


def test_the_command_line_refuses_before_any_launch(tmp_path):
    base, z, bonds = _files(tmp_path)

    def refused(extra, match):
        with pytest.raises(SystemExit, match=match):
            dssp.read_inputs(dssp.parser().parse_args((base + " " + extra).split()))
    refused(f"-top {tmp_path / 'nothing.npz'}", "no such file")
    np.savez(tmp_path / "other.npz", z=[6, 6], bonds=[[0, 1]])
    refused(f"-top {tmp_path / 'other.npz'}", "the topology has 2 atoms")
    np.savez(tmp_path / "carbon.npz", z=np.full(len(z), 6), bonds=bonds)
    refused(f"-top {tmp_path / 'carbon.npz'}", "no peptide backbone")
    ring_z, ring_bonds = R.peptide(4)
    np.savez(tmp_path / "ring.npz", z=np.concatenate([ring_z, [6]]), bonds=np.concatenate([ring_bonds, [[14, 0]]]))
    refused(f"-top {tmp_path / 'ring.npz'}", "cyclic")
    np.savez(tmp_path / "bare.npz", xyz=np.zeros((4, 17, 3), np.float32))
    with pytest.raises(SystemExit, match="z / bonds"):
        dssp.read_inputs(dssp.parser().parse_args(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'bare.npz'}".split()))
    np.savez(tmp_path / "short.npz", xyz=np.zeros((1, 17, 3), np.float32), z=z, bonds=bonds)
    with pytest.raises(SystemExit, match="at least two"):
        dssp.read_inputs(dssp.parser().parse_args(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'short.npz'}".split()))
    np.savez(tmp_path / "wide.npz", xyz=np.zeros((3, 18, 3), np.float32))
    with pytest.raises(SystemExit, match="wide.npz: xyz is"):
        dssp.read_inputs(dssp.parser().parse_args(f"-gen {tmp_path / 'wide.npz'} -ref {tmp_path / 'ref.npz'}".split()))
    with pytest.raises(SystemExit):
        dssp.parser().parse_args(["-gen", "a.npz"])                            # -ref is required


# ----------------------------------------------------------------------------- library
def test_the_library_declares_binds_and_exports_the_secondary_structure_kernel():
    names = {"cgv_dssp_max_residues", "cgv_dssp_max_structures", "cgv_dssp_wave_path_max", "cgv_dssp_bend_c2", "cgv_dssp_assign"}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.PROTOTYPES)
    lim = dssp.limits()
    lib = _lib.load()
    assert lim["residues"] >= 256 and lim["structures"] >= 4096 and 1 <= lib.cgv_dssp_wave_path_max() <= 64 < lim["residues"]
    assert np.float32(lib.cgv_dssp_bend_c2()) == R.BEND_C2     # the one constant the kernel cannot spell as a decimal


def test_the_c_entry_refuses_a_peptide_past_a_limit_with_its_reason():
    lib, lim = _lib.load(), dssp.limits()

    def refused(S, n_res, reason):
        rc = lib.cgv_dssp_assign(None, None, None, None, S, 10, n_res, None, None, None, None, None, None)
        assert rc == -1 and reason in lib.cgv_last_error_string(), lib.cgv_last_error_string()
    refused(1, lim["residues"] + 1, b"cgv_dssp_max_residues")
    refused(lim["structures"] + 1, 4, b"cgv_dssp_max_structures")
    refused(1, 0, b"at least one")
    refused(1, 4, b"null pointer")
    assert lib.cgv_dssp_assign(None, None, None, None, 0, 10, 4, None, None, None, None, None, None) == 0      # nothing to do
