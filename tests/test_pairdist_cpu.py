"""Pair-distance distributions, host side: the numpy restatement against hand-computed values and against an independent
fp64 form, the conservation identity, the classes, the statistics on hand-made histograms, the command line's refusals and
the library's -- all without a device."""
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, build, pairdist
import pairdist_restatement as R

F = np.float32


# ----------------------------------------------------------------------------- the restatement
def _line(*xs):
    x = np.zeros((len(xs), 3), F)
    x[:, 0] = xs
    return x


def test_the_restatement_against_hand_computed_values():
    # r_max = 2, four bins of 0.5: scale = 2.  Classes 0, 1, 0: the pairs (0,1) and (1,2) are class pair 1, (0,2) is class pair 0
    xyz = np.stack([_line(0.0, 1.5, 2.0), _line(0.0, 0.75, 1.75)])
    cls, none = [0, 1, 0], np.eye(3, dtype=bool)
    assert R.scale_of(2.0, 4) == F(2.0) and R.rmax2_of(2.0) == F(4.0)
    w = R.pair_hist(xyz[:1], [0, 1, 2], cls, 2, none, 2.0, 4)
    # d01 = 1.5: 1.5 * 2 is exactly 3, the UPPER bin; d12 = 0.5: exactly 1; d02 = 2.0 is exactly r_max: beyond, the test is strict
    assert w["hist"].tolist() == [[0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 0, 0]] and w["beyond"].tolist() == [1, 0, 0]
    assert w["n_pairs"].tolist() == [1, 2, 0] and not w["bad"].any()
    ex = none.copy()
    ex[1, 2] = ex[2, 1] = True                                      # an excluded pair counts nowhere
    w = R.pair_hist(xyz[:1], [0, 1, 2], cls, 2, ex, 2.0, 4)
    assert w["hist"].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]] and w["beyond"].tolist() == [1, 0, 0]
    # second structure: d01 = 0.75 -> 1.5 -> bin 1, d12 = 1.0 -> exactly 2 -> bin 2, d02 = 1.75 -> 3.5 -> bin 3
    w = R.pair_hist(xyz, [0, 1, 2], cls, 2, none, 2.0, 4)
    assert w["hist"].tolist() == [[0, 0, 0, 1], [0, 2, 1, 1], [0, 0, 0, 0]] and w["beyond"].tolist() == [1, 0, 0]
    # a selection in another order, and an atom outside it
    w = R.pair_hist(np.stack([_line(9.0, 0.0, 1.5, 2.0)]), [3, 1], [1, 1], 2, np.eye(2, dtype=bool), 2.0, 4)
    assert w["hist"].sum() == 0 and w["beyond"].tolist() == [0, 0, 1]
    # one bin takes everything in range; a NaN in a selected atom makes the structure bad
    w = R.pair_hist(xyz, [0, 1, 2], [0, 0, 0], 1, none, 2.0, 1)
    assert w["hist"].tolist() == [[5]] and w["beyond"].tolist() == [1]
    broken = xyz.copy()
    broken[1, 2, 1] = np.nan
    w = R.pair_hist(broken, [0, 1, 2], [0, 0, 0], 1, none, 2.0, 1)
    assert w["bad"].tolist() == [False, True] and w["hist"].tolist() == [[2]] and w["beyond"].tolist() == [1]


@pytest.mark.parametrize("n,C,n_bins,r_max", [(40, 1, 100, 20.0), (130, 3, 100, 12.0), (97, 8, 256, 9.0)])
def test_the_restatement_against_an_independent_fp64_form(n, C, n_bins, r_max):
    rng = np.random.default_rng(n)
    xyz = R.chains(3, n, rng)
    cls = rng.integers(0, C, n)
    excl = R.band(n, 3)
    pairs = int(np.triu(~excl, 1).sum())
    dropped = 0
    for s in range(xyz.shape[0]):
        tie = R.near_tie(xyz[s], r_max, n_bins)
        dropped += int(np.triu(tie & ~excl, 1).sum())
        w = R.pair_hist(xyz[s:s + 1], np.arange(n), cls, C, excl | tie, r_max, n_bins)
        w64 = R.pair_hist64(xyz[s], cls, C, excl, r_max, n_bins, skip=tie)
        assert np.array_equal(w["hist"], w64["hist"]) and np.array_equal(w["beyond"], w64["beyond"])
        assert w["hist"].sum() > 0.3 * pairs and (w["hist"] > 0).sum() > n_bins // 4
    print(f"n = {n}: {dropped} of {pairs * xyz.shape[0]} pairs are near ties")
    assert dropped <= 0.01 * pairs * xyz.shape[0]                   # the condition of the comparison: from the fp64 form alone


def test_the_conservation_identity():
    rng = np.random.default_rng(3)
    n, C = 70, 4
    xyz = R.chains(5, n, rng)
    xyz[2, 11, 0] = np.inf
    cls = rng.integers(0, C, n)
    w = R.pair_hist(xyz, np.arange(n), cls, C, R.band(n, 2), 8.0, 50)
    assert w["bad"].tolist() == [False, False, True, False, False]
    assert w["beyond"].sum() > 0 and w["hist"].sum() > 0
    assert np.array_equal(w["hist"].sum(1) + w["beyond"], 4 * w["n_pairs"])
    assert w["n_pairs"].sum() == n * (n - 1) // 2 - (n - 1) - (n - 2)


# ----------------------------------------------------------------------------- classes
def test_classes_of_elements_none_labels_and_too_many():
    z = np.array([6, 1, 8, 7, 6, 1, 16, 8])
    sel = np.flatnonzero(z != 1)
    cls, names = pairdist.classes_of(z, sel, "element")
    assert names == ["C", "N", "O", "S"] and cls.tolist() == [0, 2, 1, 0, 3, 2] and cls.dtype == np.int32
    cls, names = pairdist.classes_of(z, sel, "none")
    assert names == ["all"] and cls.tolist() == [0] * 6
    cls, names = pairdist.classes_of(z, sel, np.array([40, 40, 7, 7, 40, 9, 9, 12]))
    assert names == ["7", "9", "12", "40"] and cls.tolist() == [3, 0, 0, 3, 1, 2]
    assert pairdist.pair_names_of(["C", "N"]) == ["C-C", "C-N", "N-N"]
    most = pairdist.limits()["classes"]
    many = np.arange(5, 5 + most + 1)
    with pytest.raises(ValueError, match=f"{most + 1} classes .*Z5, C, N, O.*the kernel holds {most}"):
        pairdist.classes_of(many, np.arange(most + 1), "element")
    assert len(pairdist.classes_of(many, np.arange(most), "element")[1]) == most
    with pytest.raises(ValueError, match="classes"):
        pairdist.classes_of(many, np.arange(most + 1), np.arange(most + 1))
    with pytest.raises(ValueError, match="one label for each"):
        pairdist.classes_of(z, sel, np.arange(3))
    with pytest.raises(ValueError, match="classes must be"):
        pairdist.classes_of(z, sel, "residue")


@pytest.mark.parametrize("C", [1, 2, 8])
def test_the_pair_class_index(C):
    want = {}
    for a in range(C):
        for b in range(a, C):
            want[(a, b)] = len(want)                                # row by row over the upper triangle
    assert len(want) == pairdist.n_pairs_of(C) == R.n_pairs_of(C) == C * (C + 1) // 2
    for (a, b), p in want.items():
        for f in (pairdist.pair_index, R.pair_index):
            assert int(f(np.int64(a), np.int64(b), C)) == p and int(f(np.int64(b), np.int64(a), C)) == p
    assert len(pairdist.pair_names_of(range(C))) == len(want)


# ----------------------------------------------------------------------------- statistics on hand-made histograms
def _result(hist, beyond=None, bad=(0, 0), r_max=4.0, names=("A",)):
    hist = np.asarray(hist, dtype=np.int64)
    hist = hist.reshape(-1, hist.shape[-1])
    bad = np.asarray(bad, dtype=bool)
    return {"hist": hist, "beyond": np.zeros(hist.shape[0], np.int64) if beyond is None else np.asarray(beyond, dtype=np.int64), "bad": bad,
            "n_good": int((~bad).sum()), "r_max": r_max, "n_bins": hist.shape[1], "sel": np.arange(3, dtype=np.int32),
            "class_names": list(names), "pair_names": pairdist.pair_names_of(names)}


def test_compare_from_counts_on_hand_made_histograms():
    even, odd = _result([0, 3, 5, 0, 1, 0, 0, 0]), _result([0, 3, 5, 0, 1, 0, 0, 0])
    same = pairdist.compare_from_counts(even, odd, _result([0, 6, 10, 0, 2, 0, 0, 0]))
    assert tuple(same) == pairdist.PAIRDIST_STATS_KEYS
    for block in (same["overall"], same["pairs"]["A-A"]):
        assert block["jsd"] == 0.0 and block["w1"] == 0.0 and block["floor"] == 0.0 and block["w1_floor"] == 0.0
        assert block["max_diff"]["value"] == 0.0 and block["mean_ref"] == block["mean_gen"]
    assert same["floor"] == {"jsd": 0.0, "w1": 0.0} and same["r"] == [0.25 + 0.5 * k for k in range(8)]
    shifted = pairdist.compare_from_counts(even, odd, _result([0, 0, 3, 5, 0, 1, 0, 0], bad=(0, 1, 0)))
    width = 4.0 / 8
    assert shifted["overall"]["w1"] == width and shifted["pairs"]["A-A"]["w1"] == width        # exactly the bin width
    assert shifted["overall"]["jsd"] > 0 and shifted["overall"]["mean_gen"] - shifted["overall"]["mean_ref"] == pytest.approx(width)
    assert shifted["overall"]["max_diff"] == {"value": 5 / 9.0, "bin": 3, "r": 1.75}      # the reference has nothing in bin 3
    assert (shifted["n_ref"], shifted["n_gen"], shifted["n_bad_ref"], shifted["n_bad_gen"], shifted["n_atoms"]) == (4, 3, 0, 1, 3)
    # two class pairs of three; the halves differ; a share beyond r_max
    names = ("C", "O")
    e = _result([[4, 0, 0, 0], [0, 2, 2, 0], [0, 0, 0, 0]], beyond=[4, 0, 1], names=names)
    o = _result([[2, 2, 0, 0], [0, 2, 2, 0], [0, 0, 0, 0]], beyond=[4, 0, 1], names=names)
    g = _result([[0, 0, 6, 0], [0, 1, 1, 0], [0, 0, 0, 0]], beyond=[0, 0, 0], names=names)
    st = pairdist.compare_from_counts(e, o, g, params={"n_bins": 4})
    assert list(st["pairs"]) == ["C-C", "C-O", "O-O"] == st["pair_names"] and st["class_names"] == ["C", "O"]
    cc, co, oo = (st["pairs"][k] for k in st["pair_names"])
    assert cc["floor"] > 0 and cc["w1_floor"] == 0.5 * 1.0 and cc["jsd"] == 1.0 and cc["beyond_ref"] == 0.5 and cc["beyond_gen"] == 0.0
    assert cc["w1"] == pytest.approx((6 / 8.0 + 1.0) * 1.0) and cc["max_diff"] == {"value": 1.0, "bin": 2, "r": 2.5}
    assert co["jsd"] == 0.0 and co["w1"] == 0.0 and co["n_pairs_ref"] == 8 and co["n_pairs_gen"] == 2
    assert oo["jsd"] is None and oo["w1"] is None and oo["max_diff"] is None and oo["mean_ref"] is None and oo["beyond_ref"] == 1.0
    assert oo["beyond_gen"] is None
    assert st["overall"]["n_pairs_ref"] == 16 and st["overall"]["hist_gen"] == [0, 1, 7, 0] and st["params"] == {"n_bins": 4}
    assert json.loads(json.dumps(st)) == st
    with pytest.raises(ValueError, match="different bins"):
        pairdist.compare_from_counts(even, odd, g)


def test_distribution_and_wasserstein_on_hand_made_histograms():
    d = pairdist.distribution(_result([[1, 1, 2, 0], [0, 0, 0, 0], [0, 0, 0, 4]], beyond=[4, 2, 0], names=("x", "y")))
    assert d["width"] == 1.0 and d["r"].tolist() == [0.5, 1.5, 2.5, 3.5]
    assert d["p"][0].tolist() == [0.25, 0.25, 0.5, 0.0] and np.isnan(d["p"][1]).all() and d["p"][2].tolist() == [0, 0, 0, 1.0]
    assert d["mean"][0] == 1.75 and np.isnan(d["mean"][1]) and d["beyond"].tolist() == [0.5, 1.0, 0.0] and d["n"].tolist() == [4, 0, 4]
    assert d["p_all"].tolist() == [0.125, 0.125, 0.25, 0.5] and d["n_all"] == 8 and d["beyond_all"] == 6 / 14.0
    assert d["mean_all"] == (0.5 + 1.5 + 5.0 + 14.0) / 8
    assert pairdist.wasserstein1([1, 0, 0], [0, 0, 1], 0.5) == 1.0 and pairdist.wasserstein1([0, 0], [1, 1], 1.0) is None
    assert pairdist.wasserstein1([10 ** 12, 10 ** 12], [3 * 10 ** 12, 10 ** 12], 2.0) == 2.0 * 0.25


def test_summary_of_keys():
    even = _result([0, 3, 5, 0])
    stats = pairdist.compare_from_counts(even, even, even)
    short = pairdist.summary_of(stats)
    assert set(short) == {"n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_atoms", "class_names", "pair_names", "floor", "overall", "pairs"}
    assert set(short["overall"]) == set(pairdist.BLOCK_SHORT) and "hist_ref" not in short["overall"]
    assert set(short["pairs"]["A-A"]) == {"jsd", "floor", "w1", "w1_floor"}
    json.dumps(short)


# ----------------------------------------------------------------------------- refusals
def test_every_value_error_comes_before_a_device_is_touched():
    n = 12
    z, bonds = np.full(n, 6), R.chain_bonds(n)
    xyz = np.zeros((4, n, 3), F)
    lim = pairdist.limits()

    def refused(match, x=xyz, zz=z, **kw):
        with pytest.raises(ValueError, match=match):
            pairdist.pair_hist(x, zz, bonds, **kw)
    refused("z lists", zz=z[:-1])
    refused(r"\[S, n, 3\]", x=np.zeros((4, n), F))
    for r_max in (0.0, -1.0, float("nan"), float("inf"), 1e-44, 1e30):
        refused("r_max", r_max=r_max)
    refused("n_bins must be", n_bins=0)
    refused("n_bins must be", n_bins=lim["bins"] + 1)
    refused("depth", exclude=-1)
    refused("atoms must be", atoms="light")
    refused("selection is empty", zz=np.ones(n, dtype=int))
    refused("classes", zz=np.arange(5, 5 + n))
    refused("structures_per_launch", structures_per_launch=lim["structures"] + 1)
    refused("structures_per_launch", structures_per_launch=0)
    big = lim["atoms"] + 1
    with pytest.raises(ValueError, match="the kernel holds"):
        pairdist.pair_hist(np.zeros((1, big, 3), F), np.full(big, 6), np.zeros((0, 2), int))
    eye = np.eye(n, dtype=bool)
    with pytest.raises(ValueError, match="symmetric"):
        pairdist.count_pairs(xyz, np.arange(n), np.zeros(n, int), 1, np.triu(np.ones((n, n), bool)))
    with pytest.raises(ValueError, match="n_classes must be"):
        pairdist.count_pairs(xyz, np.arange(n), np.zeros(n, int), lim["classes"] + 1, eye)
    with pytest.raises(ValueError, match="cls must be"):
        pairdist.count_pairs(xyz, np.arange(n), np.full(n, 2), 2, eye)
    with pytest.raises(ValueError, match="at least two reference frames"):
        pairdist.compare(xyz[:1], xyz, z, bonds)
    with pytest.raises(ValueError, match="mapping"):
        pairdist.compare(xyz, xyz, z, bonds, classes="bead")
    with pytest.raises(RuntimeError, match="device"):               # everything before the launch went through
        pairdist.pair_hist(xyz, z, bonds, device="cpu")


def _files(tmp_path, n=12):
    z, bonds = np.full(n, 6), R.chain_bonds(n)
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "ref.npz", xyz=R.chains(4, n, rng), z=z, bonds=bonds, mapping=np.arange(n) // 4)
    np.savez(tmp_path / "gen.npz", xyz=R.chains(6, n, rng).reshape(2, 3, n, 3))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}", n


def test_the_parser_and_read_inputs(tmp_path):
    base, n = _files(tmp_path)
    args = pairdist.parser().parse_args(base.split())
    assert (args.pd_atoms, args.pd_classes, args.pd_rmax, args.pd_bins, args.pd_exclude, args.out) == ("heavy", "element", 20.0, 100, 3,
                                                                                                        "pairdist_stats.json")
    inp = pairdist.read_inputs(args)
    assert inp["gen_xyz"].shape == (6, n, 3) and inp["ref_xyz"].shape == (4, n, 3) and inp["classes"] == "element" and inp["mapping"] is None
    inp = pairdist.read_inputs(pairdist.parser().parse_args((base + " -pd_classes bead -pd_bins 256").split()))
    assert inp["classes"] == "bead" and inp["mapping"].tolist() == (np.arange(n) // 4).tolist()


def test_the_command_line_refuses_before_any_launch(tmp_path):
    base, n = _files(tmp_path)

    def refused(extra, match):
        with pytest.raises(SystemExit, match=match):
            pairdist.read_inputs(pairdist.parser().parse_args((base + " " + extra).split()))
    refused("-pd_rmax 0", "-pd_rmax")
    refused("-pd_rmax -3", "-pd_rmax")
    refused("-pd_rmax nan", "-pd_rmax")
    refused("-pd_rmax inf", "-pd_rmax")
    refused("-pd_bins 0", "-pd_bins")
    refused("-pd_bins 257", "-pd_bins")
    refused("-pd_exclude -1", "-pd_exclude")
    np.savez(tmp_path / "beads.npz", z=np.full(n, 6), bonds=R.chain_bonds(n), mapping=np.arange(n))
    refused(f"-top {tmp_path / 'beads.npz'} -pd_classes bead", f"{n} classes .*the kernel holds 8")       # more beads than classes
    np.savez(tmp_path / "bare.npz", z=np.full(n, 6), bonds=R.chain_bonds(n))
    refused(f"-top {tmp_path / 'bare.npz'} -pd_classes bead", "mapping")
    np.savez(tmp_path / "hydrogen.npz", z=np.ones(n, dtype=int), bonds=np.zeros((0, 2), dtype=int))
    refused(f"-top {tmp_path / 'hydrogen.npz'}", "selection is empty")
    refused(f"-top {tmp_path / 'nothing.npz'}", "no such file")
    with pytest.raises(SystemExit):
        pairdist.parser().parse_args((base + " -pd_classes residue").split())


# ----------------------------------------------------------------------------- library
NAMES = {"cgv_pairdist_max_atoms", "cgv_pairdist_max_structures", "cgv_pairdist_max_classes", "cgv_pairdist_max_bins",
         "cgv_pairdist_row_tile", "cgv_pairdist_col_tile", "cgv_pairdist_chunk", "cgv_pairdist_workspace_bytes", "cgv_pairdist_counts"}


def test_the_library_declares_binds_and_exports_the_pair_distance_kernel():
    assert NAMES <= set(_lib.header_symbols()) and NAMES <= set(_lib.PROTOTYPES)
    assert build.SOURCE_FLAGS["pair_hist.hip"] == ["-ffp-contract=off"]
    lim = pairdist.limits()
    assert lim["atoms"] >= 2048 and lim["structures"] >= 4096 and lim["classes"] == 8 and lim["bins"] == 256
    lib = _lib.load()
    assert lib.cgv_pairdist_workspace_bytes(10, 5) >= 10 * 5 * 16 and lib.cgv_pairdist_workspace_bytes(10, 5) % 16 == 0
    assert lib.cgv_pairdist_workspace_bytes(10, lim["atoms"] + 1) == 0 and lib.cgv_pairdist_workspace_bytes(lim["structures"] + 1, 5) == 0
    assert lib.cgv_pairdist_workspace_bytes(-1, 5) == 0
    rt, ct, ch = lib.cgv_pairdist_row_tile(), lib.cgv_pairdist_col_tile(), lib.cgv_pairdist_chunk()
    assert rt >= 1 and ct >= 32 and ct % 32 == 0 and ch >= 1
    assert rt * ct * lim["structures"] <= 2 ** 31                  # the overflow bound of the kernel's header


def test_the_c_entry_refuses_with_its_reason():
    lib, lim = _lib.load(), pairdist.limits()

    def call(S, m, C=2, n_bins=100, rmax2=400.0, scale=5.0):
        return lib.cgv_pairdist_counts(None, None, None, None, S, 1 << 20, m, C, n_bins, rmax2, scale, None, None, None, None, 0, None)

    def refused(reason, *a, **kw):
        assert call(*a, **kw) == -1 and reason in lib.cgv_last_error_string(), lib.cgv_last_error_string()
    refused(b"cgv_pairdist_max_atoms", 1, lim["atoms"] + 1)
    refused(b"cgv_pairdist_max_structures", lim["structures"] + 1, 4)
    refused(b"cgv_pairdist_max_classes", 1, 4, C=lim["classes"] + 1)
    refused(b"cgv_pairdist_max_classes", 1, 4, C=0)
    refused(b"cgv_pairdist_max_bins", 1, 4, n_bins=lim["bins"] + 1)
    refused(b"cgv_pairdist_max_bins", 1, 4, n_bins=0)
    refused(b"1 <= m", 1, 0)
    refused(b"rmax2", 1, 4, rmax2=float("nan"))
    refused(b"rmax2", 1, 4, rmax2=float("inf"))
    refused(b"scale", 1, 4, scale=0.0)
    refused(b"scale", 1, 4, scale=float("nan"))
    refused(b"null pointer", 1, 4)
    assert call(0, 4) == 0                                           # nothing to do
