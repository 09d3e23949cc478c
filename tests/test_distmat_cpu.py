"""Distance-matrix statistics without a device: the numpy restatement of K30 (csrc/dist_moments.hip) against hand-computed
values and an independent fp64 form, within bounds derived from u = 2^-24; the host reductions of ``distmat.compare`` on
hand-made tables; the command line's parser and refusals."""
import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, build, distmat
import distmat_restatement as R

F = np.float32
NAMES = {"cgv_dist_moments", "cgv_dist_moments_workspace_bytes", "cgv_dist_moments_max_atoms", "cgv_dist_moments_max_structures",
         "cgv_dist_moments_max_total", "cgv_dist_moments_row_tile", "cgv_dist_moments_col_tile", "cgv_dist_moments_chunk"}


# ----------------------------------------------------------------------------- the restatement
def test_the_restatement_against_hand_computed_values():
    tri = np.array([[[0, 0, 0], [3, 0, 0], [0, 4, 0]]], F)                     # 3-4-5
    got = R.moments(tri, [0, 1, 2])
    d = np.array([[0, 3, 4], [3, 0, 5], [4, 5, 0]])
    assert np.array_equal(got["sum_e"], d * 2 ** 20) and np.array_equal(got["sum_e2"], d * d * 2 ** 20)
    assert got["dev2"].tolist() == [50 * 2 ** 12] and got["bad"].tolist() == [False] and (got["n_good"], got["n_pairs"]) == (1, 3)
    # a pair exactly at its centre adds nothing; the others their deviation: 4 - 4.5 = -0.5, 5 - 3 = 2
    ctr = np.array([[0, 3, 4.5], [3, 0, 3], [4.5, 3, 0]], F)
    got = R.moments(np.concatenate([tri, tri]), [0, 1, 2], ctr)
    assert np.array_equal(got["sum_e"], 2 * np.array([[0, 0, -0.5], [0, 0, 2], [-0.5, 2, 0]]) * 2 ** 20)
    assert np.array_equal(got["sum_e2"], 2 * np.array([[0, 0, 0.25], [0, 0, 4], [0.25, 4, 0]]) * 2 ** 20)
    assert got["dev2"].tolist() == [int(4.25 * 2 ** 12)] * 2
    # a mask leaves a pair out of all three sums; rint is ties-to-even: e = 2^-21 and 3 * 2^-21 round to 0 and 2
    mask = np.zeros((3, 3), bool)
    mask[0, 1] = mask[1, 0] = True
    got = R.moments(tri, [0, 1, 2], None, mask)
    assert got["sum_e"][0, 1] == 0 and got["sum_e2"][1, 0] == 0 and got["dev2"].tolist() == [41 * 2 ** 12] and got["n_pairs"] == 2
    ties = np.array([[[0, 0, 0], [2.0 ** -21, 0, 0]], [[0, 0, 0], [3 * 2.0 ** -21, 0, 0]]], F)
    assert R.moments(ties[:1], [0, 1])["sum_e"][0, 1] == 0 and R.moments(ties[1:], [0, 1])["sum_e"][0, 1] == 2
    # bad: a NaN, an infinity, an atom more than 512 A from the centroid (of two atoms: 1025 A apart); 1023 A apart is good
    far = np.array([[[0, 0, 0], [1025, 0, 0]], [[0, 0, 0], [1023, 0, 0]], [[np.nan, 0, 0], [1, 0, 0]], [[0, 0, 0], [1, np.inf, 0]]], F)
    got = R.moments(far, [0, 1])
    assert got["bad"].tolist() == [True, False, True, True] and got["sum_e"][0, 1] == 1023 * 2 ** 20 and got["dev2"].tolist() == [0, 1023 ** 2 * 2 ** 12, 0, 0]


@pytest.mark.parametrize("S,m,seed", [(5, 7, 0), (33, 20, 1)])
def test_the_restatement_against_an_independent_fp64_form(S, m, seed):
    xyz = R.cloud(S, m + 2, np.random.default_rng(seed))
    sel = np.arange(1, m + 1)
    d64, mean64, std64 = R.maps64(xyz, sel)
    d_max = d64.max()
    for s in range(S):
        d32, _, _ = R.terms(xyz[s, sel], np.zeros((m, m), F))
        assert (np.abs(d32.astype(np.float64) - d64[s]) <= 4.0 * R.U * d64[s]).all()          # |d32 - d64| <= 4 u d
    mean, std, dr, ctr = R.mean_std(xyz, sel)
    off = ~np.eye(m, dtype=bool)
    # |mean - mean64| <= 4 u d_max + 2^-21: the distance error of every term, and half a unit of the 2^-20 fixed point
    assert (np.abs(mean - mean64)[off] <= R.mean_bound(d_max)).all()
    # |std - std64| <= 4 u d_max + root_change(std64^2, eta), eta as derived in distmat_restatement.std_bound
    assert (np.abs(std - std64)[off] <= R.std_bound(std64, d_max)[off]).all()
    # the distance RMSD to the centre map: 4 u d_max + root_change(drmsd64^2, u (drmsd64 + a)^2 + 2^-13)
    iu = np.triu_indices(m, 1)
    dr64 = np.sqrt(((d64 - ctr.astype(np.float64)[None]) ** 2)[:, iu[0], iu[1]].mean(1))
    assert (np.abs(dr - dr64) <= R.drmsd_bound(dr64, d_max)).all()
    assert R.std_bound(std64, d_max)[off].max() < 2e-3 and R.mean_bound(d_max) < 2e-5                # the bounds say something


def test_the_second_pass_removes_the_cancellation_at_fifty_angstrom():
    """A pair 50 A apart that jitters by 0.01 A: the two-pass standard deviation is within the derived bound, the one-pass
    form ``sqrt(<d^2> - <d>^2)`` is not -- it rounds d^2 near 2500 to fp32 (half an ulp: 1.2e-4, the size of the variance)."""
    rng = np.random.default_rng(5)
    S = 4
    xyz = np.zeros((S, 2, 3), F)
    xyz[:, 1, 0] = (50.0 + 0.01 * rng.standard_normal(S)).astype(F)
    _, _, std64 = R.maps64(xyz, [0, 1])
    _, std, _, _ = R.mean_std(xyz, [0, 1])
    bound = float(R.std_bound(std64, 50.1)[0, 1])
    assert 0.003 < std64[0, 1] < 0.03 and bound < 1e-3
    assert abs(std[0, 1] - std64[0, 1]) <= bound
    assert abs(R.one_pass_std(xyz, [0, 1])[0, 1] - std64[0, 1]) > bound


# ----------------------------------------------------------------------------- host reductions
def _maps(mean, std, m=4, drmsd=(), bad=()):
    """A result of ``mean_std`` by hand: the upper triangles ``mean`` / ``std`` (six numbers for m = 4) made symmetric."""
    iu = np.triu_indices(m, 1)
    out = {}
    for name, v in (("mean", mean), ("std", std)):
        a = np.zeros((m, m))
        a[iu] = v
        out[name] = a + a.T
    return {**out, "counted": ~np.eye(m, dtype=bool), "sel": np.arange(10, 10 + m), "drmsd": np.asarray(drmsd, float),
            "drmsd_ref": np.asarray(drmsd, float), "bad": np.asarray(bad, bool)}


def test_compare_from_moments_on_hand_made_tables():
    # pairs in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    ref = _maps([1, 2, 3, 4, 5, 6], [.1, .2, .3, .4, .5, .6])
    even = _maps([1, 2, 3, 4, 5, 6.5], [.1, .2, .3, .4, .5, .6], drmsd=[0.1, 0.2], bad=[False, False])
    odd = _maps([1, 2, 3, 4, 5, 5.5], [.1, .2, .3, .4, .7, .6], drmsd=[0.1, np.nan], bad=[False, True])
    gen = _maps([1, 2.5, 3, 2, 5.25, 7], [.1, .2, .3, .4, .5, .3], bad=[False] * 3)
    st = distmat.compare_from_moments(even, odd, ref, gen, [0.1, 0.9, 0.9], params={"k": 1})
    assert tuple(st) == distmat.DISTMAT_STATS_KEYS
    assert (st["n_ref"], st["n_gen"], st["n_bad_ref"], st["n_bad_gen"], st["n_atoms"], st["n_pairs"]) == (4, 3, 1, 0, 4, 6) and st["params"] == {"k": 1}
    assert st["ens_drms"] == pytest.approx(np.sqrt((0.25 + 4 + 0.0625 + 1) / 6), rel=1e-14)
    assert st["fluct_drms"] == pytest.approx(np.sqrt(0.09 / 6), rel=1e-12)
    assert st["floor"]["ens_drms"] == pytest.approx(np.sqrt(1.0 / 6), rel=1e-14)           # even against odd: 6.5 against 5.5
    assert st["floor"]["fluct_drms"] == pytest.approx(np.sqrt(0.04 / 6), rel=1e-12)
    sr, sg = np.array([.1, .2, .3, .4, .5, .6]), np.array([.1, .2, .3, .4, .5, .3])
    assert st["std_corr"] == pytest.approx(np.corrcoef(sr, sg)[0, 1], rel=1e-12) and 0 < st["floor"]["std_corr"] < 1
    # the five worst pairs, largest first; the unchanged pair (0, 1) / (0, 3) tie at 0: the first of them is the fifth
    assert [(w["i"], w["j"]) for w in st["worst_mean"]] == [(1, 2), (2, 3), (0, 2), (1, 3), (0, 1)]
    first = st["worst_mean"][0]
    assert (first["a"], first["b"], first["ref"], first["gen"], first["diff"]) == (11, 12, 4.0, 2.0, -2.0)
    assert (st["worst_std"][0]["i"], st["worst_std"][0]["j"]) == (2, 3) and st["worst_std"][0]["diff"] == pytest.approx(-0.3)
    assert len(st["worst_std"]) == 5 and st["groups"] is None
    # the reference's distance RMSD to its own map against the generated structures': a histogram block with a floor
    assert st["drmsd"]["mean_ref"] == pytest.approx((0.1 + 0.2 + 0.1) / 3) and st["drmsd"]["mean_gen"] == pytest.approx(1.9 / 3)
    assert st["drmsd"]["jsd"] > 0 and st["drmsd"]["floor"] is not None and st["drmsd"]["range"] == [0.0, 0.9]
    # an ensemble against itself
    same = distmat.compare_from_moments(even, odd, ref, ref, [0.1, 0.2, 0.1])
    assert same["ens_drms"] == 0.0 and same["fluct_drms"] == 0.0 and same["std_corr"] == pytest.approx(1.0) and same["floor"]["ens_drms"] > 0


def test_group_averaging_and_masked_pairs():
    ref = _maps([1, 2, 3, 4, 5, 6], [.1, .2, .3, .4, .5, .6])
    gen = _maps([1, 3, 3, 4, 7, 6], [.1, .2, .3, .4, .5, .6], bad=[False])
    half = _maps([1, 2, 3, 4, 5, 6], [.1, .2, .3, .4, .5, .6], drmsd=[0.1], bad=[False])
    # groups {0, 1} and {2, 3}: the one pair of groups averages (0,2) (0,3) (1,2) (1,3)
    mean, std, ids = distmat.group_maps(ref["mean"], ref["std"], ref["counted"], [7, 7, 9, 9])
    assert ids.tolist() == [7, 9] and mean[0, 1] == mean[1, 0] == pytest.approx(3.5) and std[0, 1] == pytest.approx(0.35) and np.isnan(mean[0, 0])
    st = distmat.compare_from_moments(half, half, ref, gen, [0.5], groups=[7, 7, 9, 9])
    g = st["groups"]
    assert (g["n_groups"], g["ids"], g["n_pairs"]) == (2, [7, 9], 1)
    assert g["ens_drms"] == pytest.approx(0.75) and g["fluct_drms"] == 0.0 and g["std_corr"] is None and g["floor"]["ens_drms"] == 0.0
    assert [(w["i"], w["j"], w["a"], w["b"]) for w in g["worst_mean"]] == [(0, 1, 7, 9)] and g["worst_mean"][0]["diff"] == pytest.approx(0.75)
    # a masked atom pair leaves the average: without (1, 3) the group pair averages 2, 3, 4
    counted = ref["counted"].copy()
    counted[1, 3] = counted[3, 1] = False
    mean, _, _ = distmat.group_maps(ref["mean"], ref["std"], counted, [7, 7, 9, 9])
    assert mean[0, 1] == pytest.approx(3.0)
    for r in (ref, gen, half):
        r["counted"] = counted
    st = distmat.compare_from_moments(half, half, ref, gen, [0.5])
    assert st["n_pairs"] == 5 and st["ens_drms"] == pytest.approx(np.sqrt(1.0 / 5)) and (1, 3) not in [(w["i"], w["j"]) for w in st["worst_mean"]]
    with pytest.raises(ValueError, match="groups"):
        distmat.compare_from_moments(half, half, ref, gen, [0.5], groups=[0, 1])


def test_maps_from_the_restatements_integers():
    """``first_mean`` / ``maps_of`` on the restatement's tables give the restatement's own maps."""
    xyz = R.cloud(9, 6, np.random.default_rng(2))
    xyz[4, 2, 1] = np.nan
    sel = np.arange(6)
    want_mean, want_std, want_dr, ctr = R.mean_std(xyz, sel)
    counted = ~np.eye(6, dtype=bool)
    first = {**R.moments(xyz, sel), "center": None, "counted": counted}
    assert np.array_equal(np.where(counted, distmat.first_mean(first), 0.0).astype(F), ctr)
    got = distmat.maps_of({**R.moments(xyz, sel, ctr), "center": ctr, "counted": counted})
    assert np.array_equal(got["mean"], want_mean) and np.array_equal(got["std"], want_std)
    assert np.array_equal(got["drmsd"], want_dr, equal_nan=True) and np.isnan(got["drmsd"][4]) and np.isfinite(np.delete(got["drmsd"], 4)).all()


def test_summary_of_keys():
    ref = _maps([1, 2, 3, 4, 5, 6], [.1, .2, .3, .4, .5, .6], drmsd=[0.1, 0.3], bad=[False, False])
    st = distmat.compare_from_moments(ref, ref, ref, ref, [0.1, 0.2], groups=[0, 0, 1, 2])
    short = distmat.summary_of(st)
    assert set(short) == {"n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "n_atoms", "n_pairs", "ens_drms", "fluct_drms", "std_corr", "floor",
                          "worst_mean", "worst_std", "drmsd", "groups"}
    assert len(short["worst_mean"]) == 1 and "hist_ref" not in short["drmsd"] and short["groups"]["n_groups"] == 3


# ----------------------------------------------------------------------------- refusals without a device
def test_every_value_error_comes_before_a_device_is_touched():
    n = 6
    xyz = np.zeros((3, n, 3), F)
    lim = distmat.limits()
    assert lim == {"structures": 2 ** 20, "atoms": 8192, "total": 2 ** 22}

    def refused(match, sel=np.arange(n), **kw):
        with pytest.raises(ValueError, match=match):
            distmat.moments(xyz, sel, device="cpu", **kw)
    refused("a distance needs two", sel=[3])
    refused("twice", sel=[0, 1, 1])
    refused("names atom", sel=[0, n])
    refused("empty", sel=[])
    refused("chunk", chunk=0)
    refused("chunk", chunk=lim["structures"] + 1)
    refused("symmetric", mask=np.triu(np.ones((n, n), bool), 1))
    refused("bool array", mask=np.zeros((n, n - 1), bool))
    refused("center must be a float array", center=np.zeros((n, n), int))
    refused(r"\[0, 1024\]", center=np.full((n, n), 1025.0))
    refused(r"\[0, 1024\]", center=np.full((n, n), np.nan))
    refused(r"\[0, 1024\]", center=-np.ones((n, n)))
    refused("symmetric", center=np.triu(np.ones((n, n)), 1))
    big = lim["atoms"] + 1
    with pytest.raises(ValueError, match="the kernel holds"):
        distmat.moments(np.zeros((1, big, 3), F), np.arange(big), device="cpu")
    # an accumulated total over 2^22 good structures: only n_good of the record says so
    counted = ~np.eye(n, dtype=bool)
    rec = {"n_good": lim["total"] - 2, "sel": np.arange(n, dtype=np.int32), "counted": counted, "center": None}
    refused("fixed-point budget", into=rec)
    refused("another selection", into={**rec, "n_good": 0, "sel": np.arange(n, dtype=np.int32)[::-1]})
    refused("another selection", into={**rec, "n_good": 0, "center": np.zeros((n, n), F)})
    with pytest.raises(ValueError, match="at least two reference frames"):
        distmat.compare(xyz, xyz[:1], np.arange(n), device="cpu")
    with pytest.raises(ValueError, match="atoms"):
        distmat.compare(xyz[:, :4], xyz, np.arange(4), device="cpu")


def _files(tmp_path, n=8, frames=4, **extra):
    rng = np.random.default_rng(0)
    z = np.array([6, 1, 7, 6, 8, 1, 6, 6])[:n]
    np.savez(tmp_path / "ref.npz", xyz=R.cloud(frames, n, rng), z=z, **extra)
    np.savez(tmp_path / "gen.npz", xyz=R.cloud(3, n, rng))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}", n


def test_the_parser_and_read_inputs(tmp_path):
    base, n = _files(tmp_path, bonds=np.stack([np.arange(7), np.arange(1, 8)], 1), mapping=np.arange(8) // 3)
    args = distmat.parser().parse_args(base.split())
    assert (args.dm_atoms, args.dm_exclude, args.dm_groups, args.maps, args.out, args.device) == ("heavy", 0, "none", None, "distmat_stats.json", "cuda")
    inp = distmat.read_inputs(args)
    assert inp["sel"].tolist() == [0, 2, 3, 4, 6, 7] and inp["mask"] is None and inp["groups"] is None
    assert inp["ref_xyz"].shape == (4, n, 3) and inp["gen_xyz"].shape == (3, n, 3)
    inp = distmat.read_inputs(distmat.parser().parse_args((base + " -dm_atoms all -dm_exclude 2 -dm_groups bead").split()))
    i = np.arange(n)
    assert np.array_equal(inp["mask"], np.abs(i[:, None] - i[None, :]) <= 2) and inp["groups"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2]
    with pytest.raises(SystemExit):
        distmat.parser().parse_args((base + " -dm_groups atom").split())


def test_the_command_line_refuses_before_any_launch(tmp_path):
    base, n = _files(tmp_path)                                       # z alone: no bonds, no mapping

    def refused(extra, match, line=None):
        with pytest.raises(SystemExit, match=match):
            distmat.read_inputs(distmat.parser().parse_args(((line or base) + " " + extra).split()))
    distmat.read_inputs(distmat.parser().parse_args(base.split()))   # -dm_exclude 0 needs no bonds
    refused("-dm_exclude 2", "missing z / bonds")
    refused("-dm_groups residue", "missing z / bonds")
    refused("-dm_groups bead", "missing z / mapping")
    refused("-dm_exclude -1", "-dm_exclude")
    np.savez(tmp_path / "nokeys.npz", xyz=np.zeros((4, n, 3), F))
    refused("", "missing z", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'nokeys.npz'}")
    refused(f"-top {tmp_path / 'nokeys.npz'}", r"missing \['z'\]")
    np.savez(tmp_path / "one.npz", xyz=np.zeros((1, n, 3), F), z=np.full(n, 6))
    refused("", "at least two reference frames", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'one.npz'}")
    np.savez(tmp_path / "h.npz", xyz=np.zeros((4, n, 3), F), z=np.array([6] + [1] * (n - 1)))
    refused("", "a distance needs two", line=f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'h.npz'}")
    np.savez(tmp_path / "chain.npz", z=np.full(n, 6), bonds=np.stack([np.arange(n - 1), np.arange(1, n)], 1))
    refused(f"-top {tmp_path / 'chain.npz'} -dm_exclude {n}", "leaves no pair")
    refused(f"-top {tmp_path / 'chain.npz'} -dm_groups residue", "peptide")
    refused("", "no such file", line=f"-gen {tmp_path / 'absent.npz'} -ref {tmp_path / 'ref.npz'}")


# ----------------------------------------------------------------------------- the library
def test_the_library_declares_binds_and_exports_the_distance_moments_kernel():
    assert NAMES <= set(_lib.header_symbols()) and NAMES <= set(_lib.PROTOTYPES)
    assert build.SOURCE_FLAGS["dist_moments.hip"] == ["-ffp-contract=off"]
    lib = _lib.load()
    assert (lib.cgv_dist_moments_row_tile(), lib.cgv_dist_moments_col_tile(), lib.cgv_dist_moments_chunk()) == (64, 64, 8)
    assert lib.cgv_dist_moments_workspace_bytes(10, 5) == 800 and lib.cgv_dist_moments_workspace_bytes(1, 8193) == 0
    assert lib.cgv_dist_moments_workspace_bytes(2 ** 20 + 1, 2) == 0


def test_the_c_entry_refuses_with_its_reason():
    lib = _lib.load()

    def call(S, n, m):
        rc = lib.cgv_dist_moments(None, None, None, None, S, n, m, None, None, None, None, None, 0, None)
        return rc, lib.cgv_last_error_string().decode()
    for (S, n, m), why in (((1, 4, 1), "2 <= m"), ((1, 4, 5), "2 <= m"), ((1, 9000, 8193), "max_atoms"), ((2 ** 20 + 1, 4, 4), "max_structures"),
                           ((-1, 4, 4), "bad size"), ((1, 4, 4), "null pointer")):
        rc, msg = call(S, n, m)
        assert rc != 0 and why in msg and "cgv_dist_moments" in msg, (S, n, m, msg)
    assert call(0, 4, 4)[0] == 0                                     # no structures: nothing to do
