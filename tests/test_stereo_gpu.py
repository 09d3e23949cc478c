"""Stereochemistry on the device: K31 (csrc/stereo.hip) against the numpy restatement.  Both sides round every operation
identically: every comparison of ``neg``, ``flat``, ``cis``, ``pierced``, ``counts`` and ``bad`` here is integer EQUALITY."""
import functools
import json

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import _lib, distmat, stereo
import stereo_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
MIRROR = np.array([1, 1, -1], F)


@functools.lru_cache(maxsize=None)
def _tiles():
    lib = _lib.load()
    return int(lib.cgv_stereo_item_tile()), int(lib.cgv_stereo_row_tile()), int(lib.cgv_stereo_col_tile()), int(lib.cgv_stereo_chunk())


def _case(S, n, C, Q, R_, B, seed=0, first=0, box=4.0):
    """Random clouds of ``n`` atoms in a small box (so that bonds do cross rings) and random tables over the atoms
    ``first .. n - 1``, with a random ``want``."""
    rng = np.random.default_rng(100003 * seed + 1009 * S + 101 * n + 31 * C + 17 * Q + 7 * R_ + B)
    xyz = R.cloud(S, n, rng, box=box)
    tab = R.random_tables(rng, n - first, C, Q, R_, B)
    for k in ("centres", "torsions", "bonds"):
        tab[k] = tab[k] + first
    tab["rings"] = np.where(tab["rings"] >= 0, tab["rings"] + first, -1).astype(np.int32)
    tab["n_atoms"] = n
    want = {"want_sign": rng.choice([-1, 1], size=C), "want_cis": rng.integers(0, 2, size=Q)}
    return xyz, tab, want


def _same(got, want, what=""):
    for k in ("neg", "flat", "cis", "pierced", "counts", "bad"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert got["n_good"] == want["n_good"], what


def _check(xyz, tab, want=None, what="", **kw):
    w = want or {}
    ref = R.counts(xyz, tab, w.get("want_sign"), w.get("want_cis"))
    got = stereo.counts(xyz, tab, want, device=DEV, **kw)
    _same(got, ref, what)
    return got, ref


# ----------------------------------------------------------------------------- tiles, chunks, slices
def test_the_tiles_are_what_the_sizes_below_stand_on():
    assert _tiles() == (256, 16, 64, 8)


@pytest.mark.parametrize("S", [1, 7, 8, 9, 63, 64, 65, 130])
def test_the_structures_end_at_every_chunk_and_slice_edge(S):
    ch = _tiles()[3]
    assert {ch - 1, ch, ch + 1} <= {1, 7, 8, 9, 63, 64, 65, 130}
    xyz, tab, want = _case(S, 23, 5, 5, 6, 9, first=2)               # a selection that is not the whole structure
    assert 0 not in R.named_atoms(tab) and 1 not in R.named_atoms(tab)
    got, _ = _check(xyz, tab, want, what=f"S = {S}")
    if S >= 63:
        assert got["pierced"].any() and got["neg"].any() and got["cis"].any() and got["counts"].any(0).all()


@pytest.mark.parametrize("N", [0, 1, 31, 32, 33, 63, 64, 65, 257])
def test_centres_torsions_and_bonds_end_at_every_word_and_tile_edge(N):
    assert _tiles()[0] + 1 == 257 and _tiles()[2] + 1 == 65
    xyz, tab, want = _case(3, 40, N, N, 3, N)
    got, _ = _check(xyz, tab, want, what=f"C = Q = B = {N}")
    if N >= 31:
        assert got["pierced"].any() and got["neg"].any() and got["cis"].any()
    xyz, tab, want = _case(3, 40, N, 7, 0, 0, seed=1)                # each of the three alone at this size
    _check(xyz, tab, want, what=f"C = {N} alone")
    xyz, tab, want = _case(3, 40, 0, N, 2, 5, seed=2)
    _check(xyz, tab, want, what=f"Q = {N} alone")


@pytest.mark.parametrize("n_rings", [0, 1, 15, 16, 17])
def test_the_rings_end_at_the_row_tile_with_every_ring_size_in_one_table(n_rings):
    assert _tiles()[1] == 16
    xyz, tab, want = _case(10, 30, 4, 4, n_rings, 33)
    if n_rings >= 15:
        assert sorted(set(stereo.ring_sizes(tab["rings"]).tolist())) == [3, 4, 5, 6, 7, 8]
    got, _ = _check(xyz, tab, want, what=f"R = {n_rings}")
    assert got["pierced"].shape == (n_rings, 33) and (n_rings == 0 or got["pierced"].any())


def test_a_tested_mask_with_cleared_bits_at_the_word_edges_and_empty_rows():
    xyz, tab, want = _case(12, 30, 0, 0, 4, 70)
    tested = np.ones((4, 70), bool)
    tested[0, [0, 31, 32, 63, 64, 69]] = False
    tested[1] = False                                                # a ring that is looked at by nothing
    tested[2, :64] = False                                           # only the second tile's bonds
    tested[3, 32:] = False                                           # only the first word's
    tab["tested"] = tested
    got, _ = _check(xyz, tab, what="cleared bits")
    assert not got["pierced"][~tested].any() and all(got["pierced"][r][tested[r]].any() for r in (0, 2, 3))
    tab["tested"] = np.ones((4, 70), bool)
    full, _ = _check(xyz, tab, what="all tested")
    assert np.array_equal(np.where(tested, full["pierced"], 0), got["pierced"]) and full["pierced"][~tested].any()


def test_all_four_tables_empty_only_bad_is_computed():
    xyz, tab, _ = _case(5, 6, 0, 0, 0, 0)
    xyz[2, 1, 1] = np.nan                                            # no atom is named: nothing is looked at
    got, _ = _check(xyz, tab, what="nothing")
    assert not got["bad"].any() and got["counts"].shape == (5, 3) and not got["counts"].any()


# ----------------------------------------------------------------------------- bad structures
def test_bad_structures_first_middle_and_last_change_nothing_but_bad():
    ch = _tiles()[3]
    S = 2 * ch + 3
    xyz, tab, want = _case(S, 26, 9, 9, 5, 20, first=1)
    named = R.named_atoms(tab)
    marked = {0: np.nan, ch - 1: np.inf, ch: -np.inf, S - 1: np.nan}
    for k, (s, v) in enumerate(marked.items()):
        xyz[s, named[(5 * k) % len(named)], k % 3] = v
    bad = sorted(marked)
    good = [s for s in range(S) if s not in bad]
    xyz[good[0], 0, 0], xyz[good[-1], 0, 2] = np.nan, np.inf         # atom 0 is named by nothing: not looked at
    got, _ = _check(xyz, tab, want, what="bad structures")
    assert np.flatnonzero(got["bad"]).tolist() == bad and got["n_good"] == S - len(bad) and not got["counts"][bad].any()
    clean = R.counts(xyz[good], tab, want["want_sign"], want["want_cis"])
    assert all(np.array_equal(got[k], clean[k]) for k in ("neg", "flat", "cis", "pierced")) and np.array_equal(got["counts"][good], clean["counts"])
    for s in bad:                                                    # alone: a launch of one bad structure counts nothing
        one, _ = _check(xyz[s:s + 1], tab, want, what=f"structure {s} alone")
        assert one["bad"].tolist() == [True] and not one["neg"].any() and not one["cis"].any() and not one["pierced"].any()


# ----------------------------------------------------------------------------- launches, want
def test_any_cut_into_launches_or_calls_and_a_second_run_give_identical_bits():
    S = 37
    xyz, tab, want = _case(S, 30, 20, 20, 17, 66)
    xyz[0, 5, 1], xyz[20, 7, 0] = np.nan, np.inf
    first, _ = _check(xyz, tab, want, what="one launch", chunk=S)
    runs = {"again": stereo.counts(xyz, tab, want, chunk=S, device=DEV)}
    for per_launch in (1, 7):
        runs[f"{per_launch} per launch"] = stereo.counts(xyz, tab, want, chunk=per_launch, device=DEV)
    part = stereo.counts(xyz[:1], tab, want, device=DEV)             # 1 + (S - 1): the first is bad
    assert part["n_good"] == 0 and not part["pierced"].any()
    runs["1 + (S - 1)"] = stereo.counts(xyz[1:], tab, want, into=part, device=DEV)
    part = stereo.counts(xyz[:5], tab, want, device=DEV)
    part = stereo.counts(xyz[5:22], tab, want, into=part, chunk=4, device=DEV)
    runs["5 + 17 + 15"] = stereo.counts(torch.from_numpy(xyz[22:]).to(DEV), tab, want, into=part)
    for name, run in runs.items():
        _same(run, first, name)
    with pytest.raises(ValueError, match="other tables"):
        stereo.counts(xyz[:2], tab, {"want_sign": want["want_sign"]}, into=part, device=DEV)


def test_a_want_that_is_null_leaves_its_counter_at_zero():
    xyz, tab, want = _case(9, 30, 33, 33, 3, 10)
    both, _ = _check(xyz, tab, want, what="both")
    assert both["counts"][:, 0].any() and both["counts"][:, 1].any()
    none, _ = _check(xyz, tab, None, what="neither")
    assert not none["counts"][:, :2].any() and np.array_equal(none["counts"][:, 2], both["counts"][:, 2])
    sign, _ = _check(xyz, tab, {"want_sign": want["want_sign"]}, what="want_sign alone")
    assert np.array_equal(sign["counts"][:, 0], both["counts"][:, 0]) and not sign["counts"][:, 1].any()
    cis, _ = _check(xyz, tab, {"want_cis": want["want_cis"], "want_sign": None}, what="want_cis alone")
    assert np.array_equal(cis["counts"][:, 1], both["counts"][:, 1]) and not cis["counts"][:, 0].any()
    assert all(np.array_equal(none[k], both[k]) for k in ("neg", "flat", "cis", "pierced"))


def test_a_flat_centre_is_counted_flat_and_wrong_for_either_want():
    x = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1]]], F)
    tab = {"centres": np.array([[0, 1, 2, 3], [0, 1, 2, 4], [0, 2, 1, 4]], np.int32), "torsions": np.zeros((0, 4), np.int32),
           "rings": np.zeros((0, 8), np.int32), "bonds": np.zeros((0, 2), np.int32), "tested": np.zeros((0, 0), bool)}
    for ws in ([1, 1, 1], [-1, -1, -1]):
        got, _ = _check(x, tab, {"want_sign": ws}, what=f"want {ws}")
        assert got["flat"].tolist() == [1, 0, 0] and got["neg"].tolist() == [0, 0, 1] and got["counts"][0, 0] == 2


# ----------------------------------------------------------------------------- limits
def test_one_past_each_limit_is_refused_without_a_launch():
    lim, lib = stereo.limits(), _lib.load()
    xyz, tab, _ = _case(2, 12, 2, 2, 1, 3)
    for key, width in (("centres", 4), ("torsions", 4), ("bonds", 2)):
        big = {**tab, key: np.zeros((lim[key] + 1, width), np.int32) + np.arange(width, dtype=np.int32)}
        if key == "bonds":
            big["tested"] = np.ones((1, lim[key] + 1), bool)
        with pytest.raises(ValueError, match="the kernel holds"):
            stereo.counts(xyz, big, device=DEV)
    many = np.full((lim["rings"] + 1, 8), -1, np.int32)
    many[:, :3] = [0, 1, 2]
    with pytest.raises(ValueError, match="the kernel holds"):
        stereo.counts(xyz, {**tab, "rings": many, "tested": np.ones((lim["rings"] + 1, 3), bool)}, device=DEV)
    wide = lim["atoms"] + 1
    chain = np.stack([np.arange(wide - 1), np.arange(1, wide)], 1).astype(np.int32)
    with pytest.raises(ValueError, match="the kernel holds"):
        stereo.counts(np.zeros((1, wide, 3), F), {**tab, "bonds": chain, "tested": np.ones((1, wide - 1), bool)}, device=DEV)
    with pytest.raises(ValueError, match="chunk"):
        stereo.counts(xyz, tab, chunk=lim["structures"] + 1, device=DEV)
    # the raw entry point, on valid pointers: refused by its sizes before anything is read or written
    dev = torch.device(DEV)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    d_xyz, d_sel, quad, ring, pair, mask = torch.zeros(2, 12, 3, device=dev), torch.arange(12, dtype=torch.int32, device=dev), i32(2, 4), i32(1, 8), i32(3, 2), i32(1, 1)
    ring[0, :3] = torch.tensor([0, 1, 2], dtype=torch.int32)
    ring[0, 3:] = -1
    outs = [torch.full(s, -7, dtype=t, device=dev) for s, t in (((2,), torch.int64), ((2,), torch.int64), ((2,), torch.int64), ((1, 3), torch.int32),
                                                                 ((2, 3), torch.int32), ((2,), torch.int32))]
    ws = torch.zeros(1024, device=dev)

    def call(S=2, n=12, P=12, C=2, Q=2, R_=1, B=3):
        rc = lib.cgv_stereo_counts(_lib.ptr(d_xyz), _lib.ptr(d_sel), _lib.ptr(quad), _lib.ptr(quad), _lib.ptr(ring), _lib.ptr(pair), _lib.ptr(mask),
                                   None, None, S, n, P, C, Q, R_, B, *[_lib.ptr(t) for t in outs], _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(S=lim["structures"] + 1), dict(P=13), dict(n=lim["atoms"] + 1, P=lim["atoms"] + 1), dict(C=lim["centres"] + 1),
               dict(Q=lim["torsions"] + 1), dict(R_=lim["rings"] + 1), dict(B=lim["bonds"] + 1), dict(P=0), dict(C=-1)):
        assert call(**kw) != 0, kw
        assert all(bool((t == -7).all()) for t in outs), kw
    small = torch.zeros(4, device=dev)
    rc = lib.cgv_stereo_counts(_lib.ptr(d_xyz), _lib.ptr(d_sel), _lib.ptr(quad), _lib.ptr(quad), _lib.ptr(ring), _lib.ptr(pair), _lib.ptr(mask), None, None,
                               2, 12, 12, 2, 2, 1, 3, *[_lib.ptr(t) for t in outs], _lib.ptr(small), 16, _lib.stream_ptr())
    assert rc != 0 and "workspace" in lib.cgv_last_error_string().decode() and all(bool((t == -7).all()) for t in outs)
    for t in outs[:4]:
        t.zero_()
    assert call() == 0                                               # and the same buffers take a valid call: twelve atoms at one point
    assert outs[1].tolist() == [2, 2] and not outs[0].any() and not outs[2].any() and not outs[3].any()
    assert not outs[4].any() and outs[5].tolist() == [0, 0]


# ----------------------------------------------------------------------------- the hand-built cases through the device
def test_a_mirror_image_flips_every_centre_and_keeps_every_distance():
    xyz, tab, _ = _case(33, 30, 40, 40, 12, 50, box=5.0)
    a, _ = _check(xyz, tab, what="as it is")
    want = {"want_sign": np.where(2 * a["neg"] > a["n_good"], -1, 1), "want_cis": (2 * a["cis"] > a["n_good"]).astype(int)}
    own, _ = _check(xyz, tab, want, what="against its own majority")
    image, _ = _check(xyz * MIRROR, tab, want, what="mirrored")
    assert not a["flat"].any() and np.array_equal(image["neg"], 33 - a["neg"])
    assert np.array_equal(image["cis"], a["cis"]) and np.array_equal(image["pierced"], a["pierced"]) and a["pierced"].any()
    assert np.array_equal(image["counts"][:, 1:], own["counts"][:, 1:]) and np.array_equal(image["counts"][:, 0], 40 - own["counts"][:, 0])
    # the point of the module: to every distance the mirror image of a structure IS the structure, and here all of its centres are wrong
    sel = np.arange(30)
    one = xyz[:1]
    target = distmat.mean_std(one, sel, device=DEV)["mean"].astype(F)
    assert distmat.drmsd(one * MIRROR, sel, target, device=DEV).tolist() == distmat.drmsd(one, sel, target, device=DEV).tolist()
    hand = {"want_sign": np.where(R.counts(one, tab)["neg"] > 0, -1, 1)}
    assert stereo.counts(one, tab, hand, device=DEV)["counts"][:, 0].tolist() == [0]
    assert stereo.counts(one * MIRROR, tab, hand, device=DEV)["counts"][:, 0].tolist() == [40]


def test_the_hexagon_and_rings_of_every_size_through_the_device():
    tab, xyz = R.one_ring(6, [seg for seg, _ in R.HEXAGON_CASES])
    got, _ = _check(xyz, tab, what="hexagon")
    assert got["pierced"][0].tolist() == [int(hit) for _, hit in R.HEXAGON_CASES]
    for k in range(3, 9):
        tab, xyz = R.one_ring(k, [((0.1, 0.05, -1), (0.1, 0.05, 1)), ((0.3, 0, -1), (0.3, 0, 1)), ((2, 2, -1), (2, 2, 1))])
        got, _ = _check(np.concatenate([xyz, xyz * MIRROR]), tab, what=f"{k}-gon")
        assert got["pierced"][0].tolist() == [2, 2, 0] and got["counts"][:, 2].tolist() == [2, 2]


# ----------------------------------------------------------------------------- end to end
def _phe_sets():
    rng = np.random.default_rng(12)
    ref, gen = R.phe_frames(40, rng), R.phe_frames(24, rng)
    edits = {3: (R.invert_ca,), 7: (R.flip_omega,), 11: (R.thread_ring,), 20: (R.invert_ca, R.flip_omega, R.thread_ring)}
    for s, fs in edits.items():
        for f in fs:
            gen[s] = f(gen[s])
    return ref, gen


def test_compare_names_exactly_the_samples_that_were_edited():
    ref, gen = _phe_sets()
    flags = {}
    st = stereo.compare(gen, ref, R.PHE_Z, R.PHE_BONDS, groups="bead", mapping=np.arange(34) // 6, device=DEV, flags=flags)
    assert tuple(st) == stereo.STEREO_STATS_KEYS and json.loads(json.dumps(st)) == st
    want = np.zeros((24, 3), np.int32)
    want[3, 0] = want[7, 1] = want[11, 2] = 1
    want[20] = 1
    assert np.array_equal(flags["counts"], want) and not flags["bad"].any()
    assert (st["n_ref"], st["n_gen"], st["n_centres"], st["n_torsions"], st["n_rings"], st["n_bonds"], st["n_tested"]) == (40, 24, 1, 2, 1, 33, 21)
    assert st["valid"]["ref"] == {"centres": 1.0, "torsions": 1.0, "rings": 1.0, "all": 1.0}
    assert st["valid"]["gen"] == {"centres": 22 / 24, "torsions": 22 / 24, "rings": 22 / 24, "all": 20 / 24}
    assert st["inversion_rate"] == {"gen": [2 / 24], "ref": [0.0]} and st["worst_centres"][0]["atom"] == R.PHE["CA"]
    assert st["worst_torsions"][0]["atoms"] == list(R.PHE["omega"][1]) and st["worst_torsions"][0]["gen"] == 2 / 24 and st["worst_torsions"][1]["gen"] == 0.0
    assert st["worst_pairs"][0]["bond_atoms"] == list(R.PHE["cl"]) and st["worst_pairs"][0]["ring_atoms"] == R.PHE["ring"] and st["worst_pairs"][1]["gen"] == 0.0
    assert st["errors"]["hist_gen"]["counts"] == [20, 3, 0, 1] and st["errors"]["jsd"] > 0 and st["errors"]["floor"] == 0.0
    assert st["groups"]["n_groups"] == 6 and st["groups"]["worst"][0]["gen"] > 0
    heavy = stereo.compare(gen, ref, R.PHE_Z, R.PHE_BONDS, atoms="heavy", device=DEV)      # the two planar carbonyl carbons are dropped
    assert heavy["n_centres"] == 1 and heavy["worst_centres"][0]["atom"] == R.PHE["CA"] and heavy["n_bonds"] == 17
    assert heavy["valid"]["gen"]["torsions"] == 22 / 24 and heavy["valid"]["gen"]["rings"] == 22 / 24
    assert heavy["valid"]["gen"]["centres"] == 1.0                   # the edit moved a hydrogen: a heavy-atom topology cannot see it


def test_the_command_line_writes_its_statistics_and_flags(tmp_path, capsys):
    ref, gen = _phe_sets()
    np.savez(tmp_path / "ref.npz", xyz=ref, z=R.PHE_Z, bonds=R.PHE_BONDS)
    np.savez(tmp_path / "gen.npz", xyz=gen.reshape(12, 2, 34, 3))
    out, flags = tmp_path / "stereo_stats.json", tmp_path / "flags.npz"
    capsys.readouterr()
    st = stereo.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -flags {flags} -out {out} -device {DEV}".split())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["stereo_stats"] == json.loads(json.dumps(stereo.summary_of(st))) and line["out"] == str(out)
    with open(out) as f:
        stored = json.load(f)
    assert tuple(stored) == stereo.STEREO_STATS_KEYS and stored["valid"]["gen"]["all"] == 20 / 24 and stored["params"]["atoms"] == "all"
    with np.load(flags) as f:
        assert sorted(f.files) == ["bad", "counts"] and f["counts"].shape == (24, 3) and np.flatnonzero(f["counts"].sum(1)).tolist() == [3, 7, 11, 20]
        assert not f["bad"].any()
