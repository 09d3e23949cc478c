"""Distance-matrix moments on the device: K30 (csrc/dist_moments.hip) against the numpy restatement.  Both sides round every
operation identically: every comparison of ``sum_e``, ``sum_e2``, ``dev2`` and ``bad`` here is integer EQUALITY."""
import functools
import json

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import _lib, distmat
import density_restatement as DR
import distmat_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


@functools.lru_cache(maxsize=None)
def _tiles():
    lib = _lib.load()
    return int(lib.cgv_dist_moments_row_tile()), int(lib.cgv_dist_moments_col_tile()), int(lib.cgv_dist_moments_chunk())


@functools.lru_cache(maxsize=None)
def _cloud(S, m, seed=0):
    """``S`` random clouds of ``m`` atoms in a 30 A box, read-only."""
    xyz = R.cloud(S, m, np.random.default_rng(1000 * m + S + seed))
    xyz.setflags(write=False)
    return xyz


def _center_of(xyz, sel):
    """A nonzero centre table: the fp32 distances of the FIRST structure, so every pair of it sits exactly on its centre."""
    d, _, _ = R.terms(np.asarray(xyz)[0, sel], F(0))
    return d


def _same(got, want, what=""):
    for k in ("sum_e", "sum_e2", "dev2", "bad"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert got["n_good"] == want["n_good"] and got["n_pairs"] == want["n_pairs"], what
    assert np.array_equal(got["sum_e"], got["sum_e"].T) and np.array_equal(got["sum_e2"], got["sum_e2"].T), what


def _check(xyz, sel, center=None, mask=None, what="", **kw):
    want = R.moments(xyz, sel, center, mask)
    got = distmat.moments(xyz, sel, center=center, mask=mask, device=DEV, **kw)
    _same(got, want, what)
    return got, want


# ----------------------------------------------------------------------------- tiles, chunks, slices
def test_the_tiles_are_what_the_sizes_below_stand_on():
    assert _tiles() == (64, 64, 8)


@pytest.mark.parametrize("m", [2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193])
def test_the_selection_ends_at_every_word_and_tile_edge(m):
    xyz, sel = _cloud(3, m), np.arange(m)
    got, _ = _check(xyz, sel, what=f"m = {m}, no centre")
    assert (got["sum_e"][~np.eye(m, dtype=bool)] > 0).all() and (got["dev2"] > 0).all()
    ctr = _center_of(xyz, sel)
    got, _ = _check(xyz, sel, center=ctr, what=f"m = {m}, centre")
    assert got["dev2"][0] == 0 and (got["dev2"][1:] > 0).all()       # the first structure IS the centre: e = 0 at every pair


@pytest.mark.parametrize("S", [1, 7, 8, 9, 63, 64, 65, 130])
def test_the_structures_end_at_every_chunk_and_slice_edge(S):
    xyz, sel = _cloud(S, 23), np.arange(1, 21)                       # a selection that is not the whole structure
    _check(xyz, sel, what=f"S = {S}")
    _check(xyz, sel, center=_center_of(xyz, sel), what=f"S = {S}, centre")


# ----------------------------------------------------------------------------- mask
def test_masks_at_the_word_edges_an_empty_tile_and_a_single_pair():
    m = 130
    xyz, sel = _cloud(5, m), np.arange(m)
    ctr = _center_of(xyz, sel)
    edges = np.zeros((m, m), bool)
    for i, j in ((0, 15), (0, 16), (0, 31), (0, 32), (1, 63), (1, 64), (2, 129), (30, 31), (31, 32), (47, 48), (63, 64), (127, 128), (128, 129)):
        edges[i, j] = edges[j, i] = True
    got, want = _check(xyz, sel, mask=edges, what="word edges")
    assert want["n_pairs"] == m * (m - 1) // 2 - 13 and not got["sum_e"][edges].any() and not got["sum_e2"][edges].any()
    tile = np.zeros((m, m), bool)                                    # rows 0..63 against columns 64..127: one whole tile
    tile[:64, 64:128] = tile[64:128, :64] = True
    got, _ = _check(xyz, sel, center=ctr, mask=tile, what="an empty tile")
    assert not got["sum_e2"][tile].any() and got["sum_e2"][:64, 128:].all()
    for i, j in ((5, 100), (0, 1), (128, 129)):
        one = np.ones((m, m), bool)
        one[i, j] = one[j, i] = False
        got, want = _check(xyz, sel, mask=one, what=f"only the pair {i}, {j}")
        assert want["n_pairs"] == 1 and np.count_nonzero(got["sum_e"]) == 2 and got["sum_e"][i, j] > 0
    none = np.ones((m, m), bool)
    got, _ = _check(xyz, sel, mask=none, what="no pair at all")
    assert not got["sum_e"].any() and not got["dev2"].any() and got["n_good"] == 5


# ----------------------------------------------------------------------------- bad structures, special distances
def test_bad_structures_first_last_and_alone_change_nothing_but_bad():
    rt, ct, ch = _tiles()
    S, n = 2 * ch + 3, 26
    xyz = _cloud(S, n).copy()
    sel = np.array([k for k in range(n) if k != 10])                 # atom 10 is outside the selection
    marked = {0: np.nan, ch - 1: np.inf, ch: -np.inf, S - 1: np.nan}
    for k, (s, v) in enumerate(marked.items()):
        xyz[s, sel[(5 * k) % len(sel)], k % 3] = v
    xyz[ch + 2, sel[3], 1] += 600.0                                  # finite, but more than 512 A from the centroid
    bad = sorted(list(marked) + [ch + 2])
    good = [s for s in range(S) if s not in bad]
    xyz[good[0], 10, 0], xyz[good[-1], 10, 2] = np.nan, 5000.0       # unselected: not looked at
    ctr = _center_of(xyz[good], sel)
    for c in (None, ctr):
        got, want = _check(xyz, sel, center=c, what="bad structures")
        assert np.flatnonzero(got["bad"]).tolist() == bad and got["n_good"] == S - len(bad) and not got["dev2"][bad].any()
        clean = R.moments(xyz[good], sel, c)
        assert np.array_equal(got["sum_e"], clean["sum_e"]) and np.array_equal(got["sum_e2"], clean["sum_e2"])
        assert np.array_equal(got["dev2"][good], clean["dev2"])
    for s in bad:                                                    # alone: a launch of one bad structure sums nothing
        got, _ = _check(xyz[s:s + 1], sel, center=ctr, what=f"structure {s} alone")
        assert got["bad"].tolist() == [True] and not got["sum_e"].any() and not got["sum_e2"].any() and got["dev2"].tolist() == [0]
    # 600 A out of a cloud of a few atoms is NOT bad: the centroid follows it (two atoms are bad only past 1024 A apart)
    far = np.zeros((3, 2, 3), F)
    far[0, 1, 0], far[1, 1, 0], far[2, 1, 0] = 600.0, 1023.0, 1025.0
    got, _ = _check(far, [0, 1], what="two atoms far apart")
    assert got["bad"].tolist() == [False, False, True] and got["sum_e"][0, 1] == (600 + 1023) * 2 ** 20


def test_a_pair_at_distance_zero_and_a_pair_exactly_at_its_centre():
    m = 70
    xyz = _cloud(4, m).copy()
    xyz[:, 69] = xyz[:, 3]                                           # atoms 3 and 69 coincide in every structure
    xyz[:, 40] = xyz[:, 8] + np.array([3, 4, 0], F)                  # nearly 5 A apart ...
    xyz[1, 8], xyz[1, 40] = (1, 2, 3), (4, 6, 3)                     # ... and exactly 5 A in structure 1
    sel = np.arange(m)
    got, _ = _check(xyz, sel, what="no centre")
    assert got["sum_e"][3, 69] == 0 and got["sum_e2"][69, 3] == 0
    ctr = _center_of(xyz, sel).copy()
    ctr[8, 40] = ctr[40, 8] = 5.0
    ctr[3, 69] = ctr[69, 3] = 1.5
    got, _ = _check(xyz, sel, center=ctr, what="centre")
    assert got["sum_e"][3, 69] == -4 * int(1.5 * 2 ** 20) and got["sum_e2"][3, 69] == 4 * int(2.25 * 2 ** 20)
    one = distmat.moments(xyz[1:2], [8, 40], center=np.array([[0, 5], [5, 0]], F), device=DEV)
    assert not one["sum_e"].any() and not one["sum_e2"].any() and one["dev2"].tolist() == [0] and one["n_good"] == 1


# ----------------------------------------------------------------------------- launches
def test_any_cut_into_launches_or_calls_and_a_second_run_give_identical_bits():
    rt, ct, ch = _tiles()
    S, m = 37, rt + 3
    xyz = _cloud(S, m).copy()
    xyz[0, 5, 1], xyz[20, 66, 0] = np.nan, np.inf
    sel = np.arange(m)
    ctr = _center_of(xyz[1:], sel)
    for c in (None, ctr):
        first, _ = _check(xyz, sel, center=c, what="one launch", chunk=S)
        runs = {"again": distmat.moments(xyz, sel, center=c, chunk=S, device=DEV)}
        for per_launch in (1, 7):
            runs[f"{per_launch} per launch"] = distmat.moments(xyz, sel, center=c, chunk=per_launch, device=DEV)
        part = distmat.moments(xyz[:1], sel, center=c, device=DEV)                         # 1 + (S - 1): the first is bad
        assert part["n_good"] == 0 and not part["sum_e"].any()
        runs["1 + (S - 1)"] = distmat.moments(xyz[1:], sel, center=c, into=part, device=DEV)
        part = distmat.moments(xyz[:5], sel, center=c, device=DEV)
        part = distmat.moments(xyz[5:22], sel, center=c, into=part, chunk=4, device=DEV)
        runs["5 + 17 + 15"] = distmat.moments(xyz[22:], sel, center=c, into=part, device=DEV)
        for name, run in runs.items():
            _same(run, first, name)


def test_the_selection_permuted_and_with_repeats():
    m = 40
    xyz = _cloud(6, m + 5)
    sel = np.random.default_rng(3).permutation(m + 5)[:m]
    got, _ = _check(xyz, sel, what="permuted")
    inorder, _ = _check(xyz, np.sort(sel), what="sorted")
    where = np.argsort(np.argsort(sel))                              # the place of sel[k] in the sorted selection
    assert np.array_equal(got["sum_e"], inorder["sum_e"][np.ix_(where, where)]) and np.array_equal(got["dev2"], inorder["dev2"])
    with pytest.raises(ValueError, match="twice"):
        distmat.moments(xyz, [0, 1, 2, 1], device=DEV)
    with pytest.raises(ValueError, match="names atom"):
        distmat.moments(xyz, [0, m + 5], device=DEV)


def test_one_atom_one_past_each_limit_and_a_full_table_are_refused_without_a_launch():
    lim, lib = distmat.limits(), _lib.load()
    n = 4
    xyz = np.zeros((2, n, 3), F)
    with pytest.raises(ValueError, match="a distance needs two"):
        distmat.moments(xyz, [2], device=DEV)
    with pytest.raises(ValueError, match="the kernel holds"):
        big = lim["atoms"] + 1
        distmat.moments(np.zeros((1, big, 3), F), np.arange(big), device=DEV)
    with pytest.raises(ValueError, match="chunk"):
        distmat.moments(xyz, np.arange(n), chunk=lim["structures"] + 1, device=DEV)
    ok = distmat.moments(xyz, np.arange(n), device=DEV)
    with pytest.raises(ValueError, match="fixed-point budget"):     # only n_good says that the tables are full
        distmat.moments(xyz, np.arange(n), into={**ok, "n_good": lim["total"] - 1}, device=DEV)
    assert distmat.moments(xyz, np.arange(n), into={**ok, "n_good": lim["total"] - 2}, device=DEV)["n_good"] == lim["total"]
    # the raw entry point, on valid pointers: refused by its sizes before anything is read or written
    dev = torch.device(DEV)
    d_xyz, d_sel = torch.zeros(2, n, 3, device=dev), torch.arange(n, dtype=torch.int32, device=dev)
    a1, a2 = (torch.full((n, n), -7, dtype=torch.int64, device=dev) for _ in range(2))
    dev2, bad = torch.full((2,), -7, dtype=torch.int64, device=dev), torch.full((2,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(1024, device=dev)

    def call(S=2, n_atoms=n, m=n):
        rc = lib.cgv_dist_moments(_lib.ptr(d_xyz), _lib.ptr(d_sel), None, None, S, n_atoms, m, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(dev2),
                                  _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(m=1), dict(m=0), dict(m=n + 1), dict(n_atoms=lim["atoms"] + 1, m=lim["atoms"] + 1), dict(S=lim["structures"] + 1)):
        assert call(**kw) != 0, kw
        assert all(bool((t == -7).all()) for t in (a1, a2, dev2, bad)), kw
    a1.zero_(), a2.zero_(), dev2.zero_()
    assert call() == 0                                               # and the same buffers take a valid call
    assert not a1.any() and not a2.any() and dev2.tolist() == [0, 0] and bad.tolist() == [0, 0]     # four atoms at one point


# ----------------------------------------------------------------------------- fp64
def test_mean_std_and_drmsd_against_the_fp64_form():
    S, m = 33, 70
    xyz, sel = _cloud(S, m + 2), np.arange(1, m + 1)
    d64, mean64, std64 = R.maps64(xyz, sel)
    d_max = d64.max()
    got = distmat.mean_std(xyz, sel, chunk=16, device=DEV)
    want_mean, want_std, want_dr, ctr = R.mean_std(xyz, sel)
    off = ~np.eye(m, dtype=bool)
    assert np.array_equal(got["center"], ctr) and np.array_equal(got["mean"][off], want_mean[off]) and np.array_equal(got["std"][off], want_std[off])
    assert np.array_equal(got["drmsd"], want_dr) and not np.diag(got["mean"]).any() and not np.diag(got["std"]).any()
    # the bounds of tests/test_distmat_cpu.py (distmat_restatement: mean_bound, std_bound, drmsd_bound), from u = 2^-24
    assert (np.abs(got["mean"] - mean64)[off] <= R.mean_bound(d_max)).all()
    assert (np.abs(got["std"] - std64)[off] <= R.std_bound(std64, d_max)[off]).all()
    iu = np.triu_indices(m, 1)
    target = mean64.astype(F)
    dr64 = np.sqrt(((d64 - target.astype(np.float64)[None]) ** 2)[:, iu[0], iu[1]].mean(1))
    dr = distmat.drmsd(xyz, sel, target, device=DEV)
    assert (np.abs(dr - dr64) <= R.drmsd_bound(dr64, d_max)).all() and (dr > 1.0).all()
    mirrored = xyz * np.array([1, 1, -1], F)                         # no superposition: a reflection changes no distance
    assert np.array_equal(distmat.drmsd(mirrored, sel, target, device=DEV), dr)
    # masked pairs are NaN in the maps and leave the distance RMSD
    mask = np.zeros((m, m), bool)
    mask[:40, :40] = True
    part = distmat.mean_std(xyz, sel, mask=mask, device=DEV)
    assert np.isnan(part["mean"][mask & off]).all() and np.array_equal(part["mean"][~mask], got["mean"][~mask])
    assert part["n_pairs"] == m * (m - 1) // 2 - 40 * 39 // 2


# ----------------------------------------------------------------------------- end to end
def _peptide_sets():
    """40 + 40 jittered frames of two conformers' worth of the four-residue peptide with one hydrogen: 22 atoms."""
    rng = np.random.default_rng(11)
    z, bonds = DR.peptide(4)
    n = z.shape[0]
    base = np.array([np.pi] + [-2.0, 2.3, np.pi] * 4)
    heavy = DR.peptide_structures(4, base[None] + rng.normal(0.0, 0.15, (80, 13)))
    h = heavy[:, n - 1] + np.array([0.6, 0.6, 0.6], F)
    xyz = np.concatenate([heavy, h[:, None]], axis=1).astype(F)
    return np.append(z, 1), np.concatenate([bonds, [[n - 1, n]]]), xyz


def test_the_command_line_on_a_peptide(tmp_path, capsys):
    z, bonds, xyz = _peptide_sets()
    n = z.shape[0]
    assert n == 22 and xyz.shape == (80, 22, 3)
    moved = 9
    shifted = xyz.copy()
    shifted[:, moved, 2] += 1.0
    np.savez(tmp_path / "ref.npz", xyz=xyz, z=z, bonds=bonds, mapping=np.arange(n) // 4)
    np.savez(tmp_path / "gen.npz", xyz=shifted.reshape(40, 2, n, 3))
    out, maps = tmp_path / "distmat_stats.json", tmp_path / "maps.npz"
    capsys.readouterr()
    same = distmat.main(f"-gen {tmp_path / 'ref.npz'} -ref {tmp_path / 'ref.npz'} -dm_atoms all -out {out} -device {DEV}".split())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["distmat_stats"] == json.loads(json.dumps(distmat.summary_of(same))) and line["out"] == str(out)
    with open(out) as f:
        stored = json.load(f)
    assert tuple(stored) == distmat.DISTMAT_STATS_KEYS == tuple(same)
    assert (stored["n_ref"], stored["n_gen"], stored["n_bad_ref"], stored["n_bad_gen"], stored["n_atoms"], stored["n_pairs"]) == (80, 80, 0, 0, 22, 231)
    assert stored["ens_drms"] == 0.0 and stored["fluct_drms"] == 0.0 and stored["std_corr"] == pytest.approx(1.0)
    assert stored["floor"]["ens_drms"] > 0 and stored["floor"]["fluct_drms"] > 0 and stored["drmsd"]["jsd"] == 0.0 and stored["drmsd"]["floor"] > 0
    stats = distmat.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -dm_atoms all -dm_exclude 1 -dm_groups residue "
                         f"-maps {maps} -out {out} -device {DEV}".split())
    assert stats["n_gen"] == 80 and stats["n_pairs"] == 231 - 21 and stats["ens_drms"] > stats["floor"]["ens_drms"] > 0
    assert len(stats["worst_mean"]) == 5 and all(moved in (w["a"], w["b"]) for w in stats["worst_mean"])
    assert stats["groups"]["n_groups"] == 4 and stats["groups"]["ens_drms"] > 0 and len(stats["groups"]["worst_mean"]) == 5
    assert stats["drmsd"]["mean_gen"] > stats["drmsd"]["mean_ref"] > 0
    with np.load(maps) as f:
        assert sorted(f.files) == ["mean_gen", "mean_ref", "sel", "std_gen", "std_ref"] and f["mean_ref"].shape == (22, 22)
        want_mean, want_std, _, _ = R.mean_std(xyz, np.arange(n), mask=distmat.excluded_pairs(bonds, n, np.arange(n), 1))
        counted = ~distmat.excluded_pairs(bonds, n, np.arange(n), 1)
        assert np.array_equal(f["mean_ref"][counted], want_mean[counted]) and np.array_equal(f["std_ref"][counted], want_std[counted])
        assert np.isnan(f["mean_ref"][0, 1]) and f["sel"].tolist() == list(range(n))
