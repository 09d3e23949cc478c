"""Pair-distance distributions on the device: K29 (csrc/pair_hist.hip) against the numpy restatement.  Both sides round every
operation identically: every comparison here is integer EQUALITY, on every entry of ``hist``, ``beyond`` and ``bad``."""
import functools
import json

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import _lib, pairdist
import density_restatement as DR
import pairdist_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


@functools.lru_cache(maxsize=None)
def _tiles():
    lib = _lib.load()
    return int(lib.cgv_pairdist_row_tile()), int(lib.cgv_pairdist_col_tile()), int(lib.cgv_pairdist_chunk())


def _runs(m, C, run=23, missing=None):
    """Classes in runs of ``run`` atoms (23 divides no tile: the runs straddle every tile edge), starting inside a run;
    ``missing``: a class that no atom has."""
    cls = ((np.arange(m) + 5) // run) % C
    if missing is not None:
        cls = np.where(cls == missing, (missing + 1) % C, cls)
    return cls


@functools.lru_cache(maxsize=None)
def _cloud(S, m, seed=0):
    """``S`` random-walk chains of ``m`` atoms (1.5 A steps), read-only."""
    xyz = R.chains(S, m, np.random.default_rng(1000 * m + S + seed))
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def _want(S, m, C, n_bins, r_max, depth=3, missing=None, seed=0):
    w = R.pair_hist(_cloud(S, m, seed), np.arange(m), _runs(m, C, missing=missing), C, R.band(m, depth), r_max, n_bins)
    for v in w.values():
        v.setflags(write=False)
    return w


def _same(got, want, what=""):
    for k in ("hist", "beyond", "bad"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert got["n_good"] == int((~want["bad"]).sum()), what
    # the conservation identity, on the device result
    assert np.array_equal(got["hist"].sum(1) + got["beyond"], got["n_good"] * want["n_pairs"]), what


def _check_cloud(S, m, C=2, n_bins=100, r_max=8.0, depth=3, missing=None, what="", **kw):
    want = _want(S, m, C, n_bins, r_max, depth, missing)
    got = pairdist.count_pairs(_cloud(S, m), np.arange(m), _runs(m, C, missing=missing), C, R.band(m, depth), r_max, n_bins,
                               device=DEV, **kw)
    _same(got, want, what)
    if m > 8:                                                       # a case with nothing in range, or nothing beyond, proves little
        assert want["hist"].sum() > 0 and want["beyond"].sum() > 0, what
    return got


# ----------------------------------------------------------------------------- tiles, chunks, slices
@pytest.mark.parametrize("which", range(8))
def test_the_selection_ends_at_every_tile_edge(which):
    rt, ct, ch = _tiles()
    sizes = [1, 2, rt - 1, rt, rt + 1, ct, ct + 1, rt + ct + 1]
    _check_cloud(3, sizes[which], what=f"m = {sizes[which]}")


@pytest.mark.parametrize("which", range(4))
def test_the_structures_end_at_every_chunk_edge(which):
    rt, ct, ch = _tiles()
    S = max([1, ch - 1, ch, ch + 1][which], 1)
    _check_cloud(S, 20, r_max=4.0, what=f"S = {S}")


@pytest.mark.parametrize("S", [63, 64, 65, 129])
def test_the_structure_axis_is_cut_into_slices(S):
    _check_cloud(S, 20, r_max=4.0, what=f"S = {S}")


# ----------------------------------------------------------------------------- classes and bins
@pytest.mark.parametrize("n_bins", [1, 2, 100, 256])
@pytest.mark.parametrize("C", [1, 2, 8])
def test_classes_and_bins_on_three_tiles(C, n_bins):
    rt, ct, ch = _tiles()
    got = _check_cloud(ch + 1, rt + ct + 1, C=C, n_bins=n_bins, what=f"C = {C}, {n_bins} bins")
    assert got["hist"].shape == (C * (C + 1) // 2, n_bins)
    if C > 1:
        assert (got["hist"].sum(1) > 0).sum() > 1                   # more than one class pair is populated


def test_a_class_that_no_atom_has_leaves_its_rows_zero():
    rt, ct, ch = _tiles()
    C, gone = 8, 5
    got = _check_cloud(3, rt + ct + 1, C=C, missing=gone, what="class 5 is empty")
    rows = [int(R.pair_index(np.int64(a), np.int64(gone), C)) for a in range(C)]
    others = [p for p in range(C * (C + 1) // 2) if p not in rows]
    assert not got["hist"][rows].any() and not got["beyond"][rows].any()
    assert (got["hist"][others].sum(1) + got["beyond"][others] > 0).all()


# ----------------------------------------------------------------------------- one pair, one ulp at a time
def _pair_with(q):
    """Atom 1 of a two-atom structure (atom 0 at the origin) whose ``sq_dist2`` is exactly the float32 ``q``: x a little
    short of sqrt(q), y from the exact remainder (about 2^-9 q: its own rounding is far below half an ulp of q)."""
    x = F(np.sqrt(np.float64(q)) * (1.0 - 2.0 ** -10))
    y = np.sqrt(F(q - x * x))
    p = np.array([x, y, 0.0], F)
    assert R.sq_dist2(p, np.zeros(3, F)) == q
    return p


def _walk(centre, steps=4):
    v, up, down = [F(centre)], F(centre), F(centre)
    for _ in range(steps):
        up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
        v = [down] + v + [up]
    return v


@pytest.mark.parametrize("r_max,n_bins", [(20.0, 100), (7.3, 256), (3.0, 2)])
def test_one_pair_walks_one_ulp_at_a_time_across_bin_edges_and_r_max(r_max, n_bins):
    scale, rmax2 = R.scale_of(r_max, n_bins), R.rmax2_of(r_max)
    edges = sorted({1, max(n_bins // 2, 1), n_bins - 1} - {0})
    centres = [F(F(k) / scale) * F(F(k) / scale) for k in edges]
    qs = [q for c in centres + [rmax2] for q in _walk(c)]
    xyz = np.zeros((len(qs), 2, 3), F)
    xyz[:, 1] = [_pair_with(q) for q in qs]
    none = np.eye(2, dtype=bool)
    want = R.pair_hist(xyz, [0, 1], [0, 0], 1, none, r_max, n_bins)
    got = pairdist.count_pairs(xyz, [0, 1], [0, 0], 1, none, r_max, n_bins, device=DEV)          # S = the steps, one launch
    _same(got, want)
    assert float(got["rmax2"]) == float(rmax2) and float(got["scale"]) == float(scale)
    for i, k in enumerate(edges):                                    # each walk alone: both bins of the edge, nothing else
        one = pairdist.count_pairs(xyz[9 * i:9 * i + 9], [0, 1], [0, 0], 1, none, r_max, n_bins, device=DEV)
        assert np.array_equal(one["hist"], R.pair_hist(xyz[9 * i:9 * i + 9], [0, 1], [0, 0], 1, none, r_max, n_bins)["hist"])
        assert set(np.flatnonzero(one["hist"][0]).tolist()) == {k - 1, k}, (k, one["hist"][0])
    last = pairdist.count_pairs(xyz[-9:], [0, 1], [0, 0], 1, none, r_max, n_bins, device=DEV)
    assert last["beyond"].tolist() == [5] and last["hist"][0, n_bins - 1] == 4 and last["hist"].sum() == 4     # strict: q = rmax2 is beyond


# ----------------------------------------------------------------------------- mask
def test_excluded_pairs_at_the_word_edges():
    m = 70
    xyz = _cloud(5, m)
    ex = np.eye(m, dtype=bool)
    for i, j in ((0, 31), (0, 32), (1, 63), (1, 64), (2, 69), (30, 31), (31, 32), (33, 64), (63, 64), (68, 69)):
        ex[i, j] = ex[j, i] = True
    cls = _runs(m, 2)
    want = R.pair_hist(xyz, np.arange(m), cls, 2, ex, 8.0, 100)
    full = R.pair_hist(xyz, np.arange(m), cls, 2, np.eye(m, dtype=bool), 8.0, 100)
    assert (full["hist"].sum() + full["beyond"].sum()) - (want["hist"].sum() + want["beyond"].sum()) == 5 * 10
    _same(pairdist.count_pairs(xyz, np.arange(m), cls, 2, ex, 8.0, 100, device=DEV), want)
    _same(pairdist.count_pairs(xyz, np.arange(m), cls, 2, np.eye(m, dtype=bool), 8.0, 100, device=DEV), full)


@pytest.mark.parametrize("exclude", [0, 3])
def test_exclude_on_a_chain(exclude):
    m = 70
    xyz, z, bonds = _cloud(5, m), np.where(np.arange(m) % 3 == 0, 7, 6), R.chain_bonds(m)
    got = pairdist.pair_hist(xyz, z, bonds, r_max=8.0, exclude=exclude, device=DEV)
    assert got["class_names"] == ["C", "N"] and got["pair_names"] == ["C-C", "C-N", "N-N"]
    assert np.array_equal(got["excluded"], R.band(m, exclude)) and got["cls"].tolist() == (np.arange(m) % 3 == 0).astype(int).tolist()
    _same(got, R.pair_hist(xyz, np.arange(m), got["cls"], 2, R.band(m, exclude), 8.0, 100))
    if exclude == 0:
        assert got["hist"][:, 18].sum() >= 5 * (m - 1)              # every bond of 1.5 A is in bin 18 of 0.08 A


# ----------------------------------------------------------------------------- bad structures
@pytest.mark.parametrize("parity", [0, 1])
def test_bad_structures_at_the_first_and_last_place_of_chunks_and_slices(parity):
    """A slice is a whole number of chunks, so the two parities together put a bad structure at the first and at the last
    place of every chunk, and with that of every slice."""
    rt, ct, ch = _tiles()
    S, n = 129, 21
    xyz = _cloud(S, n).copy()
    z = np.full(n, 6)
    z[10] = 1                                                       # atom 10 is outside the heavy-atom selection
    sel = np.flatnonzero(z != 1)
    marked = [s for s in range(S) if (s // ch) % 2 == parity and s % ch in (0, ch - 1)] + [S - 1]
    for k, s in enumerate(marked):
        xyz[s, sel[(3 * k) % len(sel)], k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    good_ones = [s for s in range(S) if s not in marked]
    xyz[good_ones[0], 10, 0], xyz[good_ones[-1], 10, 2] = np.nan, np.inf      # unselected: not looked at
    bonds = R.chain_bonds(n)
    got = pairdist.pair_hist(xyz, z, bonds, classes="none", r_max=6.0, device=DEV)
    want = R.pair_hist(xyz, sel, np.zeros(len(sel), int), 1, got["excluded"], 6.0, 100)
    _same(got, want)
    assert np.flatnonzero(got["bad"]).tolist() == sorted(set(marked)) and got["n_good"] == S - len(set(marked))
    clean = R.pair_hist(xyz[good_ones], sel, np.zeros(len(sel), int), 1, got["excluded"], 6.0, 100)
    assert np.array_equal(got["hist"], clean["hist"]) and np.array_equal(got["beyond"], clean["beyond"])


# ----------------------------------------------------------------------------- chunking
def test_any_cut_into_launches_and_a_second_call_give_identical_arrays():
    rt, ct, ch = _tiles()
    S, m = 37, rt + 3
    first = _check_cloud(S, m, C=2, what="one launch", structures_per_launch=S)
    again = _check_cloud(S, m, C=2, what="again", structures_per_launch=S)
    for per_launch in (1, 7):
        cut = _check_cloud(S, m, C=2, what=f"{per_launch} per launch", structures_per_launch=per_launch)
        for k in ("hist", "beyond", "bad"):
            assert np.array_equal(cut[k], first[k]) and np.array_equal(again[k], first[k])


# ----------------------------------------------------------------------------- limits
def test_one_past_each_limit_is_refused_and_writes_nothing():
    lim, lib = pairdist.limits(), _lib.load()
    n = 4
    xyz, eye = np.zeros((2, n, 3), F), np.eye(n, dtype=bool)
    with pytest.raises(ValueError, match="the kernel holds"):
        big = lim["atoms"] + 1
        pairdist.count_pairs(np.zeros((1, big, 3), F), np.arange(big), np.zeros(big, int), 1, np.eye(big, dtype=bool), device=DEV)
    with pytest.raises(ValueError, match="n_classes"):
        pairdist.count_pairs(xyz, np.arange(n), np.zeros(n, int), lim["classes"] + 1, eye, device=DEV)
    with pytest.raises(ValueError, match="n_bins"):
        pairdist.count_pairs(xyz, np.arange(n), np.zeros(n, int), 1, eye, n_bins=lim["bins"] + 1, device=DEV)
    with pytest.raises(ValueError, match="structures_per_launch"):
        pairdist.count_pairs(xyz, np.arange(n), np.zeros(n, int), 1, eye, structures_per_launch=lim["structures"] + 1, device=DEV)
    # the raw entry point, on valid pointers: refused by its sizes before anything is read or written
    dev = torch.device(DEV)
    d_xyz = torch.zeros(2, n, 3, device=dev)
    d_sel, d_cls = torch.arange(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    d_ex = torch.zeros(n, 1, dtype=torch.int32, device=dev)
    hist = torch.full((lim["classes"] * (lim["classes"] + 1) // 2, lim["bins"]), -7, dtype=torch.int64, device=dev)
    beyond, bad = torch.full((hist.shape[0],), -7, dtype=torch.int64, device=dev), torch.full((2,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(1024, device=dev)

    def call(S=2, n_atoms=n, m=n, C=1, n_bins=10):
        rc = lib.cgv_pairdist_counts(_lib.ptr(d_xyz), _lib.ptr(d_sel), _lib.ptr(d_cls), _lib.ptr(d_ex), S, n_atoms, m, C, n_bins, 16.0, 2.5,
                                     _lib.ptr(hist), _lib.ptr(beyond), _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(n_atoms=lim["atoms"] + 1, m=lim["atoms"] + 1), dict(C=lim["classes"] + 1), dict(n_bins=lim["bins"] + 1),
               dict(S=lim["structures"] + 1), dict(C=0), dict(n_bins=0), dict(m=0), dict(m=n + 1)):
        assert call(**kw) != 0, kw
        assert bool((hist == -7).all()) and bool((beyond == -7).all()) and bool((bad == -7).all()), kw
    hist.zero_(), beyond.zero_()
    assert call() == 0                                               # and the same buffers take a valid call
    # two structures of four atoms at one point: six pairs each at d = 0, the first bin of the one class pair
    assert int(hist.view(-1)[0]) == 12 and int(hist.sum()) == 12 and int(beyond.sum()) == 0 and bad.tolist() == [0, 0]


# ----------------------------------------------------------------------------- end to end
def _peptide_sets():
    """Eight jittered frames of one conformer of the three-residue peptide, and four samples of every frame (T = 8, K = 4)."""
    rng = np.random.default_rng(11)
    z, bonds = DR.peptide(3)
    base = np.array([np.pi, -2.0, 2.3, np.pi, -2.0, 2.3, np.pi, -2.0, 2.3, np.pi])
    ref = DR.peptide_structures(3, base[None] + rng.normal(0.0, 0.1, (8, 10)))
    gen = (ref[:, None] + rng.normal(0.0, 0.3, (8, 4) + ref.shape[1:])).astype(F)
    return z, bonds, ref, gen


def test_compare_and_the_command_line_on_a_peptide(tmp_path, capsys):
    z, bonds, ref, gen = _peptide_sets()
    n = z.shape[0]
    np.savez(tmp_path / "ref.npz", xyz=ref, z=z, bonds=bonds, mapping=np.arange(n) // 4)
    np.savez(tmp_path / "gen.npz", xyz=gen)
    out = tmp_path / "pairdist_stats.json"
    capsys.readouterr()
    stats = pairdist.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -pd_rmax 12 -pd_bins 60 -out {out} -device {DEV}".split())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["pairdist_stats"] == json.loads(json.dumps(pairdist.summary_of(stats))) and line["out"] == str(out)
    assert tuple(stats) == pairdist.PAIRDIST_STATS_KEYS
    with open(out) as f:
        assert tuple(json.load(f)) == pairdist.PAIRDIST_STATS_KEYS
    assert (stats["n_ref"], stats["n_gen"], stats["n_bad_ref"], stats["n_bad_gen"], stats["n_atoms"]) == (8, 32, 0, 0, n)
    assert stats["class_names"] == ["C", "N", "O"] and len(stats["pair_names"]) == 6 and len(stats["r"]) == 60
    assert stats["overall"]["jsd"] > stats["overall"]["floor"] >= 0 and stats["overall"]["w1"] > 0
    res = pairdist.pair_hist(gen.reshape(32, n, 3), z, bonds, r_max=12.0, n_bins=60, device=DEV)
    want = R.pair_hist(gen.reshape(32, n, 3), np.arange(n), res["cls"], 3, res["excluded"], 12.0, 60)
    _same(res, want)
    assert stats["overall"]["hist_gen"] == want["hist"].sum(0).tolist()
    assert [stats["pairs"][k]["hist_gen"] for k in stats["pair_names"]] == want["hist"].tolist()
    same = pairdist.main(f"-gen {tmp_path / 'ref.npz'} -ref {tmp_path / 'ref.npz'} -pd_rmax 12 -pd_bins 60 -pd_classes bead -out {out} "
                         f"-device {DEV}".split())
    assert same["overall"]["jsd"] == 0.0 and same["overall"]["w1"] == 0.0 and same["class_names"] == [str(b) for b in range((n + 3) // 4)]
    assert all(b["jsd"] in (0.0, None) and b["w1"] in (0.0, None) for b in same["pairs"].values())
    assert any(b["jsd"] == 0.0 for b in same["pairs"].values())
