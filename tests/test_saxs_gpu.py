"""SAXS histograms on the device: K33 (csrc/saxs_hist.hip) against ``saxs.restate``.  Both sides round every operation
identically: every comparison here is integer EQUALITY, on every entry of ``hist``, ``beyond`` and ``bad``.  The layout has two
paths -- a wave per structure up to ``cgv_saxs_small()`` atoms, ``cgv_saxs_pack()`` structures a block; above that
``cgv_saxs_blocks()`` blocks of 64 x 128 tiles per structure -- and a block stays with one structure, so the structure axis has
no slices: its edges are the packing factor and the caller's chunk."""
import functools
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, saxs
import pairdist_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


@functools.lru_cache(maxsize=None)
def _cloud(S, m, seed=0):
    """``S`` random-walk chains of ``m`` atoms (1.5 A steps) and mixed-sign weights, read-only."""
    rng = np.random.default_rng(1000 * m + S + seed)
    xyz, wq = R.chains(S, m, rng), saxs.quantise(rng.uniform(-4.0, 9.0, m))
    xyz.setflags(write=False), wq.setflags(write=False)
    return xyz, wq


@functools.lru_cache(maxsize=None)
def _want(S, m, r_max, n_bins, seed=0):
    xyz, wq = _cloud(S, m, seed)
    w = saxs.restate(xyz, np.arange(m), wq, r_max, n_bins)
    for k in ("hist", "beyond", "bad"):
        w[k].setflags(write=False)
    return w


def _same(got, want, what=""):
    for k in ("hist", "beyond", "bad"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert got["n_good"] == want["n_good"] and got["self_term"] == want["self_term"] and got["wq_sum"] == want["wq_sum"], what
    good = ~got["bad"]                                               # conservation: every pair of a good structure is somewhere
    if (got["wq"] != 0).all():
        m = got["wq"].shape[0]
        assert ((got["hist"] != 0).sum(1)[good] <= m * (m - 1) // 2).all() and (got["beyond"][good] <= m * (m - 1) // 2).all(), what


def _check_cloud(S, m, r_max=8.0, n_bins=100, what="", **kw):
    xyz, wq = _cloud(S, m)
    want = _want(S, m, r_max, n_bins)
    got = saxs.saxs_hist(xyz, np.arange(m), wq, r_max, n_bins, device=DEV, **kw)
    _same(got, want, what)
    if m > 8:                                                       # a case with nothing in range, or nothing beyond, proves little
        assert want["hist"].any() and want["beyond"].sum() > 0, what
    return got


# ----------------------------------------------------------------------------- atoms: every tile edge, both paths
@pytest.mark.parametrize("m", [1, 2, 3, 22, 63, 64, 65, 127, 128, 129, 193])
def test_the_selection_ends_at_every_tile_edge(m):
    lib = _lib.load()
    assert (lib.cgv_saxs_row_tile(), lib.cgv_saxs_col_tile(), lib.cgv_saxs_small()) == (64, 128, 64)      # what the sizes above are about
    got = _check_cloud(3, m, what=f"m = {m}")
    if m == 1:
        assert not got["hist"].any() and not got["beyond"].any()    # no pairs


@pytest.mark.parametrize("m", [21, 22])
def test_a_wave_meets_every_pair_once_for_odd_and_even_sizes(m):
    """Nothing beyond, weights of one sign: the sum of a row is sum_{i<j} wq_i wq_j exactly -- a pair met twice or not at all
    (the half-turn step of an even m) would show."""
    xyz, _ = _cloud(5, m)
    wq = saxs.quantise(np.arange(1, m + 1, dtype=np.float64))
    got = saxs.saxs_hist(xyz, np.arange(m), wq, 100.0, 1000, device=DEV)
    _same(got, saxs.restate(xyz, np.arange(m), wq, 100.0, 1000))
    assert (got["self_term"] + 2 * got["hist"].sum(1) == got["wq_sum"] ** 2).all() and not got["beyond"].any()


# ----------------------------------------------------------------------------- structures: packing, chunks, blocks
@pytest.mark.parametrize("n_bins,pack", [(100, 4), (2048, 2), (4096, 1)])
def test_the_structures_end_at_every_edge_of_the_packing_factor(n_bins, pack):
    assert _lib.load().cgv_saxs_pack(22, n_bins) == pack
    for S in sorted({max(pack - 1, 1), pack, pack + 1, 2 * pack + 1}):
        _check_cloud(S, 22, r_max=6.0, n_bins=n_bins, what=f"S = {S}, pack {pack}")


@pytest.mark.parametrize("m", [22, 70])
def test_the_structures_end_at_every_edge_of_the_chunk(m):
    S = 33
    first = _check_cloud(S, m, what="one launch", chunk=S)
    for chunk in (1, 7, 32, 4096):                                  # 33 = 32 + 1: one below, at and above a launch's end
        cut = _check_cloud(S, m, what=f"chunk {chunk}", chunk=chunk)
        for k in ("hist", "beyond", "bad"):
            assert np.array_equal(cut[k], first[k])


@pytest.mark.parametrize("split", [0, 1, 2, 3, 4])
def test_the_tiles_of_a_structure_span_several_blocks(split):
    lib = _lib.load()
    S, m = 3, 193                                                   # four row tiles, two column tiles
    assert lib.cgv_saxs_blocks(S, m, split) == (4 if split == 0 else split)
    _check_cloud(S, m, what=f"split {split}", split=split)


# ----------------------------------------------------------------------------- bin edges
def _pair_with(q):
    """Atom 1 of a two-atom structure (atom 0 at the origin) whose ``sq_dist2`` is exactly the float32 ``q``."""
    x = F(np.sqrt(np.float64(q)) * (1.0 - 2.0 ** -10))
    y = np.sqrt(F(q - x * x))
    p = np.array([x, y, 0.0], F)
    assert R.sq_dist2(p, np.zeros(3, F)) == q
    return p


def _walk(centre, steps=2):
    v, up, down = [F(centre)], F(centre), F(centre)
    for _ in range(steps):
        up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
        v = [down] + v + [up]
    return v


@pytest.mark.parametrize("r_max,n_bins", [(20.0, 200), (7.3, 4096), (3.0, 2)])
def test_one_pair_walks_across_bin_edges_and_r_max(r_max, n_bins):
    scale, rmax2 = R.scale_of(r_max, n_bins), R.rmax2_of(r_max)
    edges = sorted({1, max(n_bins // 2, 1), n_bins - 1} - {0})
    centres = [F(F(k) / scale) * F(F(k) / scale) for k in edges]
    qs = [q for c in centres + [rmax2] for q in _walk(c)]           # the last five straddle r_max: its own value is beyond (strict)
    xyz = np.zeros((len(qs), 2, 3), F)
    xyz[:, 1] = [_pair_with(q) for q in qs]
    wq = np.array([48, -32], np.int32)
    want = saxs.restate(xyz, [0, 1], wq, r_max, n_bins)
    got = saxs.saxs_hist(xyz, [0, 1], wq, r_max, n_bins, device=DEV)
    _same(got, want)
    assert float(got["rmax2"]) == float(rmax2) and float(got["scale"]) == float(scale)
    assert got["beyond"][-5:].tolist() == [0, 0, 1, 1, 1] and got["hist"][-5:, n_bins - 1].tolist() == [-1536, -1536, 0, 0, 0]
    for i, k in enumerate(edges):                                    # each walk: both bins of the edge, nothing else
        rows = got["hist"][5 * i:5 * i + 5]
        assert set(np.flatnonzero(rows.any(0)).tolist()) == {k - 1, k} and (rows.sum(1) == -1536).all(), k


def test_coincident_atoms_land_in_bin_0_and_a_pair_exactly_at_r_max_is_beyond():
    xyz = np.zeros((2, 3, 3), F)
    xyz[1, :, 0] = [0.0, 2.5, 5.0]                                   # d01 = d12 = 2.5 (a bin edge of 0.5 A bins), d02 = r_max exactly
    got = saxs.saxs_hist(xyz, [0, 1, 2], [16, 32, 48], 5.0, 10, device=DEV)
    assert got["hist"][0].tolist() == [16 * 32 + 16 * 48 + 32 * 48] + [0] * 9 and got["beyond"].tolist() == [0, 1]
    assert got["hist"][1].tolist() == [0] * 5 + [16 * 32 + 32 * 48] + [0] * 4
    _same(got, saxs.restate(xyz, [0, 1, 2], [16, 32, 48], 5.0, 10))


# ----------------------------------------------------------------------------- weights, bins
@pytest.mark.parametrize("m", [9, 70])
@pytest.mark.parametrize("kind", ["extreme", "zero", "negative"])
def test_weights_at_their_limits_zero_and_all_negative(kind, m):
    xyz, _ = _cloud(5, m)
    rng = np.random.default_rng(m)
    wq = {"extreme": np.where(rng.random(m) < 0.5, 32767, -32767), "zero": np.zeros(m, int),
          "negative": -rng.integers(1, 200, m)}[kind].astype(np.int32)
    want = saxs.restate(xyz, np.arange(m), wq, 8.0, 40)
    got = saxs.saxs_hist(xyz, np.arange(m), wq, 8.0, 40, device=DEV)
    _same(got, want, kind)
    if kind == "zero":
        assert not got["hist"].any() and got["beyond"].sum() > 0 or m <= 9          # a zero product adds nothing; beyond counts pairs
    if kind == "negative":
        assert (got["hist"] >= 0).all() and got["hist"].any()
    if kind == "extreme":
        assert np.abs(got["hist"]).max() >= 32767 ** 2 and (got["hist"] % (32767 ** 2) == 0).all()


@pytest.mark.parametrize("m", [22, 129])
@pytest.mark.parametrize("n_bins", [1, 4096])
def test_one_bin_and_the_most_bins(n_bins, m):
    got = _check_cloud(5, m, r_max=9.0, n_bins=n_bins, what=f"{n_bins} bins")
    assert got["hist"].shape == (5, n_bins)


# ----------------------------------------------------------------------------- bad structures
@pytest.mark.parametrize("m_extra", [0, 60])
def test_bad_structures_give_a_zero_row_and_unselected_atoms_are_not_looked_at(m_extra):
    S, n = 11, 23 + m_extra
    xyz = _cloud(S, n)[0].copy()
    sel = np.array([i for i in range(n) if i != 10])                # atom 10 is outside the selection
    wq = saxs.quantise(np.linspace(-2.0, 7.0, n - 1))
    xyz[0, sel[0], 0], xyz[4, sel[-1], 2], xyz[5, sel[7], 1], xyz[S - 1, sel[3], 0] = np.nan, np.inf, -np.inf, np.nan
    xyz[1, 10, 0], xyz[9, 10, 2] = np.nan, np.inf                    # unselected: the structures stay good
    want = saxs.restate(xyz, sel, wq, 8.0, 80)
    got = saxs.saxs_hist(xyz, sel, wq, 8.0, 80, device=DEV)
    _same(got, want)
    assert np.flatnonzero(got["bad"]).tolist() == [0, 4, 5, S - 1] and got["n_good"] == S - 4
    assert not got["hist"][got["bad"]].any() and not got["beyond"][got["bad"]].any()
    assert got["hist"][1].any() and got["hist"][9].any()


# ----------------------------------------------------------------------------- into
@pytest.mark.parametrize("m", [22, 70])
def test_three_unequal_launches_through_into_equal_one(m):
    S = 19
    xyz, wq = _cloud(S, m)
    sel = np.arange(m)
    whole = _check_cloud(S, m)
    part = None
    for lo, hi in ((0, 2), (2, 13), (13, S)):
        part = saxs.saxs_hist(xyz[lo:hi], sel, wq, 8.0, 100, into=part, device=DEV)
    _same(part, whole, "into")
    with pytest.raises(ValueError, match="another selection"):
        saxs.saxs_hist(xyz[:2], sel, wq, 8.0, 101, into=part, device=DEV)


# ----------------------------------------------------------------------------- end to end
def test_compare_through_the_command_line_equals_compare_from_hists_of_the_restatement(tmp_path, capsys):
    rng = np.random.default_rng(4)
    S, n = 64, 40
    z = np.tile(np.array([6, 1, 7, 6, 8]), n // 5)
    bonds = R.chain_bonds(n)
    ref = R.chains(S, n, rng)
    gen = (R.chains(S, n, rng, step=1.4) + rng.normal(0.0, 0.2, (S, n, 3))).astype(F)
    gen[5] *= 4.0                                                    # one generated structure reaches beyond the reference's r_max
    gen[9, 0, 0] = np.nan                                            # and one is bad
    np.savez(tmp_path / "ref.npz", xyz=ref, z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=gen)
    curve = tmp_path / "curve.dat"
    sel = np.flatnonzero(z != 1)
    wq = saxs.quantise(saxs.weights_of(z, bonds, sel))
    r_max, n_bins = saxs.default_r_max(ref, sel, 0.25)
    truth = saxs.restate(ref[:1], sel, wq, r_max, n_bins)
    qe = np.linspace(0.02, 0.4, 20)
    ie = 1e-3 * saxs.profile(truth["hist"][0], truth["self_term"], qe, truth["r_max"])
    curve.write_text("# q I sigma\n" + "".join(f"{a!r} {b!r} {0.02 * b!r}\n" for a, b in zip(qe.tolist(), ie.tolist())))
    out, prof = tmp_path / "saxs_stats.json", tmp_path / "profiles.npz"
    capsys.readouterr()
    stats = saxs.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -saxs_bin 0.25 -saxs_nq 26 -saxs_exp {curve} "
                      f"-profiles {prof} -out {out} -device {DEV}".split())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["saxs_stats"] == json.loads(json.dumps(saxs.summary_of(stats))) and line["out"] == str(out)
    assert tuple(stats) == saxs.SAXS_STATS_KEYS
    # the same floats from the restatement's integers: the host maths is shared
    even, odd, got = (saxs.restate(x, sel, wq, r_max, n_bins) for x in (ref[0::2], ref[1::2], gen))
    want = saxs.compare_from_hists(even, odd, got, saxs.q_grid(0.5, 26), exp=saxs.read_curve(str(curve)),
                                   params=saxs.params_of(wq, r_max, n_bins, background=False), enough=r_max)
    assert stats == want
    with open(out) as f:
        assert json.load(f) == json.loads(json.dumps(want))
    assert (stats["n_ref"], stats["n_gen"], stats["n_bad_ref"], stats["n_bad_gen"], stats["n_beyond_gen"], stats["n_atoms"]) == (64, 64, 0, 1, 1, len(sel))
    assert stats["log_rms"] > stats["floor"] >= 0 and stats["rg"]["jsd"] >= 0 and stats["dmax"]["max_ref"] <= r_max
    assert stats["exp"]["structures"]["min"] >= 0 and stats["exp"]["ref"]["chi2"] >= 0 and len(stats["exp"]["structures"]["values"]) == 62
    with np.load(prof) as f:
        assert f["profiles"].shape == (S, 26) and f["bad"].tolist() == got["bad"].tolist() and np.array_equal(f["beyond"], got["beyond"])
