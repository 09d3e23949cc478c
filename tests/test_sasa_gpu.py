"""Solvent-accessible surface on the device: K23 (csrc/sasa.hip) against the numpy restatement.  A point is buried by a
threshold on an fp32 sum that both sides round identically, and "buried by some atom" does not depend on which atoms the
kernel's pre-filter drops or in which order it tries the rest: every comparison here is integer EQUALITY."""
import functools
import json
import math

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, sasa
import density_restatement as DR
import sasa_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTS = ("counts", "class_counts", "atom_sum", "atom_sumsq", "bad")
ELEMENTS = np.array([1, 6, 7, 8, 16])


def _want(xyz, z, sel, P, classes=None, probe=1.4):
    sel = np.arange(len(z)) if sel is None else np.asarray(sel)
    r = R.inflated([R.BONDI[int(a)] for a in np.asarray(z)[sel]], probe)
    cls, ids, _ = sasa.device_classes(classes, r)
    want = R.sasa_counts(xyz, sel, r, P, cls, ids.shape[0])
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want


def _same(got, want, what=""):
    assert got["n_good"] == want["n_good"], what
    for k in INTS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _check(xyz, z, sel=None, P=64, classes=None, what="", **kw):
    got = sasa.sasa_counts(xyz, z, sel, n_points=P, classes=classes, per_atom=True, device=DEV, **kw)
    _same(got, _want(xyz, z, sel, P, classes), what)
    return got


@functools.lru_cache(maxsize=None)
def _molecule(m, S, sigma, P, seed=0):
    """``m`` atoms of mixed elements drawn from N(0, sigma) in ``S`` structures, and the restatement's result."""
    rng = np.random.default_rng(1000 * m + 10 * S + seed)
    z = ELEMENTS[rng.integers(0, len(ELEMENTS), m)]
    xyz = rng.normal(0, sigma, (S, m, 3)).astype(np.float32)
    return xyz, z, _want(xyz, z, None, P)


# ----------------------------------------------------------------------------- one and two atoms
@pytest.mark.parametrize("P", [1, 63, 64, 65, 256, 1000])
def test_one_atom_and_two_atoms_tangent_overlapping_and_nested(P):
    z = np.array([6, 8])
    r = R.inflated([1.7, 1.52])
    lone = _check(np.array([[[0.3, -1.0, 2.0], [9.0, 9.0, 9.0]]], np.float32), z, sel=[0], P=P, what="m = 1")
    assert lone["counts"].tolist() == [[P]] and lone["atom_sum"].tolist() == [P] and lone["atom_sumsq"].tolist() == [P * P]
    tangent = float(np.float32(r[0] + r[1]))
    xyz = np.array([[[0, 0, 0], [0, 0, d]] for d in (tangent, 2.5, 0.1)], np.float32)
    got = _check(xyz, z, P=P, what="m = 2")
    assert got["counts"][2, 1] == 0 and got["counts"][2, 0] == P              # O inside C's sphere: buried; C untouched
    for s in (0, 1):
        d = float(xyz[s, 1, 2])
        if not (R.near_tie(P, d, r[0], r[1]) or R.near_tie(P, d, r[1], r[0])):
            assert got["counts"][s].tolist() == [R.cap_count(P, d, r[0], r[1], 1.0), R.cap_count(P, d, r[1], r[0], -1.0)]


@pytest.mark.parametrize("shift", [0.0, 500.0])
def test_pairs_within_two_ulps_of_the_pre_filters_edge(shift):
    """Two atoms at d = r_i + r_j along each axis, the second one's coordinate moved by -2 .. +2 ulps: whatever the
    pre-filter keeps, the counts are the restatement's."""
    z = np.array([6, 16])
    r = R.inflated([1.7, 1.8])
    xyz = []
    for axis in range(3):
        for ulps in range(-2, 3):
            a = np.full(3, shift, dtype=np.float32)
            b = a.copy()
            b[axis] = np.float32(b[axis] + np.float32(r[0] + r[1]))
            for _ in range(abs(ulps)):
                b[axis] = np.nextafter(b[axis], np.float32(np.inf if ulps > 0 else -np.inf))
            xyz.append([a, b])
    got = _check(np.array(xyz, np.float32), z, P=256, what=f"shift {shift}")
    assert (got["counts"] >= 250).all() and not got["bad"].any()


# ----------------------------------------------------------------------------- random molecules
def test_a_300_atom_molecule_also_far_from_the_origin():
    """N(0, 6 A), 256 points; the third structure is the first moved by 5000 A, beyond the magnitude the pre-filter's
    derivation covers: it takes the unfiltered loop, is not bad, and still equals the restatement.  With 3 structures the
    atoms of a structure are split over 19 workgroups."""
    xyz, z, _ = _molecule(300, 2, 6.0, 256)
    x3 = np.concatenate([xyz, xyz[:1] + np.float32(5000.0)])
    got = _check(x3, z, P=256, what="300 atoms")
    assert not got["bad"].any() and 0 < (got["counts"] == 0).mean() < 1 and got["counts"].max() <= 256


def test_a_collapsed_molecule_where_every_atom_is_every_atoms_occluder():
    xyz, z, want = _molecule(200, 2, 0.5, 64)
    got = sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, device=DEV)
    _same(got, want, "collapsed")
    assert (got["counts"] == 0).mean() > 0.5


@pytest.mark.parametrize("m", [64, 65, 129])
def test_wave_and_tile_boundaries(m):
    xyz, z, want = _molecule(m, 3, 3.0, 64)
    _same(sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, device=DEV), want, f"m {m}")


def test_more_structures_than_workgroups():
    """1100 structures of 10 atoms: the grid is 1024 workgroups, so some take a second structure."""
    xyz, z, want = _molecule(10, 1100, 2.0, 64)
    _same(sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, device=DEV), want, "S 1100")


@pytest.mark.parametrize("S,P", [(1, 8), (1024, 4)])
def test_the_largest_molecule_the_kernel_holds(S, P):
    """4096 atoms, N(0, 12 A): the staged atoms and the lists need more than 64 KB of LDS.  One structure is split
    over 256 workgroups of 16 atoms; 1024 copies of it are one workgroup each, which then holds the sums of all 4096 atoms
    as well -- the 160 000 bytes the limit was sized for.  Few points keep the restatement quick."""
    xyz, z, want = _molecule(sasa.limits()["atoms"], 1, 12.0, P)
    got = sasa.sasa_counts(np.repeat(xyz, S, axis=0), z, n_points=P, per_atom=True, device=DEV)
    assert np.array_equal(got["counts"], np.repeat(want["counts"], S, axis=0)) and not got["bad"].any()
    assert np.array_equal(got["class_counts"], np.repeat(want["class_counts"], S, axis=0))
    assert np.array_equal(got["atom_sum"], S * want["atom_sum"]) and np.array_equal(got["atom_sumsq"], S * want["atom_sumsq"])
    assert 0 < got["counts"].mean() < P


# ----------------------------------------------------------------------------- selection
def test_unselected_atoms_do_not_occlude_and_the_selection_keeps_its_order():
    xyz, z, _ = _molecule(65, 3, 3.0, 64)
    sel = np.random.default_rng(5).permutation(65)[:40]
    got = _check(xyz, z, sel=sel, P=64, what="subset")
    alone = sasa.sasa_counts(np.ascontiguousarray(xyz[:, sel]), z[sel], n_points=64, per_atom=True, device=DEV)
    _same(got, alone, "subset against the molecule cut out")
    everyone = sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, device=DEV)
    assert (everyone["counts"][:, sel] <= got["counts"]).all() and (everyone["counts"][:, sel] < got["counts"]).any()


def test_two_selected_atoms_at_identical_coordinates():
    xyz, z, _ = _molecule(64, 3, 3.0, 64)
    x = xyz.copy()
    x[:, 7] = x[:, 3]
    z2 = z.copy()
    z2[3], z2[7] = 1, 16                                                        # the hydrogen sits inside the sulfur
    got = _check(x, z2, P=64, what="identical coordinates")
    assert (got["counts"][:, 3] == 0).all()


# ----------------------------------------------------------------------------- structures, launches, sums
@pytest.mark.parametrize("S", [1, 3, 4, 5])
def test_structure_counts_around_the_launch_size(S):
    xyz, z, _ = _molecule(65, 5, 3.0, 64)
    _check(xyz[:S], z, P=64, structures_per_launch=4, what=f"S {S}")


def test_sums_accumulated_over_launches_equal_those_of_one_launch():
    xyz, z, want = _molecule(65, 5, 3.0, 64)
    one = sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, device=DEV)
    two = sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, structures_per_launch=2, device=DEV)
    _same(two, one)
    _same(one, want)
    good = want["counts"].astype(np.int64)
    assert np.array_equal(one["atom_sum"], good.sum(0)) and np.array_equal(one["atom_sumsq"], (good * good).sum(0))


def test_nan_and_inf_structures_are_flagged_and_enter_no_sum():
    xyz, z, _ = _molecule(65, 5, 3.0, 64)
    sel = np.arange(1, 65)
    x = xyz.copy()
    x[0, 0, 1] = np.nan                                                        # outside the selection: of no consequence
    x[1, 64, 2] = np.nan
    x[3, 1, 0] = np.inf
    got = _check(x, z, sel=sel, P=64, structures_per_launch=2, what="bad structures")
    assert got["bad"].tolist() == [False, True, False, True, False] and got["n_good"] == 3
    assert (got["counts"][[1, 3]] == -1).all() and (got["class_counts"][[1, 3]] == -1).all()
    clean = sasa.sasa_counts(x[[0, 2, 4]], z, sel, n_points=64, per_atom=True, device=DEV)
    assert np.array_equal(got["atom_sum"], clean["atom_sum"]) and np.array_equal(got["atom_sumsq"], clean["atom_sumsq"])
    assert np.array_equal(got["counts"][[0, 2, 4]], clean["counts"])
    a = sasa.areas(got)
    assert np.isnan(a["total"][[1, 3]]).all() and np.isfinite(a["total"][[0, 2, 4]]).all()


def test_class_counts_are_the_atom_counts_summed_by_class():
    xyz, z, _ = _molecule(129, 3, 3.0, 64)
    classes = sasa.polarity(z)
    full = _check(xyz, z, P=64, classes=classes, what="classes")
    short = sasa.sasa_counts(xyz, z, n_points=64, classes=classes, device=DEV)
    assert "counts" not in short
    for k in ("class_counts", "atom_sum", "atom_sumsq", "bad"):
        assert np.array_equal(short[k], full[k]), k
    cls, ids, cr = sasa.device_classes(classes, full["r"])
    assert np.array_equal(full["class_ids"], ids) and np.array_equal(full["class_r"], cr) and len(ids) == len(set(zip(classes, full["r"])))
    for c in range(len(ids)):
        assert np.array_equal(full["class_counts"][:, c], full["counts"][:, cls == c].sum(axis=1))
    a = sasa.areas(full)
    per_atom = 4 * math.pi * full["r"].astype(np.float64) ** 2 / 64 * full["counts"]
    assert np.allclose(a["total"], per_atom.sum(axis=1), rtol=1e-12)
    assert np.allclose(a["by_class"][:, 0], per_atom[:, classes == 0].sum(axis=1), rtol=1e-12)
    assert np.allclose(a["mean"], per_atom.mean(axis=0), rtol=1e-12) and np.allclose(a["std"], per_atom.std(axis=0), rtol=1e-9, atol=1e-9)


def test_two_calls_give_identical_bytes():
    xyz, z, _ = _molecule(129, 3, 3.0, 64)
    a = sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, device=DEV)
    b = sasa.sasa_counts(xyz, z, n_points=64, per_atom=True, device=DEV)
    for k in INTS:
        assert a[k].tobytes() == b[k].tobytes(), k


# ----------------------------------------------------------------------------- limits
def test_every_limit_is_refused_before_a_launch_with_a_message():
    lim = sasa.limits()
    z = np.full(lim["atoms"] + 1, 6)
    with pytest.raises(ValueError, match="the kernel holds"):
        sasa.sasa_counts(np.zeros((1, lim["atoms"] + 1, 3), np.float32), z, device=DEV)
    with pytest.raises(ValueError, match="n_points must be"):
        sasa.sasa_counts(np.zeros((1, 4, 3), np.float32), z[:4], n_points=lim["points"] + 1, device=DEV)
    with pytest.raises(ValueError, match="distinct"):
        sasa.sasa_counts(np.zeros((1, 65, 3), np.float32), z[:65], classes=np.arange(65), device=DEV)
    with pytest.raises(ValueError, match="twice"):
        sasa.sasa_counts(np.zeros((1, 4, 3), np.float32), z[:4], sel=[0, 1, 1], device=DEV)
    with pytest.raises(ValueError, match="atomic number 26"):
        sasa.sasa_counts(np.zeros((1, 4, 3), np.float32), [6, 6, 26, 6], device=DEV)
    for args, match in (((lim["structures"] + 1, 8, 4, 64, 1), "max_structures"), ((1, 8, lim["atoms"] + 1, 64, 1), "1 <= m"),
                        ((1, lim["atoms"] + 8, lim["atoms"] + 1, 64, 1), "max_atoms"), ((1, 8, 4, lim["points"] + 1, 1), "max_points"),
                        ((1, 8, 4, 64, lim["classes"] + 1), "max_classes")):
        with pytest.raises(RuntimeError, match=match):                         # the C ABI itself: no pointer is looked at
            _lib.call("cgv_sasa_counts", None, None, None, None, None, *args, None, None, None, None, None, None, 0, None)


# ----------------------------------------------------------------------------- end to end
def _peptide_sets():
    rng = np.random.default_rng(4)
    z, bonds = DR.peptide(3)
    tors = np.full((32, 10), math.pi)
    tors[:, 1::3], tors[:, 2::3] = rng.normal(-1.2, 0.4, (32, 3)), rng.normal(2.4, 0.5, (32, 3))
    ref = DR.peptide_structures(3, tors)
    gen = (ref[:12] + rng.normal(0, 0.3, (12,) + ref.shape[1:])).astype(np.float32)
    return z, bonds, ref, gen


def test_compare_and_the_command_line_on_a_three_residue_peptide(tmp_path, capsys):
    z, bonds, ref, gen = _peptide_sets()
    stats = sasa.compare(ref, gen, z, bonds, n_points=64, device=DEV)
    assert tuple(stats) == sasa.SASA_STATS_KEYS and json.loads(json.dumps(stats)) == stats
    assert stats["n_ref"] == 32 and stats["n_gen"] == 12 and stats["n_bad_ref"] == stats["n_bad_gen"] == 0
    assert stats["labels"] == list(range(len(z))) and stats["params"]["atoms"] == list(range(len(z)))
    assert stats["params"]["radii"] == {"6": 1.7, "7": 1.55, "8": 1.52} and stats["params"]["n_points"] == 64
    even, odd = (sasa.areas(sasa.sasa_counts(ref[k::2], z, n_points=64, device=DEV)) for k in (0, 1))
    assert np.allclose(stats["mean_ref"], 0.5 * (even["mean"] + odd["mean"]), rtol=1e-12)
    assert stats["total"]["mean_ref"] == pytest.approx(np.concatenate([even["total"], odd["total"]]).mean())
    assert 0 < stats["apolar_fraction"]["mean_ref"] < 1 and stats["profile_rmse"] > 0 and len(stats["top_atoms"]) == 10
    by_residue = sasa.compare(ref, gen, z, bonds, n_points=64, groups="residue", device=DEV)
    assert by_residue["labels"] == [0, 1, 2] and sum(by_residue["mean_ref"]) == pytest.approx(sum(stats["mean_ref"]))
    np.savez(tmp_path / "ref.npz", xyz=ref, z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=gen.reshape(4, 3, len(z), 3))
    out = tmp_path / "stats.json"
    sasa.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -sasa_points 64 -out {out}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert json.loads(out.read_text()) == stats and line["sasa_stats"] == sasa.summary_of(stats)
