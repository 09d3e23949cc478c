"""lDDT and clashes on the device: K28 (csrc/lddt.hip) against the numpy restatement.  Every test of the kernel is a strict
comparison of fp32 values that both sides round identically: every comparison here is integer EQUALITY, on every output."""
import functools
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, contacts, lddt
import density_restatement as DR
import lddt_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUTPUTS = ("struct_counts", "atom_counts", "bad")
F = np.float32


def _frozen(w):
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def _same(got, want, what=""):
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    assert got["n_good"] == int((~want["bad"]).sum()), what


def _invariant(res):
    good = ~res["bad"]
    assert np.array_equal(res["atom_counts"].sum(0), 2 * res["struct_counts"][good].sum(0))
    assert (res["struct_counts"][~good] == -1).all()


def _guard(want, what=""):
    """A case with nothing or everything counted proves nothing: the restatement's own shares, before any comparison."""
    sh = R.shares(want)
    assert 0.30 <= sh["included"] <= 0.95, (what, sh)
    assert all(0.05 <= p <= 0.95 for p in sh["preserved"]), (what, sh)
    assert 0.01 <= sh["clash"] <= 0.50, (what, sh)


@functools.lru_cache(maxsize=None)
def _cloud(n, idx, T, seed=0):
    """A chain of ``n`` carbons: ``T`` independent random-walk references, a structure per entry of ``idx`` -- its reference
    plus noise of 1.5 A --, the tables, and the restatement's result at ``R.cloud_radius(n)``."""
    rng = np.random.default_rng(1000 * n + 10 * T + len(idx) + seed)
    ref = np.stack([R.chain(n, rng) for _ in range(T)])
    xyz = np.stack([R.noisy(ref[t], 1, 1.5, rng)[0] for t in idx])
    z, bonds = np.full(n, 6), R.chain_bonds(n)
    excl = contacts.excluded_pairs(bonds, n, np.arange(n), 3)
    want = _frozen(R.lddt_counts(xyz, ref, idx, np.arange(n), excl, excl, np.full(n, 1.7), R0=R.cloud_radius(n)))
    xyz.setflags(write=False), ref.setflags(write=False)
    return xyz, ref, z, bonds, want


def _run(xyz, ref, z, bonds, idx, n, **kw):
    return lddt.lddt_counts(xyz, ref, z, bonds, ref_index=np.asarray(idx), inclusion_radius=R.cloud_radius(n), device=DEV, **kw)


def _check_cloud(n, idx, T, what="", seed=0, **kw):
    xyz, ref, z, bonds, want = _cloud(n, tuple(int(i) for i in idx), T, seed)
    _guard(want, what)
    got = _run(xyz, ref, z, bonds, idx, n, **kw)
    _same(got, want, what)
    _invariant(got)
    return got


# ----------------------------------------------------------------------------- one pair, one ulp at a time
def _ulp_sweep(centre, steps=40):
    v = [F(centre)]
    for _ in range(steps):
        v.append(np.nextafter(v[-1], F(np.inf)))
    lo = [F(centre)]
    for _ in range(steps):
        lo.append(np.nextafter(lo[-1], F(-np.inf)))
    return np.array(lo[:0:-1] + v, dtype=F)                       # -40 .. +40 ulps


def _two_atoms(x1, ref1, shift=0.0):
    """Structures of two atoms on the x axis: atom 0 at ``shift``, atom 1 at the given coordinates."""
    xyz = np.zeros((len(x1), 2, 3), F)
    ref = np.zeros((len(ref1), 2, 3), F)
    xyz[:, :, 0], ref[:, :, 0] = F(shift), F(shift)
    xyz[:, 1, 0], ref[:, 1, 0] = x1, ref1
    return xyz, ref


def _pair_counts(xyz, ref, idx):
    z, bonds, none = np.array([6, 6]), np.zeros((0, 2), dtype=int), np.eye(2, dtype=bool)
    want = R.lddt_counts(xyz, ref, idx, [0, 1], none, none, [1.7, 1.7])
    got = lddt.lddt_counts(xyz, ref, z, bonds, ref_index=np.asarray(idx), exclude=0, device=DEV)
    _same(got, want)
    _invariant(got)
    return got["struct_counts"]


@pytest.mark.parametrize("shift", [0.0, 500.0])
def test_one_pair_swept_across_each_threshold_one_ulp_at_a_time(shift):
    d0 = 5.0
    x1 = np.concatenate([_ulp_sweep(shift + d0 + tk) for tk in (0.5, 1.0, 2.0, 4.0)] +
                        [_ulp_sweep(shift + d0 - tk) for tk in (0.5, 1.0, 2.0, 4.0)])
    xyz, ref = _two_atoms(x1, [F(shift + d0)], shift)
    sc = _pair_counts(xyz, ref, np.zeros(len(x1), dtype=int))
    assert (sc[:, 0] == 1).all()
    for side in range(2):
        for k in range(4):
            crossed = int(sc[81 * (4 * side + k):81 * (4 * side + k + 1), 1 + k].sum())
            assert 0 < crossed < 81, (shift, side, k, crossed)


def test_the_reference_distance_swept_across_the_inclusion_radius():
    r1 = _ulp_sweep(15.0)
    xyz, ref = _two_atoms(r1, r1)                                  # every structure against its own reference
    sc = _pair_counts(xyz, ref, np.arange(len(r1)))
    assert 0 < int(sc[:, 0].sum()) < 81 and np.array_equal(sc[:, 4], sc[:, 0])


def test_the_distance_swept_across_the_clash_bound():
    c = (F(1.7) + F(1.7)) - F(0.4)
    x1 = _ulp_sweep(c)
    xyz, ref = _two_atoms(x1, [F(3.0)])
    sc = _pair_counts(xyz, ref, np.zeros(len(x1), dtype=int))
    assert 0 < int(sc[:, 5].sum()) < 81


# ----------------------------------------------------------------------------- tiles
SEEDS = {64: 1, 129: 1}        # the draw of seed 0 is a compact walk there: the guard rejects it (included share > 0.95)


def _tile_sizes():
    lib = _lib.load()
    rt, ct = int(lib.cgv_lddt_row_tile()), int(lib.cgv_lddt_col_tile())
    return sorted({rt - 1, rt, rt + 1, ct - 1, ct, ct + 1, 2 * ct + 1})


@pytest.mark.parametrize("which", range(7))
def test_the_selection_ends_at_every_tile_boundary(which):
    sizes = _tile_sizes()
    if which >= len(sizes):
        return                                                     # fewer distinct boundaries than the seven named ones
    _check_cloud(sizes[which], (0, 0, 0), 1, what=f"m = {sizes[which]}", seed=SEEDS.get(sizes[which], 0))


# ----------------------------------------------------------------------------- ref_index
def _chunk():
    return int(_lib.load().cgv_lddt_chunk())


def test_a_new_reference_for_every_structure_and_one_for_all():
    S = 2 * _chunk() + 4
    _check_cloud(31, range(S), S, "T = S")
    _check_cloud(31, [0] * S, 1, "T = 1")


def test_a_reference_changes_inside_a_staged_chunk():
    T = _chunk() + 1
    got = _check_cloud(31, np.repeat(np.arange(T), 3), T, "K = 3")
    assert got["ref_index"].tolist() == lddt.default_ref_index(3 * T, T).tolist()


def test_a_shuffled_ref_index():
    idx = np.random.default_rng(4).integers(0, 5, 40)
    assert (np.diff(idx) < 0).any() and (np.diff(idx) > 0).any()
    _check_cloud(31, idx, 5, "shuffled")


def test_several_slices_twice_with_identical_arrays():
    idx = np.arange(1100) % 4
    first = _check_cloud(31, idx, 4, "S = 1100")
    second = _check_cloud(31, idx, 4, "S = 1100, again")
    for k in OUTPUTS:
        assert np.array_equal(first[k], second[k])


@pytest.mark.parametrize("per_launch", [7, 1])
def test_launch_cuts_inside_a_run_of_equal_ref_index(per_launch):
    _check_cloud(31, np.arange(37) // 8, 5, f"{per_launch} per launch", structures_per_launch=per_launch)


# ----------------------------------------------------------------------------- bad structures
def test_bad_structures_are_minus_one_and_enter_no_sum():
    idx = tuple(np.arange(12) // 4)
    xyz, ref, z, bonds, clean = _cloud(31, idx, 3)
    _guard(clean)
    z = z.copy()
    z[10] = 1                                                      # atom 10 is outside the heavy-atom selection
    sel = np.flatnonzero(z != 1)
    excl = contacts.excluded_pairs(bonds, 31, sel, 3)
    radii = np.full(30, 1.7)
    kw = dict(R0=R.cloud_radius(31))
    base = R.lddt_counts(xyz, ref, idx, sel, excl, excl, radii, **kw)
    _guard(base)
    broken = xyz.copy()
    broken[1, 3, 0], broken[5, 30, 2], broken[9, 0, 1] = np.nan, np.inf, -np.inf
    broken[2, 10, 1] = np.nan                                      # unselected: not looked at
    got = _run(broken, ref, z, bonds, idx, 31)
    _same(got, R.lddt_counts(broken, ref, idx, sel, excl, excl, radii, **kw), "model")
    assert got["bad"].tolist() == [s in (1, 5, 9) for s in range(12)] and (got["struct_counts"][[1, 5, 9]] == -1).all()
    keep = ~got["bad"]
    assert np.array_equal(got["struct_counts"][keep], base["struct_counts"][keep])
    assert np.array_equal(got["atom_counts"], R.lddt_counts(xyz[keep], ref, np.asarray(idx)[keep], sel, excl, excl, radii, **kw)["atom_counts"])
    _invariant(got)
    bad_ref = ref.copy()
    bad_ref[1, 7, 2] = np.nan                                      # all of reference 1's structures, and only they
    bad_ref[2, 10, 0] = np.nan                                     # unselected
    got = _run(xyz, bad_ref, z, bonds, idx, 31)
    _same(got, R.lddt_counts(xyz, bad_ref, idx, sel, excl, excl, radii, **kw), "reference")
    assert got["bad"].tolist() == [4 <= s < 8 for s in range(12)]
    assert np.array_equal(got["struct_counts"][~got["bad"]], base["struct_counts"][~got["bad"]])
    _invariant(got)


# ----------------------------------------------------------------------------- masks, radii, tolerance
def test_each_mask_removes_exactly_its_pair_from_exactly_its_quantity():
    n, i, j = 31, 5, 20
    xyz, ref, z, _, _ = _cloud(n, (0,) * 6, 1)
    xyz, ref = xyz.copy(), ref.copy()
    ref[0, j] = ref[0, i] + np.array([1.0, 0, 0], F)               # included, kept and clashing in every structure
    xyz[:, j] = xyz[:, i] + np.array([1.0, 0, 0], F)
    alone, paired = np.arange(n), np.arange(n)
    paired[j] = i                                                  # the group mask then names the pair (i, j) alone
    none, bond = np.zeros((0, 2), dtype=int), np.array([[i, j]])   # and so does the clash mask of this one bond
    kw = dict(inclusion_radius=R.cloud_radius(n), device=DEV)
    eye, r = np.eye(n, dtype=bool), np.full(n, 1.7)
    pair = eye.copy()
    pair[i, j] = pair[j, i] = True
    runs = {}
    for name, groups, bonds, ml, mc in (("base", alone, none, eye, eye), ("lddt", paired, none, pair, eye), ("clash", alone, bond, eye, pair)):
        runs[name] = lddt.lddt_counts(xyz, ref, z, bonds, ref_index=np.zeros(6, int), groups=groups, **kw)
        want = R.lddt_counts(xyz, ref, [0] * 6, np.arange(n), ml, mc, r, R0=R.cloud_radius(n))
        _guard(want, name)
        _same(runs[name], want, name)
        _invariant(runs[name])
    d_l = runs["base"]["atom_counts"] - runs["lddt"]["atom_counts"]
    d_c = runs["base"]["atom_counts"] - runs["clash"]["atom_counts"]
    only = np.zeros((n, 6), dtype=np.int64)
    only[[i, j], :5] = 6                                           # six structures, one pair, five quantities
    assert np.array_equal(d_l, only)
    only[:] = 0
    only[[i, j], 5] = 6
    assert np.array_equal(d_c, only)


def test_custom_radii_and_a_tolerance_that_leaves_no_clash():
    n = 31
    xyz, ref, z, bonds, want = _cloud(n, (0,) * 6, 1)
    excl = contacts.excluded_pairs(bonds, n, np.arange(n), 3)
    R0 = R.cloud_radius(n)
    for radii, table in (({6: 2.5}, np.full(n, 2.5)), (np.linspace(0.5, 3.0, n), np.linspace(0.5, 3.0, n))):
        w = R.lddt_counts(xyz, ref, [0] * 6, np.arange(n), excl, excl, table, R0=R0)
        assert w["struct_counts"][:, 5].sum() != want["struct_counts"][:, 5].sum() > 0
        _same(_run(xyz, ref, z, bonds, [0] * 6, n, radii=radii), w, "radii")
    got = _run(xyz, ref, z, bonds, [0] * 6, n, clash_tolerance=3.4)      # c = 3.4 - 3.4 <= 0
    _same(got, R.lddt_counts(xyz, ref, [0] * 6, np.arange(n), excl, excl, np.full(n, 1.7), R0=R0, tol=3.4))
    assert not got["struct_counts"][:, 5].any() and not got["atom_counts"][:, 5].any() and got["struct_counts"][:, 0].all()


def test_a_structure_against_itself_scores_exactly_one():
    xyz, _, z, bonds, _ = _cloud(65, (0, 0, 0), 1)
    got = lddt.lddt_counts(xyz, xyz, z, bonds, device=DEV)
    sc = lddt.scores(got)
    assert (sc["lddt"] == 1.0).all() and (got["struct_counts"][:, 0] > 0).all()
    assert (lddt.profile(got)["lddt"] == 1.0).all()
    _invariant(got)


# ----------------------------------------------------------------------------- limits
def test_one_structure_at_the_largest_selection_and_one_atom_beyond():
    m = lddt.limits()["atoms"]
    rng = np.random.default_rng(m)
    ref = R.chain(m, rng)[None]
    xyz = R.noisy(ref[0], 1, 1.5, rng)
    band = np.zeros((m, m), dtype=bool)                            # a chain's pairs at most 3 bonds apart
    for k in range(-3, 4):
        band |= np.eye(m, k=k, dtype=bool)
    r = np.full(m, 1.7, F)
    got = lddt.count_pairs(xyz, ref, [0], np.arange(m), band, band, r, device=DEV)
    _invariant(got)
    assert not got["bad"].any() and got["struct_counts"][0, 5] > 0 and 0 < got["struct_counts"][0, 1] < got["struct_counts"][0, 0]
    assert got["struct_counts"][0, 0] < np.triu(~band, 1).sum()
    rows = np.unique(np.concatenate([[0, 63, 64, 127, 128, m - 129, m - 65, m - 64, m - 1], rng.integers(0, m, 55)]))
    assert np.array_equal(got["atom_counts"][rows], R.atom_rows(rows, xyz[0], ref[0], np.arange(m), band, band, r))
    with pytest.raises(ValueError, match="the kernel holds"):
        lddt.count_pairs(np.zeros((1, m + 1, 3), F), np.zeros((1, m + 1, 3), F), [0], np.arange(m + 1), np.eye(m + 1, dtype=bool),
                         np.eye(m + 1, dtype=bool), np.ones(m + 1), device=DEV)


# ----------------------------------------------------------------------------- end to end
def _peptide_sets():
    """Twelve jittered frames of one conformer of the three-residue peptide, and for every frame two samples: the frame
    plus 0.05 A of noise, and the frame with the last residue's psi turned by 120 degrees."""
    rng = np.random.default_rng(11)
    z, bonds = DR.peptide(3)
    base = np.array([np.pi, -2.0, 2.3, np.pi, -2.0, 2.3, np.pi, -2.0, 2.3, np.pi])
    tors = base[None] + rng.normal(0.0, 0.05, (12, 10))
    ref = DR.peptide_structures(3, tors)
    turned = tors.copy()
    turned[:, 8] += np.radians(120.0)
    gen = np.stack([(ref + rng.normal(0.0, 0.05, ref.shape)).astype(F), DR.peptide_structures(3, turned)], axis=1)
    return z, bonds, ref, gen


def test_compare_and_the_command_line_on_a_peptide(tmp_path, capsys):
    z, bonds, ref, gen = _peptide_sets()
    n = z.shape[0]
    flat = gen.reshape(24, n, 3)
    stats = lddt.compare(ref, flat, z, bonds, groups="residue", device=DEV)
    assert tuple(stats) == lddt.LDDT_STATS_KEYS and (stats["n_ref"], stats["n_gen"], stats["n_bad_gen"]) == (12, 24, 0)
    labels = lddt.groups_of(z, bonds, None, "residue")
    res = lddt.lddt_counts(flat, ref, z, bonds, groups=labels, device=DEV)
    want = R.lddt_counts(flat, ref, np.arange(24) // 2, np.arange(n), lddt.same_group_pairs(labels),
                         contacts.excluded_pairs(bonds, n, np.arange(n), 3), lddt.radii_of(z, np.arange(n)))
    _same(res, want)
    score = lddt.scores(res)["lddt"]
    assert (score[0::2] > 0.95).all() and (score[1::2] < score[0::2]).all()
    worst = {w["label"]: w["lddt"] for w in stats["worst"]}
    assert 2 in worst and worst[2] < 1.0 and worst[2] < worst[0] and stats["lddt"]["min"] == score.min()     # the third residue
    assert stats["clashes"]["mean_ref"] == 0.0 and not any(stats["clashing_pairs_per_atom"]["ref"])
    assert stats["floor"]["lddt_neighbour"]["mean"] <= 1.0
    json.dumps(stats)
    clashing = flat.copy()
    clashing[:, 0] = (50.0, 0.0, 0.0)                             # the two methyl carbons, many bonds apart, 1 A from each other
    clashing[:, n - 1] = (51.0, 0.0, 0.0)
    hit = lddt.compare(ref, clashing, z, bonds, groups="residue", device=DEV)
    per_atom = np.array(hit["clashing_pairs_per_atom"]["gen"])
    assert per_atom[0] == 1.0 and per_atom[n - 1] == 1.0 and not per_atom[1:n - 1].any()
    assert hit["clashes"]["jsd"] > hit["clashes"]["floor"] and hit["clashes"]["mean_gen"] == 1.0
    np.savez(tmp_path / "ref.npz", xyz=ref, z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=gen)
    out, scores = tmp_path / "lddt_stats.json", tmp_path / "scores.npz"
    capsys.readouterr()
    cli = lddt.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -lddt_groups residue -scores {scores} -out {out} "
                    f"-device {DEV}".split())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["lddt_stats"] == json.loads(json.dumps(lddt.summary_of(cli))) and line["out"] == str(out)
    assert json.loads(json.dumps(cli)) == json.loads(json.dumps(stats))
    with open(out) as f:
        assert tuple(json.load(f)) == lddt.LDDT_STATS_KEYS
    with np.load(scores) as f:
        expect = lddt.scores({**want, "sel": np.arange(n)})
        assert np.array_equal(f["lddt"], expect["lddt"]) and np.array_equal(f["n_clashes"], expect["n_clashes"])
        assert np.array_equal(f["struct_counts"], want["struct_counts"]) and not f["bad"].any()
