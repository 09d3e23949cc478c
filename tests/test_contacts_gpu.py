"""Contact maps on the device: K20 (csrc/contact_map.hip) against the numpy restatement.  A contact is a threshold on an
fp32 sum that both sides round identically, so every integer is compared EXACTLY; rg2 within a derived bound; chunking,
repeat runs, bad structures, group maps, ``compare`` on a constructed case and the backmap command line."""
import functools
import json

import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd import backmap as bm, contacts, run_ala
import contacts_restatement as R
import internal_coords_restatement as IR

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTS = ("counts", "n_contacts", "n_native", "bad")


def _tree(n, rng):
    """Bonds of a random tree over n atoms."""
    return np.array([(i, int(rng.integers(0, i))) for i in range(1, n)], dtype=np.int64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _case(m, S, depth):
    """Coordinates uniform in an 8 A box, n = m + 7 atoms, the selection m of them scattered and in no order, the
    exclusions of a random tree at `depth`, a random symmetric native set, and the restatement's result."""
    rng = np.random.default_rng(10000 * m + 10 * S + depth)
    n = m + 7
    xyz = rng.uniform(0, 8, (S, n, 3)).astype(np.float32)
    sel = rng.permutation(n)[:m]
    excl = contacts.excluded_pairs(_tree(n, rng), n, sel, depth)
    native = np.triu(rng.random((m, m)) < 0.3, 1)
    native = native | native.T
    want = R.contact_counts(xyz, sel, 4.5, excl, native)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return xyz, sel, excl, native, want


def _same_integers(got, want, what=""):
    assert got["n_good"] == want["n_good"], what
    for k in INTS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _rg2_within_bound(got, want, m, what=""):
    """|rg2 - restatement| <= 4 m 2^-52 rg2.  Both sides are fp64 on exactly widened fp32 coordinates.  Per atom the
    two-pass formula rounds x - c once per component (entering squared: 2), the square (1) and the two additions of the
    three components (2); the sum over m atoms adds at most m - 1 roundings on any path and the division by m one: at
    most m + 5 roundings, a relative error of (m + 5) 2^-53 per side whatever the order of the sum, (m + 5) 2^-52 for
    the difference of two sides, which is <= 4 m 2^-52 from m = 2 on.  The rounding of the centroid itself moves rg2 by
    |delta c|^2, second order.  m = 1 gives exactly 0 on both sides.  (Measured on an MI355X over this file's cases: the
    worst ratio to 2^-52 rg2 was 4.8, at m = 130.)"""
    good = ~want["bad"]
    assert np.isnan(got["rg2"][~good]).all() and np.isfinite(got["rg2"][good]).all()
    err, unit = np.abs(got["rg2"][good] - want["rg2"][good]), 2.0 ** -52 * want["rg2"][good]
    ratio = float((err[unit > 0] / unit[unit > 0]).max(initial=0.0))
    print(what, "max |delta rg2| / (2^-52 rg2) =", ratio, "bound", 4 * m)
    assert (err <= 4 * m * unit).all(), (what, ratio)


# ----------------------------------------------------------------------------- the main sweep
@pytest.mark.parametrize("depth", [0, 3])
@pytest.mark.parametrize("S", [1, 3, 257])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130])
def test_counts_equal_the_restatement_exactly(m, S, depth):
    xyz, sel, excl, native, want = _case(m, S, depth)
    got = contacts.contact_counts(xyz, sel, 4.5, excl, native, device=DEV)
    _same_integers(got, want, f"m {m} S {S} depth {depth}")
    assert got["counts"].dtype == np.int64 and got["counts"].shape == (m, m)
    assert np.array_equal(got["counts"], got["counts"].T) and (np.diag(got["counts"]) == 0).all()
    assert (got["counts"][excl] == 0).all()
    if m == 1:
        assert got["counts"].sum() == 0 and (got["n_contacts"] == 0).all()
    _rg2_within_bound(got, want, m, f"m {m} S {S}")
    none = contacts.contact_counts(xyz, sel, 4.5, excl, device=DEV)            # no native set: the same, and n_native = 0
    assert np.array_equal(none["counts"], want["counts"]) and (none["n_native"] == 0).all()


def test_a_pair_on_the_threshold_is_not_in_contact_and_one_ulp_above_it_is():
    xyz = np.array([[[0, 0, 0], [3, 0, 0]]], dtype=np.float32)
    at = contacts.contact_counts(xyz, cutoff=3.0, device=DEV)
    assert at["counts"].tolist() == [[0, 0], [0, 0]] and at["n_contacts"].tolist() == [0]
    above = contacts.contact_counts(xyz, cutoff=float(np.nextafter(np.float32(3.0), np.float32(np.inf))), device=DEV)
    assert above["counts"].tolist() == [[0, 1], [1, 0]] and above["n_contacts"].tolist() == [1]
    for cutoff in (3.0, float(np.nextafter(np.float32(3.0), np.float32(np.inf)))):
        assert np.array_equal(R.contact_counts(xyz, [0, 1], cutoff)["counts"],
                              contacts.contact_counts(xyz, cutoff=cutoff, device=DEV)["counts"])


def test_chunked_launches_give_the_arrays_of_one_launch():
    xyz, sel, excl, native, want = _case(65, 3, 3)
    xyz7 = np.concatenate([xyz, xyz[::-1] + np.float32(0.25), xyz[:1] * np.float32(0.5)])
    one = contacts.contact_counts(xyz7, sel, 4.5, excl, native, device=DEV)
    two = contacts.contact_counts(xyz7, sel, 4.5, excl, native, structures_per_launch=2, device=DEV)
    _same_integers(two, one)
    assert one["rg2"].tobytes() == two["rg2"].tobytes()
    _same_integers(one, R.contact_counts(xyz7, sel, 4.5, excl, native))


def test_two_runs_give_identical_bits():
    xyz, sel, excl, native, _ = _case(130, 257, 3)
    a = contacts.contact_counts(xyz, sel, 4.5, excl, native, device=DEV)
    b = contacts.contact_counts(xyz, sel, 4.5, excl, native, device=DEV)
    assert a["rg2"].tobytes() == b["rg2"].tobytes()
    _same_integers(a, b)


def test_nan_and_inf_structures_are_flagged_and_counted_nowhere():
    xyz, sel, excl, native, _ = _case(65, 3, 0)
    x = np.concatenate([xyz, xyz[:2] + np.float32(0.5)]).copy()            # 5 structures
    outside = [a for a in range(x.shape[1]) if a not in sel][0]
    x[0, outside, 1] = np.nan                                              # outside the selection: of no consequence
    x[1, sel[64], 2] = np.nan
    x[3, sel[0], 0] = np.inf
    got = contacts.contact_counts(x, sel, 4.5, excl, native, device=DEV)
    assert got["bad"].tolist() == [False, True, False, True, False] and got["n_good"] == 3
    assert got["n_contacts"][[1, 3]].tolist() == [-1, -1] and got["n_native"][[1, 3]].tolist() == [-1, -1]
    assert np.isnan(got["rg2"][[1, 3]]).all()
    clean = contacts.contact_counts(x[[0, 2, 4]], sel, 4.5, excl, native, device=DEV)
    assert np.array_equal(got["counts"], clean["counts"])
    assert np.array_equal(got["n_contacts"][[0, 2, 4]], clean["n_contacts"])
    want = R.contact_counts(x, sel, 4.5, excl, native)
    _same_integers(got, want)
    _rg2_within_bound(got, want, 65)


# ----------------------------------------------------------------------------- group maps
@pytest.mark.parametrize("S", [3, 130])
def test_group_maps_equal_the_restatement_exactly(S):
    """Groups of 1, 5, 64 and 70 atoms with scattered members and labels that are no 0..G-1; every pair of atoms between
    the groups of 5 and of 64 is excluded, so that pair of groups can never be in contact.  A 16 A box and a 2 A cutoff
    put the pairs of groups between "rarely" and "always"."""
    rng = np.random.default_rng(S)
    sizes, ids = [1, 5, 64, 70], [7, 2, 40, 11]
    m, n = sum(sizes), sum(sizes) + 5
    xyz = rng.uniform(0, 16, (S, n, 3)).astype(np.float32)
    sel = rng.permutation(n)[:m]
    groups = rng.permutation(np.repeat(ids, sizes))
    excl = contacts.excluded_pairs(_tree(n, rng), n, sel, 1)
    between = (groups[:, None] == 2) & (groups[None, :] == 40)
    excl = excl | between | between.T
    native = np.zeros((4, 4), dtype=bool)                                  # in ascending label order: 2, 7, 11, 40
    native[0, 2] = native[2, 0] = native[2, 3] = native[3, 2] = native[0, 3] = native[3, 0] = True
    want = R.group_contact_counts(xyz, sel, groups, 2.0, excl, native)
    got = contacts.contact_counts(xyz, sel, 2.0, excl, native, groups=groups, device=DEV)
    assert got["group_ids"].tolist() == [2, 7, 11, 40] and got["counts"].shape == (4, 4)
    _same_integers(got, want, f"S {S}")
    assert got["counts"][0, 3] == 0 and got["counts"][3, 0] == 0           # the excluded pair of groups
    assert 0 < got["counts"][0, 1] < S or S == 3                           # "any" is not trivially true or false
    assert got["counts"][2, 3] == S
    _rg2_within_bound(got, want, m)
    atoms = contacts.contact_counts(xyz, sel, 2.0, excl, device=DEV)       # not derivable from the atom counts
    assert atoms["counts"][np.ix_(groups == 11, groups == 40)].sum() > got["counts"][2, 3]
    chunked = contacts.contact_counts(xyz, sel, 2.0, excl, native, groups=groups, structures_per_launch=2, device=DEV)
    _same_integers(chunked, got)


# ----------------------------------------------------------------------------- compare
def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def test_compare_on_two_rigid_conformers():
    """A 12-atom chain.  Open: a straight line, 3 A between neighbours.  Closed: a regular 12-gon of side 4 A, so the
    two ends are neighbours on the ring, 4 A apart; every other pair more than 3 bonds apart is at least 7.7 A apart.
    Only the pair (0, 11) is ever in contact at 4.5 A.  The reference is closed, closed, open, open, ... (its even and
    its odd frames are both 50:50), the generated set is open only; every frame is rotated and moved."""
    rng = np.random.default_rng(3)
    radius = 2.0 / np.sin(np.pi / 12)
    ang = 2 * np.pi * np.arange(12) / 12
    closed = np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(12)], 1)
    opened = np.stack([3.0 * np.arange(12), np.zeros(12), np.zeros(12)], 1)

    def draw(which):
        return np.array([(closed if w else opened) @ _rotation(rng).T + rng.uniform(-5, 5, 3) for w in which], np.float32)
    ref, gen = draw([1, 1, 0, 0] * 6), draw([0] * 10)
    z, bonds = np.full(12, 6), np.stack([np.arange(11), np.arange(1, 12)], 1)
    stats = contacts.compare(ref, gen, z, bonds, device=DEV)
    assert set(stats) == set(contacts.CONTACT_STATS_KEYS) and json.loads(json.dumps(stats)) == stats
    assert stats["n_ref"] == 24 and stats["n_gen"] == 10 and stats["n_bad_ref"] == stats["n_bad_gen"] == 0
    assert stats["labels"] == list(range(12)) and stats["params"]["atoms"] == list(range(12))
    assert stats["p_ref"][0][11] == 0.5 and stats["p_ref"][11][0] == 0.5 and stats["p_gen"][0][11] == 0.0
    assert np.count_nonzero(stats["p_ref"]) == 2 and np.count_nonzero(stats["p_gen"]) == 0
    top = stats["top_pairs"][0]
    assert (top["i"], top["j"], top["p_ref"], top["p_gen"]) == (0, 11, 0.5, 0.0)
    assert stats["map_max_dev"] == 0.5 and stats["floor"]["map_rmse"] == 0.0 and stats["floor"]["map_max_dev"] == 0.0
    assert stats["n_native"] == 1
    assert stats["q"]["mean_ref"] == 0.5 and stats["q"]["mean_gen"] == 0.0 and stats["q"]["floor"] == 0.0
    assert stats["q"]["jsd"] > 0.1
    # the line is the more extended: Rg 10.36 A against the ring's 7.73 A
    assert abs(stats["rg"]["mean_gen"] - 3.0 * np.sqrt(143.0 / 12.0)) < 1e-3
    assert abs(stats["rg"]["mean_ref"] - 0.5 * (3.0 * np.sqrt(143.0 / 12.0) + radius)) < 1e-3
    assert stats["rg"]["mean_gen"] > stats["rg"]["mean_ref"] and stats["rg"]["std_gen"] < 1e-3 < stats["rg"]["std_ref"]
    assert stats["rg"]["floor"] == 0.0 and sum(stats["rg"]["hist_gen"]["counts"]) == 10


# ----------------------------------------------------------------------------- CLI
def test_run_ala_contact_eval_writes_the_file_and_returns_the_short_form(tmp_path, capsys):
    """``run_ala.contact_eval`` on hand-made hold-out frames and samples (the tuple of ``evaluate.sample_ensemble``
    starts with the samples ``[T, K, n, 3]`` and the frames ``[T, n, 3]``): no training is needed to check its wiring."""
    rng = np.random.default_rng(2)
    z, bonds = np.asarray(IR.ALA_Z), np.asarray(IR.ALA_BONDS)
    n = z.shape[0]
    frames = rng.uniform(0, 6, (4, n, 3)).astype(np.float32)
    samples = (frames[:, None] + rng.normal(0, 0.3, (4, 3, n, 3))).astype(np.float32)
    frame = {"nxyz": torch.cat([torch.as_tensor(z, dtype=torch.float32)[:, None], torch.from_numpy(frames[0])], 1),
             "bond_edge_list": torch.as_tensor(bonds)}
    short = run_ala.contact_eval([frame] * 4, [0, 1, 2, 3], (samples, frames), DEV, str(tmp_path))
    full = json.loads((tmp_path / "contact_stats.json").read_text())
    assert set(full) == set(contacts.CONTACT_STATS_KEYS) and short == contacts.summary_of(full)
    assert full["n_ref"] == 4 and full["n_gen"] == 12 and full["labels"] == np.flatnonzero(z != 1).tolist()
    assert run_ala.contact_eval([frame] * 4, [0], (samples, frames), DEV, str(tmp_path)) is None      # one frame: nothing to compare
    assert "skipped" in capsys.readouterr().err


def test_backmap_cli_writes_contact_stats_and_nothing_without_the_switch(tmp_path, capsys):
    """A fresh dipeptide-shaped run directory (the fixture pattern of test_coverage_gpu.py) and a random reference of 9
    frames: the file has the documented keys; without the switch no file is written and the outputs are what they were."""
    w = cg.data.WORKLOADS["dipeptide"]
    ds = cg.CGDataset(cg.data.synthetic_frames(3, w["n_atoms"], w["n_cgs"], w["box"], seed=11))
    model = cg.build_model(64, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], w["enc_nconv"], w["dec_nconv"], w["n_cgs"], seed=123)
    d = tmp_path / "run"
    d.mkdir()
    params = {"n_basis": 64, "n_rbf": w["n_rbf"], "atom_cutoff": w["atom_cutoff"], "cg_cutoff": w["cg_cutoff"],
              "enc_nconv": w["enc_nconv"], "dec_nconv": w["dec_nconv"], "n_cgs": w["n_cgs"], "activation": "swish", "det": False,
              "invariantdec": False, "cg_mp": False, "cg_radius_graph": False, "synthetic": True,
              "mapping": ds.props["CG_mapping"][0].tolist()}
    (d / "modelparams.json").write_text(json.dumps(params))
    torch.save(model.state_dict(), d / "model.pt")
    n = len(IR.ALA_Z)
    ref = np.random.default_rng(0).uniform(0, 6, (9, n, 3)).astype(np.float32)
    np.savez(tmp_path / "cg.npz", cg_xyz=torch.stack(ds.props["CG_nxyz"])[:, :, 1:].numpy())
    np.savez(tmp_path / "top.npz", z=IR.ALA_Z, bonds=IR.ALA_BONDS)
    np.savez(tmp_path / "ref.npz", xyz=ref, z=IR.ALA_Z, bonds=IR.ALA_BONDS)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir(), (tmp_path / "c").mkdir()
    base = f"-model {d} -cg {tmp_path / 'cg.npz'} -top {tmp_path / 'top.npz'} -n_samples 4"
    bm.main(f"{base} -out {tmp_path / 'a' / 'out.npz'} --contact_stats -contact_cutoff 5.0 -ref {tmp_path / 'ref.npz'}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(line["contact_stats"]) == set(contacts.summary_of({k: None for k in contacts.CONTACT_STATS_KEYS}))
    stats = json.loads((tmp_path / "a" / "contact_stats.json").read_text())
    assert set(stats) == set(contacts.CONTACT_STATS_KEYS) and line["contact_stats"] == contacts.summary_of(stats)
    heavy = np.flatnonzero(np.asarray(IR.ALA_Z) != 1).tolist()
    assert stats["n_ref"] == 9 and stats["n_gen"] == 12 and stats["labels"] == heavy
    assert stats["params"] == {"atoms": heavy, "cutoff": 5.0, "exclude": 3, "groups": None, "native_min": 0.5, "n_bins": 20}
    assert np.asarray(stats["p_ref"]).shape == (len(heavy), len(heavy)) and stats["map_rmse"] is not None
    # groups of beads, all atoms
    bm.main(f"{base} -out {tmp_path / 'c' / 'out.npz'} --contact_stats -contact_groups bead -contact_atoms all -contact_exclude 1 "
            f"-ref {tmp_path / 'ref.npz'}".split())
    capsys.readouterr()
    beads = json.loads((tmp_path / "c" / "contact_stats.json").read_text())
    assert beads["labels"] == sorted(set(params["mapping"])) and beads["params"]["groups"] == "bead"
    assert beads["params"]["atoms"] == list(range(n)) and beads["params"]["exclude"] == 1
    bm.main(f"{base} -out {tmp_path / 'b' / 'out.npz'}".split())
    line_b = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "contact_stats" not in line_b and set(line_b) == set(line) - {"contact_stats"}
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["out.npz"]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["contact_stats.json", "out.npz"]
    with np.load(tmp_path / "a" / "out.npz") as fa, np.load(tmp_path / "b" / "out.npz") as fb:
        assert set(fa.files) == set(fb.files) and fa["xyz"].tobytes() == fb["xyz"].tobytes()
