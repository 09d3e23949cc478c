"""Contact maps without a GPU: the numpy restatement against plain loops, the exclusion search, the groups, the host
statistics on hand-built counts, the command-line switches and the C ABI's declarations."""
import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, backmap as bm, contacts, ensemble, run_ala
import contacts_restatement as R
import internal_coords_restatement as IR


# ----------------------------------------------------------------------------- the restatement
def test_the_restatement_equals_plain_loops():
    rng = np.random.default_rng(0)
    xyz = rng.uniform(0, 8, (3, 9, 3)).astype(np.float32)
    sel = [8, 1, 5, 0, 3, 2, 7]
    excl = np.eye(7, dtype=bool)
    excl[0, 3] = excl[3, 0] = excl[2, 6] = excl[6, 2] = True
    native = np.zeros((7, 7), dtype=bool)
    native[1, 2] = native[2, 1] = native[0, 6] = native[6, 0] = native[0, 3] = native[3, 0] = True
    xyz[1, 5, 0] = np.nan                                                  # a bad structure
    xyz[0, 4, 2] = np.inf                                                  # atom 4 is not selected
    a, b = R.contact_counts(xyz, sel, 4.5, excl, native), R.contact_counts_loops(xyz, sel, 4.5, excl, native)
    for k in ("counts", "n_contacts", "n_native", "bad"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_good"] == b["n_good"] == 2 and a["bad"].tolist() == [False, True, False]
    assert 0 < a["counts"].sum() < 2 * 21 * 2 and a["counts"][0, 3] == 0 and a["n_native"][0] > 0
    assert np.isnan(a["rg2"][1]) and np.isnan(b["rg2"][1])
    assert np.allclose(a["rg2"][[0, 2]], b["rg2"][[0, 2]], rtol=1e-14, atol=0)
    # the operation order is sq_dist2's: a sum whose other orders round differently
    p, q = np.float32([0.1, 0.2, 0.3]), np.float32([1.3, 2.1, 3.7])
    d = p - q
    assert R.sq_dist2(p, q) == np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    # groups: "any" per structure
    groups = np.array([4, 4, 9, 9, 9, 1, 1])
    g = R.group_contact_counts(xyz, sel, groups, 4.5, excl)
    hit = R.contact_tensor(xyz, sel, 4.5, excl)
    assert g["group_ids"].tolist() == [1, 4, 9]
    for s in range(3):
        for A, ia in enumerate(g["group_ids"]):
            for B, ib in enumerate(g["group_ids"]):
                want = A != B and any(hit[s, i, j] for i in np.flatnonzero(groups == ia) for j in np.flatnonzero(groups == ib))
                assert want == bool(R.group_contact_counts(xyz[s:s + 1], sel, groups, 4.5, excl)["counts"][A, B])
    assert np.array_equal(g["counts"], g["counts"].T) and (np.diag(g["counts"]) == 0).all()


# ----------------------------------------------------------------------------- excluded_pairs
def test_excluded_pairs_on_a_chain_a_ring_and_two_molecules():
    # butane: C0-C1-C2-C3 with hydrogens 4..13; the selection is the carbons
    bonds = [(0, 1), (1, 2), (2, 3)] + [(0, h) for h in (4, 5, 6)] + [(1, h) for h in (7, 8)] + [(2, h) for h in (9, 10)] + \
        [(3, h) for h in (11, 12, 13)]
    sel = [0, 1, 2, 3]
    d3, d2, d0 = (contacts.excluded_pairs(bonds, 14, sel, d) for d in (3, 2, 0))
    assert d3.all()                                                        # the 1-4 pair is excluded at depth 3 ...
    assert not d2[0, 3] and not d2[3, 0] and d2.sum() == 14               # ... and kept at depth 2
    assert np.array_equal(d0, np.eye(4, dtype=bool))
    for e in (d3, d2, d0):
        assert e.dtype == np.bool_ and np.array_equal(e, e.T)
    # a scattered, unordered selection: the answer follows the selection's order; paths run through unselected atoms
    got = contacts.excluded_pairs(bonds, 14, [13, 0, 4], 2)               # H13-C3 ... C0-H4: 13-3-2-1-0-4
    assert got.tolist() == [[True, False, False], [False, True, True], [False, True, True]]
    assert contacts.excluded_pairs(bonds, 14, [13, 0, 4], 5)[0].tolist() == [True, True, True]
    assert contacts.excluded_pairs(bonds, 14, [13, 0, 4], 4)[0].tolist() == [True, True, False]
    # a six-ring: the opposite atom is 3 bonds away both ways
    ring = [(i, (i + 1) % 6) for i in range(6)]
    r2, r3 = contacts.excluded_pairs(ring, 6, range(6), 2), contacts.excluded_pairs(ring, 6, range(6), 3)
    assert r3.all() and (~r2).sum() == 6 and all(not r2[i, (i + 3) % 6] for i in range(6))
    # two molecules: nothing of one is excluded from the other at any depth
    two = contacts.excluded_pairs([(0, 1), (2, 3)], 4, range(4), 10)
    assert two.tolist() == [[True, True, False, False], [True, True, False, False], [False, False, True, True], [False, False, True, True]]
    with pytest.raises(ValueError, match="names atom 4"):
        contacts.excluded_pairs([(0, 1)], 4, [0, 4])
    with pytest.raises(ValueError, match="depth"):
        contacts.excluded_pairs([(0, 1)], 4, [0, 1], -1)


def test_the_bit_masks_are_words_of_32_pairs():
    mask = np.zeros((3, 40), dtype=bool)
    mask[0, 31] = mask[1, 33] = mask[2, 0] = mask[2, 39] = True
    assert ensemble.pack_mask(mask).tolist() == [[1 << 31, 0], [0, 2], [1, 1 << 7]]
    assert ensemble.pack_mask(mask).dtype == np.uint32 and ensemble.pack_mask(np.zeros((2, 64), dtype=bool)).shape == (2, 2)
    assert float(contacts.cutoff2_of(3.0)) == 9.0 and contacts.cutoff2_of(4.5).dtype == np.float32
    assert contacts.cutoff2_of(0.1) == np.float32(np.float32(0.1) * np.float32(0.1))
    with pytest.raises(ValueError):
        contacts.cutoff2_of(float("nan"))


# ----------------------------------------------------------------------------- groups
def test_groups_of_beads_and_residues():
    z, bonds = np.asarray(IR.ALA_Z), np.asarray(IR.ALA_BONDS)
    n = z.shape[0]
    mapping = np.arange(n) % 3
    assert np.array_equal(contacts.groups_of(z, bonds, mapping, "bead"), mapping)
    with pytest.raises(ValueError, match="mapping"):
        contacts.groups_of(z, bonds, None, "bead")
    with pytest.raises(ValueError, match="lists 3 atoms"):
        contacts.groups_of(z, bonds, [0, 1, 2], "bead")
    with pytest.raises(ValueError, match="kind"):
        contacts.groups_of(z, bonds, mapping, "chain")
    res = contacts.groups_of(z, bonds, None, "residue")                    # alanine dipeptide: one residue, the caps join it
    assert res.shape == (n,) and (res == 0).all()
    # Gly-Gly without hydrogens: N0 CA1 C2(=O3) N4 CA5 C6(=O7) N8
    z2 = np.array([7, 6, 6, 8, 7, 6, 6, 8, 7])
    b2 = [(0, 1), (1, 2), (2, 3), (2, 4), (4, 5), (5, 6), (6, 7), (6, 8)]
    assert contacts.groups_of(z2, b2, None, "residue").tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="peptide"):                       # butane is no peptide
        contacts.groups_of(np.full(4, 6), [(0, 1), (1, 2), (2, 3)], None, "residue")
    with pytest.raises(ValueError, match="atom 9 is not connected"):       # an ion next to the peptide
        contacts.groups_of(np.append(z2, 11), b2, None, "residue")


# ----------------------------------------------------------------------------- compare_from_counts
def _result(counts, n_native, rg, bad=None):
    """A ``contact_counts`` result built by hand from an upper-triangle table."""
    c = np.asarray(counts, dtype=np.int64)
    bad = np.zeros(len(rg), dtype=bool) if bad is None else np.asarray(bad, dtype=bool)
    n_nat = np.where(bad, -1, np.asarray(n_native, dtype=np.int64))
    return {"counts": c + c.T, "n_good": int((~bad).sum()), "n_contacts": n_nat.copy(), "n_native": n_nat,
            "rg2": np.where(bad, np.nan, np.asarray(rg, dtype=np.float64) ** 2), "bad": bad}


def _four():
    """Four atoms, the pair (0, 1) excluded.  Reference halves of 4 structures each: (0, 2) always, (1, 3) in half of
    them, (0, 3) never, (2, 3) in a quarter.  The native set at 0.5: (0, 2) and (1, 3)."""
    allowed = ~np.eye(4, dtype=bool)
    allowed[0, 1] = allowed[1, 0] = False
    table = [[0, 0, 4, 0], [0, 0, 0, 2], [0, 0, 0, 1], [0, 0, 0, 0]]
    half = lambda: _result(table, [2, 2, 1, 1], [5.0, 5.0, 6.0, 6.0])
    return allowed, half


def test_identical_sets_have_no_deviation():
    allowed, half = _four()
    even, odd = half(), half()
    native = contacts.native_set(even, odd, allowed, 0.5)
    assert np.argwhere(np.triu(native)).tolist() == [[0, 2], [1, 3]] and np.array_equal(native, native.T)
    gen = _result(2 * np.triu(half()["counts"]), [2, 2, 1, 1] * 2, [5.0, 5.0, 6.0, 6.0] * 2)
    s = contacts.compare_from_counts(even, odd, gen, allowed, native, labels=[10, 11, 12, 13], n_bins=4, params={"cutoff": 4.5})
    assert set(s) == set(contacts.CONTACT_STATS_KEYS)
    assert s["map_rmse"] == 0.0 and s["map_max_dev"] == 0.0 and s["floor"] == {"map_rmse": 0.0, "map_max_dev": 0.0, "q_jsd": 0.0, "rg_jsd": 0.0}
    assert s["n_ref"] == 8 and s["n_gen"] == 8 and s["n_bad_ref"] == 0 and s["n_native"] == 2 and s["labels"] == [10, 11, 12, 13]
    assert s["p_ref"][0][2] == 1.0 and s["p_ref"][1][3] == 0.5 and s["p_ref"][2][3] == 0.25 and s["p_ref"] == s["p_gen"]
    assert s["q"]["jsd"] == 0.0 and s["q"]["mean_ref"] == 0.75 and s["q"]["hist_ref"]["counts"] == [0, 0, 4, 4]
    assert s["q"]["range"] == [0.0, 1.0] and s["params"] == {"cutoff": 4.5, "n_bins": 4}
    # Rg: the reference's [5, 6] widened by 20 %: [4.9, 6.1], nothing outside
    assert s["rg"]["range"] == pytest.approx([4.9, 6.1]) and s["rg"]["hist_ref"] == {"counts": [4, 0, 0, 4], "under": 0, "over": 0}
    assert s["rg"]["mean_ref"] == 5.5 and s["rg"]["std_ref"] == 0.5 and s["rg"]["jsd"] == 0.0
    assert set(contacts.summary_of(s)) == {"n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "map_rmse", "map_max_dev", "floor", "n_native", "q", "rg"}
    assert set(contacts.summary_of(s)["q"]) == {"jsd", "mean_ref", "std_ref", "mean_gen", "std_gen"}


def test_one_flipped_pair_is_found():
    allowed, half = _four()
    even, odd = half(), half()
    native = contacts.native_set(even, odd, allowed, 0.5)
    table = [[0, 0, 8, 8], [0, 0, 0, 4], [0, 0, 0, 2], [0, 0, 0, 0]]       # (0, 3) never in the reference, always here
    gen = _result(table, [2, 2, 1, 1] * 2, [5.0, 5.0, 6.0, 7.0] * 2)
    s = contacts.compare_from_counts(even, odd, gen, allowed, native, n_bins=4)
    assert s["map_max_dev"] == 1.0 and s["map_rmse"] == pytest.approx(np.sqrt(1.0 / 5.0))    # 5 pairs count, one off by 1
    assert s["top_pairs"][0] == {"i": 0, "j": 3, "p_ref": 0.0, "p_gen": 1.0} and len(s["top_pairs"]) == 5
    assert s["floor"]["map_rmse"] == 0.0 and s["q"]["jsd"] == 0.0
    # Rg 7 is above the reference's range: counted as over and left out of the distribution
    assert s["rg"]["hist_gen"] == {"counts": [4, 0, 0, 2], "under": 0, "over": 2} and s["rg"]["jsd"] > 0
    # an excluded pair never shows, whatever its counts
    table[0][1] = 8
    s2 = contacts.compare_from_counts(even, odd, _result(table, [2] * 8, [5.0] * 8), allowed, native, n_bins=4)
    assert s2["map_max_dev"] == 1.0 and all((t["i"], t["j"]) != (0, 1) for t in s2["top_pairs"])
    # the halves differ: the floor says so
    odd2 = _result([[0, 0, 4, 0], [0, 0, 0, 4], [0, 0, 0, 1], [0, 0, 0, 0]], [2, 2, 2, 2], [5.0, 5.0, 6.0, 6.0])
    f = contacts.compare_from_counts(even, odd2, gen, allowed, native, n_bins=4)["floor"]
    assert f["map_max_dev"] == 0.5 and f["map_rmse"] == pytest.approx(np.sqrt(0.25 / 5.0)) and f["q_jsd"] > 0


def test_an_empty_native_set_or_an_empty_set_gives_none():
    allowed, half = _four()
    even, odd = half(), half()
    native = contacts.native_set(even, odd, allowed, 1.5)                  # no pair reaches it
    assert not native.any()
    gen = _result(np.triu(half()["counts"]), [0] * 4, [5.0, 5.0, 6.0, 6.0])
    s = contacts.compare_from_counts(even, odd, gen, allowed, native)
    assert s["n_native"] == 0 and s["q"] is None and s["floor"]["q_jsd"] is None and s["rg"] is not None and s["map_rmse"] == 0.0
    assert contacts.summary_of(s)["q"] is None
    nothing = _result(np.zeros((4, 4), dtype=np.int64), [], [])
    e = contacts.compare_from_counts(even, odd, nothing, allowed, contacts.native_set(even, odd, allowed, 0.5))
    assert e["n_gen"] == 0 and e["p_gen"] is None and e["map_rmse"] is None and e["top_pairs"] == [] and e["q"] is None and e["rg"] is None
    assert e["floor"]["map_rmse"] == 0.0 and e["p_ref"] is not None
    assert not contacts.native_set(nothing, nothing, allowed, 0.5).any()


def test_bad_structures_are_in_no_denominator():
    allowed, half = _four()
    even, odd = half(), half()
    native = contacts.native_set(even, odd, allowed, 0.5)
    # 6 generated structures, two of them bad: the counts of the 4 good ones are the reference half's
    gen = _result(np.triu(half()["counts"]), [2, 0, 2, 1, 0, 1], [5.0, 0.0, 5.0, 6.0, 0.0, 6.0], bad=[0, 1, 0, 0, 1, 0])
    s = contacts.compare_from_counts(even, odd, gen, allowed, native, n_bins=4)
    assert s["n_gen"] == 6 and s["n_bad_gen"] == 2 and s["map_rmse"] == 0.0 and s["p_gen"][0][2] == 1.0
    assert s["q"]["mean_gen"] == 0.75 and sum(s["q"]["hist_gen"]["counts"]) == 4 and s["rg"]["mean_gen"] == 5.5
    assert sum(s["rg"]["hist_gen"]["counts"]) == 4 and s["rg"]["hist_gen"]["under"] == 0
    bad_ref = _result(np.triu(half()["counts"]), [2, 2, 1, 1, 0], [5.0, 5.0, 6.0, 6.0, 0.0], bad=[0, 0, 0, 0, 1])
    s = contacts.compare_from_counts(bad_ref, odd, gen, allowed, native, n_bins=4)
    assert s["n_ref"] == 9 and s["n_bad_ref"] == 1 and s["p_ref"][1][3] == 0.5 and s["map_rmse"] == 0.0


def test_host_wrappers_refuse_bad_arguments_without_a_launch():
    x = np.zeros((4, 6, 3), np.float32)
    with pytest.raises(ValueError, match="names atom 6"):
        contacts.contact_counts(x, [0, 6])
    with pytest.raises(ValueError, match="m = 0"):
        contacts.contact_counts(x, [])
    with pytest.raises(ValueError, match="twice"):
        contacts.contact_counts(x, [1, 1])
    with pytest.raises(ValueError, match=r"\[S, n, 3\]"):
        contacts.contact_counts(x[0])
    with pytest.raises(ValueError, match="excluded must be a bool array"):
        contacts.contact_counts(x, [0, 1], excluded=np.zeros((3, 3), dtype=bool))
    with pytest.raises(ValueError, match="symmetric"):
        contacts.contact_counts(x, [0, 1], native=np.array([[False, True], [False, False]]))
    with pytest.raises(ValueError, match="groups lists"):
        contacts.contact_counts(x, [0, 1], groups=[0, 1, 2])
    with pytest.raises(ValueError, match="cutoff"):
        contacts.contact_counts(x, cutoff=-1.0)
    with pytest.raises(ValueError, match="two reference frames"):
        contacts.compare(x[:1], x, np.full(6, 6), [(0, 1)])
    with pytest.raises(ValueError, match="groups must be"):
        contacts.compare(x, x, np.full(6, 6), [(0, 1)], groups="chain")


# ----------------------------------------------------------------------------- command line
def test_both_parsers_accept_the_switches_and_are_unchanged_without_them():
    p = bm.build_parser()
    off = p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz".split())
    assert not any(k.startswith("contact") for k in vars(off))              # what it parsed to before the switches existed
    assert bm.contact_args(off) == {"contact_stats": False, "contact_cutoff": 4.5, "contact_atoms": "heavy", "contact_exclude": 3,
                                    "contact_groups": "none"}
    on = p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz --contact_stats -contact_cutoff 6 -contact_atoms all "
                      "-contact_exclude 2 -contact_groups residue".split())
    assert bm.contact_args(on) == {"contact_stats": True, "contact_cutoff": 6.0, "contact_atoms": "all", "contact_exclude": 2,
                                   "contact_groups": "residue"}
    assert bm.contact_args(p.parse_args("-model D -cg c.npz -n_samples 4 -out o.npz --contact_stats".split()))["contact_cutoff"] == 4.5
    for bad in ("-contact_atoms backbone", "-contact_groups chain"):
        with pytest.raises(SystemExit):
            p.parse_args(f"-model D -cg c.npz -n_samples 4 -out o.npz --contact_stats {bad}".split())
    assert "contact_eval" not in vars(run_ala.build_extras_parser().parse_args([]))
    assert vars(run_ala.build_extras_parser().parse_args(["--contact_eval"]))["contact_eval"] is True
    assert not any("contact" in k for k in vars(run_ala.build_parser().parse_args("-logdir x".split())))
    got, rest = run_ala.build_extras_parser().parse_known_args("-logdir x --contact_eval -n_cgs 3".split())
    assert got.contact_eval and rest == ["-logdir", "x", "-n_cgs", "3"]


def test_an_off_switch_adds_no_key_to_modelparams():
    params = vars(run_ala.build_parser().parse_args("-logdir x".split()))
    base = dict(params)
    params.update(vars(run_ala.build_extras_parser().parse_args([])))
    assert run_ala.stored_params(params) == base
    assert run_ala.stored_params({**params, "contact_eval": False}) == base           # a caller that names it as off
    params.update(vars(run_ala.build_extras_parser().parse_args(["--contact_eval"])))
    assert run_ala.stored_params(params) == {**base, "contact_eval": True}


def test_contact_stats_inputs_are_checked(tmp_path):
    import json
    d = tmp_path / "run"
    d.mkdir()
    (d / "modelparams.json").write_text(json.dumps({"n_cgs": 2, "det": False, "mapping": [0] * 3 + [1] * 3}))
    params, p = bm.read_params(str(d)), bm.build_parser()
    cg, top, ref, hyd = tmp_path / "cg.npz", tmp_path / "top.npz", tmp_path / "ref.npz", tmp_path / "hyd.npz"
    z, bonds = np.array([6, 1, 7, 6, 1, 8]), np.stack([np.arange(5), np.arange(1, 6)], 1)
    np.savez(cg, cg_xyz=np.zeros((3, 2, 3), np.float32))
    np.savez(top, z=z, bonds=bonds)
    np.savez(ref, xyz=np.zeros((4, 6, 3), np.float32), z=z)
    np.savez(hyd, z=np.array([1, 1, 1, 1, 1, 6]), bonds=bonds)
    base = f"-model {d} -cg {cg} -n_samples 2 -out o"
    inp = bm.read_inputs(p.parse_args(f"{base} -top {top} --contact_stats -ref {ref}".split()), params)
    assert inp["ref_xyz"].shape == (4, 6, 3) and "ref_starts" not in inp
    with pytest.raises(SystemExit, match="--contact_stats needs a topology"):
        bm.read_inputs(p.parse_args(f"{base} --contact_stats -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="reference frames"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --contact_stats".split()), params)
    with pytest.raises(SystemExit, match="positive distance"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --contact_stats -contact_cutoff 0 -ref {ref}".split()), params)
    with pytest.raises(SystemExit, match="no N - CA - C' backbone"):
        bm.read_inputs(p.parse_args(f"{base} -top {top} --contact_stats -contact_groups residue -ref {ref}".split()), params)
    np.savez(ref, xyz=np.zeros((4, 6, 3), np.float32), z=np.array([1, 1, 1, 1, 1, 6]))
    with pytest.raises(SystemExit, match="fewer than two heavy atoms"):
        bm.read_inputs(p.parse_args(f"{base} -top {hyd} --contact_stats -ref {ref}".split()), params)


# ----------------------------------------------------------------------------- C ABI
def test_the_header_declares_the_entry_points_and_the_build_keeps_products_apart():
    from coarsegrainingvae_amd import build
    names = ("cgv_contact_counts", "cgv_contact_group_counts", "cgv_contact_workspace_bytes", "cgv_contact_max_atoms",
             "cgv_contact_max_structures")
    declared = _lib.header_symbols()
    assert all(n in declared and n in _lib.PROTOTYPES for n in names)
    assert build.SOURCE_FLAGS["contact_map.hip"] == ["-ffp-contract=off"]
    assert len(_lib.PROTOTYPES["cgv_contact_counts"][1]) == 16 and len(_lib.PROTOTYPES["cgv_contact_group_counts"][1]) == 18


def test_the_limits_are_refused_before_any_launch():
    import ctypes as C
    lib, lim = _lib.load(), contacts.limits()
    assert lim == {"structures": 1 << 20, "atoms": 1 << 14}
    assert lib.cgv_contact_workspace_bytes(10, 7) == 10 * 7 * 16 and lib.cgv_contact_workspace_bytes(lim["structures"] + 1, 7) == 0
    assert lib.cgv_contact_workspace_bytes(10, lim["atoms"] + 1) == 0

    def atoms(S, n, m, cutoff2=1.0):
        return lib.cgv_contact_counts(None, None, None, None, S, n, m, C.c_float(cutoff2), None, None, None, None, None, None, 0, None)

    def groups(S, n, m, G):
        return lib.cgv_contact_group_counts(None, None, None, None, None, S, n, m, G, C.c_float(1.0), None, None, None, None, None,
                                            None, 0, None)
    assert atoms(-1, 5, 2) == -1 and atoms(lim["structures"] + 1, 5, 2) == -1
    assert atoms(4, 5, 0) == -1 and atoms(4, 5, 6) == -1 and atoms(4, 1 << 15, lim["atoms"] + 1) == -1
    assert atoms(4, 5, 2, float("nan")) == -1 and atoms(4, 5, 2, -1.0) == -1
    assert atoms(4, 5, 2) == -1 and b"null" in lib.cgv_last_error_string()
    assert atoms(0, 5, 2) == 0                                             # no structures: nothing to do
    assert groups(4, 5, 2, 0) == -1 and groups(4, 5, 2, 3) == -1 and groups(4, 8192, 5000, 4097) == -1
    assert groups(4, 5, 2, 2) == -1 and b"null" in lib.cgv_last_error_string() and groups(0, 5, 2, 2) == 0
