"""Host side of the test-time evaluation (coarsegrainingvae_amd/evaluate.py): thresholds, radii, the assembly of the
reference's tuples from the metric kernel's raw outputs, the goldens' provenance.  CPU only."""
import glob
import importlib.util
import itertools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from coarsegrainingvae_amd import _lib, evaluate as ev, run_ala
from coarsegrainingvae_amd.graph import cutoff_threshold_sq

CASES = ["valid", "mixed_all", "mixed_heavy", "all_none", "both_none", "no_hydrogen", "no_bond", "ulp"]


def _golden(case):
    return load_golden("g12_sample_quality_" + case)


def raw_counts_from_golden(g):
    """The kernel's [K,6] counts and [K,2] sums as the golden pins them (integers from the reference's bond matrices,
    sums restated in float64 exactly as compute_rmsd forms them, sampling.py:228-232)."""
    counts = np.stack([g["diff.all"], g["diff.heavy"], g["signed.all"], g["signed.heavy"], g["refsum.all"], g["refsum.heavy"]], axis=1)
    d = g["gen"].astype(np.float64) - g["ref"].astype(np.float64)[None]
    per_atom = np.power(d, 2).sum(-1)
    heavy = g["z"] != 1
    return counts, np.stack([per_atom.sum(-1), per_atom[:, heavy].sum(-1)], axis=1)


def check_six(got, g, rel=1e-10):
    for name, val in zip(("all_rmsds", "heavy_rmsds"), got[:2]):
        if bool(g[f"six.{name}.none"]):
            assert val is None, name
        else:
            assert val is not None and val.shape == g[f"six.{name}"].shape, name
            np.testing.assert_allclose(val, g[f"six.{name}"], rtol=rel, atol=0)
    assert got[2] == float(g["six.valid_ratio"]) and got[3] == float(g["six.valid_allatom_ratio"])
    for val, name in ((got[4], "six.graph_val_ratio"), (got[5], "six.graph_allatom_val_ratio")):
        assert isinstance(val, list) and len(val) == len(g[name])
        np.testing.assert_allclose(np.array(val), g[name], rtol=rel, atol=0, equal_nan=True)


# ----------------------------------------------------------------------------- C ABI surface
def test_sample_quality_symbol_is_declared_prototyped_and_exported():
    assert "cgv_sample_quality" in _lib.header_symbols() and "cgv_sample_quality" in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.cgv_sample_quality_max_classes() >= 8
    assert set(_lib.header_symbols()) == set(_lib.PROTOTYPES)


# ----------------------------------------------------------------------------- thresholds and radii
def test_strict_threshold_against_brute_force_sqrt_for_every_default_class_pair():
    elements = sorted(ev.COVALENT_RADII)
    table = ev.bond_thresholds(elements, 1.3)
    assert table.shape == (len(elements), len(elements)) and torch.equal(table, table.t())
    vdw = torch.Tensor([ev.COVALENT_RADII[e] for e in elements])
    cutoff = (vdw[None, :] + vdw[:, None]) * 1.3                     # compute_bond_cutoff, sampling.py:120-126
    for a, b in itertools.combinations_with_replacement(range(len(elements)), 2):
        c = cutoff[a, b]
        s = np.float32(table[a, b].item())
        bits = int(np.array(s, dtype=np.float32).view(np.uint32))
        window = np.arange(bits - 300, bits + 301, dtype=np.uint32).view(np.float32).copy()
        bonded = (torch.sqrt(torch.from_numpy(window)) < c).numpy()
        assert bonded[:301].all() and not bonded[301:].any(), (elements[a], elements[b])
        # the non-strict sibling keeps today's meaning and is never below the strict one
        assert cutoff_threshold_sq(float(c)) >= float(s)
        assert cutoff_threshold_sq(float(c)) == cutoff_threshold_sq(float(c), strict=False)


def test_strict_threshold_differs_from_the_closed_one_where_a_root_hits_the_cutoff():
    assert cutoff_threshold_sq(5.0) >= 25.0                            # sqrt(25) <= 5 (and so do the few s above that round to 5)
    assert cutoff_threshold_sq(5.0, strict=True) < 25.0                # sqrt(25) < 5 is false
    with pytest.raises(ValueError):
        cutoff_threshold_sq(0.0, strict=True)


@pytest.mark.parametrize("case", CASES)
def test_default_radii_equal_the_ones_the_reference_used(case):
    g = _golden(case)
    assert ev.bond_radii(g["radii.z"]).tolist() == g["radii.r"].tolist()


def test_recorded_thresholds_are_strict_thresholds_of_the_recorded_radii():
    """The thresholds stored with the goldens bracket ``(r_a + r_b) * scale`` the way a correctly rounded or a 1-ulp-off
    host sqrt can: within one ulp of this host's table (equal on a host whose sqrt agrees with the recording one)."""
    for case in CASES:
        g = _golden(case)
        here = ev.bond_thresholds(g["radii.z"].tolist(), float(g["scale"])).numpy()
        rec = g["thr.sq"]
        assert rec.dtype == np.float32 and rec.shape == here.shape and np.array_equal(rec, rec.T)
        assert np.abs(rec.view(np.int32).astype(np.int64) - here.view(np.int32).astype(np.int64)).max() <= 1


def test_bond_radii_unknown_element_raises_and_caller_radii_are_taken():
    with pytest.raises(KeyError, match="atomic number"):
        ev.bond_radii([6, 26])
    assert ev.bond_radii([6, 26], radii={26: 1.34}).tolist() == [0.68, 1.34]
    assert ev.bond_radii([6], radii={6: 0.7}).tolist() == [0.7]


# ----------------------------------------------------------------------------- the pair test the kernel implements
@pytest.mark.parametrize("case", CASES)
def test_squared_sum_against_strict_threshold_reproduces_the_reference_counts(case):
    """fp32 (dx*dx + dy*dy) + dz*dz <= threshold[class pair] -- the arithmetic of csrc/sample_quality.hip restated in
    numpy -- gives the reference's bond matrices entry for entry (counts, signed sums, reference sums)."""
    g = _golden(case)
    z = g["z"]
    elements = sorted(set(z.tolist()))
    thr = g["thr.sq"]             # recorded with the bond matrices: the reference's sqrt test is host dependent
    cls = np.searchsorted(elements, z)
    heavy = z != 1

    def bonds(xyz):
        d = (xyz[:, None, :] - xyz[None, :, :]).astype(np.float32)
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + d[..., 2] * d[..., 2]
        b = s.astype(np.float32) <= thr[cls[:, None], cls[None, :]]
        np.fill_diagonal(b, False)
        return b.astype(np.int64)
    ref = bonds(g["ref"])
    counts, _ = raw_counts_from_golden(g)
    for k, xyz in enumerate(g["gen"]):
        gen = bonds(xyz)
        hh = np.ix_(heavy, heavy)
        got = [(ref != gen).sum(), (ref[hh] != gen[hh]).sum(), (ref - gen).sum(), (ref[hh] - gen[hh]).sum(), ref.sum(), ref[hh].sum()]
        assert got == counts[k].tolist(), (case, k)


# ----------------------------------------------------------------------------- assembly of the reference's tuples
@pytest.mark.parametrize("case", CASES)
def test_six_tuple_from_raw_counts(case):
    g = _golden(case)
    counts, sums = raw_counts_from_golden(g)
    got = ev.assemble_sample_qualities(counts, sums, len(g["z"]), int((g["z"] != 1).sum()))
    check_six(got, g)


def test_six_tuple_none_and_nan_branches():
    g = _golden("both_none")
    got = ev.assemble_sample_qualities(*raw_counts_from_golden(g), len(g["z"]), int((g["z"] != 1).sum()))
    assert got[0] is None and got[1] is None and got[2] == 0.0 and got[3] == 0.0
    g = _golden("all_none")
    got = ev.assemble_sample_qualities(*raw_counts_from_golden(g), len(g["z"]), int((g["z"] != 1).sum()))
    assert got[0] is None and got[1] is not None and got[1].shape[1] == 2
    g = _golden("no_bond")
    got = ev.assemble_sample_qualities(*raw_counts_from_golden(g), len(g["z"]), int((g["z"] != 1).sum()))
    assert all(np.isnan(v) for v in got[4] + got[5]) and got[2] == 1.0 and got[3] == 1.0
    g = _golden("mixed_all")                                 # rows of all_rmsds = the samples with a valid all-atom graph
    got = ev.assemble_sample_qualities(*raw_counts_from_golden(g), len(g["z"]), int((g["z"] != 1).sum()))
    assert got[0].shape[0] == int((g["diff.all"] == 0).sum()) and 0 < got[0].shape[0] < len(g["gen"])
    assert got[1].shape[0] == int((g["diff.heavy"] == 0).sum())


@pytest.mark.parametrize("case", CASES)
def test_seven_tuple_statistics_from_raw_counts(case):
    """Every sample as a one-sample reconstruction of its own frame (utils.py:239-266)."""
    g = _golden(case)
    counts, sums = raw_counts_from_golden(g)
    n, nh = len(g["z"]), int((g["z"] != 1).sum())
    per_frame = [ev.assemble_sample_qualities(counts[k:k + 1], sums[k:k + 1], n, nh) for k in range(len(counts))]
    got = np.array(ev.assemble_reconstruction(per_frame), dtype=np.float64)
    np.testing.assert_allclose(got, g["recon.stats"], rtol=1e-12, atol=0, equal_nan=True)


def test_ten_tuple_from_per_frame_tuples():
    frames = []
    for case in ("mixed_all", "both_none", "mixed_heavy"):
        g = _golden(case)
        frames.append(ev.assemble_sample_qualities(*raw_counts_from_golden(g), len(g["z"]), int((g["z"] != 1).sum())))
    all_r, heavy_r, valid, valid_all, ged, ged_all = ev.assemble_ensemble(frames)
    assert all_r.shape == (frames[0][0].shape[0], 2)                    # only the first frame has valid all-atom graphs
    assert heavy_r.shape == (frames[0][1].shape[0] + frames[2][1].shape[0], 2)
    assert valid == [f[2] for f in frames] and valid_all == [f[3] for f in frames]
    assert [len(x) for x in ged] == [16, 16, 16] and [len(x) for x in ged_all] == [16, 16, 16]
    none = ev.assemble_ensemble([frames[1]])
    assert none[0] is None and none[1] is None and none[2] == [0.0]


# ----------------------------------------------------------------------------- provenance of the goldens
def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_eval", os.path.join(GOLDEN, "make_golden_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not os.path.isdir("/root/reference/scripts"), reason="the reference checkout is not on this machine")
def test_goldens_regenerate_bit_exact_from_the_reference():
    mod = _generator()
    cases = mod.build_cases()
    assert sorted(cases) == sorted(CASES)
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "g12_sample_quality_*.npz"))) == \
        sorted(f"g12_sample_quality_{c}.npz" for c in CASES)
    for case, arrays in cases.items():
        g = _golden(case)
        assert sorted(g) == sorted(arrays), case
        for key, val in arrays.items():
            val = np.asarray(val)
            assert g[key].dtype == val.dtype and g[key].shape == val.shape, (case, key)
            assert g[key].tobytes() == val.tobytes(), (case, key)
    assert mod.cv_stats_columns() == json.load(open(os.path.join(GOLDEN, "g12_cv_stats_columns.json")))


# ----------------------------------------------------------------------------- CLI
def test_cv_stats_header_equals_the_reference_column_list(tmp_path):
    columns = json.load(open(os.path.join(GOLDEN, "g12_cv_stats_columns.json")))
    assert ev.CV_STATS_COLUMNS == columns
    stats = {c: None for c in columns}
    stats.update({"test_all_recon": 0.5, "sample_all_rmsd": float("nan")})
    run_ala.write_cv_stats(str(tmp_path / "cv_stats.csv"), stats)
    header, row = (tmp_path / "cv_stats.csv").read_text().splitlines()
    assert header.split(",") == columns
    cells = row.split(",")
    assert len(cells) == len(columns) and cells[columns.index("test_all_recon")] == "0.5"
    assert cells[columns.index("sample_heavy_rmsd")] == "" and cells[columns.index("sample_all_rmsd")] == "nan"
