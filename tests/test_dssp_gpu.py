"""Secondary structure on the device: K26 (csrc/dssp.hip) against the numpy restatement.  A class is thresholds on fp32
values that both sides round identically, then bit logic: every comparison here is integer EQUALITY, on every output of the
kernel, ``codes`` and ``hb_bits`` included.  Before the device is asked the restatement alone is held to produce something
worth comparing: a hydrogen bond in 1 - 50 % of the pairs inside the CA pre-filter of every random case with five residues
or more (one residue has no pair and two have none that can bond: those cases check the empty edge), and over the cases
together every class but the loop."""
import functools
import json

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import _lib, dssp
import dssp_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUTPUTS = ("class_counts", "n_class", "bad", "codes", "hb_bits")


def _frozen(want):
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want


def _want(xyz, z, bonds):
    t = dssp.backbone_table(z, bonds)
    return _frozen(R.assign(xyz, t["res"], t["prev"], t["link"]))


def _same(got, want, what=""):
    assert got["n_good"] == want["n_good"], what
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    good = ~got["bad"]
    assert (got["n_class"][good].sum(axis=1) == got["codes"].shape[1]).all(), what
    hist = np.stack([(got["codes"][good] == c).sum(axis=0) for c in range(8)], axis=1)
    assert np.array_equal(got["class_counts"], hist), what      # class_counts is the histogram of codes over the good structures


def _check(xyz, z, bonds, want=None, what="", **kw):
    got = dssp.assign(xyz, z, bonds, codes=True, hb_bits=True, device=DEV, **kw)
    _same(got, _want(xyz, z, bonds) if want is None else want, what)
    return got


def _launch(xyz, table):
    """``cgv_dssp_assign`` on the caller's tables: what ``assign`` does, for tables no bond graph gives."""
    x = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(DEV)
    S, n, Rn = int(x.shape[0]), int(x.shape[1]), int(table["res"].shape[0])
    d = {k: torch.from_numpy(np.ascontiguousarray(table[k], dtype=np.int32)).to(DEV) for k in ("res", "prev", "link")}
    out = {"class_counts": torch.zeros(Rn, 8, dtype=torch.int64, device=DEV), "n_class": torch.zeros(S, 8, dtype=torch.int32, device=DEV),
           "bad": torch.zeros(S, dtype=torch.int32, device=DEV), "codes": torch.zeros(S, Rn, dtype=torch.uint8, device=DEV),
           "hb_bits": torch.zeros(S, Rn, (Rn + 63) // 64, dtype=torch.int64, device=DEV)}
    _lib.call("cgv_dssp_assign", _lib.ptr(x), _lib.ptr(d["res"]), _lib.ptr(d["prev"]), _lib.ptr(d["link"]), S, n, Rn,
              *(_lib.ptr(out[k]) for k in OUTPUTS), _lib.stream_ptr())
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(n_class=got["n_class"].astype(np.int64), bad=got["bad"].astype(bool), hb_bits=got["hb_bits"].view(np.uint64))
    got["n_good"] = int((~got["bad"]).sum())
    return got


def _fraction(want):
    return want["hb"].sum() / float(max(want["inside"].sum(), 1))


SIZES = (1, 2, 5, 10, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def _chains(n_res, S, seed=0):
    """Random-torsion chains and the restatement's result, held to bond 1 - 50 % of the pairs inside the pre-filter."""
    z, bonds, xyz = R.random_chains(n_res, S, 1000 * n_res + S + seed)
    want = _want(xyz, z, bonds)
    if n_res >= 5:
        assert 0.01 <= _fraction(want) <= 0.5, (n_res, S, _fraction(want))
    else:
        assert not want["hb"].any()
    return z, bonds, xyz, want


@functools.lru_cache(maxsize=None)
def _built():
    """The built helices and sheets as ``{name: (z, bonds, xyz [1,n,3], want)}``."""
    out = {}
    for name, kind in (("alpha", R.ALPHA), ("310", R.HELIX_310), ("pi", R.PI_HELIX)):
        z, bonds = R.peptide(14, cap=True)
        out[name] = (z, bonds, R.ideal(kind, 14, cap=True)[None].astype(np.float32))
    for pose in R.SHEET_POSES:
        z, bonds, xyz = R.two_strands(pose)
        out[pose] = (z, bonds, xyz[None].astype(np.float32))
    return {k: (z, bonds, xyz, _want(xyz, z, bonds)) for k, (z, bonds, xyz) in out.items()}


def test_the_cases_together_hold_every_class_but_the_loop():
    seen = set()
    for n_res in SIZES + (dssp.limits()["residues"],):
        seen |= set(np.unique(_chains(n_res, 3)[3]["codes"]).tolist())
    seen |= set(np.unique(_chains(10, 1100)[3]["codes"]).tolist())
    for _, _, _, want in _built().values():
        seen |= set(np.unique(want["codes"]).tolist())
    assert set(range(7)) <= seen, sorted(seen)                  # H B E G I T S, by the restatement alone


# ----------------------------------------------------------------------------- sizes: both launch shapes, every word boundary
@pytest.mark.parametrize("n_res", SIZES)
@pytest.mark.parametrize("S", [1, 3])
def test_random_chains_of_every_size(n_res, S):
    z, bonds, xyz, want = _chains(n_res, S)
    _check(xyz, z, bonds, want=want, what=(n_res, S))


def test_a_peptide_at_the_limit_and_one_residue_more():
    lim = dssp.limits()
    for S in (1, 3):
        z, bonds, xyz, want = _chains(lim["residues"], S)
        got = _check(xyz, z, bonds, want=want, what=S)
        assert got["hb_bits"].shape[2] == (lim["residues"] + 63) // 64 and got["hb_bits"].any()
    z, bonds = R.peptide(lim["residues"] + 1, cap=True)
    with pytest.raises(ValueError, match="the kernel holds"):
        dssp.assign(np.zeros((1, len(z), 3), np.float32), z, bonds, device=DEV)


def test_many_structures_two_calls_and_cuts_of_the_structure_axis():
    z, bonds, xyz, want = _chains(10, 1100)                    # more structures than a block walks in one trip
    first = _check(xyz, z, bonds, want=want)
    again = _check(xyz, z, bonds, want=want)                   # two calls give identical arrays
    for k in OUTPUTS:
        assert np.array_equal(first[k], again[k]), k
    for per in (7, 1):
        _check(xyz, z, bonds, want=want, structures_per_launch=per, what=per)
    z, bonds, xyz, want = _chains(65, 3)                       # the block path
    for per in (2, 1):
        _check(xyz, z, bonds, want=want, structures_per_launch=per, what=(65, per))
    plain = dssp.assign(xyz, z, bonds, device=DEV)             # without the optional outputs
    assert "codes" not in plain and "hb_bits" not in plain
    assert np.array_equal(plain["class_counts"], want["class_counts"]) and np.array_equal(plain["n_class"], want["n_class"])


@pytest.mark.parametrize("name", ["alpha", "310", "pi", "anti", "par", "bridge"])
def test_built_helices_and_sheets(name):
    z, bonds, xyz, want = _built()[name]
    letter = {"alpha": "H", "310": "G", "pi": "I", "anti": "E", "par": "E", "bridge": "B"}[name]
    assert letter in R.strings(want["codes"])[0]
    got = _check(xyz, z, bonds, want=want, what=name)
    assert dssp.strings(got["codes"]) == R.strings(want["codes"])


# ----------------------------------------------------------------------------- the threshold
def test_an_acceptor_swept_in_one_ulp_steps_across_the_energy_threshold():
    """The carbonyl O of residue 0 of an alpha helix is moved along x until its bond to N-H of residue 4 breaks -- by
    bisection on the fp32 coordinate with the restatement -- and then swept 40 ulps to either side of that point."""
    z, bonds = R.peptide(8, cap=True)
    base = R.ideal(R.ALPHA, 8, cap=True).astype(np.float32)
    t = dssp.backbone_table(z, bonds)
    O = int(t["res"][0, 3])
    bit = lambda x: bool(R.hbonds(x[None], t["res"], t["prev"])[0][0, 0, 4])
    moved = lambda v: np.concatenate([base[:O], [[v, base[O, 1], base[O, 2]]], base[O + 1:]]).astype(np.float32)
    lo = hi = base[O, 0]
    assert bit(base)
    step = np.float32(0.25) if bit(moved(lo + np.float32(4.0))) is False else None
    assert step is not None
    while bit(moved(hi)):
        hi = np.float32(hi + step)
    lo = np.float32(hi - step)
    while np.nextafter(lo, np.float32(np.inf)) < hi:           # bonded at lo, not at hi
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        lo, hi = (mid, hi) if bit(moved(mid)) else (lo, mid)
    v = lo
    for _ in range(40):
        v = np.nextafter(v, np.float32(-np.inf))
    sweep = []
    for _ in range(81):
        sweep.append(moved(v))
        v = np.nextafter(v, np.float32(np.inf))
    xyz = np.array(sweep, dtype=np.float32)
    want = _want(xyz, z, bonds)
    assert 0 < want["hb"][:, 0, 4].sum() < len(xyz)            # the sweep contains both outcomes
    got = _check(xyz, z, bonds, want=want)
    assert np.array_equal((got["hb_bits"][:, 0, 0] >> np.uint64(4)) & np.uint64(1), want["hb"][:, 0, 4].astype(np.uint64))


# ----------------------------------------------------------------------------- bad structures
def test_structures_with_a_nan_in_a_table_atom_are_bad_and_the_rest_unchanged():
    z9, bonds9, xyz9 = R.random_chains(65, 9, 5)
    clean = _want(xyz9, z9, bonds9)
    t = dssp.backbone_table(z9, bonds9)
    broken = np.array(xyz9)
    broken[0, t["res"][5, 1], 0] = np.nan                      # a CA
    broken[4, t["prev"][0, 1], 1] = np.inf                     # the acetyl's O
    broken[8, t["res"][64, 3], 2] = -np.inf                    # the last O
    got = _check(broken, z9, bonds9, what="NaN")
    assert got["bad"].tolist() == [True, False, False, False, True, False, False, False, True] and got["n_good"] == 6
    assert (got["n_class"][[0, 4, 8]] == -1).all() and (got["codes"][[0, 4, 8]] == 255).all() and not got["hb_bits"][[0, 4, 8]].any()
    keep = [1, 2, 3, 5, 6, 7]
    for k in ("codes", "hb_bits", "n_class"):
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    z, bonds, xyz, _ = _chains(10, 3)                          # the wave path
    broken = np.array(xyz)
    broken[1, 3] = np.nan                                      # N of the first residue
    got = _check(broken, z, bonds, what="NaN, wave path")
    assert got["bad"].tolist() == [False, True, False]


def test_a_nan_in_a_side_chain_atom_is_not_bad():
    z, bonds, xyz, want = _chains(10, 3)
    z2, bonds2 = np.concatenate([z, [6, 6]]), np.concatenate([bonds, [[4, len(z)], [8, len(z) + 1]]])     # a CB on two CAs
    x2 = np.concatenate([xyz, np.zeros((3, 2, 3), np.float32)], axis=1)
    x2[0, -2], x2[1, -1] = np.nan, np.inf
    got = _check(x2, z2, bonds2, want=want)
    assert not got["bad"].any() and got["n_good"] == 3


# ----------------------------------------------------------------------------- chain breaks
def test_no_turn_and_no_bridge_across_a_chain_break():
    for name, cut in (("alpha", 6), ("anti", 2)):
        z, bonds, xyz, whole = _built()[name]
        table = dssp.backbone_table(z, bonds)
        table["link"] = table["link"].copy()
        table["link"][cut] = 0
        want = R.assign(xyz, table["res"], table["prev"], table["link"])
        assert np.array_equal(want["hb"], whole["hb"])           # the bonds are the same: only what may be made of them changes
        if name == "alpha":
            assert whole["parts"]["turn"][1, 0, cut - 3:cut + 1].all()
            assert not any(want["parts"]["turn"][n - 3, 0, cut - n + 1:cut + 1].any() for n in (3, 4, 5))     # i <= cut < i + n
            assert (want["codes"][0] == 0).sum() < (whole["codes"][0] == 0).sum()
        else:
            assert whole["parts"]["anti"][0, cut].any() and not want["parts"]["anti"][0, cut:cut + 2].any()
            assert (want["codes"][0] == 2).sum() < (whole["codes"][0] == 2).sum()
        _same(_launch(xyz, table), want, name)


def test_bits_past_the_last_residue_are_zero():
    z, bonds, xyz, want = _chains(65, 3)
    got = dssp.assign(xyz, z, bonds, hb_bits=True, device=DEV)
    assert got["hb_bits"].shape == (3, 65, 2) and not (got["hb_bits"][:, :, 1] >> np.uint64(1)).any()
    assert np.array_equal(got["hb_bits"], want["hb_bits"]) and got["hb_bits"][:, :, 0].any()


# ----------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _ensembles():
    rng = np.random.default_rng(7)
    z, bonds = R.peptide(12, cap=True)
    jitter = lambda kind, S: (rng.normal(kind[0], 3.0, (S, 12)), rng.normal(kind[1], 3.0, (S, 12)))
    helical = R.backbone(*jitter(R.ALPHA, 12), cap=True).astype(np.float32)
    extended = R.backbone(*jitter(R.STRAND, 10), cap=True).astype(np.float32)
    return z, bonds, helical, extended


def test_a_helix_that_is_lost(tmp_path, capsys):
    z, bonds, helical, extended = _ensembles()
    want_h, want_e = _want(helical, z, bonds), _want(extended, z, bonds)
    core = list(range(2, 10))
    assert (want_h["codes"][:, core] == 0).all() and not np.isin(want_e["codes"], (0, 3, 4)).any()      # the restatement says which is which
    _check(helical, z, bonds, want=want_h)
    _check(extended, z, bonds, want=want_e)
    stats = dssp.compare(helical, extended, z, bonds, device=DEV)
    assert set(stats) == set(dssp.DSSP_STATS_KEYS)
    assert set(core) <= {r for r, s in stats["lost"] if s == "H"}
    assert stats["gained"] == [] and stats["agreement_gen"] < stats["agreement_ref"] and stats["propensity_rmse"] > stats["floor"]["propensity_rmse"]
    assert stats["consensus_ref"][2:10] == "H" * 8 and stats["helix_fraction"]["mean_gen"] == 0.0 and stats["helix_fraction"]["mean_ref"] >= 8 / 12
    same = dssp.compare(helical, helical, z, bonds, device=DEV)
    assert same["propensity_rmse"] == 0.0 and same["lost"] == [] and same["agreement_ref"] == same["agreement_gen"]
    # the command line on the same files
    np.savez(tmp_path / "ref.npz", xyz=helical, z=z, bonds=bonds)
    np.savez(tmp_path / "gen.npz", xyz=extended.reshape(5, 2, -1, 3))
    out, codes = tmp_path / "stats.json", tmp_path / "codes.npz"
    capsys.readouterr()
    dssp.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -out {out} -codes {codes} -device {DEV}".split())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["out"] == str(out) and line["dssp_stats"] == json.loads(json.dumps(dssp.summary_of(stats)))
    with open(out) as f:
        written = json.load(f)
    assert set(written) == set(dssp.DSSP_STATS_KEYS) and written["lost"] == stats["lost"]
    with np.load(codes) as f:
        assert np.array_equal(f["codes"], want_e["codes"]) and f["strings"].tolist() == R.strings(want_e["codes"])
