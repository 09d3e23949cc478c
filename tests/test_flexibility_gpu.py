"""Mean structure and RMSF on the device: K21 (csrc/align_mean.hip) against the numpy restatement, whose rotation comes
from LAPACK's eigh of the same key matrix.  Tolerances are derived from the restatement's own numbers (the gap under the
key matrix's top eigenvalue, the magnitudes summed), never from what the kernel returns."""
import functools
import json

import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd import backmap as bm, flexibility, options
import flexibility_restatement as R
import internal_coords_restatement as IR

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -52
C_ROT = 32.0


def _launch(x, sel, ref, spl=4096, want_aligned=True):
    """One pass through ``flexibility.align_accumulate`` (chunks of ``spl``); host arrays."""
    p = flexibility._Passes(x, sel, spl, DEV)
    out = torch.empty(p.S, p.n, 3, dtype=torch.float32, device=DEV) if want_aligned else None
    state = p.run(torch.from_numpy(np.array(ref, dtype=np.float64)).to(DEV), aligned=out)
    torch.cuda.synchronize()
    return {"sum": state["sum"].cpu().numpy(), "dev2": state["dev2"].cpu().numpy(), "n_good": int(state["n_good"].cpu()[0]),
            "rmsd2": p.rmsd2.cpu().numpy(), "bad": p.bad.cpu().numpy().astype(bool),
            "aligned": None if out is None else out.cpu().numpy()}


def _bounds(x, sel, ref, want):
    """Per-atom bounds on |sum - restatement| (largest component) and |dev2 - restatement|, per-structure on rmsd2.

    Rotation.  Both sides solve the same key matrix K, one by Jacobi (csrc/superpose_rot.h), one by eigh.  The header
    routine, compiled for the host as a stand-alone program (-ffp-contract=off, under AddressSanitizer and UBSan) and
    run on 400 cross-covariances built exactly as this file's inputs are (n = 3 .. 600, full and scattered selections)
    plus mirrored copies, is at most 9.2 x 2^-52 |K|_F / gap from eigh's rotation in Frobenius norm -- the first-order
    perturbation scale of an eigenvector.  C_ROT = 32 is 3.5 times that.  The entries of K differ between the sides by
    the order in which M is summed over the m selected atoms: at most m 2^-52 |K|_F, which moves the rotation by that
    over the gap.  So |dR|_F <= (C_ROT + m) 2^-52 |K|_F / gap per structure.
    Centring.  The centroid (a sum of m terms, either order) and the subtraction: (m + 2) 2^-52 max|x| per coordinate;
    the same for the target.  The product R a: 4 roundings of |y|.
      d y_si  = |dR|_F |y_si| + (m + 2) 2^-52 max|x_s| + 4 2^-52 |y_si|
      d sum_i = sum_s d y_si + (S + 1) 2^-52 sum_s |y_si|            (S additions in another order)
      d dev2_i = sum_s 2 |y_si - b_i| (d y_si + d b) + (S + 8) 2^-52 sum_s |y_si - b_i|^2
    rmsd2 = max(0, G - 2 lambda) / m: lambda is within 8 2^-52 |K|_F of eigh's (csrc/superpose_eig.h: 7.4 measured
    there, 4.2 on these inputs) plus m 2^-52 |K|_F from the summation of M; G is m sums of rounded squares:
      d rmsd2_s = 2^-52 (2 (8 + m) |K|_F + (m + 8) G) / m.
    (Measured on an MI355X over this file's cases, worst error / bound: 0.038 for sum, 0.047 for dev2, 0.19 for
    rmsd2 in the main sweep; 0.068 for rmsd2 on the degenerate selections; 0.038 with bad structures; the two forms
    0.006 / 0.0007 / 0.020; the iterated mean 0.0008 and rmsf 0.00002 of their accumulated bounds.)"""
    xs = np.asarray(x, dtype=np.float64)
    S, n = xs.shape[:2]
    m = len(sel)
    good = ~want["bad"]
    b = np.asarray(ref, dtype=np.float64)
    b = b - b[np.asarray(sel)].mean(0)
    y = np.where(good[:, None, None], want["aligned"], 0.0)
    ynorm = np.linalg.norm(y, axis=2)
    rot = np.where(good, (C_ROT + m) * U * want["knorm"] / np.where(want["gap"] > 0, want["gap"], 1.0), 0.0)
    cen = np.where(good, (m + 2) * U * np.abs(np.where(np.isfinite(xs), xs, 0.0)).max((1, 2)), 0.0)
    dy = rot[:, None] * ynorm + cen[:, None] + 4 * U * ynorm
    dist = np.where(good[:, None], np.linalg.norm(y - b[None], axis=2), 0.0)
    db = (m + 2) * U * np.abs(ref).max()
    return {"sum": dy.sum(0) + (S + 1) * U * ynorm.sum(0),
            "dev2": (2 * dist * (dy + db)).sum(0) + (S + 8) * U * (dist ** 2).sum(0),
            "rmsd2": U * (2 * (8 + m) * want["knorm"] + (m + 8) * want["g"]) / m}


def _within(got, want, bounds, what, keys=("sum", "dev2", "rmsd2")):
    good = ~want["bad"]
    assert np.array_equal(got["bad"], want["bad"]) and got["n_good"] == want["n_good"], what
    assert np.isnan(got["rmsd2"][~good]).all() and np.isfinite(got["rmsd2"][good]).all(), what
    assert np.isfinite(got["sum"]).all() and np.isfinite(got["dev2"]).all(), what
    err = {"sum": np.abs(got["sum"] - want["sum"]).max(1), "dev2": np.abs(got["dev2"] - want["dev2"]),
           "rmsd2": np.abs(got["rmsd2"] - want["rmsd2"])[good]}
    lim = {"sum": bounds["sum"], "dev2": bounds["dev2"], "rmsd2": bounds["rmsd2"][good]}
    for k in keys:
        ratio = float((err[k][lim[k] > 0] / lim[k][lim[k] > 0]).max(initial=0.0))
        print(what, k, "worst error / bound =", ratio)
        assert (err[k] <= lim[k]).all(), (what, k, ratio)


@functools.lru_cache(maxsize=None)
def _case(n, S, scattered):
    """A random base in a 10 A box, S copies with 0.3 A noise, each randomly rotated and translated; the selection all
    atoms or max(3, n - 5) of them scattered and in no order; the target is the base; the restatement's result."""
    rng = np.random.default_rng(100000 * n + 10 * S + int(scattered))
    base = rng.uniform(0, 10, (n, 3))
    x = R.noisy_copies(rng, base, S, 0.3)
    sel = rng.permutation(n)[:max(3, n - 5)] if scattered else np.arange(n)
    want = R.align_accumulate(x, sel, base)
    for v in (x, base, sel, *want.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x, sel, base, want


# ----------------------------------------------------------------------------- 1. one launch against the restatement
@pytest.mark.parametrize("scattered", [False, True])
@pytest.mark.parametrize("S", [1, 2, 3, 257])                               # 257: 65 ranges of 4, the last one short
@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 130, 256, 257, 300])       # 256 | 257: a wave | a block owns a structure
def test_one_launch_equals_the_restatement_within_the_derived_bound(n, S, scattered):
    """Worst error / bound measured on an MI355X over the 72 cases: sum 0.038 (n 4, S 1, m 3), dev2 0.047 (the same
    case), rmsd2 0.19 (n 3, S 257) -- the bounds are worst-case sums of absolute values, the errors add like a random
    walk."""
    x, sel, base, want = _case(n, S, scattered)
    got = _launch(x, sel, base)
    _within(got, want, _bounds(x, sel, base, want), f"n {n} S {S} m {len(sel)}")
    # the aligned structures, rounded to fp32: half an ulp of the coordinate on top of d y
    err = np.abs(got["aligned"].astype(np.float64) - want["aligned"]).max()
    assert err <= 2.0 ** -24 * np.abs(want["aligned"]).max() + 1e-9, err


# ----------------------------------------------------------------------------- 2. degenerate selections
@pytest.mark.parametrize("kind", ["collinear", "coincident", "identical"])
def test_degenerate_selections_are_ordinary_inputs(kind):
    """The rotation about a line of atoms is free, so only what the selected atoms determine is compared: rmsd2 (within
    the bound, which needs no gap) and that the selected atoms' dev2 adds up to m x the sum of rmsd2."""
    rng = np.random.default_rng({"collinear": 1, "coincident": 2, "identical": 3}[kind])
    n, S, sel = 6, 9, np.array([4, 0, 2])
    base = rng.uniform(0, 10, (n, 3))
    if kind == "collinear":
        base[0], base[2] = base[4] + 1.5 * (base[1] - base[4]), base[4] - 0.7 * (base[1] - base[4])
    if kind == "coincident":
        base[2] = base[0]
    x = np.stack([(base @ R.random_rotation(rng).T + rng.uniform(-5, 5, 3)) for _ in range(S)]).astype(np.float32)
    if kind == "identical":
        x = np.repeat(base[None].astype(np.float32), S, 0)
    want = R.align_accumulate(x, sel, base)
    got = _launch(x, sel, base)
    assert np.isfinite(got["aligned"]).all()
    _within(got, want, _bounds(x, sel, base, want), kind, keys=("rmsd2",))
    total = got["dev2"][sel].sum()
    assert abs(total - 3 * got["rmsd2"].sum()) <= 1e-9 * max(total, 1.0) + 64 * U * want["g"].sum()
    assert got["rmsd2"].max() < 1e-9                                        # rigid copies up to fp32 storage


# ----------------------------------------------------------------------------- 3. mirror
def test_mirrored_copies_are_not_superposed():
    rng = np.random.default_rng(7)
    n = 20
    base = rng.uniform(0, 10, (n, 3))
    x = np.stack([((base * [1, 1, -1]) @ R.random_rotation(rng).T + rng.uniform(-5, 5, 3)) for _ in range(5)]).astype(np.float32)
    sel = np.arange(n)
    want = R.align_accumulate(x, sel, base)
    got = _launch(x, sel, base)
    assert want["rmsd2"].min() > 1.0 and got["rmsd2"].min() > 1.0
    _within(got, want, _bounds(x, sel, base, want), "mirror")


# ----------------------------------------------------------------------------- 4. bad structures
def test_nan_and_inf_structures_are_flagged_and_enter_nothing():
    x, sel, base, _ = _case(65, 257, True)
    clean = _launch(x, sel, base)
    bad = x.copy()
    outside = [a for a in range(65) if a not in sel][0]
    bad[0, sel[3], 1] = np.nan
    bad[5, outside, 2] = np.nan                                             # outside the selection: still a bad structure
    bad[256, sel[0], 0] = np.inf
    got = _launch(bad, sel, base)
    flagged = np.zeros(257, dtype=bool)
    flagged[[0, 5, 256]] = True
    assert np.array_equal(got["bad"], flagged) and got["n_good"] == 254 and clean["n_good"] == 257
    assert np.isnan(got["rmsd2"][flagged]).all() and np.isnan(got["aligned"][flagged]).all()
    # the others: bit for bit what they are without the injected values
    assert got["rmsd2"][~flagged].tobytes() == clean["rmsd2"][~flagged].tobytes()
    assert got["aligned"][~flagged].tobytes() == clean["aligned"][~flagged].tobytes()
    want = R.align_accumulate(bad, sel, base)
    _within(got, want, _bounds(bad, sel, base, want), "bad structures")
    # ranges 0 and 64 lose a structure each, range 1 another: every other range's partial sum is unchanged, so the
    # difference of the two runs is the three structures' own contribution within the summation bound
    gone = R.align_accumulate(x[flagged], sel, base)
    assert np.abs((clean["sum"] - got["sum"]) - gone["sum"]).max() <= 2 * 258 * U * np.abs(clean["aligned"]).sum(0).max()


# ----------------------------------------------------------------------------- 5. repeat, chunking, refusals
def test_two_identical_calls_give_identical_bits():
    for n in (130, 300):
        x, sel, base, _ = _case(n, 257, True)
        a, b = _launch(x, sel, base), _launch(x, sel, base)
        for k in ("sum", "dev2", "rmsd2", "bad", "aligned"):
            assert a[k].tobytes() == b[k].tobytes(), (n, k)
        assert a["n_good"] == b["n_good"] == 257


def test_chunked_launches_agree_within_the_summation_bound():
    """A structure's rotation, rmsd2 and aligned coordinates do not depend on the launch it is in: bit for bit.  sum and
    dev2 are S terms added in another order: each side is within (S - 1) 2^-53 sum|term| of the exact sum, the two
    within c S 2^-52 sum|term| of each other with c = 1."""
    x, sel, base, want = _case(130, 257, True)
    one, many = _launch(x, sel, base, 4096), _launch(x, sel, base, 64)
    assert one["rmsd2"].tobytes() == many["rmsd2"].tobytes() and one["aligned"].tobytes() == many["aligned"].tobytes()
    assert one["n_good"] == many["n_good"] == 257
    terms = np.abs(one["aligned"].astype(np.float64)).sum(0).max(1)
    assert (np.abs(one["sum"] - many["sum"]).max(1) <= 257 * U * terms).all()
    assert (np.abs(one["dev2"] - many["dev2"]) <= 257 * U * want["abs_dev2"] * (1 + 1e-6)).all()


def test_bad_arguments_raise_before_a_launch():
    x = torch.zeros(4, 6, 3, device=DEV)
    sel = torch.arange(3, dtype=torch.int32, device=DEV)
    ref = torch.zeros(6, 3, dtype=torch.float64, device=DEV)
    st = flexibility.new_state(6, DEV)
    per = dict(rmsd2=torch.zeros(4, dtype=torch.float64, device=DEV), bad=torch.zeros(4, dtype=torch.int32, device=DEV))
    flexibility.align_accumulate(x, sel, ref, **st, **per)                 # the well-formed call
    assert int(st["n_good"].cpu()[0]) == 4
    with pytest.raises(ValueError, match="float32"):
        flexibility.align_accumulate(x.double(), sel, ref, **st, **per)
    with pytest.raises(ValueError, match="int32"):
        flexibility.align_accumulate(x, sel.long(), ref, **st, **per)
    with pytest.raises(ValueError, match="float64"):
        flexibility.align_accumulate(x, sel, ref.float(), **st, **per)
    with pytest.raises(ValueError, match="lists 0"):
        flexibility.align_accumulate(x, sel[:0], ref, **st, **per)
    with pytest.raises(ValueError, match="rmsd2"):
        flexibility.align_accumulate(x, sel, ref, **st, rmsd2=per["rmsd2"][:3], bad=per["bad"])
    with pytest.raises(ValueError, match="m = 0"):
        flexibility.mean_structure(x, [], device=DEV)
    with pytest.raises(ValueError, match="names atom 6"):
        flexibility.mean_structure(x, [0, 1, 6], device=DEV)
    with pytest.raises(ValueError, match="atoms per structure"):
        flexibility.mean_structure(torch.zeros(1, flexibility.limits()["atoms"] + 1, 3, device=DEV))
    assert int(st["n_good"].cpu()[0]) == 4                                   # nothing ran


# ----------------------------------------------------------------------------- 6. iteration
def test_mean_structure_follows_the_restatement_pass_by_pass():
    """The bound of test 1, accumulated: pass p leaves the mean within e_p = max_i d sum_i / n_good of the restatement's.
    A target displaced by e turns the fit by at most e / r_g (r_g: the selection's radius of gyration) and so moves an
    atom at distance r from the centre by at most A e, A = 1 + max r / r_g: the error after the last pass is at most
    E = sum_p A^(P - p) e_p.  rmsf^2 = dev2 / n_good - |shift|^2 inherits d dev2_i / n_good + 4 D_i E (D_i: the atom's
    root-mean-square distance from the target), and rmsf that over 2 rmsf."""
    rng = np.random.default_rng(11)
    n, S = 40, 600
    base = rng.uniform(0, 10, (n, 3))
    x = R.noisy_copies(rng, base, S, rng.uniform(0.1, 0.3, n))
    sel = rng.permutation(n)[:33]
    want = R.mean_structure(x, sel)
    got = flexibility.mean_structure(x, sel, structures_per_launch=256, device=DEV)
    assert got["iterations"] == want["iterations"] >= 2 and got["converged"] and want["converged"]
    assert got["n_good"] == S and not got["bad"].any() and abs(got["last_move"] - want["last_move"]) < 1e-9
    c = want["mean"][sel]
    A = 1.0 + np.linalg.norm(want["mean"], axis=1).max() / np.sqrt((c ** 2).sum(1).mean())
    E, last = 0.0, None
    for k, res in enumerate(want["passes"]):
        target = x[0].astype(np.float64) if k == 0 else want["passes"][k - 1]["sum"] / S
        last = _bounds(x, sel, target, res)
        E = A * E + last["sum"].max() / S
    err_mean = np.abs(got["mean"] - want["mean"]).max()
    D = np.sqrt(want["passes"][-1]["dev2"] / S)
    lim_rmsf = (last["dev2"] / S + 4 * D * E) / (2 * want["rmsf"])
    err_rmsf = np.abs(got["rmsf"] - want["rmsf"])
    print("mean: error / bound", err_mean / E, " rmsf:", (err_rmsf / lim_rmsf).max())
    assert err_mean <= E and (err_rmsf <= lim_rmsf).all()
    assert np.abs(got["rmsd"] - want["rmsd"]).max() <= 1e-9
    # aligned() reproduces rmsd: fp32 storage of the aligned coordinates, and the mean against the last pass's target
    al = flexibility.aligned(x, got["mean"], sel, device=DEV)
    assert al.dtype == np.float32 and al.shape == (S, n, 3)
    d = al[:, sel].astype(np.float64) - (got["mean"] - got["mean"][sel].mean(0))[sel]
    again = np.sqrt((d * d).sum(2).mean(1))
    assert np.abs(again - got["rmsd"]).max() <= np.sqrt(3) * 2.0 ** -24 * np.abs(al).max() + got["last_move"] + 1e-9


# ----------------------------------------------------------------------------- 7. forced path
def test_both_forms_agree_on_a_size_both_accept():
    x, sel, base, want = _case(130, 257, True)
    bounds = _bounds(x, sel, base, want)
    try:
        options.set("align_form", 2)
        block = _launch(x, sel, base)
        options.set("align_form", 1)
        wave = _launch(x, sel, base)
        with pytest.raises(ValueError, match="does not hold 300 atoms"):
            _launch(*_case(300, 3, False)[:3])
    finally:
        options.set("align_form", 0)
    _within(block, want, bounds, "block form")
    _within(wave, want, bounds, "wave form")
    rule = _launch(x, sel, base)
    assert all(rule[k].tobytes() == wave[k].tobytes() for k in ("sum", "dev2", "rmsd2", "aligned"))
    # different reduction trees: not the same bits, but each within the bound of the restatement, so twice apart
    assert (np.abs(block["sum"] - wave["sum"]).max(1) <= 2 * bounds["sum"]).all()
    assert (np.abs(block["rmsd2"] - wave["rmsd2"]) <= 2 * bounds["rmsd2"]).all()


# ----------------------------------------------------------------------------- 8. compare and the command line
def test_compare_on_two_amplitudes():
    rng = np.random.default_rng(5)
    n = 30
    base, sigma = rng.uniform(0, 10, (n, 3)), rng.uniform(0.05, 0.3, n)
    ref, gen = R.noisy_copies(rng, base, 1200, sigma), R.noisy_copies(rng, base, 900, 0.6 * sigma)
    z, bonds = np.array([1, 1] + [6] * (n - 2)), np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    stats = flexibility.compare(ref, gen, z, bonds, device=DEV)
    assert set(stats) == set(flexibility.FLEX_STATS_KEYS) and json.loads(json.dumps(stats)) == stats
    assert stats["labels"] == list(range(2, n)) and stats["params"]["atoms"] == list(range(2, n)) and stats["params"]["groups"] is None
    assert abs(stats["ratio"] - 0.6) < 0.02 and stats["pearson"] > 0.99 and abs(stats["floor"]["ratio"] - 1.0) < 0.03
    assert stats["mean_rmsd"] < 0.05 and stats["floor"]["mean_rmsd"] < 0.05 and stats["n_bad_ref"] == 0
    sel = np.arange(2, n)
    runs = {"ref": R.mean_structure(ref, sel), "gen": R.mean_structure(gen, sel), "even": R.mean_structure(ref[0::2], sel),
            "odd": R.mean_structure(ref[1::2], sel)}
    want = flexibility.compare_from_runs(runs, sel)
    assert np.allclose(stats["rmsf_ref"], want["rmsf_ref"], rtol=0, atol=1e-9) and abs(stats["ratio"] - want["ratio"]) < 1e-9
    assert abs(stats["rmsd_to_mean"]["mean_ref"] - want["rmsd_to_mean"]["mean_ref"]) < 1e-9
    for k in ("ref", "gen", "even", "odd"):
        assert stats["convergence"][k]["iterations"] == want["convergence"][k]["iterations"] and stats["convergence"][k]["converged"]
    beads = flexibility.compare(ref, gen, z, bonds, atoms="all", groups="bead", mapping=np.arange(n) // 10, device=DEV)
    assert beads["labels"] == [0, 1, 2] and len(beads["rmsf_ref"]) == 3 and abs(beads["ratio"] - 0.6) < 0.03


def test_backmap_cli_writes_flex_stats_and_nothing_without_the_switch(tmp_path, capsys):
    """A fresh dipeptide-shaped run directory (the fixture pattern of test_contacts_gpu.py) and a random reference of 9
    frames: the files have the documented keys; without the switch no file is written and the outputs are what they were."""
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
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    base = f"-model {d} -cg {tmp_path / 'cg.npz'} -top {tmp_path / 'top.npz'} -n_samples 4"
    bm.main(f"{base} -out {tmp_path / 'a' / 'out.npz'} --flex_stats -flex_aligned {tmp_path / 'a' / 'aligned.npz'} "
            f"-ref {tmp_path / 'ref.npz'}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(line["flex_stats"]) == set(flexibility.summary_of({k: None for k in flexibility.FLEX_STATS_KEYS}))
    stats = json.loads((tmp_path / "a" / "flex_stats.json").read_text())
    assert set(stats) == set(flexibility.FLEX_STATS_KEYS) and line["flex_stats"] == flexibility.summary_of(stats)
    heavy = np.flatnonzero(np.asarray(IR.ALA_Z) != 1).tolist()
    assert stats["n_ref"] == 9 and stats["n_gen"] == 12 and stats["labels"] == heavy and len(stats["rmsf_gen"]) == len(heavy)
    assert stats["params"] == {"atoms": heavy, "groups": None, "max_iter": 10, "tol": 1e-4, "n_bins": 20}
    with np.load(tmp_path / "a" / "aligned.npz") as f:
        assert f["xyz"].shape == (12, n, 3) and f["xyz"].dtype == np.float32 and f["mean"].shape == (n, 3)
        assert f["atoms"].tolist() == heavy and f["rmsf"].shape == (n,)
        # every structure centred on its selection, up to the fp32 rounding of the stored coordinates
        assert np.abs(f["xyz"][:, heavy].astype(np.float64).mean(1)).max() <= 2.0 ** -23 * np.abs(f["xyz"]).max()
    bm.main(f"{base} -out {tmp_path / 'b' / 'out.npz'}".split())
    line_b = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "flex_stats" not in line_b and set(line_b) == set(line) - {"flex_stats"}
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["out.npz"]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["aligned.npz", "flex_stats.json", "out.npz"]
    with np.load(tmp_path / "a" / "out.npz") as fa, np.load(tmp_path / "b" / "out.npz") as fb:
        assert set(fa.files) == set(fb.files) and fa["xyz"].tobytes() == fb["xyz"].tobytes()
