"""Backmapping on the device: K14 (csrc/ensemble_check.hip) against the dense restatement, ``backmap`` against the
already pinned ``evaluate.sample_ensemble``, its invariances, the CLI, and its coexistence with a running Trainer."""
import json

import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd import _lib, backmap as bm, evaluate as ev, ops, run_ala
from coarsegrainingvae_amd.trainer import Trainer
import ensemble_check_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-4            # the suite's output tolerance (tests/test_hip_parity.py)
FILL = {2: 0.68, 3: 0.68, 4: 0.68, 5: 0.68}     # synthetic frames carry type labels 1..8: radii for the untabulated ones


def _launch(gen, z, fp, K, bonds, bond_ptr=None, radii=None):
    plan = ev.QualityPlan(z, fp, DEV, radii=radii)
    raw = ev.ensemble_check(torch.as_tensor(gen, dtype=torch.float32).reshape(-1, 3).to(DEV), K, plan, bonds, bond_ptr)
    assert raw.counts.dtype == torch.int32 and raw.pair_sums.dtype == torch.float64 and raw.counts.is_cuda
    assert raw.counts.shape == (len(fp) - 1, K, 4) and raw.pair_sums.shape == (len(fp) - 1, K, K, 2)
    return raw


def _compare(raw, want_counts, want_sums):
    counts, sums = raw.counts.cpu().long(), raw.pair_sums.cpu().numpy()
    print("counts", counts.reshape(-1, 4)[:8].tolist(), "max |rel| of pair sums",
          float(np.max(np.abs(sums - want_sums.numpy()) / np.maximum(np.abs(want_sums.numpy()), 1e-300))))
    assert torch.equal(counts, want_counts)
    np.testing.assert_allclose(sums, want_sums.numpy(), rtol=1e-10, atol=0)
    K = sums.shape[1]
    assert np.array_equal(sums, sums.transpose(0, 2, 1, 3)) and not sums[:, np.arange(K), np.arange(K)].any()


# ----------------------------------------------------------------------------- K14 vs the restatement
def test_kernel_gives_the_hand_computed_counts_on_the_hand_built_cases():
    names, gen, z, bonds, want = R.cases()
    K, n = gen.shape[:2]
    raw = _launch(gen, z, [0, n], K, bonds)
    assert raw.counts.cpu()[0].tolist() == want.tolist(), names
    _compare(raw, *R.restate(gen.reshape(-1, 3), z, [0, n], K, bonds))


def _mixed_frames(K, with_big, seed=0):
    """A 22-atom frame (n < 64), the 74-atom molecule and a 130-atom frame (neither a multiple of 64), optionally a
    2000-atom frame; per-frame bond lists; K jittered samples each."""
    rng = np.random.default_rng(seed)
    xyz_a, z_a, bonds_a, _ = R.alkane()
    frames = []
    for n, box in ((22, 4.0), (130, 7.0)) + (((2000, 17.0),) if with_big else ()):
        frames.append((rng.uniform(0, box, (n, 3)), rng.integers(1, 9, n), np.stack([np.arange(n - 1), np.arange(1, n)], 1)))
    frames.insert(1, (xyz_a, z_a, bonds_a))
    gen = [f[0][None] + 0.08 * rng.standard_normal((K,) + f[0].shape) for f in frames]
    gen[1][0] = xyz_a                                      # one valid sample among them
    z = np.concatenate([f[1] for f in frames])
    fp = np.concatenate([[0], np.cumsum([len(f[1]) for f in frames])])
    bond_ptr = np.concatenate([[0], np.cumsum([len(f[2]) for f in frames])])
    return (np.concatenate([g.reshape(-1, 3) for g in gen]).astype(np.float32), z, fp, np.concatenate([f[2] for f in frames]),
            bond_ptr)


@pytest.mark.parametrize("K,with_big", [(1, False), (3, True), (16, False), (128, False)])
def test_kernel_equals_the_restatement_on_frames_of_different_sizes(K, with_big):
    gen, z, fp, bonds, bond_ptr = _mixed_frames(K, with_big)
    raw = _launch(gen, z, fp, K, bonds, bond_ptr, radii=FILL)
    want_counts, want_sums = R.restate(gen, z, fp, K, bonds, bond_ptr, radii=FILL)
    _compare(raw, want_counts, want_sums)
    assert int(want_counts[..., 0].max()) > 0 and int(want_counts[..., 1].max()) > 0          # not vacuous
    assert want_counts[1, 0].tolist() == [0, 0, 0, 0]
    again = _launch(gen, z, fp, K, bonds, bond_ptr, radii=FILL)
    assert torch.equal(again.counts, raw.counts) and torch.equal(again.pair_sums, raw.pair_sums)   # bit for bit
    # an empty bond list: nothing can be missing, every inferred bond is extra
    none = _launch(gen, z, fp, K, np.zeros((0, 2), np.int64), radii=FILL)
    want_none = R.restate(gen, z, fp, K, np.zeros((0, 2), np.int64), radii=FILL)
    _compare(none, *want_none)
    assert not none.counts[..., 0].any() and int(none.counts[..., 1].max()) > 0
    # no topology at all: the pair sums alone
    bare = _launch(gen, z, fp, K, None, radii=FILL)
    assert not bare.counts.any() and torch.equal(bare.pair_sums, raw.pair_sums)


def test_a_limit_exceeded_is_an_error_not_a_result():
    lib = _lib.load()
    kmax, cmax = int(lib.cgv_ensemble_check_max_samples()), int(lib.cgv_ensemble_check_max_classes())
    assert kmax >= 256
    _names, gen, z, bonds, _want = R.cases()
    n = gen.shape[1]
    plan = ev.QualityPlan(z, [0, n], DEV)
    with pytest.raises(ValueError, match="samples"):
        ev.ensemble_check(torch.zeros((kmax + 1) * n, 3, device=DEV), kmax + 1, plan, bonds)
    bl = ev.BondList(bonds, plan)
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    g = torch.from_numpy(gen[0]).to(DEV)

    def call(K, T):
        _lib.call("cgv_ensemble_check", _lib.ptr(g), _lib.ptr(plan.frame_ptr), _lib.ptr(plan.cls), _lib.ptr(plan.heavy),
                  _lib.ptr(plan.thr_sq), _lib.ptr(bl.bond_ptr), _lib.ptr(bl.bonds), 1, n, K, T, n, bl.n_bonds, _lib.ptr(counts),
                  _lib.ptr(sums), _lib.stream_ptr())
    with pytest.raises(RuntimeError, match="max_samples"):           # refused before anything is written or launched
        call(kmax + 1, plan.n_classes)
    with pytest.raises(RuntimeError, match="max_classes"):
        call(1, cmax + 1)
    call(1, plan.n_classes)
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 0, 0]


# ----------------------------------------------------------------------------- backmap vs sample_ensemble
def _setup(workload, F, n_frames, seed=11):
    w = cg.data.WORKLOADS[workload]
    ds = cg.CGDataset(cg.data.synthetic_frames(n_frames, w["n_atoms"], w["n_cgs"], w["box"], seed=seed))
    ds.generate_neighbor_list(w["atom_cutoff"], w["cg_cutoff"], device=DEV, undirected=True)
    enc, dec = (2, 9) if workload == "chignolin" else (w["enc_nconv"], w["dec_nconv"])
    model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], enc, dec, w["n_cgs"], seed=123).to(DEV)
    return w, ds, model


def _beads(ds):
    return torch.stack(ds.props["CG_nxyz"])[:, :, 1:].numpy().copy()


@pytest.mark.parametrize("workload,F,n_frames,K", [("dipeptide", 64, 5, 4), ("chignolin", 600, 2, 3)])
def test_backmap_equals_sample_ensemble_bit_for_bit(workload, F, n_frames, K):
    w, ds, model = _setup(workload, F, n_frames)
    eps = torch.randn(n_frames * K * w["n_cgs"], F, generator=torch.Generator().manual_seed(5))
    want = ev.sample_ensemble(ds, model, K, eps=eps, frames_per_launch=2, graph_eval=False)[0]
    out = bm.backmap(model, _beads(ds), ds.props["CG_mapping"][0], K, w["cg_cutoff"], eps=eps, frames_per_launch=2)
    assert out["xyz"].shape == (n_frames, K, w["n_atoms"], 3) and out["xyz"].dtype == np.float32
    assert out["xyz"].reshape(want.shape).tobytes() == want.tobytes()
    assert "counts" not in out and "diversity_heavy" not in out and np.isfinite(out["diversity_all"]).all()
    assert np.array_equal(out["cg_xyz"], _beads(ds))


def test_bead_means_rigid_motion_and_checks():
    w, ds, model = _setup("dipeptide", 64, 4)
    K, n, N = 5, w["n_atoms"], w["n_cgs"]
    mapping = ds.props["CG_mapping"][0]
    z = ds.props["nxyz"][0][:, 0].numpy().astype(np.int64)
    bonds = ds.props["bond_edge_list"][0].numpy()
    eps = torch.randn(4 * K * N, 64, generator=torch.Generator().manual_seed(2))
    beads = _beads(ds)
    kw = dict(z=z, bonds=bonds, eps=eps, radii=FILL, frames_per_launch=3)
    out = bm.backmap(model, beads, mapping, K, w["cg_cutoff"], **kw)
    scale = np.abs(beads).max()
    onehot = np.zeros((N, n))
    onehot[mapping.numpy(), np.arange(n)] = 1.0
    means = np.einsum("bn,tknd->tkbd", onehot / onehot.sum(1, keepdims=True), out["xyz"].astype(np.float64))
    print("bead-mean error / scale", np.abs(means - beads[:, None]).max() / scale)
    assert np.abs(means - beads[:, None]).max() <= REL * scale
    # the checks are K14 on the generated structures
    want_counts, want_sums = R.restate(out["xyz"].reshape(-1, 3), np.tile(z, 4), np.arange(5) * n, K, bonds, radii=FILL)
    assert np.array_equal(out["counts"], want_counts.numpy())
    assert np.array_equal(out["valid_all"], (want_counts[..., 0] + want_counts[..., 1] == 0).numpy())
    np.testing.assert_allclose(out["pair_rmsd_all"], np.sqrt(want_sums[..., 0].numpy() / n), rtol=1e-9)
    # a rigid motion of the beads moves the structures with it
    Rm = cg.data.random_rotation_matrices(1, torch.Generator().manual_seed(3))[0].double().numpy()
    t = np.array([1.5, -2.0, 0.7])
    moved = bm.backmap(model, (beads.astype(np.float64) @ Rm.T + t).astype(np.float32), mapping, K, w["cg_cutoff"], **kw)
    want_xyz = out["xyz"].astype(np.float64) @ Rm.T + t
    err = np.abs(moved["xyz"] - want_xyz).max() / np.abs(want_xyz).max()
    drift = np.abs(moved["pair_rmsd_all"] - out["pair_rmsd_all"]).max() / out["pair_rmsd_all"].max()
    print("rigid motion: xyz", err, "pair rmsd", drift)
    assert err <= REL and drift <= REL
    assert np.array_equal(moved["counts"], out["counts"])


# ----------------------------------------------------------------------------- CLI
def _write_run(tmp_path, w, model, mapping, **over):
    d = tmp_path / "run"
    d.mkdir()
    params = {"n_basis": model.encoder.n_atom_basis, "n_rbf": w["n_rbf"], "atom_cutoff": w["atom_cutoff"], "cg_cutoff": w["cg_cutoff"],
              "enc_nconv": len(model.prior_net.message_blocks), "dec_nconv": len(model.equivaraintconv.message_blocks),
              "n_cgs": w["n_cgs"], "activation": "swish", "det": False, "invariantdec": False, "cg_mp": False,
              "cg_radius_graph": False, "synthetic": True, "mapping": mapping.tolist(), **over}
    (d / "modelparams.json").write_text(json.dumps(params))
    torch.save(model.state_dict(), d / "model.pt")
    return d


def test_cli_seed_reproduces_the_file_and_another_seed_does_not(tmp_path, capsys):
    w, ds, model = _setup("dipeptide", 64, 3)
    d = _write_run(tmp_path, w, model, ds.props["CG_mapping"][0])
    np.savez(tmp_path / "cg.npz", cg_xyz=_beads(ds))
    outs = []
    for name, seed in (("a", 7), ("b", 7), ("c", 8)):
        bm.main(f"-model {d} -cg {tmp_path / 'cg.npz'} -n_samples 4 -out {tmp_path / name}.npz -seed {seed} --pair_rmsd".split())
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["frames"] == 3 and line["samples"] == 12 and line["valid_all_ratio"] is None
        with np.load(tmp_path / f"{name}.npz") as f:
            outs.append({k: f[k] for k in f.files})
    assert set(outs[0]) == {"xyz", "cg_xyz", "diversity_all", "pair_rmsd_all", "mapping", "n_samples", "seed"}
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes() or k == "seed" and outs[0][k] == outs[1][k], k
    assert not np.array_equal(outs[0]["xyz"], outs[2]["xyz"])
    # what the file holds is what the library call gives for that seed, and load_run gives the saved model back
    loaded, params = bm.load_run(str(d), DEV)
    for (ka, a), (kb, b) in zip(sorted(model.state_dict().items()), sorted(loaded.state_dict().items())):
        assert ka == kb and torch.equal(a, b)
    ops.set_sample_rng_state(DEV, torch.tensor([ops.sample_seed(7), 0, 0]))
    direct = bm.backmap(loaded, _beads(ds), params["mapping"], 4, params["cg_cutoff"])
    assert direct["xyz"].tobytes() == outs[0]["xyz"].tobytes()


def test_require_valid_keeps_valid_samples_and_leaves_full_frames_alone():
    """The topology is chosen so that some draws fail: no bonds at all, and one radius for every element such that about
    half of a first draw's samples have a pair of atoms closer than the cutoff (an extra bond)."""
    w, ds, model = _setup("dipeptide", 64, 6)
    K, n = 4, w["n_atoms"]
    mapping, beads = ds.props["CG_mapping"][0], _beads(ds)
    z = ds.props["nxyz"][0][:, 0].numpy().astype(np.int64)
    none = np.zeros((0, 2), np.int64)
    state = ops.get_sample_rng_state(DEV)
    # (the same chunking as below: the device generator advances per launch, so the noise depends on frames_per_launch)
    probe = bm.backmap(model, beads, mapping, K, w["cg_cutoff"], frames_per_launch=4)["xyz"].astype(np.float64)
    d = np.linalg.norm(probe[:, :, :, None] - probe[:, :, None], axis=-1) + 1e9 * np.eye(n)
    radius = float(np.median(d.min(axis=(2, 3)))) / (2 * 1.3)
    radii = {int(e): radius for e in range(1, 9)}
    kw = dict(z=z, bonds=none, radii=radii, frames_per_launch=4)
    ops.set_sample_rng_state(DEV, state)
    first = bm.backmap(model, beads, mapping, K, w["cg_cutoff"], **kw)
    assert first["xyz"].tobytes() == probe.astype(np.float32).tobytes()
    nv0 = first["valid_all"].sum(1)
    print("valid after the first draw", nv0.tolist())
    assert 0 < nv0.sum() < nv0.size * K                              # some draws fail, some do not
    ops.set_sample_rng_state(DEV, state)
    out = bm.backmap_valid(model, beads, mapping, K, w["cg_cutoff"], which="all", max_rounds=3, **kw)
    hist = out["n_valid_rounds"]
    print("n_valid per round", hist.tolist())
    assert np.array_equal(hist[0], nv0) and (np.diff(hist, axis=0) >= 0).all() and np.array_equal(hist[-1], out["n_valid"])
    assert 2 <= len(hist) <= 4 and (hist <= K).all()                 # some frame was short: at least one redraw round ran
    for t in range(6):
        nv = int(out["n_valid"][t])
        assert out["valid_all"][t, :nv].all() and not out["valid_all"][t, nv:].any()     # kept ones valid, fill flagged
        keep0 = first["xyz"][t][first["valid_all"][t]]
        assert np.array_equal(out["xyz"][t, :len(keep0)], keep0)                          # draw order; full frames untouched
    assert out["counts"].shape == (6, K, 4) and out["xyz"].shape == (6, K, n, 3)
    ops.set_sample_rng_state(DEV, state)


def test_end_to_end_run_ala_then_backmap_cli(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    run_ala.main("-logdir run -device 0 -dataset dipeptide -n_cgs 3 -batch_size 8 -ndata 24 -nepochs 1 -atom_cutoff 8.5 "
                 "-cg_cutoff 9.5 -beta 0.05 -gamma 25.0 -dec_nconv 2 -enc_nconv 2 -lr 0.001 -n_basis 64 -n_rbf 8 -n_ensemble 2 "
                 "--synthetic".split())
    capsys.readouterr()
    logdir = next(tmp_path.glob("run_*_N3"))
    fr = cg.data.synthetic_frames(5, 22, 3, 6.0, seed=4)
    np.savez(tmp_path / "traj.npz", xyz=torch.stack(fr["nxyz"])[:, :, 1:].numpy(), z=fr["nxyz"][0][:, 0].numpy().astype(np.int64),
             bonds=fr["bond_edge_list"][0].numpy()[:, ::-1])
    T, K, n = 5, 3, 22
    bm.main(f"-model {logdir} -traj {tmp_path / 'traj.npz'} -n_samples {K} -out {tmp_path / 'out.npz'} -frames_per_launch 2 "
            "--pair_rmsd --require_valid heavy -max_rounds 1".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == T and line["samples"] == T * K and line["seconds"] > 0 and line["samples_per_s"] > 0
    assert 0.0 <= line["valid_all_ratio"] <= 1.0 and 0.0 <= line["valid_heavy_ratio"] <= 1.0 and line["diversity_all"] > 0
    with np.load(tmp_path / "out.npz") as f:
        shapes = {k: f[k].shape for k in f.files}
        assert f["xyz"].dtype == np.float32 and f["valid_all"].dtype == bool and int(f["n_samples"]) == K and int(f["seed"]) == 0
        want_cg = np.stack([np.stack([fr["nxyz"][t][fr["CG_mapping"][0] == b, 1:].numpy().mean(0) for b in range(3)]) for t in range(T)])
        np.testing.assert_allclose(f["cg_xyz"], want_cg, rtol=1e-5, atol=1e-5)
    assert shapes == {"xyz": (T, K, n, 3), "cg_xyz": (T, 3, 3), "valid_all": (T, K), "valid_heavy": (T, K), "counts": (T, K, 4),
                      "diversity_all": (T,), "diversity_heavy": (T,), "pair_rmsd_all": (T, K, K), "pair_rmsd_heavy": (T, K, K),
                      "n_valid": (T,), "mapping": (n,), "n_samples": (), "seed": ()}


# ----------------------------------------------------------------------------- next to a running trainer
def test_backmap_then_step_continues_the_run_bit_for_bit():
    w = cg.data.WORKLOADS["dipeptide"]
    losses = []
    for with_backmap in (False, True):
        torch.manual_seed(7)
        ops.reseed_sample_rng(DEV)
        _w, ds, model = _setup("dipeptide", 32, 12)
        tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"])
        batches = [cg.prepare_batch(cg.CG_collate([ds[i] for i in range(s, s + 4)]), DEV, edge_slack=0.25) for s in (0, 4)]
        tr.step(batches[0])
        tr.step(batches[1])
        if with_backmap:
            state = ops.get_sample_rng_state(DEV)
            out = bm.backmap(model, _beads(ds)[8:], ds.props["CG_mapping"][0], 3, w["cg_cutoff"],
                             z=ds.props["nxyz"][0][:, 0].numpy().astype(np.int64), bonds=ds.props["bond_edge_list"][0].numpy(), radii=FILL)
            assert np.isfinite(out["xyz"]).all() and model.training
            ops.set_sample_rng_state(DEV, state)
        after = [float(tr.step(batches[k % 2]).clone()) for k in range(3)]
        assert all(np.isfinite(after))
        losses.append(after)
    assert losses[0] == losses[1], losses
