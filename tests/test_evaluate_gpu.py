"""Test-time evaluation on the device: the fused metric kernel (csrc/sample_quality.hip) against the goldens recorded
from the reference and against a dense torch restatement, the batched ensemble against the reference's call pattern,
and its coexistence with a running Trainer."""
import json

import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd import evaluate as ev, ops, run_ala
from coarsegrainingvae_amd.trainer import Trainer
from test_evaluate_cpu import CASES, _golden, check_six, raw_counts_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-4            # the suite's output tolerance (tests/test_hip_parity.py)
FILL = {2: 0.68, 3: 0.68, 4: 0.68, 5: 0.68}     # synthetic frames carry type labels 1..8: radii for the untabulated ones


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def dense_restatement(ref, gen, z, frame_ptr, K, radii=None, scale=1.3):
    """get_bond_graphs / compare_graph / compute_rmsd (sampling.py:148-239) with dense [n,n] matrices in torch on the
    device, one (frame, sample) at a time: counts [B,K,6] int64 and sums [B,K,2] float64."""
    z = np.asarray(z).astype(np.int64)
    elements = sorted(set(z.tolist()))
    thr = ev.bond_thresholds(elements, scale, radii).to(DEV)
    cls = torch.from_numpy(np.searchsorted(elements, z)).to(DEV)
    heavy = torch.from_numpy(z != 1).to(DEV)

    def bonds(xyz, c):
        d = xyz[:, None, :] - xyz[None, :, :]
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        b = (s <= thr[c[:, None], c[None, :]]).long()
        b.fill_diagonal_(0)
        return b
    B = len(frame_ptr) - 1
    counts = torch.zeros(B, K, 6, dtype=torch.int64)
    sums = torch.zeros(B, K, 2, dtype=torch.float64)
    for f in range(B):
        lo, hi = int(frame_ptr[f]), int(frame_ptr[f + 1])
        n, h = hi - lo, heavy[lo:hi]
        r = ref[lo:hi]
        br = bonds(r, cls[lo:hi])
        for k in range(K):
            g = gen[K * lo + k * n:K * lo + (k + 1) * n]
            bg = bonds(g, cls[lo:hi])
            brh, bgh = br[h][:, h], bg[h][:, h]
            d2 = (g.double() - r.double()).pow(2).sum(-1)
            counts[f, k] = torch.stack([(br != bg).sum(), (brh != bgh).sum(), (br - bg).sum(), (brh - bgh).sum(), br.sum(), brh.sum()]).cpu()
            sums[f, k] = torch.stack([d2.sum(), d2[h].sum()]).cpu()
    return counts, sums


# ----------------------------------------------------------------------------- kernel vs the reference's goldens
@pytest.mark.parametrize("case", CASES)
def test_kernel_matches_the_reference_on_every_golden(case):
    """The bond matrices of a golden belong to the thresholds recorded with it: ``sqrt(s) < cutoff`` is evaluated with the
    recording host's fp32 sqrt, and hosts disagree in the last bit (same torch build: sqrt(3.1258237) is 1.7679999 on
    one, 1.768 on another) -- the `ulp` case sits exactly there.  The kernel takes the table as an argument."""
    g = _golden(case)
    K, n = g["gen"].shape[0], g["ref"].shape[0]
    raw = ev.sample_quality(torch.from_numpy(g["ref"]).to(DEV), torch.from_numpy(g["gen"].reshape(K * n, 3)).to(DEV),
                            g["z"], [0, n], n_samples=K, scale=float(g["scale"]), thresholds=g["thr.sq"])
    assert raw.counts.dtype == torch.int32 and raw.sums.dtype == torch.float64 and raw.counts.is_cuda
    counts, sums = raw.counts.cpu().numpy()[0], raw.sums.cpu().numpy()[0]
    want_counts, want_sums = raw_counts_from_golden(g)
    assert counts.tolist() == want_counts.tolist()                       # all six integer outputs, every sample
    np.testing.assert_allclose(sums, want_sums, rtol=1e-10, atol=0)
    six = ev.assemble_sample_qualities(counts, sums, n, int((g["z"] != 1).sum()))
    check_six(six, g, rel=1e-10)                                         # valid id sets, RMSD rows, ratios
    assert np.nonzero(counts[:, ev.DIFF_ALL] == 0)[0].tolist() == np.nonzero(g["diff.all"] == 0)[0].tolist()
    assert np.nonzero(counts[:, ev.DIFF_HEAVY] == 0)[0].tolist() == np.nonzero(g["diff.heavy"] == 0)[0].tolist()
    # the public one-frame entry point gives the same tuple
    check_six(ev.eval_sample_qualities(g["ref"], g["gen"], g["z"], scale=float(g["scale"]), thresholds=g["thr.sq"]), g, rel=1e-10)


def test_frames_of_different_sizes_and_a_2000_atom_frame_in_one_launch():
    """20-atom and 10-atom golden frames next to a 2000-atom frame (528 tile pairs per sample), two samples each:
    integers equal a dense torch restatement exactly, and the golden frames keep the reference's counts."""
    K = 2
    ga, gb = _golden("mixed_all"), _golden("no_hydrogen")
    big = cg.synthetic_batch("protein2000", n_frames=1, seed=3, device=DEV)
    xyz_big = big["_graph"].xyz
    z_big = big["nxyz"][:, 0].cpu().numpy().astype(np.int64)
    gen_big = xyz_big[None] + 0.08 * torch.randn(K, *xyz_big.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    ref = torch.cat([torch.from_numpy(ga["ref"]).to(DEV), torch.from_numpy(gb["ref"]).to(DEV), xyz_big])
    gen = torch.cat([torch.from_numpy(ga["gen"][:K].reshape(-1, 3)).to(DEV), torch.from_numpy(gb["gen"][:K].reshape(-1, 3)).to(DEV),
                     gen_big.reshape(-1, 3)])
    z = np.concatenate([ga["z"], gb["z"], z_big])
    fp = [0, 20, 30, 2030]
    raw = ev.sample_quality(ref, gen, z, fp, n_samples=K, radii=FILL)
    want_counts, want_sums = dense_restatement(ref, gen, z, fp, K, radii=FILL)
    counts = raw.counts.cpu().long()
    assert torch.equal(counts, want_counts)
    assert int(want_counts[2, :, ev.REFSUM_ALL].min()) > 0 and int(want_counts[2, :, ev.DIFF_ALL].min()) > 0   # not vacuous
    np.testing.assert_allclose(raw.sums.cpu().numpy(), want_sums.numpy(), rtol=1e-10, atol=0)
    for f, g in enumerate((ga, gb)):
        assert counts[f].tolist() == raw_counts_from_golden(g)[0][:K].tolist()
    # bitwise reproducible, fp64 sums included
    again = ev.sample_quality(ref, gen, z, fp, n_samples=K, radii=FILL)
    assert torch.equal(again.counts, raw.counts) and torch.equal(again.sums, raw.sums)


# ----------------------------------------------------------------------------- batched ensemble
def _setup(workload, F, n_frames, seed=11):
    w = cg.data.WORKLOADS[workload]
    ds = cg.CGDataset(cg.data.synthetic_frames(n_frames, w["n_atoms"], w["n_cgs"], w["box"], seed=seed))
    ds.generate_neighbor_list(w["atom_cutoff"], w["cg_cutoff"], device=DEV, undirected=True)
    enc, dec = (2, 9) if workload == "chignolin" else (w["enc_nconv"], w["dec_nconv"])
    model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], enc, dec, w["n_cgs"], seed=123).to(DEV)
    return w, ds, model


@pytest.mark.parametrize("workload,F,n_frames,K", [("dipeptide", 64, 5, 4), ("chignolin", 600, 2, 3)])
def test_batched_ensemble_equals_the_reference_call_pattern(workload, F, n_frames, K):
    """With ``eps`` supplied, ``sample_xyzs`` equal K separate ``model.decoder(cg_xyz, CG_nbr_list, H, H, mapping,
    num_CGs)`` calls on each single frame (sampling.py:265-282); chunking does not change the metrics."""
    w, ds, model = _setup(workload, F, n_frames)
    eps = torch.randn(n_frames * K * w["n_cgs"], F, generator=torch.Generator().manual_seed(5))
    out = ev.sample_ensemble(ds, model, K, eps=eps, frames_per_launch=2, radii=FILL)
    assert out[0].shape == (n_frames, K * w["n_atoms"], 3) and out[1].shape == (n_frames, w["n_atoms"], 3)
    assert out[2].shape == (n_frames, w["n_cgs"], 3) and out[3].shape == (n_frames, w["n_atoms"], 3)
    e = eps.reshape(n_frames, K, w["n_cgs"], F).to(DEV)
    with torch.no_grad():
        for f in range(n_frames):
            batch = cg.batch_to(cg.CG_collate([ds[f]]), DEV)
            z, cg_z, xyz, cg_xyz, nbr_list, CG_nbr_list, mapping, num_CGs = model.get_inputs(batch)
            H_mu, H_sigma = model.prior_net(cg_z, cg_xyz, CG_nbr_list)
            for k in range(K):
                H = e[f, k].mul(H_sigma).add_(H_mu)
                xyz_decode = model.decoder(cg_xyz, CG_nbr_list, H, H, mapping, num_CGs)
                got = out[0][f][k * w["n_atoms"]:(k + 1) * w["n_atoms"]]
                assert rel_err(got, xyz_decode) <= REL, (f, k, rel_err(got, xyz_decode))
            assert np.array_equal(out[1][f], xyz.cpu().numpy()) and np.array_equal(out[2][f], cg_xyz.cpu().numpy())
    assert len(out[6]) == n_frames and len(out[8]) == n_frames and len(out[8][0]) == K
    other = ev.sample_ensemble(ds, model, K, eps=eps, frames_per_launch=n_frames, radii=FILL)
    assert np.array_equal(other[0], out[0])
    for a, b in zip(out[4:], other[4:]):
        assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    no_eval = ev.sample_ensemble(ds, model, K, eps=eps, graph_eval=False, radii=FILL)
    assert no_eval[4:] == (None,) * 6 and np.array_equal(no_eval[0], out[0])


def test_device_drawn_noise_is_reproducible_and_differs_between_samples():
    w, ds, model = _setup("dipeptide", 64, 3)
    K = 4
    state = ops.get_sample_rng_state(DEV)
    a = ev.sample_ensemble(ds, model, K, radii=FILL)
    ops.set_sample_rng_state(DEV, state)
    b = ev.sample_ensemble(ds, model, K, radii=FILL)
    assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
    samples = a[0].reshape(3, K, w["n_atoms"], 3)
    for f in range(3):
        for i in range(K):
            for j in range(i + 1, K):
                assert not np.array_equal(samples[f, i], samples[f, j])


def test_reflection_mirrors_copies_and_keeps_the_metrics_of_a_mirrored_pair():
    """Kernel level: a mirrored sample against its mirrored frame has the counts and sums of the unmirrored pair.
    Ensemble level: ``reflection=True`` evaluates the mirrored frames and leaves the caller's dataset alone."""
    g = _golden("mixed_heavy")
    K, n = g["gen"].shape[0], g["ref"].shape[0]
    flip = np.array([1.0, -1.0, 1.0], dtype=np.float32)
    plain = ev.sample_quality(torch.from_numpy(g["ref"]).to(DEV), torch.from_numpy(g["gen"].reshape(-1, 3)).to(DEV), g["z"], [0, n], K)
    mirr = ev.sample_quality(torch.from_numpy(g["ref"] * flip).to(DEV), torch.from_numpy((g["gen"] * flip).reshape(-1, 3)).to(DEV),
                             g["z"], [0, n], K)
    assert torch.equal(plain.counts, mirr.counts) and torch.equal(plain.sums, mirr.sums)
    w, ds, model = _setup("dipeptide", 64, 3)
    before = [{k: v.clone() for k, v in ds[i].items() if torch.is_tensor(v)} for i in range(3)]
    eps = torch.randn(3 * 2 * w["n_cgs"], 64, generator=torch.Generator().manual_seed(9))
    out = ev.sample_ensemble(ds, model, 2, eps=eps, reflection=True, radii=FILL)
    for i in range(3):
        for k, v in before[i].items():
            assert torch.equal(ds[i][k], v), k
        want = before[i]["nxyz"][:, 1:].numpy() * flip
        assert np.array_equal(out[1][i], want)
        assert np.array_equal(out[2][i], before[i]["CG_nxyz"][:, 1:].numpy() * flip)
    batch = cg.prepare_batch(cg.CG_collate([ds[i] for i in range(3)]), DEV)
    keep = batch["nxyz"].clone()
    rq = ev.reconstruction_quality([batch], model, reflection=True, radii=FILL)
    assert torch.equal(batch["nxyz"], keep) and np.array_equal(rq[0], keep[:, 1:].cpu().numpy() * flip)


def test_reconstruction_quality_equals_a_dense_restatement():
    w, ds, model = _setup("dipeptide", 64, 6)
    batches = [cg.CG_collate([ds[i] for i in range(0, 4)]), cg.prepare_batch(cg.CG_collate([ds[4], ds[5]]), DEV)]
    model.train()
    true_xyz, recon_xyz, cg_xyz, all_valid, heavy_valid, all_ged, heavy_ged = ev.reconstruction_quality(batches, model, radii=FILL)
    assert model.training                                              # the mode found is restored
    n = w["n_atoms"]
    assert true_xyz.shape == (6 * n, 3) and recon_xyz.shape == (6 * n, 3) and cg_xyz.shape == (6 * w["n_cgs"], 3)
    z = np.concatenate([ds[i]["nxyz"][:, 0].numpy() for i in range(6)])
    fp = list(range(0, 6 * n + 1, n))
    counts, sums = dense_restatement(torch.from_numpy(true_xyz).to(DEV), torch.from_numpy(recon_xyz).to(DEV), z, fp, 1, radii=FILL)
    per_frame = [ev.assemble_sample_qualities(counts[f].numpy(), sums[f].numpy(), n, int((z[f * n:(f + 1) * n] != 1).sum())) for f in range(6)]
    want = ev.assemble_reconstruction(per_frame)
    np.testing.assert_allclose(np.array([all_valid, heavy_valid, all_ged, heavy_ged]), np.array(want), rtol=1e-12, equal_nan=True)


# ----------------------------------------------------------------------------- next to a running trainer
@pytest.mark.parametrize("captured", [False, True])
def test_evaluate_then_step_continues_the_run_bit_for_bit(captured):
    """An evaluation between two steps -- sample RNG state saved before and restored after -- leaves the next step's
    loss exactly what it is without the evaluation; eager and captured replay."""
    w = cg.data.WORKLOADS["dipeptide"]
    losses = []
    for with_eval in (False, True):
        torch.manual_seed(7)
        ops.reseed_sample_rng(DEV)
        _w, ds, model = _setup("dipeptide", 32, 12)
        tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"])
        batches = [cg.prepare_batch(cg.CG_collate([ds[i] for i in range(s, s + 4)]), DEV, edge_slack=0.25) for s in (0, 4)]
        tr.step(batches[0])
        if captured:
            tr.capture(batches[0], warmup=0)
        tr.step(batches[1])
        if with_eval:
            state = ops.get_sample_rng_state(DEV)
            out = ev.sample_ensemble([ds[i] for i in range(8, 12)], model, 3, radii=FILL)
            rq = ev.reconstruction_quality([cg.CG_collate([ds[8], ds[9]])], model, radii=FILL)
            assert np.isfinite(out[0]).all() and np.isfinite(rq[1]).all() and model.training
            ops.set_sample_rng_state(DEV, state)
        after = [float(tr.step(batches[k % 2]).clone()) for k in range(3)]
        assert all(np.isfinite(after))
        if captured:
            assert tr.replays > 0
        losses.append(after)
    assert losses[0] == losses[1], losses


# ----------------------------------------------------------------------------- CLI
CLI = ("-logdir run -device 0 -dataset dipeptide -n_cgs 3 -batch_size 8 -ndata 40 -nepochs 1 -atom_cutoff 8.5 -cg_cutoff 9.5 "
       "-beta 0.05 -gamma 25.0 -dec_nconv 2 -enc_nconv 2 -lr 0.001 -n_basis 64 -n_rbf 8 -n_ensemble 4 --synthetic")


def test_cli_writes_cv_stats_and_test_stats_with_graph_eval(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    run_ala.main((CLI + " --graph_eval").split())
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not summary["failed"] and summary["epochs"] == 1
    stats = summary["test_stats"]
    assert list(stats) == ev.CV_STATS_COLUMNS
    for key in ("sample_all_valid_ratio", "sample_heavy_valid_ratio", "recon_all_valid_ratio", "recon_heavy_valid_ratio"):
        assert 0.0 <= stats[key] <= 1.0, key
    assert stats["test_all_recon"] > 0 and stats["train_all_recon"] > 0 and stats["sample_all_ged"] is not None
    header, row = next(tmp_path.glob("run_*_N3/cv_stats.csv")).read_text().splitlines()
    assert header.split(",") == ev.CV_STATS_COLUMNS and len(row.split(",")) == len(ev.CV_STATS_COLUMNS)
    assert row.split(",")[ev.CV_STATS_COLUMNS.index("sample_all_valid_ratio")] == str(stats["sample_all_valid_ratio"])
    assert list(tmp_path.glob("run_*_N3/test_all_rmsd*.txt")) and list(tmp_path.glob("run_*_N3/test_heavy_rmsd*.txt"))
    with np.load(next(tmp_path.glob("run_*_N3/samples.npz"))) as f:
        assert f["sample_xyzs"].shape == (4, 4 * 22, 3) and f["data_xyzs"].shape == (4, 22, 3)      # 4 hold-out frames
        assert f["cg_xyzs"].shape == (4, 3, 3) and f["recon_xyzs"].shape == (4, 22, 3)


def test_cli_without_graph_eval_writes_samples_and_leaves_the_graph_columns_empty(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    run_ala.main(CLI.split())
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["test_stats"]
    header, row = next(tmp_path.glob("run_*_N3/cv_stats.csv")).read_text().splitlines()
    cells = dict(zip(header.split(","), row.split(",")))
    for key in ev.CV_STATS_COLUMNS:
        if key.startswith("sample_"):
            assert cells[key] == "" and stats[key] is None, key
    assert cells["test_all_recon"] != "" and cells["recon_all_ged"] != ""
    with np.load(next(tmp_path.glob("run_*_N3/samples.npz"))) as f:
        assert f["sample_xyzs"].shape == (4, 4 * 22, 3)
