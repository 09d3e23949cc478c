"""run_ala.py flag surface (reference scripts/run_ala.py:419-461) and an end-to-end CLI run."""
import json

import pytest

from coarsegrainingvae_amd import run_ala

# name -> (type, default) exactly as the reference declares them
REFERENCE_FLAGS = {
    "logdir": (str, None), "n_cgs": (int, None), "lr": (float, 2e-4), "dataset": (str, "dipeptide"),
    "n_basis": (int, 512), "n_rbf": (int, 10), "activation": (str, "swish"), "cg_method": (str, "minimal"),
    "atom_cutoff": (float, 4.0), "optimizer": (str, "adam"), "cg_cutoff": (float, 4.0), "enc_nconv": (int, 4),
    "dec_nconv": (int, 4), "batch_size": (int, 64), "nepochs": (int, 2), "ndata": (int, 200), "nsamples": (int, 200),
    "n_ensemble": (int, 16), "nevals": (int, 36), "edgeorder": (int, 2), "auxcutoff": (float, 0.0),
    "beta": (float, 0.001), "gamma": (float, 0.01), "eta": (float, 0.01), "kappa": (float, 0.01),
    "threshold": (float, 1e-3), "nsplits": (int, 5), "patience": (int, 5), "factor": (float, 0.6),
    "mapshuffle": (float, 0.0), "cgae_reg_weight": (float, 0.25),
}
STORE_TRUE = ["cross", "graph_eval", "shuffle", "cg_mp", "tqdm_flag", "det", "cg_radius_graph", "invariantdec",
              "reflectiontest"]


def test_flag_surface_matches_reference():
    parser = run_ala.build_parser()
    actions = {a.dest: a for a in parser._actions if a.dest != "help"}
    for name, (typ, default) in REFERENCE_FLAGS.items():
        a = actions[name]
        assert a.option_strings == ["-" + name], name            # single-dash long options
        assert a.type is typ and a.default == default, name
    for name in STORE_TRUE:
        a = actions[name]
        assert a.option_strings == ["--" + name] and a.default is False and a.const is True
    assert actions["dec_type"].default == "EquivariantDecoder"
    assert "device" in actions and "synthetic" in actions and "no_hip_graph" in actions and "traj" in actions     # this build's own switches
    assert len(actions) == len(REFERENCE_FLAGS) + len(STORE_TRUE) + 5
    # the two documented experiments parse (README.md:57-65)
    ns = parser.parse_args("-logdir x -device 0 -dataset chignolin -n_cgs 6 -batch_size 2 -ndata 5000 -nepochs 100 "
                           "-atom_cutoff 12.0 -cg_cutoff 25.0 -nsplits 5 -beta 0.05 -gamma 50.0 -eta 0.0 -kappa 0.0 "
                           "-activation swish -dec_nconv 9 -enc_nconv 2 -lr 0.0001 -n_basis 600 -n_rbf 10 "
                           "-cg_method cgae --graph_eval -n_ensemble 8 -factor 0.3 -patience 14".split())
    assert ns.n_basis == 600 and ns.graph_eval and ns.dec_nconv == 9


def test_logdir_naming():
    p = vars(run_ala.build_parser().parse_args("-logdir job -n_cgs 3 -ndata 50 --det --cross".split()))
    name = run_ala.resolve_logdir(p)
    assert name.startswith("job_") and name.endswith("_minimal_recon_ndata50_N3_cross")   # utils.py:22-24


@pytest.mark.gpu
def test_cli_trains_on_synthetic_frames(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    run_ala.main("-logdir run -device 0 -dataset dipeptide -n_cgs 3 -batch_size 8 -ndata 48 -nepochs 3 "
                 "-atom_cutoff 8.5 -cg_cutoff 9.5 -beta 0.05 -gamma 25.0 -dec_nconv 2 -enc_nconv 2 -lr 0.001 "
                 "-n_basis 32 -n_rbf 8 --synthetic".split())
    out = capsys.readouterr().out.strip().splitlines()
    summary = json.loads(out[-1])
    assert summary["epochs"] == 3 and not summary["failed"] and summary["skipped_steps"] == 0
    assert summary["final"]["train_loss"] == summary["final"]["train_loss"]            # not NaN
    logs = list(tmp_path.glob("run_*_N3/train_log.csv"))
    assert logs and logs[0].read_text().splitlines()[0].startswith("epoch,lr,train_loss,val_loss")
    assert list(tmp_path.glob("run_*_N3/model.pt"))


def test_trajectory_converter_round_trip(tmp_path):
    """tools/traj_to_npz.py: multi-frame .xyz -> the .npz the CLI reads (frames, atomic numbers, inferred bonds)."""
    import importlib.util
    import os
    import numpy as np
    spec = importlib.util.spec_from_file_location("traj_to_npz", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "traj_to_npz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(0)
    base = np.array([[0.0, 0, 0], [1.09, 0, 0], [1.8, 1.2, 0], [3.0, 1.4, 0]])              # H-C-C-O chain
    sym, frames = ["H", "C", "C", "O"], []
    for _ in range(3):
        frames.append(base + 0.01 * rng.standard_normal(base.shape))
    text = ""
    for fr in frames:
        text += "4\ncomment\n" + "".join(f"{s} {x:.5f} {y:.5f} {z:.5f}\n" for s, (x, y, z) in zip(sym, fr))
    (tmp_path / "t.xyz").write_text(text)
    mod.main([str(tmp_path / "t.xyz"), str(tmp_path / "t.npz")])
    with np.load(tmp_path / "t.npz") as f:
        assert f["xyz"].shape == (3, 4, 3) and f["z"].tolist() == [1, 6, 6, 8]
        assert np.allclose(f["xyz"], np.asarray(frames), atol=1e-4)
        assert sorted(map(tuple, f["bonds"].tolist())) == [(0, 1), (1, 2), (2, 3)]


@pytest.mark.gpu
def test_cli_trains_on_a_trajectory_file(tmp_path, capsys, monkeypatch):
    """``-traj file.npz``: the non-synthetic branch (run_ala.py:124-181) -- frames from a file through the on-device
    ``build_dataset`` (rotation, bead means, higher-order bond edges, batched radius graphs) into the training loop."""
    import numpy as np
    rng = np.random.default_rng(1)
    n, T = 22, 40
    base = np.cumsum(rng.standard_normal((n, 3)) * 0.9, axis=0)                    # a chain-like conformation
    xyz = (base[None] + 0.15 * rng.standard_normal((T, n, 3))).astype(np.float32)
    bonds = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    mapping = (np.arange(n) * 3) // n
    np.savez(tmp_path / "traj.npz", xyz=xyz, z=rng.integers(1, 9, n), bonds=bonds, mapping=mapping)
    monkeypatch.chdir(tmp_path)
    run_ala.main(f"-logdir run -device 0 -traj {tmp_path / 'traj.npz'} -n_cgs 3 -batch_size 8 -ndata 40 -nepochs 3 "
                 "-atom_cutoff 8.5 -cg_cutoff 9.5 -beta 0.05 -gamma 25.0 -dec_nconv 2 -enc_nconv 2 -lr 0.001 "
                 "-n_basis 32 -n_rbf 8 -edgeorder 2".split())
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["epochs"] == 3 and not summary["failed"] and summary["skipped_steps"] == 0
    assert summary["final"]["train_loss"] == summary["final"]["train_loss"] and summary["graph_replays"] > 0


@pytest.mark.gpu
def test_cli_optimizer_sgd_runs_through_the_fused_step(tmp_path, capsys, monkeypatch):
    """``-optimizer sgd`` (scripts/run_ala.py:43): plain SGD through the fused clip / skip machinery (cgv_sgd_apply), captured."""
    monkeypatch.chdir(tmp_path)
    run_ala.main("-logdir run -device 0 -dataset dipeptide -n_cgs 3 -batch_size 8 -ndata 40 -nepochs 2 -atom_cutoff 8.5 "
                 "-cg_cutoff 9.5 -beta 0.05 -gamma 25.0 -dec_nconv 2 -enc_nconv 2 -lr 0.01 -n_basis 32 -n_rbf 8 -optimizer sgd --synthetic".split())
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["epochs"] == 2 and not summary["failed"] and summary["graph_replays"] > 0


# ----------------------------------------------------------------------------- every post-evaluation analysis at once
# -edgeorder 1: the frames' bond list is the molecule's bonds alone, which is what finds the peptide backbone for --kde_eval
ALL_SWITCHES_TRAIN = ("-device 0 -n_cgs 4 -ndata 64 -atom_cutoff 8.5 -cg_cutoff 9.5 -beta 0.05 -gamma 25.0 -lr 0.001 -edgeorder 1 "
                      "-n_basis 32 -n_rbf 8 -enc_nconv 2 -dec_nconv 2 -nepochs 1 -batch_size 8 -n_ensemble 4")


@pytest.fixture(scope="module")
def all_switches_run(tmp_path_factory):
    """``run_ala.main`` once, with all six ``--*_eval`` switches, on 64 frames of the three-residue peptide of
    ``density_restatement`` (phi and psi narrow enough for a torsion's kernel to stay below period / 12 on the seven
    hold-out frames): ``(run directory, trajectory file, summary line)``."""
    import contextlib
    import io
    import math
    import numpy as np
    import density_restatement as R
    from coarsegrainingvae_amd.analyses import ANALYSES
    tmp = tmp_path_factory.mktemp("all_switches")
    rng = np.random.default_rng(11)
    torsions = np.full((64, 10), math.pi)                                 # omega_0, (phi, psi, omega) per residue
    torsions[:, 1::3], torsions[:, 2::3] = rng.normal(-1.2, 0.25, (64, 3)), rng.normal(2.4, 0.25, (64, 3))
    z, bonds = R.peptide(3)
    np.savez(tmp / "traj.npz", xyz=R.peptide_structures(3, torsions), z=z, bonds=bonds, mapping=np.arange(z.shape[0]) * 4 // z.shape[0])
    switches = " ".join(f"--{a.stem}_eval" for a in ANALYSES)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        run_ala.main(f"-logdir {tmp / 'run'} -traj {tmp / 'traj.npz'} {ALL_SWITCHES_TRAIN} -tica_lag 5 {switches}".split())
    return next(tmp.glob("run_*_N4")), tmp / "traj.npz", json.loads(out.getvalue().strip().splitlines()[-1])


def _stats_keys():
    from coarsegrainingvae_amd import contacts, coverage, density, distributions, flexibility, tica
    return {"dist": distributions.DIST_STATS_KEYS, "tica": tica.TICA_STATS_KEYS, "cov": coverage.COV_STATS_KEYS,
            "contact": contacts.CONTACT_STATS_KEYS, "flex": flexibility.FLEX_STATS_KEYS, "kde": density.KDE_STATS_KEYS}


@pytest.mark.gpu
def test_run_ala_with_every_eval_switch_writes_six_files_and_places_six_summaries(all_switches_run):
    from coarsegrainingvae_amd.analyses import ANALYSES
    logdir, _traj, summary = all_switches_run
    assert not summary["failed"] and summary["epochs"] == 1
    for a in ANALYSES:
        key = a.stem + "_stats"
        stats = json.loads((logdir / (key + ".json")).read_text())
        assert set(stats) == set(_stats_keys()[a.stem]), a.stem
        top = a.stem in ("dist", "tica", "cov")                          # the others stay under "test_stats"
        assert (key in summary) == top and (key in summary["test_stats"]) == (not top), a.stem
        assert (summary if top else summary["test_stats"])[key] == a.module.summary_of(stats), a.stem
    stored = json.loads((logdir / "modelparams.json").read_text())
    assert all(stored[a.stem + "_eval"] is True for a in ANALYSES) and stored["tica_lag"] == 5


@pytest.mark.gpu
def test_backmap_with_every_stats_switch_writes_six_files_next_to_out(all_switches_run, tmp_path, capsys):
    from coarsegrainingvae_amd import backmap
    from coarsegrainingvae_amd.analyses import ANALYSES
    logdir, traj, _summary = all_switches_run
    switches = " ".join(f"--{a.stem}_stats" for a in ANALYSES)
    backmap.main(f"-model {logdir} -traj {traj} -n_samples 4 -out {tmp_path / 'out.npz'} -tica_lag 5 -kde_grid 16 {switches}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == 64 and line["samples"] == 256
    for a in ANALYSES:
        key = a.stem + "_stats"
        stats = json.loads((tmp_path / (key + ".json")).read_text())
        assert set(stats) == set(_stats_keys()[a.stem]) and stats["n_ref"] == 64, a.stem
        assert line[key] == a.module.summary_of(stats), a.stem
