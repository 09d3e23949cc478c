"""bench.py's plain run and ``--dump-outputs``: a plain run times exactly ``--steps`` steps and prints the headline only (the
CPU oracle, parity and the side / per-kernel figures belong to ``--full``); the dump holds what the last timed step returned,
float32, under 64 MB, and two runs with the same arguments see the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_a_plain_run_times_one_repetition_and_full_keeps_five(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.reps, a.steps, a.warmup, a.dump_outputs) == (False, 1, 7, 2, None)
    a = _args(monkeypatch, "--full")
    assert a.full and a.reps == 5
    a = _args(monkeypatch, "--full", "--reps", "3", "--dump-outputs", "out")
    assert a.reps == 3 and a.dump_outputs == "out"


def _plain_run(out):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                          "--dump-outputs", out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    runs = [str(tmp_path / "a"), str(tmp_path / "b")]
    lines = [_plain_run(d) for d in runs]
    d = lines[0]
    assert d["metric"] == "train_step_frames_per_sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 6 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert d["timing"]["repetitions"] == 1 and len(d["timing"]["ms_per_step_all"]) == 1
    assert d["config"]["graph_replays_in_timed_loops"] == 2 + 6              # warm-up + timed steps, all replays
    assert d["value"] == pytest.approx(1e3 * d["config"]["global_batch"] / d["ms_per_step"], rel=1e-9)
    assert d["parity"] is None and d["cpu_baseline"] is None and d["roofline"] is None
    assert "ms_per_step_replay_only" not in d and "scatter_add" not in d

    names = sorted(os.listdir(runs[0]))
    assert names == sorted(os.listdir(runs[1]))
    assert {"loss.npy", "kl.npy", "recon.npy", "graph.npy", "S_mu.npy", "xyz_recon.npy", "parameters_sample.npy"} <= set(names)
    total = 0
    for name in names:
        a, b = (np.load(os.path.join(r, name)) for r in runs)
        total += a.nbytes
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), name
        # same seeded batches, initial weights and noise in both runs: the results agree to fp32 summation order
        scale = max(float(np.abs(b).max()), 1e-30)
        assert float(np.abs(a - b).max()) <= 1e-4 * scale, name
    assert total <= 64 << 20
    assert float(np.load(os.path.join(runs[0], "loss.npy"))) == pytest.approx(lines[0]["loss"], rel=1e-6)
