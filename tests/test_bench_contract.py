"""bench.py: the algorithmic-byte model of SURVEY.md 8(d) and the command line the driver uses."""
import importlib.util
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_algorithmic_bytes_match_survey():
    b = _bench()
    ab = b.algorithmic_bytes(100_000, 50_000, 512)
    # c2 = 50k * 2072 + (2048 + 200k) + 100k * 340 = 137.8 MB
    assert ab["step"] == 50_000 * (4 * 512 + 24) + (4 * 512 + 4 * 50_000) + 100_000 * 340
    assert abs(ab["step"] / 1e6 - 137.8) < 0.05
    assert ab["score_codebook"] + ab["particle_update"] + ab["tail"] == ab["step"]
    c5 = b.algorithmic_bytes(10_000, 50_000, 512, B=64)
    assert abs(c5["step"] / 1e6 - 334.0) < 1.0
    assert b.PER_PARTICLE_UPDATE + b.PER_PARTICLE_TAIL == 340 and b.HBM_PEAK_GBS == 8000.0


def test_bench_refuses_to_run_without_a_gpu(monkeypatch):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0"])
    with pytest.raises(SystemExit) as e:
        b.main()
    assert "MI355X" in str(e.value)  # loud failure, no CPU fallback


def test_bench_rejects_zero_steps(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        b.main()
    assert e.value.code == 2  # argparse's usage error, before any device work


def test_dump_outputs_dtypes_budget_and_sample(tmp_path):
    """--dump-outputs' writer: float32 / float64 files, integers exact as float64; over the budget the per-particle arrays keep the
    same fixed rows (sample_rows.npy), run after run, and the files stay inside the budget."""
    import numpy as np
    import torch

    b = _bench()
    N = 1000
    arrays = {"poses": torch.arange(N * 16, dtype=torch.float32).reshape(N, 4, 4), "weights": torch.linspace(0, 1, N, dtype=torch.float64),
              "ridx": torch.arange(N, dtype=torch.int32).flip(0), "rmse": torch.tensor([1.5, 2.5], dtype=torch.float64)}
    assert b.dump_outputs(str(tmp_path / "whole"), arrays, N) == {"poses": [N, 4, 4], "weights": [N], "ridx": [N], "rmse": [2]}
    ridx = np.load(tmp_path / "whole" / "ridx.npy")
    assert ridx.dtype == np.float64 and np.array_equal(ridx, np.arange(N)[::-1])
    assert np.load(tmp_path / "whole" / "poses.npy").dtype == np.float32

    budget = 48_000
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), arrays, N, budget=budget)
    names = sorted(os.listdir(tmp_path / "s1"))
    assert names == ["poses.npy", "ridx.npy", "rmse.npy", "sample_rows.npy", "weights.npy"]
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in names) <= budget
    rows = np.load(tmp_path / "s1" / "sample_rows.npy").astype(np.int64)
    assert 0 < rows.size < N and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "s1" / "poses.npy"), arrays["poses"].numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "s1" / "ridx.npy"), N - 1 - rows)
    assert np.array_equal(np.load(tmp_path / "s1" / "rmse.npy"), [1.5, 2.5])
    for f in names:
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)), f

    b.dump_outputs(str(tmp_path / "r"), arrays, N, rank=1, world=2)
    assert sorted(os.listdir(tmp_path / "r")) == ["poses_rank1.npy", "ridx_rank1.npy", "rmse_rank1.npy", "weights_rank1.npy"]


@pytest.mark.gpu
def test_dump_outputs_repeat_bit_for_bit(tmp_path):
    """bench.py --dump-outputs twice with the same arguments: the same arrays, bit for bit, beside a line with steps and ms_per_step."""
    import json
    import subprocess

    import numpy as np

    N = 4096
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "3", "--particles", str(N),
           "--codebook", "4096", "--dim", "256", "--no-cpu-baseline", "--no-profile", "--no-loop", "--no-diffuse", "--no-extras"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    lines = []
    for d in ("a", "b"):
        r = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        js = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1, r.stdout[-2000:]
        lines.append(json.loads(js[0]))
    for line in lines:
        assert line["steps"] == 5 and line["ms_per_step"] > 0
        assert line["dump_outputs"]["arrays"] == lines[0]["dump_outputs"]["arrays"]
    shapes = lines[0]["dump_outputs"]["arrays"]
    assert shapes["poses"] == [N, 4, 4] and shapes["ridx"] == [N] and shapes["rmse"] == [2]
    for name in shapes:
        a, b_ = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), name
        assert np.array_equal(a, b_), name
    ridx = np.load(tmp_path / "a" / "ridx.npy")
    assert ridx.min() >= 0 and ridx.max() < N


@pytest.mark.gpu
def test_full_adds_side_figures_and_leaves_the_timed_steps(tmp_path):
    """A plain line carries the headline only; --full adds the passes of its own (here: the materialised-every-frame and per-step
    passes) after the timed steps, which leave what the timed steps computed as it was: the same dumped arrays, bit for bit."""
    import json
    import subprocess

    import numpy as np

    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "3", "--particles", "4096",
           "--codebook", "4096", "--dim", "256"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    lines = {}
    for tag, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-profile", "--no-loop", "--no-extras"])):
        r = subprocess.run(cmd + extra + ["--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        js = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1, r.stdout[-2000:]
        lines[tag] = json.loads(js[0])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["metric"] == "filter_steps_per_sec" and line["steps"] == 5 and line["value"] > 0 and line["ms_per_step"] > 0
    assert plain["config"]["full"] is False and full["config"]["full"] is True
    assert plain["config"]["per_step"] is None and plain["config"]["steps_per_sec_materialised_every_frame"] is None
    assert "roofline" not in plain and "cpu_baseline" not in plain and plain["config"]["reference_loop_frames_per_sec"] is None
    assert full["config"]["per_step"]["ms_per_step_median"] > 0 and full["config"]["steps_per_sec_materialised_every_frame"] > 0
    assert plain["dump_outputs"]["arrays"] == full["dump_outputs"]["arrays"]
    for name in plain["dump_outputs"]["arrays"]:
        assert np.array_equal(np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))), name
