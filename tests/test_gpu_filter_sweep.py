"""`filter_sweep` - the reference's experiment (bash/run_filter.sh: objects x logs x trials) as one batch - against its single-run
yardstick: every row's statistics are exactly those of `filter(cfg, run, seed=seed + row, start="device")`.

Three synthetic objects (K = 3000 / 900 / 1777, D = 128) x two logs each, of lengths 7, 12 and 54 (frame 50 clusters) x two
trials: B = 12 rows of 700 particles, floor 300.  The yardstick runs are made once per setting and shared."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OBJECTS = (("004_sugar_box", 3000), ("025_mug", 900), ("cotter-pin", 1777))
LOGS = ((0, 7), (1, 12), (2, 54), (0, 54), (1, 7), (2, 12))  # (object, frames) of the six runs: every object a short and a long log
D, N0, FLOOR, SEED, TRIALS = 128, 700, 300, 5200, 2
KEYS = ("rmse_t", "rmse_r", "num_particles", "cluster_poses", "cluster_stds")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cfg():
    from midastouch_amd.config import load_config
    return load_config([f"expt.params.num_particles={N0}"])


@pytest.fixture(scope="module")
def objects(dev):
    """Per object: the synthetic codebook, its tactile_tree on the device and the mesh tree every run on it shares."""
    from midastouch_amd import ops
    from midastouch_amd.synthetic import make_codebook
    from midastouch_amd.tactile_tree import tactile_tree
    out = []
    for i, (name, K) in enumerate(OBJECTS):
        cb = make_codebook(name, K=K, D=D, seed=1013 + i, mesh_points=4000)
        tt = tactile_tree(torch.as_tensor(cb.poses), torch.as_tensor(cb.cam_poses), torch.as_tensor(cb.embeddings))
        tt.to_device(dev)
        out.append((cb, tt, ops.Tree(torch.as_tensor(cb.mesh_vertices).to(dev, torch.float64))))
    return out


def _run(objects, dev, i, T, seed, log_id):
    from midastouch_amd.filter import Sequence
    from midastouch_amd.synthetic import make_trajectory
    cb, tt, mesh = objects[i]
    tr = make_trajectory(cb, T=T, seed=seed)
    return Sequence(torch.as_tensor(tr.gt_poses).to(dev), torch.as_tensor(tr.meas_poses).to(dev), torch.as_tensor(tr.codes).to(dev), tt,
                    cb.mesh_vertices, cb.obj_model, mesh_tree=mesh, log_id=log_id)


@pytest.fixture(scope="module")
def runs(objects, dev):
    return [_run(objects, dev, i, T, 2100 + r, r) for r, (i, T) in enumerate(LOGS)]


def _same(got, want, who):
    assert got["traj_size"] == want["traj_size"] == len(got["rmse_t"]), who
    for k in ("rmse_t", "rmse_r", "num_particles"):
        assert got[k] == want[k], (who, k)
    for k in ("cluster_poses", "cluster_stds"):
        assert len(got[k]) == len(want[k]), (who, k)
        for f, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == b.shape and torch.equal(a, b), (who, k, f)


def _yardstick(cfg, runs, dev, **kw):
    from midastouch_amd.filter import filter as run_filter
    return [run_filter(cfg, runs[r], device=dev, seed=SEED + r * TRIALS + k, start="device", floor=FLOOR, **kw)
            for r in range(len(runs)) for k in range(TRIALS)]


@pytest.fixture(scope="module")
def default_sweep(cfg, runs, dev):
    from midastouch_amd.filter import filter_sweep
    return filter_sweep(cfg, runs, trials=TRIALS, seed=SEED, device=dev, floor=FLOOR)


def test_sweep_rows_are_single_runs(cfg, runs, dev, default_sweep):
    want = _yardstick(cfg, runs, dev)
    assert len(default_sweep) == len(want) == 12
    for row, (got, ref) in enumerate(zip(default_sweep, want)):
        r, k = divmod(row, TRIALS)
        _same(got, ref, f"row {row}")
        assert got["traj_size"] == LOGS[r][1] and len(got["time"]) == LOGS[r][1] and all(t > 0 for t in got["time"])
        assert (got["trial_id"], got["batch_rows"], got["log_id"], got["obj_name"]) == (k, 12, f"{r:02d}", OBJECTS[LOGS[r][0]][0])
        assert got["tree_size"] == OBJECTS[LOGS[r][0]][1] and got["init_particles"] == N0 and got["init_noise"] == ref["init_noise"]
        assert set(ref) | {"batch_rows"} == set(got)
    # the settings bite: trials of one run differ, annealing moved some row's count, frame 50 clustered on the long logs
    assert default_sweep[4]["rmse_t"] != default_sweep[5]["rmse_t"]
    assert any(min(s["num_particles"]) < N0 for s in default_sweep)
    assert ref["log_id"] == "05"  # (filter() reads Sequence.log_id too)


def test_sweep_other_settings(cfg, runs, dev):
    from midastouch_amd.filter import filter_sweep
    kw = dict(cluster_every=3, update_freq=2, softmax=False)
    got = filter_sweep(cfg, runs, trials=TRIALS, seed=SEED, device=dev, floor=FLOOR, **kw)
    want = _yardstick(cfg, runs, dev, **kw)
    for row, (a, b) in enumerate(zip(got, want)):
        _same(a, b, f"row {row}")
    assert any(len(c) > 1 for s in got for c in s["cluster_poses"]) or any(min(s["num_particles"]) < N0 for s in got)


def test_sweep_wide(objects, dev):
    """B = 2 rows of 16 500 particles (beyond the small-set regime: wide=True), four frames."""
    from midastouch_amd.config import load_config
    from midastouch_amd.filter import filter as run_filter, filter_sweep
    cfg = load_config(["expt.params.num_particles=16500"])
    two = [_run(objects, dev, 1, 6, 77, 0), _run(objects, dev, 2, 6, 78, 1)]
    got = filter_sweep(cfg, two, seed=31, device=dev, max_frames=4)
    for row, seq in enumerate(two):
        want = run_filter(cfg, seq, device=dev, seed=31 + row, start="device", max_frames=4)
        _same(got[row], want, f"row {row}")
        assert got[row]["traj_size"] == 4 and got[row]["init_particles"] == 16500 and got[row]["batch_rows"] == 2


def test_surplus_frames_are_never_read(cfg, runs, dev, default_sweep, monkeypatch):
    """Rows whose logs have ended are stepped on; NaN codes in their surplus frames - a frame whose weights are all NaN sets
    condition bits in its log row - change no result of any row and raise nothing."""
    from midastouch_amd import filter as fmod
    inputs = fmod.sweep_inputs
    poisoned = []

    def poison(runs_, plan, device):
        odoms, codes, gts = inputs(runs_, plan, device)
        for row, T in enumerate(plan["lengths"]):
            codes[T:, row] = float("nan")
            poisoned.append(int(codes.shape[0] - T))
        return odoms, codes, gts

    monkeypatch.setattr(fmod, "sweep_inputs", poison)
    got = fmod.filter_sweep(cfg, runs, trials=TRIALS, seed=SEED, device=dev, floor=FLOOR)
    assert sorted(set(poisoned)) == [0, 42, 47]
    for row, (a, b) in enumerate(zip(got, default_sweep)):
        _same(a, b, f"row {row}")


def test_results_root_round_trip(cfg, runs, dev, tmp_path):
    from midastouch_amd.filter import filter_sweep
    two = [runs[0], runs[4]]
    got = filter_sweep(cfg, two, trials=2, seed=9, device=dev, floor=FLOOR, max_frames=3, results_root=str(tmp_path))
    for row, st in enumerate(got):
        r, k = divmod(row, 2)
        path = tmp_path / two[r].obj_model / st["log_id"] / f"trial_{k:02d}" / "filter_stats.npy"
        assert os.path.exists(path), path
        back = np.load(path, allow_pickle=True).item()
        assert set(back) == set(st)
        _same(back, st, f"row {row}")
        assert (back["trial_id"], back["batch_rows"], back["log_id"], back["obj_name"]) == (k, 4, st["log_id"], two[r].obj_model)
        assert back["time"] == st["time"] and back["traj_size"] == 3
