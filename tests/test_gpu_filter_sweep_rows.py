"""`filter_sweep` over runs that differ in config and in runner: a ycb-like run (3000 particles, noise_t 2e-4: config/expt/ycb.yaml's
form), a mcmaster-like run (1500 particles, noise_t 1e-4: config/expt/mcmaster.yaml's scalar form) and a run under `filter_real`'s
preset (raw scores, floor 10 000, a measurement update on every second frame) in ONE sweep, two trials each: B = 6 rows of one
batch at capacity 3000.  Every row equals, exactly, `filter(run_cfg, run, seed=seed + row, start="device", softmax=..., floor=...,
update_freq=..., cluster_every=5)`.  T = 12: frames 0, 5 and 10 cluster."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_filter_sweep import OBJECTS, D, _same  # noqa: E402

T, SEED, TRIALS, EVERY = 12, 6100, 2, 5
SOFTMAX, FLOOR, FREQ = [True, True, False], [1000, 1000, 10000], [1, 1, 2]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cfgs():
    from midastouch_amd.config import load_config
    ycb = load_config(["expt.params.num_particles=3000"])
    mcm = load_config(["expt=mcmaster", "expt.params.num_particles=1500", "expt.params.noise_ratio=0.5", "expt.log_id=7"])
    assert ycb.expt.params.noise_t.sim == 2e-4 and mcm.expt.params.noise_t == 1e-4
    return ycb, mcm


@pytest.fixture(scope="module")
def runs(dev, cfgs):
    from midastouch_amd import ops
    from midastouch_amd.filter import Sequence
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    from midastouch_amd.tactile_tree import tactile_tree
    ycb, mcm = cfgs
    out = []
    for r, (i, cfg, log_id) in enumerate(((0, ycb, 3), (2, mcm, None), (1, None, 5))):  # (run 2: the sweep's cfg)
        name, K = OBJECTS[i]
        cb = make_codebook(name, K=K, D=D, seed=1013 + i, mesh_points=4000)
        tt = tactile_tree(torch.as_tensor(cb.poses), torch.as_tensor(cb.cam_poses), torch.as_tensor(cb.embeddings))
        tt.to_device(dev)
        tr = make_trajectory(cb, T=T, seed=2300 + r)
        out.append(Sequence(torch.as_tensor(tr.gt_poses).to(dev), torch.as_tensor(tr.meas_poses).to(dev), torch.as_tensor(tr.codes).to(dev),
                            tt, cb.mesh_vertices, cb.obj_model, mesh_tree=ops.Tree(torch.as_tensor(cb.mesh_vertices).to(dev, torch.float64)),
                            log_id=log_id, cfg=cfg))
    return out


def test_rows_of_two_configs_and_two_runners(dev, cfgs, runs):
    from midastouch_amd.filter import filter as run_filter, filter_sweep
    ycb, mcm = cfgs
    got = filter_sweep(ycb, runs, trials=TRIALS, seed=SEED, device=dev, cluster_every=EVERY, softmax=SOFTMAX, floor=FLOOR, update_freq=FREQ)
    assert len(got) == 6
    run_cfg = (ycb, mcm, ycb)
    for row, st in enumerate(got):
        r, k = divmod(row, TRIALS)
        want = run_filter(run_cfg[r], runs[r], device=dev, seed=SEED + row, start="device", softmax=SOFTMAX[r], floor=FLOOR[r],
                          update_freq=FREQ[r], cluster_every=EVERY)
        _same(st, want, f"row {row}")
        for key in ("init_particles", "noise_ratio", "init_noise", "log_id", "obj_name", "tree_size"):
            assert st[key] == want[key], (row, key)
        assert (st["trial_id"], st["batch_rows"], st["traj_size"]) == (k, 6, T)
    assert [s["init_particles"] for s in got] == [3000, 3000, 1500, 1500, 3000, 3000]
    assert [s["log_id"] for s in got] == ["03", "03", "07", "07", "05", "05"] and got[2]["noise_ratio"] == 0.5
    # the settings bite: some row's count moved, and the two datasets' rows are not each other's
    assert any(min(s["num_particles"]) < s["init_particles"] for s in got)
    assert got[0]["rmse_t"] != got[1]["rmse_t"]
