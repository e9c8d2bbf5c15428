"""The host side of `filter_sweep` (objects x logs x trials as one batch) and of the device start, without a device: the row plan,
the stats assembly, the refusals, the new defaults - and the start's formula (csrc/start.hip, restated by
`particle_filter.start_transforms`) in float64 against `oracle.init_filter_compose` and fixture G8."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

U = 2.0 ** -24  # float32 unit roundoff


def _seq(codebook, T, **kw):
    """A stand-in for a Sequence: what the plan reads."""
    return SimpleNamespace(codebook=codebook, gt_p=torch.zeros(T, 4, 4), **kw)


def test_row_plan_groups_by_codebook_identity():
    from midastouch_amd.filter import sweep_plan
    a, b, c = object(), object(), object()
    runs = [_seq(a, 7), _seq(b, 12), _seq(a, 54), _seq(c, 9), _seq(b, 3)]
    p = sweep_plan(runs, trials=1)
    assert p["objects"] == [0, 1, 3]  # the first run of every object, in order of first appearance
    assert p["run_object"] == [0, 1, 0, 2, 1]
    assert p["row_object"] == [0, 1, 0, 2, 1] and p["row_run"] == [0, 1, 2, 3, 4] and p["row_trial"] == [0] * 5
    assert p["lengths"] == [7, 12, 54, 9, 3] and p["run_lengths"] == [7, 12, 54, 9, 3] and p["T_max"] == 54
    # equal but distinct codebooks are distinct objects: identity, not equality
    same = [_seq((1, 2), 5), _seq(tuple([1, 2]), 5)]
    assert same[0].codebook == same[1].codebook and same[0].codebook is not same[1].codebook
    assert sweep_plan(same)["run_object"] == [0, 1]


def test_row_plan_trials_order_and_lengths():
    from midastouch_amd.filter import sweep_plan
    a, b = object(), object()
    runs = [_seq(a, 7), _seq(b, 12), _seq(a, 54)]
    p = sweep_plan(runs, trials=3)
    # row r * trials + k is run r, trial k
    assert p["row_run"] == [0, 0, 0, 1, 1, 1, 2, 2, 2] and p["row_trial"] == [0, 1, 2] * 3
    assert all(p["row_run"][r * 3 + k] == r and p["row_trial"][r * 3 + k] == k for r in range(3) for k in range(3))
    assert p["row_object"] == [0, 0, 0, 1, 1, 1, 0, 0, 0]
    assert p["lengths"] == [7] * 3 + [12] * 3 + [54] * 3 and p["T_max"] == 54
    # max_length (cfg.expt.max_length, "None" as the yaml spells it) and max_frames both cut, the shorter wins
    assert sweep_plan(runs, 1, max_length="None", max_frames=None)["lengths"] == [7, 12, 54]
    assert sweep_plan(runs, 1, max_length=10)["lengths"] == [7, 10, 10]
    q = sweep_plan(runs, 2, max_length=40, max_frames=9)
    assert q["lengths"] == [7, 7, 9, 9, 9, 9] and q["run_lengths"] == [7, 9, 9] and q["T_max"] == 9


def test_row_seeds_are_seed_plus_row():
    """The engine keys row b's streams seed + b (BatchLoopEngine); the sweep's rows are its rows, so run r, trial k draws from
    seed + r * trials + k - what the yardstick `filter(seed=seed + row)` is given."""
    from midastouch_amd.filter import sweep_plan
    p = sweep_plan([_seq(object(), 4) for _ in range(4)], trials=2)
    rows = {(r, k): row for row, (r, k) in enumerate(zip(p["row_run"], p["row_trial"]))}
    assert rows == {(r, k): r * 2 + k for r in range(4) for k in range(2)}


def _record(f, n_after, ncl=1):
    return dict(frame=f, n=n_after + 1, n_after=n_after, rmse_t=0.001 * (f + 1), rmse_r=float(f), err=0,
                cluster_poses=np.tile(np.eye(4, dtype=np.float32), (ncl, 1, 1)) * (f + 1), cluster_stds=np.full((ncl, 3), f, np.float32))


def test_stats_assembly():
    from midastouch_amd.filter import sweep_stats
    recs = [_record(f, 100 - f, ncl=1 + f % 2) for f in range(5)]
    times = [0.01 * (i + 1) for i in range(9)]  # the batch ran 9 frames: this row's log ended after 5
    host = [0.5] * 9
    st = sweep_stats(recs, times, host, obj_name="mug", tree_size=900, noise_ratio=1.0, init_noise=[0.1, 60.0], init_particles=100,
                     log_id="03", trial_id=2, batch_rows=6)
    assert st["rmse_t"] == [0.001 * (f + 1) for f in range(5)] and st["rmse_r"] == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert st["num_particles"] == [100, 99, 98, 97, 96] and st["traj_size"] == 5
    assert st["time"] == times[:5] and st["total_time"] == sum(times[:5]) and st["avg_time"] == sum(times[:5]) / 5
    assert [tuple(c.shape) for c in st["cluster_poses"]] == [(1, 4, 4), (2, 4, 4), (1, 4, 4), (2, 4, 4), (1, 4, 4)]
    assert all(torch.is_tensor(c) for c in st["cluster_poses"] + st["cluster_stds"])
    assert torch.equal(st["cluster_poses"][3], torch.as_tensor(recs[3]["cluster_poses"]))
    assert st["frames"] is recs and st["frame_idx"] == [0, 1, 2, 3, 4] and st["host_time"] == [0.5] * 5
    assert st["avg_timer"] == {"tactile": 0.0, "motion": 0.0, "meas": st["avg_time"], "host_enqueue": 0.5}
    assert (st["obj_name"], st["tree_size"], st["log_id"], st["trial_id"], st["batch_rows"]) == ("mug", 900, "03", 2, 6)
    # filter()'s keys, and the sweep's own
    want = {"rmse_t", "rmse_r", "time", "traj_size", "avg_time", "total_time", "cluster_poses", "cluster_stds", "obj_name", "tree_size",
            "noise_ratio", "init_noise", "init_particles", "num_particles", "log_id", "trial_id", "avg_timer", "frames", "frame_idx",
            "host_time", "batch_rows"}
    assert set(st) == want
    empty = sweep_stats([], times, host, log_id="00")
    assert empty["traj_size"] == 0 and empty["avg_time"] == 0 and empty["time"] == []


def test_refusals():
    from midastouch_amd.config import load_config
    from midastouch_amd.filter import filter as run_filter, filter_sweep, sweep_plan
    cfg = load_config()
    one = [_seq(object(), 5)]
    with pytest.raises(ValueError, match="at least one run"):
        filter_sweep(cfg, [])
    with pytest.raises(ValueError, match="trials >= 1"):
        filter_sweep(cfg, one, trials=0)
    with pytest.raises(ValueError, match="trials >= 1"):
        sweep_plan(one, trials=-2)
    with pytest.raises(ValueError, match="seeded sweep.*out of its scope"):
        filter_sweep(cfg, one, draws="seeded")
    with pytest.raises(ValueError, match="draws='device'"):
        filter_sweep(cfg, one, draws="host")
    with pytest.raises(ValueError, match="start must be"):
        run_filter(cfg, one[0], device="cuda:0", start="gpu")
    with pytest.raises(ValueError, match="draws='device' only"):
        run_filter(cfg, one[0], device="cuda:0", start="device", draws="seeded")


def test_codebooks_of_different_d_are_refused_by_for_objects():
    """The sweep hands its objects to BatchLoopEngine.for_objects as (tactile_tree, None, mesh tree): one D for all, checked before
    a device is asked for."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    tt = lambda D: SimpleNamespace(codebook=SimpleNamespace(D=D))  # noqa: E731
    with pytest.raises(MidasError, match=r"codebooks of one D, got \[128, 256, 128\]"):
        BatchLoopEngine.for_objects([(tt(128), None, None), (tt(256), None, None), (tt(128), None, None)], [0, 1, 2, 0], 700)


def test_sequence_log_id_default_and_fallback():
    from midastouch_amd.filter import Sequence, _log_id
    seq = Sequence(None, None, None, None, None, "mug")
    assert seq.log_id is None and seq.mesh_tree is None
    expt = SimpleNamespace(log_id=3)
    assert _log_id(seq, expt) == "03"  # as filter() always wrote it
    seq.log_id = 12
    assert _log_id(seq, expt) == "12"
    assert _log_id(Sequence(None, None, None, None, None, "mug", log_id="4"), expt) == "04"


def test_signature_defaults():
    from midastouch_amd.batch_loop_engine import BatchLoopEngine
    from midastouch_amd.filter import filter as run_filter, filter_real, filter_sweep
    from midastouch_amd.loop_engine import LoopEngine, _LoopBase
    p = inspect.signature(run_filter).parameters
    assert p["start"].default == "host" and p["cluster_every"].default == 50  # today's behaviour
    assert p["draws"].default == "device" and p["seed"].default == 4000 and p["floor"].default == 1000
    s = inspect.signature(filter_sweep).parameters
    assert list(s)[:2] == ["cfg", "runs"] and all(s[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(s)[2:])
    want = dict(trials=1, seed=4000, device=None, max_frames=None, cluster=True, cluster_every=50, softmax=True, update_freq=1,
                floor=1000, results_root=None)
    assert {k: s[k].default for k in want} == want
    assert inspect.signature(filter_real).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD  # passes start / cluster_every on
    st = inspect.signature(_LoopBase.start).parameters
    assert list(st)[:7] == ["self", "gts", "init_noise", "n", "project", "tn", "rot"]
    assert (st["n"].default, st["project"].default, st["tn"].default, st["rot"].default) == (None, True, None, None)
    assert LoopEngine.start is _LoopBase.start and BatchLoopEngine.start is _LoopBase.start
    # the batch frame keeps its parameters; the starting frames' (0, 0) noise goes through `step_still`
    assert "std_override" not in inspect.signature(BatchLoopEngine.step).parameters
    assert "std_override" in inspect.signature(LoopEngine.step).parameters
    assert inspect.signature(BatchLoopEngine.step_still).parameters["std_override"].default == (0.0, 0.0)


# ---- the start's formula ----------------------------------------------------------------------------------------------------------
def _gt(rng):
    from scipy.spatial.transform import Rotation
    G = np.eye(4, dtype=np.float32)
    G[:3, :3] = Rotation.from_rotvec(rng.normal(size=3)).as_matrix().astype(np.float32)
    G[:3, 3] = rng.normal(scale=0.1, size=3).astype(np.float32)
    return G


def test_start_formula_is_scipys_extrinsic_zyx():
    """R = Rx(rot[2]) Ry(rot[1]) Rz(rot[0]) in float64 IS from_euler("zyx", rot, degrees=True): within float64 rounding before the
    float32 rounding, hence at most one float32 rounding apart after it - and not the intrinsic "ZYX"."""
    from scipy.spatial.transform import Rotation
    from midastouch_amd.particle_filter import start_transforms
    rng = np.random.default_rng(5)
    rot = rng.normal(scale=60.0, size=(20000, 3)).astype(np.float32)
    tn = rng.normal(scale=0.08, size=(20000, 3)).astype(np.float32)
    Tn = start_transforms(tn, rot)
    Rs = Rotation.from_euler("zyx", rot, degrees=True).as_matrix()
    assert Tn.dtype == np.float32 and np.array_equal(Tn[:, :3, 3], tn)
    assert np.array_equal(Tn[:, 3], np.tile(np.float32([0, 0, 0, 1]), (20000, 1)))
    R32 = Rs.astype(np.float32)
    flips = Tn[:, :3, :3] != R32
    assert np.all(np.abs(Tn[:, :3, :3].astype(np.float64) - Rs) <= np.abs(Rs) * 2 * U + 1e-15)  # a float32 rounding of |R| <= 1 ... plus float64 noise
    assert flips.mean() < 1e-6 * 100  # (a rounding flips only where the float64 values straddle a float32 tie)
    assert np.all(np.abs(Tn[:, :3, :3] - R32)[flips] <= np.spacing(np.abs(R32))[flips])
    wrong = Rotation.from_euler("ZYX", rot[:100], degrees=True).as_matrix()
    assert np.abs(wrong - Tn[:100, :3, :3]).max() > 0.1


def test_start_formula_against_oracle_and_g8(oracle, golden):
    """gt @ Tn of the formula against `oracle.init_filter_compose` (pinned to the reference by G8), under the bound the device test
    uses - every entry within 6 u (|gt| @ |Tn|) of the float64 product of the float32 factors - and against G8's poses."""
    from midastouch_amd.particle_filter import start_transforms
    rng = np.random.default_rng(8)
    n = 50000
    gt = _gt(rng)
    tn = rng.normal(scale=0.08, size=(n, 3)).astype(np.float32)
    rot = rng.normal(scale=60.0, size=(n, 3)).astype(np.float32)
    Tn = start_transforms(tn, rot)
    exact = gt.astype(np.float64)[None] @ Tn.astype(np.float64)
    bound = 6 * U * (np.abs(gt).astype(np.float64)[None] @ np.abs(Tn).astype(np.float64))
    ref = oracle.init_filter_compose(gt, tn, rot)
    assert ref.shape == exact.shape and np.all(np.abs(ref.astype(np.float64) - exact) <= bound)
    g = golden("g8_init")
    mine = (g["gt"].astype(np.float32)[None] @ start_transforms(g["tn"], g["rot"])).astype(np.float32)
    np.testing.assert_allclose(mine, g["poses"], rtol=0, atol=2e-6)  # (test_g8_init_filter's tolerance)
    np.testing.assert_allclose(mine, oracle.init_filter_compose(g["gt"], g["tn"], g["rot"]), rtol=0, atol=2e-6)
