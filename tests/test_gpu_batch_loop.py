"""BatchLoopEngine (midas_loop_step_batch: B clustering and annealing filters per set of launches) against B single
LoopEngines - engine b built with seed + b and the same settings, stepped with row b of the operands.  After every frame, for
every trajectory: the whole log row, the frame's per-particle arrays, the annealed set and the resampled set, bit for bit.

In every case the first half of the single engines is stepped before the batch frame and the rest after it, so the single path is
exercised on both sides of the batch launches in one process.

tests/test_gpu_batch_loop_regime.py takes the same comparison to the rest of the regime: 16 384 particles, B = 64, D = 512, every
option of step() and set_particles(), the log ring and the epoch restart."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K, D = 3000, 256
PER_PARTICLE = ("poses_prop", "nn_idx", "valid", "weights", "labels_frame", "src", "ridx", "poses", "weights_res", "labels", "hint")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cb():
    from midastouch_amd.synthetic import make_codebook
    return make_codebook(K=K, D=D, seed=1013, mesh_points=20000)


def _traj(cb, T, seed):
    from midastouch_amd.synthetic import make_trajectory
    return make_trajectory(cb, T=T + 1, seed=seed)


def _near(cb, centre, m, n, rng):
    """n particles on the m codebook poses nearest to `centre` (a translation)."""
    d = np.linalg.norm(cb.poses[:, :3, 3] - centre, axis=1)
    return cb.poses[rng.choice(np.argsort(d)[:m], n)]


def _wide_start(oracle, cb, traj, N0, gseed):
    """The start of test_loop_engine_free_running_vs_oracle: noise around the first ground-truth pose, projected onto the codebook."""
    from midastouch_amd.synthetic import mesh_scale
    g = torch.Generator().manual_seed(gseed)
    sc = mesh_scale(cb.extents)
    tn0 = torch.normal(0.0, sc / 3.0 * 0.15, size=(N0, 3), generator=g).numpy()
    rot0 = torch.normal(0.0, 60.0 * 0.15, size=(N0, 3), generator=g).numpy()
    poses = oracle.init_filter_compose(traj.gt_poses[0], tn0, rot0)
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices)
    return cb.poses[loop.f.SE3_NN_idx(poses)]


def _engines(dev, cb, B, cap, seed, index=None, **kw):
    """B LoopEngines (seed + b) and the BatchLoopEngine.  index: (tactile_tree on the device, ops.Tree of the mesh) that all of
    them share instead of an index each (engine.codebook_index)."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    src = (cb.poses, cb.embeddings, cb.mesh_vertices) if index is None else (index[0], None, index[1])
    singles = [LoopEngine(*src, cap, seed=seed + b, device=dev, **kw) for b in range(B)]
    batch = BatchLoopEngine(*src, B, cap, seed=seed, device=dev, **kw)
    return singles, batch


def _start(singles, batch, starts):
    for s, p in zip(singles, starts):
        s.set_particles(torch.as_tensor(p))
    batch.set_particles([torch.as_tensor(p) for p in starts])
    assert batch.n == [len(p) for p in starts]


def _frame(singles, batch, trajs, t, gt=True, rows=None, **kw):
    """Frame t of every engine (trajectory row b = trajs[b]'s frame t + 1) and the comparison of everything it left.  gt=False:
    a frame without ground truth; rows: the trajectories whose arrays are compared (default: all) - the log row is compared for
    every trajectory, and the returned views are those of `rows`."""
    B = len(singles)
    odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
    codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
    gts = torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs]))
    first = (B + 1) // 2
    for b in range(first):
        singles[b].step(odoms[b], codes[b], gt=gts[b] if gt else None, **kw)
    batch.step(odoms, codes, gts=gts if gt else None, **kw)
    for b in range(first, B):
        singles[b].step(odoms[b], codes[b], gt=gts[b] if gt else None, **kw)
    views = []
    slot = (batch.step_count - 1) % batch.log_frames
    for b in range(B):
        # the whole log row, as bits (NaN fields included)
        assert torch.equal(batch._log[b, slot].view(torch.int64), singles[b]._log[slot].view(torch.int64)), f"frame {t}, trajectory {b}: log row"
        if rows is not None and b not in rows:
            continue
        fs, fb = singles[b].frame_view(), batch.frame_view(b)
        assert (fb["n"], fb["n_after"]) == (fs["n"], fs["n_after"])
        for k in PER_PARTICLE:
            assert fb[k].shape == fs[k].shape and torch.equal(fb[k], fs[k]), f"frame {t}, trajectory {b}: {k}"
        assert np.array_equal(fb["cluster_poses"], fs["cluster_poses"]) and np.array_equal(fb["cluster_stds"], fs["cluster_stds"])
        views.append(fb)
    if rows is None:
        assert batch.n == [v["n_after"] for v in views]
    return views


def test_free_running_batch(dev, oracle, cb):
    """B = 4 from N0 = 6000 over 40 frames, DBSCAN every 5th, floor 1000; row b follows trajectory seed 2013 + b from a start drawn
    with generator seed 11 + b.  Row 0 is test_loop_engine_free_running_vs_oracle's [6000-weighted_random-True] scenario and is also
    held against the oracle's loop body.  The oracle, run on the CPU with these seeds, gives the rows the sizes 6000 .. 1177 ..
    2050, 6000 .. 1406 .. 2439, 6000 .. 1505 .. 2859 and 6000 .. 1086 .. 2647: every row shrinks and grows, and no two agree
    beyond the first frame."""
    from test_gpu_loop import _compare_frame
    B, N0, T, seed = 4, 6000, 40, 4100
    trajs = [_traj(cb, T, 2013 + b) for b in range(B)]
    starts = [_wide_start(oracle, cb, trajs[b], N0, 11 + b) for b in range(B)]
    singles, batch = _engines(dev, cb, B, N0, seed, cluster_every=5)
    _start(singles, batch, starts)
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, cluster=True, cluster_every=5)
    poses, labels = starts[0], np.zeros(N0, dtype=np.int64)
    sizes = [[] for _ in range(B)]
    for t in range(T):
        tn, rot = oracle.philox_noise(poses.shape[0], seed, t, np.float32(2e-4), np.float32(0.5))
        ref = loop.step(poses, labels, trajs[0].odoms[t + 1], trajs[0].codes[t + 1], tn, rot, gt=trajs[0].gt_poses[t + 1],
                        mode="weighted_random", u32=None, draws=lambda n2: oracle.philox_uniform64(n2, seed, t))
        views = _frame(singles, batch, trajs, t)
        _compare_frame(views[0], ref, t, t % 5 == 0)
        poses, labels = ref["poses"], ref["labels"]
        for b in range(B):
            sizes[b].append(views[b]["n_after"])
    assert any(len({sizes[b][t] for b in range(B)}) > 1 for t in range(T)), sizes  # live counts of two rows differ at some frame
    assert any(min(s) < N0 and any(y > x for x, y in zip(s, s[1:])) for s in sizes), sizes  # a row both shrinks and grows
    log = batch.read_log()
    assert [[r["n_after"] for r in rows] for rows in log] == sizes
    assert not batch.ctl_i[:, 14].any()  # no limit / bound error flagged


def test_ragged_starts(dev, cb):
    """Capacity 5000 (no multiple of 256) with starts on either side of a wave, a workgroup and a 4096-slot block."""
    ns = [1, 63, 64, 65, 257, 4097, 5000]
    B, T, seed = len(ns), 12, 77
    trajs = [_traj(cb, T, 2021 + b) for b in range(B)]
    rng = np.random.default_rng(3)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 200, ns[b], rng) for b in range(B)]
    singles, batch = _engines(dev, cb, B, 5000, seed, floor=500, cluster_every=3)
    _start(singles, batch, starts)
    for t in range(T):
        _frame(singles, batch, trajs, t)
    assert not batch.ctl_i[:, 14].any()


def test_batch_of_one_equals_loop_engine(dev, cb):
    T, seed = 10, 901
    trajs = [_traj(cb, T, 2030)]
    starts = [_near(cb, trajs[0].gt_poses[0][:3, 3], 300, 3000, np.random.default_rng(4))]
    singles, batch = _engines(dev, cb, 1, 3000, seed, cluster_every=3)
    _start(singles, batch, starts)
    for t in range(T):
        _frame(singles, batch, trajs, t)


@pytest.mark.parametrize("kw", [dict(resample="low_var"), dict(cluster=False), dict(softmax=False)], ids=["low_var", "no_cluster", "raw_scores"])
def test_settings(dev, cb, kw):
    """The systematic resampler (its one draw keyed seed + b), frames without clustering and annealing, and raw scores as weights
    with a frame without measurement update (unit weights) on every third frame."""
    B, N0, T, seed = 3, 2500, 12, 333
    trajs = [_traj(cb, T, 2040 + b) for b in range(B)]
    rng = np.random.default_rng(8)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 400, N0 - 300 * b, rng) for b in range(B)]
    singles, batch = _engines(dev, cb, B, N0, seed, floor=600, cluster_every=3, **kw)
    _start(singles, batch, starts)
    for t in range(T):
        _frame(singles, batch, trajs, t, unit_weights=("softmax" in kw and t % 3 == 2))


def test_all_pruned_row(dev, cb):
    """Row 0 starts half a metre off the mesh: every particle is pruned in the first frame and goes back onto its codebook pose
    (filter.py:176-179), the set goes on unresampled - beside rows that are not."""
    B, N0, T, seed = 3, 1500, 6, 510
    trajs = [_traj(cb, T, 2013 + b) for b in range(B)]
    rng = np.random.default_rng(6)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 100, N0, rng) for b in range(B)]
    starts[0] = starts[0].copy()
    starts[0][:, :3, 3] += np.float32(0.5)
    singles, batch = _engines(dev, cb, B, N0, seed, floor=500, cluster_every=3)
    _start(singles, batch, starts)
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        if t == 0:
            assert views[0]["drifted"] and views[0]["kept"] == 0 and views[0]["status"] == 1
            assert not views[1]["drifted"] and not views[2]["drifted"]


def test_different_cluster_counts(dev, cb):
    """Row 0 starts on two separated clouds (the oracle's DBSCAN finds two clusters and noise in its first frames) beside rows on one."""
    B, N0, T, seed = 3, 1500, 6, 510
    trajs = [_traj(cb, T, 2013 + b) for b in range(B)]
    t3 = cb.poses[:, :3, 3]
    far = t3[int(np.argmax(np.linalg.norm(t3 - trajs[0].gt_poses[0][:3, 3], axis=1)))]
    rng = np.random.default_rng(5)
    two = np.concatenate([_near(cb, trajs[0].gt_poses[0][:3, 3], 50, N0 // 2, rng), _near(cb, far, 50, N0 - N0 // 2, rng)])
    starts = [two] + [_near(cb, trajs[b].gt_poses[0][:3, 3], 50, N0, rng) for b in range(1, B)]
    singles, batch = _engines(dev, cb, B, N0, seed, floor=500, cluster_every=3)
    _start(singles, batch, starts)
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        if t == 0:
            assert views[0]["ncl"] == 2 and views[1]["ncl"] == 1 and views[2]["ncl"] == 1, [v["ncl"] for v in views]


def test_rejections(dev, cb):
    """Outside the small-set regime, an empty batch, operands of the wrong leading size: MidasError, nothing enqueued."""
    from midastouch_amd import BatchLoopEngine, _lib
    from midastouch_amd._lib import MidasError
    mk = lambda B, cap: BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, device=dev)  # noqa: E731
    with pytest.raises(MidasError):
        mk(2, _lib.LOOP_BATCH_MAX_CAP + 1)
    with pytest.raises(MidasError):
        mk(0, 1000)
    B, n, T = 2, 1000, 2
    eng = mk(B, n)
    trajs = [_traj(cb, T, 2050 + b) for b in range(B)]
    rng = np.random.default_rng(9)
    eng.set_particles([_near(cb, tr.gt_poses[0][:3, 3], 100, n, rng) for tr in trajs])
    odoms = torch.as_tensor(np.stack([tr.odoms[1] for tr in trajs]))
    codes = torch.as_tensor(np.stack([tr.codes[1] for tr in trajs]))

    def untouched():
        torch.cuda.synchronize()
        return eng.step_count == 0 and not eng.ctl_i[:, _lib.LOOP_I_FRAME].any() and not eng.poses_prop.any()

    with pytest.raises(MidasError):
        eng.step(torch.cat([odoms, odoms[:1]]), codes)
    with pytest.raises(MidasError):
        eng.step(odoms, codes[:1])
    with pytest.raises(MidasError):
        eng.step(odoms, codes, gts=odoms[:1])
    assert untouched()
    # the entry point itself: the same frame with B = 0, with a capacity beyond the regime, with host draws, with a bound
    a = eng._args
    keep = (odoms.to(dev), codes.to(dev))
    a.odom16, a.code, a.score_epoch = keep[0].data_ptr(), keep[1].data_ptr(), 1
    a.labels, a.labels_out = eng._labels.data_ptr(), eng._labels_next.data_ptr()
    phases, stride = 1 | 4 | 8, eng.log_frames * _lib.LOOP_LOG_DOUBLES

    def call(batch):
        eng.ctx.check(eng.ctx.lib.midas_loop_step_batch(eng.ctx.h, eng.codebook.h, eng.tree6.h, eng.tree3.h, C.byref(a), phases, batch, stride))

    for field, bad, good in (("cap", _lib.LOOP_BATCH_MAX_CAP + 1, n), ("grid_n", n, 0), ("tn", keep[0].data_ptr(), None),
                             ("topk_ties", _lib.TOPK_TIES_ATEN_CPU, _lib.TOPK_TIES_INDEX), ("anneal_frozen", 1, 0)):
        setattr(a, field, bad)
        with pytest.raises(MidasError):
            call(B)
        setattr(a, field, good)
    for bad in (0, 65536):
        with pytest.raises(MidasError):
            call(bad)
    assert untouched()
    eng.step(odoms, codes)  # ... and the frame goes through once everything is in order
    assert eng.read_log()[1][0]["n"] == n and eng.step_count == 1
