"""BatchLoopEngine(wide=True) (midas_loop_step_batch_wide: sets beyond 16 384 particles per trajectory) against B single
LoopEngines - engine b built with seed + b, stepped with row b of the operands, as in tests/test_gpu_batch_loop.py whose helpers
these cases share.  After every frame, for every trajectory: the whole log row, the frame's per-particle arrays, the annealed set
and the resampled set, bit for bit.  Beyond 16 384 a single LoopEngine runs the single-kernel front and its own radix selection;
the batch runs the small-set front over more waves and that selection with the trajectory as grid.y - the comparison holds the two
fronts and the two selections to the same bits across engines.

The annealed counts asserted in the first two cases are the oracle's loop body on the CPU (OracleLoop, Philox seed 4100 + b)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from test_gpu_batch_loop import PER_PARTICLE, _frame, _near, _start, _traj, _wide_start, cb, dev  # noqa: F401 (cb, dev: fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n_after of every frame, rows 0 .. 2: floor 18 000, DBSCAN every 3rd frame, 14-frame trajectories ...
HIGH_FLOOR = [[24576, 23696, 20560, 18000, 18000, 18000, 24000, 18473, 18000, 18000, 18000, 18000],
              [24576, 23322, 21191, 18000, 18000, 18000, 18000, 18620, 18060, 18000, 18000, 18000],
              [24576, 23472, 19918, 18000, 18563, 18671, 18111, 18000, 18000, 18000, 18010, 18000]]
# ... and floor 1000, DBSCAN every 5th frame, 30-frame trajectories
LOW_FLOOR = [[24576, 23740, 21225, 14150, 13837, 13042, 12544, 11154, 10740, 9518],
             [24576, 23637, 21894, 20317, 13545, 9030, 6020, 6391, 6596, 6950],
             [24576, 23341, 18389, 12353, 8236, 5491, 3661, 3928, 4083, 4319]]


def _wide_engines(dev, cb, B, cap, seed, **kw):
    """test_gpu_batch_loop._engines with a wide batch engine: B LoopEngines (seed + b) and the BatchLoopEngine(wide=True)."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    singles = [LoopEngine(*src, cap, seed=seed + b, device=dev, **kw) for b in range(B)]
    return singles, BatchLoopEngine(*src, B, cap, seed=seed, device=dev, wide=True, **kw)


def _three_rows(dev, oracle, cb, frames, floor, every):
    """The three rows of the first two cases: trajectory seeds 2013 + b, wide starts of 24 576 particles from generator seeds 11 + b."""
    B, N0, seed = 3, 24576, 4100
    trajs = [_traj(cb, frames, 2013 + b) for b in range(B)]
    starts = [_wide_start(oracle, cb, trajs[b], N0, 11 + b) for b in range(B)]
    singles, batch = _wide_engines(dev, cb, B, N0, seed, floor=floor, cluster_every=every)
    _start(singles, batch, starts)
    return trajs, starts, singles, batch


def test_high_floor_every_frame_above_small_regime(dev, oracle, cb):
    """Floor 18 000: every frame has 5 or 6 summation blocks per trajectory.  Frame 6 duplicates 6000 particles in row 0 - three
    sort chunks of 2048 - while rows 1 and 2 do not anneal; frame 7 has a removal, a duplication and a removal side by side.
    Row 0 is also held against the oracle's loop body for frames 0 .. 6."""
    from test_gpu_loop import _compare_frame
    T, seed = 12, 4100
    trajs, starts, singles, batch = _three_rows(dev, oracle, cb, 14, 18000, 3)
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, cluster=True, cluster_every=3, floor=18000)
    poses, labels = starts[0], np.zeros(len(starts[0]), dtype=np.int64)
    sizes = [[] for _ in trajs]
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        if t <= 6:
            tn, rot = oracle.philox_noise(poses.shape[0], seed, t, np.float32(2e-4), np.float32(0.5))
            ref = loop.step(poses, labels, trajs[0].odoms[t + 1], trajs[0].codes[t + 1], tn, rot, gt=trajs[0].gt_poses[t + 1],
                            mode="weighted_random", u32=None, draws=lambda n2: oracle.philox_uniform64(n2, seed, t))
            _compare_frame(views[0], ref, t, t % 3 == 0)
            poses, labels = ref["poses"], ref["labels"]
        for b, v in enumerate(views):
            sizes[b].append(v["n_after"])
    print("annealed counts:", sizes)
    assert sizes == HIGH_FLOOR
    assert not batch.ctl_i[:, 14].any()  # no limit / bound error flagged


def test_down_through_small_regime_and_block_boundaries(dev, oracle, cb):
    """Floor 1000: the rows fall from six summation blocks through 16 384 particles and every block boundary below it, each at
    its own frame, and grow again - on the wide path's launches throughout (the grids cover the capacity)."""
    trajs, _, singles, batch = _three_rows(dev, oracle, cb, 30, 1000, 5)
    sizes = [[] for _ in trajs]
    for t in range(10):
        for b, v in enumerate(_frame(singles, batch, trajs, t)):
            sizes[b].append(v["n_after"])
    print("annealed counts:", sizes)
    assert sizes == LOW_FLOOR
    assert not batch.ctl_i[:, 14].any()


@pytest.mark.parametrize("resample", ["weighted_random", "low_var"])
def test_ragged_starts_around_small_regime_and_block(dev, cb, resample):
    """Starts on either side of 16 384 (the small regime's bound, a block boundary) and of 20 480 (the next), capacity 20 481."""
    ns = [16383, 16384, 16385, 20479, 20480, 20481]
    B, T, seed = len(ns), 4, 77
    trajs = [_traj(cb, T, 2021 + b) for b in range(B)]
    rng = np.random.default_rng(3)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 200, ns[b], rng) for b in range(B)]
    singles, batch = _wide_engines(dev, cb, B, 20481, seed, floor=500, cluster_every=3, resample=resample)
    _start(singles, batch, starts)
    for t in range(T):
        _frame(singles, batch, trajs, t)
    assert not batch.ctl_i[:, 14].any()


def test_wide_entry_equals_small_entry(dev, oracle, cb):
    """test_free_running_batch's scenario (B = 4 from N0 = 6000, DBSCAN every 5th frame), first 10 frames: a wide engine against a
    plain one - every array, control block and log row."""
    from midastouch_amd import BatchLoopEngine
    B, N0, T, seed = 4, 6000, 10, 4100
    trajs = [_traj(cb, 40, 2013 + b) for b in range(B)]
    starts = [torch.as_tensor(_wide_start(oracle, cb, trajs[b], N0, 11 + b)) for b in range(B)]
    engs = [BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, seed=seed, cluster_every=5, device=dev, wide=w) for w in (True, False)]
    for e in engs:
        e.set_particles(starts)
    for t in range(T):
        odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
        codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
        gts = torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs]))
        for e in engs:
            e.step(odoms, codes, gts=gts)
        w, s = engs
        assert torch.equal(w._log[:, t].view(torch.int64), s._log[:, t].view(torch.int64)), f"frame {t}: log rows"
        assert torch.equal(w.ctl_i, s.ctl_i) and torch.equal(w.ctl_d.view(torch.int64), s.ctl_d.view(torch.int64)), f"frame {t}: control blocks"
        for b in range(B):
            fw, fs = w.frame_view(b), s.frame_view(b)
            for k in PER_PARTICLE:
                assert fw[k].shape == fs[k].shape and torch.equal(fw[k], fs[k]), f"frame {t}, trajectory {b}: {k}"
            assert np.array_equal(fw["cluster_poses"], fs["cluster_poses"]) and np.array_equal(fw["cluster_stds"], fs["cluster_stds"])
    assert min(engs[0].n) < N0  # the rows annealed


def test_reference_size(dev, cb):
    """The reference's own num_particles (config/expt/ycb.yaml): B = 4 of 50 000, a DBSCAN frame and two plain ones."""
    B, N0, T, seed = 4, 50000, 3, 4200
    trajs = [_traj(cb, T, 2060 + b) for b in range(B)]
    rng = np.random.default_rng(12)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 400, N0, rng) for b in range(B)]
    singles, batch = _wide_engines(dev, cb, B, N0, seed)
    _start(singles, batch, starts)
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
    assert any(v["n_after"] != N0 for v in views)  # annealing acted at this size
    assert not batch.ctl_i[:, 14].any()


def test_maximum_capacity(dev, cb):
    """The largest capacity the entry takes - 131 072 particles: 2048 front waves and 32 summation blocks a trajectory - with B = 2:
    a full row beside one that starts a particle past a block boundary, a DBSCAN frame and two plain ones."""
    from midastouch_amd import _lib
    cap = _lib.LOOP_BATCH_WIDE_MAX_CAP
    B, T, seed = 2, 3, 4300
    trajs = [_traj(cb, T, 2070 + b) for b in range(B)]
    rng = np.random.default_rng(13)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 400, n, rng) for b, n in enumerate((cap, 24 * 4096 + 1))]
    singles, batch = _wide_engines(dev, cb, B, cap, seed)
    _start(singles, batch, starts)
    sizes = []
    for t in range(T):
        sizes.append([v["n_after"] for v in _frame(singles, batch, trajs, t)])
    print("annealed counts:", sizes)
    assert not batch.ctl_i[:, 14].any()


def test_wide_rejections(dev, cb):
    """Outside the wide regime: MidasError from the constructor, from the seeded forms and from the entry point, nothing enqueued."""
    from midastouch_amd import BatchLoopEngine, _lib
    from midastouch_amd._lib import MidasError
    mk = lambda B, cap, **kw: BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, device=dev, **kw)  # noqa: E731
    with pytest.raises(MidasError):
        mk(2, _lib.LOOP_BATCH_WIDE_MAX_CAP + 1, wide=True)
    with pytest.raises(MidasError):
        mk(129, _lib.LOOP_BATCH_WIDE_MAX_CAP, wide=True)  # 129 x 131 072 > 2^24
    with pytest.raises(MidasError):
        mk(2, _lib.LOOP_BATCH_MAX_CAP + 1)  # the default keeps its bound
    B, n, T = 2, 20000, 2
    eng = mk(B, n, wide=True)
    with pytest.raises(MidasError):
        eng.seed_torch_streams([1, 2])
    with pytest.raises(MidasError):
        eng.topk_ties = "aten_cpu"
    assert eng.topk_ties == "index" and eng.torch_streams is None and eng._args.topk_ties == _lib.TOPK_TIES_INDEX
    trajs = [_traj(cb, T, 2050 + b) for b in range(B)]
    rng = np.random.default_rng(9)
    eng.set_particles([_near(cb, tr.gt_poses[0][:3, 3], 100, n, rng) for tr in trajs])
    odoms = torch.as_tensor(np.stack([tr.odoms[1] for tr in trajs]))
    codes = torch.as_tensor(np.stack([tr.codes[1] for tr in trajs]))

    def untouched():
        torch.cuda.synchronize()
        return eng.step_count == 0 and not eng.ctl_i[:, _lib.LOOP_I_FRAME].any() and not eng.poses_prop.any()

    a = eng._args
    keep = (odoms.to(dev), codes.to(dev))
    a.odom16, a.code, a.score_epoch = keep[0].data_ptr(), keep[1].data_ptr(), 1
    a.labels, a.labels_out = eng._labels.data_ptr(), eng._labels_next.data_ptr()
    phases, stride = 1 | 4 | 8, eng.log_frames * _lib.LOOP_LOG_DOUBLES

    def call(batch):
        eng.ctx.check(eng.ctx.lib.midas_loop_step_batch_wide(eng.ctx.h, eng.codebook.h, eng.tree6.h, eng.tree3.h, C.byref(a), phases, batch, stride))

    for field, bad, good in (("cap", _lib.LOOP_BATCH_WIDE_MAX_CAP + 1, n), ("grid_n", n, 0), ("anneal_frozen", 1, 0),
                             ("tn", keep[0].data_ptr(), None), ("u", keep[0].data_ptr(), None),
                             ("topk_ties", _lib.TOPK_TIES_ATEN_CPU, _lib.TOPK_TIES_INDEX)):
        setattr(a, field, bad)
        with pytest.raises(MidasError):
            call(B)
        setattr(a, field, good)
    for bad in (0, 65536, (1 << 24) // n + 1):  # the last: B x cap > 2^24
        with pytest.raises(MidasError):
            call(bad)
    # the small entries keep their bound for these arguments
    for entry in (eng.ctx.lib.midas_loop_step_batch, eng.ctx.lib.midas_loop_step_batch_draws):
        with pytest.raises(MidasError):
            eng.ctx.check(entry(eng.ctx.h, eng.codebook.h, eng.tree6.h, eng.tree3.h, C.byref(a), phases, B, stride))
    assert untouched()
    eng.step(odoms, codes)  # ... and the frame goes through once everything is in order
    assert eng.read_log()[1][0]["n"] == n and eng.step_count == 1


def test_wide_batch_no_frame_allocates(dev):
    """tests/test_gpu_batch_loop_state.py's check for a wide engine - 8 trajectories of 50 000 particles through a DBSCAN frame and two
    plain ones with ground truth: the selection's per-trajectory state and pair buffers are part of the reservation, and after the
    constructor MIDAS_SCRATCH_LOG reports no chunk.  (The switch is read once per process: a child process.)"""
    code = (
        "import sys, numpy as np, torch\n"
        "from midastouch_amd import BatchLoopEngine\n"
        "from midastouch_amd.synthetic import make_codebook, make_trajectory\n"
        "dev = torch.device('cuda', 0)\n"
        "B, cap = 8, 50000\n"
        "cb = make_codebook(K=3000, D=256, seed=1013, mesh_points=20000)\n"
        "tr = make_trajectory(cb, T=4, seed=2000)\n"
        "eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=4000, device=dev, wide=True)\n"
        "sys.stderr.write('MARK\\n'); sys.stderr.flush()\n"
        "rng = np.random.default_rng(0)\n"
        "eng.set_particles(torch.as_tensor(cb.poses[rng.integers(0, 3000, (B, cap))]))\n"
        "for t in range(3):\n"
        "    rep = lambda a: torch.as_tensor(a[t + 1])[None].repeat(B, *([1] * a[t + 1].ndim)).contiguous()\n"
        "    eng.step(rep(tr.odoms), rep(tr.codes), gts=rep(tr.gt_poses))\n"
        "torch.cuda.synchronize()\n"
        "print('DONE', min(eng.n), max(eng.n))\n")
    env = dict(os.environ, MIDAS_SCRATCH_LOG="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DONE" in r.stdout
    before, after = r.stderr.split("MARK")
    assert "reserved one chunk" in before and "[midas] scratch" not in after, r.stderr
