"""BatchLoopEngine.seed_torch_streams and topk_ties="aten_cpu" (midas_loop_step_batch_draws, midas_mt19937_draws_counted_batch): B
seeded runs of the reference per set of launches - against B LoopEngines built with topk_ties="aten_cpu" and seed_torch_stream, after
every frame and bit for bit; against the reference's loop trace (G13) inside a batch; against the oracle's loop body fed from
torch's host generator; the tie rule alone, the way back to Philox, and the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from _recipes import sha

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_PARTICLE = ("poses_prop", "nn_idx", "valid", "weights", "labels_frame", "src", "ridx", "poses", "weights_res", "labels", "hint")
N, K, D, FLOOR = 6000, 2500, 256, 500  # the scenario of tests/test_gpu_loop_seeded.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cb():
    from midastouch_amd.synthetic import make_codebook
    return make_codebook("004_sugar_box", K=K, D=D, seed=1000)


@pytest.fixture(scope="module")
def traj(cb):
    from midastouch_amd.synthetic import make_trajectory
    return make_trajectory(cb, T=30, seed=2000)


@pytest.fixture(scope="module")
def wide(oracle, cb, traj):
    """N particles around the first ground-truth pose, projected onto the codebook (test_loop_engine_free_running_vs_oracle's start)."""
    from midastouch_amd.synthetic import mesh_scale
    g = torch.Generator().manual_seed(11)
    sc = mesh_scale(cb.extents)
    tn0 = torch.normal(0.0, sc / 3.0 * 0.15, size=(N, 3), generator=g).numpy()
    rot0 = torch.normal(0.0, 60.0 * 0.15, size=(N, 3), generator=g).numpy()
    poses = oracle.init_filter_compose(traj.gt_poses[0], tn0, rot0)
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices)
    return cb.poses[loop.f.SE3_NN_idx(poses)]


def _engines(dev, cb, B, cap, seed, **kw):
    """B LoopEngines (Philox seed + b, topk_ties="aten_cpu") and the BatchLoopEngine."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    singles = [LoopEngine(*src, cap, seed=seed + b, device=dev, topk_ties="aten_cpu", **kw) for b in range(B)]
    return singles, BatchLoopEngine(*src, B, cap, seed=seed, device=dev, **kw)


def _operands(traj, t, B):
    rep = lambda a: torch.as_tensor(a[t + 1])[None].repeat(B, *([1] * a[t + 1].ndim)).contiguous()  # noqa: E731
    return rep(traj.odoms), rep(traj.codes), rep(traj.gt_poses)


def _compare(singles, batch, t, rows=None):
    """tests/test_gpu_batch_loop.py's _frame, the comparison: the whole log row as bits, every array of frame_view(b)."""
    views = []
    slot = (batch.step_count - 1) % batch.log_frames
    for b, single in enumerate(singles):
        if rows is not None and b not in rows:
            continue
        assert torch.equal(batch._log[b, slot].view(torch.int64), single._log[slot].view(torch.int64)), f"frame {t}, trajectory {b}: log row"
        fs, fb = single.frame_view(), batch.frame_view(b)
        assert (fb["n"], fb["n_after"]) == (fs["n"], fs["n_after"])
        for k in PER_PARTICLE:
            assert fb[k].shape == fs[k].shape and torch.equal(fb[k], fs[k]), f"frame {t}, trajectory {b}: {k}"
        assert np.array_equal(fb["cluster_poses"], fs["cluster_poses"]) and np.array_equal(fb["cluster_stds"], fs["cluster_stds"])
        views.append(fb)
    return views


def _frame(singles, batch, traj, t, **kw):
    """Frame t of every engine - half of the singles in front of the batch's launches, half behind - and the comparison."""
    B = len(singles)
    odoms, codes, gts = _operands(traj, t, B)
    first = (B + 1) // 2
    for b in range(first):
        singles[b].step(odoms[b], codes[b], gt=gts[b], **kw)
    batch.step(odoms, codes, gts=gts, **kw)
    for b in range(first, B):
        singles[b].step(odoms[b], codes[b], gt=gts[b], **kw)
    return _compare(singles, batch, t)


def _next8(stream_to_host):
    g = torch.Generator()
    stream_to_host(g)
    return torch.rand(8, dtype=torch.float64, generator=g)


# ---- (a) ------------------------------------------------------------------------------------------------------------------
S_A = 7100
# torch.manual_seed(S_A + b) per row, chosen on the CPU with oracle.OracleLoop(floor=500, ties="aten_cpu") fed torch.normal /
# torch.rand of a host generator: the reference alone then runs (n, n_after per frame)
#   row 0  6000 6000 | 6000 4000 | 4000 3671 | 3671 3217 | 3217 2970 | 2970 2386 | .. | 2326 2422 | 2422 2245
#   row 1  6000 6000 | 6000 4000 | 4000 3756 | 3756 3231 | 3231 2154 | 2154 2309 | .. | 2458 3277 | 3277 3473
#   row 2  4097 4097 | 4097 2732 | 2732 2667 | 2667 2672 | ..
#   row 3  4096 4096 | 4096 2835 | 2835 2880 | ..
#   row 4    63   63 |   63   42 |   42   41 |   41   38 | .. |   38   50 | .. |   52   35 |   35   37   (never below 6 particles)
# - counts differ between rows, rows 0 - 2 cross 4096, every row removes and duplicates, rows 0 and 1 part after the first resample.
STARTS_A = (6000, 6000, 4097, 4096, 63)


def test_seeded_batch_equals_seeded_singles(dev, cb, traj, wide):
    B, T = len(STARTS_A), 12
    singles, batch = _engines(dev, cb, B, N, 4100, floor=FLOOR)
    for b, s in enumerate(singles):
        s.set_particles(torch.as_tensor(wide[:STARTS_A[b]]))
        assert s.seed_torch_stream(S_A + b) is s.torch_stream
    batch.set_particles([torch.as_tensor(wide[:n]) for n in STARTS_A])
    streams = batch.seed_torch_streams([S_A + b for b in range(B)])
    assert streams is batch.torch_streams and batch.topk_ties == "aten_cpu"
    for t in range(T):
        _frame(singles, batch, traj, t)  # (frame 0 is the DBSCAN frame: cluster_every = 50)
    log = batch.read_log()
    sizes = [[(r["n"], r["n_after"]) for r in rows] for rows in log]
    modes = {r["mode"] for rows in log for r in rows}
    assert any(len({sizes[b][t] for b in range(B)}) > 1 for t in range(T)), sizes          # counts differ between rows
    assert any(n > 4096 >= n2 or n <= 4096 < n2 for s in sizes for n, n2 in s), sizes      # a row crosses 4096
    assert {1, 2} <= modes, modes                                                          # a removal and a duplication
    for t in range(1, T):                                                                  # rows 0 and 1: one start, two seeds
        slot = t % batch.log_frames
        assert not torch.equal(batch._log[0, slot].view(torch.int64), batch._log[1, slot].view(torch.int64)), t
    assert min(n2 for s in sizes for _, n2 in s) >= 6
    for b, s in enumerate(singles):
        assert torch.equal(_next8(lambda g: streams.to_host(b, g)), _next8(s.torch_stream.to_host)), f"trajectory {b}: generator position"
    assert not batch.ctl_i[:, 14].any() and not batch._mt_status.any()


# ---- (b) ------------------------------------------------------------------------------------------------------------------
def test_seeded_batch_replays_reference_loop_trace(dev, golden, oracle):
    """G13 as test_loop_engine_seeded_step_replays_reference_loop_trace replays it, inside a batch of two: row 0 under
    manual_seed(3000 + t) holds the reference's kept-set and resample-index digests and annealed counts in all 64 frames; row 1, the
    same particles under 5000 + t, equals a single engine driven the same way and differs from row 0."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    g = golden("g13_loop_trace")
    cb = make_codebook(K=int(g["K"]), D=int(g["D"]), seed=int(g["cb_seed"]), mesh_points=20000)
    T13, N0 = int(g["T"]), int(g["N0"])
    traj = make_trajectory(cb, T=T13 + 1, seed=int(g["traj_seed"]))
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, ties="aten_cpu")  # carries the run from frame to frame
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    batch = BatchLoopEngine(*src, 2, N0, device=dev)
    streams = batch.seed_torch_streams([0, 0])
    single = LoopEngine(*src, N0, seed=batch.seed + 1, device=dev, topk_ties="aten_cpu")
    single.seed_torch_stream(0)
    poses, labels = g["poses0"], np.zeros(N0, dtype=np.int64)
    differ, walks = 0, set()
    for t in range(1, T13 + 1):
        n, n2 = poses.shape[0], int(g[f"N2_{t}"])
        p, lb = torch.as_tensor(poses), torch.as_tensor(labels)
        var, init = float(loop.annealer.particle_var), loop.annealer.init_particles or 0
        batch.set_particles([p, p], [lb, lb], reset_annealing=False)
        batch.set_annealing_state([var, var], [init, init])
        batch.step_count = t - 1
        streams.manual_seed([3000 + t, 5000 + t])
        single.set_particles(p, lb, reset_annealing=False)
        single.set_annealing_state(var, init)
        single.step_count = t - 1
        single.torch_stream.manual_seed(5000 + t)
        dbs = (t - 1) % 50 == 0
        odom, code, gt = torch.as_tensor(traj.odoms[t]), torch.as_tensor(traj.codes[t]), torch.as_tensor(traj.gt_poses[t])
        batch.step(odom[None].repeat(2, 1, 1), code[None].repeat(2, 1), gts=gt[None].repeat(2, 1, 1), dbscan=dbs)
        single.step(odom, code, gt=gt, dbscan=dbs)
        fv = batch.frame_view(0)
        assert fv["n"] == n and fv["n_after"] == n2, t
        assert sha(fv["src"].cpu().numpy().astype(np.int32)) == str(g[f"keep_{t}_sha"]), f"frame {t}: kept set is not the reference's"
        assert sha(fv["ridx"].cpu().numpy().astype(np.int32)) == str(g[f"ridx_{t}_sha"]), f"frame {t}: resample indices are not the reference's"
        f1 = _compare([None, single], batch, t, rows=(1,))[0]
        differ += int(f1["n_after"] != n2 or not torch.equal(f1["ridx"], fv["ridx"]))
        if fv["mode"]:  # which of the walk's four cases the frame took
            walks.add((fv["mode"], fv["k"] * 64 <= n))
        torch.manual_seed(3000 + t)
        tn, rot = torch.normal(mean=0.0, std=2e-4, size=(n, 3)), torch.normal(mean=0.0, std=0.5, size=(n, 3))
        u = torch.rand(n2, dtype=torch.float64)
        ref = loop.step(poses, labels, traj.odoms[t], traj.codes[t], tn.numpy(), rot.numpy(), gt=traj.gt_poses[t], u=u.numpy())
        assert ref["N"] == n2
        poses, labels = ref["poses"], ref["labels"]
    assert differ > 0  # another seed, other resample indices
    # removal and growth, each by nth_element (k * 64 > n) and by partial_sort (k * 64 <= n)
    assert walks == {(1, False), (1, True), (2, False), (2, True)}, walks


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def test_seeded_batch_row_against_the_oracle(dev, oracle, cb, traj, wide):
    """Row 0 of three free-running trajectories from 4096 particles against OracleLoop(ties="aten_cpu") fed torch.normal / torch.rand
    of a host generator under the same seed, continuing from frame to frame: annealed counts and sets, resample indices, poses."""
    from midastouch_amd import BatchLoopEngine
    B, N0, T, s = 3, 4096, 8, 7103  # (7103: row 3 of case (a) - 4096 2835 2880 2753 2804 2803 3044 2707 .. in the reference)
    batch = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, floor=FLOOR, device=dev)
    batch.set_particles([torch.as_tensor(wide[:N0])] * B)
    batch.seed_torch_streams([s, s + 10, s + 20])
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, floor=FLOOR, ties="aten_cpu")
    gen = torch.Generator().manual_seed(s)
    poses, labels = wide[:N0], np.zeros(N0, dtype=np.int64)
    sizes = []
    for t in range(T):
        n = poses.shape[0]
        tn = torch.normal(0.0, 2e-4, size=(n, 3), generator=gen).numpy()
        rot = torch.normal(0.0, 0.5, size=(n, 3), generator=gen).numpy()
        ref = loop.step(poses, labels, traj.odoms[t + 1], traj.codes[t + 1], tn, rot, gt=traj.gt_poses[t + 1],
                        draws=lambda n2: torch.rand(n2, dtype=torch.float64, generator=gen).numpy())
        batch.step(*_operands(traj, t, B))
        fv = batch.frame_view(0)
        assert fv["n"] == n and fv["n_after"] == ref["N"], f"frame {t}: annealed size {fv['n_after']} vs {ref['N']}"
        assert np.array_equal(fv["src"].cpu().numpy(), ref["keep"]), f"frame {t}: annealed set"
        assert np.array_equal(fv["ridx"].cpu().numpy(), ref["ridx"]), f"frame {t}: resample indices"
        assert np.array_equal(fv["poses"].cpu().numpy(), ref["poses"]), f"frame {t}: resampled poses"
        poses, labels = ref["poses"], ref["labels"]
        sizes.append(ref["N"])
    assert len(set(sizes)) > 2, sizes
    assert torch.equal(_next8(lambda g: batch.torch_streams.to_host(0, g)), torch.rand(8, dtype=torch.float64, generator=gen))


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_tie_rule_alone_and_the_way_back_to_philox(dev, cb, traj, wide):
    from midastouch_amd import BatchLoopEngine
    B, N0 = 3, 3000
    starts = [torch.as_tensor(wide[:n]) for n in (3000, 2999, 1025)]
    singles, batch = _engines(dev, cb, B, N0, 610, floor=FLOOR, cluster_every=3)
    assert batch.topk_ties == "index"
    batch.topk_ties = "aten_cpu"  # Philox draws, ATen's tie rule
    for s, p in zip(singles, starts):
        s.set_particles(p)
    batch.set_particles(starts)
    modes = set()
    for t in range(6):
        modes |= {v["mode"] for v in _frame(singles, batch, traj, t)}
    assert {1, 2} & modes, modes  # the walk ran
    # seeded frames, then back: from there on the bits of a Philox batch that starts from the same state
    batch.seed_torch_streams([1, 2, 3])
    for t in range(6, 8):
        batch.step(*_operands(traj, t, B))
    assert batch.seed_torch_streams(None) is None and batch.torch_streams is None and batch.topk_ties == "index"
    fresh = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, seed=610, floor=FLOOR, cluster_every=3, device=dev)
    for name in ("ctl_i", "ctl_d", "_poses", "_hint", "_labels"):
        getattr(fresh, name).copy_(getattr(batch, name))
    fresh.step_count = batch.step_count
    for t in range(8, 11):
        ops = _operands(traj, t, B)
        batch.step(*ops)
        fresh.step(*ops)
        slot = (batch.step_count - 1) % batch.log_frames
        assert torch.equal(batch._log[:, slot].view(torch.int64), fresh._log[:, slot].view(torch.int64)), t
        for b in range(B):
            fa, fb = batch.frame_view(b), fresh.frame_view(b)
            for k in PER_PARTICLE:
                assert fa[k].shape == fb[k].shape and torch.equal(fa[k], fb[k]), (t, b, k)


# ---- (e) ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_untouched(dev, cb, traj, wide):
    from midastouch_amd import BatchLoopEngine, _lib
    from midastouch_amd._lib import MidasError
    B, n = 2, 1000
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    eng = BatchLoopEngine(*src, B, n, device=dev)
    eng.set_particles([torch.as_tensor(wide[:n])] * B)
    torch.cuda.synchronize()
    ci0, cd0 = eng.ctl_i.clone(), eng.ctl_d.clone()

    def untouched():
        torch.cuda.synchronize()
        return eng.step_count == 0 and torch.equal(eng.ctl_i, ci0) and torch.equal(eng.ctl_d, cd0) and not eng.poses_prop.any()

    for seeds in ([1], [1, 2, 3]):
        with pytest.raises(MidasError, match="seeds"):
            eng.seed_torch_streams(seeds)
    assert eng.torch_streams is None and eng.topk_ties == "index" and untouched()
    low = BatchLoopEngine(*src, B, n, resample="low_var", device=dev)
    with pytest.raises(MidasError, match="weighted_random"):
        low.seed_torch_streams([1, 2])
    assert low.torch_streams is None and low.topk_ties == "index"
    # the entry point itself
    odoms, codes, _ = _operands(traj, 0, B)
    keep = (odoms.to(dev), codes.to(dev), torch.zeros((B, n, 3), device=dev))
    a = eng._args
    a.odom16, a.code, a.score_epoch = keep[0].data_ptr(), keep[1].data_ptr(), 1
    a.labels, a.labels_out = eng._labels.data_ptr(), eng._labels_next.data_ptr()
    a.topk_ties = _lib.TOPK_TIES_ATEN_CPU
    phases, stride = 1 | 4 | 8, eng.log_frames * _lib.LOOP_LOG_DOUBLES

    def call(batch):
        eng.ctx.check(eng.ctx.lib.midas_loop_step_batch_draws(eng.ctx.h, eng.codebook.h, eng.tree6.h, eng.tree3.h, C.byref(a), phases, batch, stride))

    for field, bad, good in (("tn", keep[2].data_ptr(), None), ("cap", _lib.LOOP_BATCH_MAX_CAP + 1, n), ("grid_n", n, 0), ("anneal_frozen", 1, 0)):
        setattr(a, field, bad)
        with pytest.raises(MidasError):
            call(B)
        setattr(a, field, good)
    with pytest.raises(MidasError):
        call(0)
    assert untouched()
    a.topk_ties = _lib.TOPK_TIES_INDEX
    eng.step(odoms, codes)  # ... and the frame goes through once everything is in order
    assert eng.read_log()[1][0]["n"] == n and eng.step_count == 1


def test_a_short_draw_is_reported_for_its_trajectory(dev, cb, traj, wide):
    """A row of 5 particles (15 normal values: ATen's scalar path) beside a row of 64: read_log names trajectory 1, and only it."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, 2, 64, floor=2, device=dev)
    eng.set_particles([torch.as_tensor(wide[:64]), torch.as_tensor(wide[:5])])
    eng.seed_torch_streams([1, 2])
    eng.step(*_operands(traj, 0, 2))
    with pytest.raises(MidasError, match="trajectory 1, frame 0.*16 normal values") as e:
        eng.read_log()
    assert "trajectory 0" not in str(e.value)
    assert len(eng.read_log(rows=(0,))[0]) == 1
    with pytest.warns(UserWarning, match="16 normal values"):
        assert len(eng.read_log(strict=False)[1]) == 1


def test_seeded_batch_no_frame_allocates(dev):
    """8 trajectories of MIDAS_LOOP_BATCH_MAX_CAP particles through a DBSCAN frame and two plain ones with seeded streams: the generator's
    raw words and the walk's queues are part of what seed_torch_streams reserves - MIDAS_SCRATCH_LOG reports no chunk behind it.  (The
    switch is read once per process: a child process.)"""
    code = (
        "import sys, numpy as np, torch\n"
        "from midastouch_amd import BatchLoopEngine, _lib\n"
        "from midastouch_amd.synthetic import make_codebook, make_trajectory\n"
        "dev = torch.device('cuda', 0)\n"
        "B, cap = 8, _lib.LOOP_BATCH_MAX_CAP\n"
        "cb = make_codebook(K=2500, D=256, seed=1000)\n"
        "tr = make_trajectory(cb, T=4, seed=2000)\n"
        "eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=4000, device=dev)\n"
        "eng.seed_torch_streams(range(B))\n"
        "sys.stderr.write('MARK\\n'); sys.stderr.flush()\n"
        "rng = np.random.default_rng(0)\n"
        "eng.set_particles(torch.as_tensor(cb.poses[rng.integers(0, 2500, (B, cap))]))\n"
        "for t in range(3):\n"
        "    rep = lambda a: torch.as_tensor(a[t + 1])[None].repeat(B, *([1] * a[t + 1].ndim)).contiguous()\n"
        "    eng.step(rep(tr.odoms), rep(tr.codes), gts=rep(tr.gt_poses))\n"
        "torch.cuda.synchronize()\n"
        "print('DONE', min(eng.n), max(eng.n), len(eng.read_log()[0]))\n")
    env = dict(os.environ, MIDAS_SCRATCH_LOG="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DONE" in r.stdout
    before, after = r.stderr.split("MARK")
    assert "reserved one chunk" in before and "[midas] scratch" not in after, r.stderr
