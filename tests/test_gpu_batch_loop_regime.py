"""BatchLoopEngine over the rest of what `midas_loop_step_batch` accepts: the upper half of the regime (three and four 4096-slot
blocks per trajectory, up to MIDAS_LOOP_BATCH_MAX_CAP = 16 384 particles), the published shape (B = 64, 10 000 particles, D = 512),
the other row widths of the batch front, and every option of step() and set_particles() that LoopEngine has - the log ring, the
epoch restart and the refusals included.  The comparison is test_gpu_batch_loop's `_frame`: after every frame the log row, the
counts and every per-particle array of every compared trajectory against a LoopEngine built with seed + b, bit for bit."""
import numpy as np
import pytest

from test_gpu_batch_loop import PER_PARTICLE, _engines, _frame, _near, _start, _traj, _wide_start

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K, D = 3000, 256
BLOCK = 4096  # slots of one block of the block-order chains (k_loop_xe, k_loop_scan, k_loop_resample)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cb():
    from midastouch_amd.synthetic import make_codebook
    return make_codebook(K=K, D=D, seed=1013, mesh_points=20000)


def _near_run(dev, cb, B, N0, T, seed, tseed, rseed, m=300, step=250, **kw):
    """B trajectories (seeds tseed + b) from N0 - step * b particles near their first pose, the engines started on them."""
    trajs = [_traj(cb, T, tseed + b) for b in range(B)]
    rng = np.random.default_rng(rseed)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], m, N0 - step * b, rng) for b in range(B)]
    singles, batch = _engines(dev, cb, B, N0, seed, **kw)
    _start(singles, batch, starts)
    return trajs, singles, batch


def _same_records(got, want):
    """Two lists of read_log records, field for field (NaN equal to NaN)."""
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), (x["frame"], k)


# ---- 1. the upper half of the regime -----------------------------------------------------------------------------------
# the oracle's annealed counts (n_after of frames 0, 1, ...) of rows 0 and 1 of the two 16 384-particle scenarios, computed on the CPU
HIGH_FLOOR_COUNTS = ([16384, 15904, 14025, 12500, 12500, 12500, 12500, 12941, 12500],
                     [16384, 15616, 14733, 12500, 12500, 12500, 13743, 15335, 14399, 12500, 13013, 12855])
BOUNDARY_COUNTS = ([16384, 16150, 15654, 13502, 9002, 9553, 8870, 7066, 5029, 3353],
                   [16384, 15704, 14506, 13511, 9008, 6006, 4004],
                   [16384, 15340, 12677, 8452, 7403, 5736])


def test_high_floor_four_blocks(dev, oracle, cb):
    """B = 3 from 16 384 particles with floor 12 500, DBSCAN every 3rd frame, 12 frames: every frame of every row has more than
    12 288 live particles - four blocks per trajectory in every block-order chain, rows 12 to 15 of the one-workgroup selection -
    and row 1 grows by 1243 and 1592 duplicates and shrinks again.  Row b follows trajectory seed 2013 + b (the first 12 frames of
    a 14-frame trajectory: the one the oracle's counts above were computed on - a trajectory's measurement noise depends on its
    length) from the wide start of generator seed 11 + b.  Row 0 is held against the oracle's loop body for 8 frames (its first
    growth is frame 7; an oracle frame of 16k particles is about a second of host time), rows 1 and 2 against their single
    engines for all 12; the device's annealed counts are the oracle's.
    Measured on an MI355X machine: 3.5 to 4.0 s in three runs, most of it the eight oracle frames on its host."""
    from test_gpu_loop import _compare_frame
    B, N0, T, seed, floor = 3, 16384, 12, 4100, 12500
    TRAJ_FRAMES = 14  # the length of the trajectories the oracle's counts belong to; their first T frames are run
    trajs = [_traj(cb, TRAJ_FRAMES, 2013 + b) for b in range(B)]
    starts = [_wide_start(oracle, cb, trajs[b], N0, 11 + b) for b in range(B)]
    singles, batch = _engines(dev, cb, B, N0, seed, floor=floor, cluster_every=3)
    _start(singles, batch, starts)
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, cluster=True, cluster_every=3, floor=floor)
    poses, labels = starts[0], np.zeros(N0, dtype=np.int64)
    sizes = [[] for _ in range(B)]
    for t in range(T):
        if t < 8:
            tn, rot = oracle.philox_noise(poses.shape[0], seed, t, np.float32(2e-4), np.float32(0.5))
            ref = loop.step(poses, labels, trajs[0].odoms[t + 1], trajs[0].codes[t + 1], tn, rot, gt=trajs[0].gt_poses[t + 1],
                            mode="weighted_random", u32=None, draws=lambda n2: oracle.philox_uniform64(n2, seed, t))
            poses, labels = ref["poses"], ref["labels"]
        views = _frame(singles, batch, trajs, t)
        if t < 8:
            _compare_frame(views[0], ref, t, t % 3 == 0)
        for b in range(B):
            assert views[b]["n"] > 3 * BLOCK and views[b]["n_after"] > 3 * BLOCK, (t, b, views[b]["n"], views[b]["n_after"])
            sizes[b].append(views[b]["n_after"])
    print("annealed counts:", sizes)
    assert any(any(y > x for x, y in zip(s, s[1:])) and any(y < x for x, y in zip(s, s[1:])) for s in sizes), sizes  # a row grows and shrinks
    for b, want in enumerate(HIGH_FLOOR_COUNTS):
        assert sizes[b][:len(want)] == want[:T], (b, sizes[b])
    assert [[r["n_after"] for r in rows] for rows in batch.read_log()] == sizes
    assert not batch.ctl_i[:, 14].any()


def test_through_every_block_boundary(dev, oracle, cb):
    """The same three rows with floor 1000 and DBSCAN every 5th frame, 10 frames (of 30-frame trajectories: those of the oracle's
    counts above): every row shrinks from four blocks to one or two, row 0 across 12 288, 8192 (twice: it grows by 551 in frame
    5) and 4096.  Against single engines; the device's annealed counts are the oracle's."""
    B, N0, T, seed = 3, 16384, 10, 4100
    TRAJ_FRAMES = 30  # the length of the trajectories the oracle's counts belong to; their first T frames are run
    trajs = [_traj(cb, TRAJ_FRAMES, 2013 + b) for b in range(B)]
    starts = [_wide_start(oracle, cb, trajs[b], N0, 11 + b) for b in range(B)]
    singles, batch = _engines(dev, cb, B, N0, seed, floor=1000, cluster_every=5)
    _start(singles, batch, starts)
    sizes = [[] for _ in range(B)]
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        for b in range(B):
            sizes[b].append(views[b]["n_after"])
    print("annealed counts:", sizes)
    assert any(any(x > 2 * BLOCK and min(s[i + 1:]) < BLOCK for i, x in enumerate(s[:-1])) for s in sizes), sizes
    for b, want in enumerate(BOUNDARY_COUNTS):
        assert sizes[b][:len(want)] == want, (b, sizes[b])
    assert not batch.ctl_i[:, 14].any()


@pytest.mark.parametrize("resample", ["weighted_random", "low_var"])
def test_ragged_starts_upper_boundaries(dev, cb, resample):
    """test_ragged_starts two blocks up: capacity 16 384 with starts on either side of 8192, 12 288 and 16 384 - and once with
    the systematic resampler, whose one draw per trajectory crosses the same boundaries."""
    ns = [8191, 8192, 8193, 12287, 12288, 12289, 16383, 16384]
    B, T, seed = len(ns), 6, 77
    trajs = [_traj(cb, T, 2021 + b) for b in range(B)]
    rng = np.random.default_rng(3)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 200, ns[b], rng) for b in range(B)]
    singles, batch = _engines(dev, cb, B, 16384, seed, floor=500, cluster_every=3, resample=resample)
    _start(singles, batch, starts)
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        if t == 0:
            assert [v["n"] for v in views] == ns
    assert not batch.ctl_i[:, 14].any()


# ---- 2. the published shape, shortened -----------------------------------------------------------------------------------
def _shared_index(dev, cb):
    """One codebook index and one mesh index for any number of engines (engine.codebook_index)."""
    from midastouch_amd import ops
    from midastouch_amd.tactile_tree import tactile_tree
    tt = tactile_tree(torch.as_tensor(cb.poses).to(dev), torch.as_tensor(cb.cam_poses).to(dev), torch.as_tensor(cb.embeddings).to(dev))
    return tt, ops.Tree(torch.as_tensor(cb.mesh_vertices).to(dev, torch.float64))


def test_published_shape(dev):
    """B = 64 trajectories of 10 000 particles on a K = 5003 (no multiple of 64), D = 512 codebook - tools/bench_batch_loop.py's
    shape - for 6 frames, DBSCAN every 3rd, floor 1000: every per-trajectory slice of the scratch and grid.y up to b = 63.  Even
    rows start from 10 000 particles, odd row b from 10 000 - 37 b, so the live counts differ from the first frame on.  The 64
    single engines and the batch engine share ONE codebook index and mesh index.  Every array of rows 0, 1, 7, 8, 31, 62 and 63
    and the log row of all 64, every frame.
    Measured on an MI355X machine: 0.9 s (the codebook, the 64 trajectories and the 65 engines included)."""
    from midastouch_amd.synthetic import make_codebook
    B, N0, T, seed = 64, 10000, 6, 5200
    cb5 = make_codebook(K=5003, D=512, seed=1013, mesh_points=20000)
    trajs = [_traj(cb5, T, 3000 + b) for b in range(B)]
    rng = np.random.default_rng(12)
    ns = [N0 if b % 2 == 0 else N0 - 37 * b for b in range(B)]
    starts = [_near(cb5, trajs[b].gt_poses[0][:3, 3], 300, ns[b], rng) for b in range(B)]
    singles, batch = _engines(dev, cb5, B, N0, seed, index=_shared_index(dev, cb5), floor=1000, cluster_every=3, log_frames=8)
    assert all(s.tree6 is batch.tree6 and s.tree3 is batch.tree3 and s.codebook is batch.codebook for s in singles)
    _start(singles, batch, starts)
    rows = (0, 1, 7, 8, 31, 62, 63)
    for t in range(T):
        _frame(singles, batch, trajs, t, rows=rows)
    log = batch.read_log()
    assert [rec[0]["n"] for rec in log] == ns
    assert len({rec[-1]["n_after"] for rec in log}) > B // 2, [rec[-1]["n_after"] for rec in log]  # the rows went their own ways
    assert all(rec[-1]["n_after"] < rec[0]["n"] for rec in log)  # ... and every one of them annealed
    assert not batch.ctl_i[:, 14].any()


@pytest.mark.parametrize("Kc,Dc", [(1030, 128), (1030, 1024)])
def test_front_row_widths(dev, Kc, Dc):
    """The other two row widths k_front_small's batch form scores (D = 128 and 1024; 256 and 512 above), K no multiple of 64,
    B = 9 - one row beyond eight."""
    from midastouch_amd.synthetic import make_codebook
    cbs = make_codebook(K=Kc, D=Dc, seed=1013, mesh_points=20000)
    B, T = 9, 5
    trajs, singles, batch = _near_run(dev, cbs, B, 2500, T, 640, 3100, 13, m=200, step=111, floor=600, cluster_every=2)
    for t in range(T):
        _frame(singles, batch, trajs, t)
    assert not batch.ctl_i[:, 14].any()


# ---- 3. everything step() and set_particles() accept -------------------------------------------------------------------------
def test_host_u32(dev, cb):
    """The systematic resampler with the host's draw on even frames (u32 = 0.37, shared by all rows as B single engines given it
    share it) and the device's (keyed seed + b) on odd ones."""
    B, T = 3, 8
    trajs, singles, batch = _near_run(dev, cb, B, 2500, T, 333, 2040, 8, floor=600, cluster_every=3, resample="low_var")
    for t in range(T):
        _frame(singles, batch, trajs, t, u32=0.37 if t % 2 == 0 else -1.0)
    assert not batch.ctl_i[:, 14].any()


def test_multiplier(dev, cb):
    """Motion noise three times as wide on every third frame."""
    B, T = 3, 9
    trajs, singles, batch = _near_run(dev, cb, B, 2500, T, 334, 2043, 9, floor=600, cluster_every=3)
    for t in range(T):
        _frame(singles, batch, trajs, t, multiplier=3.0 if t % 3 == 0 else 1.0)
    assert not batch.ctl_i[:, 14].any()


def test_forced_dbscan(dev, cb):
    """DBSCAN forced on frames the cadence (every 4th) skips, and off on one it takes."""
    B, T = 4, 8
    trajs, singles, batch = _near_run(dev, cb, B, 3000, T, 335, 2046, 10, floor=600, cluster_every=4)
    for t in range(T):
        _frame(singles, batch, trajs, t, dbscan={1: True, 4: False, 6: True}.get(t))
    assert not batch.ctl_i[:, 14].any()


def test_no_ground_truth(dev, cb):
    """A whole run without ground truth (`part_rmse` NULL): the log's rmse fields hold what the single engines' hold, as bits."""
    B, T = 3, 6
    trajs, singles, batch = _near_run(dev, cb, B, 2500, T, 336, 2049, 11, floor=600, cluster_every=3)
    for t in range(T):
        _frame(singles, batch, trajs, t, gt=False)
    _same_records(sum(batch.read_log(), []), sum((s.read_log() for s in singles), []))
    assert not batch.ctl_i[:, 14].any()


def test_given_labels(dev, cb):
    """set_particles(labels=...): row 0 on test_different_cluster_counts' two separated clouds with labels 0 / 1, row 1 with labels
    0 / 1 / 2 on one cloud, row 2 with the default.  cluster_every = 50 and frame 0's DBSCAN (0 % 50 == 0) switched off by
    dbscan=False: no DBSCAN frame replaces the given labels within the six frames."""
    B, N0, T, seed = 3, 1500, 6, 510
    trajs = [_traj(cb, T, 2013 + b) for b in range(B)]
    t3 = cb.poses[:, :3, 3]
    far = t3[int(np.argmax(np.linalg.norm(t3 - trajs[0].gt_poses[0][:3, 3], axis=1)))]
    rng = np.random.default_rng(5)
    two = np.concatenate([_near(cb, trajs[0].gt_poses[0][:3, 3], 50, N0 // 2, rng), _near(cb, far, 50, N0 - N0 // 2, rng)])
    starts = [torch.as_tensor(p) for p in [two] + [_near(cb, trajs[b].gt_poses[0][:3, 3], 50, N0, rng) for b in range(1, B)]]
    labels = [torch.arange(N0) // (N0 // 2), torch.arange(N0) % 3, None]
    singles, batch = _engines(dev, cb, B, N0, seed, floor=500, cluster_every=50)
    for s, p, lb in zip(singles, starts, labels):
        s.set_particles(p, labels=lb)
    batch.set_particles(starts, labels=labels[:2] + [torch.zeros(N0)])  # (a batch takes B label sets or none: zeros are the default)
    for t in range(T):
        views = _frame(singles, batch, trajs, t, dbscan=False if t == 0 else None)
        if t == 0:
            assert [v["ncl"] for v in views] == [2, 3, 1]
    assert not batch.ctl_i[:, 14].any()


def test_restart_in_mid_run(dev, cb):
    """Five frames, set_particles with new starts of other sizes on the batch and on the singles, five more - with the stamps,
    scores and hints of the first run behind them.  The second half is also held against FRESH single engines: set_particles
    starts annealing over, empties the hints and zeroes the labels, and stale stamps never equal a later epoch, so all that a
    restarted engine keeps is its frame counter - the Philox counter and the DBSCAN cadence.  A fresh engine is given that counter
    (`step_count`, its public attribute) and nothing else; its per-particle arrays, counts and log rows are then the restarted
    engines'."""
    from midastouch_amd.loop_engine import LoopEngine
    B, N0, T, seed = 3, 3000, 5, 337
    trajs = [_traj(cb, 2 * T, 2052 + b) for b in range(B)]
    rng = np.random.default_rng(14)
    first = [_near(cb, trajs[b].gt_poses[0][:3, 3], 300, N0 - 400 * b, rng) for b in range(B)]
    again = [_near(cb, trajs[b].gt_poses[T][:3, 3], 300, 1800 + 600 * b, rng) for b in range(B)]
    singles, batch = _engines(dev, cb, B, N0, seed, floor=600, cluster_every=3)
    _start(singles, batch, first)
    for t in range(T):
        _frame(singles, batch, trajs, t)
    _start(singles, batch, again)
    fresh = [LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0, seed=seed + b, floor=600, cluster_every=3, device=dev) for b in range(B)]
    for f, p in zip(fresh, again):
        f.step_count = T
        f.set_particles(torch.as_tensor(p))
    for t in range(T, 2 * T):
        views = _frame(singles, batch, trajs, t)
        for b, f in enumerate(fresh):
            f.step(torch.as_tensor(trajs[b].odoms[t + 1]), torch.as_tensor(trajs[b].codes[t + 1]), gt=torch.as_tensor(trajs[b].gt_poses[t + 1]))
            ff = f.frame_view()
            assert (views[b]["n"], views[b]["n_after"]) == (ff["n"], ff["n_after"]), f"frame {t}, trajectory {b}: fresh engine"
            for k in PER_PARTICLE:
                assert torch.equal(views[b][k], ff[k]), f"frame {t}, trajectory {b}: {k} of a fresh engine"
            assert torch.equal(batch._log[b, t].view(torch.int64), f._log[t].view(torch.int64)), f"frame {t}, trajectory {b}: fresh engine's log row"
    assert not batch.ctl_i[:, 14].any()


def test_project_to_codebook(dev, oracle, cb):
    """A start off the codebook (init_filter's composition without its projection): project_to_codebook() leaves every row the
    poses and hints it leaves the single engines, and the frames go on from there."""
    from midastouch_amd.synthetic import mesh_scale
    B, N0, T, seed = 3, 2500, 4, 338
    trajs = [_traj(cb, T, 2055 + b) for b in range(B)]
    sc, starts = mesh_scale(cb.extents), []
    for b in range(B):
        g = torch.Generator().manual_seed(21 + b)
        n = N0 - 300 * b
        tn0 = torch.normal(0.0, sc / 3.0 * 0.15, size=(n, 3), generator=g).numpy()
        rot0 = torch.normal(0.0, 60.0 * 0.15, size=(n, 3), generator=g).numpy()
        starts.append(oracle.init_filter_compose(trajs[b].gt_poses[0], tn0, rot0))
    singles, batch = _engines(dev, cb, B, N0, seed, floor=600, cluster_every=2)
    _start(singles, batch, starts)
    for s in singles:
        s.project_to_codebook()
    batch.project_to_codebook()
    moved = 0
    for b, s in enumerate(singles):
        n = len(starts[b])
        assert torch.equal(batch._poses[b, :n], s._poses[:n]) and torch.equal(batch._hint[b], s._hint)
        assert int(batch._hint[b, :n].min()) >= 0 and bool((batch._hint[b, n:] == -1).all())
        moved += int((batch._poses[b, :n] != torch.as_tensor(starts[b]).to(dev)).flatten(1).any(1).sum())
    assert moved > 0  # the start was off the codebook
    for t in range(T):
        _frame(singles, batch, trajs, t)
    assert not batch.ctl_i[:, 14].any()


def test_log_ring(dev, cb):
    """A log ring of four frames run for ten: read_log() gives frames 6 to 9 of every row, read_log(first, last, rows=...) those
    rows in the order asked for, and frame 9's view reads slot 1."""
    B, T = 3, 10
    trajs, singles, batch = _near_run(dev, cb, B, 2000, T, 339, 2058, 15, floor=600, cluster_every=3, log_frames=4)
    assert batch._log.shape[1] == 4 and all(s._log.shape[0] == 4 for s in singles)
    for t in range(T):
        _frame(singles, batch, trajs, t)
    log = batch.read_log()
    assert len(log) == B
    for b in range(B):
        assert [r["frame"] for r in log[b]] == [6, 7, 8, 9]
        _same_records(log[b], singles[b].read_log())
    some = batch.read_log(7, 9, rows=(2, 0))
    assert len(some) == 2
    for got, b in zip(some, (2, 0)):
        assert [r["frame"] for r in got] == [7, 8]
        _same_records(got, singles[b].read_log(7, 9))
    for b in range(B):
        fv = batch.frame_view(b)
        assert fv["frame"] == 9 and int(batch._log[b, 1, 0]) == 9  # slot 9 % 4 holds frame 9's row (its first field: the frame count) ...
        assert (fv["n"], fv["n_after"]) == (int(batch._log[b, 1, 1]), int(batch._log[b, 1, 2])) == (log[b][3]["n"], log[b][3]["n_after"])
        assert int(batch._log[b, 2, 0]) == 6  # ... and the slot behind it frame 6's


def test_epoch_restart(dev, cb):
    """advance_epoch's restart of the (B, K) stamps, the batch counterpart of test_epoch_wrap_restarts_stamps_and_lists: a batch
    engine and a set of singles four epochs before the limit, beside a second batch engine left alone - eight frames, every one bit
    for bit, the restart in the fourth."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.engine import EPOCH_LIMIT
    B, N0, T, seed = 3, 2500, 8, 340
    trajs, singles, batch = _near_run(dev, cb, B, N0, T, seed, 2061, 16, floor=600, cluster_every=3)
    other = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, seed=seed, floor=600, cluster_every=3, device=dev)
    other.set_particles([batch._poses[b, :n].clone() for b, n in enumerate(batch.n)])
    for e in singles + [batch]:
        e._epoch = EPOCH_LIMIT - 4
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        other.step(*(torch.as_tensor(np.stack([getattr(tr, k)[t + 1] for tr in trajs])) for k in ("odoms", "codes")),
                   gts=torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs])))
        assert torch.equal(other._log[:, t].view(torch.int64), batch._log[:, t].view(torch.int64)), f"frame {t}: log rows of the engine left alone"
        for b in range(B):
            fo = other.frame_view(b)
            for k in PER_PARTICLE:
                assert torch.equal(fo[k], views[b][k]), f"frame {t}, trajectory {b}: {k} of the engine left alone"
        assert 0 < batch._epoch < EPOCH_LIMIT
    assert all(0 < e._epoch < 100 for e in singles + [batch]) and other._epoch == T  # restarted
    assert not batch.ctl_i[:, 14].any()


def test_refused_codebooks(dev, cb):
    """A codebook that cannot be scored sparsely - float64 rows that float32 does not hold, D outside {128, 256, 512, 1024} - is
    refused at construction."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    e64 = cb.embeddings.astype(np.float64) * (1.0 + 1e-9)  # not float32-representable: stays float64 in HBM (test_score_codebook)
    with pytest.raises(MidasError):
        BatchLoopEngine(cb.poses, e64, cb.mesh_vertices, 3, 1000, device=dev)
    rng = np.random.default_rng(100)
    e100 = rng.standard_normal((K, 100)).astype(np.float32)
    e100 /= np.linalg.norm(e100, axis=1, keepdims=True)
    with pytest.raises(MidasError):
        BatchLoopEngine(cb.poses, e100, cb.mesh_vertices, 3, 1000, device=dev)


def test_refused_calls_change_nothing(dev, cb):
    """frame_view before a frame, frame_view(B) and set_particles with a wrong number of label sets or of labels raise and leave
    the control blocks and the particles as they were."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    B, n = 3, 800
    tr = _traj(cb, 2, 2064)
    rng = np.random.default_rng(17)
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, n, seed=341, floor=300, device=dev)
    eng.set_particles([_near(cb, tr.gt_poses[0][:3, 3], 100, n - 100 * b, rng) for b in range(B)])
    state = lambda: [x.clone() for x in (eng.ctl_i, eng.ctl_d, eng._poses, eng._labels, eng._hint)]  # noqa: E731
    other = [torch.as_tensor(_near(cb, tr.gt_poses[0][:3, 3], 100, m, rng)) for m in (10, 20, 30)]

    def refused(no_frame_yet=False):
        before = state()
        if no_frame_yet:
            with pytest.raises(MidasError):
                eng.frame_view(0)
        with pytest.raises(MidasError):
            eng.frame_view(B)
        with pytest.raises(MidasError):
            eng.frame_view(-1)
        with pytest.raises(MidasError):
            eng.set_particles(other, labels=[torch.zeros(10), torch.zeros(20)])
        with pytest.raises(MidasError):
            eng.set_particles(other, labels=[torch.zeros(10), torch.zeros(20), torch.zeros(29)])
        for x, y in zip(before, state()):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))

    refused(no_frame_yet=True)
    rep = lambda a: torch.as_tensor(a)[None].repeat(B, *([1] * a.ndim)).contiguous()  # noqa: E731
    eng.step(rep(tr.odoms[1]), rep(tr.codes[1]))
    assert eng.frame_view(B - 1)["n"] == n - 100 * (B - 1)
    refused()
    eng.step(rep(tr.odoms[2]), rep(tr.codes[2]))
    assert all(rec[0]["err"] == 0 for rec in eng.read_log(1, 2))
