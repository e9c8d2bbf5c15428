"""BatchLoopEngine.for_objects (midas_loop_step_batch_objects: the rows of one batch on different objects) against single
LoopEngines - engine b built on row b's object with seed + b and the same settings, stepped with row b of the operands.  After
every frame, for every row: the whole log row, the frame's per-particle arrays, the annealed and the resampled set, the cluster
rows and the live counts, bit for bit (test_gpu_batch_loop._frame: half of the singles step before the batch frame, half after).

Three synthetic objects of different extents and codebook sizes, D = 128: scores and stamps are (B, 3000) and a row on the mug
uses the first 900 slots of its rows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OBJECTS = (("004_sugar_box", 3000), ("025_mug", 900), ("cotter-pin", 1777))
D = 128


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cbs():
    from midastouch_amd.synthetic import make_codebook
    return [make_codebook(name, K=K, D=D, seed=1013 + i, mesh_points=4000) for i, (name, K) in enumerate(OBJECTS)]


def _triple(cb):
    return (cb.poses, cb.embeddings, cb.mesh_vertices)


def _engines(dev, cbs, rows, cap, seed, single_kw=None, **kw):
    """One LoopEngine per row (on its object, seed + b) and the for_objects engine over `cbs`."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    singles = [LoopEngine(*_triple(cbs[i]), cap, seed=seed + b, device=dev, **{k: v for k, v in kw.items() if k not in ("wide", "batched_dbscan")},
                          **(single_kw or {})) for b, i in enumerate(rows)]
    batch = BatchLoopEngine.for_objects([_triple(c) for c in cbs], rows, cap, seed=seed, device=dev, **kw)
    assert batch.row_object == list(rows) and batch.Ks == [c.poses.shape[0] for c in cbs] and batch.K == max(batch.Ks)
    assert batch._scores.shape == (len(rows), batch.K) and batch._stamps.shape == (len(rows), batch.K)
    return singles, batch


def _trajs(cbs, rows, T, seed0):
    from test_gpu_batch_loop import _traj
    return [_traj(cbs[i], T, seed0 + b) for b, i in enumerate(rows)]


def _near_starts(cbs, rows, trajs, m, ns, seed):
    from test_gpu_batch_loop import _near
    rng = np.random.default_rng(seed)
    return [_near(cbs[i], trajs[b].gt_poses[0][:3, 3], min(m, cbs[i].poses.shape[0]), ns[b], rng) for b, i in enumerate(rows)]


def test_free_running(dev, cbs):
    """B = 7 rows interleaved over the three objects from the reference's wide start (narrowed to 15 % like
    test_free_running_batch's), projected onto each row's own codebook by project_to_codebook(); 12 frames, DBSCAN every 3rd."""
    from midastouch_amd.synthetic import wide_start
    from test_gpu_batch_loop import _frame, _start
    rows, N0, T, seed = [0, 1, 2, 0, 1, 2, 2], 1500, 12, 4100
    trajs = _trajs(cbs, rows, T, 2013)
    starts = [wide_start(tuple(0.15 * e for e in cbs[i].extents), trajs[b].gt_poses[0], N0, 11 + b) for b, i in enumerate(rows)]
    singles, batch = _engines(dev, cbs, rows, N0, seed, floor=400, cluster_every=3)
    _start(singles, batch, starts)
    for s in singles:
        s.project_to_codebook()
    batch.project_to_codebook()
    for b, s in enumerate(singles):  # every row onto its own object's codebook
        assert torch.equal(batch._poses[b], s._poses) and torch.equal(batch._hint[b], s._hint), b
    sizes, nn_max = [[] for _ in rows], [0] * len(rows)
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        for b, v in enumerate(views):
            sizes[b].append(v["n_after"])
            nn_max[b] = max(nn_max[b], int(singles[b].frame_view()["nn_idx"].max()))
    # (conditions on the singles' results, the reference here)
    assert any(len({sizes[b][t] for b in range(len(rows))}) > 1 for t in range(T)), sizes  # two rows' live counts differ at some frame
    assert any(min(s) < N0 for s in sizes), sizes  # some row shrinks
    # a row read against another object's codebook would show: indices beyond the smaller codebooks are in use
    assert max(nn_max[b] for b, i in enumerate(rows) if i == 0) >= 1777, nn_max
    assert max(nn_max[b] for b, i in enumerate(rows) if i == 2) >= 900, nn_max
    assert all(nn_max[b] < batch.Ks[i] for b, i in enumerate(rows)), nn_max
    assert [[r["n_after"] for r in rr] for rr in batch.read_log()] == sizes
    assert not batch.ctl_i[:, 14].any()  # no limit / bound error flagged


@pytest.mark.parametrize("drift_row,rows", [(2, [0, 2, 1]), (0, [1, 0, 2])], ids=["row2", "row0"])
def test_all_pruned_row(dev, cbs, drift_row, rows):
    """A row on object 1 starts half a metre off its mesh: every particle is pruned in the first frame, the row reports `drifted`
    and goes back onto poses of ITS codebook (filter.py:176-179) - the per-row table of poses for a row that is not row 0, the
    pointer handed over as `cb_poses` for one that is."""
    from test_gpu_batch_loop import _frame, _start
    N0, T, seed = 1500, 6, 510
    assert rows[drift_row] == 1
    trajs = _trajs(cbs, rows, T, 2013)
    starts = _near_starts(cbs, rows, trajs, 100, [N0] * 3, 6)
    starts[drift_row] = starts[drift_row].copy()
    starts[drift_row][:, :3, 3] += np.float32(0.5)
    singles, batch = _engines(dev, cbs, rows, N0, seed, floor=500, cluster_every=3)
    _start(singles, batch, starts)
    own = torch.as_tensor(cbs[1].poses).to(dev)
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        if t == 0:
            v = views[drift_row]
            assert v["drifted"] and v["kept"] == 0 and v["status"] == 1
            assert all(not views[b]["drifted"] for b in range(3) if b != drift_row)
            assert torch.equal(v["poses_prop"], own[v["nn_idx"].long()])  # back on its own object's poses


def test_one_object_equals_plain_engine(dev, cbs):
    """for_objects([obj], [0] * B) is BatchLoopEngine(obj, B): the same bits in every array of the state, 8 frames."""
    from midastouch_amd import BatchLoopEngine
    B, N0, T, seed = 3, 1500, 8, 77
    cb = cbs[0]
    trajs = _trajs([cb], [0] * B, T, 2030)
    starts = _near_starts([cb], [0] * B, trajs, 300, [N0, N0 - 200, N0 - 401], 4)
    plain = BatchLoopEngine(*_triple(cb), B, N0, seed=seed, device=dev, floor=500, cluster_every=3)
    objs = BatchLoopEngine.for_objects([_triple(cb)], [0] * B, N0, seed=seed, device=dev, floor=500, cluster_every=3)
    for e in (plain, objs):
        e.set_particles([torch.as_tensor(p) for p in starts])
    for t in range(T):
        odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
        codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
        gts = torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs]))
        plain.step(odoms, codes, gts=gts)
        objs.step(odoms, codes, gts=gts)
        for attr, _, _, dt, _ in plain._state:
            if attr in ("telemetry", "_stamps", "_scores"):  # (stamps and scores: compared below, where the frame used them)
                continue
            x, y = getattr(plain, attr), getattr(objs, attr)
            bits = {8: torch.int64, 4: torch.int32, 1: torch.uint8}[x.element_size()]
            assert torch.equal(x.view(bits), y.view(bits)), f"frame {t}: {attr}"
        assert torch.equal(plain._stamps, objs._stamps)
        used = plain._stamps == plain._epoch
        assert torch.equal(plain._scores[used].view(torch.int64), objs._scores[used].view(torch.int64))
        assert plain.n == objs.n


@pytest.mark.parametrize("kw", [dict(resample="low_var"), dict(cluster=False), dict(softmax=False)], ids=["low_var", "no_cluster", "raw_scores"])
def test_settings(dev, cbs, kw):
    """test_gpu_batch_loop.test_settings on three objects: the systematic resampler, frames without clustering, raw scores with a
    frame of unit weights on every third frame."""
    from test_gpu_batch_loop import _frame, _start
    rows, N0, T, seed = [2, 0, 1], 1500, 9, 333
    trajs = _trajs(cbs, rows, T, 2040)
    starts = _near_starts(cbs, rows, trajs, 400, [N0 - 300 * b for b in range(3)], 8)
    singles, batch = _engines(dev, cbs, rows, N0, seed, floor=400, cluster_every=3, **kw)
    _start(singles, batch, starts)
    for t in range(T):
        _frame(singles, batch, trajs, t, unit_weights=("softmax" in kw and t % 3 == 2))


def test_seeded(dev, cbs):
    """seed_torch_streams([5, 6, 7]) on two objects against LoopEngine(topk_ties="aten_cpu") with seed_torch_stream."""
    from test_gpu_batch_loop import _frame, _start
    rows, N0, T, seeds = [1, 0, 1], 1500, 6, [5, 6, 7]
    trajs = _trajs(cbs, rows, T, 2060)
    starts = _near_starts(cbs, rows, trajs, 300, [N0] * 3, 12)
    singles, batch = _engines(dev, cbs[:2], rows, N0, 900, single_kw=dict(topk_ties="aten_cpu"), floor=500, cluster_every=3)
    _start(singles, batch, starts)
    for s, sd in zip(singles, seeds):
        s.seed_torch_stream(sd)
    batch.seed_torch_streams(seeds)
    assert batch.topk_ties == "aten_cpu"
    for t in range(T):
        _frame(singles, batch, trajs, t)


def test_wide(dev, cbs):
    """wide=True at capacity 16 448 - one wave beyond the small-set regime - starting full, on two objects."""
    from test_gpu_batch_loop import _frame, _start
    rows, cap, T, seed = [2, 0], 16448, 4, 61
    trajs = _trajs(cbs, rows, T, 2070)
    starts = _near_starts(cbs, rows, trajs, 400, [cap] * 2, 13)
    singles, batch = _engines(dev, cbs, rows, cap, seed, floor=5000, cluster_every=2, wide=True)
    _start(singles, batch, starts)
    for t in range(T):
        _frame(singles, batch, trajs, t)


def test_batched_and_serial_dbscan(dev, cbs):
    """batched_dbscan=False beside the default: the same bits, both equal to the singles'."""
    from midastouch_amd import BatchLoopEngine
    from test_gpu_batch_loop import PER_PARTICLE, _frame, _start
    rows, N0, T, seed = [1, 2, 0], 1500, 6, 444
    trajs = _trajs(cbs, rows, T, 2080)
    starts = _near_starts(cbs, rows, trajs, 200, [N0, N0 - 100, N0 - 333], 14)
    singles, batch = _engines(dev, cbs, rows, N0, seed, floor=500, cluster_every=2)
    serial = BatchLoopEngine.for_objects([_triple(c) for c in cbs], rows, N0, seed=seed, device=dev, floor=500, cluster_every=2,
                                         batched_dbscan=False)
    assert batch.batched_dbscan and not serial.batched_dbscan
    _start(singles, batch, starts)
    serial.set_particles([torch.as_tensor(p) for p in starts])
    for t in range(T):
        odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
        codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
        gts = torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs]))
        serial.step(odoms, codes, gts=gts)
        _frame(singles, batch, trajs, t)
        slot = t % batch.log_frames
        assert torch.equal(serial._log[:, slot].view(torch.int64), batch._log[:, slot].view(torch.int64)), t
        for b in range(len(rows)):
            fa, fb = serial.frame_view(b), batch.frame_view(b)
            for k in PER_PARTICLE:
                assert torch.equal(fa[k], fb[k]), (t, b, k)


def test_refusals_on_the_device(dev, cbs):
    """A float64 codebook among the objects (through for_objects and at midas_object_set_create itself), a row index the entry is
    handed directly, a set_particles call with the wrong number of rows, a step whose B is not the set's: MidasError, and the
    engine that stands beside them - its state, its device arrays - is as it was; the frame then goes through."""
    from midastouch_amd import BatchLoopEngine, _lib, ops
    from midastouch_amd._lib import MidasError
    rows, n = [1, 0], 1000
    trajs = _trajs(cbs, rows, 2, 2050)
    eng = BatchLoopEngine.for_objects([_triple(c) for c in cbs[:2]], rows, n, device=dev)
    eng.set_particles(_near_starts(cbs, rows, trajs, 100, [n] * 2, 9))
    odoms = torch.as_tensor(np.stack([tr.odoms[1] for tr in trajs]))
    codes = torch.as_tensor(np.stack([tr.codes[1] for tr in trajs]))
    before = {attr: getattr(eng, attr).clone() for attr, *_ in eng._state}

    def untouched():
        torch.cuda.synchronize()
        return eng.step_count == 0 and eng.n == [n, n] and all(torch.equal(getattr(eng, a).view(torch.uint8), v.view(torch.uint8)) for a, v in before.items())

    lossy = cbs[1].embeddings.astype(np.float64) + 1e-12  # not float32-representable: the codebook stays float64
    with pytest.raises(MidasError, match="float32"):
        BatchLoopEngine.for_objects([_triple(cbs[0]), (cbs[1].poses, lossy, cbs[1].mesh_vertices)], rows, n, device=dev)
    cb64 = ops.Codebook(torch.as_tensor(lossy).to(dev))
    assert cb64.emb.dtype == torch.float64
    o1 = eng.objects[1]
    bad = [o1, type(o1)(cb_poses=o1.cb_poses, tree6=o1.tree6, tree3=o1.tree3, codebook=cb64)]
    with pytest.raises(MidasError, match="not float32"):
        ops.ObjectSet(eng.ctx, bad, rows)
    with pytest.raises(MidasError, match=r"outside \[0, n_obj\)"):
        ops.ObjectSet(eng.ctx, eng.objects, [0, 2])
    with pytest.raises(MidasError):
        eng.set_particles([trajs[0].gt_poses[:1]])  # one set for two rows
    with pytest.raises(MidasError):
        eng.set_particles(torch.zeros(3, 10, 4, 4))
    assert untouched()
    # the step entry: a batch size that is not the set's, a regime flag that is none, host draws on the wide regime
    a = eng._args
    keep = (odoms.to(dev), codes.to(dev))
    a.odom16, a.code, a.score_epoch = keep[0].data_ptr(), keep[1].data_ptr(), 1
    a.labels, a.labels_out = eng._labels.data_ptr(), eng._labels_next.data_ptr()
    stride = eng.log_frames * _lib.LOOP_LOG_DOUBLES

    def call(B, wide):
        eng.ctx.check(eng.ctx.lib.midas_loop_step_batch_objects(eng.ctx.h, eng._set.h, C.byref(a), 1 | 4 | 8, B, stride, wide))

    for B, wide in ((1, 0), (3, 0), (2, 2)):
        with pytest.raises(MidasError):
            call(B, wide)
    a.tn = a.rot = keep[0].data_ptr()
    with pytest.raises(MidasError):
        call(2, 1)
    a.tn = a.rot = None
    assert untouched()
    eng.step(odoms, codes)  # ... and the frame goes through once everything is in order
    assert [r[0]["n"] for r in eng.read_log()] == [n, n] and eng.step_count == 1
