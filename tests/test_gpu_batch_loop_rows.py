"""BatchLoopEngine with the filter's parameters per row (midas_loop_step_batch_rows: motion noise, prune threshold, annealing floor,
softmax and unit weights from a table of B records) against single LoopEngines - engine b built on row b's object with seed + b and
ROW b's parameters, stepped with row b of the operands.  After every frame, for every row: the whole log row, the frame's
per-particle arrays, the annealed and the resampled set, the cluster rows and the live counts, bit for bit.

The three objects of test_gpu_batch_loop_objects (K = 3000 / 900 / 1777, D = 128); the singles are stepped half before and half after
the batch frame, as everywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_batch_loop import PER_PARTICLE  # noqa: E402
from test_gpu_batch_loop_objects import OBJECTS, D, _near_starts, _trajs, _triple  # noqa: E402

ROW_KEYS = ("sig_t", "sig_r", "pen_max", "floor", "softmax")
# six rows, six different parameter sets (the reference's two datasets and two runners and what lies between them)
SIX = dict(sig_t=[2e-4, 1e-4, 3e-4, 2e-4, 5e-5, 4e-4], sig_r=[0.5, 0.25, 1.0, 0.3, 0.5, 0.7],
           pen_max=[0.002, 0.0025, 0.004, 0.003, 0.002, 0.001], floor=[1000, 1500, 1000, 1500, 1500, 1000],
           softmax=[True, True, True, False, True, False])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cbs():
    from midastouch_amd.synthetic import make_codebook
    return [make_codebook(name, K=K, D=D, seed=1013 + i, mesh_points=4000) for i, (name, K) in enumerate(OBJECTS)]


def _engines(dev, cbs, rows, cap, seed, params, **kw):
    """One LoopEngine per row - on its object, seed + b, ITS parameters - and the for_objects engine given the B values of each."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    single_kw = {k: v for k, v in kw.items() if k not in ("wide", "batched_dbscan")}
    singles = [LoopEngine(*_triple(cbs[i]), cap, seed=seed + b, device=dev, **{k: v[b] for k, v in params.items()}, **single_kw)
               for b, i in enumerate(rows)]
    batch = BatchLoopEngine.for_objects([_triple(c) for c in cbs], rows, cap, seed=seed, device=dev, **params, **kw)
    return singles, batch


def _start(singles, batch, starts, particle_vars=None, init=None):
    for s, p in zip(singles, starts):
        s.set_particles(torch.as_tensor(p))
    batch.set_particles([torch.as_tensor(p) for p in starts])
    if particle_vars is not None:  # annealing's memory, so that the first frame's rule acts as the test wants it to
        for s, pv in zip(singles, particle_vars):
            s.set_annealing_state(pv, init)
        batch.set_annealing_state(particle_vars, [init] * len(singles))


def _frame(singles, batch, trajs, t, unit=False, still=False):
    """Frame t of every engine and the comparison of everything it left; unit: a bool or one per row; still: the frame without
    motion noise (step_still / std_override (0, 0))."""
    B = len(singles)
    units = list(unit) if isinstance(unit, (list, tuple)) else [unit] * B
    odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
    codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
    gts = torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs]))
    first = (B + 1) // 2
    one = lambda b: singles[b].step(odoms[b], codes[b], gt=gts[b], unit_weights=units[b], std_override=(0.0, 0.0) if still else None)  # noqa: E731
    for b in range(first):
        one(b)
    (batch.step_still if still else batch.step)(odoms, codes, gts=gts, unit_weights=unit)
    for b in range(first, B):
        one(b)
    views = []
    slot = (batch.step_count - 1) % batch.log_frames
    for b in range(B):
        assert torch.equal(batch._log[b, slot].view(torch.int64), singles[b]._log[slot].view(torch.int64)), f"frame {t}, row {b}: log row"
        fs, fb = singles[b].frame_view(), batch.frame_view(b)
        assert (fb["n"], fb["n_after"]) == (fs["n"], fs["n_after"])
        for k in PER_PARTICLE:
            assert fb[k].shape == fs[k].shape and torch.equal(fb[k], fs[k]), f"frame {t}, row {b}: {k}"
        assert np.array_equal(fb["cluster_poses"], fs["cluster_poses"]) and np.array_equal(fb["cluster_stds"], fs["cluster_stds"])
        views.append(fb)
    assert batch.n == [v["n_after"] for v in views]
    return views


def test_six_rows_six_parameter_sets(dev, cbs):
    """B = 6 over the three objects, starts of 2000 .. 5000 particles, 8 frames with DBSCAN on frames 0, 3 and 6, a frame whose
    unit weights differ between the rows (4), one where all rows have them (5) and a still frame (7).  Annealing's memory is set so
    that frame 0's rule removes in rows 0 and 1 - in row 1 down to ITS floor of 1500, which the other rows' 1000 would not stop -,
    duplicates in row 2 and rests in row 4 (its third more would exceed init_particles); rows 3 and 5 weigh by raw scores, row 5
    under half the usual threshold: whatever their rule decides, it is the single engines'."""
    rows, T, seed = [0, 1, 2, 0, 1, 2], 8, 4100
    ns = [2000, 2200, 2900, 3600, 4300, 5000]
    trajs = _trajs(cbs, rows, T, 2013)
    starts = _near_starts(cbs, rows, trajs, 300, ns, 21)
    singles, batch = _engines(dev, cbs, rows, 5000, seed, SIX, cluster_every=3)
    assert batch.per_row == ROW_KEYS and batch.row_params() == SIX
    _start(singles, batch, starts, particle_vars=[1.0, 1.0, 1e-12, 1.0, 1e-12, 1.0], init=5000)
    sizes = []
    for t in range(T):
        unit = [False, True, False, True, False, False] if t == 4 else t == 5
        views = _frame(singles, batch, trajs, t, unit=unit, still=t == 7)
        sizes.append([v["n_after"] for v in views])
        if t == 0:
            assert [views[b]["mode"] for b in (0, 1, 2, 4)] == [1, 1, 2, 0], [(v["mode"], v["k"]) for v in views]
            assert views[1]["k"] == 2200 - 1500 and views[1]["n_after"] == 1500  # the row's own floor cut the removal short
            assert views[0]["k"] == 2000 // 3 and views[2]["k"] == 2900 // 3
            assert [bool(v["raw"]) for v in views] == [not s for s in SIX["softmax"]]
        if t == 4:  # unit weights: the row's weights are its prune mask over the raw sum (softmax rows: over S)
            assert [bool(v["raw"]) for v in views] == [not s or u for s, u in zip(SIX["softmax"], unit)]
    assert all(min(col) >= f for col, f in zip(zip(*sizes), SIX["floor"])) and sizes[0][1] == 1500
    # the tables: the moving frames' (frames 0-3 and 6), frame 4's, frame 5's and the still frame's - four contents, four uploads
    assert batch.row_table_uploads == 4
    assert not batch.ctl_i[:, 14].any()


def test_edge_rows(dev, cbs):
    """Beside an ordinary row: a row without motion noise (sigma 0), a row whose threshold is +inf - it keeps every particle - and a
    row that starts half a metre off its mesh: all of its particles are pruned and it goes back onto ITS object's poses (the drift
    re-projection) under its own threshold."""
    rows, N0, T, seed = [0, 1, 2, 1], 1500, 4, 510
    params = dict(sig_t=[2e-4, 0.0, 1e-4, 3e-4], sig_r=[0.5, 0.0, 0.25, 0.5], pen_max=[0.002, 0.002, float("inf"), 0.001],
                  floor=[500, 400, 600, 500], softmax=[True, True, False, True])
    trajs = _trajs(cbs, rows, T, 2013)
    starts = _near_starts(cbs, rows, trajs, 100, [N0] * 4, 6)
    starts[3] = starts[3].copy()
    starts[3][:, :3, 3] += np.float32(0.5)
    singles, batch = _engines(dev, cbs, rows, N0, seed, params, cluster_every=3)
    _start(singles, batch, starts)
    own = torch.as_tensor(cbs[1].poses).to(dev)
    for t in range(T):
        views = _frame(singles, batch, trajs, t)
        assert views[2]["kept"] == views[2]["n"]  # +inf: nothing is pruned, on any frame
        if t == 0:
            v = views[3]
            assert v["drifted"] and v["kept"] == 0 and torch.equal(v["poses_prop"], own[v["nn_idx"].long()])
            assert not any(views[b]["drifted"] for b in range(3))
            # sigma 0: the row's particles moved by the odometry alone - particles that shared a pose still do
            p0, pp = torch.as_tensor(starts[1]).to(dev), views[1]["poses_prop"]
            same = (p0[1:] == p0[:1]).flatten(1).all(dim=1)
            assert same.any() and (pp[1:][same] == pp[:1]).all()


def test_wide_rows(dev, cbs):
    """wide=True at capacity 16 448: two rows held above 16 384 by floors of 16 400 and 16 420 - the decision in front of the radix
    select reads each row's own - beside a small row with floor 1000."""
    rows, cap, T, seed = [2, 0, 1], 16448, 3, 61
    params = dict(sig_t=[2e-4, 1e-4, 2e-4], sig_r=[0.5, 0.5, 0.25], pen_max=[0.002, 0.003, 0.002], floor=[16400, 16420, 1000],
                  softmax=[True, True, False])
    trajs = _trajs(cbs, rows, T, 2070)
    starts = _near_starts(cbs, rows, trajs, 400, [cap, cap, 3000], 13)
    singles, batch = _engines(dev, cbs, rows, cap, seed, params, cluster_every=2, wide=True)
    _start(singles, batch, starts, particle_vars=[1.0, 1.0, 1.0], init=cap)
    for t in range(T):
        views = _frame(singles, batch, trajs, t, unit=[False, False, t == 1])
        if t == 0:
            assert [(v["mode"], v["k"], v["n_after"]) for v in views[:2]] == [(1, 48, 16400), (1, 28, 16420)]
    assert all(v["n_after"] > 16384 for v in views[:2])


def test_block_edges(dev, cbs):
    """The small regime either side of a 4096-slot summation block: 4095 / 4096 / 4097 particles, each row with its own softmax
    switch and unit-weight frame - the block sums and the weights of the second block's one slot."""
    rows, T, seed = [0, 1, 2], 3, 97
    params = dict(sig_t=[2e-4, 1e-4, 3e-4], sig_r=[0.5, 0.25, 0.5], pen_max=[0.002, 0.0015, 0.003], floor=[4000, 1000, 4097],
                  softmax=[False, True, True])
    trajs = _trajs(cbs, rows, T, 2090)
    starts = _near_starts(cbs, rows, trajs, 300, [4095, 4096, 4097], 15)
    singles, batch = _engines(dev, cbs, rows, 4097, seed, params, cluster_every=2)
    _start(singles, batch, starts)
    for t in range(T):
        views = _frame(singles, batch, trajs, t, unit=[t == 1, False, t == 2])
        if t == 0:
            assert [v["n"] for v in views] == [4095, 4096, 4097]


def test_set_row_params_between_frames(dev, cbs):
    """set_row_params: per-row values in, changed, made shared again and back - the singles' attributes follow (LoopEngine takes
    them on every call).  With scalars only the engine is on the shared-parameter entry: no table, no upload."""
    rows, N0, T, seed = [2, 0, 1], 1500, 8, 333
    shared = dict(sig_t=2e-4, sig_r=0.5, pen_max=0.002, floor=400, softmax=True)
    trajs = _trajs(cbs, rows, T, 2040)
    starts = _near_starts(cbs, rows, trajs, 400, [N0 - 300 * b for b in range(3)], 8)
    singles, batch = _engines(dev, cbs, rows, N0, seed, {}, cluster_every=3, **shared)
    _start(singles, batch, starts)
    steps = {2: dict(sig_t=[1e-4, 2e-4, 4e-4], floor=[400, 700, 500]), 4: dict(softmax=[True, False, True], sig_t=3e-4),
             5: dict(pen_max=[0.002, 0.001, float("inf")], sig_r=[0.1, 0.5, 1.0]), 6: dict(shared)}
    for t in range(T):
        if t == 3:  # a shared parameter set as a plain attribute, as the shared frame follows it, while others are per row: a new table
            batch.sig_r = 0.8
            for s in singles:
                s.sig_r = 0.8
        if t in steps:
            batch.set_row_params(**steps[t])
            for k, v in steps[t].items():
                for b, s in enumerate(singles):
                    setattr(s, k, v[b] if isinstance(v, list) else v)
        _frame(singles, batch, trajs, t)
        if t < 2 or t >= 6:
            assert batch.per_row == ()
    assert batch.row_table_uploads == 4  # frame 2, frame 3 (the attribute), frame 4, frame 5
    assert batch.row_params() == {k: [v] * 3 for k, v in shared.items()}


def _state(eng):
    return {attr: getattr(eng, attr).clone() for attr, *_ in eng._state}


def _same_state(x, y, skip=()):
    for attr, v in x.items():
        if attr not in skip:
            assert torch.equal(v.view(torch.uint8), y[attr].view(torch.uint8)), attr


def test_equal_rows_are_the_shared_frame(dev, cbs):
    """B equal records are the shared-parameter frame: an engine given lists of one value each (the rows entry, a table) against an
    engine given the scalars (midas_loop_step_batch_objects as ever) and against a plain one-codebook engine given per-row lists
    (it builds a one-object set of its own): every array of the state, bit for bit."""
    from midastouch_amd import BatchLoopEngine
    B, N0, T, seed = 3, 1500, 6, 77
    cb = cbs[0]
    trajs = _trajs([cb], [0] * B, T, 2030)
    starts = _near_starts([cb], [0] * B, trajs, 300, [N0, N0 - 200, N0 - 401], 4)
    kw = dict(seed=seed, device=dev, cluster_every=3)
    scalars = BatchLoopEngine.for_objects([_triple(cb)], [0] * B, N0, floor=500, pen_max=0.0015, **kw)
    lists = BatchLoopEngine.for_objects([_triple(cb)], [0] * B, N0, floor=[500] * B, pen_max=[0.0015] * B, **kw)
    plain = BatchLoopEngine(*_triple(cb), B, N0, floor=[500] * B, pen_max=0.0015, softmax=[True] * B, **kw)
    assert scalars.per_row == () and lists.per_row == ("pen_max", "floor") and plain.per_row == ("floor", "softmax") and plain._set is None
    engines = (scalars, lists, plain)
    for e in engines:
        e.set_particles([torch.as_tensor(p) for p in starts])
    for t in range(T):
        odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
        codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
        gts = torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs]))
        for e in engines:
            e.step(odoms, codes, gts=gts, unit_weights=t == 4)
        want = _state(scalars)
        for e in engines[1:]:
            _same_state(want, _state(e), skip=("telemetry", "_scores"))
            used = scalars._stamps == scalars._epoch
            assert torch.equal(scalars._scores[used].view(torch.int64), e._scores[used].view(torch.int64))
    assert scalars.row_table_uploads == 0 and scalars._row_tables == {}
    assert lists.row_table_uploads == 2 and plain.row_table_uploads == 2  # (the frame with unit weights is another content)
    assert plain._row_set is not None and plain._set is None


def test_refusals_leave_the_engine_untouched(dev, cbs):
    """Another length than B, a negative or NaN sigma, a floor below 1, per-row values together with seeded streams or the ATen tie
    rule, and - at the entry itself - no table, a misaligned table, host draws: MidasError, nothing enqueued, nothing changed; the
    frame then goes through."""
    from midastouch_amd import BatchLoopEngine, _lib
    from midastouch_amd._lib import MidasError
    rows, n = [1, 0], 1000
    trajs = _trajs(cbs, rows, 2, 2050)
    objs = [_triple(c) for c in cbs[:2]]
    for bad in (dict(sig_t=[1e-4]), dict(floor=[1, 2, 3]), dict(sig_r=[0.5, -0.1]), dict(sig_t=[float("nan"), 1e-4]), dict(floor=[0, 500]),
                dict(softmax=[True] * 3), dict(sig_t=-1e-4), dict(floor=0), dict(sig_r=torch.tensor(float("nan")))):
        with pytest.raises(MidasError):
            BatchLoopEngine.for_objects(objs, rows, n, device=dev, **bad)
    eng = BatchLoopEngine.for_objects(objs, rows, n, device=dev, sig_t=[1e-4, 2e-4], floor=[500, 600])
    eng.set_particles(_near_starts(cbs, rows, trajs, 100, [n] * 2, 9))
    odoms = torch.as_tensor(np.stack([tr.odoms[1] for tr in trajs]))
    codes = torch.as_tensor(np.stack([tr.codes[1] for tr in trajs]))
    before, params = _state(eng), eng.row_params()

    def untouched():
        torch.cuda.synchronize()
        _same_state(before, _state(eng))
        return eng.step_count == 0 and eng.n == [n, n] and eng.row_params() == params and eng._epoch == 0 and eng.row_table_uploads == 0

    for bad in (dict(sig_t=[1e-4]), dict(sig_r=[0.5, 0.5, 0.5]), dict(sig_t=-1e-4), dict(sig_r=[0.5, float("nan")]), dict(floor=0),
                dict(floor=[500, -3]), dict(pen_max=[0.002]), dict(sig_t=3e-4, floor=[500]), dict(eps=[1e-2, 1e-2]), dict(multiplier=2.0)):
        with pytest.raises(MidasError):
            eng.set_row_params(**bad)
    for bad in ([True], [True, False, True]):
        with pytest.raises(MidasError):
            eng.step(odoms, codes, unit_weights=bad)
    # a frame refused for its operands, its parameters in order: no table was built, sent or counted for it
    with pytest.raises(MidasError):
        eng.step(odoms[:1], codes)
    with pytest.raises(MidasError):
        eng.step(odoms, codes[:, :D // 2], unit_weights=[True, False])
    assert eng._row_tables == {}
    with pytest.raises(MidasError, match="shared-parameter"):
        eng.seed_torch_streams([5, 6])
    with pytest.raises(MidasError, match="shared-parameter"):
        eng.topk_ties = "aten_cpu"
    assert eng.torch_streams is None and eng.topk_ties == "index" and untouched()
    # the other way round: an engine under the ATen tie rule refuses per-row values, in set_row_params and in a frame's unit weights
    aten = BatchLoopEngine.for_objects(objs, rows, n, device=dev)
    aten.topk_ties = "aten_cpu"
    with pytest.raises(MidasError, match="ties by index"):
        aten.set_row_params(floor=[500, 600])
    with pytest.raises(MidasError, match="ties by index"):
        aten.step(odoms, codes, unit_weights=[True, False])
    assert aten.per_row == () and aten.step_count == 0
    # the entry itself
    a = eng._args
    keep = (odoms.to(dev), codes.to(dev))
    a.odom16, a.code, a.score_epoch, a.score_stamps = keep[0].data_ptr(), keep[1].data_ptr(), 1, eng._stamps.data_ptr()
    stride = eng.log_frames * _lib.LOOP_LOG_DOUBLES
    table = torch.zeros(2 * 40 + 8, dtype=torch.uint8, device=dev)

    def call(rows_ptr, B=2, wide=0):
        eng.ctx.check(eng.ctx.lib.midas_loop_step_batch_rows(eng.ctx.h, eng._set.h, C.byref(a), rows_ptr, 1 | 4 | 8, B, stride, wide))

    for kw in (dict(rows_ptr=None), dict(rows_ptr=table.data_ptr() + 4), dict(rows_ptr=table.data_ptr(), B=3),
               dict(rows_ptr=table.data_ptr(), wide=2)):
        with pytest.raises(MidasError):
            call(**kw)
    a.tn = a.rot = keep[0].data_ptr()
    with pytest.raises(MidasError):
        call(table.data_ptr())
    a.tn = a.rot = None
    a.topk_ties = _lib.TOPK_TIES_ATEN_CPU
    with pytest.raises(MidasError):
        call(table.data_ptr())
    a.topk_ties = _lib.TOPK_TIES_INDEX
    assert untouched()
    eng.step(odoms, codes)
    assert [r[0]["n"] for r in eng.read_log()] == [n, n] and eng.step_count == 1 and eng.row_table_uploads == 1
