"""The systematic offset from DEVICE memory (u32 = MIDAS_U32_FROM_U: the first double of a trajectory's row of uniforms), at every
site that forms it - k_search, the loop engines' k_loop_resample, the tails k_tail_b / k_tail_b2, the folded resample of the
pipelined fronts (lazy_source in k_frame_front, k_frame_front_a, k_presort_fused, k_presort_search) - against THE SAME SITE with the
same value passed as the host's `u32`: index for index.  The rule itself (which slot a location selects) is pinned by
tests/test_gpu_resample_pin.py on the host-offset form; here the two sources must agree, and a batch's rows must each take THEIR
offset: B = 3 rows with three different values, every row equal to its own single run.

Offsets: 0, the largest float32 below 1 (the largest value torch.rand(1) returns), an ordinary value, and 1.25 - a value that WRAPS the
last locations (loc >= 1 -> loc - 1).  torch.rand(1) itself never wraps one: fl32(r / N) + (N - 1) / N stays below 1 for every float32
r < 1 at these sizes (checked below for the sizes used), but `u32` is also a caller's number, and the branch is the kernels' own.
Sizes: 1, 255 | 256 | 257, 4095 | 4096 | 4097 (one summation block and the slot past it).  Needs an MI355X."""
import numpy as np
import pytest

from _recipes import expected_slots, recipe_weights, systematic_locs, tie_weights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BELOW1 = float(np.nextafter(np.float32(1), np.float32(0)))
PLAIN, WRAP = 0.37, 1.25
OFFSETS = (0.0, BELOW1, PLAIN, WRAP)
ROWS = ((0.0, BELOW1, WRAP), (PLAIN, WRAP, 0.0), (BELOW1, PLAIN, PLAIN))  # three rows, three different offsets (and one repeat)
SIZES = (1, 255, 256, 257, 4095, 4096, 4097)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _pin():
    import test_gpu_resample_pin as pin  # the frames and the world of the search's pin (imported, not edited)
    return pin


def _t(a, dev, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).to(dev)


def _row(N, r, dev):
    """A single trajectory's row of uniforms with the offset in its first double (the rest is never read: poisoned)."""
    u = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
    u[0] = float(np.float32(r))
    return u


def test_offsets_of_the_test():
    """What the module's docstring says about its values: 1.25 wraps, the largest float32 below 1 does not (at the sizes used)."""
    for N in SIZES + (9000, 10241):
        assert systematic_locs(N, BELOW1)[-1] >= systematic_locs(N, BELOW1)[0]
        loc = np.arange(N) / float(N) + np.float64(np.float32(WRAP) / np.float32(N))
        assert loc[-1] >= 1.0 and systematic_locs(N, WRAP)[-1] < 1.0


# ---- k_search --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_resample_search(dev, oracle, N):
    """ops.resample_search on crafted CDFs (flat runs, ties, a masked recipe), M = N, 1 and 2 N: the offset read from u_dev[0] gives the
    host offset's indices - and numpy's upper bound over the restated locations."""
    from midastouch_amd import _lib, ops
    rng = np.random.default_rng([N, 19])
    sets = {"random": rng.random(N), "tie half": tie_weights(N, "half").astype(np.float64)}
    if N >= 4:
        w = rng.random(N)
        w[: max(N // 5, 1)] = 0.0
        w[N - max(N // 9, 1):] = 0.0
        sets["zero runs"] = w
        sets["masked recipe"] = recipe_weights(N, "masked", 5)
    for name, w in sets.items():
        c_dev, status = ops.cdf(_t(w, dev))
        assert int(status.item()) == 0
        c = c_dev.cpu().numpy()
        for M in (N, 1, 2 * N):
            for r in OFFSETS:
                host = ops.resample_search(c_dev, M, _lib.RESAMPLE_SYSTEMATIC, u32=r)
                got = ops.resample_search(c_dev, M, _lib.RESAMPLE_SYSTEMATIC, u=_row(1, r, dev), u32=_lib.U32_FROM_U)
                assert torch.equal(got, host), f"k_search {name} N={N} M={M} u32={r}"
                assert np.array_equal(got.cpu().numpy(), expected_slots(c, systematic_locs(M, r), True)), f"k_search {name} N={N} M={M} u32={r}"
    # Locations ON the table: a CDF made of the restated locations themselves and the values one step above them - every location
    # equals an entry (the upper bound takes the slot behind it) and sits one step below the next.  The offset is fl32(r / M)
    # (particle_filter.py:291: a float32 tensor over an int); the float64 quotient is another number, which moves most locations
    # off their entries - the case that tells the two apart.
    for M in (N, 2 * N):
        for r in (PLAIN, BELOW1):
            locs = systematic_locs(M, r)
            c = np.unique(np.concatenate([locs, np.nextafter(locs, 1.0), [1.0]]))  # (and one step above: both directions of the error)
            c_on = _t(c, dev)
            exp = expected_slots(c, locs, True)
            host = ops.resample_search(c_on, M, _lib.RESAMPLE_SYSTEMATIC, u32=r)
            got = ops.resample_search(c_on, M, _lib.RESAMPLE_SYSTEMATIC, u=_row(1, r, dev), u32=_lib.U32_FROM_U)
            assert torch.equal(got, host) and np.array_equal(got.cpu().numpy(), exp), f"k_search locations on the table M={M} u32={r}"
            if M >= 255 and M & (M - 1) and r == PLAIN:  # (a power of two divides exactly in both formats)
                loc64 = np.fmod(np.arange(M, dtype=np.float64) / float(M) + np.float64(np.float32(r)) / float(M), 1.0)
                assert not np.array_equal(expected_slots(c, loc64, True), exp), "the case does not tell a float64 quotient from the float32 one"
    with pytest.raises(_lib.MidasError):
        ops.resample_search(c_dev, N, _lib.RESAMPLE_SYSTEMATIC, u32=_lib.U32_FROM_U)  # the sentinel without the memory it names


# ---- the loop engines: k_loop_resample -------------------------------------------------------------------------------------------
def _loop_frames(N):
    pin = _pin()
    out = [pin.tie_frame(N, "all", 1)]
    if N >= 4:
        out += [pin.tie_frame(N, "half", 1), pin.tie_frame(N, "first", -1)]
    if N >= 257:
        out.append(pin.real_frame(N))
    return out


@pytest.mark.parametrize("N", SIZES)
def test_loop_engines(dev, N):
    """LoopEngine (cluster=False: the frame is front + resample) with the offset in `u[0]` against the host `u32`; then a
    BatchLoopEngine of B = 3 rows stepped with three offsets at once: every row is the LoopEngine on seed + b with ITS offset."""
    from midastouch_amd import _lib
    from midastouch_amd.batch_loop_engine import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    pin = _pin()
    cb, _ = pin._world()
    B = 3
    for fr in _loop_frames(N):
        kw = dict(fr.kw, resample="low_var", cluster=False, device=dev)
        od, co, start = _t(fr.odom, dev), _t(fr.code, dev), _t(fr.start, dev)
        singles = [LoopEngine(cb.poses, fr.emb, cb.mesh_vertices, N, **dict(kw, seed=fr.kw["seed"] + b)) for b in range(B)]
        batch = BatchLoopEngine(cb.poses, fr.emb, cb.mesh_vertices, B, N, **kw)

        def single(b, **draws):
            e = singles[b]
            e.set_particles(start)
            e.step_count = 0
            e.step(od, co, **draws)
            return e.frame_view()["ridx"].clone()

        host = {(b, r): single(b, u32=r) for b in range(B) for r in OFFSETS}
        for r in OFFSETS:
            got = single(0, u=_row(N, r, dev), u32=_lib.U32_FROM_U)
            assert torch.equal(got, host[0, r]), f"LoopEngine {fr.key} u32={r}"
        if N > 1:  # (the offsets do select different particles: see _rows_case)
            assert not torch.equal(host[0, 0.0], host[0, WRAP if fr.tie else PLAIN]), f"LoopEngine {fr.key}: the offsets select the same particles"
        for rows in ROWS:
            batch.set_particles(torch.stack([start] * B))
            batch.step_count = 0
            batch.step(torch.stack([od] * B), torch.stack([co] * B), u32=_t(np.array(rows, dtype=np.float32), dev))
            for b in range(B):
                assert torch.equal(batch.frame_view(b)["ridx"], host[b, rows[b]]), f"BatchLoopEngine {fr.key} rows={rows}: row {b}"
        # a host list, and the refusals
        batch.set_particles(torch.stack([start] * B))
        batch.step_count = 0
        batch.step(torch.stack([od] * B), torch.stack([co] * B), u32=list(ROWS[0]))
        assert torch.equal(batch.frame_view(2)["ridx"], host[2, ROWS[0][2]])
        with pytest.raises(_lib.MidasError):
            batch.step(torch.stack([od] * B), torch.stack([co] * B), u32=[0.1, 0.2])


# ---- the eager tails: k_tail_b2 (deferred scores) and k_tail_b (D = 96: no fused front) ---------------------------------------------
def _fixed_frames(N, d):
    pin = _pin()
    out = [pin.tie_frame(N, "all", 1, d)]
    if N >= 4:
        out += [pin.tie_frame(N, "half", 1, d), pin.tie_frame(N, "second", -1, d)]
    if N >= 257:
        out.append(pin.real_frame(N, d=d))
    return out


def _rows_case(dev, single_cls, batch_cls, fr, d, what, folded=(False,)):
    """One frame through a single engine (host offset, then the offset in u[0]) and through its batch engine with B = 3 offsets at
    once: row b against the same batch stepped with the host offset rows[b] (any frame), and against the single engine on a frame
    without motion noise (where a row's draws do not depend on its place in the batch)."""
    from midastouch_amd import _lib
    pin = _pin()
    cb, _ = pin._world(d)
    N, B = fr.N, 3
    kw = dict(fr.kw, resample="low_var", device=dev)
    od, co, start = _t(fr.odom, dev), _t(fr.code, dev), _t(fr.start, dev)
    one = single_cls(cb.poses, fr.emb, cb.mesh_vertices, N, **kw)
    many = batch_cls(cb.poses, fr.emb, cb.mesh_vertices, B, N, **kw) if batch_cls is not None else None
    odB, coB, startB = torch.stack([od] * B), torch.stack([co] * B), torch.stack([start] * B)

    def run(e, fold, o, c, s, **draws):
        e.set_particles(s)
        e.step_count = 0
        e.step(o, c, **draws)
        if fold:
            e.step(o, c)       # the next frame's front resolves the pending resample
            return e._ridx.clone()
        return e.ridx.clone()  # (a pipelined engine: flush())

    for fold in folded:
        tag = f"{what} {'front' if fold else 'tail'} {fr.key}"
        host = {r: run(one, fold, od, co, start, u32=r) for r in OFFSETS}
        for r in OFFSETS:
            got = run(one, fold, od, co, start, u=_row(N, r, dev), u32=_lib.U32_FROM_U)
            assert torch.equal(got, host[r]), f"{tag} u32={r}"
        # the offsets do select different particles (or the rows below would show nothing): on equal weights every offset in [0, 1)
        # selects slot i for location i and only the wrapping one another slot, on real scores an ordinary one differs from 0 already
        if N > 1:
            assert not torch.equal(host[0.0], host[WRAP if fr.tie else PLAIN]), f"{tag}: the offsets select the same particles"
        if many is None:
            continue
        hostB = {r: run(many, fold, odB, coB, startB, u32=r) for r in OFFSETS}
        for rows in ROWS:
            got = run(many, fold, odB, coB, startB, u32=_t(np.array(rows, dtype=np.float32), dev))
            for b in range(B):
                assert torch.equal(got[b], hostB[rows[b]][b]), f"{tag} rows={rows}: row {b} is not the batch's row under its own offset"
                if fr.tie:
                    assert torch.equal(got[b], host[rows[b]]), f"{tag} rows={rows}: row {b} is not its single run"
        got = run(many, fold, odB, coB, startB, u32=list(ROWS[1]))  # (a host list)
        assert torch.equal(got[1], hostB[ROWS[1][1]][1])
        with pytest.raises(_lib.MidasError):
            many.step(odB, coB, u32=[0.5, 0.25])


@pytest.mark.parametrize("N", SIZES)
def test_eager_tails(dev, N):
    from midastouch_amd.engine import BatchFilterEngine, FilterEngine
    for fr in _fixed_frames(N, 128):
        _rows_case(dev, FilterEngine, BatchFilterEngine, fr, 128, "k_tail_b2")


@pytest.mark.parametrize("N", (255, 4097))
def test_legacy_tail(dev, N):
    """D = 96 has no fused front and no sparse scoring: separate scoring and particle-update launches, then k_tail_a + k_tail_b."""
    from midastouch_amd.engine import BatchFilterEngine, FilterEngine
    for fr in _fixed_frames(N, 96):
        _rows_case(dev, FilterEngine, BatchFilterEngine, fr, 96, "k_tail_b")


# ---- the pipelined fronts: the folded resample ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (255, 256, 257, 4095, 4096, 4097, 10241))
def test_pipelined_fronts(dev, N):
    """PipelinedFilterEngine: N <= 512 is the two-kernel front (k_frame_front_a), beyond it k_frame_front with per-wave tables;
    PipelinedBatchFilterEngine: the presort in front of the batch front - k_presort_fused up to 10 240 slots, k_presort_search beyond.
    Folded into the next frame's front, and by flush() (k_tail_b2 on the pipelined tables)."""
    from midastouch_amd.engine import PipelinedBatchFilterEngine, PipelinedFilterEngine
    for fr in _fixed_frames(N, 128):
        _rows_case(dev, PipelinedFilterEngine, PipelinedBatchFilterEngine, fr, 128, "pipelined", folded=(True, False))


def test_pipelined_front_workgroup_tables(dev):
    """More than 64 summation blocks: the front with workgroup-level resample tables (single trajectory only)."""
    from midastouch_amd.engine import PipelinedFilterEngine
    pin = _pin()
    N = 262_144 + 4096 + 1
    _rows_case(dev, PipelinedFilterEngine, None, pin.tie_frame(N, "half", 1), 128, "pipelined 266241", folded=(True, False))
