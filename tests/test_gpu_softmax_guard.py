"""The softmax guard pinned at every site.  get_similarity (modules/particle_filter.py:449-469) skips the softmax when
isclose(max(x) - min(x), 0) holds over ALL particles of the frame - |max - min| <= 1e-8 in float64, NaN never close, pruned
particles included (the prune comes after: filter/filter.py:168-176) - and every place that turns scores into weights decides
that again behind a hand-written extrema reduction.  A frame of widely spread scores applies the softmax whichever values a
reduction drops, a frame of identical scores has nothing to drop: only a cloud collapsed onto one score with ONE dissenting
particle sees a slot, a lane, a wave, a group, a block or a shard that a reduction misses - the weights then come out as the raw
scores instead of a distribution (or the reverse).  Every frame here is of that kind (tests/_recipes.py recipe_guard_scores,
guard_frame): the base score +0.0, the dissenter wide (+-1 / sqrt 5: the max and the min reduction), at the 1e-8 edge (the float32
rows either side of it: below32 raw, above32 applied; direct scores: exactly 1e-8 and the float64 neighbours, -0.0) or NaN, at the
first and last slot of every lane / wave / group / block boundary of N = 12 345 = 3 * 4096 + 57, at every slot of N = 1, 2, 15,
16, 17, beyond 64 blocks (266 297) and beyond 256 blocks (1 052 729), with nobody pruned, half of the others pruned, or the
dissenter itself pruned (its score still counts).

The sites, and what reaches them (routes read from launch_tail_a2 / launch_shard_tail_a / launch_step_tail, tail.hip; filter_step_impl,
lazy_step_impl and lazy_flush_impl, api_step.hip; the front's launcher, front.hip):

  #  site                               reached through                                          shown by
  1  k_extrema + k_exp_partial          ops.softmax_weights, direct scores, every kind           weights vs the oracle bit for bit, vs torch
  2  k_tail_a2 (N < 16), k_tail_a2d     midas_shard_tail_a, direct scores (N >= 16: the grouped  bmax / bmin records, which blocks wrote the raw
     (MIDAS_TAIL_GROUPED=0), k_tail_a3  form by default, read per launch)                        tables, every table against the oracle
  3  k_tail_b2                          FilterEngine D = 128; PipelinedFilterEngine.flush()      weights, status, ridx
  4  k_tail_a + k_tail_b                FilterEngine D = 96 (no fused front: the legacy tail)    weights, status, ridx
  5  lazy_tables_wave                   PipelinedFilterEngine, 513 <= N <= 262 144 (the single   the next frame's _ridx under u_i = (i + 0.5) / N
                                        kernel with per-wave tables): 513, 10 240, 10 241, 12 345 against the oracle's search on the oracle's CDF
  6  lazy_tables                        PipelinedFilterEngine N <= 512 (the two-kernel form,     the same
                                        k_frame_front_a: 1 .. 17 and 512) and N = 266 297 (the
                                        single kernel with workgroup tables)
  7  batch fronts and tails             BatchFilterEngine, PipelinedBatchFilterEngine, B = 3:    per-row weights, ridx (a guard shared by the rows
                                        row 0 flat (every score 1.0), rows 1, 2 dissenters.      turns the flat row into a softmax)
                                        The pipelined batch front is presorted and the presort
                                        decides the guard (lazy_tables_wave in front_batch.hip):
                                        k_presort_fused up to 10 240 particles, k_presort_search
                                        beyond - 16, 17, 10 240, 10 241, 12 345; the tails
                                        k_tail_a2 / k_tail_a2d with grid.y = 3 and k_tail_b2
  8  k_estimate_moments                 the pipelined engines' estimate=True (from the tables;   the centre against cluster_reference of the
                                        the eager engines' estimate reads the weights)           oracle's weights
  9  launch_tail_fin, k_shard_route     ShardedFilterEngine in lock-step, 2 and 3 shards,        concatenated weights / ridx / CDF against the
                                        allgather, a2a_fixed, peer_c; also > 256 blocks in all   oracle; against FilterEngine at shards of 4096
  10 loop_weights_head                  LoopEngine (with and without clustering), BatchLoopEngine ctl_i[LOOP_I_RAW], LOOP_D_XMAX / XMIN, weights, ridx
                                        plain and wide, live count below the capacity

Expectations come from the frame's construction and the oracle's arithmetic (guard_expected: e = exp_spec(x - 1) or x, S the
blocked sum over all particles, w = e / S * mask, the blocked CDF of e * mask), the same at every size; the device's nn_idx is read
back and must equal the construction.  Weights, indices and status match bit for bit.  Site 8: only the wide kinds - raw weights would
put the whole weight on the dissenter, which stands at least 1 cm from the cloud's mean; at the edge kinds the centre's own float32
flatten rule (abs(float32(max - min)) <= 1e-8) makes both variants uniform and the two cannot be told apart there.  NaN at the engine
sites is a NaN in the dissenting codebook row (no constructor rejects it); on a NaN frame the folded resample's indices are not
compared (the frame is not resampled).  Needs an MI355X."""
import numpy as np
import pytest

from _recipes import (GUARD_EDGE_SLOTS, GUARD_KINDS, GUARD_N, GUARD_N66, GUARD_N258, GUARD_ROWS, GUARD_SLOTS, GUARD_SLOTS66, GUARD_SLOTS258,
                      GUARD_SMALL, GUARD_WIDE_KINDS, assert_cluster, cluster_reference, guard_cases, guard_expected, guard_frame,
                      guard_rule_torch, guard_world, recipe_guard_scores)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROW_KINDS = tuple(GUARD_ROWS)
SEEN = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _t(a, dev, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).to(dev)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _count(site, n=1):
    SEEN[site] = SEEN.get(site, 0) + n


def _report(*sites):
    for s in sites or sorted(SEEN):
        if s in SEEN:
            print(f"softmax guard [{s}]: {SEEN[s]} frames")


def _draws(N):
    return (np.arange(N, dtype=np.float64) + 0.5) / N


def _slots(N):
    if N == GUARD_N:
        return GUARD_SLOTS
    return {GUARD_N66: GUARD_SLOTS66, GUARD_N258: GUARD_SLOTS258}.get(N, tuple(range(N)))


def _frames(N, kind, slots=None, pruned=("none", "half", "dissenter"), d=128):
    """The frames of one size and kind: the wide kinds at every slot of the size's list, the others at GUARD_EDGE_SLOTS of 12 345
    (every slot of the other sizes); the dissenter itself pruned only where the softmax applies and somebody else is left."""
    if slots is None:
        slots = _slots(N)
        if N == GUARD_N and kind not in GUARD_WIDE_KINDS:
            slots = GUARD_EDGE_SLOTS
    out = []
    for slot in slots:
        for p in pruned:
            if p == "dissenter" and (N == 1 or kind == "nan" or not GUARD_KINDS[kind][1]):
                continue
            out.append(guard_frame(N, kind, slot, p, d))
    return out


def _check_frame(oracle, fr, E, what, weights, status, nn_idx=None, ridx=None, u=None):
    """Weights bit for bit, status, the nearest entries of the construction; the indices where the frame is resampled."""
    if nn_idx is not None:
        assert np.array_equal(_np(nn_idx), fr.nn), f"{what}: nn_idx is not the construction's"
    w = _np(weights)
    bad = np.flatnonzero(~((w == E["weights"]) | (np.isnan(w) & np.isnan(E["weights"]))))
    if bad.size:
        raw = np.array_equal(w, fr.x * fr.mask, equal_nan=True)
        raise AssertionError(f"{what}: {bad.size} of {fr.N} weights differ (expected {'softmax' if E['applied'] else 'raw'}; the device's "
                             f"{'are the raw scores' if raw else 'are neither'}); first: slot {bad[0]}: {w[bad[0]]!r}, want {E['weights'][bad[0]]!r}")
    assert _np(status).reshape(-1).tolist() == [E["status"], E["V"]], f"{what}: status {_np(status)}, want {[E['status'], E['V']]}"
    if fr.pruned == "dissenter":
        assert E["applied"] and E["status"] == 0 and w[fr.slot] == 0.0
    if ridx is not None and E["status"] == 0:
        exp = oracle.search_lower(E["cdf"], u)
        got = _np(ridx).reshape(-1)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{what}: {bad.size} of {fr.N} resample indices differ; first: draw {bad[0]} -> {got[bad[0]]}, want {exp[bad[0]]}"


# ---- 1: ops.softmax_weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", list(GUARD_SMALL) + [GUARD_N, GUARD_N66, GUARD_N258])
def test_ops_softmax_weights(dev, oracle, N):
    """k_extrema + k_exp_partial on direct scores: every kind (the exact float64 edge included), every slot of the size."""
    from midastouch_amd import ops
    worst = 0.0
    for _, kind, slot in (c for c in guard_cases(big=(GUARD_N66, GUARD_N258)) if c[0] == N):
        x = recipe_guard_scores(N, kind, slot)
        w = ops.softmax_weights(_t(x, dev)).cpu().numpy()
        ref, applied = oracle.softmax_weights(x)
        what = f"ops.softmax_weights N={N} {kind} slot {slot}"
        assert np.array_equal(w, ref, equal_nan=True), f"{what}: differs from the oracle (expected {'softmax' if applied else 'raw'})"
        tw, tap = guard_rule_torch(x)
        if N == 1 and kind == "nan":
            assert np.isnan(w).all()
        elif np.isnan(tw).any():
            assert tap and np.isnan(tw).all() and np.isnan(w).all(), what
        elif not tap:
            assert np.array_equal(w.view(np.uint64), tw.view(np.uint64)), what
        else:
            rel = float(np.max(np.abs(w - tw) / tw))
            worst = max(worst, rel)
            assert rel <= N * 2.0 ** -52, f"{what}: {rel:.3g} from the torch restatement"
        _count(f"ops.softmax_weights N={N}")
    print(f"largest relative difference from torch where applied: {worst:.3g} (bound {N * 2.0 ** -52:.3g})")
    _report(f"ops.softmax_weights N={N}")


# ---- 2: the tail's first kernel, direct scores ------------------------------------------------------------------------------
SENTINEL = -123.0
_TAIL_REF = {}


def _tail_a_run(dev, N, scores, nn, valid):
    """midas_shard_tail_a as tests/test_gpu_tail_group.py calls it, the tables filled with a sentinel first."""
    from midastouch_amd import _lib
    from test_gpu_tail_group import _tables_len
    ctx = _lib.context(dev)
    nb = -(-N // 4096)
    tables = torch.full((_tables_len(N),), SENTINEL, dtype=torch.float64, device=dev)
    r1 = torch.zeros(5 * nb + 4, dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ctx.call("midas_shard_tail_a", N, _lib._ptr(scores), _lib._ptr(nn), _lib._ptr(valid), 1, _lib._ptr(tables), _lib._ptr(r1), _lib._ptr(status))
    torch.cuda.synchronize()
    return tables.cpu().numpy(), r1.cpu().numpy(), status.cpu().numpy()


def _tail_a_reference(oracle, N, x, valid, key):
    """Per 4096-slot block by the oracle (tests/_oracle_shard_backend.py tail_a): e, the block-local prefix sums of e * valid and of
    x * valid and their totals, the block sum of e, numpy's max / min of the block's scores (NaN for a block with a NaN)."""
    if key in _TAIL_REF:
        return _TAIL_REF[key]
    nb = -(-N // 4096)
    e = oracle.exp_spec(x, 1.0)
    em, xm = e * valid, x * valid
    R = dict(e=e, lp=np.empty(N), lpr=np.empty(N), bsum=np.empty(nb), btot=np.empty(nb), btotr=np.empty(nb), bmax=np.empty(nb), bmin=np.empty(nb))
    for b in range(nb):
        sl = slice(b * 4096, min((b + 1) * 4096, N))
        R["bsum"][b] = oracle.blocked_scan(e[sl])[1]
        R["lp"][sl], R["btot"][b] = oracle.blocked_scan(em[sl])
        R["lpr"][sl], R["btotr"][b] = oracle.blocked_scan(xm[sl])
        R["bmax"][b], R["bmin"][b] = np.max(x[sl]), np.min(x[sl])
    R["close"] = np.abs(R["bmax"] - R["bmin"]) <= 1e-8
    _TAIL_REF.clear()   # (one case at a time: a million-slot reference is 40 MB)
    _TAIL_REF[key] = R
    return R


def _tail_a_cases(N):
    return [c for c in guard_cases(big=(GUARD_N66, GUARD_N258)) if c[0] == N]


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "block"])
@pytest.mark.parametrize("N", list(GUARD_SMALL) + [GUARD_N, GUARD_N66, GUARD_N258])
def test_tail_a_block_rule(dev, oracle, monkeypatch, N, grouped):
    """k_tail_a2 (N < 16), k_tail_a2d (MIDAS_TAIL_GROUPED=0) and k_tail_a3: the per-block extrema records and the block-local rule -
    a block writes the raw-variant tables exactly when ITS OWN spread is within 1e-8 (every block but the dissenter's; the
    dissenter's too at the raw kinds; never a block with a NaN)."""
    monkeypatch.setenv("MIDAS_TAIL_GROUPED", "1" if grouped else "0")
    nb, Np = -(-N // 4096), -(-N // 16) * 16
    site = f"tail_a {'grouped' if grouped else 'block'} N={N}"
    for _, kind, slot in _tail_a_cases(N):
        for pruned in ("none", "half"):
            x = recipe_guard_scores(N, kind, slot)
            valid = np.ones(N, np.uint8)
            if pruned == "half":
                valid[np.random.default_rng([N, slot, 7]).random(N) < 0.5] = 0
                valid[slot] = 1
            # the scores as a two-row "codebook": row 0 the base, row 1 the dissenter's
            sc = np.array([0.0, GUARD_KINDS[kind][0]])
            nn = np.zeros(N, np.int32)
            nn[slot] = 1
            t, r1, status = _tail_a_run(dev, N, _t(sc, dev), _t(nn, dev), _t(valid, dev))
            R = _tail_a_reference(oracle, N, x, valid, (N, kind, slot, pruned))
            what = f"{site} {kind} slot {slot} pruned {pruned}"
            rec = {k: r1[i * nb:(i + 1) * nb] for i, k in enumerate(("bsum", "btot", "btotr", "bmax", "bmin"))}
            assert np.array_equal(rec["bmax"], R["bmax"], equal_nan=True), f"{what}: bmax {rec['bmax']} vs {R['bmax']}"
            assert np.array_equal(rec["bmin"], R["bmin"], equal_nan=True), f"{what}: bmin {rec['bmin']} vs {R['bmin']}"
            assert np.array_equal(np.signbit(rec["bmin"]), np.signbit(R["bmin"])) or kind == "signed_zero", what
            e, xr, lp, lpr = (t[i * Np:i * Np + N] for i in range(4))
            assert np.array_equal(e, R["e"], equal_nan=True), f"{what}: e"
            assert np.array_equal(lp, R["lp"], equal_nan=True), f"{what}: the softmax variant's prefix sums"
            assert np.array_equal(rec["bsum"], R["bsum"], equal_nan=True) and np.array_equal(rec["btot"], R["btot"], equal_nan=True), what
            close = np.repeat(R["close"], 4096)[:N]
            wrote = xr != SENTINEL
            assert np.array_equal(wrote, close), (f"{what}: raw tables written by blocks {np.unique(np.flatnonzero(wrote) // 4096).tolist()}, "
                                                  f"close are {np.flatnonzero(R['close']).tolist()}")
            assert np.array_equal(xr[close], x[close]) and np.array_equal(lpr[close], R["lpr"][close]), f"{what}: the raw tables"
            assert (lpr[~close] == SENTINEL).all(), f"{what}: raw prefix sums written by a block that is not close"
            assert np.array_equal(rec["btotr"][R["close"]], R["btotr"][R["close"]]), f"{what}: the raw totals"
            assert int(status[1]) == int(valid.sum()) and (int(status[0]) & 2 != 0) == (kind == "nan"), f"{what}: status {status}"
            assert (r1[5 * nb] != 0) == (kind == "nan") and r1[5 * nb + 1] == valid.sum(), what
            _count(site)
    _report(site)


# ---- 3, 4: the eager engine -------------------------------------------------------------------------------------------------------
def _eager_frames(dev, oracle, cls, frames, site, **extra):
    cb, _ = guard_world(frames[0].d)
    engs = {}
    for fr in frames:
        E = guard_expected(fr)
        key = (fr.N, fr.kind, fr.kstar)
        if key not in engs:
            engs[key] = cls(cb.poses, fr.emb, cb.mesh_vertices, fr.N, resample="weighted_random", device=dev, **fr.kw, **extra)
        e = engs[key]
        u = _draws(fr.N)
        e.set_particles(_t(fr.start, dev))
        e.step_count = 0
        e.step(_t(fr.odom, dev), _t(fr.code, dev), u=_t(u, dev))
        _check_frame(oracle, fr, E, f"{site} {fr.key[1:5]}", e.weights, e.status, e.nn_idx, e.ridx, u)
        if E["status"] != 0:   # the resampler returns its input (particle_filter.py:237-241)
            assert np.array_equal(_np(e.ridx), np.arange(fr.N)), f"{site} {fr.key[1:5]}: ridx of a frame that is not resampled"
        _count(site)


def _small_frames(kind, d=128):
    return [fr for N in GUARD_SMALL for fr in _frames(N, kind, d=d)]


@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("N", ["small", GUARD_N, GUARD_N66, GUARD_N258])
def test_filter_engine(dev, oracle, N, kind):
    """The eager step at D = 128: k_tail_a3 / k_tail_a2 and k_tail_b2, whose BPT rounds over the block records start their second
    round at 1 052 729."""
    from midastouch_amd.engine import FilterEngine
    site = f"FilterEngine N={N}"
    _eager_frames(dev, oracle, FilterEngine, _small_frames(kind) if N == "small" else _frames(N, kind), site)
    _report(site)


@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("N", ["small", GUARD_N, GUARD_N66])
def test_filter_engine_unfused_tail(dev, oracle, N, kind):
    """D = 96 has no fused front: k_tail_a's extrema from the particle update's partials and k_tail_b."""
    from midastouch_amd.engine import FilterEngine
    site = f"FilterEngine D=96 N={N}"
    _eager_frames(dev, oracle, FilterEngine, _small_frames(kind, 96) if N == "small" else _frames(N, kind, d=96), site)
    _report(site)


# ---- 3, 5, 6: the pipelined engine ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("N", ["small", 512, 513, 10_240, 10_241, GUARD_N, GUARD_N66])
def test_pipelined_engine(dev, oracle, N, kind):
    """The draws given with frame t are searched by the front of frame t + 1 from tables it rebuilds behind its own guard: `_ridx`.
    launch_frame_front (front.hip, `split_front`): a pipelined set of at most 512 particles takes the two-kernel form, whose
    k_frame_front_a calls lazy_tables (the small sets and 512); from 513 up to 64 blocks (262 144) the single kernel with per-wave
    tables, lazy_tables_wave (513, 10 240, 10 241, 12 345 - one form: this engine changes nothing at 10 240); beyond, the single kernel
    with workgroup tables, lazy_tables again (266 297).  And by flush() (k_tail_b2): weights, status, ridx."""
    from midastouch_amd.engine import PipelinedFilterEngine
    cb, _ = guard_world()
    if N == "small":
        frames = _small_frames(kind)
    elif N in (512, 513):
        frames = _frames(N, kind, slots=(0, 63, 64, 255, 256, N - 1))
    elif N in (10_240, 10_241):
        frames = _frames(N, kind, slots=(0, 4095, 4096, 8191, N - 1))
    else:
        frames = _frames(N, kind)
    site = f"PipelinedFilterEngine N={N}"
    engs = {}
    for fr in frames:
        E = guard_expected(fr)
        key = (fr.N, fr.kind, fr.kstar)
        if key not in engs:
            engs[key] = PipelinedFilterEngine(cb.poses, fr.emb, cb.mesh_vertices, fr.N, resample="weighted_random", device=dev, **fr.kw)
        e = engs[key]
        u = _draws(fr.N)
        od, co = _t(fr.odom, dev), _t(fr.code, dev)
        what = f"{site} {fr.key[1:5]}"
        for folded in (True, False):
            e.set_particles(_t(fr.start, dev))
            e.step_count = 0
            e.step(od, co, u=_t(u, dev))
            if folded:
                if E["status"] == 0:
                    e.step(od, co)   # the next frame's front resolves the pending resample
                    got, exp = _np(e._ridx), oracle.search_lower(E["cdf"], u)
                    bad = np.flatnonzero(got != exp)
                    assert bad.size == 0, (f"{what} front: {bad.size} of {fr.N} indices differ (expected {'softmax' if E['applied'] else 'raw'} "
                                           f"tables); first: draw {bad[0]} -> {got[bad[0]]}, want {exp[bad[0]]}")
                    _count(site + " front")
            else:
                _check_frame(oracle, fr, E, what + " flush", e.weights, e.status, e.nn_idx, e.ridx, u)
                _count(site + " flush")
    _report(site + " front", site + " flush")


# ---- 7: the batch engines --------------------------------------------------------------------------------------------------------
BATCH_SIZES = list(GUARD_SMALL) + [10_240, 10_241, GUARD_N]
# (PipelinedBatchFilterEngine takes 16 <= N <= 262 144: its constructor says so)
BATCH_CASES = ([("BatchFilterEngine", n) for n in BATCH_SIZES + [GUARD_N66]] + [("PipelinedBatchFilterEngine", n) for n in BATCH_SIZES if n >= 16])


@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("engine,N", BATCH_CASES)
def test_batch_engines(dev, oracle, N, engine, kind):
    """B = 3 on one codebook: row 0 flat (the code e_1, nobody on the dissenting row: every score exactly 1.0, raw), rows 1 and 2
    with dissenters at different slots - extrema or a decision shared by the rows give row 0 a softmax.  The tails with
    grid.y = 3 (launch_tail_a2): k_tail_a2 for the eager batch at every size (no table strides), k_tail_a2d for the pipelined batch,
    then k_tail_b2.
    The pipelined batch front is presorted (launch_presort, front_batch.hip) and the presort decides the guard, by lazy_tables_wave,
    before it stages `apply ? lp : lp_raw`: k_presort_fused up to PS_LP_MAX = 10 240 particles (one workgroup holds the
    trajectory's whole prefix table), k_presort_search + k_presort_group beyond - 10 240 and 10 241 are the last and the first set
    of the two, with dissenters in block 0, block 1, block 2 and at the last slot.  1, 2, 15 and 266 297 run on the eager batch alone:
    the pipelined batch engine takes 16 .. 262 144 particles (at most 64 blocks; no k_tail_a2 in it, then)."""
    from midastouch_amd import engine as Eng
    cb, _ = guard_world()
    B = 3
    if N == GUARD_N:
        slots = GUARD_SLOTS if kind in GUARD_WIDE_KINDS else GUARD_EDGE_SLOTS
    elif N in (10_240, 10_241):
        slots = (0, 4095, 4096, 8191, 8192, N - 1)
    else:
        slots = _slots(N)
    pairs = [(slots[i], slots[-1 - i]) for i in range((len(slots) + 1) // 2)] + [(slots[-1], slots[0])]
    if N == GUARD_N and kind not in GUARD_WIDE_KINDS:
        pairs = [(0, 12344), (10114, 0), (12344, 10114)]
    pipelined = engine.startswith("Pipelined")
    eng = None
    for pruned in ("none", "half"):
        for s1, s2 in pairs:
            frs = [guard_frame(N, kind, None, pruned), guard_frame(N, kind, s1, pruned), guard_frame(N, kind, s2, pruned)]
            assert len({f.kstar for f in frs}) == 1 and all(np.array_equal(f.emb, frs[0].emb, equal_nan=True) for f in frs)
            Es = [guard_expected(f) for f in frs]
            assert not Es[0]["applied"] and np.array_equal(Es[0]["weights"], frs[0].mask.astype(np.float64))
            if eng is None:
                eng = getattr(Eng, engine)(cb.poses, frs[0].emb, cb.mesh_vertices, B, N, resample="weighted_random", device=dev, **frs[0].kw)
                assert eng.sparse_scores   # the float64 scores of the single-trajectory step
            u = _draws(N)
            od, co = _t(np.stack([f.odom for f in frs]), dev), _t(np.stack([f.code for f in frs]), dev)
            for folded in ((True, False) if pipelined else (False,)):
                eng.set_particles(_t(np.stack([f.start for f in frs]), dev))
                eng.step_count = 0
                eng.step(od, co, u=_t(np.stack([u] * B), dev))
                site = engine + ((" front" if folded else " flush") if pipelined else "")
                if folded:
                    if all(E["status"] == 0 for E in Es):
                        eng.step(od, co)
                        got = _np(eng._ridx)
                        for b in range(B):
                            assert np.array_equal(got[b], oracle.search_lower(Es[b]["cdf"], u)), f"{site} N={N} {kind} slots {s1}, {s2} pruned {pruned} row {b}"
                        _count(site)
                    continue
                w, st, nn, ridx = _np(eng.weights), _np(eng.status), _np(eng.nn_idx), _np(eng.ridx)
                for b in range(B):
                    _check_frame(oracle, frs[b], Es[b], f"{site} N={N} {kind} slots {s1}, {s2} pruned {pruned} row {b}", w[b], st[b], nn[b], ridx[b], u)
                _count(site)
    _report(*[s for s in SEEN if s.startswith(engine)])


# ---- 8: the estimate from the tables --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GUARD_WIDE_KINDS)
@pytest.mark.parametrize("engine", ["FilterEngine", "PipelinedFilterEngine", "BatchFilterEngine", "PipelinedBatchFilterEngine"])
def test_estimate(dev, oracle, engine, kind):
    """estimate=True: the pipelined engines' centre comes from the tail's tables behind k_estimate_moments' own guard (the eager
    engines' from the weights: beside them for the same expectation).  Under the softmax the weights are all but uniform; raw, the
    whole weight sits on the dissenter, at least 1 cm from the cloud's mean."""
    from midastouch_amd import engine as Eng
    cb, _ = guard_world()
    N = GUARD_N
    batch = "Batch" in engine
    eng = None
    for slot in (0, 63, 4096, 10114, 12344):
        for pruned in ("none", "half"):
            fr = guard_frame(N, kind, slot, pruned)
            E = guard_expected(fr)
            t = fr.start[:, :3, 3].astype(np.float64)
            mean = t[fr.mask].mean(axis=0)
            if np.linalg.norm(t[slot] - mean) < 0.01:
                continue
            if eng is None:
                args = (cb.poses, fr.emb, cb.mesh_vertices) + ((2, N) if batch else (N,))
                eng = getattr(Eng, engine)(*args, resample="weighted_random", device=dev, estimate=True, **fr.kw)
            rows = lambda a: np.stack([a, a]) if batch else a   # noqa: E731
            eng.set_particles(_t(rows(fr.start), dev))
            eng.step_count = 0
            eng.step(_t(rows(fr.odom), dev), _t(rows(fr.code), dev), u=_t(rows(_draws(N)), dev))
            c, s = (_np(a) for a in eng.estimate)
            ref = cluster_reference(fr.start, E["weights"], np.zeros(N, dtype=np.int64))   # (identity odometry, no noise: poses_prop = start)
            for b in range(2 if batch else 1):
                cb_, sb = (c[b], s[b]) if batch else (c, s)
                assert np.linalg.norm(cb_[:3, 3] - t[slot]) > 5e-3, f"{engine} {kind} slot {slot} pruned {pruned}: the centre sits on the dissenter (raw weights)"
                assert_cluster(cb_[None], sb[None], ref, -(-N // 256), f"{engine} {kind} slot {slot} pruned {pruned} row {b}")
            _count(f"estimate {engine}")
    assert SEEN.get(f"estimate {engine}", 0) >= 4
    _report(f"estimate {engine}")


# ---- 9: the sharded engine ---------------------------------------------------------------------------------------------------------
class FakeComm:
    def __init__(self, r, w):
        self.rank, self.world = r, w

    def all_gather(self, t):
        raise AssertionError("lock-step test never calls the communicator")

    all_to_all = all_gather


def _sharded_frames(dev, oracle, frames, shards, n_loc, exchange, site):
    from midastouch_amd.dist import HipShardBackend, ShardedFilterEngine, connect_local_peers, run_lockstep
    cb, _ = guard_world()
    groups, out = {}, []
    for fr in frames:
        E = guard_expected(fr, shard=(shards, n_loc))
        key = (fr.kind, fr.kstar)
        if key not in groups:
            be = HipShardBackend(cb.poses, fr.emb, cb.mesh_vertices, dev)
            engs = [ShardedFilterEngine(num_particles=n_loc, backend=be, comm=FakeComm(r, shards), resample="weighted_random", exchange=exchange, **fr.kw)
                    for r in range(shards)]
            if exchange == "peer_c":
                connect_local_peers(engs, exchange)
            for e in engs:
                e.seg_cap = -(-n_loc // 8) * 8
            groups[key] = engs
        engs = groups[key]
        u = _draws(fr.N)
        for r, e in enumerate(engs):
            e.set_particles(_t(fr.start[r * n_loc:(r + 1) * n_loc], dev))
            e.step_count = 0
        od, co = _t(fr.odom, dev), _t(fr.code, dev)
        run_lockstep(engs, [((od, co), dict(u=_t(u, dev))) for _ in engs])
        what = f"{site} x{shards} {fr.key[1:5]}"
        status = _np(engs[0].status)
        for e in engs[1:]:
            assert np.array_equal(_np(e.status), status), f"{what}: the ranks disagree on the status"
        _check_frame(oracle, fr, E, what, torch.cat([e.weights for e in engs]), status, torch.cat([e.st.nn_idx for e in engs]),
                     torch.cat([e.ridx for e in engs]), u)
        if exchange == "allgather" and E["status"] == 0:
            assert np.array_equal(_np(torch.cat([e.st.cdf for e in engs])), E["cdf"]), f"{what}: CDF"
        out.append((_np(torch.cat([e.weights for e in engs])), _np(torch.cat([e.ridx for e in engs])), status))
        _count(site)
    return out


@pytest.mark.parametrize("exchange", ["allgather", "a2a_fixed", "peer_c"])
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_engine(dev, oracle, shards, exchange):
    """Shards of 4096 + 2 slots in lock-step on one GPU: the dissenter at the first shard's first and last slot, the next shard's
    first, a middle shard's last and the last shard's last - launch_tail_fin's guard over the gathered records and k_shard_route's."""
    n_loc = 4098
    N = shards * n_loc
    slots = sorted({0, 4095, n_loc - 1, n_loc, (shards - 1) * n_loc - 1, N - 1})
    site = f"ShardedFilterEngine {exchange}"
    for kind in ROW_KINDS:
        _sharded_frames(dev, oracle, _frames(N, kind, slots=slots), shards, n_loc, exchange, site)
    _report(site)


@pytest.mark.parametrize("exchange", ["allgather", "a2a_fixed", "peer_c"])
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_engine_equals_single_engine(dev, oracle, shards, exchange):
    """Shards of exactly 4096 slots: every rank is one whole summation block, the ranks' blocks are the one-process frame's blocks
    and the concatenated weights and indices equal FilterEngine's on the whole set bit for bit (and the oracle's).  With any other
    shard size a rank's slots form blocks of their own (include/midas_hip.h), the sums are added in another order and only the
    oracle with the same padding (guard_expected's `shard`) is a bitwise yardstick: test_sharded_engine, 4098 slots a shard."""
    from midastouch_amd.engine import FilterEngine
    cb, _ = guard_world()
    n_loc = 4096
    N = shards * n_loc
    site = f"ShardedFilterEngine {exchange} = FilterEngine"
    for kind in ROW_KINDS:
        frames = _frames(N, kind, slots=(0, n_loc - 1, n_loc, N - 1))
        got = _sharded_frames(dev, oracle, frames, shards, n_loc, exchange, site)
        single = {}
        for fr, (w, ridx, status) in zip(frames, got):
            key = (fr.kind, fr.kstar)
            if key not in single:
                single[key] = FilterEngine(cb.poses, fr.emb, cb.mesh_vertices, N, resample="weighted_random", device=dev, **fr.kw)
            e = single[key]
            e.set_particles(_t(fr.start, dev))
            e.step_count = 0
            e.step(_t(fr.odom, dev), _t(fr.code, dev), u=_t(_draws(N), dev))
            what = f"{site} x{shards} {fr.key[1:5]}"
            assert np.array_equal(w, _np(e.weights), equal_nan=True), f"{what}: weights"
            assert np.array_equal(status, _np(e.status)), f"{what}: status {status} vs {_np(e.status)}"
            assert np.array_equal(ridx, _np(e.ridx)), f"{what}: ridx"
    _report(site)


@pytest.mark.parametrize("exchange", ["allgather", "a2a_fixed", "peer_c"])
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_engine_second_round(dev, oracle, shards, exchange):
    """More than 256 blocks in all (2 x 130, 3 x 87): the second round of the strided loops over the gathered block records."""
    n_loc = {2: 129, 3: 86}[shards] * 4096 + 58
    N = shards * n_loc
    assert shards * -(-n_loc // 4096) > 256
    site = f"ShardedFilterEngine {exchange} {N}"
    for kind in ("wide_hi", "wide_lo", "above32_lo", "below32_hi"):
        _sharded_frames(dev, oracle, _frames(N, kind, slots=(n_loc - 1, N - 1), pruned=("half",)), shards, n_loc, exchange, site)
    _report(site)


# ---- 10: the loop engines ------------------------------------------------------------------------------------------------------
def _check_loop(oracle, fr, E, fv, what, u=None, u32=None):
    from midastouch_amd import _lib
    n = fr.N
    assert fv["n"] == n and fv["n_after"] == n, f"{what}: n {fv['n']} -> {fv['n_after']}"
    assert int(fv["ctl_i"][_lib.LOOP_I_RAW]) == int(not E["applied"]), f"{what}: LOOP_I_RAW {fv['ctl_i'][_lib.LOOP_I_RAW]}, applied {E['applied']}"
    xmax, xmin = fv["ctl_d"][_lib.LOOP_D_XMAX], fv["ctl_d"][_lib.LOOP_D_XMIN]
    assert np.array_equal([xmax, xmin], [np.max(fr.x), np.min(fr.x)], equal_nan=True), f"{what}: extrema {xmax!r}, {xmin!r}"
    assert np.array_equal(_np(fv["nn_idx"]), fr.nn), f"{what}: nn_idx"
    w = _np(fv["weights"])
    assert np.array_equal(w, E["weights"], equal_nan=True), f"{what}: weights (expected {'softmax' if E['applied'] else 'raw'})"
    assert int(fv["ctl_i"][_lib.LOOP_I_STATUS]) == E["status"] and int(fv["ctl_i"][_lib.LOOP_I_KEPT]) == E["V"], f"{what}: status"
    if E["status"] == 0:
        exp = oracle.search_lower(E["cdf"], u) if u is not None else oracle.search_systematic(E["cdf"], n, u32)
        assert np.array_equal(_np(fv["ridx"]), exp), f"{what}: ridx"
    assert np.array_equal(_np(fv["src"]), np.arange(n)), what


@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("N,cluster", [("small", False), (GUARD_N, False), (GUARD_N, True), (GUARD_N66, False), (GUARD_N66, True)])
def test_loop_engine(dev, oracle, N, kind, cluster):
    """loop_weights_head at the head of k_loop_weights and of k_loop_weights_moments (clustering on), the live count below the
    capacity: the block records beyond the live blocks hold whatever an earlier frame left.  (DBSCAN's min_samples = N // 5 needs
    more than a handful of particles: the small sets run without clustering.)"""
    from midastouch_amd.loop_engine import LoopEngine
    cb, _ = guard_world()
    frames = _small_frames(kind) if N == "small" else _frames(N, kind)
    site = f"LoopEngine {'cluster' if cluster else 'plain'} N={N}"
    engs = {}
    for fr in frames:
        E = guard_expected(fr)
        key = (fr.N, fr.kind, fr.kstar)
        if key not in engs:
            engs[key] = LoopEngine(cb.poses, fr.emb, cb.mesh_vertices, fr.N + 4096 + 300, floor=max(fr.N // 3, 1), cluster=cluster,
                                   resample="weighted_random", device=dev, **fr.kw)
        e = engs[key]
        u = _draws(fr.N)
        e.set_particles(_t(fr.start, dev))
        e.step(_t(fr.odom, dev), _t(fr.code, dev), u=_t(u, dev))
        _check_loop(oracle, fr, E, e.frame_view(), f"{site} {fr.key[1:5]}", u=u)
        _count(site)
    _report(site)


@pytest.mark.parametrize("wide", [False, True], ids=["plain", "wide"])
@pytest.mark.parametrize("kind", ROW_KINDS)
def test_batch_loop_engine(dev, oracle, kind, wide):
    """B = 3 (row 0 flat, rows 1 and 2 dissenters, the last live slot among them), the live count below the capacity; wide=True
    with a capacity beyond 16 384 runs the wide launches.  BatchLoopEngine takes u32 alone: the systematic sampler."""
    from midastouch_amd import BatchLoopEngine
    cb, _ = guard_world()
    N, B, u32 = GUARD_N, 3, 0.37
    cap = 20_000 if wide else N + 300
    slots = GUARD_SLOTS if kind in GUARD_WIDE_KINDS else GUARD_EDGE_SLOTS
    pairs = [(slots[-1 - i], slots[i]) for i in range(len(slots) // 2)] + [(slots[0], slots[-1])]
    site = f"BatchLoopEngine {'wide' if wide else 'plain'}"
    eng = None
    for cluster in (False, True):
        eng = None
        for pruned in ("none", "half"):
            for s1, s2 in pairs:
                frs = [guard_frame(N, kind, None, pruned), guard_frame(N, kind, s1, pruned), guard_frame(N, kind, s2, pruned)]
                Es = [guard_expected(f) for f in frs]
                if eng is None:
                    eng = BatchLoopEngine(cb.poses, frs[0].emb, cb.mesh_vertices, B, cap, floor=N // 3, cluster=cluster, resample="low_var",
                                          device=dev, wide=wide, **frs[0].kw)
                eng.set_particles([_t(f.start, dev) for f in frs])
                eng.step(_t(np.stack([f.odom for f in frs]), dev), _t(np.stack([f.code for f in frs]), dev), u32=u32)
                for b in range(B):
                    _check_loop(oracle, frs[b], Es[b], eng.frame_view(b), f"{site} cluster={cluster} {kind} slots {s1}, {s2} pruned {pruned} row {b}", u32=u32)
                _count(site)
    _report(site)
