"""The resample search pinned at every site: which particle a draw selects is decided by seven hand-written searches (k_search,
k_tail_b / k_tail_b2, search_in_block_t of the pipelined front and of the shard route, k_presort_search, the loop engines' draw
search) that all claim one rule - the lower bound over cdf_i = (BP_b + lp_i) / total for multinomial draws (torch.multinomial),
the upper bound for the systematic sampler (the reference's `sampleLocs[c] < weightsSum[i]` loop).  All but the first probe without
a division and repair the result on the quotients; a random draw never lands where probe and quotient could disagree, so every
case here takes its draws FROM the frame's own CDF (tests/_recipes.py crafted_draws: on the entries, one step below and above
them, the ends of the range) or makes the systematic locations land on it (the tie frames: raw weights of exactly +-1.0 * mask,
u32 = 0, so that loc_i = i / N is an entry whenever the valid count divides N).

Every case builds its expectation alike: the frame on the CPU oracle, cdf = oracle.cdf of the masked weights the device builds
its tables from (e * mask, which is +-1.0 * mask on a tie frame), the draws crafted from it and handed to the engine as host draws,
`ridx` against numpy's searchsorted exactly, and against the oracle's search, which keeps the two references tied
(tests/test_resample_reference.py holds them together on the CPU).  The engines' weights are compared with the oracle's first, bit
for bit, so that a differing index is the search's.  On a frame with pruned particles: a draw below or above an entry never
selects a weightless slot, a draw ON an entry selects one exactly where the lower bound names one (the first slot of a flat run
at the start of the table: ATen does the same).  Needs an MI355X."""
import copy
import functools
import types

import numpy as np
import pytest

from _recipes import RS_KINDS, RS_SIZES, crafted_draws, expected_slots, recipe_weights, systematic_locs, tie_share, tie_weights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K, D, SEED = 800, 128, 4600
U32_PLAIN = 0.37
PRUNED = ("all", "half", "second", "first", "last")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


# ---- frames -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _world(d=D):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook("004_sugar_box", K=K, D=d, seed=1005)
    return cb, make_trajectory(cb, T=8, seed=2005)


@functools.lru_cache(maxsize=None)
def tie_frame(N, pruned="all", sign=1, d=D):
    """One-hot codebook rows and a one-hot code: every particle scores exactly +-1.0, the isclose guard skips the softmax
    (particle_filter.py:459-468) and the raw weights are +-1.0 * mask; the pruned particles stand 5 m off the surface
    (pen_max = 0.5), no motion noise, identity odometry."""
    cb, _ = _world(d)
    emb = np.zeros((K, d), dtype=np.float32)
    emb[:, 0] = 1.0
    code = np.zeros(d)
    code[0] = float(sign)
    mask = tie_weights(N, pruned)
    start = cb.poses[np.random.default_rng([N, 1]).integers(0, K, N)].copy()
    start[~mask, :3, 3] += 5.0
    return types.SimpleNamespace(key=("tie", N, pruned, sign, d), N=N, emb=emb, code=code, odom=np.eye(4, dtype=np.float32), start=start,
                                 kw=dict(sig_t=0.0, sig_r=0.0, pen_max=0.5, seed=SEED), tie=True, mask=mask, sign=sign)


@functools.lru_cache(maxsize=None)
def real_frame(N, sig_t=2e-4, d=D):
    """Softmax weights of a cloud on the codebook's poses one odometry step on, the default prune: about nine particles in ten
    are lost and the CDF has long flat runs."""
    cb, traj = _world(d)
    start = cb.poses[np.random.default_rng([N, 2]).integers(0, K, N)].copy()
    return types.SimpleNamespace(key=("real", N, sig_t, d), N=N, emb=cb.embeddings, code=traj.codes[1], odom=traj.odoms[1], start=start,
                                 kw=dict(sig_t=sig_t, sig_r=0.5, pen_max=0.002, seed=SEED), tie=False, mask=None, sign=1)


_REF = {}


def reference(oracle, fr, rows=1, row=0, d=D):
    """The oracle's frame (computed once per process, shared, never written to): the masked weights `em` the CDF is built from
    (e * mask - the normalisation cancels in prefix / total, oracle.OracleFilter.step), their CDF, the weights the engine reports.
    rows / row: the frame as trajectory `row` of a batch of `rows` (the device's motion noise is keyed by b * N + n)."""
    key = (fr.key, rows, row)
    if key not in _REF:
        cb, _ = _world(d)
        N = fr.N
        tn, rot = oracle.philox_noise(rows * N, SEED, 0, np.float32(fr.kw["sig_t"]), np.float32(fr.kw["sig_r"]))
        sl = slice(row * N, (row + 1) * N)
        ofl = oracle.OracleFilter(cb.poses, fr.emb, cb.mesh_vertices, pen_max=fr.kw["pen_max"])
        ref = ofl.step(fr.start, fr.odom, fr.code, tn[sl], rot[sl], u=np.zeros(N))
        e, applied = oracle.softmax_numerators(ref["scores"][ref["nn_idx"]], True, shift=1.0)
        em = e * ref["mask"]
        c, status = oracle.cdf(em)
        assert status == 0 and ref["status"] == 0
        if fr.tie:
            assert np.array_equal(ref["mask"], fr.mask) and np.array_equal(em, fr.sign * fr.mask.astype(np.float64))
        else:
            assert 0 < ref["mask"].sum() < N  # flat runs
        _REF[key] = dict(em=em, cdf=c, weights=ref["weights"], V=int(ref["mask"].sum()), N=N, e=e, applied=applied)
    return _REF[key]


def _draws(R, kind, salt=0, M=None):
    return crafted_draws(R["cdf"], kind, np.random.default_rng([R["N"], RS_KINDS.index(kind), salt]), M=M)


SEEN = {}


def _check(oracle, R, got, what, u=None, u32=None, kind=None, site=None):
    """`got` against numpy's bound and the oracle's search; the weightless-slot property; -> the number of draws ON an entry."""
    c, em = R["cdf"], R["em"]
    got = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got).reshape(-1)
    if u is not None:
        x = np.asarray(u, dtype=np.float64).reshape(-1)
        exp, orc = expected_slots(c, x, False), oracle.search_lower(c, x)
    else:
        x = systematic_locs(got.shape[0], u32)
        exp, orc = expected_slots(c, x, True), oracle.search_systematic(c, got.shape[0], u32)
    assert np.array_equal(orc, exp), f"{what}: the oracle's search and numpy's bound differ"
    ties = np.isin(x, c)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (f"{what}: {bad.size} of {exp.shape[0]} slots differ ({int(ties[bad].sum())} of them on draws that equal an entry); "
                           f"first: draw {bad[0]} = {x[bad[0]]!r} -> slot {got[bad[0]]}, want {exp[bad[0]]}")
    if (em == 0).any():
        if u is None or kind in ("below", "above"):
            assert (em[got] != 0).all(), f"{what}: a weightless slot was selected"
        else:
            assert np.array_equal(em[got] == 0, em[exp] == 0), what
    if site is not None:
        s = SEEN.setdefault(site, dict(draws=0, ties=0, cases=0))
        s["draws"] += x.shape[0]
        s["ties"] += int(ties.sum())
        s["cases"] += 1
    return int(ties.sum())


def _report(site):
    s = SEEN.get(site)
    if s:
        print(f"resample pin [{site}]: {s['cases']} index sets, {s['draws']} draws, {s['ties']} on a CDF entry")


def _assert_inputs(R, kind, u, what):
    if kind == "on" and (R["cdf"] < 1.0).any():   # (one particle, or one with weight: no entry below 1, and 1 is drawn as 1 - 2^-53)
        assert tie_share(R["cdf"], u) >= 0.5, f"{what}: the crafted draws miss the CDF"


def _t(a, dev, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).to(dev)


# ---- ops.resample_search -------------------------------------------------------------------------------------------------------
def _hand_weights(N):
    rng = np.random.default_rng([N, 3])
    sets = {"random": rng.random(N), "equal": np.full(N, 0.37), "negative": -rng.random(N)}
    if N >= 4:
        w = rng.random(N)
        w[: max(N // 5, 1)] = 0.0
        w[N // 2: N // 2 + max(N // 7, 1)] = 0.0
        w[N - max(N // 9, 1):] = 0.0
        sets["zero runs"] = w
        sets["masked recipe"] = recipe_weights(N, "masked", 5)
    for pruned in PRUNED:
        m = tie_weights(N, pruned)
        if m.any():
            sets[f"tie {pruned}"] = m.astype(np.float64)
            sets[f"tie {pruned} negated"] = -m.astype(np.float64)
    return sets


@pytest.mark.parametrize("N", RS_SIZES)
def test_ops_resample_search(dev, oracle, N):
    """k_search on ops.cdf of hand-made weights: every recipe kind with M = N, 1 and 2 N draws, the systematic locations at u32 = 0
    (ties on the +-1.0 * mask sets) and at an ordinary u32 with M = N, 1 and 2 N."""
    from midastouch_amd import _lib, ops
    for name, w in _hand_weights(N).items():
        c_dev, status = ops.cdf(_t(w, dev))
        c, st = oracle.cdf(w)
        assert st == 0 and int(status.item()) == 0 and np.array_equal(c_dev.cpu().numpy(), c), (name, N)
        R = dict(cdf=c, em=w, N=N)
        for M in (N, 1, 2 * N):
            for kind in RS_KINDS:
                u = _draws(R, kind, M, M=M)
                if M == N:   # (a single draw, M = 1, may be 1 - 2^-53 alone)
                    _assert_inputs(R, kind, u, f"k_search {name} N={N}")
                got = ops.resample_search(c_dev, M, _lib.RESAMPLE_MULTINOMIAL, u=_t(u, dev))
                _check(oracle, R, got, f"k_search {name} N={N} M={M} {kind}", u=u, kind=kind, site="ops.resample_search")
            for u32 in (0.0, U32_PLAIN):
                got = ops.resample_search(c_dev, M, _lib.RESAMPLE_SYSTEMATIC, u32=u32)
                n = _check(oracle, R, got, f"k_search {name} N={N} M={M} u32={u32}", u32=u32, site="ops.resample_search systematic")
                if name.startswith("tie") and u32 == 0.0 and M == N and N % max(int((w != 0).sum()), 1) == 0:
                    assert n >= int((w != 0).sum()) - 1
    _report("ops.resample_search")
    _report("ops.resample_search systematic")


# ---- FilterEngine ---------------------------------------------------------------------------------------------------------------
def _frames_for(N, d=D):
    """The frames of a fixed-N site: the real scores and the tie frames, +1.0 and negated (sets too small to halve: `all` only)."""
    out = [real_frame(N, d=d)] if N >= 257 else []
    for pruned in (PRUNED if N >= 4 else ("all",)):
        for sign in (1, -1):
            out.append(tie_frame(N, pruned, sign, d))
    out += [tie_frame(N, f"lead{k}", 1, d) for k, _ in BLOCK_END_OVERSHOOT.get(N, ())]
    return out


# Tie frames whose first k particles are pruned, chosen so that the division-free probe errs AT A BLOCK'S LAST SLOT: the entry
# there is x = fl(p / V) with p = slot + 1 - k and V = N - k, and fl(x V) > p - the probe calls the slot "left" of a draw that
# equals its entry, every slot of the block's last chunk is then left, and the fix-up starts beyond the block (`l2 >= b_hi`,
# `pos >= U`).  (With nobody pruned p is a power of two there, and fl(fl(p / V) V) never exceeds a power of two.)
BLOCK_END_OVERSHOOT = {9000: ((10, 4095), (4, 8191)), 10241: ((12, 4095),)}


def _assert_block_end_overshoot(R, fr):
    for k, slot in BLOCK_END_OVERSHOOT.get(fr.N, ()):
        if fr.key[2] == f"lead{k}":
            x, p, V = R["cdf"][slot], float(slot + 1 - k), float(fr.N - k)
            assert x == p / V and x * V > p, (fr.key, slot)


def _eager_case(dev, oracle, cls, fr, site, d=D):
    """One frame through an eager engine, every draw set: the four kinds, u32 = 0 (ties on a tie frame), an ordinary u32."""
    cb, _ = _world(d)
    R = reference(oracle, fr, d=d)
    _assert_block_end_overshoot(R, fr)
    N = fr.N
    engs = {mode: cls(cb.poses, fr.emb, cb.mesh_vertices, N, resample=mode, device=dev, **fr.kw) for mode in ("weighted_random", "low_var")}
    od, co, start = _t(fr.odom, dev), _t(fr.code, dev), _t(fr.start, dev)

    def run(mode, **draws):
        e = engs[mode]
        e.set_particles(start)
        e.step_count = 0
        e.step(od, co, **draws)
        assert np.array_equal(e.weights.cpu().numpy(), R["weights"]), f"{site} {fr.key}: weights"
        assert e.status.cpu().numpy().tolist() == [0, R["V"]]
        return e.ridx

    for kind in RS_KINDS:
        u = _draws(R, kind)
        _assert_inputs(R, kind, u, f"{site} {fr.key}")
        _check(oracle, R, run("weighted_random", u=_t(u, dev)), f"{site} {fr.key} {kind}", u=u, kind=kind, site=site)
    for u32 in (0.0, U32_PLAIN):
        n = _check(oracle, R, run("low_var", u32=u32), f"{site} {fr.key} u32={u32}", u32=u32, site=site + " systematic")
        if fr.tie and u32 == 0.0 and N % R["V"] == 0:
            assert n >= R["V"] - 1, f"{site} {fr.key}: {n} systematic ties"


@pytest.mark.parametrize("N", [1, 2, 17, 257, 4095, 4096, 4097, 8193, 9000])
def test_filter_engine(dev, oracle, N):
    """The eager step's tail at D = 128: the deferred branch of launch_step_tail, k_tail_b2 - the kernel flush() runs for the
    pipelined engines (k_tail_b, the legacy tail, is test_filter_engine_unfused_tail's)."""
    from midastouch_amd.engine import FilterEngine
    for fr in _frames_for(N):
        _eager_case(dev, oracle, FilterEngine, fr, "FilterEngine")
    _report("FilterEngine")
    _report("FilterEngine systematic")


def test_filter_engine_coarse_chunk_table(dev, oracle):
    """N = 140 003: more than 8192 chunks - the coarse chunk-end table plus probes of the global one (cshift > 0), ragged last block."""
    from midastouch_amd.engine import FilterEngine
    for fr in (real_frame(140_003), tie_frame(140_003, "all", -1), tie_frame(140_003, "half", 1), tie_frame(140_003, "first", 1)):
        _eager_case(dev, oracle, FilterEngine, fr, "FilterEngine 140003")
    _report("FilterEngine 140003")
    _report("FilterEngine 140003 systematic")


def test_filter_engine_unfused_tail(dev, oracle):
    """D = 96 has no fused front: separate scoring and particle-update launches and the legacy tail."""
    from midastouch_amd.engine import FilterEngine
    for fr in (real_frame(5000, d=96), tie_frame(5000, "all", 1, 96), tie_frame(5000, "half", -1, 96), tie_frame(5000, "first", 1, 96)):
        _eager_case(dev, oracle, FilterEngine, fr, "FilterEngine D=96", d=96)
    _report("FilterEngine D=96")
    _report("FilterEngine D=96 systematic")


# ---- PipelinedFilterEngine ------------------------------------------------------------------------------------------------------
def _pipelined_case(dev, oracle, fr, site, kinds=RS_KINDS):
    """The draws given with frame t are searched by the front of frame t + 1 (search_in_block_t; `_ridx`) or by flush()
    (k_tail_b2): both, from the same start."""
    from midastouch_amd.engine import PipelinedFilterEngine
    cb, _ = _world()
    R = reference(oracle, fr)
    _assert_block_end_overshoot(R, fr)
    N = fr.N
    engs = {mode: PipelinedFilterEngine(cb.poses, fr.emb, cb.mesh_vertices, N, resample=mode, device=dev, **fr.kw)
            for mode in ("weighted_random", "low_var")}
    od, co, start = _t(fr.odom, dev), _t(fr.code, dev), _t(fr.start, dev)

    def run(mode, folded, **draws):
        e = engs[mode]
        e.set_particles(start)
        e.step_count = 0
        e.step(od, co, **draws)
        if folded:
            e.step(od, co)                     # the next frame's front resolves the pending resample
            return e._ridx
        assert np.array_equal(e.weights.cpu().numpy(), R["weights"]), f"{site} {fr.key}: weights"   # (flushes)
        assert e.status.cpu().numpy().tolist() == [0, R["V"]]
        return e.ridx

    for folded in (True, False):
        s = f"{site} {'front' if folded else 'flush'}"
        for kind in kinds:
            u = _draws(R, kind)
            _assert_inputs(R, kind, u, f"{s} {fr.key}")
            _check(oracle, R, run("weighted_random", folded, u=_t(u, dev)), f"{s} {fr.key} {kind}", u=u, kind=kind, site=s)
        for u32 in (0.0, U32_PLAIN):
            n = _check(oracle, R, run("low_var", folded, u32=u32), f"{s} {fr.key} u32={u32}", u32=u32, site=s + " systematic")
            if fr.tie and u32 == 0.0 and N % R["V"] == 0:
                assert n >= R["V"] - 1, f"{s} {fr.key}: {n} systematic ties"


@pytest.mark.parametrize("guide", ["1", "0"])
@pytest.mark.parametrize("N", [257, 4097, 9000, 10240, 10241])
def test_pipelined_engine(dev, oracle, monkeypatch, N, guide):
    """10 240 / 10 241: the last set of the one-kernel front (tables in LDS) and the first of the two-kernel form; with and without
    the guide tables."""
    monkeypatch.setenv("MIDAS_GUIDE", guide)
    site = f"PipelinedFilterEngine guide={guide}"
    for fr in _frames_for(N):
        _pipelined_case(dev, oracle, fr, site)
    for s in ("front", "flush"):
        _report(f"{site} {s}")
        _report(f"{site} {s} systematic")


@pytest.mark.parametrize("guide", ["1", "0"])
def test_pipelined_engine_wide_noise(dev, oracle, monkeypatch, guide):
    """sig_t = 3e-3 loses all but a few particles in a hundred: guide bins that span many units fall back to the table lines."""
    monkeypatch.setenv("MIDAS_GUIDE", guide)
    fr = real_frame(9000, sig_t=3e-3)
    assert reference(oracle, fr)["V"] < 9000 // 10
    _pipelined_case(dev, oracle, fr, f"PipelinedFilterEngine sig_t=3e-3 guide={guide}")
    for s in ("front", "flush"):
        _report(f"PipelinedFilterEngine sig_t=3e-3 guide={guide} {s}")


def test_pipelined_engine_workgroup_tables(dev, oracle):
    """More than 64 blocks (262 144 slots): the fronts with workgroup-level resample tables; ragged last block."""
    N = 262_144 + 4096 + 1
    for fr in (real_frame(N), tie_frame(N, "all", -1), tie_frame(N, "half", 1)):
        _pipelined_case(dev, oracle, fr, "PipelinedFilterEngine 266241")
    for s in ("front", "flush"):
        _report(f"PipelinedFilterEngine 266241 {s}")
        _report(f"PipelinedFilterEngine 266241 {s} systematic")


# ---- batch engines --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["BatchFilterEngine", "PipelinedBatchFilterEngine"])
@pytest.mark.parametrize("N", [4097, 40_000])
def test_batch_engines(dev, oracle, engine, N):
    """B = 3, a different recipe kind per row (k_presort_search and the batch tail / flush); 40 000 particles: more chunk ends than
    the search kernel stages in LDS (PS_GEND_MAX).  The pipelined engine: folded into the next frame's front, and by flush()."""
    from midastouch_amd import engine as E
    cb, _ = _world()
    B = 3
    frames = [tie_frame(N, "half", 1), tie_frame(N, "second", -1), tie_frame(N, "all", 1), tie_frame(N, "first", 1)]
    if N == 4097:
        frames.insert(0, real_frame(N))
    pipelined = engine.startswith("Pipelined")
    for fr in frames:
        # one start for the three rows; on the real-score frame the rows differ by their motion noise (keyed b * N + n)
        Rs = [reference(oracle, fr, B, b) for b in range(B)] if not fr.tie else [reference(oracle, fr)] * B
        engs = {mode: getattr(E, engine)(cb.poses, fr.emb, cb.mesh_vertices, B, N, resample=mode, device=dev, **fr.kw)
                for mode in ("weighted_random", "low_var")}
        assert all(e.sparse_scores for e in engs.values())  # the float64 scores of the single-trajectory step
        od, co = _t(np.stack([fr.odom] * B), dev), _t(np.stack([fr.code] * B), dev)
        start = _t(np.stack([fr.start] * B), dev)

        def run(mode, folded, **draws):
            e = engs[mode]
            e.set_particles(start)
            e.step_count = 0
            e.step(od, co, **draws)
            if folded:
                e.step(od, co)
                return e._ridx
            w = e.weights.cpu().numpy()
            for b in range(B):
                assert np.array_equal(w[b], Rs[b]["weights"]), f"{engine} {fr.key} row {b}: weights"
            return e.ridx

        for folded in ((True, False) if pipelined else (False,)):
            site = engine + ((" front" if folded else " flush") if pipelined else "")
            for rot in range(2):
                kinds = [RS_KINDS[(b + 2 * rot) % 4] for b in range(B)]   # on, below, above / above, ends, on
                us = [_draws(Rs[b], kinds[b], b) for b in range(B)]
                ridx = run("weighted_random", folded, u=_t(np.stack(us), dev))
                for b in range(B):
                    _assert_inputs(Rs[b], kinds[b], us[b], f"{site} {fr.key} row {b}")
                    _check(oracle, Rs[b], ridx[b], f"{site} {fr.key} row {b} {kinds[b]}", u=us[b], kind=kinds[b], site=site)
            for u32 in (0.0, U32_PLAIN):
                ridx = run("low_var", folded, u32=u32)
                for b in range(B):
                    n = _check(oracle, Rs[b], ridx[b], f"{site} {fr.key} row {b} u32={u32}", u32=u32, site=site + " systematic")
                    if fr.tie and u32 == 0.0 and N % Rs[b]["V"] == 0:
                        assert n >= Rs[b]["V"] - 1
    for s in list(SEEN):
        if s.startswith(engine):
            _report(s)


# ---- ShardedFilterEngine --------------------------------------------------------------------------------------------------------
class FakeComm:
    def __init__(self, r, w):
        self.rank, self.world = r, w

    def all_gather(self, t):
        raise AssertionError("lock-step test never calls the communicator")

    all_to_all = all_gather


def _sharded_reference(oracle, R, shards, n_loc):
    """The frame's CDF and weights as `shards` ranks of n_loc particles sum them: every rank's slots form summation blocks of
    their own (a rank's first slot starts a block; include/midas_hip.h: equal to the one-process frame only where n_loc is a multiple
    of 4096), the blocks are added in rank order.  By the oracle: every rank's values padded with +0.0 to whole blocks - a missing
    trailing element counts as +0.0 in the summation spec - and the padding taken out again."""
    pad = (-n_loc) % 4096
    padded = lambda a: np.concatenate([np.concatenate([a[r * n_loc:(r + 1) * n_loc], np.zeros(pad)]) for r in range(shards)])  # noqa: E731
    keep = np.concatenate([np.arange(n_loc) + r * (n_loc + pad) for r in range(shards)])
    c, status = oracle.cdf(padded(R["em"]))
    assert status == 0
    S = oracle.blocked_scan(padded(R["e"]))[1] if R["applied"] else 1.0
    out = dict(R, cdf=c[keep], weights=R["e"] / S * (R["em"] != 0))
    assert out["cdf"][-1] == 1.0 and np.abs(out["cdf"] - R["cdf"]).max() < 1e-13
    return out


@pytest.mark.parametrize("exchange", ["allgather", "a2a_fixed", "peer_c"])
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_engine(dev, oracle, shards, exchange):
    """Shards of 4096 + 2 slots (a block and a ragged chunk; the sharded step takes an even count per rank, and ranks that are no
    whole blocks sum in their own block order: _sharded_reference) stepped in lock-step (tests/test_gpu_dist.py), the uniforms of
    ALL slots given to every shard: the all_gather form's own search and search_in_block_t in shard_route.hip (the owner-side
    forms)."""
    from midastouch_amd.dist import HipShardBackend, ShardedFilterEngine, connect_local_peers, run_lockstep
    cb, _ = _world()
    n_loc = 4098
    N = shards * n_loc
    site = f"ShardedFilterEngine {exchange}"
    for fr in (real_frame(N), tie_frame(N, "all", 1), tie_frame(N, "half", 1), tie_frame(N, "half", -1), tie_frame(N, "last", 1)):
        R = _sharded_reference(oracle, reference(oracle, fr), shards, n_loc)
        be = HipShardBackend(cb.poses, fr.emb, cb.mesh_vertices, dev)
        groups = {}
        for mode in ("weighted_random", "low_var"):
            engs = [ShardedFilterEngine(num_particles=n_loc, backend=be, comm=FakeComm(r, shards), resample=mode, exchange=exchange, **fr.kw)
                    for r in range(shards)]
            if exchange == "peer_c":
                connect_local_peers(engs, exchange)
            for e in engs:
                e.seg_cap = -(-n_loc // 8) * 8   # a crafted draw set may send a rank every row it holds to one destination
            groups[mode] = engs
        od, co = _t(fr.odom, dev), _t(fr.code, dev)

        def run(mode, **draws):
            engs = groups[mode]
            for r, e in enumerate(engs):
                e.set_particles(_t(fr.start[r * n_loc:(r + 1) * n_loc], dev))
                e.step_count = 0
            run_lockstep(engs, [((od, co), dict(draws)) for _ in engs])
            assert np.array_equal(torch.cat([e.weights for e in engs]).cpu().numpy(), R["weights"]), f"{site} {fr.key}: weights"
            if exchange == "allgather":  # (the form that materialises the quotients)
                assert np.array_equal(torch.cat([e.st.cdf for e in engs]).cpu().numpy(), R["cdf"]), f"{site} {fr.key}: CDF"
            return torch.cat([e.ridx for e in engs])

        for kind in RS_KINDS:
            u = _draws(R, kind)
            _assert_inputs(R, kind, u, f"{site} {fr.key}")
            _check(oracle, R, run("weighted_random", u=_t(u, dev)), f"{site} x{shards} {fr.key} {kind}", u=u, kind=kind, site=site)
        for u32 in (0.0, U32_PLAIN):
            n = _check(oracle, R, run("low_var", u32=u32), f"{site} x{shards} {fr.key} u32={u32}", u32=u32, site=site + " systematic")
            if fr.tie and u32 == 0.0 and N % R["V"] == 0:
                assert n >= R["V"] - 1
    _report(site)
    _report(site + " systematic")


# ---- loop engines ---------------------------------------------------------------------------------------------------------------
def _loop_em(oracle, emb, code, ref):
    """The masked weights of the annealed set the loop's resampler searches: (e * mask)[keep] (oracle.OracleLoop.step)."""
    e = oracle.softmax_numerators(oracle.score_codebook(emb, code)[ref["nn_idx"]], True, shift=1.0)[0]
    return (e * ref["mask"])[ref["keep"]]


@pytest.mark.parametrize("N0", [300, 5000])
def test_loop_engine_annealed_set(dev, oracle, N0):
    """Host draws `u` on frames whose annealing changed the set size (the table of the frame's N particles, draws over the annealed
    N'): the frame is split in front of RESAMPLE, the draws are crafted from the oracle loop's annealed weights, one kind a frame."""
    from midastouch_amd import _lib
    from midastouch_amd.loop_engine import LoopEngine
    from midastouch_amd.synthetic import mesh_scale
    cb, traj = _world()
    floor = N0 // 3
    g = torch.Generator().manual_seed(11)
    sc = mesh_scale(cb.extents)
    tn0 = torch.normal(0.0, sc / 3.0 * 0.15, size=(N0, 3), generator=g).numpy()
    rot0 = torch.normal(0.0, 60.0 * 0.15, size=(N0, 3), generator=g).numpy()
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, floor=floor, cluster_every=3)
    poses = cb.poses[loop.f.SE3_NN_idx(oracle.init_filter_compose(traj.gt_poses[0], tn0, rot0))]
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0, seed=SEED, floor=floor, cluster_every=3, device=dev)
    eng.set_particles(_t(poses, dev))
    labels = np.zeros(N0, dtype=np.int64)
    kinds, changed = list(RS_KINDS), 0
    for t in range(7):
        n = poses.shape[0]
        tn, rot = oracle.philox_noise(n, SEED, t, np.float32(2e-4), np.float32(0.5))
        probe = copy.deepcopy(loop).step(poses, labels, traj.odoms[t + 1], traj.codes[t + 1], tn, rot, u=np.zeros(2 * N0))
        od, co = _t(traj.odoms[t + 1], dev), _t(traj.codes[t + 1], dev)
        if probe["status"] != 0 or not kinds or (probe["N"] == n and not changed):
            # an ordinary frame on the device's own draws, until annealing moves
            ref = loop.step(poses, labels, traj.odoms[t + 1], traj.codes[t + 1], tn, rot, draws=lambda n2: oracle.philox_uniform64(n2, SEED, t))
            eng.step(od, co)
        else:
            kind = kinds.pop(0)
            changed += int(probe["N"] != n)
            em = _loop_em(oracle, cb.embeddings, traj.codes[t + 1], probe)
            R = dict(em=em, cdf=oracle.cdf(em)[0], N=em.shape[0])
            u = _draws(R, kind, t)
            _assert_inputs(R, kind, u, f"LoopEngine frame {t}")
            eng.step(od, co, phases=_lib.LOOP_FRONT | _lib.LOOP_DBSCAN | _lib.LOOP_ANNEAL)
            assert int(eng.ctl_i[_lib.LOOP_I_NSET].item()) == probe["N"] == u.shape[0]
            eng.step(None, None, u=_t(u, dev), phases=_lib.LOOP_RESAMPLE)
            ref = loop.step(poses, labels, traj.odoms[t + 1], traj.codes[t + 1], tn, rot, u=u)
            fv = eng.frame_view()
            assert np.array_equal(fv["weights"].cpu().numpy(), ref["weights"]) and np.array_equal(fv["src"].cpu().numpy(), ref["keep"])
            _check(oracle, R, fv["ridx"], f"LoopEngine N0={N0} frame {t} (n {n} -> {probe['N']}) {kind}", u=u, kind=kind, site="LoopEngine")
            assert np.array_equal(fv["ridx"].cpu().numpy(), ref["ridx"])
        poses, labels = ref["poses"], ref["labels"]
    assert changed >= 1 and "on" not in kinds, (changed, kinds)
    _report("LoopEngine")


_LOOP_REF = {}


def _loop_tie_reference(oracle, fr):
    """The oracle loop's first frame on a tie frame (once per process): annealing takes its first variance and keeps every
    particle, the resampler searches the CDF of (e * mask)[keep] = +-1.0 * mask."""
    if fr.key not in _LOOP_REF:
        cb, _ = _world()
        loop = oracle.OracleLoop(cb.poses, fr.emb, cb.mesh_vertices, pen_max=fr.kw["pen_max"], floor=fr.N // 3)
        z = np.zeros((fr.N, 3), dtype=np.float32)
        ref = loop.step(fr.start, np.zeros(fr.N, dtype=np.int64), fr.odom, fr.code, z, z, mode="low_var", u32=0.0)
        em = _loop_em(oracle, fr.emb, fr.code, ref)
        assert ref["N"] == fr.N and np.array_equal(ref["keep"], np.arange(fr.N)) and np.array_equal(em, fr.sign * fr.mask.astype(np.float64))
        _LOOP_REF[fr.key] = dict(em=em, cdf=oracle.cdf(em)[0], N=fr.N, weights=ref["weights"], V=int(fr.mask.sum()))
    return _LOOP_REF[fr.key]


@pytest.mark.parametrize("N0", [300, 5000])
def test_loop_engine_tie_frames(dev, oracle, N0):
    """The loop's draw search on the tie frames: host draws of every kind, u32 = 0 and an ordinary u32."""
    from midastouch_amd.loop_engine import LoopEngine
    cb, _ = _world()
    for fr in (tie_frame(N0, "all", 1), tie_frame(N0, "half", 1), tie_frame(N0, "second", -1), tie_frame(N0, "first", 1), tie_frame(N0, "last", 1)):
        od, co = _t(fr.odom, dev), _t(fr.code, dev)
        R = _loop_tie_reference(oracle, fr)

        def run(mode, **draws):
            eng = LoopEngine(cb.poses, fr.emb, cb.mesh_vertices, N0, floor=N0 // 3, resample=mode, device=dev, **fr.kw)
            eng.set_particles(_t(fr.start, dev))
            eng.step(od, co, **draws)
            fv = eng.frame_view()
            assert fv["n_after"] == N0 and np.array_equal(fv["weights"].cpu().numpy(), R["weights"]), f"LoopEngine {fr.key}: weights"
            return fv["ridx"]

        for kind in RS_KINDS:
            u = _draws(R, kind)
            _assert_inputs(R, kind, u, f"LoopEngine {fr.key}")
            _check(oracle, R, run("weighted_random", u=_t(u, dev)), f"LoopEngine {fr.key} {kind}", u=u, kind=kind, site="LoopEngine tie frames")
        for u32 in (0.0, U32_PLAIN):
            n = _check(oracle, R, run("low_var", u32=u32), f"LoopEngine {fr.key} u32={u32}", u32=u32, site="LoopEngine tie frames systematic")
            if u32 == 0.0 and N0 % R["V"] == 0:
                assert n >= R["V"] - 1
    _report("LoopEngine tie frames")
    _report("LoopEngine tie frames systematic")


@pytest.mark.parametrize("N0", [300, 5000])
def test_batch_loop_engine_tie_frames(dev, oracle, N0):
    """BatchLoopEngine takes u32 alone: the systematic tie frames, B = 2, a different mask per row."""
    from midastouch_amd import BatchLoopEngine
    cb, _ = _world()
    for pair in ((("all", 1), ("half", 1)), (("second", -1), ("first", 1)), (("half", -1), ("last", 1))):
        frs = [tie_frame(N0, p, s) for p, s in pair]
        for u32 in (0.0, U32_PLAIN):
            # (rows of one batch share the codebook: the negated code gives the negated frame)
            eng = BatchLoopEngine(cb.poses, frs[0].emb, cb.mesh_vertices, 2, N0, floor=N0 // 3, resample="low_var", device=dev, **frs[0].kw)
            eng.set_particles([_t(f.start, dev) for f in frs])
            eng.step(_t(np.stack([f.odom for f in frs]), dev), _t(np.stack([f.code for f in frs]), dev), u32=u32)
            for b, fr in enumerate(frs):
                R = _loop_tie_reference(oracle, fr)
                fv = eng.frame_view(b)
                assert fv["n_after"] == N0 and np.array_equal(fv["weights"].cpu().numpy(), R["weights"])
                n = _check(oracle, R, fv["ridx"], f"BatchLoopEngine {fr.key} u32={u32}", u32=u32, site="BatchLoopEngine systematic")
                if u32 == 0.0 and N0 % R["V"] == 0:
                    assert n >= R["V"] - 1
    _report("BatchLoopEngine systematic")
