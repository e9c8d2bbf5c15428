"""The resample search's references held to each other on the CPU: the oracle's two searches (oracle/midas_oracle.c
mo_search_lower, mo_search_systematic - what every GPU parity test compares indices with) against numpy's searchsorted on draws
that EQUAL CDF entries (tests/_recipes.py crafted_draws), against the reference's own low-variance loop restated in torch
(modules/particle_filter.py:251-307), and torch.multinomial itself against the lower bound.  A random float64 draw meets an entry
about once in 1e13 tries, so without crafted draws `<` against `<=` is pinned nowhere.  tests/test_gpu_resample_pin.py runs the
same draws through every search on the device."""
import numpy as np
import pytest

from _recipes import (RS_KINDS, RS_SIZES, U_MAX, crafted_draws, expected_slots, recipe_weights, structural_slots, systematic_locs,
                      tie_share, tie_weights)

torch = pytest.importorskip("torch")


def _both(oracle, w, u, u32s=(0.0, 0.37, 1.0 - 2.0 ** -24), M=None):
    """Both oracle searches against numpy on the blocked CDF of w; -> the CDF."""
    c, status = oracle.cdf(w)
    assert status == 0
    N = c.shape[0]
    assert np.array_equal(oracle.search_lower(c, u), expected_slots(c, u, False))
    for u32 in u32s:
        m = N if M is None else M
        assert np.array_equal(oracle.search_systematic(c, m, u32), expected_slots(c, systematic_locs(m, u32), True)), u32
    return c


def _weight_sets(N, rng):
    yield "random", rng.random(N)
    yield "equal", np.full(N, 0.37)
    yield "negative", -rng.random(N)                 # total < 0: p = w / sum(w) >= 0
    if N >= 4:
        w = rng.random(N)
        w[: max(N // 5, 1)] = 0.0                    # runs of zeros at the start, in the middle and at the end
        w[N // 2: N // 2 + max(N // 7, 1)] = 0.0
        w[N - max(N // 9, 1):] = 0.0
        yield "zero runs", w
        yield "masked recipe", recipe_weights(N, "masked", 5)
    for pruned in ("all", "half", "second", "first", "last"):
        m = tie_weights(N, pruned)
        if m.any():
            yield f"tie {pruned}", m.astype(np.float64)
            yield f"tie {pruned} negated", -m.astype(np.float64)


@pytest.mark.parametrize("N", RS_SIZES)
def test_oracle_searches_equal_numpy_on_crafted_draws(oracle, N):
    rng = np.random.default_rng([N, 1])
    for name, w in _weight_sets(N, rng):
        c = oracle.cdf(w)[0]
        for kind in RS_KINDS:
            u = crafted_draws(c, kind, rng)
            _both(oracle, w, u)
            if kind == "on":
                distinct = np.unique(c).shape[0]
                assert tie_share(c, u) >= min(distinct - 1, N) / N - 1e-12, (name, N)   # every entry below 1 is drawn
                # the opposite bound differs on every tie: the draws really tell `<` from `<=`
                ties = np.isin(u, c)
                assert (expected_slots(c, u, True)[ties] != expected_slots(c, u, False)[ties]).all() or N == 1, (name, N)
        for M in (1, 2 * N):
            u = crafted_draws(c, "on", rng, M=M)
            assert u.shape == (M,)
            _both(oracle, w, u, M=M)


def test_recipe_takes_the_structural_entries_first():
    """More distinct entries than draws: the entries at the chunk, group, block and unit ends and around them are all drawn."""
    rng = np.random.default_rng(3)
    N = 9000
    c = np.cumsum(rng.random(N))
    c /= c[-1]
    u = crafted_draws(c, "on", rng, M=N // 2)
    s = structural_slots(c)
    assert {14, 15, 16, 254, 255, 256, 4094, 4095, 4096, 8190, 8191, 8192, 3, 7, N - 2} <= set(s.tolist())
    want = c[s]
    assert np.isin(np.where(want >= 1.0, U_MAX, want), u).all()
    assert tie_share(c, u) >= (N // 2 - 1) / (N // 2)
    flat = np.repeat(np.arange(1, 11) / 10.0, 7)                  # runs of seven equal entries: both ends of each are structural
    s = set(structural_slots(flat).tolist())
    assert {0, 6, 7, 13, 63, 69} <= s


@pytest.mark.parametrize("tag", ["soft4096", "soft1000", "peaky2048", "masked3000", "n1", "n2", "n65"])
def test_oracle_searches_equal_numpy_on_the_goldens(golden, oracle, tag):
    g = golden("g2_resampler")
    w = g[f"{tag}_w"].astype(np.float64)
    rng = np.random.default_rng(7)
    c = _both(oracle, w, g[f"{tag}_weighted_random_u"], u32s=(float(g[f"{tag}_low_var_u"][0]), 0.0))
    for kind in RS_KINDS:
        _both(oracle, w, crafted_draws(c, kind, rng))


def test_tie_constructions_tie(oracle):
    """The systematic tie frames: weights 1.0 * mask, u32 = 0 - loc_i = i / N equals a CDF entry for all but loc_0 whenever the
    valid count V divides N (fl(i / N) and fl(k / V) round the same quotient); V - 1 ties at the least, on which the bounds differ."""
    for N in (16, 4096, 4098, 8192, 9000):
        for pruned, V in (("all", N), ("half", N // 2), ("second", N // 2), ("first", N // 2)):
            for sign in (1.0, -1.0):
                w = sign * tie_weights(N, pruned)
                c = oracle.cdf(w)[0]
                loc = systematic_locs(N, 0.0)
                ties = np.isin(loc, c)
                assert ties.sum() >= V - 1, (N, pruned)
                up, lo = expected_slots(c, loc, True), expected_slots(c, loc, False)
                assert (up[ties] != lo[ties]).all()
                assert np.array_equal(oracle.resample_indices(w, "low_var", u32=0.0)[0], up)
                assert (w[up] != 0).all()  # the upper bound never selects a pruned particle


def _reference_low_var(w, u32):
    """The reference's low-variance resampler restated (modules/particle_filter.py:237, 251-261, 295-303): normalised weights,
    torch.cumsum in float64, locations i / N + float32(u32) / N modulo 1, and the two-pointer loop on `loc < weightsSum[i]`."""
    w = torch.as_tensor(np.asarray(w, dtype=np.float64))
    n = w.shape[0]
    sums = torch.cumsum(w / torch.sum(w), dim=0, dtype=torch.float64)
    locs = torch.remainder(torch.arange(n, dtype=torch.float64) / n + torch.tensor([u32], dtype=torch.float32) / n, 1).tolist()
    out, cur = [], 0
    for i, s in enumerate(sums.tolist()):
        while cur < n and locs[cur] < s:
            out.append(i)
            cur += 1
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("u32", [0.0, 0.5, float(np.nextafter(np.float32(1.0), np.float32(0.0)))])
def test_oracle_low_var_equals_the_reference_loop(oracle, u32):
    """The reference sums the NORMALISED weights one after the other, the oracle the raw ones in blocks and divides after: the two
    CDFs differ in the last bits unless every sum is exact.  So the tie cases (uniform and pruned uniform weights at u32 = 0,
    where N - 1 locations equal an entry) take N a power of two, where 1 / N and every running sum are exact in both; at u32 = 0.5
    and just below 1 the locations lie half a step and 2^-24 of a step (1e-11 at these sizes) from the entries, far beyond the
    1e-16 between the two CDFs, and any N serves."""
    rng = np.random.default_rng(11)
    sizes = (16, 256, 4096) if u32 == 0.0 else (16, 17, 1000, 4096, 4097)
    for N in sizes:
        sets = [("uniform", np.ones(N)), ("half pruned", tie_weights(N, "half").astype(np.float64)),
                ("second half pruned", tie_weights(N, "second").astype(np.float64)), ("random", rng.random(N))]
        for name, w in sets:
            got, status = oracle.resample_indices(w, "low_var", u32=u32)
            ref = _reference_low_var(w, u32)
            assert status == 0 and np.array_equal(got, ref), (name, N, u32)
            if u32 == 0.0 and name != "random":
                c = oracle.cdf(w)[0]
                assert np.isin(systematic_locs(N, 0.0), c).sum() >= int((w != 0).sum()) - 1


def _exact_weights(rng, N, total_log2=12):
    """Small integer weights (zeros among them) that add up to 2^total_log2: every running sum of w / total is exact."""
    w = rng.integers(0, 4, N).astype(np.float64)
    w[rng.random(N) < 0.3] = 0.0
    w[0] += 2.0 ** total_log2 - w.sum()
    assert w[0] > 0 and w.sum() == 2.0 ** total_log2
    return w


def test_torch_multinomial_is_the_lower_bound(oracle):
    """torch.multinomial(w, N, True) under torch.manual_seed(s) against the lower bound over ATen's own CDF (oracle.cdf_sequential)
    at the stream's draws (oracle.torch_rand64, pinned to torch.rand in tests/test_torch_stream.py), with weights whose running sums
    are exact - small integers over a total of 2^12 - so that the blocked CDF is the same array and an entry is a dyadic number a
    53-bit draw can equal.  The frames on which a draw of the stream EQUALS an entry are counted: over these 3000 seeds of 64 draws
    there is none (an entry k / 4096 needs the low 41 bits of a draw to be zero: about 1e-7 for all the draws together), so what
    this test holds torch to is the bound on the stream's ordinary draws; the tie itself is the next test's (a crafted generator
    state), beside ATen's source (`cum_dist[mid] < uniform_sample` moves left: the lower bound).  The global generator is left as
    it was found."""
    rng = np.random.default_rng(5)
    N, tie_frames = 64, 0
    state = torch.get_rng_state()
    try:
        for seed in range(3000):
            w = _exact_weights(rng, N)
            c = oracle.cdf_sequential(w)
            assert np.array_equal(c, oracle.cdf(w)[0])
            u = oracle.torch_rand64(seed, N)
            tie_frames += int(np.isin(u, c).any())
            torch.manual_seed(seed)
            idx = torch.multinomial(torch.as_tensor(w), N, True).numpy()
            assert np.array_equal(idx, expected_slots(c, u, False)), seed
            assert np.array_equal(idx, oracle.search_lower(c, u)), seed
    finally:
        torch.set_rng_state(state)
    print(f"torch.multinomial: {tie_frames} of 3000 seeded frames drew a CDF entry")


def _untemper(y):
    """The inverse of MT19937's output tempering, word by word."""
    y = np.asarray(y, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    y = y ^ (y >> np.uint64(18))
    y = y ^ ((y << np.uint64(15)) & np.uint64(0xEFC60000))
    t = y.copy()
    for _ in range(5):
        t = y ^ ((t << np.uint64(7)) & np.uint64(0x9D2C5680))
    y = t & np.uint64(0xFFFFFFFF)
    t = y.copy()
    for _ in range(3):
        t = y ^ (t >> np.uint64(11))
    return t & np.uint64(0xFFFFFFFF)


def _generator_state_drawing(u):
    """A state of torch's CPU generator whose next float64 uniforms are `u` (at most 311 multiples of 2^-53): the state words
    are the untempered halves of the draws, 623 of the 624 words of a block stay to be read (`left` = 624, `next` = 0; the legacy
    layout of torch.get_rng_state: seed u64, left i32, seeded i32, next u64, 624 words as u64)."""
    u = np.asarray(u, dtype=np.float64)
    v = (u * 2.0 ** 53).astype(np.uint64)
    assert u.shape[0] <= 311 and np.array_equal(v.astype(np.float64) * 2.0 ** -53, u)
    words = np.zeros(624, dtype=np.uint64)
    words[0:2 * len(u):2] = v >> np.uint64(32)
    words[1:2 * len(u):2] = v & np.uint64(0xFFFFFFFF)
    torch.manual_seed(0)
    s = torch.get_rng_state().numpy().copy()
    assert s.shape == (5056,)
    s[8:12] = np.frombuffer(np.int32(624).tobytes(), dtype=np.uint8)
    s[16:24] = 0
    s[24:24 + 624 * 8] = np.frombuffer(_untemper(words).astype("<u8").tobytes(), dtype=np.uint8)
    return torch.from_numpy(s)


def test_torch_multinomial_on_ties_from_a_crafted_generator_state(oracle):
    """No seed draws a CDF entry (the test above), but a generator STATE can: MT19937's tempering is a bijection, so the state whose
    next outputs are the halves of chosen draws is written down directly.  torch.rand under that state returns the draws - the
    check that the state is what it is meant to be - and torch.multinomial under it, every draw ON an entry of its own CDF, returns
    the lower bound and not the upper one, on every kind of the recipe."""
    rng = np.random.default_rng(9)
    state = torch.get_rng_state()
    try:
        for N in (17, 256, 311):
            w = _exact_weights(rng, N)
            c = oracle.cdf_sequential(w)
            assert np.array_equal(c, oracle.cdf(w)[0])
            for kind in RS_KINDS:
                u = crafted_draws(c, kind, rng)
                u = np.floor(u * 2.0 ** 53) * 2.0 ** -53   # (the filler draws: onto the generator's grid; entries are on it already)
                torch.set_rng_state(_generator_state_drawing(u))
                assert np.array_equal(torch.rand(N, dtype=torch.float64).numpy(), u)
                torch.set_rng_state(_generator_state_drawing(u))
                idx = torch.multinomial(torch.as_tensor(w), N, True).numpy()
                lo, up = expected_slots(c, u, False), expected_slots(c, u, True)
                assert np.array_equal(idx, lo), (N, kind)
                assert np.array_equal(idx, oracle.search_lower(c, u)), (N, kind)
                if kind == "on":
                    assert tie_share(c, u) >= 0.5 and (lo != up).sum() >= N // 2
    finally:
        torch.set_rng_state(state)
