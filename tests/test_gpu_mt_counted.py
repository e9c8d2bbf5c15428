"""midas_mt19937_draws_counted: draws of torch's CPU stream whose sizes stand in device memory (the reference's loop: normal
(n, 3) twice with the live count, then n_set float64 uniforms, modules/particle_filter.py:326-335, :245) - against the
host-counted midas_mt19937_draws on a copy of the same state and against torch's CPU generator itself, bit for bit: the outputs,
the 626-word state row afterwards and, handed back by to_host(), the next 8 torch.rand values."""
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 4242
SENTINEL = -7.5  # exactly representable in float32 and float64: what the outputs hold where the call must not write


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _count(dev, *values):
    """Counts no host code hands over: each element is written by a fill kernel enqueued on the stream just before the draw."""
    c = torch.empty(len(values), dtype=torch.int32, device=dev)
    for i, v in enumerate(values):
        c[i:i + 1].fill_(v)
    return c


def _stream(dev, prior_skip=0, pos0=False):
    """A device stream under manual_seed(SEED) that a prior call has stepped `prior_skip` words on.  pos0: the state row rewritten as
    'first block twisted, none of its words consumed' - the same place in the stream as the fresh seed ('a twist is due')."""
    from midastouch_amd.torch_rng import TorchCpuStream
    st = TorchCpuStream(SEED, dev, pieces=0)
    if pos0:
        st.skip_words(1).rand64(0)
        st.state[624:625].fill_(0)
    elif prior_skip:
        st.skip_words(prior_skip).rand64(0)
    return st


def _torch_side(prior_skip):
    torch.manual_seed(SEED)
    torch.randint(0, 2, (prior_skip,))  # one 32-bit output per value


def _sentinel_outs(dev, spec):
    """Bound-sized outputs of a counted spec, filled with the sentinel."""
    outs = []
    for it in spec:
        numel, dt = (it[3], torch.float64) if it[0] == "rand64" else (it[5] * it[6], torch.float32)
        outs.append(torch.full((numel,), SENTINEL, dtype=dt, device=dev))
    return outs


def _check(dev, ref_spec, counted_spec, counts, torch_draws, prior_skip=0, pos0=False, pending_skip=0):
    """ref_spec: the host-counted draws; counted_spec: the same draws by count; counts: their numels; torch_draws(): the same draws on
    torch's CPU generator (already seeded and skipped)."""
    _torch_side(prior_skip + pending_skip)
    want = torch_draws()
    next8 = torch.rand(8, dtype=torch.float64)
    a, b = _stream(dev, prior_skip, pos0), _stream(dev, prior_skip, pos0)
    a.skip_words(pending_skip), b.skip_words(pending_skip)
    if sum(counts):
        ref, ev = a.draws_async(ref_spec)
    else:
        ref, ev = [torch.empty(0) for _ in ref_spec], None  # (nothing to draw: the state of the seed itself is the reference)
    outs = _sentinel_outs(dev, counted_spec)
    got, ev2 = b.draws_counted_async(counted_spec, outs=outs)
    for e in (ev, ev2):
        if e is not None:
            e.synchronize()
    torch.cuda.synchronize(dev)
    assert b.counted_status() == 0
    for g, r, w, n in zip(got, ref, want, counts):
        assert torch.equal(g[:n].cpu(), w.reshape(-1)), "not torch's numbers"
        assert torch.equal(g[:n].cpu(), r.reshape(-1).cpu()), "not the host-counted call's numbers"
        assert bool((g[n:] == SENTINEL).all()), "written at or beyond per * count"
    assert torch.equal(a.state.cpu(), b.state.cpu()), "state row differs from the host-counted call's"
    assert b._hist_words == 0 and b.pending_skip == 0  # the next host-counted call walks sequentially
    g = torch.Generator()
    b.to_host(g)
    assert torch.equal(torch.rand(8, dtype=torch.float64, generator=g), next8), "words consumed differ from torch's"
    return b


@pytest.mark.parametrize("n", [6, 208, 209, 1000])  # 18 values: tail redraw inside a block; 624: a multiple of 16, exactly a block; 627; several blocks
def test_counted_normal_equals_host_counted_and_torch(dev, n):
    bound = n + 37
    cnt = _count(dev, 0, n)
    _check(dev, [("normal", 0.25, 2.0, (n, 3))], [("normal", 0.25, 2.0, cnt, 1, 3, bound)], [3 * n],
           lambda: [torch.normal(0.25, 2.0, size=(n, 3))])


@pytest.mark.parametrize("n", [0, 1, 311, 312, 313, 2000])  # 312 doubles are exactly 624 words
def test_counted_rand64_equals_host_counted_and_torch(dev, n):
    cnt = _count(dev, n)
    _check(dev, [("rand64", n)], [("rand64", cnt, 0, n + 5)], [n], lambda: [torch.rand(n, dtype=torch.float64)])


@pytest.mark.parametrize("start", [0, 1, 623, 624, "pos0"])
def test_counted_frame_of_three_segments_from_every_start_position(dev, start):
    """[normal n, normal n, rand64 m], n != m, the reference's frame - from a state a prior skip has left 0, 1, 623 or 624 words into
    the stream (0 and 624: a twist is due) and from position 0 of a twisted block."""
    n, m = 1000, 777
    cnt = _count(dev, n, m)
    pos0 = start == "pos0"
    _check(dev, [("normal", 0.0, 2e-4, (n, 3)), ("normal", 0.0, 0.5, (n, 3)), ("rand64", m)],
           [("normal", 0.0, 2e-4, cnt, 0, 3, 1400), ("normal", 0.0, 0.5, cnt, 0, 3, n), ("rand64", cnt, 1, 1024)], [3 * n, 3 * n, m],
           lambda: [torch.normal(0.0, 2e-4, size=(n, 3)), torch.normal(0.0, 0.5, size=(n, 3)), torch.rand(m, dtype=torch.float64)],
           prior_skip=0 if pos0 else start, pos0=pos0)


def test_counted_call_applies_its_own_skip_and_a_zero_segment_consumes_nothing(dev):
    n = 100
    cnt = _count(dev, n, 0)
    _check(dev, [("rand64", n), ("rand64", 0), ("normal", 0.0, 1.0, (n, 3))],
           [("rand64", cnt, 0, 128), ("rand64", cnt, 1, 64), ("normal", 0.0, 1.0, cnt, 0, 3, 128)], [n, 0, 3 * n],
           lambda: [torch.rand(n, dtype=torch.float64), torch.empty(0, dtype=torch.float64), torch.normal(0.0, 1.0, size=(n, 3))],
           pending_skip=7)


@pytest.mark.parametrize("case", ["normal_short", "count_over_bound"])
def test_counted_failure_sets_its_bit_and_touches_nothing(dev, case):
    """n = 5 (15 normal values: ATen's scalar path) resp. a count above its bound, each in a call of its own with a valid segment in
    front: the status bit, state and outputs untouched, and a following valid call is torch's."""
    from midastouch_amd import _lib
    from midastouch_amd.torch_rng import TorchCpuStream
    st = TorchCpuStream(SEED, dev)
    torch.cuda.synchronize(dev)  # (the seed is written on the generator's stream)
    before = st.state.clone()
    cnt = _count(dev, 64, 5, 300)
    bad = ("normal", 0.0, 1.0, cnt, 1, 3, 16) if case == "normal_short" else ("rand64", cnt, 2, 299)
    spec = [("rand64", cnt, 0, 64), bad]
    outs = _sentinel_outs(dev, spec)
    st.skip_words(3)
    _, ev = st.draws_counted_async(spec, outs=outs)
    ev.synchronize()
    assert st.counted_status() == (_lib.MT_STATUS_NORMAL_SHORT if case == "normal_short" else _lib.MT_STATUS_COUNT_RANGE)
    assert torch.equal(st.state.cpu(), before.cpu())
    assert all(bool((o == SENTINEL).all()) for o in outs)
    st._status.zero_()
    torch.manual_seed(SEED)
    want = torch.rand(64, dtype=torch.float64)
    (u,), ev = st.draws_counted_async([("rand64", cnt, 0, 64)])
    ev.synchronize()
    assert st.counted_status() == 0 and torch.equal(u.cpu(), want)
