"""The `rand32` draw kind of the device replica of torch's CPU generator (csrc/mt19937.hip, MIDAS_MT_SEGMENT_RAND32): the float32
`torch.rand(1)` the reference's systematic resampler takes as its offset (modules/particle_filter.py:291) - one generator output, its
low 24 bits times 2^-24 - in the three call forms: TorchCpuStream.rand32() / an item of draws_async, the counted call (the draw
happens when a control word in device memory is not zero) and the counted batch call.  Against torch itself, bit for bit: the value,
the words consumed (the stream handed back to a host generator continues equal to the host's)."""
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SENTINEL = -7.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _stream(dev, seed):
    from midastouch_amd.torch_rng import TorchCpuStream
    return TorchCpuStream(seed, dev, overlap=False, pieces=0)


def _continues_equal(st, n=8, b=None):
    """The stream, handed back to a host generator, goes on with the numbers torch's default generator goes on with."""
    g = torch.Generator()
    st.to_host(g) if b is None else st.to_host(b, g)
    assert torch.equal(torch.rand(n, dtype=torch.float64, generator=g), torch.rand(n, dtype=torch.float64))


@pytest.mark.parametrize("seed", (0, 42, 3001, 2**32 + 5))
def test_rand32_equals_torch_rand1_after_every_kind_of_draw(dev, seed):
    st = _stream(dev, seed)
    torch.manual_seed(seed)
    got = st.rand32()
    assert got.dtype == torch.float32 and got.shape == (1,) and got.is_cuda
    assert torch.equal(got.cpu(), torch.rand(1)), "after manual_seed"
    a = st.normal(0.0, 2e-4, (1000, 3))
    b = st.normal(0.0, 0.5, (1000, 3))
    assert torch.equal(a.cpu(), torch.normal(0.0, 2e-4, size=(1000, 3))) and torch.equal(b.cpu(), torch.normal(0.0, 0.5, size=(1000, 3)))
    assert torch.equal(st.rand32().cpu(), torch.rand(1)), "after a normal (n, 3) pair"
    assert torch.equal(st.rand64(311).cpu(), torch.rand(311, dtype=torch.float64))
    assert torch.equal(st.rand32().cpu(), torch.rand(1)), "after a rand64(n)"
    assert torch.equal(st.rand32().cpu(), torch.rand(1)), "after another rand32"
    # as an item of draws_async: the float64 that holds the float32 value exactly, between other draws of one walk
    (n1, u, r), ev = st.draws_async([("normal", 0.0, 0.5, (100, 3)), ("rand32",), ("rand64", 5)])
    assert ev is None and u.dtype == torch.float64 and u.shape == (1,)
    assert torch.equal(n1.cpu(), torch.normal(0.0, 0.5, size=(100, 3)))
    assert torch.equal(u.cpu(), torch.rand(1).double()) and torch.equal(r.cpu(), torch.rand(5, dtype=torch.float64))
    _continues_equal(st)


@pytest.mark.parametrize("before", (620, 621, 622, 623, 624, 625, 1247, 1248))
def test_rand32_at_the_block_boundary(dev, before):
    """The draw as word `before` of the stream: the last words of a 624-word block, the first of the next, and the same one block on."""
    st = _stream(dev, 7)
    torch.manual_seed(7)
    assert torch.equal(st.rand64(before // 2).cpu(), torch.rand(before // 2, dtype=torch.float64))
    if before % 2:
        assert torch.equal(st.rand32().cpu(), torch.rand(1))
    assert torch.equal(st.rand32().cpu(), torch.rand(1)), before
    assert torch.equal(st.rand32().cpu(), torch.rand(1)), before
    _continues_equal(st)


def test_rand32_skip_and_hand_over(dev):
    """skip_rand32 steps over a host draw; from_host / to_host leave the host generator where a host run stands."""
    st = _stream(dev, 11)
    torch.manual_seed(11)
    torch.normal(0.0, 1.0, size=(64, 3))
    torch.rand(1)                      # a host draw ...
    st.skip_normal(192).skip_rand32()  # ... stepped over on the device
    assert torch.equal(st.rand32().cpu(), torch.rand(1))
    st.from_host()
    want = torch.rand(1)
    assert torch.equal(st.rand32().cpu(), want)
    st.skip_rand32()
    torch.rand(1)
    _continues_equal(st)
    from midastouch_amd import _lib
    with pytest.raises(_lib.MidasError):
        st.draws_async([("rand32", 2)])  # only the single draw is modelled


@pytest.mark.parametrize("word", (0, 1, 4096))
def test_counted_rand32_draws_by_the_control_word(dev, word):
    """The counted form: 0 -> no value, no word consumed (the stream stands still); 1 and 4096 -> one value, one word."""
    st = _stream(dev, 21)
    torch.manual_seed(21)
    ctl = torch.zeros(32, dtype=torch.int32, device=dev)
    ctl[3:4].fill_(word)
    ctl[1:2].fill_(100)
    tn = torch.full((3 * 128,), SENTINEL, dtype=torch.float32, device=dev)
    out = torch.full((4096,), SENTINEL, dtype=torch.float64, device=dev)
    before = st.state.clone()
    # a frame's two calls: the normals sized by one word, then the offset switched by another
    st.draws_counted_async([("normal", 0.0, 0.5, ctl, 1, 3, 128)], outs=[tn])
    mid = st.state.clone()
    got, ev = st.draws_counted_async([("rand32", ctl, 3, 4096)], outs=[out])
    torch.cuda.synchronize(dev)
    assert ev is None and got[0] is out and st.counted_status() == 0
    assert torch.equal(tn[:300].cpu(), torch.normal(0.0, 0.5, size=(100, 3)).reshape(-1))
    assert not torch.equal(before, mid)
    if word == 0:
        assert torch.equal(st.state, mid), "the stream moved on a control word of 0"
        assert bool((out == SENTINEL).all())
    else:
        assert torch.equal(out[:1].cpu(), torch.rand(1).double())
        assert bool((out[1:] == SENTINEL).all()), "written beyond the one value"
    _continues_equal(st)


def test_counted_rand32_word_beyond_its_bound_draws_nothing(dev):
    from midastouch_amd import _lib
    st = _stream(dev, 22)
    ctl = torch.full((32,), 5000, dtype=torch.int32, device=dev)
    out = torch.full((4096,), SENTINEL, dtype=torch.float64, device=dev)
    before = st.state.clone()
    st.draws_counted_async([("rand32", ctl, 0, 4096)], outs=[out])
    torch.cuda.synchronize(dev)
    assert st.counted_status() == _lib.MT_STATUS_COUNT_RANGE
    assert torch.equal(st.state, before) and bool((out == SENTINEL).all())


def test_counted_batch_rand32_mixed_words_and_seeds(dev):
    """B = 3 streams on different seeds, control words 4096 / 0 / 1: rows 0 and 2 draw their torch.rand(1), row 1 stands still; every
    row is the single counted call on it."""
    from midastouch_amd.torch_rng import TorchCpuStreams
    seeds, words, CAP = (101, 202, 303), (4096, 0, 1), 4096
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    torch.randint(0, 2, (623,), generator=gens[2])  # row 2 stands on the last word of its block
    st = TorchCpuStreams(gens, dev, overlap=False, pieces=0)
    ctl = torch.zeros((3, 32), dtype=torch.int32, device=dev)
    for b, w in enumerate(words):
        ctl[b, 15:16].fill_(w)
    out = torch.full((3, CAP), SENTINEL, dtype=torch.float64, device=dev)
    before = st.state.clone()
    got, ev = st.draws_counted_async([("rand32", ctl, 15, CAP)], outs=[out])
    torch.cuda.synchronize(dev)
    assert ev is None and got[0] is out and st.counted_status() == [0, 0, 0]
    for b, w in enumerate(words):
        one = _stream(dev, 0)
        one.state.copy_(before[b])
        o1 = torch.full((CAP,), SENTINEL, dtype=torch.float64, device=dev)
        one.draws_counted_async([("rand32", ctl[b].clone(), 15, CAP)], outs=[o1])
        torch.cuda.synchronize(dev)
        assert torch.equal(out[b], o1) and torch.equal(st.state[b], one.state), f"row {b}: not the single call"
        if w:
            assert torch.equal(out[b, :1].cpu(), torch.rand(1, generator=gens[b]).double()), f"row {b}"
        else:
            assert torch.equal(st.state[b], before[b]) and bool((out[b] == SENTINEL).all()), f"row {b} moved"
        assert bool((out[b, 1:] == SENTINEL).all())
        g = torch.Generator()
        st.to_host(b, g)
        assert torch.equal(torch.rand(8, dtype=torch.float64, generator=g), torch.rand(8, dtype=torch.float64, generator=gens[b])), f"row {b}"
    # the uncounted batch form: one value a stream
    st.from_host(gens)
    (u,), ev = st.draws_async([("rand32",)])
    torch.cuda.synchronize(dev)
    assert u.shape == (3, 1) and u.dtype == torch.float64
    for b in range(3):
        assert torch.equal(u[b].cpu(), torch.rand(1, generator=gens[b]).double()), f"row {b}"
