"""midas_mt19937_draws_counted_batch (TorchCpuStreams.draws_counted_async): B of torch's CPU streams drawn by one call, every
stream's sizes read from ITS row of a (B, 32) count tensor - row for row against midas_mt19937_draws_counted on a copy of that state
row and against torch's CPU generator itself, bit for bit: outputs, state rows, status words and the words consumed."""
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEEDS = (101, 202, 303, 404)
ADVANCED, ODD = 2, 333       # stream 2 has handed out 333 words before: the rows stand at different places in their blocks
SENTINEL = -7.5              # exactly representable in float32 and float64
NB, UB = 1024, 700           # bounds: normal rows (x 3 values), uniforms
NORMALS = (16, 311, 1000, 0)  # 48 values (a multiple of 16), 933 (tail redraw), 3000 (several blocks), none
UNIFORMS = (312, 313, 0, UB)  # exactly one block of 624 words, one more, none, the bound
MEAN, STD = 0.25, 2.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _generators(seeds=SEEDS):
    gs = [torch.Generator().manual_seed(s) for s in seeds]
    if len(gs) > ADVANCED:
        torch.randint(0, 2, (ODD,), generator=gs[ADVANCED])  # one 32-bit output per value
    return gs


def _streams(dev, seeds=SEEDS):
    from midastouch_amd.torch_rng import TorchCpuStreams
    return TorchCpuStreams(_generators(seeds), dev, overlap=False, pieces=0)


def _counts(dev, normals, uniforms):
    """(B, 32) counts written by fill kernels on the stream just before the draw: column 0 the normal rows, column 1 the uniforms."""
    c = torch.zeros((len(normals), 32), dtype=torch.int32, device=dev)
    for b, (n, m) in enumerate(zip(normals, uniforms)):
        c[b, 0:1].fill_(n)
        c[b, 1:2].fill_(m)
    return c


def _spec(cnt):
    return [("normal", MEAN, STD, cnt, 0, 3, NB), ("rand64", cnt, 1, UB)]


def _outs(dev, B):
    return [torch.full((B, 3 * NB), SENTINEL, dtype=torch.float32, device=dev), torch.full((B, UB), SENTINEL, dtype=torch.float64, device=dev)]


def _draw(dev, normals, uniforms, seeds=SEEDS):
    """One batch call: (streams, state rows before, outputs, status array (B, 7) with the words in column 3)."""
    st = _streams(dev, seeds)
    before = st.state.clone()
    cnt = _counts(dev, normals, uniforms)
    outs = _outs(dev, st.B)
    status = torch.zeros((st.B, 7), dtype=torch.int32, device=dev)
    got, ev = st.draws_counted_async(_spec(cnt), outs=outs, status=(status, 3, 7))
    assert ev is None and got[0] is outs[0] and got[1] is outs[1]
    torch.cuda.synchronize(dev)
    return st, before, outs, status, cnt


@pytest.fixture(scope="module")
def clean(dev):
    """The fault-free call every test compares with (computed once, never modified)."""
    return _draw(dev, NORMALS, UNIFORMS)


def _single(dev, row, cnt_row):
    """midas_mt19937_draws_counted on a copy of one state row with one row of counts: (outputs, state, status)."""
    from midastouch_amd.torch_rng import TorchCpuStream
    s = TorchCpuStream(0, dev, overlap=False, pieces=0)
    s.state.copy_(row)
    c = cnt_row.clone()
    outs = [o[0].clone() for o in _outs(dev, 1)]
    s.draws_counted_async(_spec(c), outs=outs)
    torch.cuda.synchronize(dev)
    return outs, s.state.clone(), s.counted_status()


def test_rows_equal_the_single_call_and_torch(dev, clean):
    st, before, outs, status, cnt = clean
    assert not status.any() and st.counted_status() == [0] * 4
    gens = _generators()
    assert len({int(r[624]) for r in before.cpu()}) > 1  # the rows do stand at different positions
    for b, (n, m) in enumerate(zip(NORMALS, UNIFORMS)):
        one, state1, bits1 = _single(dev, before[b], cnt[b])
        assert bits1 == 0
        for got, ref, k in ((outs[0][b], one[0], 3 * n), (outs[1][b], one[1], m)):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"row {b}: not the single call's output"
            assert bool((got[k:] == SENTINEL).all()), f"row {b}: written at or beyond its count"
        assert torch.equal(st.state[b], state1), f"row {b}: state row differs from the single call's"
        g = gens[b]
        if n:
            want = torch.normal(MEAN, STD, size=(n, 3), generator=g)
            assert torch.equal(outs[0][b, :3 * n].cpu(), want.reshape(-1)), f"row {b}: not torch.normal's numbers"
        want = torch.rand(m, dtype=torch.float64, generator=g)
        assert torch.equal(outs[1][b, :m].cpu(), want), f"row {b}: not torch.rand's numbers"
        g2 = torch.Generator()
        st.to_host(b, g2)
        assert torch.equal(torch.rand(8, dtype=torch.float64, generator=g2), torch.rand(8, dtype=torch.float64, generator=g)), \
            f"row {b}: words consumed differ from torch's"


@pytest.mark.parametrize("case", ["normal_short", "count_over_bound"])
def test_a_faulty_row_reports_alone_and_the_others_proceed(dev, clean, case):
    from midastouch_amd import _lib
    st0, _, outs0, _, _ = clean
    normals, uniforms = list(NORMALS), list(UNIFORMS)
    if case == "normal_short":
        normals[1], bit = 5, _lib.MT_STATUS_NORMAL_SHORT  # 15 values: ATen's scalar path
    else:
        uniforms[1], bit = UB + 1, _lib.MT_STATUS_COUNT_RANGE
    st, before, outs, status, _ = _draw(dev, normals, uniforms)
    want = torch.zeros((4, 7), dtype=torch.int32)
    want[1, 3] = bit
    assert torch.equal(status.cpu(), want), "the status bit belongs in the faulty row's own word only"
    assert torch.equal(st.state[1], before[1]), "a faulty row consumes nothing"
    assert all(bool((o[1] == SENTINEL).all()) for o in outs), "a faulty row writes nothing"
    for b in (0, 2, 3):
        assert torch.equal(st.state[b], st0.state[b]), f"row {b}: state differs from the fault-free call's"
        for o, o0 in zip(outs, outs0):
            assert torch.equal(o[b].view(torch.int32), o0[b].view(torch.int32)), f"row {b}: draws differ from the fault-free call's"


def test_batch_of_one_is_the_single_call(dev):
    st, before, outs, status, cnt = _draw(dev, NORMALS[1:2], UNIFORMS[1:2], SEEDS[:1])
    one, state1, bits1 = _single(dev, before[0], cnt[0])
    assert bits1 == 0 and not status.any()
    assert torch.equal(outs[0][0].view(torch.int32), one[0].view(torch.int32)) and torch.equal(outs[1][0].view(torch.int32), one[1].view(torch.int32))
    assert torch.equal(st.state[0], state1)
    want = torch.normal(MEAN, STD, size=(NORMALS[1], 3), generator=torch.Generator().manual_seed(SEEDS[0]))
    assert torch.equal(outs[0][0, :3 * NORMALS[1]].cpu(), want.reshape(-1))


def test_scratch_is_b_times_the_single_calls(dev, clean):
    from midastouch_amd.torch_rng import TorchCpuStream
    st, _, _, _, cnt = clean
    single = TorchCpuStream.counted_scratch_bytes(_spec(cnt[0]))
    assert st.counted_scratch_bytes(_spec(cnt)) <= st.B * single
    assert st.counted_scratch_bytes(_spec(cnt)) >= st.B * 4 * (3 * NB + 16 + 2 * UB)  # (the raw words at the bounds)
