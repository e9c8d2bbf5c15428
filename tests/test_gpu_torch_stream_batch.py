"""B of torch's CPU streams on the device at once (midas_mt19937_draws_batch, torch_rng.TorchCpuStreams) and the batch engines'
seeded mode (BatchFilterEngine.seed_torch_streams): trajectory b of a batch takes exactly the numbers a process of the reference
under torch.manual_seed(s_b) takes - torch.normal (N, 3) twice and torch.multinomial's N float64 uniforms per frame
(modules/particle_filter.py:326-335, :245).  Every comparison is on the bits.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _frame_spec(N):
    return [("normal", 0.0, 1.0, (N, 3)), ("normal", 0.0, 1.0, (N, 3)), ("rand64", N)]


def _host_frame(g, N):
    return (torch.normal(0.0, 1.0, size=(N, 3), generator=g), torch.normal(0.0, 1.0, size=(N, 3), generator=g),
            torch.rand(N, dtype=torch.float64, generator=g))


def _draws(st, spec, dev):
    outs, ev = st.draws_async(spec)
    if ev is not None:
        torch.cuda.current_stream(dev).wait_event(ev)
    return [o.cpu() for o in outs]


def _generators(seeds, lead=None):
    """Host generators under torch.manual_seed(s_b); lead[b] float64 uniforms drawn first (streams at different positions)."""
    gens = [torch.Generator().manual_seed(int(s)) for s in seeds]
    if lead is not None:
        for g, n in zip(gens, lead):
            if n:
                torch.rand(int(n), dtype=torch.float64, generator=g)
    return gens


# ---- 1. the kernel against torch itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pieces", [0, 6])
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("N", [16, 1000, 10000, 10007])
def test_batch_draws_equal_torch(dev, B, N, pieces):
    from midastouch_amd.torch_rng import TorchCpuStreams
    seeds = [1000 + 7 * b for b in range(B)]
    lead = [(b * 389) % 1500 for b in range(B)]  # 0 .. 1499 uniforms: rows inside different blocks, at different offsets
    host = _generators(seeds, lead)
    st = TorchCpuStreams(_generators(seeds, lead), dev, pieces=pieces)
    st.chain_after = 1  # in pieces from the second call on
    for call in range(4):
        if call == 2:  # a call behind a skip (skip_words is part of the jump distance)
            k = 333 + N
            st.skip_words(2 * k)
            for g in host:
                torch.rand(k, dtype=torch.float64, generator=g)
        got = _draws(st, _frame_spec(N), dev)
        for b, g in enumerate(host):
            ref = _host_frame(g, N)
            for i in range(3):
                assert torch.equal(got[i][b], ref[i]), (call, b, i)


@pytest.mark.parametrize("pieces", [0, 6])
def test_batch_of_one_is_the_single_stream_call(dev, pieces):
    from midastouch_amd.torch_rng import TorchCpuStream, TorchCpuStreams
    one, many = TorchCpuStream(77, dev, pieces=pieces), TorchCpuStreams([77], dev, pieces=pieces)
    one.chain_after = many.chain_after = 1
    for N in (10007, 10007, 10007, 300, 20000):
        spec = [("rand64", N), ("normal", 0.0, 1.0, (N, 3)), ("normal", 0.5, 2.0, (N, 3))]
        a = _draws(one, spec, dev)
        b = _draws(many, spec, dev)
        for x, y in zip(a, b):
            assert torch.equal(x, y[0]), N
    torch.cuda.synchronize()
    assert torch.equal(one.state, many.state[0]) and torch.equal(one._hist, many._hist[0])


def test_batch_draws_leave_state_and_history_of_single_calls(dev):
    from midastouch_amd.torch_rng import TorchCpuStream, TorchCpuStreams
    seeds = [5, 6, 7]
    singles = [TorchCpuStream(s, dev, pieces=6) for s in seeds]
    many = TorchCpuStreams(seeds, dev, pieces=6)
    for s in singles + [many]:
        s.chain_after = 1
    spec = _frame_spec(10000)
    for _ in range(3):
        _draws(many, spec, dev)
        for s in singles:
            _draws(s, spec, dev)
    torch.cuda.synchronize()
    for b, s in enumerate(singles):
        assert torch.equal(many.state[b], s.state) and torch.equal(many._hist[b], s._hist), b


# ---- 2. hand-over ---------------------------------------------------------------------------------------------------------------
def test_batch_streams_hand_over_to_host(dev):
    from midastouch_amd.torch_rng import TorchCpuStreams
    seeds = [11, 12, 13, 14]
    host = _generators(seeds)
    st = TorchCpuStreams(seeds, dev)
    st.chain_after = 1
    for N in (10000, 10000, 10000, 777):
        _draws(st, _frame_spec(N), dev)
        for g in host:
            _host_frame(g, N)
    st.skip_normal(48)  # a pending skip is applied by the hand-over
    for g in host:
        torch.normal(0.0, 1.0, size=(48,), generator=g)
    for b in (2, 0, 3, 1):
        g = torch.Generator()
        st.to_host(b, g)
        assert torch.equal(torch.rand(5, generator=g), torch.rand(5, generator=host[b])), b
    # and back: streams continued from host generators that stand at different positions
    st.from_host(host)
    got = _draws(st, [("rand64", 1000)], dev)[0]
    for b, g in enumerate(host):
        assert torch.equal(got[b], torch.rand(1000, dtype=torch.float64, generator=g)), b


# ---- 3. / 4. engines, seeded against host-drawn ----------------------------------------------------------------------------------
def _scene(B, N, K=3000, D=256, seed=0):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook("004_sugar_box", K=K, D=D, seed=1100 + seed)
    trs = [make_trajectory(cb, T=12, seed=2100 + seed + b) for b in range(B)]
    od = torch.as_tensor(np.stack([t.odoms for t in trs], axis=1))
    co = torch.as_tensor(np.stack([t.codes for t in trs], axis=1))
    gt = torch.as_tensor(np.stack([t.gt_poses for t in trs], axis=1))
    rng = np.random.default_rng(seed)
    start = torch.as_tensor(cb.poses[rng.integers(0, K, (B, N))])
    return cb, od, co, gt, start


def _host_draws(gens, N, sig_t, sig_r):
    tn, rot, u = [], [], []
    for g in gens:
        tn.append(torch.normal(0.0, sig_t, size=(N, 3), generator=g))
        rot.append(torch.normal(0.0, sig_r, size=(N, 3), generator=g))
        u.append(torch.rand(N, dtype=torch.float64, generator=g))
    return torch.stack(tn), torch.stack(rot), torch.stack(u)


def _same(a, b, t):
    assert torch.equal(a.ridx, b.ridx), f"frame {t}: resample indices"
    assert torch.equal(a.poses, b.poses), f"frame {t}: poses"
    assert torch.equal(a.weights, b.weights), f"frame {t}: weights"
    assert torch.equal(a.rmse, b.rmse), f"frame {t}: rmse"


def _run_pair(dev, cls, B, N, motion, frames, pipelined_reads=False, seeds=None, chain_after=None, pieces=0):
    cb, od, co, gt, start = _scene(B, N, seed=N % 7)
    seeds = seeds or [3000 + 17 * b for b in range(B)]
    a = cls(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)
    h = cls(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)
    for e in (a, h):
        e.set_particles(start)
        e.project_to_codebook()
    st = a.seed_torch_streams(seeds, motion=motion, pieces=pieces)
    if chain_after is not None:
        st.chain_after = chain_after
    gens = _generators(seeds)
    od, co, gt = od.to(dev), co.to(dev), gt.to(dev)
    for t in range(1, frames + 1):
        tn, rot, u = _host_draws(gens, N, a.sig_t, a.sig_r)
        if motion:
            a.step(od[t], co[t], gt[t])
        else:
            a.step(od[t], co[t], gt[t], tn=tn, rot=rot)
        h.step(od[t], co[t], gt[t], tn=tn, rot=rot, u=u)
        if pipelined_reads:
            if t == 4:
                a.flush()
                h.flush()
            if t % 3 == 0:
                _same(a, h, t)
        else:
            _same(a, h, t)
    _same(a, h, frames)
    return a, gens


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("N", [1000, 10000])
def test_eager_batch_engine_seeded_equals_host_draws(dev, N, motion):
    from midastouch_amd.engine import BatchFilterEngine
    a, gens = _run_pair(dev, BatchFilterEngine, 4, N, motion, 8)
    g = torch.Generator()
    a.torch_streams.to_host(2, g)
    assert torch.equal(torch.rand(9, generator=g), torch.rand(9, generator=gens[2]))


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("N", [1000, 10000])
def test_pipelined_batch_engine_seeded_equals_host_draws(dev, N, motion):
    from midastouch_amd.engine import PipelinedBatchFilterEngine
    a, gens = _run_pair(dev, PipelinedBatchFilterEngine, 4, N, motion, 8, pipelined_reads=True, chain_after=1, pieces=6)
    g = torch.Generator()
    a.torch_streams.to_host(1, g)
    if motion:  # the pipelined engine has drawn the next frame's normals already
        torch.normal(0.0, 1.0, size=(N, 3), generator=gens[1])
        torch.normal(0.0, 1.0, size=(N, 3), generator=gens[1])
    assert torch.equal(torch.rand(9, generator=g), torch.rand(9, generator=gens[1]))


def test_seeded_from_host_generators(dev):
    """seeds given as torch.Generators (at different positions) are continued where they stand."""
    from midastouch_amd.engine import BatchFilterEngine
    B, N = 3, 1000
    cb, od, co, gt, start = _scene(B, N, seed=3)
    a = BatchFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)
    h = BatchFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)
    for e in (a, h):
        e.set_particles(start)
    seeds, lead = [41, 42, 43], [0, 5, 1234]
    a.seed_torch_streams(_generators(seeds, lead), motion=True)
    gens = _generators(seeds, lead)
    for t in range(1, 5):
        tn, rot, u = _host_draws(gens, N, a.sig_t, a.sig_r)
        a.step(od[t].to(dev), co[t].to(dev))
        h.step(od[t].to(dev), co[t].to(dev), tn=tn, rot=rot, u=u)
        assert torch.equal(a.ridx, h.ridx) and torch.equal(a.poses, h.poses), t
    a.seed_torch_streams(None)  # back to Philox
    assert a.torch_streams is None
    a.step(od[5].to(dev), co[5].to(dev))


# ---- 5. against the oracle -------------------------------------------------------------------------------------------------------
def test_seeded_trajectory_equals_oracle(dev, oracle):
    """Trajectory b of a seeded batch against the CPU oracle driven by torch.manual_seed(s_b)'s own draws: resample indices equal."""
    from midastouch_amd.engine import BatchFilterEngine
    B, N, b = 3, 1500, 1
    cb, od, co, gt, start = _scene(B, N, K=3000, seed=5)
    ofl = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    eng = BatchFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)
    eng.set_particles(start)
    seeds = [901, 902, 903]
    eng.seed_torch_streams(seeds, motion=True)
    poses = start[b].numpy()
    torch.manual_seed(seeds[b])  # the reference's process for trajectory b
    for t in range(1, 7):
        tn = torch.normal(mean=0.0, std=eng.sig_t, size=(N, 3))
        rot = torch.normal(mean=0.0, std=eng.sig_r, size=(N, 3))
        u = torch.rand(N, dtype=torch.float64)
        ref = ofl.step(poses, od[t, b].numpy(), co[t, b].numpy(), tn.numpy(), rot.numpy(), u=u.numpy())
        eng.step(od[t].to(dev), co[t].to(dev))
        assert np.array_equal(eng.poses_prop[b].cpu().numpy(), ref["poses_prop"]), t
        assert np.array_equal(eng.ridx[b].cpu().numpy(), ref["ridx"]), t
        assert np.array_equal(eng.poses[b].cpu().numpy(), ref["poses"]), t
        poses = ref["poses"]
    assert len(np.unique(eng.ridx[b].cpu().numpy())) < N


# ---- 6. c5 size -------------------------------------------------------------------------------------------------------------------
def test_c5_size_seeded_motion_equals_host_draws(dev):
    """B = 64 x N = 10000 with the motion noise from the streams, in pieces from the second frame on."""
    from midastouch_amd.engine import PipelinedBatchFilterEngine
    a, _ = _run_pair(dev, PipelinedBatchFilterEngine, 64, 10000, True, 3, chain_after=1, pieces=6)
    assert a.torch_streams.pieces > 0 and a.torch_streams._polys  # the jump tables were used


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------
def test_seeded_errors(dev):
    from midastouch_amd._lib import MidasError
    from midastouch_amd.engine import BatchFilterEngine, PipelinedBatchFilterEngine
    B, N = 2, 1000
    cb, od, co, gt, start = _scene(B, N, seed=6)
    eng = BatchFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)
    eng.set_particles(start)
    with pytest.raises(MidasError):
        eng.seed_torch_streams([1, 2, 3])
    with pytest.raises(MidasError):
        eng.seed_torch_streams([torch.Generator()])
    low = BatchFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, resample="low_var", device=dev)
    with pytest.raises(MidasError):
        low.seed_torch_streams([1, 2])
    for e in (eng, PipelinedBatchFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)):
        e.set_particles(start)
        e.seed_torch_streams([1, 2], motion=True)
        tn = torch.zeros((B, N, 3))
        with pytest.raises(MidasError):
            e.step(od[1].to(dev), co[1].to(dev), tn=tn, rot=tn)
        with pytest.raises(MidasError):
            e.step(od[1].to(dev), co[1].to(dev), u=torch.rand((B, N), dtype=torch.float64))
