"""`ShardedFilterEngine(estimate=True)` on the device: after every frame every shard holds the pose estimate of ALL particles
(filter/filter.py:184-186), bit for bit what `FilterEngine(shards * n_loc, estimate=True)` leaves when n_loc is a multiple of
4096 - in every exchange form, in lock-step shards of one process, under a one-rank RCCL group (the one-call entries and
`run()`), and in two processes sharing the GPU over gloo; the finish built for thousands of blocks against the fixed-N engines'
finish on the same partials.  Needs an MI355X."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


class FakeComm:
    def __init__(self, r, w):
        self.rank, self.world = r, w

    def all_gather(self, t):
        raise AssertionError("lock-step test never calls the communicator")

    all_to_all = all_gather


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.allclose(a, b, rtol=0.0, atol=0.0, equal_nan=True)


def _scene(N, K=4000, D=256, T=12, seed=0):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook(K=K, D=D, seed=1000)
    traj = make_trajectory(cb, T=T, seed=2000)
    start = cb.poses[np.random.default_rng(seed).integers(0, K, N)]
    return cb, traj, start


def _shards(cb, start, dev, shards, n_loc, exchange, be=None, **kw):
    from midastouch_amd.dist import HipShardBackend, ShardedFilterEngine, connect_local_peers
    be = be or HipShardBackend(cb.poses, cb.embeddings, cb.mesh_vertices, dev)
    engs = [ShardedFilterEngine(num_particles=n_loc, backend=be, comm=FakeComm(r, shards), exchange=exchange, **kw) for r in range(shards)]
    if exchange in ("peer", "peer_c"):
        connect_local_peers(engs, exchange)
    for r, e in enumerate(engs):
        e.set_particles(torch.as_tensor(start[r * n_loc:(r + 1) * n_loc]))
        e.project_to_codebook()
    return engs, be


STATE = ("nn_idx", "weights", "ridx", "poses", "weights_res", "hint")


@pytest.mark.parametrize("exchange", ["a2a", "allgather", "a2a_fixed", "peer", "peer_c"])
@pytest.mark.parametrize("shards,mode", [(2, "weighted_random"), (3, "low_var"), (1, "weighted_random")])
def test_every_exchange_form_against_the_single_engine(dev, shards, mode, exchange):
    """Every frame, every shard: `estimate` equals the single engine's bit for bit; the shard state still equals the single
    engine's; a twin set of shards built WITHOUT the keyword ends in the same state (the estimate changes nothing else)."""
    from midastouch_amd._lib import MidasError
    from midastouch_amd.dist import run_lockstep
    from midastouch_amd.engine import FilterEngine
    n_loc = 4096 * 2
    N = shards * n_loc
    cb, traj, start = _scene(N)
    single = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, resample=mode, device=dev, estimate=True)
    single.set_particles(torch.as_tensor(start))
    single.project_to_codebook()
    engs, be = _shards(cb, start, dev, shards, n_loc, exchange, resample=mode, estimate=True)
    twins, _ = _shards(cb, start, dev, shards, n_loc, exchange, be=be, resample=mode)
    for t in range(1, 10):
        od, code, gt = (torch.as_tensor(a[t]).to(dev) for a in (traj.odoms, traj.codes, traj.gt_poses))
        single.step(od, code, gt=gt)
        run_lockstep(engs, [((od, code), {"gt": gt}) for _ in engs])
        run_lockstep(twins, [((od, code), {"gt": gt}) for _ in twins])
        sc, ss = single.estimate
        assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(ss).all())
        for e in engs:
            c, s = e.estimate
            assert c.shape == (4, 4) and s.shape == (3,) and c.dtype == torch.float32 and c.device == sc.device
            assert torch.equal(c, sc) and torch.equal(s, ss), (t, c, sc, s, ss)
        for name in STATE:
            got = torch.cat([getattr(e, name) for e in engs])
            assert torch.equal(got, getattr(single, name)), (t, name)
            assert torch.equal(got, torch.cat([getattr(e, name) for e in twins])), (t, name)
    for e in twins:
        assert not hasattr(e.st, "est_part")
        with pytest.raises(MidasError, match="estimate=True"):
            e.estimate


def test_codebook_rows_sharded(dev):
    from midastouch_amd.dist import HipShardBackend, ShardedFilterEngine, run_lockstep
    from midastouch_amd.engine import FilterEngine
    shards, n_loc = 2, 4096
    N = shards * n_loc
    cb, traj, start = _scene(N, T=8)
    single = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, device=dev, estimate=True)
    single.set_particles(torch.as_tensor(start))
    engs = []
    for r in range(shards):
        be = HipShardBackend(cb.poses, cb.embeddings, cb.mesh_vertices, dev, row_shard=(r, shards))
        e = ShardedFilterEngine(num_particles=n_loc, backend=be, comm=FakeComm(r, shards), estimate=True)
        e.set_particles(torch.as_tensor(start[r * n_loc:(r + 1) * n_loc]))
        engs.append(e)
    for t in range(1, 6):
        od, code = torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev)
        single.step(od, code)
        run_lockstep(engs, [((od, code), {}) for _ in engs])
        for e in engs:
            assert torch.equal(e.estimate[0], single.estimate[0]) and torch.equal(e.estimate[1], single.estimate[1]), t
        assert torch.equal(torch.cat([e.weights for e in engs]), single.weights), t


@pytest.mark.parametrize("exchange", ["a2a", "allgather", "peer"])
def test_host_uniforms_replicated(dev, exchange):
    from midastouch_amd.dist import run_lockstep
    from midastouch_amd.engine import FilterEngine
    shards, n_loc = 2, 4096
    N = shards * n_loc
    cb, traj, start = _scene(N, K=3000, D=128, T=6, seed=3)
    single = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, device=dev, estimate=True)
    single.set_particles(torch.as_tensor(start))
    single.project_to_codebook()
    engs, _ = _shards(cb, start, dev, shards, n_loc, exchange, estimate=True)
    for t in range(1, 5):
        od, code = torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev)
        torch.manual_seed(77 + t)
        u = torch.rand(N, dtype=torch.float64).to(dev)
        single.step(od, code, u=u)
        run_lockstep(engs, [((od, code), {"u": u}) for _ in engs])
        for e in engs:
            assert torch.equal(e.estimate[0], single.estimate[0]) and torch.equal(e.estimate[1], single.estimate[1]), t
        assert torch.equal(torch.cat([e.ridx for e in engs]), single.ridx), t


def test_softmax_off(dev):
    """Raw scores of mixed sign make a CDF that is not monotone: the owner-side search of the sharded frame and the single engine's
    search may then pick different sources (the reference's p = w / sum(w) is undefined there; tests/test_gpu_estimate.py records
    the same between two single engines).  The estimate is taken BEFORE the resample, so it is compared every frame on the same
    propagated poses and weights, and both sides then go on from the single engine's resampled set."""
    from midastouch_amd.dist import run_lockstep
    from midastouch_amd.engine import FilterEngine
    shards, n_loc = 2, 4096
    N = shards * n_loc
    cb, traj, start = _scene(N, T=6)
    single = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, device=dev, softmax=False, estimate=True)
    single.set_particles(torch.as_tensor(start))
    single.project_to_codebook()
    engs, _ = _shards(cb, start, dev, shards, n_loc, "a2a", softmax=False, estimate=True)
    for t in range(1, 5):
        od, code = torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev)
        single.step(od, code)
        run_lockstep(engs, [((od, code), {}) for _ in engs])
        assert torch.equal(torch.cat([e.poses_prop for e in engs]), single.poses_prop), t
        assert torch.equal(torch.cat([e.weights for e in engs]), single.weights), t
        for e in engs:
            assert torch.equal(e.estimate[0], single.estimate[0]) and torch.equal(e.estimate[1], single.estimate[1]), t
        same = torch.equal(torch.cat([e.ridx for e in engs]), single.ridx)
        mixed = bool((single.weights < 0).any()) and bool((single.weights > 0).any())
        print(f"softmax off, frame {t}: weights of mixed sign: {mixed}; sharded and single resample indices equal: {same}")
        nxt = single.poses.clone()  # the next frame of both sides starts from the single engine's resampled set
        single.set_particles(nxt)
        for r, e in enumerate(engs):
            e.set_particles(nxt[r * n_loc:(r + 1) * n_loc])


def test_all_particles_pruned(dev):
    """A world started 1 m off the object: every weight 0, the flatten branch (every particle counts 1)."""
    from midastouch_amd.dist import run_lockstep
    from midastouch_amd.engine import FilterEngine
    shards, n_loc = 2, 4096
    N = shards * n_loc
    cb, traj, start = _scene(N, T=4)
    start = start.copy()
    start[:, :3, 3] += 1.0
    single = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, device=dev, estimate=True)
    single.set_particles(torch.as_tensor(start))
    engs, _ = _shards(cb, start, dev, shards, n_loc, "a2a", estimate=True)
    for e, r in zip(engs, range(shards)):
        e.set_particles(torch.as_tensor(start[r * n_loc:(r + 1) * n_loc]))  # (not projected: they stay off the object)
    for t in range(1, 3):
        od, code = torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev)
        single.step(od, code)
        run_lockstep(engs, [((od, code), {}) for _ in engs])
        assert float(torch.cat([e.weights for e in engs]).abs().max()) == 0.0
        c0, s0 = engs[0].estimate
        assert bool(torch.isfinite(c0).all()) and bool(torch.isfinite(s0).all())
        for e in engs:
            assert torch.equal(e.estimate[0], c0) and torch.equal(e.estimate[1], s0)
        assert torch.equal(c0, single.estimate[0]) and torch.equal(s0, single.estimate[1])


def test_more_than_256_block_records(dev):
    """Two shards of 131 x 4096 particles: 262 global 4096-slot block records (more than a kernel stages in LDS) and 4192 moment
    blocks - the size class the finish over gathered partials is built for."""
    from midastouch_amd.dist import run_lockstep
    from midastouch_amd.engine import FilterEngine
    shards, n_loc = 2, 131 * 4096
    N = shards * n_loc
    cb, traj, start = _scene(N, T=5)
    single = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, device=dev, estimate=True)
    single.set_particles(torch.as_tensor(start))
    single.project_to_codebook()
    engs, _ = _shards(cb, start, dev, shards, n_loc, "auto", estimate=True)
    assert engs[0].st.est_part.numel() * shards == 4192 * 36
    for t in range(1, 4):
        od, code = torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev)
        single.step(od, code)
        run_lockstep(engs, [((od, code), {}) for _ in engs])
        for e in engs:
            assert torch.equal(e.estimate[0], single.estimate[0]) and torch.equal(e.estimate[1], single.estimate[1]), t
        assert torch.equal(torch.cat([e.weights for e in engs]), single.weights), t


def test_n_not_a_multiple_of_256(dev, oracle):
    """n_loc = 5000: "each rank's own blocks, ranks in order" - equal on both shards, and the oracle's estimate of the
    concatenated shards within the tolerances of tests/test_gpu_estimate.py."""
    from midastouch_amd.dist import run_lockstep
    shards, n_loc = 2, 5000
    N = shards * n_loc
    cb, traj, start = _scene(N, T=6)
    engs, _ = _shards(cb, start, dev, shards, n_loc, "a2a", estimate=True)
    for t in range(1, 5):
        od, code = torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev)
        run_lockstep(engs, [((od, code), {}) for _ in engs])
        c0, s0 = engs[0].estimate
        assert torch.equal(engs[1].estimate[0], c0) and torch.equal(engs[1].estimate[1], s0)
        pp = torch.cat([e.poses_prop for e in engs]).cpu().numpy()
        w = torch.cat([e.weights for e in engs]).cpu().numpy()
        _, oc, os_ = oracle.cluster_centers(pp, w, np.zeros(N, dtype=np.int64))
        assert np.abs(c0.cpu().numpy() - oc[0]).max() < 2e-6
        np.testing.assert_allclose(s0.cpu().numpy(), os_[0], rtol=2e-4, atol=1e-9)


@pytest.mark.parametrize("N", [1, 255, 256, 4097, 30_011, 1_000_000])
def test_new_finish_against_the_fixed_n_finish(dev, N):
    """The same partials (k_estimate_moments on one trajectory) through ops.pose_estimate's finish and through
    midas_shard_estimate_finish: centre and spread equal bit for bit, NaN patterns included."""
    from midastouch_amd import _lib, ops
    from midastouch_amd._lib import _ptr
    from test_cluster_centers import _clustered
    for variant in ("weights", "flat", "nan"):
        P, w, _ = _clustered([N], seed=40 + N % 7)
        if variant == "flat":
            w = np.full(N, 0.37)
        P, w = torch.as_tensor(P).to(dev).contiguous(), torch.as_tensor(w).to(dev).contiguous()
        if variant == "nan":
            w[N // 2] = float("nan")
        old_c, old_s = ops.pose_estimate(P[None], w[None])
        ctx = _lib.context(dev)
        nb = -(-N // 256)
        part = torch.empty(nb * 36, dtype=torch.float64, device=dev)
        c, s = torch.empty((4, 4), dtype=torch.float32, device=dev), torch.empty((3,), dtype=torch.float32, device=dev)
        ctx.call("midas_shard_estimate_moments", N, _ptr(P), _ptr(w), _ptr(part))
        ctx.call("midas_shard_estimate_finish", nb, _ptr(part), _ptr(c), _ptr(s))
        torch.cuda.synchronize()
        assert _same(c, old_c[0]) and _same(s, old_s[0]), (N, variant, c, old_c[0], s, old_s[0])


# ---- world 1 under a one-rank nccl group: the one-call entries and run(), in a child process of its own ----------------------
def _nccl1_worker(rank, port):
    import torch.distributed as dist
    from midastouch_amd.dist import ShardedFilterEngine
    from midastouch_amd.engine import FilterEngine
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        n, T = 4096, 12
        cb, traj, start = _scene(n, K=2000, T=T + 2)
        ods, codes = torch.as_tensor(traj.odoms[1:T + 1]).to(dev), torch.as_tensor(traj.codes[1:T + 1]).to(dev)
        ref = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, n, device=dev, estimate=True)
        a = ShardedFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, n, device=dev, exchange="peer_c", estimate=True)
        b = ShardedFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, n, device=dev, exchange="peer_c", estimate=True)
        assert a.world == 1 and a.exchange == "peer_c" and a._ccomm is not None, a.peer_error
        for e in (ref, a, b):
            e.set_particles(torch.as_tensor(start))
            e.project_to_codebook()
        a.run(ods, codes)
        log = a.estimate_log
        assert log[0].shape == (T, 4, 4) and log[1].shape == (T, 3)
        for t in range(T):  # the twin, stepped frame by frame through the one-call step entry; and the single engine
            b.step(ods[t], codes[t])
            ref.step(ods[t], codes[t])
            assert torch.equal(log[0][t], b.estimate[0]) and torch.equal(log[1][t], b.estimate[1]), t
            assert torch.equal(log[0][t], ref.estimate[0]) and torch.equal(log[1][t], ref.estimate[1]), t
        assert b.estimate[0].data_ptr() == b.st.est_center.data_ptr()
        assert torch.equal(a.estimate[0], log[0][T - 1]) and a.estimate[0].data_ptr() == log[0][T - 1].data_ptr()
        assert torch.equal(a.ridx, b.ridx) and torch.equal(a.weights, b.weights) and torch.equal(a.poses, b.poses)
        first = (log[0].clone(), log[1].clone())
        a.run(ods, codes)  # a second run(): fresh tensors, the first log untouched
        assert a.estimate_log[0].data_ptr() != log[0].data_ptr() and a.estimate_log[1].data_ptr() != log[1].data_ptr()
        assert torch.equal(log[0], first[0]) and torch.equal(log[1], first[1])
        a.step(ods[0], codes[0])  # step() afterwards writes the engine's own rows again
        assert a.estimate[0].data_ptr() == a.st.est_center.data_ptr() and a.estimate[1].data_ptr() == a.st.est_stds.data_ptr()
        assert bool(torch.isfinite(a.estimate[0]).all())
        assert int(a.status[0]) == 0
        a.close()
        b.close()
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world_one_nccl_run_and_step(dev):
    import torch.multiprocessing as mp
    mp.spawn(_nccl1_worker, args=(_free_port(),), nprocs=1, join=True)


# ---- two processes ---------------------------------------------------------------------------------------------------------
N_LOC2, FRAMES2, SEED2 = 8192, 6, 4000


def _two_worker(rank, world, port, exchange, out_dir, shared_gpu):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0 if shared_gpu else rank)
    torch.cuda.set_device(dev)
    if shared_gpu:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    from midastouch_amd.dist import ShardedFilterEngine
    cb, traj, start = _scene(2 * N_LOC2, T=FRAMES2 + 1)
    eng = ShardedFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N_LOC2, seed=SEED2, device=dev, exchange=exchange, estimate=True)
    eng.set_particles(torch.as_tensor(start[rank * N_LOC2:(rank + 1) * N_LOC2]))
    res = []
    for t in range(1, FRAMES2 + 1):
        eng.step(torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev))
        res.append({"center": eng.estimate[0].cpu(), "stds": eng.estimate[1].cpu(), "weights": eng.weights.cpu()})
    res[0]["exchange"] = eng.exchange
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    eng.close()
    dist.destroy_process_group()


def _two_processes(tmp_path, dev, exchange, shared_gpu):
    import torch.multiprocessing as mp
    from midastouch_amd.engine import FilterEngine
    mp.spawn(_two_worker, args=(2, _free_port(), exchange, str(tmp_path), shared_gpu), nprocs=2, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), f"r{r}.pt"), weights_only=False) for r in range(2)]
    assert all(p[0]["exchange"] == exchange for p in parts)
    cb, traj, start = _scene(2 * N_LOC2, T=FRAMES2 + 1)
    single = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, 2 * N_LOC2, seed=SEED2, device=dev, estimate=True)
    single.set_particles(torch.as_tensor(start))
    for t in range(1, FRAMES2 + 1):
        single.step(torch.as_tensor(traj.odoms[t]).to(dev), torch.as_tensor(traj.codes[t]).to(dev))
        c, s = single.estimate[0].cpu(), single.estimate[1].cpu()
        assert torch.equal(parts[0][t - 1]["center"], parts[1][t - 1]["center"]) and torch.equal(parts[0][t - 1]["stds"], parts[1][t - 1]["stds"]), t
        assert torch.equal(parts[0][t - 1]["center"], c) and torch.equal(parts[0][t - 1]["stds"], s), t
        assert torch.equal(torch.cat([p[t - 1]["weights"] for p in parts]), single.weights.cpu()), t


@pytest.mark.parametrize("exchange", ["peer_c", "peer", "a2a"])
def test_two_processes_sharing_one_gpu(tmp_path, dev, exchange):
    """gloo carries the exchanges ("peer_c": the split phases around the gloo gathers)."""
    _two_processes(tmp_path, dev, exchange, shared_gpu=True)


@pytest.mark.parametrize("exchange", ["peer_c", "peer", "a2a"])
def test_two_ranks_over_rccl(tmp_path, dev, exchange):
    """One GPU per process ("peer_c": midas_shard_step_estimate on the library's communicator).  Has never run: no machine with
    two GPUs has seen this suite."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _two_processes(tmp_path, dev, exchange, shared_gpu=False)
