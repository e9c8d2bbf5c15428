"""`ShardedFilterEngine(estimate=True)` without a GPU: the sharding logic of the per-frame pose estimate (one more exchange of
per-block moment partials, added in rank order on every rank) under torch.distributed gloo and in lock-step, on the
oracle-backed backend of tests/_oracle_shard_estimate.py; the new C entries' surface."""
import ctypes
import inspect
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LOC, K, D, FRAMES = 4096, 1500, 64, 4  # (the sizes of tests/test_dist_cpu.py)


def _data(shards):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook(K=K, D=D, seed=1000)
    traj = make_trajectory(cb, T=FRAMES + 1, seed=2000)
    start = cb.poses[np.random.default_rng(0).integers(0, K, shards * N_LOC)]
    return cb, traj, start


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, exchange, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from midastouch_amd.dist import ShardedFilterEngine
    from tests._oracle_shard_estimate import OracleEstimateBackend
    cb, traj, start = _data(world)
    eng = ShardedFilterEngine(num_particles=N_LOC, backend=OracleEstimateBackend(cb.poses, cb.embeddings, cb.mesh_vertices),
                              seed=4000, exchange=exchange, estimate=True)
    eng.set_particles(torch.as_tensor(start[rank * N_LOC:(rank + 1) * N_LOC]))
    res = []
    for t in range(1, FRAMES + 1):
        eng.step(torch.as_tensor(traj.odoms[t]), torch.as_tensor(traj.codes[t]))
        c, s = eng.estimate
        res.append({"center": c.numpy().copy(), "stds": s.numpy().copy(), "ridx": eng.ridx.numpy().copy(),
                    "weights": eng.weights.numpy().copy()})
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _one_shard_and_oracle(oracle, shards):
    """Per frame: the estimate of the same backend run as ONE shard of all particles, and the oracle's cluster_centers of the
    oracle filter's own frame; plus the oracle frame (ridx, weights)."""
    from midastouch_amd.dist import ShardedFilterEngine, SingleComm
    from tests._oracle_shard_estimate import OracleEstimateBackend
    cb, traj, start = _data(shards)
    N = shards * N_LOC
    one = ShardedFilterEngine(num_particles=N, backend=OracleEstimateBackend(cb.poses, cb.embeddings, cb.mesh_vertices),
                              comm=SingleComm(), seed=4000, estimate=True)
    one.set_particles(torch.as_tensor(start))
    ofl = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    poses, out = start, []
    for t in range(1, FRAMES + 1):
        one.step(torch.as_tensor(traj.odoms[t]), torch.as_tensor(traj.codes[t]))
        tn, rot = oracle.philox_noise(N, 4000, t - 1, np.float32(2e-4), np.float32(0.5))
        ref = ofl.step(poses, traj.odoms[t], traj.codes[t], tn, rot, u=oracle.philox_uniform64(N, 4000, t - 1))
        _, oc, os_ = oracle.cluster_centers(ref["poses_prop"], ref["weights"], np.zeros(N, dtype=np.int64))
        out.append({"center": one.estimate[0].numpy().copy(), "stds": one.estimate[1].numpy().copy(), "oc": oc[0], "os": os_[0],
                    "ridx": ref["ridx"], "weights": ref["weights"]})
        poses = ref["poses"]
    return out


def _check(per_shard, ref, t):
    """per_shard: every shard's (centre, spreads) of one frame."""
    c0, s0 = per_shard[0]
    for c, s in per_shard[1:]:
        assert np.array_equal(c, c0) and np.array_equal(s, s0), f"frame {t}: the shards disagree"
    assert np.array_equal(c0, ref["center"]) and np.array_equal(s0, ref["stds"]), f"frame {t}: not the one-shard bits"
    # the tolerances of tests/test_gpu_estimate.py against the oracle
    assert np.abs(c0 - ref["oc"]).max() < 2e-6, (t, np.abs(c0 - ref["oc"]).max())
    np.testing.assert_allclose(s0, ref["os"], rtol=2e-4, atol=1e-9)
    assert np.isfinite(c0).all() and c0[3].tolist() == [0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("exchange", ["a2a", "allgather", "a2a_fixed"])
def test_two_rank_gloo_estimate(tmp_path, oracle, exchange):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), exchange, str(tmp_path)), nprocs=world, join=True)
    parts = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=False) for r in range(world)]
    refs = _one_shard_and_oracle(oracle, world)
    for t in range(FRAMES):
        _check([(p[t]["center"], p[t]["stds"]) for p in parts], refs[t], t + 1)
        # the frame itself is the one the existing tests pin
        assert np.array_equal(np.concatenate([p[t]["ridx"] for p in parts]), refs[t]["ridx"])
        assert np.array_equal(np.concatenate([p[t]["weights"] for p in parts]), refs[t]["weights"])


class FakeComm:
    def __init__(self, r, w):
        self.rank, self.world = r, w


def test_lockstep_three_shards_estimate_and_twin_without(oracle):
    """Three shards of one process, no collective library: same assertions; a twin set built WITHOUT the keyword computes the
    same frame, allocates no estimate and refuses `estimate`."""
    from midastouch_amd._lib import MidasError
    from midastouch_amd.dist import ShardedFilterEngine, run_lockstep
    from tests._oracle_shard_estimate import OracleEstimateBackend
    shards = 3
    cb, traj, start = _data(shards)
    be = OracleEstimateBackend(cb.poses, cb.embeddings, cb.mesh_vertices)
    engs = [ShardedFilterEngine(num_particles=N_LOC, backend=be, comm=FakeComm(r, shards), estimate=True) for r in range(shards)]
    twins = [ShardedFilterEngine(num_particles=N_LOC, backend=be, comm=FakeComm(r, shards)) for r in range(shards)]
    for r in range(shards):
        for e in (engs[r], twins[r]):
            e.set_particles(torch.as_tensor(start[r * N_LOC:(r + 1) * N_LOC]))
    refs = _one_shard_and_oracle(oracle, shards)
    for t in range(1, FRAMES + 1):
        args = [((torch.as_tensor(traj.odoms[t]), torch.as_tensor(traj.codes[t])), {}) for _ in engs]
        run_lockstep(engs, args)
        run_lockstep(twins, args)
        _check([(e.estimate[0].numpy(), e.estimate[1].numpy()) for e in engs], refs[t - 1], t)
        for name in ("ridx", "weights", "poses", "weights_res", "hint", "nn_idx"):
            assert torch.equal(torch.cat([getattr(e, name) for e in engs]), torch.cat([getattr(e, name) for e in twins])), (t, name)
        assert np.array_equal(np.concatenate([e.ridx.numpy() for e in twins]), refs[t - 1]["ridx"])
        assert np.array_equal(np.concatenate([e.weights.numpy() for e in twins]), refs[t - 1]["weights"])
    for e in twins:
        assert not hasattr(e.st, "est_part") and not hasattr(e.st, "est_center")
        with pytest.raises(MidasError, match="estimate=True"):
            e.estimate


def test_estimate_leaves_a_pending_overflow_check_alone():
    """exchange="a2a_fixed" leaves a pending overflow check behind every frame; reading the particle set looks at it (and may
    wait), reading `estimate` must not: the check is still pending afterwards, and the particle views then consume it."""
    from midastouch_amd.dist import ShardedFilterEngine, run_lockstep
    from tests._oracle_shard_estimate import OracleEstimateBackend
    shards = 2
    cb, traj, start = _data(shards)
    be = OracleEstimateBackend(cb.poses, cb.embeddings, cb.mesh_vertices)
    engs = [ShardedFilterEngine(num_particles=N_LOC, backend=be, comm=FakeComm(r, shards), exchange="a2a_fixed", estimate=True)
            for r in range(shards)]
    for r, e in enumerate(engs):
        e.set_particles(torch.as_tensor(start[r * N_LOC:(r + 1) * N_LOC]))
    run_lockstep(engs, [((torch.as_tensor(traj.odoms[1]), torch.as_tensor(traj.codes[1])), {}) for _ in engs])
    for e in engs:
        pending = list(e._ovf_pending)
        assert sum(p is not None for p in pending) == 1
        c, s = e.estimate
        assert c.shape == (4, 4) and s.shape == (3,)
        assert e._ovf_pending == pending and all(a is b for a, b in zip(e._ovf_pending, pending))
        e.ridx  # a particle view looks at the check
        assert all(p is None for p in e._ovf_pending)


def test_shard_estimate_entries_declared_exported_bound():
    from midastouch_amd import _lib, dist
    lib = ctypes.CDLL(_lib.build())
    text = open(os.path.join(REPO, "include", "midas_hip.h")).read()
    names = ("midas_shard_estimate_moments", "midas_shard_estimate_finish", "midas_shard_step_estimate", "midas_shard_run_estimate")
    for name in names:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), f"{name} not exported"
        assert re.search(r"int\s+%s\s*\(\s*midas_ctx\s*\*\s*ctx" % name, text), name
        # every entry cites the reference's call site in the header
        assert re.search(r"%s\s+\(filter/filter\.py:184-186\)" % name, text), name
    # the one-call forms: midas_shard_step's / midas_shard_run's arguments (the phases of a step are fixed) + the four pointers;
    # midas_shard_step_args itself is unchanged
    step, run = _lib.SIGNATURES["midas_shard_step"][1], _lib.SIGNATURES["midas_shard_run"][1]
    assert _lib.SIGNATURES["midas_shard_step_estimate"][1] == step[:-1] + [ctypes.c_void_p] * 4
    assert _lib.SIGNATURES["midas_shard_run_estimate"][1] == run + [ctypes.c_void_p] * 4
    p = inspect.signature(dist.ShardedFilterEngine.__init__).parameters["estimate"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert isinstance(inspect.getattr_static(dist.ShardedFilterEngine, "estimate"), property)
    for m in ("estimate_moments", "estimate_finish"):
        assert callable(getattr(dist.HipShardBackend, m))
    assert dist.EST_MOM * 8 == 288


def test_softmax_off_estimate_compared_before_the_resample():
    """softmax=False: raw scores of mixed sign, a CDF that is not monotone - the owner-side search of two shards and the search of
    one shard may pick different sources (the reference's p = w / sum(w) is undefined there), so the FRAMES part after the first
    resample.  The estimate is taken before the resample: on the same propagated poses and weights it is the one shard's, bit for
    bit, every frame; both sides go on from the one shard's resampled set."""
    from midastouch_amd.dist import ShardedFilterEngine, SingleComm, run_lockstep
    from tests._oracle_shard_estimate import OracleEstimateBackend
    shards = 2
    cb, traj, start = _data(shards)
    be = OracleEstimateBackend(cb.poses, cb.embeddings, cb.mesh_vertices)
    one = ShardedFilterEngine(num_particles=shards * N_LOC, backend=be, comm=SingleComm(), softmax=False, exchange="a2a", estimate=True)
    engs = [ShardedFilterEngine(num_particles=N_LOC, backend=be, comm=FakeComm(r, shards), softmax=False, exchange="a2a", estimate=True)
            for r in range(shards)]
    nxt = torch.as_tensor(start)
    for t in range(1, FRAMES + 1):
        one.set_particles(nxt)
        for r, e in enumerate(engs):
            e.set_particles(nxt[r * N_LOC:(r + 1) * N_LOC])
        args = (torch.as_tensor(traj.odoms[t]), torch.as_tensor(traj.codes[t]))
        one.step(*args)
        run_lockstep(engs, [(args, {}) for _ in engs])
        w = one.weights
        assert bool((w < 0).any()) and bool((w > 0).any())  # (the case this test is for)
        assert torch.equal(torch.cat([e.poses_prop for e in engs]), one.poses_prop) and torch.equal(torch.cat([e.weights for e in engs]), w)
        for e in engs:
            assert torch.equal(e.estimate[0], one.estimate[0]) and torch.equal(e.estimate[1], one.estimate[1]), t
        nxt = one.poses.clone()
