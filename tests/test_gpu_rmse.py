"""The rotation half of the per-frame statistic (particle_rmse, modules/particle_filter.py:472-496) on the device: the stand-alone
operator and every place that adds the per-particle terms up, against the oracle at _recipes.RMSE_R_REL (2e-6 relative, no absolute
slack: kernel and oracle feed bit-identical (tr - 1) / 2 to acosf, DESIGN.md "The rmse's rotation column") and, for the operator,
against a float64 geodesic angle as well.

The per-particle terms come from one function (csrc/pose.hpp::rmse_terms); what differs between the forms is who adds them up:
  k_rmse_part / k_rmse_final   particles.hip:57,73     ops.rmse: a wave per 64 particles, then 256 threads striding the wave sums
                                                      (the strided loop runs a second time from 16 385 particles: particles.hip:77)
  frame_rmse                   tail.hip:241           the step tails (k_tail_a2d tail.hip:301, k_tail_a3 tail.hip:321, k_tail_b
                                                      tail.hip:571, k_tail_b2 tail.hip:850): the front's per-wave sums, strided by 256
  k_rmse_parts                 front_batch.hip:230    the presorted batch front's per-slot terms, re-summed per wave in slot order
  k_reduce_partials            front.hip:452          a shard's per-wave sums where the Python-side exchange finalises
  k_shard_fin / k_shard_route  shard_route.hip:77,328 the ranks' sums from the exchange records
  loop_weights_finalise        loop_weights.hpp:124   the loop engines' first workgroup, over the LIVE particles
Every test prints the largest relative deviation of the rotation column it saw.  Needs an MI355X."""
import functools

import numpy as np
import pytest

from _recipes import (RMSE_CLOUDS, RMSE_R_REL, RMSE_R_REL_F64, RMSE_T_REL_F64, assert_rmse, rmse_cloud, rmse_edge_terms,
                      rmse_mixed_cloud, rmse_ref64, rmse_rel_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from midastouch_amd import ops
    return ops


def _rmse(ops, dev, poses, gt):
    return ops.rmse(torch.as_tensor(poses).to(dev), torch.as_tensor(gt).to(dev)).cpu().numpy()


def _cls(v):
    return "nan" if np.isnan(v) else "inf" if np.isinf(v) else "zero" if v == 0 else "finite"


def _same_bits(a, b):
    """Two rmse tensors as bits, NaN equal to NaN."""
    a, b = (np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64) for x in (a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---- 1. the stand-alone operator ------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16383, 16385, 100003)


@functools.lru_cache(maxsize=None)
def _cloud_refs(kind):
    """The clouds of every size with the oracle's and the float64 reference's values, computed once."""
    from oracle import oracle as orc
    out = {}
    for n in SIZES:
        poses, gt = rmse_cloud(kind, n)
        out[n] = (poses, gt, orc.particle_rmse(poses, gt), rmse_ref64(poses, gt, angles=True))
    return out


@pytest.mark.parametrize("kind", RMSE_CLOUDS)
def test_rmse_op_clouds(dev, ops, oracle, kind):
    """ops.rmse on the band and noise clouds at sizes on either side of a wave (64), of the final's 256 threads and of its strided
    loop (16 384 = 256 waves): the oracle's value through assert_rmse, and the float64 geodesic angle.  From 255 particles on at the
    tolerances of tests/test_oracle_math.py::test_rmse_clouds_vs_float64 (every size stands around that test's gt: at 0.5 degrees the
    float32 formula's distance from the float64 angle is mostly a term common to a gt's particles, see there).  Below, the
    roundings of a few terms do not average out and a single small angle can carry the statistic, so the bound is the worst
    case of one term: dx = 5.4e-7 on the acos argument (six roundings of 2^-24 on a trace of magnitude <= 3), d(theta) <= dx /
    sin(theta_min) with theta_min the smallest float64 angle of the cloud; an RMS of terms each off by at most that is off by at
    most that."""
    worst, worst64 = 0.0, 0.0
    for n, (poses, gt, ref, f64) in _cloud_refs(kind).items():
        out = _rmse(ops, dev, poses, gt)
        worst = max(worst, assert_rmse(out, ref, f"{kind} N={n}"))
        worst64 = max(worst64, rmse_rel_dev(out[1], f64[1]))
        if n >= 255:
            assert out[1] == pytest.approx(f64[1], rel=RMSE_R_REL_F64[kind], abs=0), (kind, n)
        else:
            assert abs(out[1] - f64[1]) <= np.degrees(5.4e-7 / np.sin(np.radians(f64[2].min()))), (kind, n)
        # rmse_t: 1e-8 where a few thousand terms average their float32 roundings out (the bound of the N = 2000 clouds); for fewer,
        # the worst case of one term: two rounded differences and the three roundings of the fma chain, 5 * 2^-24 on e^2, half on e
        assert out[0] == pytest.approx(f64[0], rel=RMSE_T_REL_F64 if n >= 2000 else 2.5 * 2.0 ** -24, abs=0), (kind, n)
    print(f"rmse_r, ops.rmse {kind}: max rel dev vs oracle {worst:.3g}, vs float64 {worst64:.3g}")


def test_rmse_op_edge_terms(dev, ops, oracle):
    """Every edge term as an N = 1 call (rmse_r = |angle| exactly: the square of a float32 and its root are exact in float64): the
    oracle's class (NaN / Inf / zero / finite) in both columns, finite values within RMSE_R_REL - and the deviation in ulp of the
    float32 angle, the evidence behind that constant: device acosf (4 ulp by the OpenCL bound) and glibc's (1 ulp), one product."""
    terms = rmse_edge_terms()
    worst_rel, worst_ulp, at = 0.0, 0.0, ""
    for name, P, G in terms:
        ref = oracle.particle_rmse(P[None], G)
        out = _rmse(ops, dev, P[None], G)
        assert (_cls(out[0]), _cls(out[1])) == (_cls(ref[0]), _cls(ref[1])), (name, out, ref)
        worst_rel = max(worst_rel, assert_rmse(out, ref, name))
        if _cls(ref[1]) == "finite":
            ulp = abs(out[1] - ref[1]) / float(np.spacing(np.float32(ref[1])))
            if ulp > worst_ulp:
                worst_ulp, at = ulp, f"{name} ({ref[1]:.9g} deg)"
    print(f"rmse_r, ops.rmse, {len(terms)} single terms: max rel dev {worst_rel:.3g}, max {worst_ulp:.3g} ulp of the float32 angle at {at}")


def test_rmse_op_single_term_sweep(dev, ops, oracle):
    """The N = 1 sweep over the angle: 400 single terms from 0.01 to 179.99 degrees (log-spaced towards both ends, where acos is
    steepest), each within RMSE_R_REL of the oracle; prints the largest deviation in ulp of the float32 angle."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(11)
    small = np.geomspace(0.01, 90.0, 200)
    angles = np.concatenate([small, 180.0 - small])
    gt = rmse_cloud("band5", 1, 3)[1]
    worst_rel = worst_ulp = 0.0
    for a in angles:
        ax = rng.standard_normal(3)
        P = gt.copy()
        P[:3, :3] = gt[:3, :3].astype(np.float64) @ Rotation.from_rotvec(ax / np.linalg.norm(ax) * np.deg2rad(a)).as_matrix()
        ref = oracle.particle_rmse(P[None], gt)
        out = _rmse(ops, dev, P[None], gt)
        worst_rel = max(worst_rel, assert_rmse(out, ref, f"{a:.6g} deg"))
        if ref[1] != 0 and np.isfinite(ref[1]):
            worst_ulp = max(worst_ulp, abs(out[1] - ref[1]) / float(np.spacing(np.float32(ref[1]))))
    print(f"rmse_r, ops.rmse, sweep of {len(angles)} single terms: max rel dev {worst_rel:.3g}, max {worst_ulp:.3g} ulp of the float32 angle")


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("nan_translation_last", [False, True])
def test_rmse_op_mixed_waves(dev, ops, oracle, n, nan_translation_last):
    """Edge terms at lane 0, lane 63, the first lane of the last (partial) wave and the very last particle among ordinary 0.5 degree
    terms: NaN-to-0 next to finite ones, a 180 degree term, an exact zero.  With a NaN translation in the last particle only, column
    0 is NaN and column 1 is what it was."""
    poses, gt = rmse_mixed_cloud(n, nan_translation_last=nan_translation_last)
    ref = oracle.particle_rmse(poses, gt)
    out = _rmse(ops, dev, poses, gt)
    assert np.isnan(ref[0]) == nan_translation_last and ref[1] > 1.0
    dev_r = assert_rmse(out, ref, f"N={n}")
    plain = oracle.particle_rmse(*rmse_mixed_cloud(n))
    assert ref[1] == plain[1]
    # the terms one at a time, as the wave sees them: every particle alone has the oracle's class
    for i in sorted({0, 1, 62, 63, 64, (n - 1) // 64 * 64, n - 1}):
        o1, r1 = _rmse(ops, dev, poses[i:i + 1], gt), oracle.particle_rmse(poses[i:i + 1], gt)
        assert (_cls(o1[0]), _cls(o1[1])) == (_cls(r1[0]), _cls(r1[1])), (i, o1, r1)
    print(f"rmse_r, ops.rmse mixed waves N={n} nan_t={nan_translation_last}: rel dev {dev_r:.3g}")


# ---- 2. every finaliser, through the engines, with adversarial ground truth -------------------------------------------------------
K, D, FRAMES = 4000, 256, 8
KINDS = ("trajectory", "a particle's pose", "that pose turned by pi", "that pose, rows scaled 1 + 2^-20", "identity at the origin",
         "NaN rotation entry", "NaN translation entry", "trajectory again")


@functools.lru_cache(maxsize=None)
def _codebook():
    from midastouch_amd.synthetic import make_codebook
    return make_codebook(K=K, D=D, seed=1000)


@functools.lru_cache(maxsize=None)
def _world(traj_seed=2000):
    from midastouch_amd.synthetic import make_trajectory
    return _codebook(), make_trajectory(_codebook(), T=FRAMES + 2, seed=traj_seed)


def _near_start(oracle, cb, traj, N, seed, ratio=0.05):
    """init_filter's cloud around the first ground-truth pose (particle_filter.py:129-145), projected onto the codebook."""
    from midastouch_amd.synthetic import mesh_scale
    g = torch.Generator().manual_seed(seed)
    tn = torch.normal(0.0, mesh_scale(cb.extents) / 3.0 * ratio, size=(N, 3), generator=g).numpy()
    rot = torch.normal(0.0, 60.0 * ratio, size=(N, 3), generator=g).numpy()
    poses = oracle.init_filter_compose(traj.gt_poses[0], tn, rot)
    return cb.poses[oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices).SE3_NN_idx(poses)]


def _mid_wave(n):
    return min(n - 1, (n // 2) // 64 * 64 + 37)


def _adversarial_gt(kind, traj_gt, prop):
    """The ground truth of a frame, from the frame's own propagated particles (the rmse needs only gt to be adversarial, and gt is a
    free input of the frame).  j: a particle in the middle of a wave."""
    P = prop[_mid_wave(len(prop))].copy()
    G = np.array(traj_gt, dtype=np.float32, copy=True)
    if kind == 1:
        G = P
    elif kind == 2:
        G = P
        G[:3, 1:3] = -G[:3, 1:3]  # a turn by exactly pi about the pose's own x axis: two columns negated, no rounding
    elif kind == 3:
        G = P
        G[:3, :3] *= np.float32(1.0 + 2.0 ** -20)
    elif kind == 4:
        G = np.eye(4, dtype=np.float32)
    elif kind == 5:
        G[1, 2] = np.nan
    elif kind == 6:
        G[0, 3] = np.nan
    return np.ascontiguousarray(G)


def _check_kind(oracle, kind, prop, gt, want):
    """The oracle's value has the shape the kind is there for."""
    rt, rr = want
    if kind == 1:
        assert np.isfinite(rt) and np.isfinite(rr)
        j = _mid_wave(len(prop))
        assert oracle.particle_rmse(prop[j:j + 1], gt)[0] == 0.0  # the identical-pose term
    elif kind == 2:
        assert rr > 170.0
    elif kind == 3:
        j = _mid_wave(len(prop))
        one = np.array([oracle.particle_rmse(prop[i:i + 1], gt)[1] for i in range(max(0, j - 128), min(len(prop), j + 128))])
        assert (one == 0).any()  # NaN-to-0 terms ...
        assert len(prop) < 64 or (one > 0).any()  # ... beside finite ones
    elif kind == 4:
        assert rr > 5.0
    elif kind == 5:
        assert rr == 0.0 and np.isfinite(rt)
    elif kind == 6:
        assert np.isnan(rt) and rr > 0.0
    else:
        assert np.isfinite(rt) and 0.0 < rr < 90.0


def _frame_gt(oracle, t, traj_gt, prop, shift=0):
    """Frame t (1-based) takes kind (t - 1 + shift) % 8; frame FRAMES + 1 has no ground truth.  -> (gt or None, oracle's rmse)."""
    if t > FRAMES:
        return None, None
    kind = (t - 1 + shift) % len(KINDS)
    gt = _adversarial_gt(kind, traj_gt, prop)
    want = oracle.particle_rmse(prop, gt)
    _check_kind(oracle, kind, prop, gt, want)
    return gt, want


def _dev(a, dev):
    return None if a is None else torch.as_tensor(a).to(dev)


@pytest.mark.parametrize("mode", ["weighted_random", "low_var"])
@pytest.mark.parametrize("N", [100, 4097])
def test_filter_engine_rmse(dev, oracle, N, mode):
    """FilterEngine (midas_filter_step: the front's per-wave sums, frame_rmse in the step tail's first workgroup - tail.hip:571,
    :850), host draws in the reference's order as tests/test_gpu_step.py::test_step_parity_host_draws.  N = 100: two waves, the
    second partial; 4097: a block and a slot, 65 waves.  Then a frame without ground truth: rmse as it was, the frame the oracle's."""
    from midastouch_amd.engine import FilterEngine
    cb, traj = _world()
    ofl = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    eng = FilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, resample=mode, device=dev)
    poses = _near_start(oracle, cb, traj, N, 5)
    eng.set_particles(torch.as_tensor(poses))
    worst = 0.0
    for t in range(1, FRAMES + 2):
        torch.manual_seed(3000 + t)
        tn = torch.normal(mean=0.0, std=2e-4, size=(N, 3))
        rot = torch.normal(mean=0.0, std=0.5, size=(N, 3))
        u, u32 = (torch.rand(N, dtype=torch.float64), -1.0) if mode == "weighted_random" else (None, float(torch.rand(1).item()))
        ref = ofl.step(poses, traj.odoms[t], traj.codes[t], tn.numpy(), rot.numpy(), u=None if u is None else u.numpy(), mode=mode, u32=u32)
        gt, want = _frame_gt(oracle, t, traj.gt_poses[t], ref["poses_prop"])
        before = eng.rmse.clone()
        eng.step(_dev(traj.odoms[t], dev), _dev(traj.codes[t], dev), gt=_dev(gt, dev), tn=tn.to(dev), rot=rot.to(dev),
                 u=None if u is None else u.to(dev), u32=u32)
        for name in ("poses_prop", "nn_idx", "weights", "ridx", "poses"):
            assert np.array_equal(getattr(eng, name).cpu().numpy(), ref[name]), f"frame {t}: {name}"
        if gt is None:
            assert _same_bits(eng.rmse, before), "a frame without ground truth leaves rmse as it was"
        else:
            worst = max(worst, assert_rmse(eng.rmse, want, f"frame {t} ({KINDS[(t - 1) % 8]})"))
        poses = ref["poses"]
    print(f"rmse_r vs oracle, FilterEngine {mode} N={N}, adversarial gt: max rel dev {worst:.3g}")


@pytest.mark.parametrize("grouped", ["1", "0"])
@pytest.mark.parametrize("N", [16, 512, 513, 4097])
def test_pipelined_engine_rmse(dev, oracle, monkeypatch, N, grouped):
    """PipelinedFilterEngine, device draws: frame_rmse under the grouped tail k_tail_a3 (tail.hip:321) and under k_tail_a2d
    (tail.hip:301).  launch_tail_a2 (tail.hip:369) takes the grouped form for every N >= 16 whose grid is resident
    (tail_grouped_ok, tail.hip:346) unless MIDAS_TAIL_GROUPED=0, so both forms are run at every size: N = 16, the smallest the
    direct tail takes (SCAN_CHUNK); 512 and 513, the two-kernel front's boundary (launch_frame_front); 4097, a block and a slot.
    step() frame by frame against the oracle, then the same frames by one run() on a second engine: its log rows are the
    per-frame values as bits.  Then a frame without ground truth."""
    from midastouch_amd.engine import PipelinedFilterEngine
    monkeypatch.setenv("MIDAS_TAIL_GROUPED", grouped)
    cb, traj = _world()
    seed = 4400
    ofl = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    engs = [PipelinedFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N, seed=seed, device=dev) for _ in range(2)]
    poses = _near_start(oracle, cb, traj, N, 6)
    for e in engs:
        e.set_particles(torch.as_tensor(poses))
    eng, twin = engs
    worst, gts, seen = 0.0, [], []
    for t in range(1, FRAMES + 2):
        tn, rot = oracle.philox_noise(N, seed, t - 1, np.float32(2e-4), np.float32(0.5))
        ref = ofl.step(poses, traj.odoms[t], traj.codes[t], tn, rot, u=oracle.philox_uniform64(N, seed, t - 1))
        gt, want = _frame_gt(oracle, t, traj.gt_poses[t], ref["poses_prop"])
        before = eng.rmse.clone()
        eng.step(_dev(traj.odoms[t], dev), _dev(traj.codes[t], dev), gt=_dev(gt, dev))
        assert np.array_equal(eng.poses_prop.cpu().numpy(), ref["poses_prop"]), f"frame {t}: propagated poses"
        assert np.array_equal(eng.nn_idx.cpu().numpy(), ref["nn_idx"]), f"frame {t}: NN index"
        if gt is None:
            assert _same_bits(eng.rmse, before), "a frame without ground truth leaves rmse as it was"
            assert not eng._flushed
            for name in ("ridx", "poses", "weights"):
                assert np.array_equal(getattr(eng, name).cpu().numpy(), ref[name]), f"frame {t}: {name}"
            assert _same_bits(eng.rmse, before)
        else:
            worst = max(worst, assert_rmse(eng.rmse, want, f"frame {t} ({KINDS[(t - 1) % 8]})"))
            gts.append(gt)
            seen.append(eng.rmse.cpu().numpy().copy())
        poses = ref["poses"]
    log = twin.run(_dev(traj.odoms[1:FRAMES + 1], dev), _dev(traj.codes[1:FRAMES + 1], dev), _dev(np.stack(gts), dev))
    assert _same_bits(log[:, :2], np.stack(seen)), "run()'s log rows are the per-frame values"
    assert _same_bits(twin.rmse, seen[-1])
    print(f"rmse_r vs oracle, PipelinedFilterEngine N={N} grouped tail={grouped}, adversarial gt: max rel dev {worst:.3g}")


@pytest.mark.parametrize("N", [2000, 11000])
def test_batch_engines_rmse(dev, oracle, N):
    """BatchFilterEngine against the oracle per trajectory, PipelinedBatchFilterEngine against it as bits (the style of
    tests/test_gpu_step.py::test_pipelined_batch_engine_equals_batch_engine).  B = 3, trajectory b starts its list of ground
    truths b places on, so a row offset in part_rmse or in the rmse triple shows.  The pipelined batch step runs presorted and forms
    the per-wave sums by k_rmse_parts (front_batch.hip:230): N = 2000 through the one-kernel form with its tables in LDS, N = 11 000
    (beyond its 10 240 slots) through the two-kernel form.  Then a frame without ground truth."""
    from midastouch_amd.engine import BatchFilterEngine, PipelinedBatchFilterEngine
    B, seed = 3, 4000
    cb = _world()[0]
    trajs = [_world(2100 + b)[1] for b in range(B)]
    ofl = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    a, p = (cls(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, sig_t=1e-4, sig_r=0.5, seed=seed, device=dev)
            for cls in (BatchFilterEngine, PipelinedBatchFilterEngine))
    poses = np.stack([_near_start(oracle, cb, trajs[b], N, 20 + b) for b in range(B)])
    for e in (a, p):
        e.set_particles(torch.as_tensor(poses))
    worst = 0.0
    for t in range(1, FRAMES + 2):
        tn_all, rot_all = oracle.philox_noise(B * N, seed, t - 1, np.float32(1e-4), np.float32(0.5))
        u_all = oracle.philox_uniform64(B * N, seed, t - 1)
        refs, gts, wants = [], [], []
        for b in range(B):
            sl = slice(b * N, (b + 1) * N)
            refs.append(ofl.step(poses[b], trajs[b].odoms[t], trajs[b].codes[t], tn_all[sl], rot_all[sl], u=u_all[sl]))
            gt, want = _frame_gt(oracle, t, trajs[b].gt_poses[t], refs[b]["poses_prop"], shift=b)
            gts.append(gt)
            wants.append(want)
        odoms = _dev(np.stack([tr.odoms[t] for tr in trajs]), dev)
        codes = _dev(np.stack([tr.codes[t] for tr in trajs]), dev)
        g = None if gts[0] is None else _dev(np.stack(gts), dev)
        before = (a.rmse.clone(), p.rmse.clone())
        for e in (a, p):
            e.step(odoms, codes, g)
        assert a.sparse_scores
        assert torch.equal(a.poses_prop, p.poses_prop) and torch.equal(a.nn_idx, p.nn_idx), f"frame {t}"
        assert _same_bits(a.rmse, p.rmse), f"frame {t}: rmse, pipelined batch against batch"
        for b in range(B):
            for name in ("poses_prop", "nn_idx", "ridx", "poses"):
                assert np.array_equal(getattr(a, name)[b].cpu().numpy(), refs[b][name]), f"frame {t} b {b}: {name}"
            if g is not None:
                worst = max(worst, assert_rmse(a.rmse[b], wants[b], f"frame {t} b {b} ({KINDS[(t - 1 + b) % 8]})"))
            poses[b] = refs[b]["poses"]
        if g is None:
            assert _same_bits(a.rmse, before[0]) and _same_bits(p.rmse, before[1]), "a frame without ground truth leaves rmse as it was"
            assert torch.equal(a.ridx, p.ridx) and torch.equal(a.poses, p.poses)
    print(f"rmse_r vs oracle, BatchFilterEngine / PipelinedBatchFilterEngine B={B} N={N}, adversarial gt: max rel dev {worst:.3g}")


class FakeComm:
    def __init__(self, r, w):
        self.rank, self.world = r, w

    def all_gather(self, t):
        raise AssertionError("lock-step test never calls the communicator")

    all_to_all = all_gather


@pytest.mark.parametrize("exchange", ["a2a", "peer_c"])
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_engine_rmse(dev, oracle, shards, exchange):
    """ShardedFilterEngine on one GPU in lock-step (HipShardBackend, as tests/test_gpu_dist.py): every rank's rmse against the
    oracle of ALL particles.  n_loc = 4096.  "a2a": the Python-side frame - k_reduce_partials (front.hip:452) per shard, the ranks'
    sums added by k_shard_fin's block 0 (shard_route.hip:77); "peer_c": the C-side frame - the shard tail's frame_rmse leaves raw
    sums in the exchange record (tail.hip:410-414), k_shard_route adds the ranks' (shard_route.hip:328)."""
    from midastouch_amd.dist import HipShardBackend, ShardedFilterEngine, connect_local_peers, run_lockstep
    n_loc, seed = 4096, 4000
    N = shards * n_loc
    cb, traj = _world()
    ofl = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    poses = _near_start(oracle, cb, traj, N, 7)
    be = HipShardBackend(cb.poses, cb.embeddings, cb.mesh_vertices, dev)
    engs = [ShardedFilterEngine(num_particles=n_loc, backend=be, comm=FakeComm(r, shards), exchange=exchange) for r in range(shards)]
    if exchange == "peer_c":
        connect_local_peers(engs, exchange)
    for r, e in enumerate(engs):
        e.set_particles(torch.as_tensor(poses[r * n_loc:(r + 1) * n_loc]))
    cat = lambda name: torch.cat([getattr(e, name) for e in engs]).cpu().numpy()
    worst = 0.0
    for t in range(1, FRAMES + 2):
        tn, rot = oracle.philox_noise(N, seed, t - 1, np.float32(2e-4), np.float32(0.5))
        ref = ofl.step(poses, traj.odoms[t], traj.codes[t], tn, rot, u=oracle.philox_uniform64(N, seed, t - 1))
        gt, want = _frame_gt(oracle, t, traj.gt_poses[t], ref["poses_prop"])
        od, code = _dev(traj.odoms[t], dev), _dev(traj.codes[t], dev)
        before = [e.rmse.clone() for e in engs]
        run_lockstep(engs, [((od, code), {} if gt is None else {"gt": _dev(gt, dev)}) for _ in engs])
        for name in ("poses_prop", "nn_idx", "weights", "ridx", "poses"):
            assert np.array_equal(cat(name), ref[name]), f"frame {t}: {name}"
        for r, e in enumerate(engs):
            if gt is None:
                assert _same_bits(e.rmse, before[r]), "a frame without ground truth leaves rmse as it was"
            else:
                worst = max(worst, assert_rmse(e.rmse, want, f"frame {t} rank {r} ({KINDS[(t - 1) % 8]})"))
                assert _same_bits(e.rmse, engs[0].rmse), f"frame {t}: rank {r} against rank 0"
        poses = ref["poses"]
    print(f"rmse_r vs oracle, ShardedFilterEngine {shards} x {n_loc} {exchange}, adversarial gt: max rel dev {worst:.3g}")


def test_loop_engines_rmse(dev, oracle):
    """LoopEngine against the oracle's loop body, BatchLoopEngine (B = 3) against the LoopEngines as bits (the style of
    tests/test_gpu_batch_loop.py): loop_weights_finalise (loop_weights.hpp:124), the statistic over the LIVE particles.  Capacity
    3000 (47 waves, all in the first workgroup's first pass: the strided second pass of loop_weights.hpp:132 starts at 16 385 live
    particles, which tests/test_gpu_batch_loop_regime.py's 16 384-particle scenarios stop short of and an 8-frame test cannot
    reach cheaply) with DBSCAN every 5th frame and annealing on, from init_filter's wide start: the live count falls below the
    capacity and is no multiple of 64.  Row b follows its own trajectory and starts the list of ground truths b places on.  Then a
    frame without ground truth: the log's rmse fields repeat the previous frame's (ctl_d is not written)."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    from test_gpu_loop import _compare_frame
    B, N0, seed = 3, 3000, 4100
    cb = _world()[0]
    trajs = [_world(2013 + b)[1] for b in range(B)]
    kw = dict(cluster=True, cluster_every=5, device=dev)
    singles = [LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0, seed=seed + b, **kw) for b in range(B)]
    batch = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, seed=seed, **kw)
    loops = [oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, cluster=True, cluster_every=5) for _ in range(B)]
    poses = [_near_start(oracle, cb, trajs[b], N0, 11 + b, ratio=0.15) for b in range(B)]
    labels = [np.zeros(N0, dtype=np.int64) for _ in range(B)]
    for s, q in zip(singles, poses):
        s.set_particles(torch.as_tensor(q))
    batch.set_particles([torch.as_tensor(q) for q in poses])
    worst, live, prev = 0.0, [], [None] * B
    for t in range(FRAMES + 1):
        refs, gts, wants = [], [], []
        for b in range(B):
            n = poses[b].shape[0]
            tn, rot = oracle.philox_noise(n, seed + b, t, np.float32(2e-4), np.float32(0.5))
            refs.append(loops[b].step(poses[b], labels[b], trajs[b].odoms[t + 1], trajs[b].codes[t + 1], tn, rot, gt=None,
                                      mode="weighted_random", u32=None, draws=lambda n2, b=b: oracle.philox_uniform64(n2, seed + b, t)))
            gt, want = _frame_gt(oracle, t + 1, trajs[b].gt_poses[t + 1], refs[b]["poses_prop"], shift=b)
            gts.append(gt)
            wants.append(want)
            live.append(n)
        odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
        codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
        g = None if gts[0] is None else torch.as_tensor(np.stack(gts))
        for b in range(B):
            singles[b].step(odoms[b], codes[b], gt=None if g is None else g[b])
        batch.step(odoms, codes, gts=g)
        for b in range(B):
            fs, fb = singles[b].frame_view(), batch.frame_view(b)
            _compare_frame(fs, refs[b], t, t % 5 == 0)
            assert fb["n"] == fs["n"] and torch.equal(fb["poses_prop"], fs["poses_prop"]) and torch.equal(fb["poses"], fs["poses"])
            got = (fs["rmse_t"], fs["rmse_r"])
            assert _same_bits(np.array([fb["rmse_t"], fb["rmse_r"]]), np.array(got)), f"frame {t} row {b}: batch against single"
            if g is None:
                assert _same_bits(np.array(got), np.array(prev[b])), "a frame without ground truth repeats the previous frame's rmse"
            else:
                worst = max(worst, assert_rmse(np.array(got), wants[b], f"frame {t} row {b} ({KINDS[(t + b) % 8]})"))
            prev[b] = got
            poses[b], labels[b] = refs[b]["poses"], refs[b]["labels"]
    assert min(live) < N0 and any(n % 64 for n in live), live
    print(f"rmse_r vs oracle, LoopEngine / BatchLoopEngine B={B} from {N0}, live counts {min(live)} .. {max(live)}, adversarial gt: "
          f"max rel dev {worst:.3g}")
