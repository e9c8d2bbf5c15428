"""The finishers that share cluster_rot.hpp's closed forms with `ops.cluster_centers` - k_estimate_finish (ops.pose_estimate),
k_shard_estimate_finish (the sharded engine's, over concatenated partials) and k_loop_cluster_finish with cluster_rotation_write
beside the annealing (one LoopEngine frame) - on the sets where the arithmetic is under strain: a cluster 1 m from the origin with
the loop's own noise, the same collapsed onto one pose, uniformly random rotations, centres on a half turn about x, y, z and
(1,1,0)/sqrt 2, and 129 blocks.  Each is bit for bit `ops.cluster_centers` on the same set AND inside `_recipes.assert_cluster`'s
bounds against `_recipes.cluster_reference`.  Needs an MI355X."""
import numpy as np
import pytest

from _recipes import CL_FIN_ROWS as FIN_ROWS, assert_cluster, cluster_reference, cluster_set, cluster_set_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIN_SETS = sorted({n for row in FIN_ROWS for n in row})


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _same(a, b):
    """Bit for bit - -0.0 is not +0.0 - with a NaN equal to a NaN whatever its payload."""
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.contiguous().view(torch.int32)[~na], b.contiguous().view(torch.int32)[~nb]))


@pytest.fixture(scope="module")
def single(dev):
    """name -> (poses, float64 weights on the device, ops.cluster_centers's centre (4,4) and spread (3,)), each set once."""
    from midastouch_amd import ops
    out = {}
    for name in FIN_SETS:
        s = cluster_set(name)
        P, w = torch.as_tensor(s["poses"]).to(dev), torch.as_tensor(np.asarray(s["w"], dtype=np.float64)).to(dev)
        c, sd, _ = ops.cluster_centers(P, w, torch.zeros(P.shape[0], dtype=torch.int64, device=dev), torch.tensor([0], device=dev))
        out[name] = (P, w, c[0], sd[0])
    return out


def _against_reference(name, c, sd, log, what):
    if not cluster_set(name).get("reference", True):  # (weights of mixed sign, a zero weight sum: no reference applies, the forms
        return                                         # agree bit for bit)
    s, ref = cluster_set_reference(name)
    assert_cluster(c[None], sd[None], ref, -(-len(s["labels"]) // 256), f"{what} on {name}", log=log)


def _show(what, log):
    print(f"\n{what}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in log.items()))


def test_single_call_on_the_finishers_sets(single):
    log = {}
    for name, (_, _, c, sd) in single.items():
        _against_reference(name, c, sd, log, "k_cluster_finish")
    _show("k_cluster_finish (64 threads)", log)


@pytest.mark.parametrize("row", range(len(FIN_ROWS)))
def test_pose_estimate_rows_of_different_regimes(dev, single, row):
    """k_estimate_finish (256 threads, the extrema on the second wave): B = 3 trajectories of different regimes by one call."""
    from midastouch_amd import ops
    names, log = FIN_ROWS[row], {}
    c, sd = ops.pose_estimate(torch.stack([single[n][0] for n in names]), torch.stack([single[n][1] for n in names]))
    for b, name in enumerate(names):
        assert _same(c[b], single[name][2]) and _same(sd[b], single[name][3]), (name, c[b], single[name][2], sd[b], single[name][3])
        _against_reference(name, c[b], sd[b], log, "k_estimate_finish")
    _show(f"k_estimate_finish, rows {names}", log)


@pytest.mark.parametrize("slices", [2, 3])
def test_sharded_finish_over_concatenated_partials(dev, single, slices):
    """midas_shard_estimate_moments over two and three slices of the set (all but the last a multiple of 4096 particles: "each
    rank's own blocks, ranks in order" are then the single call's blocks), the partials concatenated, midas_shard_estimate_finish."""
    from midastouch_amd import _lib
    from midastouch_amd._lib import _ptr
    ctx, log = _lib.context(dev), {}
    for name, (P, w, c1, s1) in single.items():
        N = P.shape[0]
        cut = (N // slices) // 4096 * 4096
        bounds = [k * cut for k in range(slices)] + [N]
        assert cut > 0 and all(b % 4096 == 0 for b in bounds[:-1])
        parts = []
        for lo, hi in zip(bounds, bounds[1:]):
            Ps, ws = P[lo:hi].contiguous(), w[lo:hi].contiguous()
            part = torch.empty(-(-(hi - lo) // 256) * 36, dtype=torch.float64, device=dev)
            ctx.call("midas_shard_estimate_moments", hi - lo, _ptr(Ps), _ptr(ws), _ptr(part))
            parts.append(part)
        allp = torch.cat(parts)
        assert allp.numel() == -(-N // 256) * 36
        c, sd = torch.empty((4, 4), dtype=torch.float32, device=dev), torch.empty((3,), dtype=torch.float32, device=dev)
        ctx.call("midas_shard_estimate_finish", allp.numel() // 36, _ptr(allp), _ptr(c), _ptr(sd))
        torch.cuda.synchronize()
        assert _same(c, c1) and _same(sd, s1), (name, slices, c, c1, sd, s1)
        _against_reference(name, c, sd, log, f"k_shard_estimate_finish, {slices} slices")
    _show(f"k_shard_estimate_finish, {slices} slices", log)


# ---- the loop step's finisher ---------------------------------------------------------------------------------------------------
LOOP_REGIMES = ("far", "far_weighted", "collapsed", "uniform", "pi_x", "pi_y", "pi_z", "pi_xy", "blocks129")


@pytest.fixture(scope="module")
def loop_scene():
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook(K=2000, D=256, seed=1013, mesh_points=20000)
    traj = make_trajectory(cb, T=3, seed=2013)
    return cb, traj


@pytest.mark.parametrize("regime", LOOP_REGIMES)
def test_loop_frame_cluster_centre(dev, oracle, loop_scene, regime):
    """k_loop_cluster_finish (256 threads) with the rotation solved by cluster_rotation_write beside the annealing: one LoopEngine
    frame with cluster=True on a set placed by set_particles (labels 0, no DBSCAN), read from frame_view().  The weights are the
    frame's own: the reference gets fv["weights"] and fv["poses_prop"].  far / collapsed: the object and its codebook moved 1 m
    from the origin, every particle on one codebook pose with the loop's 2e-4 m of noise / with none (one score: the weights are
    equal, the flattened moments) - far_weighted: on that pose and its two nearest neighbours, three scores, the WEIGHTED one-pass
    moments at 1 m; uniform, pi_*: rotations
    drawn uniformly / around a half turn at translations of the codebook's; blocks129: 32 769 particles.  `var` is the float32 mean
    of the frame's own spreads; whether it is the reference's float32 is printed, not asserted (DESIGN.md says where it is)."""
    from scipy.spatial.transform import Rotation

    from _recipes import CL_AXES
    from midastouch_amd import ops
    from midastouch_amd.loop_engine import LoopEngine
    cb, traj = loop_scene
    rng = np.random.default_rng([LOOP_REGIMES.index(regime), 31])
    N = 32769 if regime == "blocks129" else 4099
    cb_poses, verts = cb.poses.copy(), np.asarray(cb.mesh_vertices).copy()
    tn = np.zeros((N, 3), dtype=np.float32)
    if regime in ("far", "far_weighted", "collapsed"):
        off = np.float32([0.6, -0.64, 0.48])
        cb_poses[:, :3, 3] += off
        verts = (verts.astype(np.float32) + off).astype(verts.dtype)
        start = np.repeat(cb_poses[777][None], N, axis=0)
        if regime == "far_weighted":  # entry 777 and its two nearest neighbours: three scores, unequal weights, the weighted moments
            near = np.argsort(np.linalg.norm(cb_poses[:, :3, 3] - cb_poses[777, :3, 3], axis=1))[:3]
            start = cb_poses[near[rng.integers(0, 3, N)]].copy()
        if regime != "collapsed":
            tn = rng.normal(0.0, 2e-4, (N, 3)).astype(np.float32)
    else:
        start = cb_poses[rng.integers(0, cb_poses.shape[0], N)].copy()
        if regime == "uniform":
            start[:, :3, :3] = Rotation.random(N, random_state=5).as_matrix()
        elif regime.startswith("pi_"):
            Rc = Rotation.from_rotvec(np.array(CL_AXES[regime[3:]]) * np.pi)
            start[:, :3, :3] = (Rc * Rotation.from_rotvec(0.05 * rng.standard_normal((N, 3)))).as_matrix()
    eng = LoopEngine(cb_poses, cb.embeddings, verts, N, seed=4100, cluster=True, cluster_every=5, device=dev)
    eng.set_particles(torch.as_tensor(start))
    eng.step(torch.eye(4), torch.as_tensor(traj.codes[1]), tn=torch.as_tensor(tn), rot=torch.zeros(N, 3), dbscan=False)
    fv = eng.frame_view()
    assert fv["n"] == N and fv["clusters"] == 1 and fv["err"] == 0
    pp, w = fv["poses_prop"], fv["weights"]
    w_np = w.cpu().numpy()
    ref = cluster_reference(pp.cpu().numpy(), w_np, np.zeros(N, dtype=np.int64))
    assert ref[0]["flat"] or (w_np >= 0).all()  # (equal scores: the raw, negative scores are the weights - flattened to 1)
    assert ref[0]["flat"] == (regime in ("far", "collapsed")), regime  # (one codebook entry: one score; everything else is weighted)
    c1, s1, _ = ops.cluster_centers(pp, w, torch.zeros(N, dtype=torch.int64, device=dev), torch.tensor([0], device=dev))
    got_c, got_s = fv["cluster_poses"], fv["cluster_stds"]
    assert got_c.shape == (1, 4, 4) and got_s.shape == (1, 3)
    assert np.array_equal(got_c.view(np.int32), c1.cpu().numpy().view(np.int32)), (regime, got_c, c1)  # (bits: -0.0 is not +0.0)
    assert np.array_equal(got_s.view(np.int32), s1.cpu().numpy().view(np.int32)), (regime, got_s, s1)
    log = {}
    assert_cluster(got_c, got_s, ref, -(-N // 256), f"k_loop_cluster_finish, {regime}", log=log)
    assert np.float32(fv["var"]) == oracle.cluster_var(got_s), (fv["var"], got_s)
    var_ref = oracle.cluster_var(ref[0]["std"][None])
    _show(f"k_loop_cluster_finish, {regime}: flat {ref[0]['flat']}, valid {int(fv['valid'].sum())} of {N}, drifted {fv['drifted']}, "
          f"max|t| {ref[0]['tmax']:.3g}, spread {got_s[0]}, var {np.float32(fv['var'])!r} vs the reference's {var_ref!r} "
          f"(equal: {np.float32(fv['var']) == var_ref})", log)
