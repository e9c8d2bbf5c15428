"""The per-frame pose estimate of the fixed-N engines (`estimate=True`, midas_pose_estimate / midas_lazy_run_estimate): for every
trajectory of a frame, bit for bit, what `ops.cluster_centers` gives on that trajectory's propagated poses and masked pre-resample
weights with every label 0 (filter/filter.py:184-186 on a particle set nobody has clustered) - from the eager engines' weights and
from the pipelined engines' tables without a flush - and nothing else about the engine changes.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K, D = 12000, 256  # the sizes of tests/knob_case.py
STATE = ("nn_idx", "poses_prop", "ridx", "poses", "weights", "weights_res", "hint", "status", "rmse")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scene(dev):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook("004_sugar_box", K=K, D=D, seed=1301)
    traj = make_trajectory(cb, T=40, seed=2301)
    od, co, gt = (torch.as_tensor(x).to(dev) for x in (traj.odoms, traj.codes, traj.gt_poses))
    return cb, od, co, gt


def _single(poses, weights):
    """Today's call for one trajectory: (centre (4,4), stds (3,))."""
    from midastouch_amd import ops
    N = poses.shape[0]
    c, s, _ = ops.cluster_centers(poses, weights, torch.zeros(N, dtype=torch.int64, device=poses.device), torch.tensor([0], device=poses.device))
    return c[0], s[0]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.allclose(a, b, rtol=0.0, atol=0.0, equal_nan=True)


# ---- 1, 5: the plain batched call ---------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 4097, 30_011])
def test_batched_call_matches_single_calls_and_oracle(dev, oracle, N):
    from _recipes import assert_cluster, cluster_reference
    from midastouch_amd import ops
    from test_cluster_centers import _clustered
    B = 5
    poses, weights = [], []
    for b in range(B):
        P, w, _ = _clustered([N], seed=40 + b)
        if b == 2:
            w = np.full(N, 0.37)        # all equal: the flatten branch
        elif b == 3:
            w = np.zeros(N)             # all 0 (every particle pruned): flat as well
        elif b == 4:
            w = np.resize(np.array([1.0, -1.0, 2.0, -2.0]), N)  # mixed sign; at N = 256 the sum is exactly 0 and the set is not flat
        poses.append(P)
        weights.append(w.astype(np.float64))
    if N == 256:
        assert weights[4].astype(np.float32).sum(dtype=np.float64) == 0.0 and weights[4].max() != weights[4].min()
    P = torch.as_tensor(np.stack(poses)).to(dev)
    W = torch.as_tensor(np.stack(weights)).to(dev)
    c, s = ops.pose_estimate(P, W)
    assert c.shape == (B, 4, 4) and s.shape == (B, 3) and c.dtype == torch.float32 and s.dtype == torch.float32
    for b in range(B):
        c1, s1 = _single(P[b], W[b])
        if b == 4:  # (oracle.cluster_centers raises on it: eigh of a matrix of NaN - no yardstick there)
            assert _same(c[b], c1) and _same(s[b], s1), (N, b)
            continue
        assert torch.equal(c[b], c1) and torch.equal(s[b], s1), (N, b)
        _, ref_c, ref_s = oracle.cluster_centers(poses[b], weights[b], np.zeros(N, dtype=np.int64))
        assert np.isfinite(ref_c).all() and np.isfinite(ref_s).all(), (N, b)
        assert np.abs(c[b].cpu().numpy() - ref_c[0]).max() < 2e-6, (N, b)
        np.testing.assert_allclose(s[b].cpu().numpy(), ref_s[0], rtol=2e-4, atol=1e-9)
        assert_cluster(c[b][None], s[b][None], cluster_reference(poses[b], weights[b], np.zeros(N, dtype=np.int64)), -(-N // 256), f"N {N}, row {b}")
    # the same call twice: the same bits (fixed summation order, no atomics)
    c2, s2 = ops.pose_estimate(P, W)
    assert _same(c, c2) and _same(s, s2)


def test_batched_call_checks_its_operands(dev):
    from midastouch_amd import ops
    from midastouch_amd._lib import MidasError
    with pytest.raises(MidasError):
        ops.pose_estimate(torch.zeros(2, 8, 4, 4, device=dev), torch.zeros(2, 7, device=dev))
    with pytest.raises(MidasError):
        ops.pose_estimate(torch.zeros(8, 4, 4, device=dev), torch.zeros(8, device=dev))


# ---- 2: the four engines beside a twin built without the keyword -------------------------------------------
def _make(kind, scene, dev, estimate, softmax=True, **kw):
    from midastouch_amd import engine
    cb, od, co, gt = scene
    rng = np.random.default_rng(5)
    if kind in ("FilterEngine", "PipelinedFilterEngine"):
        N = 30_011 if kind == "FilterEngine" else 100_000
        eng = getattr(engine, kind)(cb.poses, cb.embeddings, cb.mesh_vertices, N, seed=4100, softmax=softmax, device=dev, estimate=estimate, **kw)
        eng.set_particles(torch.as_tensor(cb.poses[rng.integers(0, K, N)]))  # a wide start
        if kind == "PipelinedFilterEngine":
            eng.project_to_codebook()
        return eng, lambda t: dict(odom=od[t], code=co[t], gt=gt[t])
    B, N = 6, 5000
    eng = getattr(engine, kind)(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, seed=4300, softmax=softmax, device=dev, estimate=estimate, **kw)
    eng.set_particles(torch.as_tensor(np.stack([cb.poses[rng.integers(0, K, N)] for _ in range(B)])))
    if kind == "PipelinedBatchFilterEngine":
        eng.project_to_codebook()
    return eng, lambda t: dict(odoms=torch.stack([od[t]] * B), codes=torch.stack([co[t]] * B), gts=torch.stack([gt[t]] * B))


def _check_frame(eng, twin, tag):
    """eng.estimate against today's call on the TWIN's poses_prop / weights (on a pipelined twin the read flushes it)."""
    c, s = eng.estimate
    pp, w = twin.poses_prop, twin.weights
    if pp.dim() == 3:
        assert c.shape == (4, 4) and s.shape == (3,)
        c, s, pp, w = c[None], s[None], pp[None], w[None]
    assert c.shape == (pp.shape[0], 4, 4) and s.shape == (pp.shape[0], 3) and c.dtype == torch.float32 and s.dtype == torch.float32
    for b in range(pp.shape[0]):
        c1, s1 = _single(pp[b], w[b])
        assert _same(c[b], c1) and _same(s[b], s1), (tag, b, c[b], c1, s[b], s1)


def _check_state(eng, twin, tag):
    for name in STATE:
        assert torch.equal(getattr(eng, name), getattr(twin, name)), (tag, name)


ENGINES = ["FilterEngine", "PipelinedFilterEngine", "BatchFilterEngine", "PipelinedBatchFilterEngine"]


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("kind", ENGINES)
def test_engine_estimate_beside_twin(dev, scene, kind, softmax):
    from midastouch_amd._lib import MidasError
    eng, frame = _make(kind, scene, dev, True, softmax)
    twin, _ = _make(kind, scene, dev, False, softmax)
    with pytest.raises(MidasError):
        twin.estimate
    rows = eng.estimate
    for t in range(1, 9):
        eng.step(**frame(t))
        twin.step(**frame(t))
        _check_frame(eng, twin, (kind, softmax, t))
        assert eng.estimate[0].data_ptr() == rows[0].data_ptr() and eng.estimate[1].data_ptr() == rows[1].data_ptr()  # allocated once
        if not softmax and hasattr(eng, "flush"):
            # Raw scores of mixed sign make a CDF that is not monotone: the folded search and the materialised one may then pick
            # different sources (so do two engines built WITHOUT the keyword, one only stepped, one read every frame - see the
            # module's last test).  The twin's weights were just read, i.e. it is flushed: the engine follows, so that both take the
            # same path into the next frame.  The folded path with raw weights: test_reading_estimate_keeps_resample_folded.
            assert eng._pending and not eng._flushed
            eng.flush()
    if softmax:  # (a converging filter: the estimate is a pose and a spread, finite)
        assert torch.isfinite(eng.estimate[0]).all() and torch.isfinite(eng.estimate[1]).all()
    _check_state(eng, twin, (kind, softmax))


@pytest.mark.parametrize("kind", ["BatchFilterEngine", "PipelinedBatchFilterEngine"])
def test_batch_flatten_branch_and_pruned_trajectory(dev, scene, kind):
    """Trajectory 2: no motion noise and every particle on one codebook pose - equal scores, equal weights, the flatten branch.
    Trajectory 4: every particle started 1 m off the object - all of them pruned, all weights 0, the flatten branch as well (the
    unweighted mean, finite)."""
    from midastouch_amd import engine
    cb, od, co, gt = scene
    B, N = 6, 5000
    rng = np.random.default_rng(9)
    start = np.stack([cb.poses[rng.integers(0, K, N)] for _ in range(B)])
    start[2] = cb.poses[1234]
    start[4, :, :3, 3] += np.float32(1.0)
    engs = []
    for est in (True, False):
        e = getattr(engine, kind)(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, sig_t=0.0, sig_r=0.0, seed=4300, device=dev, estimate=est)
        e.set_particles(torch.as_tensor(start))
        engs.append(e)
    eng, twin = engs
    for t in range(1, 5):
        fr = dict(odoms=torch.stack([od[t]] * B), codes=torch.stack([co[t]] * B))
        eng.step(**fr)
        twin.step(**fr)
        _check_frame(eng, twin, (kind, t))
        w = twin.weights
        assert bool(w[2].max() == w[2].min()), "trajectory 2 was built to carry equal weights"
        assert bool((w[4] == 0).all()), "trajectory 4 was built to be pruned whole"
        c, s = eng.estimate
        assert torch.isfinite(c[2]).all() and torch.isfinite(s[2]).all() and torch.isfinite(c[4]).all() and torch.isfinite(s[4]).all()
        # flat: the unweighted mean - for identical particles the particle itself (to the float32 rounding of a rotation that went
        # through four float32 products and the quaternion round trip: 1e-5) with no spread (the moments' float64 rounding: 1e-6 m)
        assert torch.allclose(c[2], twin.poses_prop[2, 0], atol=1e-5) and float(s[2].abs().max()) < 1e-6
    _check_state(eng, twin, kind)


# ---- 3: reading the estimate materialises nothing ---------------------------------------------------------
@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("kind", ["PipelinedFilterEngine", "PipelinedBatchFilterEngine"])
def test_reading_estimate_keeps_resample_folded(dev, scene, kind, softmax):
    """Engine and twin are only ever stepped (the estimate is read every frame, nothing else): both stay pending, every frame
    folds the previous resample in, and after n frames - for several n, so that folded frames of every age are the last one -
    the estimate is today's call on the twin's materialised frame."""
    for n in (1, 2, 3, 5, 8):
        eng, frame = _make(kind, scene, dev, True, softmax)
        twin, _ = _make(kind, scene, dev, False, softmax)
        for t in range(1, n + 1):
            eng.step(**frame(t))
            twin.step(**frame(t))
            c, s = eng.estimate
            c, s = c.cpu(), s.cpu()  # (read back: a host turn per frame)
            assert (eng._pending, eng._flushed) == (twin._pending, twin._flushed) == (True, False), (n, t)
            if t > 1:  # the frame folded the previous resample in: its indices, without a flush on either side
                assert torch.equal(eng._ridx, twin._ridx), (n, t)
            assert torch.equal(eng.poses_prop, twin.poses_prop) and torch.equal(eng.nn_idx, twin.nn_idx), (n, t)
        if softmax:
            assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(s).all())
        _check_frame(eng, twin, (kind, softmax, n))
        assert eng._pending and not eng._flushed  # (the twin's weights were read, the engine's were not)
        _check_state(eng, twin, (kind, softmax, n))


# ---- 4: T frames by one C call -----------------------------------------------------------------------
def test_run_leaves_every_frames_estimate(dev, scene):
    cb, od, co, gt = scene
    eng, _ = _make("PipelinedFilterEngine", scene, dev, True)
    twin, frame = _make("PipelinedFilterEngine", scene, dev, True)
    log = eng.run(od[1:13], co[1:13], gts=gt[1:13])
    ec, es = eng.estimate_log
    assert ec.shape == (12, 4, 4) and es.shape == (12, 3) and ec.dtype == torch.float32 and es.dtype == torch.float32
    assert log.shape == (12, 3)
    assert eng._pending and not eng._flushed
    for f in range(12):
        twin.step(**frame(1 + f))
        c, s = twin.estimate
        assert torch.equal(ec[f], c) and torch.equal(es[f], s), f
        assert torch.equal(log[f, :2], twin.rmse), f
    assert torch.equal(eng.estimate[0], ec[11]) and torch.equal(eng.estimate[1], es[11])
    # a second run() gives fresh tensors (the first log stays the caller's), and step() goes back to the engine's own rows
    first = (ec.clone(), es.clone())
    eng.run(od[13:16], co[13:16], gts=gt[13:16])
    assert eng.estimate_log[0].shape == (3, 4, 4) and torch.equal(ec, first[0]) and torch.equal(es, first[1])
    for t in range(13, 16):
        twin.step(**frame(t))
    assert torch.equal(eng.estimate[0], twin.estimate[0]) and torch.equal(eng.estimate[1], twin.estimate[1])
    eng.step(**frame(16))
    twin.step(**frame(16))
    assert torch.equal(eng.estimate[0], twin.estimate[0]) and torch.equal(eng.estimate[1], twin.estimate[1])
    _check_state(eng, twin, "run")
    # and a twin built without the keyword runs the same frames to the same state
    plain, _ = _make("PipelinedFilterEngine", scene, dev, False)
    plain.run(od[1:13], co[1:13], gts=gt[1:13])
    plain.run(od[13:16], co[13:16], gts=gt[13:16])
    plain.step(**frame(16))
    assert not hasattr(plain, "estimate_log")
    _check_state(eng, plain, "run, plain twin")


def test_raw_mixed_sign_weights_folded_and_materialised_paths(dev, scene):
    """Why the twin test keeps engine and twin in step with softmax=False: this records what two engines built WITHOUT the keyword
    do there - one only stepped, one whose weights are read (flushed) every frame.  Nothing is asserted about whether they agree
    (the reference resamples with p = w / sum(w), undefined for weights of mixed sign); with the softmax on they must."""
    for softmax in (True, False):
        a, frame = _make("PipelinedFilterEngine", scene, dev, False, softmax)
        b, _ = _make("PipelinedFilterEngine", scene, dev, False, softmax)
        same = []
        for t in range(1, 6):
            a.step(**frame(t))
            b.step(**frame(t))
            b.weights  # flushes b only
            same.append(torch.equal(a.poses_prop, b.poses_prop))
        print("softmax", softmax, "stepped-only == read-every-frame, per frame:", same)
        if softmax:
            assert all(same)
