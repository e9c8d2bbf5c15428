"""The device start (csrc/start.hip: midas_init_particles_batch, midas_project_batch; `_LoopBase.start`): `init_filter`
(modules/particle_filter.py:129-145) and the projection behind it (filter/filter.py:159-160) for B rows in two launches.

Bound of the composition: every entry within 6 u (|gt| @ |Tn|), u = 2^-24, of the float64 product of the float32 gt and the
reference's float32 Tn - a float32 dot product of four terms errs by at most gamma_4 = 4 u, and one flipped float32 rounding of a
rotation entry (the device's float64 sin / cos against scipy's) adds 2 u.

Three synthetic objects as in test_gpu_batch_loop_objects (K = 3000 / 900 / 1777, D = 128); ragged rows 1 .. 4097 of capacity 4200:
the edges of a wave, of a workgroup and of a 4096-block."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OBJECTS = (("004_sugar_box", 3000), ("025_mug", 900), ("cotter-pin", 1777))
D = 128
U = 2.0 ** -24
NS = [1, 63, 64, 65, 255, 257, 4097]
ROWS = [0, 1, 2, 0, 2, 1, 2]  # every object, no two rows of one object adjacent
CAP = 4200
SENTINEL = 7.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cbs():
    from midastouch_amd.synthetic import make_codebook
    return [make_codebook(name, K=K, D=D, seed=1013 + i, mesh_points=4000) for i, (name, K) in enumerate(OBJECTS)]


@pytest.fixture(scope="module")
def batch(dev, cbs):
    from midastouch_amd import BatchLoopEngine
    return BatchLoopEngine.for_objects([(c.poses, c.embeddings, c.mesh_vertices) for c in cbs], ROWS, CAP, seed=9100, device=dev, floor=300)


@pytest.fixture(scope="module")
def case(cbs):
    """Ground truths on each row's object, per-row sigmas, and draws already scaled (sigma 60 degrees and 0.08 m at the most)."""
    from midastouch_amd.synthetic import make_trajectory
    rng = np.random.default_rng(21)
    B = len(ROWS)
    gts = np.stack([make_trajectory(cbs[i], T=2, seed=300 + b).gt_poses[0] for b, i in enumerate(ROWS)]).astype(np.float32)
    sig = np.stack([np.float32([0.01 + 0.01 * b, 10.0 + 8.0 * b]) for b in range(B)])  # (B, 2): every row its own
    tn = (rng.normal(size=(B, CAP, 3)) * sig[:, None, :1]).astype(np.float32)
    rot = (rng.normal(size=(B, CAP, 3)) * sig[:, None, 1:]).astype(np.float32)
    return gts, sig, tn, rot


def _reference_tn(tn, rot):
    """The float32 Tn of init_filter as the reference builds it: scipy's float64 matrix stored into float32."""
    from scipy.spatial.transform import Rotation
    Tn = np.zeros((tn.shape[0], 4, 4), dtype=np.float32)
    Tn[:, :3, :3] = Rotation.from_euler("zyx", np.asarray(rot, dtype=np.float32), degrees=True).as_matrix().astype(np.float32)
    Tn[:, :3, 3], Tn[:, 3, 3] = tn, 1.0
    return Tn


def _bound(gt, Tn):
    return 6 * U * (np.abs(gt).astype(np.float64)[None] @ np.abs(Tn).astype(np.float64))


def _prefill(eng):
    eng._poses.fill_(SENTINEL)
    eng._hint.fill_(-5)
    eng._labels.fill_(3)
    eng.ctl_i.fill_(9)
    eng.ctl_d.fill_(2.5)


def _check_blocks(eng, ns):
    """The control blocks as set_particles(reset_annealing=True) leaves them, labels 0."""
    from midastouch_amd import _lib
    ci = eng.ctl_i.cpu().numpy()
    want = np.zeros_like(ci)
    want[:, _lib.LOOP_I_N] = want[:, _lib.LOOP_I_NSET] = ns
    want[:, _lib.LOOP_I_NCL] = 1
    assert np.array_equal(ci, want)
    assert not eng.ctl_d.any() and not eng._labels.any() and eng.n == list(ns)


def test_given_draws_within_the_bound_and_ragged_rows(batch, case):
    gts, sig, tn, rot = case
    _prefill(batch)
    batch.starts = 0
    batch.start(gts, sig, n=NS, project=False, tn=tn, rot=rot)
    assert batch.starts == 1
    P = batch._poses.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(NS):
        Tn = _reference_tn(tn[b, :n], rot[b, :n])
        exact = gts[b].astype(np.float64)[None] @ Tn.astype(np.float64)
        err, bound = np.abs(P[b, :n].astype(np.float64) - exact), _bound(gts[b], Tn)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) * 6)
        assert np.all(err <= bound), (b, n, float((err / np.maximum(bound, 1e-300)).max()) * 6)
        assert np.all(P[b, n:] == SENTINEL), (b, n)  # slots behind n_b: untouched
    print(f"worst error {worst:.2f} u (|gt| @ |Tn|)")
    assert torch.all(batch._hint == -1)  # off the codebook
    _check_blocks(batch, NS)


def test_philox_draws_match_the_oracle_stream(batch, case, oracle):
    """Row b draws philox_noise(n, seed + b, 0xFFFFFFFF - draw, its own sigmas); a second start draws fresh numbers (draw 1)."""
    gts, sig, _, _ = case
    batch.starts = 0
    first = None
    for draw in (0, 1):
        _prefill(batch)
        batch.start(gts, sig, n=NS, project=False, reset_annealing=True)
        assert batch.starts == draw + 1
        P = batch._poses.cpu().numpy()
        for b, n in enumerate(NS):
            tn, rot = oracle.philox_noise(n, batch.seed + b, 0xFFFFFFFF - draw, float(sig[b, 0]), float(sig[b, 1]))
            ref = oracle.init_filter_compose(gts[b], tn, rot)
            err = np.abs(P[b, :n].astype(np.float64) - ref.astype(np.float64))
            assert np.all(err <= _bound(gts[b], _reference_tn(tn, rot))), (draw, b, n)
            assert np.all(P[b, n:] == SENTINEL)
        _check_blocks(batch, NS)
        if first is None:
            first = P
    assert not np.array_equal(first[6, :4097], P[6, :4097]) and not np.array_equal(first[0, :1], P[0, :1])  # two starts differ


def test_same_draw_repeats_its_bits_and_keys_are_per_row(dev, case):
    from midastouch_amd import ops
    gts, sig, _, _ = case
    g, s = torch.as_tensor(gts).to(dev), torch.as_tensor(sig).to(dev)
    out = [torch.full((len(NS), CAP, 4, 4), SENTINEL, device=dev) for _ in range(4)]
    ops.init_particles_batch(out[0], g, s, NS, seed=77, draw=5)
    ops.init_particles_batch(out[1], g, s, NS, seed=77, draw=5)
    ops.init_particles_batch(out[2], g, s, NS, seed=77, draw=6)
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])
    # rows of one gt and one sigma still differ (key seed + b), and row b of seed s is row 0 of seed s + b
    g1, s1 = g[:1].repeat(3, 1, 1), s[:1].repeat(3, 1)
    same = torch.full((3, CAP, 4, 4), SENTINEL, device=dev)
    ops.init_particles_batch(same, g1, s1, [500] * 3, seed=77, draw=0)
    assert not torch.equal(same[0, :500], same[1, :500]) and not torch.equal(same[1, :500], same[2, :500])
    alone = torch.full((1, CAP, 4, 4), SENTINEL, device=dev)
    ops.init_particles_batch(alone, g1[:1], s1[:1], [500], seed=79, draw=0)
    assert torch.equal(alone[0], same[2])


def test_zero_sigma_is_the_ground_truth(batch, case):
    gts, _, _, _ = case
    _prefill(batch)
    batch.start(gts, (0.0, 0.0), n=NS, project=False)
    P = batch._poses.cpu().numpy()
    for b, n in enumerate(NS):
        assert np.all(P[b, :n] == gts[b][None]), b
        assert np.all(P[b, n:] == SENTINEL)


def test_refused_call_leaves_everything(dev, case):
    from midastouch_amd import ops
    from midastouch_amd._lib import MidasError
    gts, sig, _, _ = case
    g, s = torch.as_tensor(gts).to(dev), torch.as_tensor(sig).to(dev)
    P = torch.full((len(NS), CAP, 4, 4), SENTINEL, device=dev)
    H = torch.full((len(NS), CAP), -5, dtype=torch.int32, device=dev)
    for bad in ([CAP + 1] + NS[1:], NS[:-1] + [0]):
        with pytest.raises(MidasError):
            ops.init_particles_batch(P, g, s, bad)
    with pytest.raises(MidasError):
        ops.init_particles_batch(P, g, s, NS, tn=torch.zeros(len(NS), CAP, 3, device=dev))  # tn without rot
    with pytest.raises(MidasError):
        ops.project_batch(P, H, NS)  # neither a set nor a tree
    torch.cuda.synchronize()
    assert torch.all(P == SENTINEL) and torch.all(H == -5)


def test_projection_is_the_nn6_route_on_every_rows_object(batch, case):
    """start(project=True) row b == gather_rows(cb_poses, nn6(tree6, se3_feature(poses))) of start(project=False)'s poses on ITS
    object, poses and hints bit for bit; rows on the smaller codebooks would show a read of another object's index."""
    from midastouch_amd import ops
    gts, sig, tn, rot = case
    _prefill(batch)
    batch.start(gts, sig, n=NS, project=False, tn=tn, rot=rot, reset_annealing=True)
    off = batch._poses.clone()
    _prefill(batch)
    batch.start(gts, sig, n=NS, project=True, tn=tn, rot=rot, reset_annealing=True)
    top = [0, 0, 0]
    for b, n in enumerate(NS):
        o = batch.objects[ROWS[b]]
        idx = ops.nn6(o.tree6, ops.se3_feature(off[b, :n]))
        assert torch.equal(batch._hint[b, :n], idx), b
        assert torch.equal(batch._poses[b, :n], ops.gather_rows(o.cb_poses, idx)), b
        assert torch.all(batch._hint[b, n:] == -1) and torch.all(batch._poses[b, n:] == SENTINEL)
        assert not torch.equal(batch._poses[b, :n], off[b, :n])
        top[ROWS[b]] = max(top[ROWS[b]], int(idx.max()))
    assert top[0] >= 1777 and top[2] >= 900 and all(t < K for t, (_, K) in zip(top, OBJECTS)), top
    _check_blocks(batch, NS)


def test_projection_without_a_set(dev, cbs, case):
    """A plain BatchLoopEngine (every row on the one codebook): the entry's other branch, the same rule."""
    from midastouch_amd import BatchLoopEngine, ops
    gts, sig, tn, rot = case
    cb, ns = cbs[2], [65, 257, 1000]
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, 3, 1000, seed=5, device=dev)
    g = np.stack([gts[2], gts[4], gts[6]])  # (the rows of ROWS on object 2)
    eng.start(g, sig[:3], n=ns, project=False)
    off = eng._poses.clone()
    eng.starts = 0
    eng.start(g, sig[:3], n=ns)
    for b, n in enumerate(ns):
        idx = ops.nn6(eng.tree6, ops.se3_feature(off[b, :n]))
        assert torch.equal(eng._hint[b, :n], idx) and torch.equal(eng._poses[b, :n], ops.gather_rows(eng.cb_poses, idx)), b
        assert torch.all(eng._hint[b, n:] == -1)


class _Still:
    """The batch engine behind LoopEngine.step's `std_override` keyword: `_frame` hands one set of keywords to both kinds of engine,
    the batch takes this one through `step_still`."""

    def __init__(self, eng):
        self.__dict__["eng"] = eng

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def step(self, odoms, codes, gts=None, std_override=None, **kw):
        if std_override is None:
            return self.eng.step(odoms, codes, gts=gts, **kw)
        self.eng.step_still(odoms, codes, gts=gts, std_override=std_override, **kw)
        assert self.eng._std_override is None  # (the override does not outlive its frame)


def test_row_rule_start_and_six_frames(dev, cbs):
    """Batch start() row b is LoopEngine(seed + b).start() on its object - poses, hints, control blocks - and stays it: a frame,
    the second start the reference makes on frame 1 (annealing kept, fresh draws), five more frames; after every frame the whole
    log row, the per-particle arrays and the sets (test_gpu_batch_loop._frame)."""
    from test_gpu_batch_loop import _frame
    from test_gpu_batch_loop_objects import _engines, _trajs
    from midastouch_amd.synthetic import mesh_scale
    rows, N0, seed = [2, 0, 1, 2], 1500, 640
    ns = [1500, 1337, 1500, 900]
    trajs = _trajs(cbs, rows, 6, 2013)
    singles, batch = _engines(dev, cbs, rows, N0, seed, floor=400, cluster_every=3)
    sig = [[mesh_scale(cbs[i].extents) / 3.0 * 0.15, 9.0] for i in rows]

    def start(t):
        gts = np.stack([tr.gt_poses[t] for tr in trajs])
        for b, s in enumerate(singles):
            s.start(gts[b], sig[b], n=ns[b])
        batch.start(gts, sig, n=ns)
        for b, s in enumerate(singles):
            n = ns[b]
            assert torch.equal(batch._poses[b, :n], s._poses[:n]) and torch.equal(batch._hint[b], s._hint), (t, b)
            assert torch.equal(batch.ctl_i[b], s.ctl_i) and torch.equal(batch.ctl_d[b], s.ctl_d), (t, b)
            assert torch.equal(batch._labels[b], s._labels)
            assert s.n == n and int(s.ctl_i[0]) == n
        assert batch.n == ns and batch.starts == t + 1 and all(s.starts == t + 1 for s in singles)

    start(0)
    first = batch._poses.clone()
    _frame(singles, _Still(batch), trajs, 0, std_override=(0.0, 0.0))
    start(1)
    assert not torch.equal(first[0], batch._poses[0])
    assert int(batch.ctl_i[0, 12]) == 1 and int(singles[0].ctl_i[12]) == 1  # the frame count is kept (LOOP_I_FRAME)
    _frame(singles, _Still(batch), trajs, 1, std_override=(0.0, 0.0))
    for t in range(2, 6):
        _frame(singles, batch, trajs, t)
    assert not batch.ctl_i[:, 14].any()  # no limit / bound error flagged
