"""DBSCAN on the device at its edges (csrc/dbscan.hip, csrc/dbscan_nd.hip): the lattice cases of tests/_recipes.py - points exactly on
eps, neighbour counts exactly at min_samples and one short, cells of 1 .. 300 coincident particles, clusters joined by one pair,
border points whose only link lies on the sphere, the corner cells of the 5 x 5 x 5 walk - and the rounding cases of the float64
predicate, at every site that launches the kernels.  Labels, cluster count and error word are compared with the recipes' integer
reference (the rounding cases: the float64 restatement) by exact equality; tests/test_dbscan_edges_reference.py holds the same cases
against the oracle, sklearn and fixture G17 on the CPU.  DESIGN.md, "DBSCAN's rule", has the sites:

  D1 ops.dbscan, dense grid                     D5 BatchLoopEngine, batched_dbscan True and False
  D2 ops.dbscan, hashed table                   D6 particle_filter.cluster_particles(method="euclidean") on G17
  D3 ops.dbscan_batch, a case per row           D7 ops.dbscan_points, 2 .. 6 dimensions
  D4 LoopEngine's DBSCAN frame"""
import numpy as np
import pytest

from _recipes import DB_POINTS_SIZES, db_edge_cases, db_f64_dbscan, db_fixture_cases, db_int_dbscan, db_points_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K, D = 3000, 256


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    return db_edge_cases()  # (the recipes assert their conditions while they build: a case that is not what its name says fails here)


@pytest.fixture(scope="module")
def cb():
    from midastouch_amd.synthetic import make_codebook
    return make_codebook(K=K, D=D, seed=1014, mesh_points=20000)


def _poses_of(X):
    P = torch.eye(4)[None].repeat(len(X), 1, 1).clone()
    P[:, :3, 3] = torch.as_tensor(np.asarray(X, dtype=np.float32))
    return P


def _flip_point(c):
    """A point that changes the case's labels if a stale slot holding it is read: another copy of the probe's site p makes p a core
    point at c + 1; elsewhere another copy of the first point moves a count."""
    return c["X"][c.get("p", c.get("x", 0))]


_REF = {}


def _reference(c, eps, ms):
    """The labels of case c under another row's eps and min_samples (a batch has one of each): the integer reference on the same
    lattice, the float64 restatement otherwise."""
    ms = len(c["X"]) // 5 if ms < 0 else ms
    if eps == c["eps"] and ms == c["ms"]:
        return c["labels"], c["ncl"]
    key = (c["name"], eps, ms)
    if key not in _REF:
        if "V" in c and eps == c["eps"]:
            _REF[key] = db_int_dbscan(c["V"], c["m"] * c["m"], ms)[:2]
        else:
            assert len(c["X"]) <= 500
            _REF[key] = db_f64_dbscan(c["X"], eps, ms)[:2]
    return _REF[key]


# ---- D1, D2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hashed", [False, True], ids=["D1-dense", "D2-hashed"])
def test_single_pass_every_case(dev, cases, hashed):
    """ops.dbscan on every case with its min_samples given and, where the case's min_samples is n // 5, left to the entry."""
    from midastouch_amd import ops
    ran = 0
    for c in cases.values():
        if c["hashed"] != hashed:
            continue
        P = _poses_of(c["X"]).to(dev)
        for ms in ([c["ms"], -1] if c["fifth"] else [c["ms"]]):
            lab, info = ops.dbscan(P, c["eps"], ms)
            lab, info = lab.cpu().numpy(), info.cpu().tolist()
            bad = np.flatnonzero(lab != c["labels"])
            assert not len(bad), (c["name"], ms, len(bad), bad[:8].tolist(), lab[bad[:8]].tolist(), c["labels"][bad[:8]].tolist())
            assert info == [c["ncl"], 0], (c["name"], ms, info)
            ran += 1
    print(f"D{2 if hashed else 1}: {ran} invocations")
    assert ran >= 100


# ---- D3 -------------------------------------------------------------------------------------------------------------------------
def _batch_groups(cases, B):
    """Groups of B cases with one eps (a batch has one eps and one min_samples): every case is row 0 of one group - the group runs
    under ITS min_samples -, the other rows are the next small cases of the same eps in the list, dense and hashed alternating."""
    by_eps = {}
    for c in cases.values():
        by_eps.setdefault(c["eps"], []).append(c)
    groups = []
    for eps, lst in by_eps.items():
        small = [c for c in lst if len(c["X"]) <= 500] or lst
        dense, hashed = [c for c in small if not c["hashed"]], [c for c in small if c["hashed"]]
        for i, c in enumerate(lst):
            rows = [c]
            for j in range(1, B):
                pool = (hashed if (j % 2) != c["hashed"] else dense) or small
                rows.append(pool[(i * (B - 1) + j) % len(pool)])
            groups.append(rows)
    return groups


@pytest.mark.parametrize("B", [3, 6])
def test_batch_a_case_per_row(dev, cases, B):
    """ops.dbscan_batch: S = floor(2^21 / B) is no power of two; dense and hashed rows in one call, ragged counts, the slots behind
    n_b filled with a point that flips the row's labels if read.  Once with the first row's min_samples, and once with n_b // 5."""
    from midastouch_amd import ops
    ran = rows_checked = mixed = 0
    for rows in _batch_groups(cases, B):
        eps = rows[0]["eps"]
        ns = [len(c["X"]) for c in rows]
        cap = max(ns) + 3
        P = torch.eye(4).repeat(B, cap, 1, 1).clone()
        for b, c in enumerate(rows):
            P[b, :ns[b], :3, 3] = torch.as_tensor(c["X"])
            P[b, ns[b]:, :3, 3] = torch.as_tensor(_flip_point(c))
        P = P.to(dev)
        mixed += len({c["hashed"] for c in rows}) == 2
        for ms in ((rows[0]["ms"], -1) if rows[0]["fifth"] else (rows[0]["ms"],)):
            out = torch.full((B, cap), -7, dtype=torch.int32, device=dev)
            lab, info = ops.dbscan_batch(P, counts=ns, eps=eps, min_samples=ms, out=out)
            lab, info = lab.cpu().numpy(), info.cpu().tolist()
            for b, c in enumerate(rows):
                ref, ncl = _reference(c, eps, ms)
                assert np.array_equal(lab[b, :ns[b]], ref), (rows[0]["name"], b, c["name"], ms)
                assert (lab[b, ns[b]:] == -7).all() and info[b] == [ncl, 0], (rows[0]["name"], b, c["name"], ms, info[b])
                rows_checked += 1
            ran += 1
    print(f"D3 B={B}: {ran} invocations, {rows_checked} rows, {mixed} groups with dense and hashed rows")
    assert ran >= len(cases) and mixed >= 100


# ---- D4, D5: the loop engines' DBSCAN frame -------------------------------------------------------------------------------------
def _loop_cases(cases):
    """The cases whose min_samples is n // 5 (the loop engines take no other), the tiny sets below 5 points included, by eps."""
    by_eps = {}
    for c in cases.values():
        if c["fifth"]:
            by_eps.setdefault(c["eps"], []).append(c)
    return by_eps


def _check_frame(fv, c, what):
    X = fv["poses_prop"][:, :3, 3].cpu().numpy()
    assert X.shape == c["X"].shape and np.array_equal(X.view(np.uint32), c["X"].view(np.uint32)), f"{what}: poses_prop is not the lattice"
    lab = fv["labels_frame"].cpu().numpy()
    assert np.array_equal(lab, c["labels"]), (what, np.flatnonzero(lab != c["labels"])[:8].tolist())
    assert (fv["ncl"], fv["err"], fv["n"]) == (c["ncl"], 0, len(c["X"])), (what, fv["ncl"], fv["err"], fv["n"])


def test_loop_engine_frame(dev, cases, cb):
    """LoopEngine: launch_dbscan on a live count below the capacity with n // 5 and the loop's 62-cluster ranking; no motion noise and
    identity odometry, so the frame's propagated translations are the lattice bit for bit (asserted); stale slots behind n as in D3."""
    from midastouch_amd.loop_engine import LoopEngine
    from midastouch_amd.synthetic import make_trajectory
    code = torch.as_tensor(make_trajectory(cb, T=2, seed=2014).codes[1]).to(dev)
    cap = 2800
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, cap, seed=4400, floor=100000, pen_max=1e3, device=dev)
    odom = torch.eye(4, device=dev)
    ran = 0
    for eps, lst in _loop_cases(cases).items():
        eng.eps = eps
        for c in lst:
            n = len(c["X"])
            eng.set_particles(_poses_of(c["X"]))
            eng._poses[n:] = _poses_of(_flip_point(c)[None]).to(dev)
            z = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            eng.step(odom, code, tn=z, rot=z, u=torch.full((cap,), 0.5, dtype=torch.float64, device=dev), dbscan=True)
            _check_frame(eng.frame_view(), c, c["name"])
            ran += 1
    print(f"D4: {ran} frames")
    assert ran >= 45


@pytest.mark.parametrize("batched", [True, False], ids=["D5-batched", "D5-serial"])
def test_batch_loop_engine_frame(dev, cases, cb, batched):
    """BatchLoopEngine, a case per trajectory: the one batched pass and the serial passes; sig_t = sig_r = 0 and identity odometry."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.synthetic import make_trajectory
    code = torch.as_tensor(make_trajectory(cb, T=2, seed=2014).codes[1])
    ran = 0
    for eps, lst in _loop_cases(cases).items():
        B, cap = len(lst), 2800
        eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=4500, floor=100000, pen_max=1e3, eps=eps, sig_t=0.0, sig_r=0.0,
                              device=dev, batched_dbscan=batched)
        assert eng.batched_dbscan is batched
        eng.set_particles([_poses_of(c["X"]) for c in lst])
        for b, c in enumerate(lst):
            eng._poses[b, len(c["X"]):] = _poses_of(_flip_point(c)[None]).to(dev)
        eng.step(torch.eye(4)[None].repeat(B, 1, 1), code[None].repeat(B, 1), dbscan=True)
        for b, c in enumerate(lst):
            _check_frame(eng.frame_view(b), c, f"row {b}: {c['name']}")
            ran += 1
        assert not eng.ctl_i[:, 14].any()
    print(f"D5 batched={batched}: {ran} rows")
    assert ran >= 45


# ---- D6 -------------------------------------------------------------------------------------------------------------------------
def test_class_surface_on_g17(dev, golden):
    """particle_filter.cluster_particles(method="euclidean") on fixture G17, the reference's own labels at the edges."""
    from midastouch_amd.particle_filter import Particles, particle_filter
    g = golden("g17_dbscan_edges")
    g = {k: g[k] for k in g.files}
    pf = particle_filter.__new__(particle_filter)
    assert len(g["names"]) == len(db_fixture_cases())
    for i, name in enumerate(g["names"]):
        at, n, k = int(g["case_at"][i]), int(g["case_n"][i]), int(g["case_k"][i])
        X = ((g["local"][at:at + n].astype(np.int64) + g["case_off"][i]) * 2.0 ** -k).astype(np.float32)
        parts = pf.cluster_particles(Particles(_poses_of(X).to(dev)), eps=int(g["case_m"][i]) * 2.0 ** -k)
        lab = parts.labels.cpu().numpy()
        assert lab.dtype == np.int64 and np.array_equal(lab, g["labels"][at:at + n].astype(np.int64)), str(name)
    print(f"D6: {len(g['names'])} calls")


# ---- D7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3, 4, 5, 6])
def test_points_all_pairs(dev, dim):
    """ops.dbscan_points on float64 lattices (beyond float32's reach except in three dimensions) at N = 255, 256, 257, 513: counts
    exactly at min_samples through on-eps neighbours, a chain whose number travels more than one spread step, a second cluster at
    m^2 + 1, on-eps border points; in three dimensions also against the grid kernel."""
    from midastouch_amd import ops
    for N in DB_POINTS_SIZES:
        c = db_points_case(dim, N)
        lab, info = ops.dbscan_points(torch.as_tensor(c["X"]).to(dev), c["eps"], c["ms"])
        lab, info = lab.cpu().numpy(), info.cpu().tolist()
        assert np.array_equal(lab, c["labels"]), (c["name"], np.flatnonzero(lab != c["labels"])[:8].tolist())
        assert info[0] == c["ncl"] and info[1] >= 3, (c["name"], info)   # (a synchronous spread needs 6 .. 10 steps on these chains)
        if dim == 3:
            lab3, info3 = ops.dbscan(_poses_of(c["X"]).to(dev), c["eps"], c["ms"])
            assert np.array_equal(lab3.cpu().numpy(), c["labels"]) and info3.cpu().tolist() == [c["ncl"], 0], c["name"]
