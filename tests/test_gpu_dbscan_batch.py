"""midas_dbscan_batch (one DBSCAN pass for B clouds, every row in its own region of the one set of cell tables) and the batch loop
engines' batched DBSCAN frame.  Every row of every case is held against oracle.dbscan on the CPU and against ops.dbscan on that row
alone; the engine cases against B single LoopEngines and against the engine that runs the serial passes, bit for bit.

The clouds are built by the functions at the head of the file; tests/test_dbscan_batch_abi.py checks on the CPU that they have the
properties the cases rely on (cluster counts, cells per axis)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-2
H = EPS * 0.577  # cell side (csrc/dbscan.hip DB_CELL)


# ---- the clouds -----------------------------------------------------------------------------------------------------------
def isolation_clouds():
    """Case 1 and the stream case 4 continues: cloud(k) = k points of a 1 mm blob + 1000 - k spread over a metre.  cloud(190) has no
    cluster at min_samples = 1000 // 5 = 200, twice over it would have one of 380; cloud(210) has one of 210."""
    rng = np.random.default_rng(11)
    cloud = lambda k: np.concatenate([rng.normal(0, 0.001, (k, 3)), rng.uniform(-0.5, 0.5, (1000 - k, 3))]).astype(np.float32)  # noqa: E731
    a = cloud(190)
    b = cloud(210)
    return rng, a, b


def many_cluster_rows():
    """Case 4: 80 centres x 12 points + 40 noise points (80 clusters at min_samples = 5: more than the 62 of the LDS ranking), a row
    with one cluster and a row with three.  1000 slots a row."""
    rng, _, _ = isolation_clouds()
    cen = rng.uniform(-0.3, 0.3, (80, 3))
    many = np.concatenate([rng.normal(c, 0.0015, (12, 3)) for c in cen] + [rng.uniform(-0.3, 0.3, (40, 3))])
    many = many[rng.permutation(len(many))]
    one = np.concatenate([rng.normal(0.1, 0.002, (300, 3)), rng.uniform(-0.3, 0.3, (200, 3))])
    three = np.concatenate([rng.normal(c, 0.002, (150, 3)) for c in ([0, 0, 0], [0.1, 0, 0], [0, -0.1, 0.05])] + [rng.uniform(-0.2, 0.2, (300, 3))])
    three = three[rng.permutation(len(three))]
    return [x.astype(np.float32) for x in (many, one, three)]


def mixed_rows():
    """Case 2: the recipes of test_dbscan_matches_oracle (tests/test_gpu_loop.py) side by side, ragged: (points, first blob centre)."""
    rng = np.random.default_rng(29)
    blobs = np.concatenate([rng.normal(c, 0.004, (400, 3)) for c in ([0, 0, 0], [0.03, 0, 0], [0, 0.04, 0.01])] + [rng.uniform(-0.03, 0.07, (300, 3))])
    t = rng.uniform(0, 0.5, 6000)
    chain = np.stack([t, 0.01 * np.sin(40 * t), rng.normal(0, 0.001, 6000)], axis=1)
    cen = rng.uniform(-1.5, 1.5, (4, 3))
    wide = np.concatenate([rng.normal(c, 0.004, (900, 3)) for c in cen] + [rng.uniform(-1.5, 1.5, (400, 3))])
    wide = wide[rng.permutation(len(wide))]
    dense = rng.normal(0, 0.0015, (5000, 3))
    one = np.array([[0.2, -0.1, 0.05]])
    rows = [(blobs, [0, 0, 0]), (chain, chain[0]), (wide, cen[0]), (dense, [0, 0, 0]), (one, one[0]), (np.zeros((0, 3)), [0, 0, 0])]
    return [(x.astype(np.float32), np.asarray(c, dtype=np.float32)) for x, c in rows]


def cells_per_axis(X):
    """Cells per axis as k_db_setup / k_dbb_setup count them: floor(extent / h) + 1 on the float32 bounds."""
    ext = X.max(axis=0).astype(np.float64) - X.min(axis=0).astype(np.float64)
    return (np.floor(ext / H) + 1).astype(np.int64)


def marked_blob(rng, n, cells, centre=None):
    """n - 2 points of a 1 mm blob (a cluster at min_samples = n // 5) and two marker points that give the cloud `cells` cells per axis."""
    far = (np.asarray(cells, dtype=np.float64) - 0.5) * H
    c = far / 2 if centre is None else np.asarray(centre)
    X = np.concatenate([np.zeros((1, 3)), rng.normal(c, 0.001, (n - 2, 3)), far[None]])
    return np.clip(X, 0.0, far).astype(np.float32)


def distinct_cells_row():
    """512 points, 8 x 8 x 8, 5.1 cells apart: 36 cells per axis (46 656 > 32 768: hashed), every point in a cell of its own."""
    g = (np.arange(8) * 5.1 + 0.5) * H
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def boundary_rows(last):
    """Case 3: 64 rows of up to 512 points, S = 32 768 slots a region.  Row 0: exactly 32 x 32 x 32 cells (dense, the region is full);
    row 1: 33 x 32 x 32 (hashed); row 2: distinct cells; row 63: `last` = "dense" (the full grid again: its closing cell_start entry
    is the tables' last) or "hashed"; the rest: blobs of 100 .. 512 points over 2 .. 40 cells per axis."""
    rng = np.random.default_rng(63)
    rows = []
    for b in range(64):
        if b == 0 or (b == 63 and last == "dense"):
            rows.append(marked_blob(rng, 512, (32, 32, 32)))
        elif b == 1 or (b == 63 and last == "hashed"):
            rows.append(marked_blob(rng, 512, (33, 32, 32)))
        elif b == 2:
            rows.append(distinct_cells_row())
        else:
            rows.append(marked_blob(rng, int(rng.integers(100, 513)), rng.integers(2, 41, 3)))
    return rows


# ---- helpers --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _stack(rows, cap, fill=None):
    """(B, cap, 4, 4) poses: row b's points, the slots behind them at fill[b] (a point that would change the counts if read)."""
    P = torch.eye(4).repeat(len(rows), cap, 1, 1).clone()
    for b, X in enumerate(rows):
        P[b, :len(X), :3, 3] = torch.as_tensor(X)
        if fill is not None:
            P[b, len(X):, :3, 3] = torch.as_tensor(fill[b])
    return P


def _check_rows(dev, oracle, rows, cap, ms, fill=None, max_clusters=0, counts=True):
    """ops.dbscan_batch on the rows against the oracle and the single pass, row by row; slots behind n_b keep their -7."""
    from midastouch_amd import ops
    P = _stack(rows, cap, fill).to(dev)
    out = torch.full((len(rows), cap), -7, dtype=torch.int32, device=dev)
    ns = [len(X) for X in rows]
    lab, info = ops.dbscan_batch(P, counts=ns if counts else None, eps=EPS, min_samples=ms, max_clusters=max_clusters, out=out)
    assert lab is out
    lab, info = lab.cpu().numpy(), info.cpu().numpy()
    for b, X in enumerate(rows):
        n = len(X)
        ref, ncl = oracle.dbscan(X, EPS, n // 5 if ms < 0 else ms) if n else (np.zeros(0, dtype=np.int64), 0)
        assert np.array_equal(lab[b, :n], ref), f"row {b}: labels against the oracle"
        assert (lab[b, n:] == -7).all(), f"row {b}: slots behind the live count were written"
        if max_clusters == 0:
            assert info[b].tolist() == [ncl, 0], f"row {b}"
        if n:
            one, one_info = ops.dbscan(P[b, :n], EPS, ms)
            assert np.array_equal(lab[b, :n], one.cpu().numpy()), f"row {b}: labels against the single pass"
            if max_clusters == 0:
                assert info[b].tolist() == one_info.cpu().tolist()
    return lab, info


# ---- midas_dbscan_batch ---------------------------------------------------------------------------------------------------
def test_rows_do_not_see_each_other(dev, oracle):
    """Rows 0 and 1 are the same cloud, 190 points of a blob below min_samples = 200: counted together they would be a cluster of
    380.  A table shared between rows fails this."""
    _, a, b = isolation_clouds()
    lab, info = _check_rows(dev, oracle, [a, a, b], 1000, -1, counts=False)
    assert (lab[:2] == -1).all() and info[:2].tolist() == [[0, 0], [0, 0]]
    assert info[2].tolist() == [1, 0] and (lab[2] == 0).sum() == 210


@pytest.mark.parametrize("ms", [-1, 25])
def test_mixed_rows_and_ragged_counts(dev, oracle, ms):
    """B = 6 (S = 349 525: no power of two): dense and hashed rows, 6000 .. 1 .. 0 points, in one call."""
    rows = mixed_rows()
    X = [x for x, _ in rows]
    assert [len(x) for x in X] == [1500, 6000, 4000, 5000, 1, 0]
    assert cells_per_axis(X[2]).max() > 128 and cells_per_axis(X[0]).max() <= 128 and cells_per_axis(X[3]).max() <= 128
    _check_rows(dev, oracle, X, 6000, ms, fill=[c for _, c in rows])


@pytest.mark.parametrize("last", ["dense", "hashed"])
def test_region_boundary(dev, oracle, last):
    rows = boundary_rows(last)
    assert cells_per_axis(rows[0]).tolist() == [32, 32, 32] and cells_per_axis(rows[1]).tolist() == [33, 32, 32]
    assert cells_per_axis(rows[63]).tolist() == ([32, 32, 32] if last == "dense" else [33, 32, 32])
    assert cells_per_axis(rows[2]).tolist() == [36, 36, 36]
    lab, info = _check_rows(dev, oracle, rows, 512, -1)
    assert info[0].tolist() == [1, 0] and info[1].tolist() == [1, 0] and info[63].tolist() == [1, 0] and info[2].tolist() == [0, 0]


def test_more_clusters_than_the_lds_ranking(dev, oracle):
    """80 clusters in one row of three (the prefix ranking per row); with max_clusters = 62 that row alone reports the limit, as
    the single pass does in the loop."""
    from midastouch_amd import ops
    rows = many_cluster_rows()
    lab, info = _check_rows(dev, oracle, rows, 1000, 5)
    assert info[:, 0].tolist() == [80, 1, 3]
    P = _stack(rows, 1000).to(dev)
    lab62, info62 = ops.dbscan_batch(P, counts=[len(x) for x in rows], eps=EPS, min_samples=5, max_clusters=62)
    info62 = info62.cpu().numpy()
    # (the limit leaves the clusters the LDS ranking holds, LOOP_MAX_CLUSTERS - 1 = 63 of them - which 63 is not defined - and bit 1)
    assert info62.tolist() == [[63, 2], [1, 0], [3, 0]]
    assert np.array_equal(lab62[1:].cpu().numpy(), np.where(np.arange(1000)[None] < np.array([[len(rows[1])], [len(rows[2])]]), lab[1:], -1))


def test_a_bad_row_stays_alone(dev, oracle):
    """One NaN translation in row 1: its flags are the single pass's, rows 0 and 2 hold the oracle's labels."""
    from midastouch_amd import ops
    rows = [x.copy() for x in many_cluster_rows()]
    P = _stack(rows, 1000).to(dev)
    P[1, 17, 0, 3] = float("nan")
    ns = [len(x) for x in rows]
    lab, info = ops.dbscan_batch(P, counts=ns, eps=EPS, min_samples=5)
    _, one_info = ops.dbscan(P[1, :ns[1]], EPS, 5)
    assert info[1, 1].item() == one_info[1].item()
    for b in (0, 2):
        ref, ncl = oracle.dbscan(rows[b], EPS, 5)
        assert np.array_equal(lab[b, :ns[b]].cpu().numpy(), ref) and info[b].cpu().tolist() == [ncl, 0], b


def test_beyond_the_bound_is_refused(dev):
    from midastouch_amd import _lib, ops
    with pytest.raises(_lib.MidasError, match="DBSCAN_BATCH_MAX_POINTS"):
        ops.dbscan_batch(torch.zeros((65, 16384, 4, 4), device=dev))


# ---- the engines ----------------------------------------------------------------------------------------------------------
from test_gpu_batch_loop import PER_PARTICLE, _near, _traj, cb  # noqa: E402, F401 (cb: fixture)

STARTS = (6000, 6000, 4097, 4096, 63)


def _blob_starts(cb, trajs):
    """Rows 0 and 1: two blobs on the codebook (around the first ground-truth pose and around the codebook pose farthest from it) and
    a fifth of the particles spread over a metre, off the object - 170 cells per axis at eps = 1e-2: the first frame's row is
    hashed; the spread particles are pruned and gone after the first resample.  Rows 2 .. 4: one blob."""
    rng = np.random.default_rng(41)
    t3 = cb.poses[:, :3, 3]
    starts = []
    for b, n in enumerate(STARTS):
        here = trajs[b].gt_poses[0][:3, 3]
        if b < 2:
            far = t3[int(np.argmax(np.linalg.norm(t3 - here, axis=1)))]
            k = n // 5
            spread = cb.poses[rng.integers(0, len(cb.poses), k)].copy()
            spread[:, :3, 3] = rng.uniform(-0.5, 0.5, (k, 3)).astype(np.float32)
            p = np.concatenate([_near(cb, here, 12, (n - k) // 2, rng), _near(cb, far, 12, n - k - (n - k) // 2, rng), spread])
            starts.append(p[rng.permutation(n)])
        else:
            starts.append(_near(cb, here, 60, n, rng))
    return starts


def _state(e, b=None):
    """Every array an engine carries from frame to frame and leaves behind a frame (row b of a batch engine)."""
    names = ("ctl_i", "ctl_d", "_poses", "poses_prop", "_hint", "_nn_idx", "_valid", "_x", "_e", "_w", "_w_res", "_labels", "_labels_prev",
             "_src", "_ridx", "_cl_poses", "_cl_stds")
    out = {}
    for k in names:
        v = getattr(e, k)
        out[k] = (v if b is None else v[b]).reshape(-1)
    return out


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _three_way_frame(singles, batched, serial, trajs, t, dbscan, gt=True):
    """Frame t of the B single engines, the batched-DBSCAN engine and the serial-DBSCAN engine; then row by row the log row, the
    control blocks and every per-particle array, bit for bit (the two batch engines over their whole capacity)."""
    B = len(singles)
    odoms = torch.as_tensor(np.stack([tr.odoms[t + 1] for tr in trajs]))
    codes = torch.as_tensor(np.stack([tr.codes[t + 1] for tr in trajs]))
    gts = torch.as_tensor(np.stack([tr.gt_poses[t + 1] for tr in trajs]))
    first = (B + 1) // 2
    for b in range(first):
        singles[b].step(odoms[b], codes[b], gt=gts[b], dbscan=dbscan)
    batched.step(odoms, codes, gts=gts, dbscan=dbscan)
    serial.step(odoms, codes, gts=gts, dbscan=dbscan)
    for b in range(first, B):
        singles[b].step(odoms[b], codes[b], gt=gts[b], dbscan=dbscan)
    slot = (batched.step_count - 1) % batched.log_frames
    assert _same_bits(batched._log[:, slot], serial._log[:, slot]), f"frame {t}: log rows, batched against serial passes"
    sa, sb = _state(batched), _state(serial)
    for k in sa:
        assert _same_bits(sa[k], sb[k]), f"frame {t}: {k}, batched against serial passes"
    views = []
    for b in range(B):
        assert _same_bits(batched._log[b, slot], singles[b]._log[slot]), f"frame {t}, trajectory {b}: log row"
        assert _same_bits(batched.ctl_i[b], singles[b].ctl_i) and _same_bits(batched.ctl_d[b], singles[b].ctl_d), f"frame {t}, trajectory {b}: control blocks"
        fs, fb = singles[b].frame_view(), batched.frame_view(b)
        assert (fb["n"], fb["n_after"]) == (fs["n"], fs["n_after"])
        for k in PER_PARTICLE:
            assert _same_bits(fb[k], fs[k]), f"frame {t}, trajectory {b}: {k}"
        assert np.array_equal(fb["cluster_poses"], fs["cluster_poses"]) and np.array_equal(fb["cluster_stds"], fs["cluster_stds"])
        views.append(fb)
    return views


def _build(dev, cb, B, cap, seed, single_kw=None, **kw):
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    wide = kw.pop("wide", False)
    singles = [LoopEngine(*src, cap, seed=seed + b, device=dev, **kw, **(single_kw or {})) for b in range(B)]
    batched = BatchLoopEngine(*src, B, cap, seed=seed, device=dev, wide=wide, **kw)
    serial = BatchLoopEngine(*src, B, cap, seed=seed, device=dev, wide=wide, batched_dbscan=False, **kw)
    assert batched.batched_dbscan and batched._args.dbscan_batched == 1 and not serial.batched_dbscan and serial._args.dbscan_batched == 0
    return singles, batched, serial


def test_engine_small_regime(dev, oracle, cb):
    """B = 5 from 6000, 6000, 4097, 4096 and 63 particles; DBSCAN on frames 0 (hashed rows 0 and 1: two clusters and noise), 3 and
    4 (back to back: the pass reuses its scratch).  The default engine takes the batched pass."""
    B, T, seed = len(STARTS), 6, 6100
    trajs = [_traj(cb, T, 2013 + b) for b in range(B)]
    starts = _blob_starts(cb, trajs)
    singles, batched, serial = _build(dev, cb, B, 6000, seed, floor=500)
    for s, p in zip(singles, starts):
        s.set_particles(torch.as_tensor(p))
    for e in (batched, serial):
        e.set_particles([torch.as_tensor(p) for p in starts])
    for t in range(T):
        dbscan = t in (0, 3, 4)
        views = _three_way_frame(singles, batched, serial, trajs, t, dbscan)
        if dbscan:
            for b, v in enumerate(views):
                X = v["poses_prop"][:, :3, 3].cpu().numpy()
                ref, ncl = oracle.dbscan(X, EPS, len(X) // 5)
                assert np.array_equal(v["labels_frame"].cpu().numpy(), ref) and v["ncl"] == ncl, f"frame {t}, trajectory {b}"
                if t == 0 and b < 2:
                    assert ncl >= 2 and (ref == -1).any() and cells_per_axis(X).max() > 128, (ncl, cells_per_axis(X))
    assert not batched.ctl_i[:, 14].any()


def test_engine_seeded(dev, cb):
    """The seeded batch (torch CPU streams, the ATen tie rule; FRONT | DBSCAN | ANNEAL, then RESAMPLE) through its DBSCAN frame."""
    B, seed = len(STARTS), 6200
    trajs = [_traj(cb, 2, 2013 + b) for b in range(B)]
    starts = _blob_starts(cb, trajs)
    singles, batched, serial = _build(dev, cb, B, 6000, seed, single_kw=dict(topk_ties="aten_cpu"), floor=500)
    for b, (s, p) in enumerate(zip(singles, starts)):
        s.set_particles(torch.as_tensor(p))
        s.seed_torch_stream(7300 + b)
    for e in (batched, serial):
        e.set_particles([torch.as_tensor(p) for p in starts])
        e.seed_torch_streams([7300 + b for b in range(B)])
    for t in range(2):
        _three_way_frame(singles, batched, serial, trajs, t, t == 0)
    assert not batched.ctl_i[:, 14].any() and not batched._mt_status.any()


def test_engine_wide(dev, cb):
    """wide=True, 3 x 20 000 (beyond the small-set regime: the radix selection per row) through a DBSCAN frame and a plain one."""
    B, N0, seed = 3, 20000, 6300
    trajs = [_traj(cb, 2, 2013 + b) for b in range(B)]
    rng = np.random.default_rng(43)
    starts = [_near(cb, trajs[b].gt_poses[0][:3, 3], 300, N0 - 3000 * b, rng) for b in range(B)]
    singles, batched, serial = _build(dev, cb, B, N0, seed, wide=True, floor=1000)
    for s, p in zip(singles, starts):
        s.set_particles(torch.as_tensor(p))
    for e in (batched, serial):
        e.set_particles([torch.as_tensor(p) for p in starts])
    for t in range(2):
        _three_way_frame(singles, batched, serial, trajs, t, t == 0)


def test_engine_beyond_the_bound_takes_the_serial_passes(dev, cb):
    """65 x 16 384 slots are more than the one set of cell tables holds for a batch: the default engine clusters row after row."""
    from midastouch_amd import BatchLoopEngine, ops
    B, cap, n = 65, 16384, 300
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=6400, device=dev)
    assert not eng.batched_dbscan and eng._args.dbscan_batched == 0
    tr = _traj(cb, 1, 2013)
    rng = np.random.default_rng(44)
    eng.set_particles([torch.as_tensor(_near(cb, tr.gt_poses[0][:3, 3], 100, n, rng)) for _ in range(B)])
    rep = lambda a: torch.as_tensor(a[1])[None].repeat(B, *([1] * a[1].ndim)).contiguous()  # noqa: E731
    eng.step(rep(tr.odoms), rep(tr.codes), gts=rep(tr.gt_poses), dbscan=True)
    for b in range(B):
        lab, info = ops.dbscan(eng.poses_prop[b, :n], EPS)
        assert torch.equal(eng._labels_prev[b, :n], lab) and eng.ctl_i[b, 10].item() == info[0].item(), b


def test_batched_dbscan_no_frame_allocates(dev):
    """8 x 16 384 through a batched DBSCAN frame and two plain ones: after the constructor MIDAS_SCRATCH_LOG reports no chunk.  (The
    switch is read once per process: a child process.)"""
    code = (
        "import sys, numpy as np, torch\n"
        "from midastouch_amd import BatchLoopEngine, _lib\n"
        "from midastouch_amd.synthetic import make_codebook, make_trajectory\n"
        "dev = torch.device('cuda', 0)\n"
        "B, cap = 8, _lib.LOOP_BATCH_MAX_CAP\n"
        "cb = make_codebook(K=3000, D=256, seed=1013, mesh_points=20000)\n"
        "tr = make_trajectory(cb, T=4, seed=2000)\n"
        "eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, cap, seed=4000, device=dev)\n"
        "assert eng.batched_dbscan\n"
        "sys.stderr.write('MARK\\n'); sys.stderr.flush()\n"
        "rng = np.random.default_rng(0)\n"
        "eng.set_particles(torch.as_tensor(cb.poses[rng.integers(0, 3000, (B, cap))]))\n"
        "for t in range(3):\n"
        "    rep = lambda a: torch.as_tensor(a[t + 1])[None].repeat(B, *([1] * a[t + 1].ndim)).contiguous()\n"
        "    eng.step(rep(tr.odoms), rep(tr.codes), gts=rep(tr.gt_poses))\n"
        "torch.cuda.synchronize()\n"
        "print('DONE', min(eng.n), max(eng.n))\n")
    env = dict(os.environ, MIDAS_SCRATCH_LOG="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DONE" in r.stdout
    before, after = r.stderr.split("MARK")
    assert "reserved one chunk" in before and "[midas] scratch" not in after, r.stderr
