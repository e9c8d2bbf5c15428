"""BatchLoopEngine(centers="logmap"): row b is bit for bit a LoopEngine(seed + b, centers="logmap", <row b's object and
parameters>) - the whole log row and every per-particle array, after every frame - in every regime the batch has: plain, the
three objects with per-row parameters, wide with rows above 16 384 beside a small one, 4095 / 4096 / 4097 particles, batched and
serial DBSCAN.  The comparisons are those of tests/test_gpu_batch_loop.py and tests/test_gpu_batch_loop_rows.py, whose helpers
pass the keyword to both sides."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_batch_loop as plain  # noqa: E402
import test_gpu_batch_loop_rows as per_row  # noqa: E402
from test_gpu_batch_loop import cb, dev  # noqa: E402,F401  (fixtures)
from test_gpu_batch_loop_objects import _near_starts, _trajs  # noqa: E402
from test_gpu_batch_loop_rows import cbs  # noqa: E402,F401  (fixture: the three objects, K = 3000 / 900 / 1777)

T = 6


def _logmap_frames_differ(views, batch):
    """The log-map form ran: a frame's centres are not the quaternion form's on the same frame."""
    from midastouch_amd import ops
    v = views[0]
    uniq = torch.unique(v["labels_frame"]).to(torch.int64)
    cq = ops.cluster_centers(v["poses_prop"], v["weights"], v["labels_frame"].to(torch.int64), uniq)[0].cpu().numpy()
    cl = ops.cluster_centers(v["poses_prop"], v["weights"], v["labels_frame"].to(torch.int64), uniq, method="logmap")[0].cpu().numpy()
    assert batch.centers == "logmap" and np.array_equal(v["cluster_poses"].view(np.int32), cl.view(np.int32))
    assert not np.array_equal(v["cluster_poses"], cq)


@pytest.mark.parametrize("batched", [None, False], ids=["batched_dbscan", "serial_dbscan"])
def test_plain(dev, oracle, cb, batched):
    B, N0, seed = 3, 3000, 4100
    trajs = [plain._traj(cb, T, 2013 + b) for b in range(B)]
    starts = [plain._wide_start(oracle, cb, trajs[b], N0, 11 + b) for b in range(B)]
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    singles = [LoopEngine(*src, N0, seed=seed + b, device=dev, cluster_every=3, centers="logmap") for b in range(B)]
    batch = BatchLoopEngine(*src, B, N0, seed=seed, device=dev, cluster_every=3, centers="logmap", batched_dbscan=batched)
    assert batch.batched_dbscan == (batched is None)
    plain._start(singles, batch, starts)
    modes = []
    for t in range(T):
        views = plain._frame(singles, batch, trajs, t)
        modes += [v["mode"] for v in views]
        if t == 1:
            _logmap_frames_differ(views, batch)
    assert any(modes)
    assert not batch.ctl_i[:, 14].any()


def test_objects_with_per_row_parameters(dev, cbs):
    rows, seed = [0, 1, 2, 0, 1, 2], 4100
    ns = [2000, 2200, 2900, 3600, 4300, 5000]
    trajs = _trajs(cbs, rows, T, 2013)
    starts = _near_starts(cbs, rows, trajs, 300, ns, 21)
    singles, batch = per_row._engines(dev, cbs, rows, 5000, seed, per_row.SIX, cluster_every=3, centers="logmap")
    assert batch.per_row == per_row.ROW_KEYS and all(s.centers == "logmap" for s in singles)
    per_row._start(singles, batch, starts, particle_vars=[1.0, 1.0, 1e-12, 1.0, 1e-12, 1.0], init=5000)
    for t in range(T):
        views = per_row._frame(singles, batch, trajs, t, unit=[False, True, False, True, False, False] if t == 4 else t == 5)
        if t == 0:
            assert [views[b]["mode"] for b in (0, 1, 2, 4)] == [1, 1, 2, 0]
        if t == 1:
            _logmap_frames_differ(views, batch)
    assert not batch.ctl_i[:, 14].any()


def test_wide_rows(dev, cbs):
    """Two rows held above 16 384 by floors of 16 400 and 16 420 (the decision with a launch of its own, one workgroup a row, in
    front of the radix select) beside a small row."""
    rows, cap, seed = [2, 0, 1], 16448, 61
    params = dict(sig_t=[2e-4, 1e-4, 2e-4], sig_r=[0.5, 0.5, 0.25], pen_max=[0.002, 0.003, 0.002], floor=[16400, 16420, 1000],
                  softmax=[True, True, False])
    trajs = _trajs(cbs, rows, T, 2070)
    starts = _near_starts(cbs, rows, trajs, 400, [cap, cap, 3000], 13)
    singles, batch = per_row._engines(dev, cbs, rows, cap, seed, params, cluster_every=2, wide=True, centers="logmap")
    per_row._start(singles, batch, starts, particle_vars=[1.0, 1.0, 1.0], init=cap)
    for t in range(T):
        views = per_row._frame(singles, batch, trajs, t, unit=[False, False, t == 1])
        if t == 0:
            assert [v["n_after"] for v in views[:2]] == [16400, 16420]
        if t == 1:
            _logmap_frames_differ(views, batch)
    assert all(v["n_after"] > 16384 for v in views[:2])


def test_block_edges(dev, cbs):
    rows, seed = [0, 1, 2], 97
    params = dict(sig_t=[2e-4, 1e-4, 3e-4], sig_r=[0.5, 0.25, 0.5], pen_max=[0.002, 0.0015, 0.003], floor=[4000, 1000, 4097],
                  softmax=[False, True, True])
    trajs = _trajs(cbs, rows, T, 2090)
    starts = _near_starts(cbs, rows, trajs, 300, [4095, 4096, 4097], 15)
    singles, batch = per_row._engines(dev, cbs, rows, 4097, seed, params, cluster_every=2, centers="logmap")
    per_row._start(singles, batch, starts)
    for t in range(T):
        views = per_row._frame(singles, batch, trajs, t, unit=[t == 1, False, t == 2])
        if t == 0:
            assert [v["n"] for v in views] == [4095, 4096, 4097]
