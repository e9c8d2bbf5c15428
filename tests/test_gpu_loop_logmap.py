"""LoopEngine(centers="logmap"): the frame's cluster centres are `ops.cluster_centers(method="logmap")` on the frame's own
propagated poses, masked weights and labels - bit for bit, for the merged weights-and-moments launch, the DBSCAN frames' separate
moment launch, the single-workgroup annealing and the multi-launch form above its limit - the annealing decision follows their
spreads exactly, the quaternion form is what an engine built without the keyword runs, and the phase bit is refused where it
selects nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_batch_loop import PER_PARTICLE, _traj, _wide_start, cb, dev  # noqa: E402,F401  (fixtures: the K = 3000 codebook)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _run(dev, oracle, cb, N0, T, dbscan_on, seeded=False, spare=0, **kw):
    """T frames of a LoopEngine(centers="logmap") from the wide start; after every frame the checks of the module docstring.
    -> the frames' (n, mode, k, clusters)."""
    from midastouch_amd import ops
    from midastouch_amd.loop_engine import LoopEngine
    traj = _traj(cb, T, 2013)
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0 + spare, seed=4100, device=dev, cluster_every=4, centers="logmap", **kw)
    assert eng.centers == "logmap"
    eng.set_particles(torch.as_tensor(_wide_start(oracle, cb, traj, N0, 11)))
    if seeded:
        eng.seed_torch_stream(7)
    ann = oracle.Annealer()
    out = []
    for t in range(T):
        eng.step(torch.as_tensor(traj.odoms[t + 1]), torch.as_tensor(traj.codes[t + 1]), gt=torch.as_tensor(traj.gt_poses[t + 1]),
                 dbscan=t in dbscan_on)
        fv = eng.frame_view()
        assert fv["err"] == 0, (t, fv["err"])
        n, pp, w, lab = fv["n"], fv["poses_prop"], fv["weights"], fv["labels_frame"]
        uniq = torch.unique(lab)
        c1, s1, cnt = ops.cluster_centers(pp, w, lab.to(torch.int64), uniq.to(torch.int64), method="logmap")
        got_c, got_s = fv["cluster_poses"], fv["cluster_stds"]
        assert got_c.shape == (len(uniq), 4, 4) and fv["clusters"] == len(uniq), (t, got_c.shape, uniq)
        assert np.array_equal(_bits(got_c), _bits(c1.cpu().numpy())), (t, got_c, c1)
        if not seeded:  # (the ATen tie rule takes the spreads once more, in two passes around the frame's centre: k_loop_std_two_pass)
            assert np.array_equal(_bits(got_s), _bits(s1.cpu().numpy())), (t, got_s, s1)
        else:
            np.testing.assert_allclose(got_s, s1.cpu().numpy(), rtol=1e-4, atol=1e-9)
        cq = ops.cluster_centers(pp, w, lab.to(torch.int64), uniq.to(torch.int64))[0].cpu().numpy()
        assert not np.array_equal(got_c, cq), t  # (not the quaternion form's centre)
        # annealing's decision from the device's own spreads
        var = oracle.cluster_var(got_s, "aten_cpu" if seeded else "running")
        assert np.float32(fv["var"]) == var, (t, fv["var"], var)
        mode, k = _decide(ann, n, var, eng.floor)
        assert (fv["mode"], fv["k"]) == (mode, k), (t, fv["mode"], fv["k"], mode, k)
        out.append((n, fv["mode"], fv["k"], fv["clusters"]))
    return out


def _decide(ann, n, var, floor):
    """oracle.Annealer's rule on a count alone: step() with n equal weights returns the surviving index set; mode and k from its size."""
    idx = ann.step(np.arange(n, dtype=np.float64), np.float32(var), floor)
    n2 = len(idx)
    return (0, 0) if n2 == n else (1, n - n2) if n2 < n else (2, n2 - n)


def test_small_set_frames(dev, oracle, cb):
    """3000 particles, K = 3000, 8 frames, DBSCAN on frames 0 and 4: the single-workgroup annealing, the merged weights-and-moments
    launch on the frames without DBSCAN and k_loop_cluster_moments_logmap behind DBSCAN."""
    out = _run(dev, oracle, cb, 3000, 8, (0, 4))
    assert any(m != 0 for _, m, _, _ in out), out  # annealing acted


def test_capacity_beyond_the_set(dev, oracle, cb):
    """777 slots nobody has written behind the 3000 particles: zero matrices, whose logarithm is NaN - the lanes that read them
    in the merged launch must not reach the sums (0 x NaN)."""
    _run(dev, oracle, cb, 3000, 3, (0,), spare=777)


def test_multi_launch_form(dev, oracle, cb):
    """Above the single-workgroup limit (16 384): k_loop_decide launched with one workgroup, then the radix select."""
    out = _run(dev, oracle, cb, 20000, 4, (0,))
    assert out[0][0] == 20000 and any(m != 0 for _, m, _, _ in out), out


def test_seeded_frames(dev, oracle, cb):
    """seed_torch_stream with topk_ties="aten_cpu": the split frame and the decision with a launch of its own."""
    _run(dev, oracle, cb, 3000, 5, (0, 4), seeded=True, topk_ties="aten_cpu")


def test_quat_avg_is_the_engine_without_the_keyword(dev, oracle, cb):
    from midastouch_amd.loop_engine import LoopEngine
    T, N0 = 6, 3000
    traj = _traj(cb, T, 2013)
    start = torch.as_tensor(_wide_start(oracle, cb, traj, N0, 11))
    engs = [LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0, seed=4100, device=dev, cluster_every=4, **kw)
            for kw in ({}, {"centers": "quat_avg"})]
    for e in engs:
        e.set_particles(start)
    for t in range(T):
        views = []
        for e in engs:
            e.step(torch.as_tensor(traj.odoms[t + 1]), torch.as_tensor(traj.codes[t + 1]), gt=torch.as_tensor(traj.gt_poses[t + 1]))
            views.append(e.frame_view())
        slot = (engs[0].step_count - 1) % engs[0].log_frames
        assert torch.equal(engs[0]._log[slot].view(torch.int64), engs[1]._log[slot].view(torch.int64)), t
        for k in PER_PARTICLE:
            assert torch.equal(views[0][k], views[1][k]), (t, k)
        assert np.array_equal(_bits(views[0]["cluster_poses"]), _bits(views[1]["cluster_poses"]))


def _state(eng):
    return [getattr(eng, attr).clone() for attr, *_ in eng._state]


def test_refusals(dev, oracle, cb):
    """The bit without MIDAS_LOOP_ANNEAL - at the engine's step(phases=) and at the entry - and an unknown `centers`: refused before
    any launch, the engine's state as it was."""
    from midastouch_amd import _lib
    from midastouch_amd._lib import MidasError
    from midastouch_amd.loop_engine import LoopEngine
    traj = _traj(cb, 2, 2013)
    with pytest.raises(MidasError, match="centers"):
        LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, 3000, device=dev, centers="mean")
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, 3000, seed=4100, device=dev, centers="logmap")
    eng.set_particles(torch.as_tensor(_wide_start(oracle, cb, traj, 3000, 11)))
    eng.step(torch.as_tensor(traj.odoms[1]), torch.as_tensor(traj.codes[1]))
    torch.cuda.synchronize()
    before, count = _state(eng), eng.step_count
    for phases in (_lib.LOOP_CENTERS_LOGMAP, _lib.LOOP_FRONT | _lib.LOOP_CENTERS_LOGMAP,
                   _lib.LOOP_FRONT | _lib.LOOP_DBSCAN | _lib.LOOP_RESAMPLE | _lib.LOOP_CENTERS_LOGMAP, 32 | _lib.LOOP_ANNEAL):
        # at the entry, with the engine's own argument record
        rc = eng.ctx.lib.midas_loop_step(eng.ctx.h, eng.codebook.h, eng.tree6.h, eng.tree3.h, C.byref(eng._args), int(phases))
        assert rc == -1, (phases, rc)  # MIDAS_ERR_INVALID
    with pytest.raises(MidasError):  # at the engine
        eng.step(torch.as_tensor(traj.odoms[2]), torch.as_tensor(traj.codes[2]), phases=_lib.LOOP_FRONT | _lib.LOOP_CENTERS_LOGMAP)
    torch.cuda.synchronize()
    after = _state(eng)
    assert eng.step_count == count
    for (attr, *_), a, b in zip(eng._state, before, after):
        if attr in ("telemetry",):
            continue
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), attr
