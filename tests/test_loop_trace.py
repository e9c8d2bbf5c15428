"""The fused-step specs against traces of the reference's loop body.

* `OracleFilter.step` - the formulation every engine test compares the kernels with (exp(x - 1) shift, CDF from
  e * mask with blocked sums) - against G10 (T = 24, N = 256, the reference's own compose, teacher-forced per frame) and
  G10b (T = 64, N = 4096, free-running): NN exact, resample indices exact, weights 1e-12.
* `OracleLoop.step` - the same plus DBSCAN / cluster centres / annealing / variable particle count - against G13
  (T = 64, N0 = 4096): N per frame, kept lists, DBSCAN labels, resample indices exact.
* Both on ONE torch stream across guard frames - against G14 (T = 16, N0 = 2048, `torch.manual_seed(777)` once): the reference's
  resampler returns before it draws when every particle was pruned or the weights hold a NaN (particle_filter.py:237-241), so the
  stream stands still on such a frame and every later frame depends on the replay knowing that.
Fixtures: tools/gen_trace_golden.py, tools/gen_loop_trace.py, tools/gen_guard_trace.py (the real reference functions)."""
import numpy as np
import pytest
import torch

from _recipes import guard_trace_inputs, sha


def _check_digest(g, key, a):
    a = np.ascontiguousarray(a)
    assert np.array_equal(a[:32], g[key + "_head"]) and np.array_equal(a[-32:], g[key + "_tail"]), key
    assert sha(a) == str(g[key + "_sha"]), key


def _close_digest(g, key, a, rtol):
    np.testing.assert_allclose(a[:32], g[key + "_head"], rtol=rtol, atol=0, err_msg=key)
    np.testing.assert_allclose(a[-32:], g[key + "_tail"], rtol=rtol, atol=0, err_msg=key)


def _draws(t, N):
    torch.manual_seed(3000 + t)
    tn = torch.normal(mean=0.0, std=2e-4, size=(N, 3)).numpy()
    rot = torch.normal(mean=0.0, std=0.5, size=(N, 3)).numpy()
    return tn, rot


def test_oracle_filter_step_vs_g10_trace(golden, oracle):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    g = golden("g10_trace")
    cb = make_codebook(K=1200, D=256, seed=1000, mesh_points=20000)
    traj = make_trajectory(cb, T=25, seed=2000)
    f = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    N, T = int(g["N"]), int(g["T"])
    poses = g["poses0"]
    for t in range(1, T + 1):
        tn, rot = _draws(t, N)
        u = torch.rand(N, dtype=torch.float64).numpy()
        r = f.step(poses, traj.odoms[t], traj.codes[t], tn, rot, u=u)
        np.testing.assert_allclose(r["poses_prop"], g[f"prop_{t}"], rtol=0, atol=2e-6)
        # from the reference's own propagated poses on (teacher forcing: a float32 ulp must not cascade)
        r = f.step(poses, traj.odoms[t], traj.codes[t], tn, rot, u=u, prop_override=g[f"prop_{t}"])
        assert np.array_equal(r["nn_idx"], g[f"nn_{t}"]), t
        np.testing.assert_allclose(r["weights_pre"], g[f"wsim_{t}"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(r["weights"], g[f"wprune_{t}"], rtol=1e-12, atol=0)
        assert np.array_equal(r["weights"] == 0, g[f"wprune_{t}"] == 0)
        assert r["drifted"] == bool(g[f"drifted_{t}"])
        assert np.array_equal(r["ridx"], g[f"ridx_{t}"]), f"frame {t}"
        poses = g[f"prop_{t}"][g[f"ridx_{t}"]]


def test_oracle_filter_step_vs_g10b_trace64(golden, oracle):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    g = golden("g10b_trace64")
    cb = make_codebook(K=int(g["K"]), D=int(g["D"]), seed=int(g["cb_seed"]), mesh_points=20000)
    assert sha(cb.embeddings.astype(np.float32)) == str(g["cb_sha"])
    traj = make_trajectory(cb, T=int(g["T"]) + 1, seed=int(g["traj_seed"]))
    f = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    N = int(g["N0"])
    poses = g["poses0"]
    for t in range(1, int(g["T"]) + 1):
        tn, rot = _draws(t, N)
        u = torch.rand(N, dtype=torch.float64).numpy()
        r = f.step(poses, traj.odoms[t], traj.codes[t], tn, rot, u=u)
        _check_digest(g, f"nn_{t}", r["nn_idx"])
        _close_digest(g, f"wsim_{t}", r["weights_pre"], 1e-12)
        _close_digest(g, f"wprune_{t}", r["weights"], 1e-12)
        _check_digest(g, f"ridx_{t}", r["ridx"])
        rt, rr = oracle.particle_rmse(r["poses_prop"], traj.gt_poses[t])
        assert rt == pytest.approx(float(g[f"rmse_{t}"][0]), rel=1e-5)
        # (golden of the reference: torch's trace order, amplified by acos near 1 - hence the 0.03 deg)
        assert rr == pytest.approx(float(g[f"rmse_{t}"][1]), rel=1e-4, abs=0.03)
        poses = r["poses"]


def test_oracle_loop_vs_g13_trace(golden, oracle):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    g = golden("g13_loop_trace")
    cb = make_codebook(K=int(g["K"]), D=int(g["D"]), seed=int(g["cb_seed"]), mesh_points=20000)
    traj = make_trajectory(cb, T=int(g["T"]) + 1, seed=int(g["traj_seed"]))
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices)
    poses, labels = g["poses0"], np.zeros(int(g["N0"]), dtype=np.int64)
    n_tie = 0
    for t in range(1, int(g["T"]) + 1):
        N = poses.shape[0]
        assert N == int(g[f"N_{t}"]), t
        tn, rot = _draws(t, N)
        tie = bool(g[f"tie_{t}"])
        n_tie += tie
        # on a tie frame (torch.topk's choice among equal weights: implementation-defined) follow the reference's list
        r = loop.step(poses, labels, traj.odoms[t], traj.codes[t], tn, rot, gt=traj.gt_poses[t],
                      draws=lambda n: torch.rand(n, dtype=torch.float64).numpy(),
                      keep_override=g[f"keep_{t}"] if tie else None)
        _check_digest(g, f"nn_{t}", r["nn_idx"])
        _close_digest(g, f"wprune_{t}", r["weights"], 1e-12)
        assert r["drifted"] == bool(g[f"drifted_{t}"])
        if f"dbscan_{t}_sha" in g.files:
            _check_digest(g, f"dbscan_{t}", r["labels_frame"].astype(np.int32))
        assert np.array_equal(r["cluster_labels"], g[f"cl_labels_{t}"])
        assert r["var"] == np.float32(g[f"var_{t}"])
        _check_digest(g, f"keep_{t}", r["keep"])
        assert r["N"] == int(g[f"N2_{t}"])
        _check_digest(g, f"ridx_{t}", r["ridx"])
        assert r["rmse"][0] == pytest.approx(float(g[f"rmse_{t}"][0]), rel=1e-5)
        poses, labels = r["poses"], r["labels"]
    assert n_tie < int(g["T"])  # some frames are decided without ties


def _stream_draws(N):
    """add_noise_to_odom's draws from the stream as it stands (no reseed)."""
    tn = torch.normal(mean=0.0, std=2e-4, size=(N, 3)).numpy()
    rot = torch.normal(mean=0.0, std=0.5, size=(N, 3)).numpy()
    return tn, rot


def _rand64(n):
    return torch.rand(n, dtype=torch.float64).numpy()


def test_oracle_loop_vs_g14_guard_trace_one_stream(golden, oracle):
    """OracleLoop (ATen's tie rule) on one continuous torch stream through the drift frame: every particle pruned, annealing still
    acts on the all-zero weights (a fully tied top-k), the resampler draws nothing - and the ten frames behind it hold the
    reference's kept sets, resample indices and particle counts only if the replay drew nothing either."""
    g = golden("g14_guard_trace")
    cb, odoms, codes, gts = guard_trace_inputs(g, "loop")
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, floor=int(g["floor"]), cluster_every=int(g["cluster_every"]),
                             ties="aten_cpu")
    poses, labels = g["poses0"], np.zeros(int(g["N0"]), dtype=np.int64)
    torch.manual_seed(int(g["stream_seed"]))
    guards = 0
    for t in range(1, int(g["T"]) + 1):
        N = poses.shape[0]
        assert N == int(g[f"loop_N_{t}"]), f"frame {t}"
        tn, rot = _stream_draws(N)
        r = loop.step(poses, labels, odoms[t], codes[t], tn, rot, gt=gts[t], draws=_rand64)
        _check_digest(g, f"loop_nn_{t}", r["nn_idx"])
        _close_digest(g, f"loop_wprune_{t}", r["weights"], 1e-12)
        assert r["drifted"] == bool(g[f"loop_drifted_{t}"]), f"frame {t}"
        if f"loop_dbscan_{t}_sha" in g.files:
            _check_digest(g, f"loop_dbscan_{t}", r["labels_frame"].astype(np.int32))
        assert np.array_equal(r["cluster_labels"], g[f"loop_cl_labels_{t}"]), f"frame {t}"
        assert r["var"] == np.float32(g[f"loop_var_{t}"]), f"frame {t}"
        _check_digest(g, f"loop_keep_{t}", r["keep"])
        assert r["N"] == int(g[f"loop_N2_{t}"]), f"frame {t}"
        _check_digest(g, f"loop_ridx_{t}", r["ridx"])
        assert (r["status"] != 0) == (not bool(g[f"loop_consumed_{t}"])), f"frame {t}"
        assert r["rmse"][0] == pytest.approx(float(g[f"loop_rmse_{t}"][0]), rel=1e-5)
        guards += r["status"] != 0
        poses, labels = r["poses"], r["labels"]
    assert guards == 1 and bool(g[f"loop_drifted_{int(g['shift_frame'])}"])
    assert np.array_equal(_rand64(8), g["loop_tail_u"])  # the stream ends where the reference's does


def test_oracle_filter_vs_g14_guard_trace_one_stream(golden, oracle):
    """OracleFilter (fixed N) on one continuous torch stream through a drift frame (status 1) and a NaN-code frame (status 2): neither
    consumes a uniform, and the frames behind each hold the reference's resample indices."""
    g = golden("g14_guard_trace")
    cb, odoms, codes, gts = guard_trace_inputs(g, "fixed")
    f = oracle.OracleFilter(cb.poses, cb.embeddings, cb.mesh_vertices)
    poses = g["poses0"]
    N = int(g["N0"])
    torch.manual_seed(int(g["stream_seed"]))
    seen = []
    for t in range(1, int(g["T"]) + 1):
        assert N == int(g[f"fixed_N_{t}"]) == int(g[f"fixed_N2_{t}"])
        tn, rot = _stream_draws(N)
        r = f.step(poses, odoms[t], codes[t], tn, rot, draws=_rand64)
        _check_digest(g, f"fixed_nn_{t}", r["nn_idx"])
        _close_digest(g, f"fixed_wprune_{t}", r["weights"], 1e-12)
        assert r["drifted"] == bool(g[f"fixed_drifted_{t}"]), f"frame {t}"
        _check_digest(g, f"fixed_ridx_{t}", r["ridx"])
        assert (r["status"] != 0) == (not bool(g[f"fixed_consumed_{t}"])), f"frame {t}"
        if r["status"]:
            seen.append((t, r["status"]))
        # filter.py:176-179: a set that drifted as a whole goes on from the codebook poses nearest to it
        prop = cb.poses[r["nn_idx"]] if r["drifted"] else r["poses_prop"]
        rt, rr = oracle.particle_rmse(r["poses_prop"], gts[t])
        assert rt == pytest.approx(float(g[f"fixed_rmse_{t}"][0]), rel=1e-5)
        assert rr == pytest.approx(float(g[f"fixed_rmse_{t}"][1]), rel=1e-4, abs=0.03)  # (golden: torch's trace order)
        poses = prop[r["ridx"]]
    assert seen == [(int(g["shift_frame"]), 1), (int(g["nan_frame"]), 2)]
    assert np.array_equal(_rand64(8), g["fixed_tail_u"])


def test_cluster_var_is_torch_mean(oracle):
    """`var` of a replay of the reference (ties="aten_cpu"; filter.py:189) is torch.mean of the float32 (C, 3) cluster spreads on the
    CPU: ATen's sum in its own order (oracle.aten_sum_f32), not the running sum of the loop with ties by index - for every cluster count the frame's arrays hold (1 .. 64; the scalar row sum below 8
    values, whole vectors, leftover vectors and a tail above), at the magnitudes of a spread.  The running sum is shown to differ."""
    torch.set_num_threads(1)
    rng = np.random.default_rng(14)
    running_differs = 0
    for C in range(1, 65):
        for _ in range(40):
            stds = (rng.random((C, 3)) * 1e-2).astype(np.float32)
            want = np.float32(torch.mean(torch.tensor(stds)).item())
            assert oracle.cluster_var(stds, "aten_cpu") == want, \
                f"{C} clusters: oracle.aten_sum_f32 restates the 8-lane (AVX2) build of ATen's CPU sum kernel, the one x86 builds of " \
                f"torch dispatch to; this host's torch ({torch.backends.cpu.get_cpu_capability()}) adds in another order"
            running_differs += oracle.cluster_var(stds) != want
    assert running_differs > 100
