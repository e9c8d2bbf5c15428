"""Seeded loops across guard frames: the reference's resampler returns its input BEFORE it draws when the weights are all zero or
hold a NaN (modules/particle_filter.py:237-241), so torch's generator stands still on such a frame.  The engines' streams have to
do the same (ctl_i[LOOP_I_NDRAW], written ahead of the counted draw) or every later frame leaves the reference's particles.
Against G14 (tools/gen_guard_trace.py: the real reference functions on ONE torch stream, a drift frame and a NaN frame), for
LoopEngine, BatchLoopEngine (the skip is per row) and the runner's draws="host" / "seeded"; device (Philox) draws keep their bits."""
import numpy as np
import pytest

from _recipes import guard_trace_inputs, sha

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PER_PARTICLE = ("poses_prop", "nn_idx", "valid", "weights", "labels_frame", "src", "ridx", "poses", "weights_res", "labels", "hint")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_guard_trace")


@pytest.fixture(scope="module")
def inputs(g14):
    """trace -> (codebook, odoms, codes, gts) as tensors' sources; the codebook is built once."""
    return {trace: guard_trace_inputs(g14, trace) for trace in ("loop", "fixed", "plain")}


def _t(a):
    return torch.as_tensor(a)


def _close(g, key, a):
    np.testing.assert_allclose(a[:32], g[key + "_head"], rtol=1e-12, atol=0, err_msg=key)
    np.testing.assert_allclose(a[-32:], g[key + "_tail"], rtol=1e-12, atol=0, err_msg=key)


def _check_frame(g, tr, t, fv, cluster, var_miss):
    """One completed frame (a frame_view) against trace `tr` of the fixture.  A `var` that is not the fixture's float32 goes to
    `var_miss` and the caller asserts the list empty at its end, so that the frames behind it are still compared."""
    from midastouch_amd import _lib
    k = f"{tr}_"
    assert fv["n"] == int(g[k + f"N_{t}"]) and fv["n_after"] == int(g[k + f"N2_{t}"]), (tr, t, fv["n"], fv["n_after"])
    assert sha(fv["nn_idx"].cpu().numpy().astype(np.int32)) == str(g[k + f"nn_{t}_sha"]), f"{tr} frame {t}: NN"
    _close(g, k + f"wprune_{t}", fv["weights"].cpu().numpy())
    assert fv["drifted"] == bool(g[k + f"drifted_{t}"]), (tr, t)
    consumed = bool(g[k + f"consumed_{t}"])
    assert (fv["status"] != 0) == (not consumed), f"{tr} frame {t}: status {fv['status']}"
    assert int(fv["ctl_i"][_lib.LOOP_I_NDRAW]) == (fv["n_after"] if consumed else 0), f"{tr} frame {t}: NDRAW"
    assert fv["err"] == 0, (tr, t, fv["err"])
    if cluster:
        if k + f"dbscan_{t}_sha" in g.files:
            assert sha(fv["labels_frame"].cpu().numpy().astype(np.int32)) == str(g[k + f"dbscan_{t}_sha"]), f"{tr} frame {t}: DBSCAN labels"
        assert fv["clusters"] == len(g[k + f"cl_labels_{t}"]), (tr, t)
        if np.float32(fv["var"]) != np.float32(g[k + f"var_{t}"]):
            var_miss.append((tr, t, float(np.float32(fv["var"])), float(np.float32(g[k + f"var_{t}"])), fv["cluster_stds"].tolist()))
        assert sha(fv["src"].cpu().numpy().astype(np.int32)) == str(g[k + f"keep_{t}_sha"]), f"{tr} frame {t}: kept set is not the reference's"
    else:
        assert torch.equal(fv["src"].cpu(), torch.arange(fv["n"], dtype=torch.int32)), (tr, t)
    assert sha(fv["ridx"].cpu().numpy().astype(np.int32)) == str(g[k + f"ridx_{t}_sha"]), f"{tr} frame {t}: resample indices are not the reference's"


def _loop_engine(dev, g, cb, cluster, **kw):
    from midastouch_amd.loop_engine import LoopEngine
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, int(g["N0"]), floor=int(g["floor"]), cluster=cluster,
                     cluster_every=int(g["cluster_every"]), log_frames=64, device=dev, **kw)
    eng.set_particles(_t(g["poses0"]))
    return eng


@pytest.mark.parametrize("tr", ["loop", "fixed"])
def test_seeded_loop_engine_holds_the_reference_across_guard_frames(dev, g14, inputs, tr):
    """seed_torch_stream(777) once, one step() a frame, nothing teacher-forced: every frame of the trace - the drift frame (status 1;
    in the loop trace annealing duplicates on its fully tied weights), in the fixed trace the NaN frame (status 2), and the frames
    behind them - and the stream ends where the reference's does."""
    g = g14
    cb, odoms, codes, gts = inputs[tr]
    cluster = tr == "loop"
    eng = _loop_engine(dev, g, cb, cluster, topk_ties="aten_cpu")
    st = eng.seed_torch_stream(int(g["stream_seed"]))
    seen, var_miss = [], []
    for t in range(1, int(g["T"]) + 1):
        eng.step(_t(odoms[t]), _t(codes[t]), gt=_t(gts[t]))
        fv = eng.frame_view()
        _check_frame(g, tr, t, fv, cluster, var_miss)
        if fv["status"]:
            seen.append((t, fv["status"], fv["mode"] != 0))
    want = [(int(g["shift_frame"]), 1, cluster)] + ([] if cluster else [(int(g["nan_frame"]), 2, False)])
    assert seen == want, seen
    assert not eng._mt_status.any()
    eng.read_log()  # (strict: no frame raised a condition)
    gen = torch.Generator()
    st.to_host(gen)
    assert np.array_equal(torch.rand(8, dtype=torch.float64, generator=gen).numpy(), g[f"{tr}_tail_u"]), "the stream is not where the reference's ends"
    assert not var_miss, f"var is not the reference's float32 in {len(var_miss)} frame(s): {var_miss}"


def test_seeded_batch_skips_the_draw_per_row(dev, g14, inputs):
    """B = 3 under seeds (777, 778, 777): rows 0 and 2 run the jump and hold the fixture in every frame; row 1 runs the plain
    trajectory and holds a seeded LoopEngine(778)'s bits - log rows, arrays, the state row of its stream: a guard frame in one row
    moves nobody else's stream."""
    from midastouch_amd import BatchLoopEngine, _lib
    g = g14
    cb, odoms, codes, gts = inputs["loop"]
    plain = inputs["plain"][1]
    B, N0, seeds = 3, int(g["N0"]), [int(g["stream_seed"]), int(g["stream_seed"]) + 1, int(g["stream_seed"])]
    batch = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, floor=int(g["floor"]), cluster_every=int(g["cluster_every"]),
                            log_frames=64, device=dev)
    batch.set_particles([_t(g["poses0"])] * B)
    streams = batch.seed_torch_streams(seeds)
    single = _loop_engine(dev, g, cb, True, topk_ties="aten_cpu")
    single.seed_torch_stream(seeds[1])
    shift_t, var_miss = int(g["shift_frame"]), []
    for t in range(1, int(g["T"]) + 1):
        od = torch.stack([_t(odoms[t]), _t(plain[t]), _t(odoms[t])])
        batch.step(od, _t(codes[t])[None].repeat(B, 1).contiguous(), gts=_t(gts[t])[None].repeat(B, 1, 1).contiguous())
        single.step(_t(plain[t]), _t(codes[t]), gt=_t(gts[t]))
        for b in (0, 2):
            _check_frame(g, "loop", t, batch.frame_view(b), True, var_miss)
        slot = (batch.step_count - 1) % batch.log_frames
        assert torch.equal(batch._log[1, slot].view(torch.int64), single._log[slot].view(torch.int64)), f"frame {t}: row 1's log row"
        fs, fb = single.frame_view(), batch.frame_view(1)
        assert fs["status"] == 0 and not fs["drifted"]
        for k in PER_PARTICLE:
            assert fb[k].shape == fs[k].shape and torch.equal(fb[k], fs[k]), f"frame {t}, row 1: {k}"
        if t == shift_t:
            assert int(fb["ctl_i"][_lib.LOOP_I_NDRAW]) == fb["n_after"]
            assert int(batch.ctl_i[0, _lib.LOOP_I_NDRAW]) == 0 == int(batch.ctl_i[2, _lib.LOOP_I_NDRAW])
    assert not batch.ctl_i[:, _lib.LOOP_I_ERR].any() and not batch._mt_status.any()
    for b in (0, 2):
        gen = torch.Generator()
        streams.to_host(b, gen)
        assert np.array_equal(torch.rand(8, dtype=torch.float64, generator=gen).numpy(), g["loop_tail_u"]), f"row {b}: stream position"
    streams.to_host(1, torch.Generator())
    single.torch_stream.to_host(torch.Generator())
    assert torch.equal(streams.state[1], single.torch_stream.state), "row 1's stream state"
    assert not torch.equal(streams.state[1], streams.state[0])
    assert not var_miss, f"var is not the reference's float32 in {len(var_miss)} (row, frame)s: {var_miss}"


def test_device_draws_through_the_drift_frame_equal_the_oracle(dev, g14, inputs, oracle):
    """Philox draws (no stream, ties by index): the launches and the bits are what they were - every field
    tests/test_gpu_loop.py::_compare_frame holds a frame to (propagated poses, NN, mask, weights, DBSCAN labels, clusters, var,
    centres, spreads, annealed set, status, resample indices, resampled set, labels) against OracleLoop through the drift frame and
    the frames behind it, and the NDRAW word is never written.
    One pinned difference, on the drift frame only: every particle sits on a codebook pose there, a cluster's members coincide
    and its spread is exactly 0 in the spec's two-pass form; this mode keeps the closed form on the moments (S_tt - 2 m S_t + m^2
    S_w, whose cancellation error is a few float64 steps of mean(t^2) <= 0.01 m^2, i.e. < 1e-16 m^2, a spread below 1e-8 m) and so
    leaves up to 1e-8 where 0 belongs.  That frame's spreads are held to 1e-8 absolute and its `var` to one float32 step of the
    oracle's; the replay mode (ties="aten_cpu") computes them in two passes and is held exactly, above.  DESIGN.md section 7."""
    from midastouch_amd import _lib
    from test_gpu_loop import _compare_frame
    g = g14
    cb, odoms, codes, gts = inputs["loop"]
    seed, every = 4100, int(g["cluster_every"])
    eng = _loop_engine(dev, g, cb, True, seed=seed)
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, floor=int(g["floor"]), cluster_every=every)
    poses, labels = g["poses0"], np.zeros(int(g["N0"]), dtype=np.int64)
    drifted = []
    for t in range(10):
        n = poses.shape[0]
        tn, rot = oracle.philox_noise(n, seed, t, np.float32(2e-4), np.float32(0.5))
        ref = loop.step(poses, labels, odoms[t + 1], codes[t + 1], tn, rot, draws=lambda m: oracle.philox_uniform64(m, seed, t))
        eng.step(_t(odoms[t + 1]), _t(codes[t + 1]), gt=_t(gts[t + 1]))
        fv = eng.frame_view()
        if ref["drifted"]:  # the pinned difference: then the frame is compared with the device's own spreads and var in their place
            np.testing.assert_allclose(fv["cluster_stds"], ref["cluster_stds"][:8], rtol=1e-5, atol=1e-8)
            assert abs(np.float32(fv["var"]) - ref["var"]) <= np.spacing(ref["var"]), (fv["var"], ref["var"])
            ref = dict(ref, var=np.float32(fv["var"]), cluster_stds=fv["cluster_stds"])
        _compare_frame(fv, ref, t, t % every == 0)
        assert int(fv["ctl_i"][_lib.LOOP_I_NDRAW]) == 0 and fv["err"] == 0
        drifted.append(ref["drifted"])
        poses, labels = ref["poses"], ref["labels"]
    assert drifted == [t + 1 == int(g["shift_frame"]) for t in range(10)]


# ---- var and the spreads of the replay mode, 1 .. 64 cluster rows ------------------------------------------------------------
@pytest.mark.parametrize("rows,noise", [(1, False), (2, True), (3, False), (5, True), (6, False), (10, True), (11, False), (16, True),
                                        (21, False), (22, True), (43, False), (64, True)])
def test_replay_mode_var_and_spreads_many_clusters(dev, g14, inputs, oracle, rows, noise):
    """topk_ties="aten_cpu" with forced labels, `rows` cluster rows present (with `noise` one of them is label -1): 3, 6 .. 192
    spreads, so that the device's restatement of ATen's sum (aten_sum_f32) runs its scalar row sum (< 8 values), whole vectors with
    and without leftover vectors and a scalar tail, and the four-accumulator groups (>= 32 values); k_loop_std_two_pass runs with
    non-flat weights in every cluster, one cluster whose members coincide (spread exactly 0) and one whose weights are all 0 (flat).
    `var` is bit for bit oracle.cluster_var of the device's own spreads in ATen's order; the spreads are oracle.cluster_centers' to
    one float32 step (two float64 sums of the same terms in different orders differ by ~n 2^-53 relative: they round to the same
    float32 or, on a boundary, to neighbours), and where they are the same bits `var` is the oracle's."""
    from midastouch_amd.loop_engine import LoopEngine
    g = g14
    cb, odoms, codes, gts = inputs["plain"]
    n = 2048
    rng = np.random.default_rng(100 + rows)
    poses = cb.poses[rng.integers(0, cb.poses.shape[0], n)].copy()
    labels = (np.arange(n) % rows).astype(np.int64) - (1 if noise else 0)
    rng.shuffle(labels)
    last = labels.max()
    poses[labels == last] = poses[np.nonzero(labels == last)[0][0]]  # a cluster whose members coincide
    if rows >= 3:
        poses[labels == last - 1, :3, 3] += np.float32(0.5)           # a cluster off the mesh: all pruned, weights all 0 (flat)
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, n, floor=500, sig_t=0.0, sig_r=0.0, log_frames=8, device=dev,
                     topk_ties="aten_cpu")
    eng.set_particles(_t(poses), _t(labels))
    eng.step(torch.eye(4), _t(codes[1]), gt=_t(gts[1]), dbscan=False)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (more than 8 rows: the LOG row keeps the first 8 centres and says so; the engine's arrays hold all)
        fv = eng.frame_view()
    assert fv["err"] & ~8 == 0 and fv["clusters"] == rows and not fv["drifted"]
    w = fv["weights"].cpu().numpy()
    prop = fv["poses_prop"].cpu().numpy()
    uniq, _, stds = oracle.cluster_centers(prop, w, labels)
    assert len(uniq) == rows
    dev_stds = eng._cl_stds[:rows].cpu().numpy()
    assert np.all(np.abs(dev_stds - stds) <= np.spacing(np.maximum(dev_stds, stds))), np.abs(dev_stds - stds).max()
    assert np.array_equal(dev_stds[-1], np.zeros(3, np.float32)) and np.array_equal(stds[-1], np.zeros(3, np.float32))
    assert np.float32(fv["var"]) == oracle.cluster_var(dev_stds, "aten_cpu"), (fv["var"], oracle.cluster_var(dev_stds, "aten_cpu"))
    if np.array_equal(dev_stds, stds):
        assert np.float32(fv["var"]) == oracle.cluster_var(stds, "aten_cpu")
    if rows > 1:
        assert (w[labels == uniq[0]] > 0).any() and len(np.unique(w[labels == uniq[0]])) > 1  # (non-flat weights)
    if rows >= 3:
        assert not w[labels == last - 1].any() and stds[-2].max() > 0


# ---- the runner ---------------------------------------------------------------------------------------------------------
RUN_N, RUN_T, RUN_JUMP, RUN_FLOOR = 2048, 12, 6, 500


def _same(x, y):
    if isinstance(x, np.ndarray):
        return x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    return x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y))


def test_runner_host_and_seeded_draws_agree_across_a_jump(dev):
    """filter(draws="host") and filter(draws="seeded") over a sequence whose measured poses jump 0.5 m off the object at one frame:
    equal records, an equal generator state behind the run - and that state is the one a generator reaches by drawing what the log
    says the reference drew: init_filter on the initial frames, per moving frame normal (n, 3) twice, then rand(n_after) only where
    the frame's status is 0."""
    from midastouch_amd.config import load_config
    from midastouch_amd.filter import filter as run_filter
    from midastouch_amd.filter import synthetic_sequence
    from midastouch_amd.particle_filter import particle_filter
    cfg = load_config([f"expt.params.num_particles={RUN_N}", "expt.codebook_size=2500"])
    seq = synthetic_sequence(cfg, dev, T=RUN_T)
    seq.meas_p[RUN_JUMP:, :3, 3] += 0.5  # one odometry step with the jump; the steps behind it are unchanged
    runs, states = {}, {}
    for draws in ("host", "seeded"):
        torch.manual_seed(77)
        runs[draws] = run_filter(cfg, seq=seq, device=dev, draws=draws, floor=RUN_FLOOR)
        states[draws] = torch.get_rng_state()
    a, b = runs["host"], runs["seeded"]
    assert len(a["frames"]) == len(b["frames"]) == RUN_T
    for ra, rb in zip(a["frames"], b["frames"]):
        assert ra.keys() == rb.keys()
        for k in ra:
            assert _same(ra[k], rb[k]), (ra["frame"], k)
    guard = [i for i, r in enumerate(a["frames"]) if r["status"] != 0]
    assert guard == [RUN_JUMP] and a["frames"][RUN_JUMP]["drifted"], [(r["frame"], r["status"], r["kept"]) for r in a["frames"]]
    assert len(a["frames"]) - 1 - RUN_JUMP >= 3
    assert torch.equal(states["host"], states["seeded"]), "torch's generator does not stand where the host-draw run leaves it"
    # the same stream from the log alone
    pf = particle_filter(cfg, seq.mesh_vertices, cfg.expt.params.noise_ratio, downsample=1, device=dev)
    mn = pf.motion_noise
    torch.manual_seed(77)
    for idx, r in enumerate(a["frames"]):
        if idx < 2:  # the frames seen while prev_idx == 0 re-initialise and do not call motionModel
            pf.init_filter(seq.gt_p[idx, :], RUN_N)
        else:
            torch.normal(mean=mn["mu"], std=mn["sig_t"], size=(r["n"], 3))
            torch.normal(mean=mn["mu"], std=mn["sig_r"], size=(r["n"], 3))
        if r["status"] == 0:
            torch.rand(r["n_after"], dtype=torch.float64)
    assert torch.equal(torch.get_rng_state(), states["host"]), "the run drew something the log does not account for"
