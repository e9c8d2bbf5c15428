"""Seeded SYSTEMATIC resampling through the engines, the class surface and the runners: the reference's `low_var` resampler
(modules/particle_filter.py:251-261, 288-307) draws one float32 `torch.rand(1)` a frame on torch's CPU generator; here that draw
comes from the generator's replica on the device (the `rand32` draw kind, tests/test_gpu_mt_rand32.py), is never read back, and is
read by the resample kernels from device memory (tests/test_gpu_low_var_sites.py) - one per trajectory.

  * a seeded LoopEngine replays G19, the reference's own low_var loop (tools/gen_loop_trace_low_var.py), in all frames;
  * filter(draws="seeded", resample="low_var") == filter(draws="host", resample="low_var"), and torch's generator ends alike;
  * BatchLoopEngine, B = 3 seeds: every row is its seeded LoopEngine after every frame - one row driven onto all-pruned frames,
    where the reference's resampler returns before it draws and the stream must stand still (checked against a host generator);
  * the fixed-N engines (PipelinedFilterEngine, BatchFilterEngine, PipelinedBatchFilterEngine), motion both ways, against a host
    loop that draws torch.normal / torch.rand(1) per row and passes them in;
  * particle_filter.seed_device_stream + resampler("low_var") against G2's low_var entries;
  * filter_sweep(resample="low_var") against its filter() yardsticks;
  * the refusals that remain."""
import numpy as np
import pytest

from _recipes import sha

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


# ---- G19 --------------------------------------------------------------------------------------------------------------------------
def test_seeded_loop_engine_replays_g19(dev, golden, oracle):
    """G19 as tests/test_gpu_loop_seeded.py replays G13: per-frame set_particles / set_annealing_state from the oracle's loop (which
    carries the run), the engine's stream under manual_seed(3000 + t), ONE step() a frame - the kept-set and resample-index digests
    the reference wrote hold in all frames, the offset the engine used is the stored one, and the stream moved by one word."""
    from midastouch_amd.loop_engine import LoopEngine
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    g = golden("g19_loop_trace_low_var")
    cb = make_codebook(K=int(g["K"]), D=int(g["D"]), seed=int(g["cb_seed"]), mesh_points=20000)
    T, N0, S = int(g["T"]), int(g["N0"]), int(g["frame_seed"])
    traj = make_trajectory(cb, T=T + 1, seed=int(g["traj_seed"]))
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, ties="aten_cpu")
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0, resample="low_var", device=dev, topk_ties="aten_cpu")
    st = eng.seed_torch_stream_low_var(0)
    poses, labels = g["poses0"], np.zeros(N0, dtype=np.int64)
    for t in range(1, T + 1):
        n, n2 = poses.shape[0], int(g[f"N2_{t}"])
        eng.set_particles(torch.as_tensor(poses), torch.as_tensor(labels), reset_annealing=False)
        eng.set_annealing_state(float(loop.annealer.particle_var), loop.annealer.init_particles or 0)
        eng.step_count = t - 1
        st.manual_seed(S + t)
        eng.step(torch.as_tensor(traj.odoms[t]), torch.as_tensor(traj.codes[t]), gt=torch.as_tensor(traj.gt_poses[t]), dbscan=(t - 1) % 50 == 0)
        fv = eng.frame_view()
        assert fv["n"] == n and fv["n_after"] == n2 and fv["status"] == 0, t
        assert np.float32(eng._u[0].item()) == np.float32(g[f"u32_{t}"]) and eng._u[0].item() == float(np.float32(g[f"u32_{t}"])), t
        assert sha(fv["src"].cpu().numpy().astype(np.int32)) == str(g[f"keep_{t}_sha"]), f"frame {t}: kept set is not the reference's"
        assert sha(fv["ridx"].cpu().numpy().astype(np.int32)) == str(g[f"ridx_{t}_sha"]), f"frame {t}: resample indices are not the reference's"
        # the host generator under the same seed: the draws' sizes, then where the stream must stand
        torch.manual_seed(S + t)
        tn, rot = torch.normal(mean=0.0, std=2e-4, size=(n, 3)), torch.normal(mean=0.0, std=0.5, size=(n, 3))
        u32 = torch.rand(1)
        gen = torch.Generator()
        st.to_host(gen)
        assert torch.equal(torch.rand(4, dtype=torch.float64, generator=gen), torch.rand(4, dtype=torch.float64)), f"frame {t}: words consumed"
        ref = loop.step(poses, labels, traj.odoms[t], traj.codes[t], tn.numpy(), rot.numpy(), gt=traj.gt_poses[t], mode="low_var",
                        u32=np.float32(u32.item()))
        assert ref["N"] == n2
        poses, labels = ref["poses"], ref["labels"]
    assert not eng.read_log(T - 1, T)[0]["err"]


# ---- the runner -----------------------------------------------------------------------------------------------------------------------
N_RUN, T_RUN, FLOOR_RUN = 3000, 16, 300


@pytest.fixture(scope="module")
def scenario(dev):
    from midastouch_amd.config import load_config
    from midastouch_amd.filter import synthetic_sequence
    cfg = load_config([f"expt.params.num_particles={N_RUN}", "expt.codebook_size=2500"])
    return cfg, synthetic_sequence(cfg, dev, T=T_RUN)


def _same_stats(a, b, who=""):
    assert a["num_particles"] == b["num_particles"], who
    assert a["rmse_t"] == b["rmse_t"] and a["rmse_r"] == b["rmse_r"], who
    for x, y in zip(a["cluster_stds"], b["cluster_stds"]):
        assert torch.equal(x, y), who
    for x, y in zip(a["cluster_poses"], b["cluster_poses"]):
        assert torch.equal(x, y), who
    assert [f["kept"] for f in a["frames"]] == [f["kept"] for f in b["frames"]], who


@pytest.mark.parametrize("resample", ["low_var", "low_var_batch"])
def test_filter_seeded_equals_host_low_var(dev, scenario, resample):
    from midastouch_amd.filter import filter as run_filter
    cfg, seq = scenario
    torch.manual_seed(78)
    a = run_filter(cfg, seq=seq, device=dev, draws="host", floor=FLOOR_RUN, resample=resample)
    after_host = torch.rand(8, dtype=torch.float64)
    torch.manual_seed(78)
    b = run_filter(cfg, seq=seq, device=dev, draws="seeded", floor=FLOOR_RUN, resample=resample)
    after_seeded = torch.rand(8, dtype=torch.float64)
    _same_stats(a, b)
    assert min(a["num_particles"]) < N_RUN  # it annealed
    assert torch.equal(after_host, after_seeded), "torch's generator does not stand where the host-draw run leaves it"
    # and the mode is what ran: the multinomial run under the same seed is another run
    torch.manual_seed(78)
    c = run_filter(cfg, seq=seq, device=dev, draws="seeded", floor=FLOOR_RUN)
    assert c["rmse_t"] != b["rmse_t"]
    with pytest.raises(ValueError):
        run_filter(cfg, seq=seq, device=dev, resample="stratified")


def test_filter_real_passes_resample_through(dev, scenario):
    from midastouch_amd.filter import filter as run_filter
    from midastouch_amd.filter import filter_real
    cfg, seq = scenario
    torch.manual_seed(3)  # (init_filter draws on the host generator)
    a = filter_real(cfg, seq, device=dev, floor=FLOOR_RUN, resample="low_var", max_frames=6)
    torch.manual_seed(3)
    b = run_filter(cfg, seq, device=dev, floor=FLOOR_RUN, softmax=False, resample="low_var", max_frames=6)
    torch.manual_seed(3)
    c = filter_real(cfg, seq, device=dev, floor=FLOOR_RUN, max_frames=6)
    _same_stats(a, b)
    assert a["rmse_t"] != c["rmse_t"]


# ---- BatchLoopEngine -------------------------------------------------------------------------------------------------------------------
PER_PARTICLE = ("poses_prop", "nn_idx", "valid", "weights", "labels_frame", "src", "ridx", "poses", "weights_res", "labels", "hint")


def test_seeded_batch_rows_equal_seeded_singles(dev, oracle):
    """B = 3 seeds, N0 = 4096, low_var: every row against its seeded LoopEngine after every frame, bit for bit.  Row 1 is thrown 5 m
    off the object on frame 3: every particle is pruned there, the resampler returns before it draws (NDRAW = 0) and the row's stream
    takes that frame's motion noise only - every row's position at the end is the host generator's after exactly its draws."""
    from midastouch_amd import _lib
    from midastouch_amd.batch_loop_engine import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    from midastouch_amd.synthetic import make_codebook, make_trajectory, mesh_scale
    from midastouch_amd.torch_rng import normal_words
    B, N0, T, FLOOR, SEEDS, SHIFT = 3, 4096, 8, 500, (7301, 7302, 7303), 3
    cb = make_codebook("004_sugar_box", K=2500, D=256, seed=1000)
    traj = make_trajectory(cb, T=T + 2, seed=2000)
    g = torch.Generator().manual_seed(11)
    sc = mesh_scale(cb.extents)
    tn0 = torch.normal(0.0, sc / 3.0 * 0.15, size=(N0, 3), generator=g).numpy()
    rot0 = torch.normal(0.0, 60.0 * 0.15, size=(N0, 3), generator=g).numpy()
    start = cb.poses[oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices).f.SE3_NN_idx(oracle.init_filter_compose(traj.gt_poses[0], tn0, rot0))]
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    kw = dict(floor=FLOOR, resample="low_var", device=dev)
    singles = [LoopEngine(*src, N0, seed=4100 + b, topk_ties="aten_cpu", **kw) for b in range(B)]
    batch = BatchLoopEngine(*src, B, N0, seed=4100, **kw)
    for b, s in enumerate(singles):
        s.set_particles(torch.as_tensor(start))
        s.seed_torch_stream_low_var(SEEDS[b])
    batch.set_particles([torch.as_tensor(start)] * B)
    streams = batch.seed_torch_streams_low_var(SEEDS)
    assert batch.topk_ties == "aten_cpu"
    ndraw = []
    for t in range(T):
        od = torch.as_tensor(np.stack([traj.odoms[t + 1]] * B)).clone()
        if t == SHIFT:
            od[1, :3, 3] += 5.0
        co, gt = torch.as_tensor(np.stack([traj.codes[t + 1]] * B)), torch.as_tensor(np.stack([traj.gt_poses[t + 1]] * B))
        singles[0].step(od[0], co[0], gt=gt[0])
        batch.step(od, co, gts=gt)
        singles[1].step(od[1], co[1], gt=gt[1])
        singles[2].step(od[2], co[2], gt=gt[2])
        slot = (batch.step_count - 1) % batch.log_frames
        ndraw.append([int(v) for v in batch.ctl_i[:, _lib.LOOP_I_NDRAW].cpu()])
        for b, s in enumerate(singles):
            assert torch.equal(batch._log[b, slot].view(torch.int64), s._log[slot].view(torch.int64)), f"frame {t}, row {b}: log row"
            fs, fb = s.frame_view(), batch.frame_view(b)
            for k in PER_PARTICLE:
                assert fb[k].shape == fs[k].shape and torch.equal(fb[k], fs[k]), f"frame {t}, row {b}: {k}"
            assert batch._u[b, 0].item() == s._u[0].item(), f"frame {t}, row {b}: offset"
    log = batch.read_log()
    assert log[1][SHIFT]["status"] != 0 and log[1][SHIFT]["kept"] == 0 and ndraw[SHIFT][1] == 0, (ndraw, log[1][SHIFT])  # row 1: no draw there
    assert all(ndraw[t][b] == (0 if log[b][t]["status"] else log[b][t]["n_after"]) for t in range(T) for b in range(B)), ndraw
    assert all(log[b][t]["status"] == 0 for t in range(T) for b in (0, 2))                           # rows 0 and 2 draw every frame
    assert len({batch._u[b, 0].item() for b in range(B)}) == B                                       # three offsets in one frame
    assert any(log[0][t]["n_after"] != log[2][t]["n_after"] for t in range(T))                       # the rows part
    for b, s in enumerate(singles):
        # the host generator after exactly the reference's draws: two normal (n, 3) a frame, one rand(1) where the resampler drew
        gen = torch.Generator().manual_seed(SEEDS[b])
        for t in range(T):
            n = log[b][t]["n"]
            assert normal_words(3 * n)
            torch.normal(0.0, 1.0, size=(n, 3), generator=gen), torch.normal(0.0, 1.0, size=(n, 3), generator=gen)
            if log[b][t]["status"] == 0:
                torch.rand(1, generator=gen)
        want = torch.rand(8, dtype=torch.float64, generator=gen)
        for to_host in (lambda q: streams.to_host(b, q), s.torch_stream.to_host):
            q = torch.Generator()
            to_host(q)
            assert torch.equal(torch.rand(8, dtype=torch.float64, generator=q), want), f"row {b}: generator position"
    assert not batch._mt_status.any()


# ---- the fixed-N engines ---------------------------------------------------------------------------------------------------------------
def _scene(B, N, K=3000, D=256, seed=0):
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook("004_sugar_box", K=K, D=D, seed=1100 + seed)
    trs = [make_trajectory(cb, T=8, seed=2100 + seed + b) for b in range(B)]
    od = torch.as_tensor(np.stack([t.odoms for t in trs], axis=1))
    co = torch.as_tensor(np.stack([t.codes for t in trs], axis=1))
    gt = torch.as_tensor(np.stack([t.gt_poses for t in trs], axis=1))
    start = torch.as_tensor(cb.poses[np.random.default_rng(seed).integers(0, K, (B, N))])
    return cb, od, co, gt, start


def _host_row_draws(gens, N, sig_t, sig_r):
    """A frame's draws of every row on its own generator, in the reference's order: tn, rot, then the systematic offset."""
    tn, rot, u32 = [], [], []
    for q in gens:
        tn.append(torch.normal(0.0, sig_t, size=(N, 3), generator=q))
        rot.append(torch.normal(0.0, sig_r, size=(N, 3), generator=q))
        u32.append(torch.rand(1, generator=q))
    return torch.stack(tn), torch.stack(rot), torch.cat(u32)


def _same_engines(a, h, t):
    for k in ("ridx", "poses", "weights", "rmse"):
        assert torch.equal(getattr(a, k), getattr(h, k)), f"frame {t}: {k}"


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("N", [1000, 4097])
@pytest.mark.parametrize("engine", ["PipelinedFilterEngine", "BatchFilterEngine", "PipelinedBatchFilterEngine"])
def test_fixed_n_engines_seeded_equal_host_draws(dev, engine, N, motion):
    """The seeded engine (systematic mode: one rand32 per trajectory per frame) against the same engine fed by a host loop that draws
    torch.normal (N, 3) twice and torch.rand(1) per row on generators seeded alike and passes them in - the offsets as B values."""
    from midastouch_amd import engine as E
    cls, single = getattr(E, engine), engine == "PipelinedFilterEngine"
    B, T = (1 if single else 3), 5
    cb, od, co, gt, start = _scene(B, N, seed=N % 7)
    lead = () if single else (B,)
    mk = lambda: cls(cb.poses, cb.embeddings, cb.mesh_vertices, *lead, N, resample="low_var", device=dev)  # noqa: E731
    a, h = mk(), mk()
    sq = (lambda x: x[0]) if single else (lambda x: x)
    for e in (a, h):
        e.set_particles(sq(start))
        e.project_to_codebook()
    seeds = [3000 + 17 * b for b in range(B)]
    st = a.seed_torch_stream(seeds[0], motion=motion) if single else a.seed_torch_streams_low_var(seeds, motion=motion)
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    od, co, gt = od.to(dev), co.to(dev), gt.to(dev)
    pipelined = engine.startswith("Pipelined")
    for t in range(1, T + 1):
        tn, rot, u32 = _host_row_draws(gens, N, a.sig_t, a.sig_r)
        if motion:
            a.step(sq(od[t]), sq(co[t]), sq(gt[t]))
        else:
            a.step(sq(od[t]), sq(co[t]), sq(gt[t]), tn=sq(tn), rot=sq(rot))
        h.step(sq(od[t]), sq(co[t]), sq(gt[t]), tn=sq(tn), rot=sq(rot), u32=float(u32[0]) if single else u32)
        if not pipelined or t in (3, T):   # (reading a pipelined engine materialises the resample: mostly left folded)
            _same_engines(a, h, t)
    g = torch.Generator()
    st.to_host(g) if single else st.to_host(B - 1, g)
    if motion and pipelined:  # the pipelined engines have drawn the next frame's unit normals already
        torch.normal(0.0, 1.0, size=(N, 3), generator=gens[-1]), torch.normal(0.0, 1.0, size=(N, 3), generator=gens[-1])
    assert torch.equal(torch.rand(9, generator=g), torch.rand(9, generator=gens[-1])), "generator position"
    assert a.ridx.shape == h.ridx.shape and not torch.equal(a.ridx[..., :N], torch.arange(N, device=dev).expand_as(a.ridx)), "no resample ran"


# ---- the class surface ---------------------------------------------------------------------------------------------------------------
def test_particle_filter_low_var_on_the_device_stream(dev, golden, monkeypatch):
    """seed_device_stream(s) + resampler("low_var") == the reference under torch.manual_seed(s) (G2's low_var entries), with the host
    generator untouched and nothing read back for the offset (torch.rand is not called)."""
    from midastouch_amd.config import load_config
    from midastouch_amd.particle_filter import Particles, particle_filter
    g = golden("g2_resampler")
    pf = particle_filter(load_config(), np.zeros((8, 3)), 1.0, downsample=1, device=dev)

    def no_host_draw(*a, **k):
        raise AssertionError("the seeded resampler drew on the host generator")

    for tag in ["soft4096", "soft1000", "peaky2048", "masked3000", "n1", "n2", "n65"]:
        w = g[f"{tag}_w"]
        n = len(w)
        poses = torch.eye(4)[None].repeat(n, 1, 1).clone()
        poses[:, 0, 3] = torch.arange(n, dtype=torch.float32)
        parts = Particles(poses.to(dev), torch.as_tensor(w).to(dev), torch.arange(n, dtype=torch.float32).to(dev))
        pf.seed_device_stream(int(g[f"{tag}_low_var_seed"]))
        torch.manual_seed(1)
        state = torch.get_rng_state()
        with monkeypatch.context() as m:
            m.setattr(torch, "rand", no_host_draw)
            out = pf.resampler(parts, resample="low_var")
        idx = out.poses[:, 0, 3].cpu().numpy().astype(np.int64)
        assert np.array_equal(idx, g[f"{tag}_low_var_idx"]), tag
        assert np.array_equal(out.weights.cpu().numpy(), w[idx])
        assert torch.equal(torch.get_rng_state(), state)
        # the stream moved by the one word: its next draw is the host's second
        torch.manual_seed(int(g[f"{tag}_low_var_seed"]))
        assert np.float32(torch.rand(1).item()) == np.float32(g[f"{tag}_low_var_u"][0])
        assert torch.equal(pf.torch_stream.rand32().cpu(), torch.rand(1))
    pf.seed_device_stream(None)
    torch.manual_seed(int(g["n65_low_var_seed"]))
    out = pf.resampler(parts, resample="low_var")  # without a stream: the host generator, as ever
    assert np.array_equal(out.poses[:, 0, 3].cpu().numpy().astype(np.int64), g["n65_low_var_idx"])


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
def test_filter_sweep_low_var_rows_equal_their_yardsticks(dev):
    """Two runs (two objects, logs of 7 and 9 frames) x two trials, resample="low_var": every row is filter(..., seed=seed + row,
    start="device", resample="low_var") exactly; and the sweep's mode is what ran."""
    from midastouch_amd import ops
    from midastouch_amd.config import load_config
    from midastouch_amd.filter import Sequence, filter_sweep
    from midastouch_amd.filter import filter as run_filter
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    from midastouch_amd.tactile_tree import tactile_tree
    N0, FLOOR, SEED, TRIALS = 700, 300, 5300, 2
    cfg = load_config([f"expt.params.num_particles={N0}"])
    runs = []
    for i, (name, K, T) in enumerate((("004_sugar_box", 1500, 7), ("025_mug", 900, 9))):
        cb = make_codebook(name, K=K, D=128, seed=1013 + i, mesh_points=4000)
        tt = tactile_tree(torch.as_tensor(cb.poses), torch.as_tensor(cb.cam_poses), torch.as_tensor(cb.embeddings))
        tt.to_device(dev)
        tr = make_trajectory(cb, T=T, seed=2100 + i)
        runs.append(Sequence(torch.as_tensor(tr.gt_poses).to(dev), torch.as_tensor(tr.meas_poses).to(dev), torch.as_tensor(tr.codes).to(dev), tt,
                             cb.mesh_vertices, cb.obj_model, mesh_tree=ops.Tree(torch.as_tensor(cb.mesh_vertices).to(dev, torch.float64)), log_id=i))
    kw = dict(floor=FLOOR, cluster_every=3, resample="low_var")
    rows = filter_sweep(cfg, runs, trials=TRIALS, seed=SEED, device=dev, **kw)
    assert len(rows) == 4
    for r in range(2):
        for k in range(TRIALS):
            row = r * TRIALS + k
            want = run_filter(cfg, runs[r], device=dev, seed=SEED + row, start="device", **kw)
            _same_stats(rows[row], want, f"row {row}")
    other = filter_sweep(cfg, runs, trials=TRIALS, seed=SEED, device=dev, floor=FLOOR, cluster_every=3)
    assert other[0]["rmse_t"] != rows[0]["rmse_t"]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_remain(dev):
    from midastouch_amd._lib import MidasError
    from midastouch_amd.batch_loop_engine import BatchLoopEngine
    from midastouch_amd.engine import PipelinedFilterEngine
    from midastouch_amd.loop_engine import LoopEngine
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    cb = make_codebook("004_sugar_box", K=900, D=128, seed=1000)
    traj = make_trajectory(cb, T=3, seed=2000)
    src = (cb.poses, cb.embeddings, cb.mesh_vertices)
    B, n = 2, 200
    od, co = torch.as_tensor(np.stack([traj.odoms[1]] * B)), torch.as_tensor(np.stack([traj.codes[1]] * B))
    start = torch.as_tensor(cb.poses[:n])
    wide = BatchLoopEngine(*src, B, n, resample="low_var", floor=100, wide=True, device=dev)
    with pytest.raises(MidasError, match="wide"):
        wide.seed_torch_streams_low_var([1, 2])
    with pytest.raises(MidasError, match="wide"):
        wide.step(od, co, u32=[0.1, 0.2])
    rows = BatchLoopEngine(*src, B, n, resample="low_var", floor=[100, 120], device=dev)
    with pytest.raises(MidasError, match="per"):
        rows.seed_torch_streams_low_var([1, 2])
    with pytest.raises(MidasError, match="per-row"):
        rows.set_particles([start] * B) or rows.step(od, co, u32=[0.1, 0.2])
    low = BatchLoopEngine(*src, B, n, resample="low_var", floor=100, device=dev)
    low.set_particles([start] * B)
    with pytest.raises(MidasError, match="_low_var"):  # the plain call still means multinomial's draws: a systematic engine has its own method
        low.seed_torch_streams([1, 2])
    assert low.torch_streams is None and low.topk_ties == "index"
    low.seed_torch_streams_low_var([1, 2])
    for u32 in (0.5, 0.0, [0.1, 0.2]):
        with pytest.raises(MidasError, match="desynchronise"):
            low.step(od, co, u32=u32)
    assert low.step_count == 0
    with pytest.raises(MidasError, match="per"):
        low.set_row_params(floor=[100, 120])
    low.step(od, co)  # (and the seeded frame itself runs)
    one = LoopEngine(*src, n, resample="low_var", floor=100, device=dev)
    one.set_particles(start)
    with pytest.raises(MidasError, match="_low_var"):
        one.seed_torch_stream(3)
    one.seed_torch_stream_low_var(3)
    with pytest.raises(MidasError, match="desynchronise"):
        one.step(od[0], co[0], u32=0.25)
    one.step(od[0], co[0])
    assert one.read_log()[0]["n"] == n
    # per-row offsets belong to the systematic mode
    multi = BatchLoopEngine(*src, B, n, floor=100, device=dev)
    multi.set_particles([start] * B)
    with pytest.raises(MidasError, match="low_var"):  # ... and so does the seeding of the systematic mode
        multi.seed_torch_streams_low_var([1, 2])
    with pytest.raises(MidasError, match="low_var"):
        multi.step(od, co, u32=[0.1, 0.2])
    # the pipelined engine no longer ignores its stream in systematic mode: the frame takes the stream's offset, the stream moves on
    a, b = (PipelinedFilterEngine(*src, n, resample="low_var", device=dev) for _ in range(2))
    for e in (a, b):
        e.set_particles(start)
    st = a.seed_torch_stream(5)
    a.step(od[0], co[0])
    torch.manual_seed(5)
    r = torch.rand(1)
    b.step(od[0], co[0], u32=float(r))
    assert a._draw[1] == -2.0 and a._draw[0][0].item() == float(r)  # the offset in device memory is torch.rand(1) under the seed
    assert torch.equal(a.ridx, b.ridx)
    g = torch.Generator()
    st.to_host(g)
    assert torch.equal(torch.rand(4, generator=g), torch.rand(4))
