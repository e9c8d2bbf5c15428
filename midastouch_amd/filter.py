"""Filter runner: the reference's per-frame loop (`midastouch/filter/filter.py:42-256`) on the MI355X path.

Two ways to run a sequence:

* `filter(cfg, ...)`  - the reference's loop body call for call (motionModel -> particle_rmse -> SE3_NN ->
  get_similarity -> remove_invalid_particles -> cluster_particles/get_cluster_centers -> annealing ->
  resampler), same order of operations, same RNG draw order, same guards and the same `filter_stats`
  keys (:99-116).  It is the counterpart of row H of SURVEY.md 8(a).
* `step(...) / update_weights(...) / resample(...)` - the north-star aliases.  `step` drives a
  `FilterEngine` (one fused C-ABI call per frame, fixed N); `update_weights` is SE3_NN + get_similarity
  without the (N, D) gather; `resample` is `particle_filter.resampler`.

Upstream perception (TDN/TCN, `filter.py:144-147`) is out of scope: tactile codes are inputs.  The
datasets of the reference are external downloads, so sequences come from `synthetic.py`.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .engine import FilterEngine
from .particle_filter import Particles, cfg_motion_noise, particle_filter, particle_rmse
from .synthetic import make_codebook, make_trajectory
from .tactile_tree import tactile_tree


@dataclass
class Sequence:
    """What the reference loads per log: gt / measured poses (`extract_poses_sim`, pose.py:272-300) and,
    instead of tactile images, the tactile codes the TCN would emit for them."""
    gt_p: torch.Tensor       # (T,4,4) f32
    meas_p: torch.Tensor     # (T,4,4) f32
    codes: torch.Tensor      # (T,D)   f64
    codebook: tactile_tree
    mesh_vertices: np.ndarray
    obj_model: str
    mesh_tree: Optional[object] = None  # an ops.Tree over mesh_vertices already on the device (shared with other engines)
    log_id: Optional[object] = None     # the log's number in `filter_stats` (None: cfg.expt.log_id)
    cfg: Optional[object] = None        # the run's own config in a `filter_sweep` (None: the sweep's) - its dataset's noise_t, noise_r,
                                        # num_particles and noise_ratio (config/expt/ycb.yaml, mcmaster.yaml) and pen.max


def synthetic_sequence(cfg, device, T: int = 100, D: Optional[int] = None, seed: int = 0) -> Sequence:
    obj = cfg.expt.obj_model
    K = int(cfg.expt.codebook_size)
    D = int(D if D is not None else cfg.tcn.model.output_dim)
    cb = make_codebook(obj, K=K, D=D, seed=1000 + seed)
    traj = make_trajectory(cb, T=T, seed=2000 + seed)
    tree = tactile_tree(torch.as_tensor(cb.poses), torch.as_tensor(cb.cam_poses), torch.as_tensor(cb.embeddings))
    tree.to_device(device)
    return Sequence(torch.as_tensor(traj.gt_poses).to(device), torch.as_tensor(traj.meas_poses).to(device),
                    torch.as_tensor(traj.codes).to(device), tree, cb.mesh_vertices, obj)


def load_sequence(sequence_npz: str, codebook_path: str, device, obj_model: str = "object", check_logmap: bool = False) -> Sequence:
    """A recorded sequence: `codebook_path` is a `codebook.npz` or a reference `codebook.pkl` (codebook_io.py);
    `sequence_npz` holds `gt_poses (T,4,4)`, `meas_poses (T,4,4)`, `codes (T,D)` (the TCN outputs, upstream of this
    path) and `mesh_vertices (M,3)` (the decimated STL vertices of `particle_filter.__init__`, :108-110)."""
    tree = tactile_tree.load(codebook_path, device=device, check_logmap=check_logmap)
    with np.load(sequence_npz) as z:
        need = ("gt_poses", "meas_poses", "codes", "mesh_vertices")
        missing = [k for k in need if k not in z.files]
        if missing:
            raise ValueError(f"{sequence_npz}: arrays {missing} missing")
        gt, meas, codes, verts = (np.asarray(z[k]) for k in need)
    if codes.shape[1] != tree.embeddings.shape[1]:
        raise ValueError(f"tactile codes are {codes.shape[1]}-d, the codebook's embeddings {tree.embeddings.shape[1]}-d")
    return Sequence(torch.as_tensor(gt, dtype=torch.float32).to(device), torch.as_tensor(meas, dtype=torch.float32).to(device),
                    torch.as_tensor(codes, dtype=torch.float64).to(device), tree, verts, obj_model)


# ---- north-star aliases ---------------------------------------------------------------------------
def update_weights(pf: particle_filter, codebook: tactile_tree, particles: Particles, tactile_code: torch.Tensor,
                   softmax: bool = True) -> Particles:
    """particles.weights <- similarity of the tactile code to each particle's nearest codebook pose
    (filter/filter.py:170-173) - the codebook is scored once, no (N, D) gather."""
    _, _, nn_codes = codebook.SE3_NN(particles.poses)
    particles.weights = pf.get_similarity(tactile_code, nn_codes, softmax=softmax)
    return particles


def resample(pf: particle_filter, particles: Particles, mode: str = "weighted_random") -> Particles:
    return pf.resampler(particles, resample=mode)


def step(engine: FilterEngine, odom: torch.Tensor, tactile_code: torch.Tensor, gt_pose: torch.Tensor = None, **draws):
    """One fused frame on a FilterEngine (propagate -> score/NN -> weights -> prune -> resample)."""
    engine.step(odom, tactile_code, gt=gt_pose, **draws)
    return engine


# ---- the reference loop -----------------------------------------------------------------------------
def _log_id(seq, expt_cfg) -> str:
    """`filter_stats["log_id"]` (filter.py:114): the sequence's own number when it carries one, the config's otherwise."""
    own = getattr(seq, "log_id", None)
    return str(expt_cfg.log_id if own is None else own).zfill(2)


def filter(cfg, seq: Optional[Sequence] = None, viz=None, device=None, pace: str = "fixed", max_frames: int = None,
           cluster: bool = True, progress: bool = False, softmax: bool = True, update_freq: int = 1, floor: int = 1000,
           results_path: Optional[str] = None, draws: str = "device", seed: int = 4000, start: str = "host",
           cluster_every: int = 50, resample: str = "weighted_random", centers: str = "quat_avg") -> dict:
    """Run the filter over a sequence; returns the reference's `filter_stats` dict (filter.py:99-116).

    The loop body (filter.py:150-190: motionModel -> particle_rmse -> SE3_NN + get_similarity -> remove_invalid_particles
    [-> re-projection] -> cluster_particles every 50th frame -> get_cluster_centers -> annealing -> resampler) is one
    `LoopEngine.step` per frame: same order of operations, same guards, the particle count on the device, nothing read back
    between frames; rmse, particle counts and cluster centres come out of the engine's frame log after the last frame.

    draws="device" (default): Philox streams on the device, frames are enqueued back to back.  draws="host": the
    reference's own random streams - torch.normal tn, rot and the resampler's torch.rand on the CPU generator, in its
    order - which needs the particle count on the host twice per frame (bit-parity with the reference under
    torch.manual_seed, at the price of those read-backs and of the host generator); annealing's top-k then also resolves its
    ties the way torch.topk does on the CPU (LoopEngine(topk_ties="aten_cpu")), so the particle SET is the reference's too.
    draws="seeded": the SAME numbers as draws="host" - torch's default CPU generator continued on the device (torch_rng.py:
    its mt19937 stream, `torch.normal`'s float32 transform as tables read off torch itself, `torch.rand` float64) - without the
    host generating and uploading 6 N normals and N uniforms a frame and without either read-back: the draws take their sizes
    from the counts on the device (LoopEngine.seed_torch_stream), so frames are enqueued back to back as with draws="device";
    the host-side draws of `init_filter` take the stream over and hand it back, and at the end torch's generator stands where
    draws="host" leaves it.  (A live count below 6 - fewer than 16 normal values, another code path of ATen - is an error of the
    frame log, not a host draw.)
    pace="fixed" steps one frame per iteration; pace="wallclock" reproduces `idx = int(frame_rate * total_time)`
    (:134-135: slow iterations skip frames, fast ones repeat) and therefore waits for every frame.
    The defaults are `filter/filter.py`'s; `filter_real(...)` presets the real-data script's variations
    (`filter/filter_real.py`: raw scores :208-210, measurement update every `update_freq`-th frame with unit weights in
    between :205-212, annealing floor 10000 :228).  results_path: directory `filter_stats.npy` is written to (:252).
    start="host" (default): the frames seen while prev_idx == 0 start as the reference does - `init_filter` on the host (torch.normal,
    scipy's Euler conversion), an upload and the projection.  start="device": `LoopEngine.start` - the same arithmetic in two
    launches, the draws from Philox (draws="device" only); what `filter_sweep` does for every row, so the single-run yardstick of a
    sweep.  cluster_every: DBSCAN on every cluster_every-th frame (50: filter.py:182).
    resample: the mode `pf.resampler(particles, resample=...)` is called with (particle_filter.py:230-261) - "weighted_random"
    (the reference's call), or "low_var" / "low_var_batch": the systematic resampler, whose one draw a frame is a float32
    `torch.rand(1)` (:291) - with draws="host" drawn here when the resampler draws at all (NDRAW > 0), with draws="seeded" by the
    device stream, with draws="device" from Philox.
    centers: the method `pf.get_cluster_centers(particles, ...)` is called with - "quat_avg" (filter.py:184-186), or "logmap", the
    reference signature's default: `filter_stats["cluster_poses"]` / `["cluster_stds"]` and annealing's spread are then the log-map
    centres' (LoopEngine(centers="logmap")).
    """
    from . import _lib
    from .engine import RESAMPLE_MODES
    from .loop_engine import LoopEngine

    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if resample not in RESAMPLE_MODES:
        raise ValueError(f"resample must be one of {sorted(RESAMPLE_MODES)}")
    systematic = RESAMPLE_MODES[resample] == _lib.RESAMPLE_SYSTEMATIC
    if draws not in ("device", "host", "seeded"):
        raise ValueError("draws must be 'device', 'host' or 'seeded'")
    if start not in ("host", "device"):
        raise ValueError("start must be 'host' or 'device'")
    if start == "device" and draws != "device":
        raise ValueError("start='device' draws the initial particles from Philox: draws='device' only")
    cluster_every = max(int(cluster_every), 1)
    expt_cfg = cfg.expt
    init_particles = int(expt_cfg.params.num_particles)
    noise_ratio = expt_cfg.params.noise_ratio
    frame_rate = expt_cfg.frame_rate
    if seq is None:
        seq = synthetic_sequence(cfg, device)
    gt_p, meas_p, codebook = seq.gt_p, seq.meas_p, seq.codebook
    traj_size = gt_p.shape[0] if expt_cfg.max_length in (None, "None") else min(gt_p.shape[0], int(expt_cfg.max_length))
    if max_frames is not None:
        traj_size = min(traj_size, max_frames)
    pf = particle_filter(cfg, seq.mesh_vertices, noise_ratio, downsample=1, device=device)
    if seq.mesh_tree is not None:
        pf._mesh_tree = seq.mesh_tree
    eng = LoopEngine(codebook, None, pf.mesh_kdtree, init_particles, sig_t=pf.motion_noise["sig_t"], sig_r=pf.motion_noise["sig_r"],
                     pen_max=pf.pen_max, seed=seed, softmax=softmax, resample=resample, floor=floor, cluster=cluster,
                     log_frames=max(traj_size + 8, 64), device=device, topk_ties="aten_cpu" if draws in ("host", "seeded") else "index",
                     centers=centers)
    # seeded: the engine draws every frame's numbers from torch's stream on the device (LoopEngine.seed_torch_stream)
    stream = (eng.seed_torch_stream_low_var if systematic else eng.seed_torch_stream)(0) if draws == "seeded" else None
    on_device = False  # seeded: who holds torch's stream at the moment (False: the host's default generator)

    def stream_to(dev_side: bool):
        nonlocal on_device
        if stream is None or on_device == dev_side:
            return
        stream.from_host() if dev_side else stream.to_host()
        on_device = dev_side
    # odom = inv(meas[prev]) @ meas[idx] (:154): the inverses in one call, and - frame after frame in fixed pace - the
    # products too (a 4x4 product per frame through the BLAS library costs more device time than the whole frame's kernels)
    inv_meas = torch.linalg.inv(meas_p)
    step_odoms = torch.matmul(inv_meas[:-1], meas_p[1:]).contiguous() if meas_p.shape[0] > 1 else None
    eye = torch.eye(4, device=device)
    heatmap_poses, _ = codebook.get_poses()
    heatmap_embeddings = codebook.get_embeddings()
    every_frame = pace == "wallclock" or viz is not None or progress  # somebody looks at every frame: wait for it

    filter_stats = {
        "rmse_t": [], "rmse_r": [], "time": [], "traj_size": traj_size, "avg_time": None, "total_time": 0,
        "cluster_poses": [], "cluster_stds": [], "obj_name": seq.obj_model, "tree_size": len(codebook),
        "noise_ratio": noise_ratio, "init_noise": pf.init_noise, "init_particles": init_particles,
        "num_particles": [], "log_id": _log_id(seq, expt_cfg), "trial_id": 0,
    }
    motion_time = []
    events = [torch.cuda.Event(enable_timing=True)]
    events[0].record()
    prev_idx, count, fixed_idx, total_time = 0, 0, 0, 0.0
    frame_idx = []  # the sequence frame each iteration looked at (pace="wallclock" skips and repeats)
    records = []    # frame-log rows read back so far
    import gc
    gc.collect()
    gc.freeze()  # the libraries' ~10^6 long-lived objects out of the collector's way: no 30 ms pass in the middle of a run
    try:
        while True:
            if pace == "wallclock":
                idx = int(frame_rate * total_time)
            else:
                idx = fixed_idx
                fixed_idx += 1
            if idx >= traj_size:
                break
            if count and count % eng.log_frames == 0:
                # wall-clock pace on a fast host repeats frames: more iterations than the engine's frame log (a ring) holds
                records.extend(eng.read_log(count - eng.log_frames, count))
            t_start = time.time()  # (the reference's `start`; here that name is the parameter)
            moving = prev_idx > 0
            if not moving:  # (filter.py:152,156-160) - like the reference, frames seen while prev_idx == 0 re-initialise
                if start == "device":
                    eng.start(gt_p[idx, :], pf.init_noise, n=init_particles, reset_annealing=count == 0)
                else:
                    stream_to(False)  # init_filter draws on the host generator
                    particles = pf.init_filter(gt_p[idx, :], init_particles)
                    eng.set_particles(particles.poses, reset_annealing=count == 0)
                    eng.project_to_codebook()
                odom = eye
            else:
                odom = step_odoms[prev_idx] if idx == prev_idx + 1 else inv_meas[prev_idx] @ meas_p[idx, :]
            unit = count % max(int(update_freq), 1) != 0  # filter_real.py:205-212: no measurement update on this frame
            kw = dict(gt=gt_p[idx, :], dbscan=cluster and count % cluster_every == 0, unit_weights=unit, std_override=None if moving else (0.0, 0.0))
            if draws == "host":
                n = eng.n
                if moving:  # add_noise_to_odom's draws, its order (:326-335); the initial frames draw inside init_filter
                    kw["tn"] = torch.normal(mean=pf.motion_noise["mu"], std=pf.motion_noise["sig_t"], size=(n, 3))
                    kw["rot"] = torch.normal(mean=pf.motion_noise["mu"], std=pf.motion_noise["sig_r"], size=(n, 3))
                else:
                    kw["tn"], kw["rot"] = torch.zeros((n, 3)), torch.zeros((n, 3))
                eng.step(odom, seq.codes[idx], phases=_lib.LOOP_FRONT | _lib.LOOP_DBSCAN | _lib.LOOP_ANNEAL, stream_draws=True, **kw)
                # multinomial's stream (:245) - which the resampler does not touch when the weights are all zero or hold a NaN
                # (:237-241): the device says how many uniforms this frame draws (NDRAW: n_set or 0)
                ci = eng.ctl_i.cpu()
                n_set, n_draw = int(ci[_lib.LOOP_I_NSET]), int(ci[_lib.LOOP_I_NDRAW])
                if systematic:  # low_var's one draw (:291), when the resampler gets as far as drawing
                    eng.step(None, None, u32=float(torch.rand(1)) if n_draw else -1.0, phases=_lib.LOOP_RESAMPLE, stream_draws=True)
                else:
                    u = torch.rand(n_draw, dtype=torch.float64) if n_draw else torch.zeros(n_set, dtype=torch.float64)  # (unused)
                    eng.step(None, None, u=u, phases=_lib.LOOP_RESAMPLE, stream_draws=True)
            elif draws == "seeded":
                # the same draws, sized on the device: nothing is read back (frames seen while prev_idx == 0 do not call motionModel)
                stream_to(True)
                eng.step(odom, seq.codes[idx], motion_draws=moving, **kw)
            else:
                eng.step(odom, seq.codes[idx], **kw)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
            if every_frame:
                ev.synchronize()
                total_time += events[-2].elapsed_time(ev) * 1e-3 if pace != "wallclock" else time.time() - t_start
            if viz is not None:
                heatmap_weights = pf.get_similarity(seq.codes[idx][None], heatmap_embeddings, softmax=False)
                rec = eng.frame_view()
                # the visualiser reads particles.poses asynchronously (viz/visualizer.py:329-361): hand it a snapshot
                snap = Particles(rec["poses"].clone(), rec["weights_res"].clone(), rec["labels"].clone())
                viz.update(snap, torch.as_tensor(rec["cluster_poses"]), torch.as_tensor(rec["cluster_stds"]), gt_p[idx, :], heatmap_poses,
                           heatmap_weights, None, None, None, idx)
            if progress:
                rec = eng.read_log(count, count + 1)[0]
                print(f"[{idx}] RMSE {1000 * rec['rmse_t']:.1f} mm {rec['rmse_r']:.0f} deg P {rec['n_after']} "
                      f"rate {1.0 / max(events[-2].elapsed_time(ev) * 1e-3, 1e-9):.1f} Hz")
            motion_time.append(time.time() - t_start)
            frame_idx.append(idx)
            prev_idx = idx
            count += 1
        torch.cuda.synchronize(device)
        stream_to(False)  # seeded: torch's generator continues where the run's draws ended
    finally:
        gc.unfreeze()  # also when a frame raises: a frozen collector would outlive the run
    records.extend(eng.read_log(len(records), count))
    for rec, e0, e1 in zip(records, events, events[1:]):
        filter_stats["rmse_t"].append(rec["rmse_t"])
        filter_stats["rmse_r"].append(rec["rmse_r"])
        filter_stats["cluster_poses"].append(torch.as_tensor(rec["cluster_poses"]))
        filter_stats["cluster_stds"].append(torch.as_tensor(rec["cluster_stds"]))
        filter_stats["num_particles"].append(rec["n_after"])
        filter_stats["time"].append(e0.elapsed_time(e1) * 1e-3)  # frame to frame on the device's clock
    filter_stats["total_time"] = sum(filter_stats["time"])
    filter_stats["avg_time"] = filter_stats["total_time"] / max(len(filter_stats["time"]), 1)
    # the reference's three timers: perception is upstream of this path; motion and measurement share one launch here
    filter_stats["avg_timer"] = {"tactile": 0.0, "motion": 0.0, "meas": filter_stats["avg_time"],
                                 "host_enqueue": float(np.average(motion_time)) if motion_time else 0.0}
    filter_stats["frames"] = records
    filter_stats["frame_idx"] = frame_idx
    filter_stats["host_time"] = motion_time  # seconds the host spent on each iteration (enqueueing; waiting too when somebody looks at every frame)
    if results_path is not None:
        save_filter_stats(filter_stats, results_path)
    return filter_stats


def save_filter_stats(filter_stats: dict, results_path: str) -> str:
    """`np.save(results_path/filter_stats.npy, filter_stats)` (filter.py:252) - a pickled dict, read back with
    `np.load(..., allow_pickle=True).item()`; device tensors are moved to the host first."""
    import os

    os.makedirs(results_path, exist_ok=True)
    host = {k: ([t.cpu() if torch.is_tensor(t) else t for t in v] if isinstance(v, list) else
                (v.cpu() if torch.is_tensor(v) else v)) for k, v in filter_stats.items()}
    path = os.path.join(results_path, "filter_stats.npy")
    np.save(path, host)
    return path


def filter_real(cfg, seq: Optional[Sequence] = None, **kw) -> dict:
    """The loop with `filter/filter_real.py`'s settings: raw similarity scores as weights, annealing floor 10000."""
    kw.setdefault("softmax", False)
    kw.setdefault("floor", 10000)
    return filter(cfg, seq, **kw)


# ---- the reference's experiment: objects x logs x trials (bash/run_filter.sh) as one batch -----------------------------------------
def sweep_plan(runs, trials: int = 1, max_length=None, max_frames=None) -> dict:
    """Rows of a sweep, on the host: runs that share one `codebook` object are one object of the batch (in order of first
    appearance), row r * trials + k is run r, trial k.  -> objects (for each object the index of its first run), run_object,
    row_object, row_run, row_trial, run_lengths and lengths (frames of every run and of every row: the log's, cut by max_length -
    cfg.expt.max_length - and max_frames) and T_max."""
    runs = list(runs)
    if not runs:
        raise ValueError("filter_sweep needs at least one run")
    if int(trials) < 1:
        raise ValueError(f"filter_sweep needs trials >= 1, got {trials}")
    trials = int(trials)
    seen, objects, run_object = {}, [], []
    for r, seq in enumerate(runs):
        key = id(seq.codebook)
        if key not in seen:
            seen[key] = len(objects)
            objects.append(r)
        run_object.append(seen[key])
    run_len = []
    for seq in runs:
        T = int(seq.gt_p.shape[0])
        if max_length not in (None, "None"):
            T = min(T, int(max_length))
        if max_frames is not None:
            T = min(T, int(max_frames))
        run_len.append(T)
    row_run = [r for r in range(len(runs)) for _ in range(trials)]
    row_trial = [k for _ in range(len(runs)) for k in range(trials)]
    lengths = [run_len[r] for r in row_run]
    return dict(objects=objects, run_object=run_object, row_object=[run_object[r] for r in row_run], row_run=row_run,
                row_trial=row_trial, run_lengths=run_len, lengths=lengths, T_max=max(lengths))


def sweep_row_params(cfg, runs, plan, softmax=True, floor=1000, update_freq=1) -> dict:
    """What the rows of a sweep take for themselves, on the host: run r's config is `runs[r].cfg` (None: the sweep's `cfg`) - its
    num_particles, noise_ratio, motion noise (noise_t, noise_r) and prune threshold (tdn.render.pen.max) - and its runner's preset is
    softmax / floor / update_freq, each one value for the sweep or one per run (filter/filter.py: softmax, floor 1000;
    filter/filter_real.py: raw scores, floor 10 000, update_freq).  Row r * trials + k takes run r's.
    -> run_cfgs; per row: num_particles, noise_ratio, sig_t, sig_r, pen_max, softmax, floor, update_freq; capacity (the largest
    count), wide (beyond 16 384) and engine: the keywords `BatchLoopEngine.for_objects` gets - a scalar where all rows agree (with
    scalars only the batch runs the shared-parameter frame), a list of B values otherwise."""
    from . import _lib
    from .particle_filter import _cfg_get

    R = len(runs)

    def per_run(name, v, conv):
        if isinstance(v, (list, tuple)):
            if len(v) != R:
                raise ValueError(f"filter_sweep: {len(v)} values of {name} for {R} runs (one value, or one per run)")
            return [conv(x) for x in v]
        return [conv(v)] * R
    presets = dict(softmax=per_run("softmax", softmax, bool), floor=per_run("floor", floor, int),
                   update_freq=[max(u, 1) for u in per_run("update_freq", update_freq, int)])
    run_cfgs = [cfg if getattr(seq, "cfg", None) is None else seq.cfg for seq in runs]
    noise = [cfg_motion_noise(c) for c in run_cfgs]
    of_run = dict(num_particles=[int(c.expt.params.num_particles) for c in run_cfgs],
                  noise_ratio=[c.expt.params.noise_ratio for c in run_cfgs],
                  sig_t=[m["sig_t"] for m in noise], sig_r=[m["sig_r"] for m in noise],
                  pen_max=[float(_cfg_get(c, "tdn", "render", "pen", "max")) for c in run_cfgs], **presets)
    out = {k: [v[r] for r in plan["row_run"]] for k, v in of_run.items()}
    out["run_cfgs"] = run_cfgs
    out["capacity"] = max(out["num_particles"])
    out["wide"] = out["capacity"] > _lib.LOOP_BATCH_MAX_CAP
    out["engine"] = {k: (out[k][0] if all(v == out[k][0] for v in out[k]) else list(out[k])) for k in ("sig_t", "sig_r", "pen_max", "floor", "softmax")}
    return out


def sweep_stats(records, times, host_times, **fixed) -> dict:
    """One row's `filter_stats` (filter.py:99-116, the keys `filter` returns) from its frame-log records and the batch frames'
    periods - both cut to the row's own frames by the caller; fixed: the entries that do not depend on the frames."""
    n = len(records)
    times, host_times = [float(t) for t in times[:n]], [float(t) for t in host_times[:n]]
    stats = dict(fixed)
    stats.update(rmse_t=[rec["rmse_t"] for rec in records], rmse_r=[rec["rmse_r"] for rec in records], time=times,
                 cluster_poses=[torch.as_tensor(rec["cluster_poses"]) for rec in records],
                 cluster_stds=[torch.as_tensor(rec["cluster_stds"]) for rec in records],
                 num_particles=[rec["n_after"] for rec in records], traj_size=n)
    stats["total_time"] = sum(times)
    stats["avg_time"] = stats["total_time"] / max(n, 1)
    stats["avg_timer"] = {"tactile": 0.0, "motion": 0.0, "meas": stats["avg_time"],
                          "host_enqueue": float(np.average(host_times)) if host_times else 0.0}
    stats["frames"], stats["frame_idx"], stats["host_time"] = records, list(range(n)), host_times
    return stats


def sweep_inputs(runs, plan, device):
    """The frames of every row, time-major and built once - (T_max, B, 4, 4) odometry, (T_max, B, D) tactile codes, (T_max, B, 4, 4)
    ground truth - so that a frame's operands are slices.  Odometry is `filter`'s: identity on the frames the filter starts from,
    inv(meas[t-1]) @ meas[t] behind them.  A row whose log has ended goes on with identity odometry, its last code and its last gt."""
    T_max, per_run = plan["T_max"], []
    for seq, T in zip(runs, plan["run_lengths"]):
        meas_p = seq.meas_p.to(device)
        odom = torch.eye(4, device=device).repeat(T_max, 1, 1)
        if T > 2:  # (exactly filter()'s products: the whole log's, then cut)
            odom[2:T] = torch.matmul(torch.linalg.inv(meas_p)[:-1], meas_p[1:])[1:T - 1]
        last = torch.full((T_max - T,), T - 1, dtype=torch.long, device=device)
        pick = torch.cat([torch.arange(T, device=device), last])
        per_run.append((odom, seq.codes.to(device, torch.float64)[pick], seq.gt_p.to(device, torch.float32)[pick]))
    rows = plan["row_run"]
    return tuple(torch.stack([per_run[r][i] for r in rows], dim=1).contiguous() for i in range(3))


def filter_sweep(cfg, runs, *, trials: int = 1, seed: int = 4000, device=None, max_frames: int = None, cluster: bool = True,
                 cluster_every: int = 50, softmax=True, update_freq=1, floor=1000,
                 results_root: Optional[str] = None, draws: str = "device", resample: str = "weighted_random",
                 centers: str = "quat_avg") -> list:
    """The reference's experiment - `bash/run_filter.sh`: objects x logs x trials, one `filter/filter.py` process each - as ONE batch
    on the device: every (run, trial) is a row of a `BatchLoopEngine.for_objects`, a frame of all rows is one `step()`.

    runs: a list of `Sequence`; runs that share one `codebook` object stand on one object of the batch.  Row r * trials + k is run r,
    trial k, on the Philox streams of seed + row: it holds, frame for frame, what `filter(run_cfg, runs[r], seed=seed + row,
    start="device", softmax=..., floor=..., update_freq=..., cluster_every=..., resample=..., centers=...)` computes.  run_cfg is the run's own `Sequence.cfg`
    (None: `cfg`): a run takes its dataset's noise_t, noise_r, num_particles, noise_ratio and pen.max from it - config/expt/ycb.yaml
    and mcmaster.yaml in one sweep; the batch's capacity is the largest count, wide beyond 16 384.  softmax, floor and update_freq are
    each one value or one per run - `filter` and `filter_real`'s presets as rows of one batch.  Rows that differ in any of these go
    through the engine's per-row parameter table (two uploads a sweep: the still and the moving frames); eps, the DBSCAN cadence and
    the resample mode (`resample`, as `filter`'s) stay the sweep's.  Pace is fixed: frame t of every row is frame t of its log.  Rows start on the device on the frames
    seen while prev_idx == 0 (frames 0 and 1, filter.py:152-160; `BatchLoopEngine.start`); DBSCAN runs on every cluster_every-th
    frame, the measurement update on every update_freq-th (unit weights in between, filter_real.py:205-212).  Logs of different
    lengths: a row whose log has ended is stepped on (identity odometry, its last code and gt) and its surplus frames are never read
    - not their results, not their condition bits; a condition inside a row's own frames raises as in `filter`.
    -> one `filter_stats` dict per row (`filter`'s keys; `time` is the batch frame's period on the device's clock) with
    `batch_rows`, `trial_id` = k and `log_id` = the run's `Sequence.log_id` (None: cfg.expt.log_id); with results_root each is saved to
    `<results_root>/<obj>/<log>/trial_<kk>/filter_stats.npy` (filter.py:252).
    draws: "device" only - a seeded sweep would need one host generator per row through `init_filter`."""
    import gc
    import os

    from .batch_loop_engine import BatchLoopEngine
    from .loop_engine import log_records

    if draws != "device":
        raise ValueError(f"filter_sweep draws on the device (draws='device'), not {draws!r}: a seeded sweep needs a host generator "
                         "per row through init_filter, which is out of its scope - run filter(draws='seeded') per row")
    expt_cfg = cfg.expt
    runs = list(runs)
    plan = sweep_plan(runs, trials, expt_cfg.max_length, max_frames)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    rp = sweep_row_params(cfg, runs, plan, softmax, floor, update_freq)
    cluster_every = max(int(cluster_every), 1)
    B, T_max = len(plan["row_run"]), plan["T_max"]

    pfs = []
    for r, seq in enumerate(runs):  # one particle_filter per RUN, deliberately, where one per object did before: init_noise (the mesh's
        # diagonal x the run's noise_ratio), pen_max and log_id follow the run's own cfg.  Runs of one object repeat the mesh's host-side
        # set-up (vertices, diagonal: no device work); the mesh tree is asked of an object's first run only.  Same results.
        pf = particle_filter(rp["run_cfgs"][r], seq.mesh_vertices, rp["run_cfgs"][r].expt.params.noise_ratio, downsample=1, device=device)
        if seq.mesh_tree is not None:
            pf._mesh_tree = seq.mesh_tree
        pfs.append(pf)
    eng = BatchLoopEngine.for_objects([(runs[r].codebook, None, pfs[r].mesh_kdtree) for r in plan["objects"]],
                                      plan["row_object"], rp["capacity"], seed=seed, cluster=cluster, cluster_every=cluster_every,
                                      log_frames=max(T_max + 8, 64), device=device, wide=rp["wide"], resample=resample, centers=centers,
                                      **rp["engine"])
    odoms, codes, gts = sweep_inputs(runs, plan, device)
    init_noise = torch.tensor([pfs[r].init_noise for r in plan["row_run"]], dtype=torch.float32, device=device)
    counts = rp["num_particles"]
    shared_freq = rp["update_freq"][0] if len(set(rp["update_freq"])) == 1 else None

    events = [torch.cuda.Event(enable_timing=True)]
    host_times = []
    gc.collect()
    gc.freeze()  # (as in filter)
    try:
        events[0].record()
        for t in range(T_max):
            t0 = time.time()
            starting = t < 2  # prev_idx == 0 (filter.py:152): frames 0 and 1 re-initialise
            if starting:
                eng.start(gts[t], init_noise, n=counts, reset_annealing=t == 0)
            # (the reference does not call motionModel on the starting frames: no motion noise there)
            unit = t % shared_freq != 0 if shared_freq is not None else [t % f != 0 for f in rp["update_freq"]]
            (eng.step_still if starting else eng.step)(odoms[t], codes[t], gts=gts[t], dbscan=cluster and t % cluster_every == 0,
                                                       unit_weights=unit)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
            host_times.append(time.time() - t0)
        torch.cuda.synchronize(device)
    finally:
        gc.unfreeze()
    times = [e0.elapsed_time(e1) * 1e-3 for e0, e1 in zip(events, events[1:])]
    log = eng._log.cpu().numpy()  # one read-back; every row is parsed up to its own last frame only
    out = []
    for row, (r, k, T) in enumerate(zip(plan["row_run"], plan["row_trial"], plan["lengths"])):
        seq, pf = runs[r], pfs[r]
        stats = sweep_stats(log_records(log[row], 0, T, who=f"row {row}, "), times[:T], host_times[:T], obj_name=seq.obj_model,
                            tree_size=len(seq.codebook), noise_ratio=rp["noise_ratio"][row], init_noise=pf.init_noise,
                            init_particles=counts[row], log_id=_log_id(seq, rp["run_cfgs"][r].expt), trial_id=k, batch_rows=B)
        if results_root is not None:
            save_filter_stats(stats, os.path.join(results_root, str(seq.obj_model), stats["log_id"], f"trial_{k:02d}"))
        out.append(stats)
    return out


def main(argv=None):
    import sys

    from .config import load_config

    cfg = load_config(list(sys.argv[1:] if argv is None else argv))
    stats = filter(cfg, progress=True, results_path=".")
    print(f"Total time: {stats['total_time']:.3f}, Per iteration time: {stats['avg_time']:.4f}")
    t = stats["avg_timer"]
    print(f'Avg time: tactile: {t["tactile"]:.2f}, motion : {t["motion"]:.2f}, meas : {t["meas"]:.2f} ')


if __name__ == "__main__":
    main()
