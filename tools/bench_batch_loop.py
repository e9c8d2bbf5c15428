#!/usr/bin/env python3
"""Batch frame of BatchLoopEngine (midas_loop_step_batch: B clustering and annealing filters per set of launches) against what the
same trajectories cost one after the other: B x the frame of a single LoopEngine with the same settings.

usage: bench_batch_loop.py [B [N0 [K [T [repeats]]]]]   (64, 10000, 50000, 300 frames, 3 repeats; D = 512, floor 1000, DBSCAN
every 50th frame).  Every frame is bracketed by device events.  Per repeat: median and mean of the DBSCAN frames and of the others.
One JSON line per engine form with each figure's median over the repeats and [min, max]:
  batch_loop      BatchLoopEngine, B trajectories per frame
  single_loop     one LoopEngine on trajectory 0 (seed + 0) - and B x its median frame, the figure the batch frame has to beat
  pipelined_fixed PipelinedBatchFilterEngine at the same B and N0: the fixed-N frame without clustering or annealing (orientation)
--seeded: the seeded forms instead - B runs of the reference under torch.manual_seed(s + b), ATen's tie rule:
  batch_loop_seeded   BatchLoopEngine.seed_torch_streams (midas_loop_step_batch_draws, the draws sized on the device per trajectory)
  single_loop_seeded  one LoopEngine(topk_ties="aten_cpu").seed_torch_stream on trajectory 0 - B x its frame is what the sweep cost before
  batch_loop          the Philox batch frame (orientation: the seeded batch frame should sit near it plus one seeded single frame)
--wide: BatchLoopEngine(wide=True) (midas_loop_step_batch_wide: sets beyond 16 384 particles per trajectory, e.g. 16 50000) against B single
  LoopEngine frames; --floor=N: annealing's floor (default 1000).  The fixed-N form is left out.
--dbscan serial|batched: the batch engine's DBSCAN frame as B passes one after the other (batched_dbscan=False) or as the one batched pass
  (batched_dbscan=True; B x N0 <= 2^20); default: the engine's own choice (batched whenever it fits).
--profile: frames of the batch engine only (for rocprofv3 --kernel-trace --stats; with --seeded the seeded batch), no timing."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from midastouch_amd import BatchLoopEngine
from midastouch_amd.engine import PipelinedBatchFilterEngine
from midastouch_amd.loop_engine import LoopEngine
from midastouch_amd.synthetic import make_codebook, make_trajectory, wide_start

DBSCAN = None  # BatchLoopEngine(batched_dbscan=...): None = the engine's choice
args = sys.argv[1:]
if "--dbscan" in args:  # `--dbscan VALUE`: taken out with its value, so that the value is no positional argument
    i = args.index("--dbscan")
    args[i:i + 2] = ["--dbscan=" + (args[i + 1] if i + 1 < len(args) else "")]
for a in args:
    if a.startswith("--dbscan="):
        if a.split("=", 1)[1] not in ("serial", "batched"):
            sys.exit("bench_batch_loop.py: --dbscan serial|batched")
        DBSCAN = a.split("=", 1)[1] == "batched"
argv = [a for a in args if not a.startswith("--")]
profile, seeded, wide = "--profile" in sys.argv, "--seeded" in sys.argv, "--wide" in sys.argv
B, N0, K, T, R = (int(argv[i]) if len(argv) > i else d for i, d in enumerate((64, 10000, 50000, 300, 3)))
D, FLOOR, EVERY, SEED = 512, 1000, 50, 4000
if wide and seeded:
    sys.exit("bench_batch_loop.py: --wide and --seeded exclude each other (a wide BatchLoopEngine draws from Philox: seed_torch_streams raises on it)")
for a in sys.argv[1:]:
    if a.startswith("--floor="):
        FLOOR = int(a.split("=", 1)[1])
dev = torch.device("cuda", 0)
cb = make_codebook(K=K, D=D, seed=1000)
trajs = [make_trajectory(cb, T=T + 1, seed=2000 + b) for b in range(B)]
odoms = torch.as_tensor(np.stack([tr.odoms for tr in trajs], axis=1)).to(dev)            # (T + 1, B, 4, 4)
codes = torch.as_tensor(np.stack([tr.codes for tr in trajs], axis=1)).to(dev)            # (T + 1, B, D)
gts = torch.as_tensor(np.stack([tr.gt_poses for tr in trajs], axis=1)).to(dev, torch.float32)
starts = torch.as_tensor(np.stack([wide_start(cb.extents, trajs[b].gt_poses[0], N0, 3000 + b) for b in range(B)])).to(dev, torch.float32)
kw = dict(floor=FLOOR, cluster_every=EVERY, device=dev)


def timed(step, frames):
    """ms of every frame by events around its enqueue (the stream is idle at the start, the frames queue behind each other)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(frames + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for t in range(frames):
        step(t)
        ev[t + 1].record()
    torch.cuda.synchronize()
    return [ev[t].elapsed_time(ev[t + 1]) for t in range(frames)]


def summary(ms):
    db = [v for t, v in enumerate(ms) if t % EVERY == 0]
    rest = [v for t, v in enumerate(ms) if t % EVERY != 0]
    us = lambda v: round(1e3 * v, 2)  # noqa: E731
    return {"frame_median_us": us(statistics.median(rest)), "frame_mean_us": us(statistics.fmean(rest)),
            "dbscan_frame_median_us": us(statistics.median(db)), "dbscan_frame_mean_us": us(statistics.fmean(db))}


def over_repeats(rows):
    return {k: {"median": statistics.median(r[k] for r in rows), "min": min(r[k] for r in rows), "max": max(r[k] for r in rows)} for k in rows[0]}


def run_batch(seeds=None):
    eng = BatchLoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, seed=SEED, batched_dbscan=DBSCAN, **kw, **({"wide": True} if wide else {}))
    if seeds is not None:
        eng.seed_torch_streams(seeds)
    eng.set_particles(starts)
    eng.project_to_codebook()
    ms = timed(lambda t: eng.step(odoms[t + 1], codes[t + 1], gts=gts[t + 1]), T)
    n = eng.n
    return ms, {"n_final_min": min(n), "n_final_max": max(n)}


def run_single(seed=None):
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0, seed=SEED, topk_ties="index" if seed is None else "aten_cpu", **kw)
    if seed is not None:
        eng.seed_torch_stream(seed)
    eng.set_particles(starts[0])
    eng.project_to_codebook()
    ms = timed(lambda t: eng.step(odoms[t + 1, 0], codes[t + 1, 0], gt=gts[t + 1, 0]), T)
    return ms, {"n_final": eng.n}


def run_fixed():
    eng = PipelinedBatchFilterEngine(cb.poses, cb.embeddings, cb.mesh_vertices, B, N0, seed=SEED, device=dev)
    eng.set_particles(starts)
    eng.project_to_codebook()
    ms = timed(lambda t: eng.step(odoms[t + 1], codes[t + 1], gts=gts[t + 1]), T)
    eng.flush()
    return ms, {}


def run_batch_seeded():
    return run_batch([SEED + b for b in range(B)])


def run_single_seeded():
    return run_single(SEED)


if profile:
    (run_batch_seeded if seeded else run_batch)()
    torch.cuda.synchronize()
    sys.exit(0)

head = {"B": B, "N0": N0, "K": K, "D": D, "floor": FLOOR, "cluster_every": EVERY, "frames": T, "repeats": R, **({"wide": True} if wide else {}),
        **({} if DBSCAN is None else {"dbscan": "batched" if DBSCAN else "serial"})}
out = {}
forms = (("batch_loop", run_batch), ("single_loop", run_single), ("pipelined_fixed", run_fixed))
if wide:
    forms = forms[:2]
if seeded:
    forms = (("batch_loop_seeded", run_batch_seeded), ("single_loop_seeded", run_single_seeded), ("batch_loop", run_batch))
for name, run in forms:
    run()  # warm-up: code objects, scratch, allocator
    rows, extra = [], {}
    for _ in range(R):
        ms, extra = run()
        rows.append(summary(ms))
    out[name] = over_repeats(rows)
    print(json.dumps({"form": name, **head, **out[name], **extra, "per_repeat": rows}), flush=True)
one, batch = (out["single_loop_seeded"], out["batch_loop_seeded"]) if seeded else (out["single_loop"], out["batch_loop"])
print(json.dumps({"form": "comparison_seeded" if seeded else "comparison", **head,
                  "B_single_frames_us": round(B * one["frame_median_us"]["median"], 1),
                  "batch_frame_us": batch["frame_median_us"]["median"],
                  "speedup_frame": round(B * one["frame_median_us"]["median"] / batch["frame_median_us"]["median"], 2),
                  "B_single_dbscan_frames_us": round(B * one["dbscan_frame_median_us"]["median"], 1),
                  "batch_dbscan_frame_us": batch["dbscan_frame_median_us"]["median"],
                  "speedup_dbscan_frame": round(B * one["dbscan_frame_median_us"]["median"] / batch["dbscan_frame_median_us"]["median"], 2)}), flush=True)
