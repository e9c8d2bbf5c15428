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
--objects G: the rows stand on G synthetic objects (K, D as above; row b on object b G // B, an object's rows side by side) - BatchLoopEngine.for_objects, one launch set
  for the mixed batch (midas_loop_step_batch_objects).  Forms, each selectable alone with --form=NAME (a process per form, to alternate):
  objects_mixed   the for_objects engine, B rows over the G objects per frame
  objects_split   how a sweep over objects ran before: G plain BatchLoopEngines of the rows of one object each (B / G), stepped one
                  after the other - a frame is all G steps; engine i is seeded with its first row's key, so every row replays its row of
                  the mixed batch (compare n_final_min / n_final_max).  It uses the plain constructor only: to take the figure on an
                  earlier commit, copy this file into that checkout's tools/ and run it there with --form=objects_split
  single_object   one plain BatchLoopEngine of the same B with every row on object 0 (what G codebooks cost beside one)
  objects_rows    objects_mixed with the filter's parameters per row (midas_loop_step_batch_rows), the SAME values in every row: the same
                  work, so the difference to objects_mixed is the cost of the parameter table (--form=objects_rows only)
--resample=MODE: the engines' resample mode (weighted_random by default; low_var: the systematic resampler - with --seeded its one
  float32 offset per row and frame in place of n_set float64 uniforms).
--centers=METHOD: the form of the frames' cluster centres (quat_avg by default; logmap: the log-map centres, MIDAS_LOOP_CENTERS_LOGMAP)
  in every loop engine form.
--profile: frames of the batch engine only (for rocprofv3 --kernel-trace --stats; with --seeded the seeded batch, with --objects the mixed
  batch, with --form=NAME that form), no timing."""
import json
import os
import statistics
import sys
import time

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
G, FORM = 0, None
if "--objects" in args:  # `--objects G`, as --dbscan
    i = args.index("--objects")
    args[i:i + 2] = ["--objects=" + (args[i + 1] if i + 1 < len(args) else "")]
for a in args:
    if a.startswith("--objects="):
        G = int(a.split("=", 1)[1])
    if a.startswith("--form="):
        FORM = a.split("=", 1)[1]
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
if G and (seeded or G < 1 or G > B):
    sys.exit("bench_batch_loop.py: --objects G with 1 <= G <= B, Philox draws")
dev = torch.device("cuda", 0)
NAMES = ("004_sugar_box", "035_power_drill", "025_mug", "cotter-pin")
cbs = [make_codebook(NAMES[i % len(NAMES)], K=K, D=D, seed=1000 + i) for i in range(max(G, 1))]
cb, ROW_OBJ = cbs[0], [b * max(G, 1) // B for b in range(B)]  # (an object's rows side by side: a plain engine seeded with the first replays them)
trajs = [make_trajectory(cbs[ROW_OBJ[b]], T=T + 1, seed=2000 + b) for b in range(B)]
odoms = torch.as_tensor(np.stack([tr.odoms for tr in trajs], axis=1)).to(dev)            # (T + 1, B, 4, 4)
codes = torch.as_tensor(np.stack([tr.codes for tr in trajs], axis=1)).to(dev)            # (T + 1, B, D)
gts = torch.as_tensor(np.stack([tr.gt_poses for tr in trajs], axis=1)).to(dev, torch.float32)
starts = torch.as_tensor(np.stack([wide_start(cbs[ROW_OBJ[b]].extents, trajs[b].gt_poses[0], N0, 3000 + b) for b in range(B)])).to(dev, torch.float32)
kw = dict(floor=FLOOR, cluster_every=EVERY, device=dev)
for a in sys.argv[1:]:
    if a.startswith("--resample="):
        kw["resample"] = a.split("=", 1)[1]
    if a.startswith("--centers="):
        kw["centers"] = a.split("=", 1)[1]
SYSTEMATIC = kw.get("resample", "weighted_random") != "weighted_random"  # (a seeded systematic engine: seed_torch_stream_low_var)
HOST_US = None  # of the latest timed() run


def timed(step, frames):
    """ms of every frame by events around its enqueue (the stream is idle at the start, the frames queue behind each other)."""
    global HOST_US
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(frames + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    t0 = time.perf_counter()
    for t in range(frames):
        step(t)
        ev[t + 1].record()
    HOST_US = round(1e6 * (time.perf_counter() - t0) / frames, 2)  # the host's time to enqueue a frame (and record its event)
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
        (eng.seed_torch_streams_low_var if SYSTEMATIC else eng.seed_torch_streams)(seeds)
    eng.set_particles(starts)
    eng.project_to_codebook()
    ms = timed(lambda t: eng.step(odoms[t + 1], codes[t + 1], gts=gts[t + 1]), T)
    n = eng.n
    return ms, {"n_final_min": min(n), "n_final_max": max(n)}


def run_single(seed=None):
    eng = LoopEngine(cb.poses, cb.embeddings, cb.mesh_vertices, N0, seed=SEED, topk_ties="index" if seed is None else "aten_cpu", **kw)
    if seed is not None:
        (eng.seed_torch_stream_low_var if SYSTEMATIC else eng.seed_torch_stream)(seed)
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


def triple(c):
    return (c.poses, c.embeddings, c.mesh_vertices)


def run_objects_mixed(per_row=False):
    rows_kw = dict(floor=[FLOOR] * B, sig_t=[2e-4] * B, sig_r=[0.5] * B, pen_max=[0.002] * B, softmax=[True] * B) if per_row else {}
    eng = BatchLoopEngine.for_objects([triple(c) for c in cbs], ROW_OBJ, N0, seed=SEED, batched_dbscan=DBSCAN, **{**kw, **rows_kw},
                                      **({"wide": True} if wide else {}))
    eng.set_particles(starts)
    eng.project_to_codebook()
    ms = timed(lambda t: eng.step(odoms[t + 1], codes[t + 1], gts=gts[t + 1]), T)
    n = eng.n
    return ms, {"n_final_min": min(n), "n_final_max": max(n), "host_enqueue_us": HOST_US, **({"row_table_uploads": eng.row_table_uploads} if per_row else {})}


def run_objects_rows():
    return run_objects_mixed(per_row=True)


def run_objects_split():
    rows = [torch.as_tensor([b for b in range(B) if ROW_OBJ[b] == i], device=dev) for i in range(G)]
    # (engine i's row j is row rows[i][0] + j of the mixed batch: the same Philox key, the same trajectory, the same live counts)
    engs = [BatchLoopEngine(*triple(cbs[i]), len(rows[i]), N0, seed=SEED + int(rows[i][0]), batched_dbscan=DBSCAN, **kw, **({"wide": True} if wide else {}))
            for i in range(G)]
    ops = [(odoms[:, r].contiguous(), codes[:, r].contiguous(), gts[:, r].contiguous()) for r in rows]
    for e, r in zip(engs, rows):
        e.set_particles(starts[r])
        e.project_to_codebook()

    def step(t):
        for e, (o, c, g) in zip(engs, ops):
            e.step(o[t + 1], c[t + 1], gts=g[t + 1])
    ms = timed(step, T)
    n = [v for e in engs for v in e.n]
    return ms, {"n_final_min": min(n), "n_final_max": max(n), "engines": G}


def run_single_object():
    tr = [make_trajectory(cb, T=T + 1, seed=2000 + b) for b in range(B)]
    o, c, g = (torch.as_tensor(np.stack([getattr(x, k) for x in tr], axis=1)).to(dev) for k in ("odoms", "codes", "gt_poses"))
    st = torch.as_tensor(np.stack([wide_start(cb.extents, tr[b].gt_poses[0], N0, 3000 + b) for b in range(B)])).to(dev, torch.float32)
    eng = BatchLoopEngine(*triple(cb), B, N0, seed=SEED, batched_dbscan=DBSCAN, **kw, **({"wide": True} if wide else {}))
    eng.set_particles(st)
    eng.project_to_codebook()
    ms = timed(lambda t: eng.step(o[t + 1], c[t + 1], gts=g[t + 1].float()), T)
    n = eng.n
    return ms, {"n_final_min": min(n), "n_final_max": max(n)}


def run_batch_seeded():
    return run_batch([SEED + b for b in range(B)])


def run_single_seeded():
    return run_single(SEED)


head = {"B": B, "N0": N0, "K": K, "D": D, "floor": FLOOR, "cluster_every": EVERY, "frames": T, "repeats": R, **({"wide": True} if wide else {}),
        **({} if DBSCAN is None else {"dbscan": "batched" if DBSCAN else "serial"}), **({"objects": G} if G else {}),
        **({"resample": kw["resample"]} if "resample" in kw else {}), **({"centers": kw["centers"]} if "centers" in kw else {})}
out = {}
forms = (("batch_loop", run_batch), ("single_loop", run_single), ("pipelined_fixed", run_fixed))
if wide:
    forms = forms[:2]
if seeded:
    forms = (("batch_loop_seeded", run_batch_seeded), ("single_loop_seeded", run_single_seeded), ("batch_loop", run_batch))
if G:
    forms = (("objects_mixed", run_objects_mixed), ("objects_split", run_objects_split), ("single_object", run_single_object))
if FORM is not None:
    forms = tuple(f for f in forms + ((("objects_rows", run_objects_rows),) if G else ()) if f[0] == FORM)
    if not forms:
        sys.exit(f"bench_batch_loop.py: no form {FORM!r} in this mode")
if profile:  # (the first form: the batch engine of the mode, or the one --form names)
    forms[0][1]()
    torch.cuda.synchronize()
    sys.exit(0)
for name, run in forms:
    run()  # warm-up: code objects, scratch, allocator
    rows, extra = [], {}
    for _ in range(R):
        ms, extra = run()
        rows.append(summary(ms))
    out[name] = over_repeats(rows)
    print(json.dumps({"form": name, **head, **out[name], **extra, "per_repeat": rows}), flush=True)
if G and FORM is None:
    mixed, split, one_obj = (out[k]["frame_median_us"]["median"] for k in ("objects_mixed", "objects_split", "single_object"))
    print(json.dumps({"form": "comparison_objects", **head, "mixed_frame_us": mixed, "split_frame_us": split, "single_object_frame_us": one_obj,
                      "split_over_mixed": round(split / mixed, 3), "mixed_over_single_object": round(mixed / one_obj, 3)}), flush=True)
if G or FORM is not None:
    sys.exit(0)
one, batch = (out["single_loop_seeded"], out["batch_loop_seeded"]) if seeded else (out["single_loop"], out["batch_loop"])
print(json.dumps({"form": "comparison_seeded" if seeded else "comparison", **head,
                  "B_single_frames_us": round(B * one["frame_median_us"]["median"], 1),
                  "batch_frame_us": batch["frame_median_us"]["median"],
                  "speedup_frame": round(B * one["frame_median_us"]["median"] / batch["frame_median_us"]["median"], 2),
                  "B_single_dbscan_frames_us": round(B * one["dbscan_frame_median_us"]["median"], 1),
                  "batch_dbscan_frame_us": batch["dbscan_frame_median_us"]["median"],
                  "speedup_dbscan_frame": round(B * one["dbscan_frame_median_us"]["median"] / batch["dbscan_frame_median_us"]["median"], 2)}), flush=True)
