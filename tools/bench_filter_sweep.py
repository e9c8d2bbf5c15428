#!/usr/bin/env python3
"""The reference's experiment (bash/run_filter.sh: objects x logs x trials) as one `filter_sweep` against the same runs as `filter()`
calls in turn, and the start of such a batch on the device against the host route.

usage: bench_filter_sweep.py --form=NAME [G [B [N0 [K [T [repeats]]]]]]   (10 objects, 50 rows, 10000 particles, K = 50000, 300 frames,
3 repeats; D = 512, floor 1000, DBSCAN every 50th frame; B / G logs per object, one trial each).  One process per form, so that forms
and commits can be alternated; one JSON line with each figure's median over the repeats and [min, max]:
  sweep         filter_sweep over the B runs: wall seconds of the call, median of the batch frame's period, mean of the first two
                (the starting) frames
  filter_runs   filter() on each of the B runs in turn (seed + row): wall seconds of all B calls, median frame.  --start=device: with
                filter(start="device").  It uses nothing newer than filter() itself: to take the figure on an earlier commit, copy this
                file into that checkout's tools/ and run it there
  sweep_mixed   two datasets in ONE sweep: the first G / 2 objects' runs under a ycb-like config (N0 particles, noise_t 2e-4), the others'
                under a mcmaster-like one (N0 / 2 particles, or --nb=N of them; noise_t 1e-4) through `Sequence.cfg` - the rows take their parameters from
                the engine's per-row table
  sweep_split   the same runs as two sweeps in turn, one per config - what the two datasets cost before (works on an earlier commit, as
                filter_runs does): wall seconds of both calls, the moving-frame median of each
  start_device  BatchLoopEngine.start() of the B rows: wall milliseconds of the call with the device drained behind it
  start_host    the host route for the same rows: init_filter per row, set_particles, project_to_codebook (works on an earlier commit, as
                filter_runs does)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from midastouch_amd import BatchLoopEngine, ops
from midastouch_amd import filter as runner
from midastouch_amd.config import load_config
from midastouch_amd.particle_filter import particle_filter
from midastouch_amd.synthetic import make_codebook, make_trajectory
from midastouch_amd.tactile_tree import tactile_tree

FORM, START, NB = None, "host", None
for a in sys.argv[1:]:
    if a.startswith("--nb="):
        NB = int(a.split("=", 1)[1])
    if a.startswith("--form="):
        FORM = a.split("=", 1)[1]
    if a.startswith("--start="):
        START = a.split("=", 1)[1]
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
G, B, N0, K, T, R = (int(argv[i]) if len(argv) > i else d for i, d in enumerate((10, 50, 10000, 50000, 300, 3)))
D, FLOOR, SEED = 512, 1000, 4000
if FORM not in ("sweep", "filter_runs", "sweep_mixed", "sweep_split", "start_device", "start_host") or B % G:
    sys.exit("bench_filter_sweep.py --form=sweep|filter_runs|sweep_mixed|sweep_split|start_device|start_host [G B N0 K T repeats], G dividing B")
dev = torch.device("cuda", 0)
NAMES = ("004_sugar_box", "035_power_drill", "025_mug", "cotter-pin")
cfg = load_config([f"expt.params.num_particles={N0}"])
runs = []
for i in range(G):
    cb = make_codebook(NAMES[i % len(NAMES)], K=K, D=D, seed=1000 + i)
    tt = tactile_tree(torch.as_tensor(cb.poses), torch.as_tensor(cb.cam_poses), torch.as_tensor(cb.embeddings))
    tt.to_device(dev)
    mesh = ops.Tree(torch.as_tensor(cb.mesh_vertices).to(dev, torch.float64))
    for j in range(B // G):
        tr = make_trajectory(cb, T=T, seed=2000 + i * (B // G) + j)
        seq = runner.Sequence(torch.as_tensor(tr.gt_poses).to(dev), torch.as_tensor(tr.meas_poses).to(dev), torch.as_tensor(tr.codes).to(dev), tt,
                              cb.mesh_vertices, cb.obj_model, mesh_tree=mesh)
        seq.log_id = j  # (a plain attribute where Sequence has no such field yet)
        runs.append(seq)


def spread(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def frames_us(stats):
    """Median period of the moving frames and mean of the two starting frames, over all the given runs."""
    rest = [1e6 * v for s in stats for t, v in enumerate(s["time"]) if t >= 2 and t % 50]
    first = [1e6 * v for s in stats for v in s["time"][:2]]
    return round(statistics.median(rest), 2), round(statistics.fmean(first), 2)


def form_sweep():
    w, stats = wall(lambda: runner.filter_sweep(cfg, runs, seed=SEED, device=dev, floor=FLOOR))
    med, first = frames_us(stats[:1])  # (every row carries the batch frame's periods)
    return {"wall_s": round(w, 4), "frame_median_us": med, "start_frame_mean_us": first}


def form_filter_runs():
    kw = {"start": START} if START != "host" else {}
    w, stats = wall(lambda: [runner.filter(cfg, seq, device=dev, seed=SEED + row, floor=FLOOR, **kw) for row, seq in enumerate(runs)])
    med, first = frames_us(stats)
    return {"wall_s": round(w, 4), "frame_median_us": med, "start_frame_mean_us": first}


# the two datasets of sweep_mixed / sweep_split: the runs of the first G / 2 objects and of the others
HALF = (G // 2) * (B // G)
CFG_B = load_config(["expt=mcmaster", f"expt.params.num_particles={N0 // 2 if NB is None else NB}"])


def form_sweep_mixed():
    for row, seq in enumerate(runs):
        seq.cfg = cfg if row < HALF else CFG_B
    w, stats = wall(lambda: runner.filter_sweep(cfg, runs, seed=SEED, device=dev, floor=FLOOR))
    med, first = frames_us(stats[:1])
    return {"wall_s": round(w, 4), "frame_median_us": med, "start_frame_mean_us": first}


def form_sweep_split():
    w, (a, b) = wall(lambda: (runner.filter_sweep(cfg, runs[:HALF], seed=SEED, device=dev, floor=FLOOR),
                              runner.filter_sweep(CFG_B, runs[HALF:], seed=SEED + HALF, device=dev, floor=FLOOR)))
    (med_a, _), (med_b, _) = frames_us(a[:1]), frames_us(b[:1])
    return {"wall_s": round(w, 4), "frame_median_us": round(med_a + med_b, 2), "frame_median_a_us": med_a, "frame_median_b_us": med_b}


def start_engine():
    objs, pfs = [], []
    for i in range(G):
        seq = runs[i * (B // G)]
        pf = particle_filter(cfg, seq.mesh_vertices, cfg.expt.params.noise_ratio, downsample=1, device=dev)
        pf._mesh_tree = seq.mesh_tree
        pfs.append(pf)
        objs.append((seq.codebook, None, seq.mesh_tree))
    rows = [b * G // B for b in range(B)]
    eng = BatchLoopEngine.for_objects(objs, rows, N0, seed=SEED, floor=FLOOR, device=dev)
    return eng, pfs, rows


def form_start_device():
    eng, pfs, rows = start_engine()
    gts = torch.stack([seq.gt_p[0] for seq in runs])
    sig = torch.tensor([pfs[i].init_noise for i in rows], dtype=torch.float32, device=dev)
    eng.start(gts, sig, n=N0)  # warm-up: code objects
    w, _ = wall(lambda: eng.start(gts, sig, n=N0, reset_annealing=True))
    return {"wall_ms": round(1e3 * w, 3)}


def form_start_host():
    eng, pfs, rows = start_engine()

    def start():
        eng.set_particles([pfs[i].init_filter(seq.gt_p[0], N0).poses for i, seq in zip(rows, runs)])
        eng.project_to_codebook()
    start()  # warm-up
    w, _ = wall(start)
    return {"wall_ms": round(1e3 * w, 3)}


run = {"sweep": form_sweep, "filter_runs": form_filter_runs, "sweep_mixed": form_sweep_mixed, "sweep_split": form_sweep_split,
       "start_device": form_start_device, "start_host": form_start_host}[FORM]
if FORM.startswith("sweep"):
    run()  # warm-up: code objects, scratch, allocator
if FORM == "filter_runs":
    runner.filter(cfg, runs[0], device=dev, seed=SEED, floor=FLOOR, **({"start": START} if START != "host" else {}))  # (the same)
rows_ = [run() for _ in range(R)]
head = {"form": FORM + ("_device_start" if FORM == "filter_runs" and START == "device" else ""), "G": G, "B": B, "N0": N0, "K": K, "D": D,
        "floor": FLOOR, "frames": T, "repeats": R}
print(json.dumps({**head, **{k: spread([r[k] for r in rows_]) for k in rows_[0]}, "per_repeat": rows_}), flush=True)
