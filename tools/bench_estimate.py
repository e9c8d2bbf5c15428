#!/usr/bin/env python3
"""What the per-frame pose estimate of the fixed-N engines costs (`estimate=True`, midas_pose_estimate / midas_lazy_run_estimate).

Workloads:
  c2  PipelinedFilterEngine, N = 100 000 particles, K = 50 000 x D = 512 (the headline of bench.py);
  c5  PipelinedBatchFilterEngine, B = 64 trajectories x N = 10 000, cotter pin 50k x 512 (BASELINE config 5);
  s2  ShardedFilterEngine at c2's size on ONE GPU: world 1 under a one-rank nccl group, exchange "peer_c" (the whole frame by one
      C call on the library's communicator), step() and run().  Column c is the only route a caller had before the keyword:
      all_gather of poses_prop and weights over the group, then one ops.cluster_centers.  (`--configs s2` only: not in the default.)
  finish  no timing of its own: `--frames` launches of the fixed-N finish (ops.pose_estimate) and of the sharded engine's finish
      (midas_shard_estimate_moments / _finish) on one trajectory of 1 000 000, 100 000 and 10 240 particles (3907, 391 and 40
      blocks) - to be run under `rocprofv3 --kernel-trace --stats`, which gives the kernels' own times.
Three columns, us per (batch) frame over `--frames` frames after `--warmup`, device events around the whole run as bench.py
takes them, median of `--repeats` with min / max, the columns interleaved inside every repeat:
  a  estimate=False;
  b  estimate=True;
  c  estimate=False and, after each step(), one ops.cluster_centers per trajectory on eng.poses_prop / eng.weights - what a caller
     could do before the keyword existed (reading `weights` flushes the pipelined engine).
Column c has no run() form: for c2 the three columns are taken with step() calls, and a and b once more through run().

`--columns a,c` times a tree whose engines do not take the keyword yet; `--package-root DIR` imports midastouch_amd from DIR
(another build of the package) instead of from this tree.  One GPU process; run it under a timeout of its own."""
import argparse
import gc
import json
import os
import sys

import numpy as np


def spread(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def timed(torch, frames, body):
    """us per frame of frames x body(i) between two events on the current stream."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(frames):
        body(i)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / frames


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--columns", default="a,b,c")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--finish-sizes", default="1000000,100000,10240", help="particle counts of the `finish` workload (one per profiled run keeps the kernels' statistics apart)")
    ap.add_argument("--out", help="also write the result as JSON to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch

    from midastouch_amd import engine, ops
    from midastouch_amd.synthetic import make_codebook, make_trajectory, wide_start

    if not torch.cuda.is_available():
        raise SystemExit("bench_estimate.py: no HIP device - the figures are device times")
    dev = torch.device("cuda", 0)
    cols = [c for c in args.columns.split(",") if c]
    F, W = args.frames, args.warmup
    lab0 = torch.tensor([0], device=dev)
    result = {"package": os.path.dirname(os.path.abspath(engine.__file__)), "frames": F, "warmup": W, "repeats": args.repeats}

    def today(eng, zeros):
        """Column c's per-frame work: one cluster-centre call per trajectory on the engine's own tensors."""
        pp, w = eng.poses_prop, eng.weights
        if pp.dim() == 3:
            ops.cluster_centers(pp, w, zeros, lab0)
        else:
            for b in range(pp.shape[0]):
                ops.cluster_centers(pp[b], w[b], zeros, lab0)

    def measure(name, engines, start, step, runner=None, today=today):
        """engines: column -> engine; start(eng): the particle set of a repeat; step(eng, i): frame i; runner(eng, i0, n): n frames
        by one call; today(eng, zeros): column c's extra work per frame."""
        zeros = torch.zeros(next(iter(engines.values())).N, dtype=torch.int64, device=dev)
        us = {}
        for rep in range(args.repeats):
            for col, eng in engines.items():
                def frame(i, eng=eng, col=col, off=0):
                    step(eng, off + i)
                    if col == "c":
                        today(eng, zeros)
                start(eng)
                for i in range(W):
                    frame(i)
                us.setdefault(col + "_step", []).append(timed(torch, F, lambda i: frame(i, off=W)))
                if runner is not None and col != "c":
                    start(eng)
                    runner(eng, 0, W)
                    us.setdefault(col + "_run", []).append(timed(torch, 1, lambda i: runner(eng, W, F)) / F)
        result[name] = {k: spread(v) for k, v in us.items()}
        for k, v in result[name].items():
            print(f"{name} {k:7s} us/frame median {v['median']:9.2f}  min {v['min']:9.2f}  max {v['max']:9.2f}", flush=True)

    def build(cls, *a, **kw):
        return {col: cls(*a, **kw, **({"estimate": True} if col == "b" else {})) for col in cols}

    gc.collect()
    gc.disable()
    if "c2" in args.configs.split(","):
        N, K, D = 100_000, 50_000, 512
        cb = make_codebook("004_sugar_box", K=K, D=D, seed=1001)
        T = W + F + 2
        traj = make_trajectory(cb, T=T, seed=2001)
        od, co, gt = (torch.as_tensor(x).to(dev) for x in (traj.odoms, traj.codes, traj.gt_poses))
        p0 = torch.as_tensor(wide_start(cb.extents, traj.gt_poses[0], N, 100))
        engines = build(engine.PipelinedFilterEngine, cb.poses, cb.embeddings, cb.mesh_vertices, N, seed=4000, device=dev)

        def start(eng):
            eng.set_particles(p0)
            eng.project_to_codebook()

        measure("c2", engines, start, lambda eng, i: eng.step(od[1 + i], co[1 + i], gt=gt[1 + i]),
                lambda eng, i0, n: eng.run(od[1 + i0:1 + i0 + n], co[1 + i0:1 + i0 + n], gt[1 + i0:1 + i0 + n]))
        del engines
    if "c5" in args.configs.split(","):
        B, N, K, D = 64, 10_000, 50_000, 512
        cb = make_codebook("cotter-pin", K=K, D=D, seed=1005)
        trs = [make_trajectory(cb, T=W + F + 2, seed=2200 + b) for b in range(8)]  # (one continuous walk: no wrap-around inside a repeat)
        od = torch.as_tensor(np.stack([trs[b % 8].odoms for b in range(B)], axis=1)).to(dev)
        co = torch.as_tensor(np.stack([trs[b % 8].codes for b in range(B)], axis=1)).to(dev)
        rng = np.random.default_rng(1)
        near = []
        for b in range(B):  # a start near the truth (bench.py's c5 "near")
            d0 = np.linalg.norm(cb.poses[:, :3, 3] - trs[b % 8].gt_poses[0][:3, 3], axis=1)
            near.append(cb.poses[rng.choice(np.argsort(d0)[:2500], N)])
        p0 = torch.as_tensor(np.stack(near))
        engines = build(engine.PipelinedBatchFilterEngine, cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)

        def start5(eng):
            eng.set_particles(p0)
            eng.project_to_codebook()

        measure("c5", engines, start5, lambda eng, i: eng.step(od[1 + i], co[1 + i]))
    if "s2" in args.configs.split(","):
        import torch.distributed as dist

        from midastouch_amd.dist import ShardedFilterEngine
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:  # a free port of this host
            import socket
            with socket.socket() as sock:
                sock.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        N, K, D = 100_000, 50_000, 512
        cb = make_codebook("004_sugar_box", K=K, D=D, seed=1001)
        traj = make_trajectory(cb, T=W + F + 2, seed=2001)
        od, co, gt = (torch.as_tensor(x).to(dev) for x in (traj.odoms, traj.codes, traj.gt_poses))
        p0 = torch.as_tensor(wide_start(cb.extents, traj.gt_poses[0], N, 100))
        engines = build(ShardedFilterEngine, cb.poses, cb.embeddings, cb.mesh_vertices, N, seed=4000, device=dev, exchange="peer_c")
        def start_s(eng):
            eng.set_particles(p0)
            eng.project_to_codebook()

        def today_s(eng, zeros):  # today's route: gather every rank's particles and weights, then the cluster-centre call
            ops.cluster_centers(eng.comm.all_gather(eng.poses_prop), eng.comm.all_gather(eng.weights), zeros, lab0)

        measure("s2", engines, start_s, lambda eng, i: eng.step(od[1 + i], co[1 + i], gt=gt[1 + i]),
                lambda eng, i0, n: eng.run(od[1 + i0:1 + i0 + n], co[1 + i0:1 + i0 + n], gt[1 + i0:1 + i0 + n]), today=today_s)
        for eng in engines.values():
            eng.close()
        del engines
        dist.destroy_process_group()
    if "finish" in args.configs.split(","):
        from midastouch_amd import _lib
        ctx = _lib.context(dev)
        g = torch.Generator().manual_seed(5)
        for N in (int(v) for v in args.finish_sizes.split(",")):
            P = torch.eye(4).repeat(N, 1, 1)
            P[:, :3, 3] = 0.05 * torch.randn(N, 3, generator=g)
            P, w = P.to(dev).contiguous(), torch.rand(N, dtype=torch.float64, generator=g).to(dev)
            nb = -(-N // 256)
            part = torch.empty(nb * 36, dtype=torch.float64, device=dev)
            c, s = torch.empty((4, 4), dtype=torch.float32, device=dev), torch.empty(3, dtype=torch.float32, device=dev)
            for _ in range(W + F):
                old = ops.pose_estimate(P[None], w[None])
                ctx.call("midas_shard_estimate_moments", N, _lib._ptr(P), _lib._ptr(w), _lib._ptr(part))
                ctx.call("midas_shard_estimate_finish", nb, _lib._ptr(part), _lib._ptr(c), _lib._ptr(s))
            torch.cuda.synchronize()
            result.setdefault("finish", {})[str(nb)] = {"equal": bool(torch.equal(old[0][0], c) and torch.equal(old[1][0], s))}
            print(f"finish {nb} blocks: launched {W + F} pairs, results equal: {result['finish'][str(nb)]['equal']}", flush=True)
    gc.enable()
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
