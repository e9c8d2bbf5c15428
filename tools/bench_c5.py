#!/usr/bin/env python3
"""c5 (B=64 x N=10k, K=50k, D=512) batch-step time with particles spread over the object or started near the truth.
--scores dense_f64: BatchFilterEngine with the float64 dense pass on the matrix cores (midas_score_batch_f64).
--seeded {resample,all}: the step with every trajectory on its own seeded torch stream (seed_torch_streams; `all`: motion noise too)
against the unseeded step of the same run, the generator alone per frame (events on its stream, sequential walk and in pieces) and
the host alternative (B CPU generators drawing the frame's numbers, then the upload) - one JSON line."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from midastouch_amd.engine import BatchFilterEngine, PipelinedBatchFilterEngine
from midastouch_amd.synthetic import make_codebook, make_trajectory
dev = torch.device("cuda", 0)
cb = make_codebook("cotter-pin", K=50000, D=512, seed=1005)
B, N = 64, 10000
trs = [make_trajectory(cb, T=40, seed=2200 + b) for b in range(8)]
od = torch.as_tensor(np.stack([trs[b % 8].odoms for b in range(B)], axis=1)).to(dev)
co = torch.as_tensor(np.stack([trs[b % 8].codes for b in range(B)], axis=1)).to(dev)
SCORES = sys.argv[sys.argv.index("--scores") + 1] if "--scores" in sys.argv else "auto"
ENG = PipelinedBatchFilterEngine if os.environ.get("MIDAS_C5_PIPELINED", "1") != "0" and SCORES == "auto" else BatchFilterEngine
SEEDED = sys.argv[sys.argv.index("--seeded") + 1] if "--seeded" in sys.argv else None


def seeded_bench(motion):
    from midastouch_amd.torch_rng import TorchCpuStreams
    rng = np.random.default_rng(1)
    start = torch.as_tensor(np.stack([cb.poses[rng.integers(0, 50000, N)] for _ in range(B)]))
    seeds = [7000 + b for b in range(B)]
    res = {"metric": "c5_seeded", "seeded": SEEDED, "engine": ENG.__name__, "B": B, "N": N}

    def step_us(eng, T=60):
        eng.set_particles(start); eng.project_to_codebook()
        for i in range(10): eng.step(od[1 + i % 38], co[1 + i % 38])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(T): eng.step(od[1 + (10 + i) % 38], co[1 + (10 + i) % 38])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / T * 1e6

    res["unseeded_step_us"] = step_us(ENG(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev))
    for pieces in (0, 6):
        eng = ENG(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev)
        eng.seed_torch_streams(seeds, motion=motion, pieces=pieces)
        res[f"seeded_step_us_pieces{pieces}"] = step_us(eng)
    # the generator alone: one frame's walk, timed by events on its own stream
    spec = [("normal", 0.0, 1.0, (N, 3)), ("normal", 0.0, 1.0, (N, 3)), ("rand64", N)] if motion else [("rand64", N)]
    for pieces in (0, 6):
        st = TorchCpuStreams(seeds, dev, pieces=pieces)
        st.reserve(spec)
        for _ in range(5): st.draws_async(spec)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        T = 50
        e0.record(st.side)
        for _ in range(T): st.draws_async(spec)
        e1.record(st.side)
        e1.synchronize()
        res[f"generator_us_pieces{pieces}"] = e0.elapsed_time(e1) / T * 1e3
    # what a caller does without it: B host generators draw the frame, then the upload
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    T = 5
    t0 = time.perf_counter()
    for _ in range(T):
        tn, rot, u = [], [], []
        for g in gens:
            if motion:
                tn.append(torch.normal(0.0, 1e-4, size=(N, 3), generator=g)); rot.append(torch.normal(0.0, 0.5, size=(N, 3), generator=g))
            else:
                torch.normal(0.0, 1e-4, size=(N, 3), generator=g); torch.normal(0.0, 0.5, size=(N, 3), generator=g)
            u.append(torch.rand(N, dtype=torch.float64, generator=g))
        up = [torch.stack(x).to(dev) for x in ((tn, rot, u) if motion else (u,))]
        torch.cuda.synchronize()
    res["host_draws_us"] = (time.perf_counter() - t0) / T * 1e6
    best = min(res["seeded_step_us_pieces0"], res["seeded_step_us_pieces6"])
    res["seeded_over_unseeded"] = best / res["unseeded_step_us"]
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in res.items()}))


if SEEDED is not None:
    if SEEDED not in ("resample", "all"):
        sys.exit("--seeded takes resample or all")
    seeded_bench(SEEDED == "all")
    sys.exit(0)
for init in ("spread", "near"):
    eng = ENG(cb.poses, cb.embeddings, cb.mesh_vertices, B, N, device=dev, scores=SCORES)
    rng = np.random.default_rng(1)
    if init == "spread":
        start = np.stack([cb.poses[rng.integers(0, 50000, N)] for _ in range(B)])
    else:
        start = []
        for b in range(B):
            d0 = np.linalg.norm(cb.poses[:, :3, 3] - trs[b % 8].gt_poses[0][:3, 3], axis=1)
            start.append(cb.poses[rng.choice(np.argsort(d0)[:2500], N)])
        start = np.stack(start)
    eng.set_particles(torch.as_tensor(start)); eng.project_to_codebook()
    for i in range(10): eng.step(od[1 + i % 38], co[1 + i % 38])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(60): eng.step(od[1 + (10 + i) % 38], co[1 + (10 + i) % 38])
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / 60 * 1e6
    tele = eng.telemetry.cpu().numpy()[:2] / 70.0
    print(f"   tree fallbacks per batch step: nn {tele[0]:.1f}, prune {tele[1]:.1f}")
    print(f"c5 init={init}: {us:.1f} us per batch step, {B * 1e6 / us:.0f} trajectory-steps/s, engine={ENG.__name__}, scores={SCORES}")
