#!/usr/bin/env python3
"""top_n_error (eval/single_touch_test.py:35-73) at K = 50 000, D = 256, n = 25 - the reference's only dense GEMM (K x K x D =
1.28 TFLOP) - end to end, with the matrix-core rate of k_selfsim_mfma inside it (HIP events around a panel's GEMM alone).
--precision f64: the exact float64 form instead (midas_selfsim_topn_f64, k_selfsim_mfma_f64): end to end, the panel kernel's
rate against the 78.6 TFLOP/s float64 matrix peak, the thin route (query tiles through score_batch(q, "f64") + topn_pose_error)
and the GEMV default (timed at K_small, scaled by (K / K_small)^2) - one JSON line.
usage: tools/bench_topn.py [--precision f32|f64] [K] [D] [panel_rows]"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from midastouch_amd import ops
from midastouch_amd.single_touch import top_n_error
from midastouch_amd.synthetic import make_codebook
dev = torch.device("cuda", 0)
precision = "f32"
if "--precision" in sys.argv:
    k = sys.argv.index("--precision")
    precision = sys.argv[k + 1]
    del sys.argv[k:k + 2]


def bench_f64(K, D, R):
    """float64 forms at K x D; R = panel rows (None: the default)."""
    cb = make_codebook("004_sugar_box", K=K, D=D, seed=1001)
    emb = torch.as_tensor(cb.embeddings).to(dev)
    poses = torch.as_tensor(cb.poses[:, :3, 3]).to(dev)
    flop = 2.0 * K * K * D
    top_n_error(emb[:4096].contiguous(), poses[:4096].contiguous(), fast=True, precision="f64")  # warm-up (library, scratch)
    torch.cuda.synchronize()
    res = {"K": K, "D": D, "n": 25}
    times = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        err, idx = top_n_error(emb, poses, fast=True, precision="f64", panel_rows=R, want_idx=True)
        torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    res["f64_end_to_end"] = {"seconds": min(times), "runs": times, "tflops": flop / min(times) / 1e12,
                             "floor_ms_at_78.6": flop / 78.6e12 * 1e3, "x_floor": min(times) / (flop / 78.6e12),
                             "mean_err_mm": float(err.mean()) * 1e3}
    # the panel kernel alone, HIP events
    codebook = ops.Codebook(emb)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rows in (2048, 4096):
        panel = torch.empty((rows, K), dtype=torch.float64, device=dev)
        codebook.ctx.call("midas_selfsim_panel_f64", codebook.h, 0, rows, ops._ptr(panel), K)
        e0.record()
        for _ in range(5):
            codebook.ctx.call("midas_selfsim_panel_f64", codebook.h, 0, rows, ops._ptr(panel), K)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 5
        tf = 2.0 * rows * K * D / (ms * 1e-3) / 1e12
        res[f"k_selfsim_mfma_f64_{rows}"] = {"panel_rows": rows, "ms": ms, "tflops": tf, "frac_of_78.6": tf / 78.6}
        del panel
    # the thin route: query tiles through score_batch(q, "f64") + the selection
    feat = poses.to(torch.float64).contiguous()
    def thin(tile=256):
        out = torch.empty((K,), dtype=torch.float64, device=dev)
        ia = torch.empty((K, 25), dtype=torch.int32, device=dev)
        for i0 in range(0, K, tile):
            sc = codebook.score_batch(codebook.emb[i0:i0 + tile].to(torch.float64), precision="f64")
            out[i0:i0 + tile], ia[i0:i0 + tile] = ops.topn_pose_error(sc, i0, 25, feat, want_idx=True)
        return out, ia
    thin(); torch.cuda.synchronize()
    t0 = time.perf_counter(); terr, tidx = thin(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
    res["thin_score_batch_f64"] = {"seconds": dt, "tflops": flop / dt / 1e12, "x_dedicated": dt / min(times),
                                   "same_result": bool(torch.equal(terr, err) and torch.equal(tidx, idx))}
    # the GEMV default at a small K, scaled by the quadratic work
    Ks = min(K, 5000)
    es, ps = emb[:Ks].contiguous(), poses[:Ks].contiguous()
    top_n_error(es, ps); torch.cuda.synchronize()
    t0 = time.perf_counter(); top_n_error(es, ps); torch.cuda.synchronize(); dt = time.perf_counter() - t0
    t0 = time.perf_counter(); top_n_error(es, ps, fast=True, precision="f64"); torch.cuda.synchronize(); dts = time.perf_counter() - t0
    scaled = dt * (K / Ks) ** 2
    res["gemv_default"] = {"K_small": Ks, "seconds_at_K_small": dt, "f64_seconds_at_K_small": dts, "seconds_scaled_to_K": scaled,
                           "x_dedicated": scaled / min(times)}
    return res


if precision == "f64":
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    D = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    R = int(sys.argv[3]) if len(sys.argv) > 3 else None
    print(json.dumps(bench_f64(K, D, R)))
    sys.exit(0)
if precision != "f32":
    sys.exit(f"--precision f32|f64, got {precision!r}")
K = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
D = int(sys.argv[2]) if len(sys.argv) > 2 else 256
R = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
cb = make_codebook("004_sugar_box", K=K, D=D, seed=1001)
emb = torch.as_tensor(cb.embeddings).to(dev)
poses = torch.as_tensor(cb.poses[:, :3, 3]).to(dev)
top_n_error(emb[:4096].contiguous(), poses[:4096].contiguous(), fast=True)  # warm-up (library, scratch)
torch.cuda.synchronize()
res = {}
for rows in (R, 4096):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    err = top_n_error(emb, poses, fast=True, panel_rows=rows)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    res[f"panel_{rows}"] = {"seconds": dt, "gemm_tflop": 2.0 * K * K * D / 1e12, "end_to_end_tflops": 2.0 * K * K * D / dt / 1e12, "mean_err_mm": float(err.mean()) * 1e3}
# the GEMM alone: one panel, HIP events
codebook = ops.Codebook(emb)
ldo = -(-K // 128) * 128
panel = torch.empty((-(-R // 128) * 128, ldo), dtype=torch.float32, device=dev)
lib, ctx = codebook.ctx.lib, codebook.ctx
import ctypes as C
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for R in (R, 4096, 8192):
    panel = torch.empty((-(-R // 128) * 128, ldo), dtype=torch.float32, device=dev)
    for _ in range(2):
        ctx.call("midas_selfsim_panel", codebook.h, 0, R, ops._ptr(panel), ldo)
    e0.record()
    for _ in range(5):
        ctx.call("midas_selfsim_panel", codebook.h, 0, R, ops._ptr(panel), ldo)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    res[f"k_selfsim_mfma_{R}"] = {"panel_rows": R, "ms": ms, "tflops": 2.0 * R * K * D / (ms * 1e-3) / 1e12, "frac_of_157.3": 2.0 * R * K * D / (ms * 1e-3) / 1e12 / 157.3}
print(json.dumps(res))
