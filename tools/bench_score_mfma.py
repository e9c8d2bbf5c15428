#!/usr/bin/env python3
"""midas_score_batch (k_score_mfma; --precision f64: midas_score_batch_f64, k_score_mfma_f64) at c5's shape and a few others: us per
call, TFLOP/s, GB/s of the codebook stream, and - with --precision f64 - the B-launch midas_score GEMV loop on the same codes, which
the float64 kernel replaces (GPU box only)."""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from midastouch_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--precision", choices=("f32", "f64"), default="f32")
ap.add_argument("--shapes", default="", help="K,D,B;K,D,B;... (default: the fixed list)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
shapes = ((50_000, 512, 64), (50_000, 256, 64), (500_000, 512, 64), (50_000, 512, 16), (5_000, 256, 64), (50_000, 512, 128))
if args.shapes:
    shapes = tuple(tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";"))


def time_us(fn, n=30):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


res = {}
for K, D, B in shapes:
    E = torch.randn((K, D), device=dev)
    cb = ops.Codebook(E)
    codes = torch.randn((B, D), dtype=torch.float64, device=dev)
    us = time_us(lambda: cb.score_batch(codes, precision=args.precision))
    key = "us_per_call_incl_codes_prepare" if args.precision == "f32" else "us_per_call"
    r = {key: round(us, 2), "TFLOPs": round(2.0 * K * D * B / us / 1e6, 1), "codebook_GBps": round(K * D * 4 / us / 1e3)}
    if args.precision == "f64":
        gemv = time_us(lambda: cb.score(codes), n=10)
        r["gemv_loop_us"] = round(gemv, 1)
        r["speedup_vs_gemv_loop"] = round(gemv / us, 2)
    res[f"K{K}_D{D}_B{B}"] = r
    del cb, E
print(json.dumps({"precision": args.precision, **res}))
