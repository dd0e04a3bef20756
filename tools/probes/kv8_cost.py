#!/usr/bin/env python3
"""Decode cost of the opt-in fp8 K/V cache (O3VEngine.kv_cache_dtype = "fp8") at 7B dims, 128 new tokens, ms per decode step, median
of 7 with bf16 K/V and fp8 K/V alternated in one process.  Independent rows (text-only prompts of S random tokens per row: the K/V
bytes and the attention are those of a video prompt, without the tower): 32 rows x S = 4490 (bench.py's batched_videos shape),
8 rows x S = 20394, 1 row x S = 4490 (fp8 K/V runs the stand-alone chain there instead of the one-launch block).  Also
o3v_kv8_quantize alone on the 32 x 4490 prompt against its byte floor.  Prints one JSON line (profiles/kv8_cost.json).
`--shape 32x4490 --pairs 2`: one shape, fewer pairs (the run profiles/kv8_32x4490_kernel_stats.csv was taken from)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from open_o3_video_amd import _lib  # noqa: E402
from open_o3_video_amd.config import O3VConfig, qwen25vl_7b_dict  # noqa: E402
from open_o3_video_amd.engine import O3VEngine  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, random_getter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", action="append", help="ROWSxS, repeatable; default: the three shapes of the docstring")
ap.add_argument("--pairs", type=int, default=8, help="bf16 / fp8 pairs per shape; the first one warms up")
ap.add_argument("--no-quantize", action="store_true")
args = ap.parse_args()
shapes = [tuple(int(v) for v in s.split("x")) for s in (args.shape or ["32x4490", "8x20394", "1x4490"])]

cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
dev = torch.device("cuda")
eng = O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev, batched_decode=True))
T = 128
rng = np.random.default_rng(1234)
result = {"tokens": T, "unit": "ms per decode step, median of %d, bf16 / fp8 K/V alternated" % (args.pairs - 1), "shapes": {}}
for rows, S in shapes:
    ids = rng.integers(1000, 50000, size=(rows, S))
    ms = {"bf16": [], "fp8": []}
    info = {}
    for i in range(args.pairs):
        for which in ("bf16", "fp8"):
            eng.kv_cache_dtype = which
            out = eng.generate(ids, None, max_new_tokens=T, sync_timings=True, return_margins=False, repetition_penalty=1.05)
            assert out.timings["kv_cache_dtype"] == which
            info[which] = {"launches_per_layer": out.timings["launches_per_layer"], "kv_cache_bytes": out.timings["kv_cache_bytes"],
                           "fused_attention_layers": out.timings["fused_attention_layers"]}
            if i:
                ms[which].append(out.timings["decode_ms"] / T)
            del out
    bf, f8 = statistics.median(ms["bf16"]), statistics.median(ms["fp8"])
    result["shapes"][f"{rows}x{S}"] = {"bf16": round(bf, 4), "fp8": round(f8, 4), "delta_pct": round(100 * (f8 / bf - 1), 2),
                                       "bf16_min_max": [round(min(ms["bf16"]), 4), round(max(ms["bf16"]), 4)],
                                       "fp8_min_max": [round(min(ms["fp8"]), 4), round(max(ms["fp8"]), 4)], "info": info}
eng.kv_cache_dtype = "bf16"

if not args.no_quantize:
    t = cfg.text
    L, B, Hkv, S, D = t.num_hidden_layers, 32, t.num_key_value_heads, 4490, t.head_dim
    k = torch.randn((L, B, Hkv, S, D), dtype=torch.bfloat16, device=dev)
    v = torch.randn((L, B, Hkv, S, D), dtype=torch.bfloat16, device=dev)
    Tmax = S + T
    k8, v8 = (torch.empty((L, B, Hkv, Tmax, D), dtype=torch.uint8, device=dev) for _ in range(2))
    ks, vs = (torch.empty((L, B, Hkv, Tmax), dtype=torch.float32, device=dev) for _ in range(2))
    p = lambda x: C.c_void_p(x.data_ptr())
    times = []
    for i in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call("o3v_kv8_quantize", p(k), p(v), p(k8), p(v8), p(ks), p(vs), L * B * Hkv, S, Tmax, D,
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        e1.record()
        torch.cuda.synchronize()
        if i:
            times.append(e0.elapsed_time(e1))
    nbytes = 2 * L * B * Hkv * S * (D * 2 + D + 4)
    med = statistics.median(times)
    result["quantize_32x4490"] = {"ms": round(med, 3), "bytes": nbytes, "GBps": round(nbytes / med / 1e6, 1),
                                  "floor_ms_at_8TBps": round(nbytes / 8e12 * 1e3, 3)}
print(json.dumps(result), flush=True)
