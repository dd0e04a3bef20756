#!/usr/bin/env python3
"""Cost of continuous batching (O3VEngine.generate_continuous, the ragged decode regime) at 7B dims, one process, device events
around synchronised work, every shape warmed first, the versions alternated.  Prints one JSON line
(profiles/continuous_batching.json).

(a) per step: decode ms/step of the ragged regime (`_debug_ragged`: the existing generate call decoding through row_base, staging
    rows and o3v_attn_decode_ragged) against the static path, 32 equal rows x S = 4490 and 8 x 20000, text-only prompts of random
    tokens.  The static path runs twice per round ("static", "static_again"): their difference is the run-to-run spread the ragged
    figure is to be read against.  Expected: equal bytes plus 512 B of staging per (row, kv head, layer).
(b) workload: 128 requests over S = 4490 with max_new drawn from a seeded uniform 32..512 (stored below), 32 rows: static batches
    of 32 in input order against one generate_continuous call.  decode_forwards is host arithmetic (exact); wall time covers the
    prompts too (static: 4 prefills of 32 rows, continuous: 128 single-row prefills at admission)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from open_o3_video_amd.config import O3VConfig, qwen25vl_7b_dict  # noqa: E402
from open_o3_video_amd.engine import O3VEngine  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, random_getter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", action="append", help="ROWSxS, repeatable; default: 32x4490 and 8x20000")
ap.add_argument("--rounds", type=int, default=5, help="rounds of (static, ragged, static_again) per shape; the first one warms up")
ap.add_argument("--rounds-long", type=int, default=3, help="the same for shapes of S >= 10000 (their prefill dominates the run)")
ap.add_argument("--tokens", type=int, default=64, help="decode steps per run of part (a)")
ap.add_argument("--requests", type=int, default=128, help="requests of part (b); 0 skips it")
ap.add_argument("--prompt", type=int, default=4490, help="prompt length of part (b)")
args = ap.parse_args()
shapes = [tuple(int(v) for v in s.split("x")) for s in (args.shape or ["32x4490", "8x20000"])]

cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
dev = torch.device("cuda")
eng = O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev, batched_decode=True))
rng = np.random.default_rng(1234)
T = args.tokens
result = {"per_step": {"tokens": T, "unit": "ms per decode step, median over the rounds after the first", "shapes": {}}}

for rows, S in shapes:
    ids = rng.integers(1000, 50000, size=(rows, S))
    ms = {"static": [], "ragged": [], "static_again": []}
    rounds = args.rounds if S < 10000 else args.rounds_long
    for i in range(rounds):
        print(f"(a) {rows}x{S} round {i}", file=sys.stderr, flush=True)
        for which in ("static", "ragged", "static_again"):
            eng._debug_ragged = which == "ragged"
            out = eng.generate(ids, None, max_new_tokens=T, sync_timings=True, return_margins=False, repetition_penalty=1.05)
            if i:
                ms[which].append(out.timings["decode_ms"] / T)
            lpl = out.timings["launches_per_layer"]
            del out
    eng._debug_ragged = False
    med = {k: statistics.median(v) for k, v in ms.items()}
    result["per_step"]["shapes"][f"{rows}x{S}"] = {
        **{k: round(v, 4) for k, v in med.items()},
        "min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "static_spread_pct": round(100 * abs(med["static_again"] / med["static"] - 1), 2),
        "ragged_vs_static_pct": round(100 * (med["ragged"] / (0.5 * (med["static"] + med["static_again"])) - 1), 2),
        "rounds": rounds - 1, "launches_per_layer_static": lpl}

if args.requests:
    n, S, rows = args.requests, args.prompt, 32
    max_new = [int(v) for v in rng.integers(32, 513, size=n)]
    prompts = rng.integers(1000, 50000, size=(n, S))
    reqs = [dict(ids=prompts[i], max_new_tokens=max_new[i]) for i in range(n)]

    def run_static():
        fw = 0
        for c0 in range(0, n, rows):
            out = eng.generate(prompts[c0:c0 + rows], None, max_new_tokens=max(max_new[c0:c0 + rows]), return_margins=False,
                               repetition_penalty=1.05)
            fw += out.timings["decode_forwards"]
            del out
        return fw, {}

    def run_continuous():
        outs = eng.generate_continuous(reqs, rows, repetition_penalty=1.05, return_margins=False)
        assert [len(o.tokens) for o in outs] == max_new
        tm = outs[0].timings
        return tm["decode_forwards"], {k: tm[k] for k in ("rows_refilled", "sessions", "launches_per_layer", "kv_cache_bytes", "nsplit")}

    # warm both versions on a short list of the same shapes, then one timed run each, static first and last
    warm = [dict(ids=prompts[i], max_new_tokens=4) for i in range(rows + 1)]
    eng.generate(prompts[:rows], None, max_new_tokens=4, return_margins=False, repetition_penalty=1.05)
    eng.generate_continuous(warm, rows, repetition_penalty=1.05, return_margins=False)
    work = {"requests": n, "prompt_tokens": S, "rows": rows, "max_new": max_new, "tokens": int(sum(max_new)), "runs": []}
    for name, fn in (("static", run_static), ("continuous", run_continuous), ("static_again", run_static)):
        print(f"(b) {name}", file=sys.stderr, flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fw, extra = fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        work["runs"].append({"version": name, "decode_forwards": int(fw), "wall_s": round(wall, 3),
                             "tokens_per_s": round(sum(max_new) / wall, 1), **extra})
    # the exact step counts behind decode_forwards: a static batch runs to its longest row (the last forward is skipped)
    work["static_forwards_expected"] = int(sum(max(max_new[c0:c0 + rows]) - 1 for c0 in range(0, n, rows)))
    result["workload"] = work
print(json.dumps(result), flush=True)
