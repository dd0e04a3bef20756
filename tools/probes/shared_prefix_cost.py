#!/usr/bin/env python3
"""Five questions about one video, 128 greedy tokens each, at 7B dims, through the three ways the engine can serve them -- median of
7, the three paths alternated in one process (the first round warms up), at S = 4490 and S = 20394 shared tokens:

  sequential   one request after another with `prefix_key`: the shared prefix is prefilled by the first request, every request
               decodes alone at batch 1 (the prefix cache is dropped before each round, so each round pays that one prefill);
  independent  one call, five left-padded independent rows: every row prefills and keeps the whole prompt;
  group        one call with `shared_prefix_len`: the prefix prefilled once, the five suffixes behind it, the rows decoded as a
               group that reads the prefix K/V once per step.

Text-only prompts (S random tokens + a question of 9..21 tokens per row: the K/V bytes and the attention are those of a video
prompt, without the tower).  Per path: prefill ms (all calls of the path), ms per decode step of the FIVE rows (sequential: the
five batch-1 steps added up) and timings["kv_cache_bytes"] (sequential: of one request).  Prints one JSON line
(profiles/shared_prefix_cost.json)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from open_o3_video_amd.config import O3VConfig, qwen25vl_7b_dict  # noqa: E402
from open_o3_video_amd.engine import O3VEngine  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, random_getter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--S", action="append", type=int, help="shared prefix length, repeatable; default 4490 and 20394")
ap.add_argument("--rounds", type=int, default=8, help="rounds per length; the first one warms up")
args = ap.parse_args()

cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
dev = torch.device("cuda")
eng = O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev, batched_decode=True))
T, ROWS = 128, 5
rng = np.random.default_rng(1234)
kw = dict(max_new_tokens=T, sync_timings=True, return_margins=False, repetition_penalty=1.05)
PATHS = ("sequential", "independent", "group")
result = {"rows": ROWS, "tokens": T, "unit": "ms, median of %d, the three paths alternated" % (args.rounds - 1), "lengths": {}}
for S in (args.S or [4490, 20394]):
    prefix = rng.integers(1000, 50000, size=S).tolist()
    rows = [prefix + rng.integers(1000, 50000, size=n).tolist() for n in (21, 9, 14, 17, 12)]
    L = max(len(r) for r in rows)
    ids = np.asarray([[cfg.pad_token_id] * (L - len(r)) + r for r in rows])
    mask = np.asarray([[0] * (L - len(r)) + [1] * len(r) for r in rows])
    pre, step, info = {p: [] for p in PATHS}, {p: [] for p in PATHS}, {}
    for i in range(args.rounds):
        for path in PATHS:
            eng.drop_prefix_cache()
            if path == "sequential":
                outs = [eng.generate([r], None, prefix_key="video", **kw) for r in rows]
                assert [o.timings["prefix_tokens_reused"] for o in outs] == [0] + [S] * (ROWS - 1)
            elif path == "independent":
                outs = [eng.generate(ids, mask, **kw)]
            else:
                outs = [eng.generate(ids, mask, shared_prefix_len=S, **kw)]
                assert outs[0].timings["shared_prefix_rows"] == ROWS
            info[path] = {"kv_cache_bytes": outs[0].timings["kv_cache_bytes"], "calls": len(outs),
                          "launches_per_layer": outs[0].timings["launches_per_layer"]}
            if i:
                pre[path].append(sum(o.timings["prefill_ms"] for o in outs))
                step[path].append(sum(o.timings["decode_ms"] for o in outs) / T)
            del outs
    eng.drop_prefix_cache()
    med = statistics.median
    result["lengths"][str(S)] = {
        p: {"prefill_ms": round(med(pre[p]), 2), "prefill_min_max": [round(min(pre[p]), 2), round(max(pre[p]), 2)],
            "ms_per_step": round(med(step[p]), 4), "step_min_max": [round(min(step[p]), 4), round(max(step[p]), 4)], **info[p]}
        for p in PATHS}
print(json.dumps(result), flush=True)
