#!/usr/bin/env python3
"""Decode cost of the top-N log-probs at 7B dims: ms per decode step with logprobs 0 / 5 / 20, batch 1 (greedy, the eval path) and
G = 8 sampled completions of one prompt (the rollout), 128 new tokens, best of 3.  Prints one JSON line per configuration."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench import build_prompt  # noqa: E402
from open_o3_video_amd.config import O3VConfig, qwen25vl_7b_dict  # noqa: E402
from open_o3_video_amd.engine import O3VEngine  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, random_getter  # noqa: E402

cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
dev = torch.device("cuda")
eng = O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev))
ids = build_prompt(cfg, 32, 120, 4490)
frames = torch.randint(0, 256, (32, 3, 224, 420), dtype=torch.uint8, device=dev)
T = 128
configs = {"B1_greedy": dict(num_return_sequences=1), "G8_sampled": dict(num_return_sequences=8, do_sample=True, top_p=0.95, seed=1)}
for name, kw in configs.items():
    base_seq = None
    for n in (0, 5, 20):
        best = None
        for _ in range(3):
            out = eng.generate([ids], None, frames=frames, max_new_tokens=T, sync_timings=True, return_margins=False, logprobs=n, **kw)
            ms = out.timings["decode_ms"] / T
            best = ms if best is None else min(best, ms)
        same = base_seq is None or torch.equal(base_seq, out.sequences)
        base_seq = out.sequences if base_seq is None else base_seq
        print(json.dumps({"config": name, "logprobs": n, "decode_ms_per_step_best_of_3": round(best, 4), "same_ids_as_off": same,
                          "launches_per_layer": out.timings["launches_per_layer"]}), flush=True)
