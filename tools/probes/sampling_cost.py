#!/usr/bin/env python3
"""Decode cost of the extended sampling controls (o3v_sampling_opts) at 7B dims, 128 new tokens, ms per decode step, median of 7 with
on and off alternated in one process.  B = 1 greedy: repetition penalty alone against repetition + presence + frequency + bias.
G = 8 sampled completions of one prompt: top_k 50 / top_p 0.95 against the same plus min_p 0.05 and the penalties.  Prints one JSON
line."""
import json
import os
import statistics
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
penalties = dict(presence_penalty=0.5, frequency_penalty=0.3)
configs = {
    "B1_greedy": (dict(num_return_sequences=1, repetition_penalty=1.05),
                  dict(penalties, token_bias={t: 0.5 * (t % 5 - 2) for t in range(1000, 1400)})),
    "G8_sampled": (dict(num_return_sequences=8, do_sample=True, top_k=50, top_p=0.95, seed=1, repetition_penalty=1.05),
                   dict(penalties, min_p=0.05)),
}
result = {"tokens": T, "unit": "ms per decode step, median of 7, on / off alternated"}
for name, (base, extra) in configs.items():
    ms = {"off": [], "on": []}
    launches = {}
    for i in range(8):      # the first pair warms up
        for which, kw in (("off", base), ("on", dict(base, **extra))):
            out = eng.generate([ids], None, frames=frames, max_new_tokens=T, sync_timings=True, return_margins=False, **kw)
            launches[which] = out.timings["launches_per_layer"]
            if i:
                ms[which].append(out.timings["decode_ms"] / T)
    off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
    result[name] = {"off": round(off, 4), "on": round(on, 4), "delta_pct": round(100 * (on / off - 1), 2),
                    "off_min_max": [round(min(ms["off"]), 4), round(max(ms["off"]), 4)],
                    "on_min_max": [round(min(ms["on"]), 4), round(max(ms["on"]), 4)],
                    "launches_per_layer": launches}
print(json.dumps(result), flush=True)
