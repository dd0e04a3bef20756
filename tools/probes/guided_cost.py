#!/usr/bin/env python3
"""Decode cost of guided decoding (o3v_guided_opts) at 7B dims, 64 new tokens, ms per decode step, best of 3 with on and off
alternated in one process.  The guide is a 40-state table over the full vocabulary (i16 [40, 152064], ~30 % of the tokens allowed per
state, random next states): per pass and row the sampler reads one table row, as many bytes as the row of bf16 logits.  1 row greedy,
8 and 32 sampled completions of one prompt (top_k 50 / top_p 0.95); "off" is the same call without a guide.  Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench import build_prompt  # noqa: E402
from open_o3_video_amd.config import O3VConfig, qwen25vl_7b_dict  # noqa: E402
from open_o3_video_amd.engine import O3VEngine  # noqa: E402
from open_o3_video_amd.guided import Guide  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, random_getter  # noqa: E402

cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
dev = torch.device("cuda")
eng = O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev))
ids = build_prompt(cfg, 32, 120, 4490)
frames = torch.randint(0, 256, (32, 3, 224, 420), dtype=torch.uint8, device=dev)
T, N_STATES = 64, 40
V = cfg.text.vocab_size
ldn = (V + 7) // 8 * 8
g = torch.Generator().manual_seed(7)
table = torch.randint(0, N_STATES, (N_STATES, ldn), generator=g).to(torch.int16)
table[torch.rand((N_STATES, ldn), generator=g) >= 0.3] = -1
table[:, V:] = -1
guide = Guide(table=table.to(dev), n_states=N_STATES, ldn=ldn, start=0, host_table=table.numpy())
configs = {
    "rows_1_greedy": dict(num_return_sequences=1),
    "rows_8_sampled": dict(num_return_sequences=8, do_sample=True, top_k=50, top_p=0.95, seed=1),
    "rows_32_sampled": dict(num_return_sequences=32, do_sample=True, top_k=50, top_p=0.95, seed=1),
}
result = {"tokens": T, "guide_states": N_STATES, "unit": "ms per decode step, best of 3, on / off alternated"}
for name, base in configs.items():
    ms = {"off": [], "on": []}
    launches = {}
    for i in range(4):      # the first pair warms up
        for which, kw in (("off", base), ("on", dict(base, guide=guide))):
            out = eng.generate([ids], None, frames=frames, max_new_tokens=T, sync_timings=True, return_margins=False, **kw)
            launches[which] = out.timings["launches_per_layer"]
            if i:
                ms[which].append(out.timings["decode_ms"] / T)
    off, on = min(ms["off"]), min(ms["on"])
    result[name] = {"off": round(off, 4), "on": round(on, 4), "delta_pct": round(100 * (on / off - 1), 2),
                    "off_all": [round(v, 4) for v in ms["off"]], "on_all": [round(v, 4) for v in ms["on"]],
                    "launches_per_layer": launches}
print(json.dumps(result), flush=True)
