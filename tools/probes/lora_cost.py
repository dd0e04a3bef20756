#!/usr/bin/env python3
"""Cost of a merged LoRA adapter (O3VEngine.load_adapter -> o3v_lora_merge + o3v_repack_rows) at Qwen2.5-VL-7B dims, all 7 LLM
linears of every layer targeted at r = 64, on ONE engine in one run:
  * the adapter push (a second load_adapter with the same targets: the trainer's per-step push; A and B on the device) in ms, the
    bytes of A and B the caller hands over and the bytes the device moves for it, against a full load_weights of the same engine from
    a device bf16 state dict (what a LoRA trainer had to do before: merge on its side and push every matrix);
  * ms per decode step (B = 1 and G = 8 rows of one S = 4490 text prompt, 128 new tokens) with the adapter on and inside
    adapter_disabled(), alternated;
  * adapter_bytes().
Median of `--reps` - 1 after one warm-up.  Prints one JSON line and writes it to profiles/lora_cost.json."""
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
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--rank", type=int, default=64)
ap.add_argument("--fp8", action="store_true", help="an engine with the fp8 decode images (the adapter then owns those too)")
args = ap.parse_args()
dev = torch.device("cuda")
T, S, r = 128, 4490, args.rank
cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
eng = O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev, fp8_decode=args.fp8))
dw = eng.w
LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
mods = [f"model.language_model.layers.{i}.{m}" for i in range(cfg.text.num_hidden_layers) for m in LINEARS]
gen = torch.Generator(device=dev).manual_seed(7)
adapter = []
for m in mods:
    N, K = dw.update_plan[m + ".weight"].shape
    adapter.append((f"base_model.model.{m}.lora_A.default.weight", (torch.randn((r, K), device=dev, generator=gen) * 0.02).to(torch.bfloat16)))
    adapter.append((f"base_model.model.{m}.lora_B.default.weight", (torch.randn((N, r), device=dev, generator=gen) * 0.02).to(torch.bfloat16)))
ab_bytes = sum(t.numel() * t.element_size() for _, t in adapter)
result = {"probe": "lora_cost", "model": "Qwen2.5-VL-7B dims (random_getter)", "rank": r, "targets": len(mods), "fp8_decode": bool(args.fp8),
          "unit": "ms, median of %d" % (args.reps - 1)}


def timed(fn):
    times = []
    for i in range(args.reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            times.append(a.elapsed_time(b))
    return round(statistics.median(times), 3), [round(t, 3) for t in times]


eng.load_adapter(adapter, lora_alpha=2 * r)          # the first load allocates the images
names = [m + ".weight" for m in mods]
rd, wr = dw.update_bytes(names)                      # the repack half of a push: reads the staged merge, writes every image
merge_bytes = 2 * rd                                 # the merge half: reads the base rows, writes the staging tensor
push_ms, push_all = timed(lambda: eng.load_adapter(adapter, lora_alpha=2 * r))
result["adapter_push"] = {"ms": push_ms, "ms_all": push_all, "bytes_from_caller": ab_bytes, "bytes_moved_on_device": merge_bytes + rd + wr}
get = random_getter(cfg, 4321, dev)
sd = {name: get(name) for name in dw.update_plan}
frd, fwr = dw.update_bytes()
full_ms, full_all = timed(lambda: eng.load_weights(sd.items()))       # re-merges the adapter's targets too: images are never stale
result["full_load_weights_with_adapter_resident"] = {"ms": full_ms, "ms_all": full_all, "bytes_from_caller": frd}
eng.unload_adapter()
full_ms, full_all = timed(lambda: eng.load_weights(sd.items()))
result["full_load_weights"] = {"ms": full_ms, "ms_all": full_all, "bytes_from_caller": frd, "bytes_moved_on_device": frd + fwr}
result["push_over_full_load_weights"] = round(push_ms / full_ms, 4)
del sd
torch.cuda.empty_cache()

eng.load_adapter(adapter, lora_alpha=2 * r)
result["adapter_bytes"] = dw.adapter_bytes()
result["base_bytes"] = dw.nbytes()
ids = np.random.default_rng(1234).integers(1000, 50000, size=(1, S))
result["decode_ms_per_step"] = {}
for G in (1, 8):
    ms = {"on": [], "off": []}
    for i in range(args.reps):
        for state in ("on", "off"):
            eng.set_adapter_enabled(state == "on")
            out = eng.generate(ids, None, max_new_tokens=T, num_return_sequences=G, sync_timings=True, return_margins=False,
                               repetition_penalty=1.05)
            if i:
                ms[state].append(out.timings["decode_ms"] / T)
            del out
    med = {s: statistics.median(v) for s, v in ms.items()}
    result["decode_ms_per_step"]["B=1" if G == 1 else f"G={G}"] = {
        "on": round(med["on"], 4), "off": round(med["off"], 4), "on_over_off": round(med["on"] / med["off"], 4),
        "min_max": {s: [round(min(v), 4), round(max(v), 4)] for s, v in ms.items()}}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "lora_cost.json"), "w") as f:
    f.write(line + "\n")
