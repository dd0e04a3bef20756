#!/usr/bin/env python3
"""Cost of an in-place weight update (DeviceWeights.load_weights -> o3v_repack_rows) at Qwen2.5-VL-7B dims: a full update from a
device bf16 state dict, without and with the fp8 decode images.  Median of 7 timed updates after 2 warm-ups (device events),
bytes read / written by the plan, rate against the 6.29 TB/s copy ceiling, and -- for comparison -- the time and the peak extra
memory of building a fresh DeviceWeights from the same dict (which must give the same bytes).  One JSON line.
--quick: one update per mode and nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from open_o3_video_amd.config import O3VConfig, qwen25vl_7b_dict  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, getter_from_dict, random_getter  # noqa: E402

COPY_CEILING = 6.29e12   # B/s, device-to-device copy on the MI355X
quick = "--quick" in sys.argv
cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
dev = torch.device("cuda")
out = {"probe": "weight_update_cost", "model": "Qwen2.5-VL-7B dims (random_getter)", "source": "device bf16 state dict"}
for fp8 in (False, True):
    dw = DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev, fp8_decode=fp8)
    get = random_getter(cfg, 4321, dev)
    sd = {name: get(name) for name in dw.update_plan}
    rd, wr = dw.update_bytes()
    times = []
    for i in range(1 if quick else 9):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dw.load_weights(sd.items())
        b.record()
        b.synchronize()
        if i >= 2:
            times.append(a.elapsed_time(b))
    r = {"bytes_read": rd, "bytes_written": wr, "tensors": len(sd)}
    if not quick:
        ms = statistics.median(times)
        r.update(update_ms_median=round(ms, 3), update_ms_all=[round(t, 3) for t in times],
                 TBps=round((rd + wr) / ms / 1e9, 3), frac_of_copy_ceiling=round((rd + wr) / ms / 1e9 / (COPY_CEILING / 1e12), 4))
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fresh = DeviceWeights(cfg, getter_from_dict(sd), dev, fp8_decode=fp8)
        torch.cuda.synchronize()
        r["fresh_load_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        r["fresh_load_peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
        r["bytes_equal_fresh_load"] = all(torch.equal(dw.t[k].view(torch.uint8), v.view(torch.uint8)) for k, v in fresh.t.items())
        del fresh
    out["fp8_decode" if fp8 else "bf16"] = r
    del dw, sd
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
