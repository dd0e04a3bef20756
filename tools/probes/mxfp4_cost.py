#!/usr/bin/env python3
"""Decode cost of the opt-in MXFP4 MLP weights (DeviceWeights(mxfp4_decode=True)) at 7B dims: ms per decode step for bf16 / fp8 /
mxfp4 weights at B = 1 and at G = 8 and 16 rows of one prompt (text-only prompt of S = 4490 random tokens, 128 new tokens), the three
engines alternated in one process on one box, median of `--pairs` - 1 runs.  The yardstick of the mxfp4 column is the fp8 column of
the same run.  Also: the MLP's two launches alone (gate/up + SwiGLU, down_proj + residual) in the three formats, walking the 28
layers' matrices so that no launch finds its weights in the last-level cache; and the quantisation error -- max and mean |diff| of
the decode-step logits of an mxfp4 engine against the bf16 engine on the UNMODIFIED medium fixture weights (informational: on-load
round-to-nearest with no calibrated reference behind it).  Prints one JSON line (profiles/mxfp4_cost.txt)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from open_o3_video_amd import _lib  # noqa: E402
from open_o3_video_amd.config import O3VConfig, qwen25vl_7b_dict  # noqa: E402
from open_o3_video_amd.engine import O3VEngine  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, getter_from_dict, random_getter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=6, help="runs per format and shape; the first one warms up")
ap.add_argument("--no-error", action="store_true", help="skip the quantisation error on the medium fixture")
args = ap.parse_args()
dev = torch.device("cuda")
T, S = 128, 4490
FORMATS = ("bf16", "fp8", "mxfp4")
result = {"tokens": T, "prompt": S, "unit": "ms per decode step, median of %d, bf16 / fp8 / mxfp4 alternated" % (args.pairs - 1)}


def p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


# ---- quantisation error on the medium fixture (decode-step logits: the logits a k-token call sampled its last token from)
if not args.no_error:
    import fixture_models as fm
    mcfg = fm.medium_config()
    mc = O3VConfig.from_dict(mcfg)
    W = fm.make_weights(mcfg, 6)
    pair = [O3VEngine(mc, DeviceWeights(mc, getter_from_dict(W), dev, **kw)) for kw in ({}, {"mxfp4_decode": True})]
    frames = fm.make_frames(2, 112, 140, seed=3)
    _, grid = pair[0].pixels_from_frames(frames)
    ids = np.asarray([fm.make_prompt(mcfg, [tuple(g) for g in grid.tolist()], seed=3)])
    diffs, steps = [], 0
    for k in range(2, 14):
        lg, seqs = [], []
        for e in pair:
            e._debug_keep = True
            out = e.generate(ids, None, frames=frames, max_new_tokens=k, pad_token_id=mcfg["pad_token_id"])
            lg.append(e._debug_last["logits"].float().clone())
            seqs.append(out.sequences[0, -k:].tolist())
            e._debug_keep, e._debug_last = False, None
        if seqs[0][:-1] != seqs[1][:-1]:      # the contexts part ways: later steps compare different sequences
            break
        diffs.append((lg[0] - lg[1]).abs())
        steps += 1
    d = torch.stack(diffs)
    result["medium_fixture_logit_error_vs_bf16"] = {"steps": steps, "max_abs": round(d.max().item(), 4), "mean_abs": round(d.mean().item(), 5),
                                                    "logit_abs_max": round(lg[0].abs().max().item(), 2)}
    del pair, W

# ---- whole decode steps at 7B dims
cfg = O3VConfig.from_dict(qwen25vl_7b_dict())
eng = {"bf16": O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev)),
       "fp8": O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev, fp8_decode=True)),
       "mxfp4": O3VEngine(cfg, DeviceWeights(cfg, random_getter(cfg, 1234, dev), dev, mxfp4_decode=True))}
rng = np.random.default_rng(1234)
ids = rng.integers(1000, 50000, size=(1, S))
result["steps"] = {}
for G in (1, 8, 16):
    ms = {f: [] for f in FORMATS}
    for i in range(args.pairs):
        for f in FORMATS:
            out = eng[f].generate(ids, None, max_new_tokens=T, num_return_sequences=G, sync_timings=True, return_margins=False,
                                  repetition_penalty=1.05)
            assert out.timings["mlp_weights"] == f, (f, out.timings["mlp_weights"])
            if i:
                ms[f].append(out.timings["decode_ms"] / T)
            del out
    med = {f: statistics.median(ms[f]) for f in FORMATS}
    result["steps"]["B=1" if G == 1 else f"G={G}"] = {
        **{f: round(med[f], 4) for f in FORMATS}, "mxfp4_over_fp8": round(med["mxfp4"] / med["fp8"], 4),
        "min_max": {f: [round(min(ms[f]), 4), round(max(ms[f]), 4)] for f in FORMATS}}

# ---- the MLP's two launches alone, us per launch
t, tc = eng["mxfp4"].w.t, cfg.text
H, I, L = tc.hidden_size, tc.inter_pad, tc.num_hidden_layers
lib = _lib.load()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ln = torch.ones(H, dtype=torch.bfloat16, device=dev)


def launch(fmt, which, M, l, x, res, out):
    k = f"l{l}.{which}_w"
    N, K, No, epi = (2 * I, H, I, _lib.EPI_SWIGLU) if which == "gu" else (H, I, H, _lib.EPI_RESIDUAL)
    r = p(res) if which == "down" else None
    norm = p(ln) if which == "gu" and M <= 3 else None
    a = (M, N, K, K, No, H if which == "down" else 0, epi, stream)
    if fmt == "bf16":
        return lib.o3v_linear_decode(p(x), norm, 1e-6, p(t[k]), p(t[k + "p"]), None, r, p(out), *a)
    if fmt == "fp8" and M <= 3:
        return lib.o3v_linear_decode_fp8(p(x), norm, 1e-6, p(t[k + "8"]), p(t[k + "8s"]), None, r, p(out), *a)
    if fmt == "fp8":
        return lib.o3v_linear_decode_fp8_rows(p(x), p(t[k + "8p"]), p(t[k + "8s"]), None, r, p(out), *a)
    if M <= 3:
        return lib.o3v_linear_decode_mxfp4(p(x), norm, 1e-6, p(t[k + "4"]), p(t[k + "4s"]), None, r, p(out), *a)
    return lib.o3v_linear_decode_mxfp4_rows(p(x), p(t[k + "4p"]), p(t[k + "4ps"]), None, r, p(out), *a)


result["mlp_kernels_us"] = {}
for M in (1, 8, 16):
    row = {}
    for which in ("gu", "down"):
        K, No = (H, I) if which == "gu" else (I, H)
        x = torch.randn((M, K), device=dev).to(torch.bfloat16)
        res = torch.randn((M, H), device=dev).to(torch.bfloat16)
        out = torch.empty((M, No), dtype=torch.bfloat16, device=dev)
        for fmt in FORMATS:
            times = []
            for rep in range(4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for l in range(L):
                    rc = launch(fmt, which, M, l, x, res, out)
                    assert rc == 0, (fmt, which, M, rc)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times.append(e0.elapsed_time(e1) * 1e3 / L)
            row[f"{which}_{fmt}"] = round(statistics.median(times), 2)
    result["mlp_kernels_us"][f"M={M}"] = row
bytes_w = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1.0 / 32}
result["mlp_bytes_per_layer_MB"] = {f: round(3 * H * I * b / 1e6, 1) for f, b in bytes_w.items()}
print(json.dumps(result), flush=True)
