"""Test helpers of the ragged decode (continuous batching): a torch-tensor wrapper over o3v_attn_decode_ragged in the style of
kernel_ops.py, the random cases its kernel tests share, and the request lists of the engine tests."""
from __future__ import annotations

import math

import numpy as np
import torch

from kernel_ops import _buf, _p, _s
from open_o3_video_amd import _lib

BF = torch.bfloat16
NAN16 = -1      # 0xFFFF as int16: a bf16 NaN


def attn_decode_ragged(q, kc, vc, knew, vnew, row_base, step, nsplit, scale, poison=False, out=None, D=None, Hkv=None):
    """q [B, Hq, D]; kc / vc bf16 [B, Hkv, Tmax, D] (written in place: slot ctx_b - 1 of every live row); knew / vnew [B, Hkv, D];
    row_base i32 [B].  -> out [B, Hq, D]."""
    B, Hq, Dq = q.shape
    _, Hk, Tmax, _ = kc.shape
    ns = abs(nsplit)
    if out is None:
        out = _buf(q.shape, q.dtype, q.device, poison)
    po = _buf(B * Hq * max(ns, 1) * Dq, torch.float32, q.device, poison)
    pm = _buf(B * Hq * max(ns, 1) * 2, torch.float32, q.device, poison)
    _lib.call("o3v_attn_decode_ragged", _p(q), _p(kc), _p(vc), _p(knew), _p(vnew), _p(out), _p(po), _p(pm), _p(row_base), step, B, Hq,
              Hk if Hkv is None else Hkv, Dq if D is None else D, Tmax, nsplit, float(scale), _s())
    return out


def ragged_case(dev, ctxs, Hq, Hkv, D, seed, step=5, Tmax=None):
    """Random bf16 K/V (the magnitudes of test_gpu_kv8.py::_case) for rows whose contexts are `ctxs`; an entry <= 0 or > Tmax makes
    an idle row.  `kfull` / `vfull` hold every slot (the reference reads them: the staging row is already at slot ctx_b - 1);
    `kc` / `vc` are what the ragged call gets: slots >= ctx_b - 1 of a live row, and every slot of an idle row, hold 0xFFFF."""
    gen = torch.Generator().manual_seed(seed)
    B = len(ctxs)
    Tmax = Tmax or max(ctxs) + 3
    kfull = (torch.randn(B, Hkv, Tmax, D, generator=gen) * torch.exp2(torch.randint(-3, 3, (B, Hkv, Tmax, 1), generator=gen).float())).to(BF)
    vfull = (torch.randn(B, Hkv, Tmax, D, generator=gen) * torch.exp2(torch.randint(-6, 4, (B, Hkv, Tmax, 1), generator=gen).float())).to(BF)
    q = (torch.randn(B, Hq, D, generator=gen) * 0.7).to(BF)
    knew, vnew = (torch.randn(B, Hkv, D, generator=gen).to(BF) for _ in range(2))
    kc, vc = kfull.clone(), vfull.clone()
    live = [1 <= c <= Tmax for c in ctxs]
    for b, c in enumerate(ctxs):
        if live[b]:
            knew[b], vnew[b] = kfull[b, :, c - 1], vfull[b, :, c - 1]
            for t in (kc, vc):
                t[b, :, c - 1:].view(torch.int16).fill_(NAN16)
        else:
            for t in (kc, vc):
                t[b].view(torch.int16).fill_(NAN16)
    row_base = torch.tensor([c - 1 - step for c in ctxs], dtype=torch.int32)
    to = lambda t: t.to(dev)
    return dict(q=to(q), kfull=to(kfull), vfull=to(vfull), kc=to(kc), vc=to(vc), knew=to(knew), vnew=to(vnew), row_base=to(row_base),
                step=step, ctxs=list(ctxs), live=live, Tmax=Tmax, scale=1.0 / math.sqrt(D))


def raw(t):
    return t.view(torch.int16)


# ---- engine tests: request lists over the fixture models
POSTS = (6, 9, 13)      # text tokens behind the frame block: three prompt lengths


def request_prompts(cfg, n, seed, clips=2, max_new=(3, 9, 20), prompt_seeds=None):
    """n requests over `clips` one-frame clips (56 x 84) with 3 distinct prompt lengths -> [(ids, clip index, max_new_tokens)] and the
    clips' frames.  prompt_seeds: the text seed of every request (default: seed * 1000 + i).  Pure host code: the seed search of
    the continuous-batching tests runs the CPU oracle on the same lists."""
    import fixture_models as fm
    frames = [fm.make_frames(1, 56, 84, seed=100 + seed * 10 + c) for c in range(clips)]
    ps = cfg["vision_config"]["patch_size"]
    grid = [(1, 56 // ps, 84 // ps)]
    out = []
    for i in range(n):
        ids = fm.make_prompt(cfg, grid, n_text_post=POSTS[i % len(POSTS)], seed=seed * 1000 + i if prompt_seeds is None else int(prompt_seeds[i]))
        out.append((ids, i % clips, int(max_new[(i * 7 + seed) % len(max_new)])))
    return out, frames


def make_requests(eng, cfg, n, seed, **kw):
    """The same as generate_continuous requests (the clips' visual tokens computed once per clip) -> (requests, frames per request)."""
    prompts, frames = request_prompts(cfg, n, seed, **kw)
    vis = []
    for f in frames:
        px, grid = eng.pixels_from_frames(f)
        vis.append((eng.vit_forward(px, grid), grid))
    reqs = [dict(ids=np.asarray(ids, dtype=np.int64), max_new_tokens=m, vis_embeds=vis[c][0], image_grid_thw=vis[c][1])
            for ids, c, m in prompts]
    return reqs, [frames[c] for _, c, _ in prompts]


def seeded_eos(V, seed, share=8, keep=()):
    """About V / share token ids drawn with `seed`, none of `keep`: rows end at scattered steps."""
    rng = np.random.RandomState(seed)
    ids = rng.choice(V, size=V // share, replace=False)
    return sorted(int(t) for t in ids if int(t) not in keep)
