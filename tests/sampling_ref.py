"""fp32 torch definition of the extended sampling controls (vLLM 0.7.2 V0 sampler as restated in include/o3v.h, o3v_sampling_opts;
parity unpinned against vLLM, pinned against transformers' processors where it has the same operation: tests/test_sampling_params_cpu.py).

Per row and step, from the bf16 logit x_i, c_i = how often the row has emitted token i, seen_i = token i is in the prompt or was emitted:
  1. x += bias_i            one dense vector: logit_bias, -inf at banned ids and outside the allowed set (and, before min_tokens,
                            at every stop id)
  2. repetition penalty     seen_i: x > 0 ? x / r : x * r                       (logprobs_ref.processed_scores)
  3. x -= frequency * c_i + presence * [c_i > 0]                                (unpinned: transformers has no counterpart)
  4. s = x / temperature, top-k, top-p (logprobs_ref.kept_mask), then min_p: with e_i = exp(s_i - max s) over what is left,
     drop e_i < min_p.  Greedy rows: steps 1-3 only.
"""
from __future__ import annotations

import numpy as np
import torch

from logprobs_ref import kept_mask as _kept_k_p


def static_bias(V: int, logit_bias=None, allowed=None, banned=None, stop_ids=()) -> torch.Tensor:
    """The dense f32 [V] vector of step 1; `stop_ids` non-empty gives the early vector used while fewer than min_tokens are out."""
    b = torch.zeros(V, dtype=torch.float32)
    for t, v in (logit_bias or {}).items():
        b[int(t)] += float(v)
    if allowed is not None:
        out = torch.ones(V, dtype=torch.bool)
        out[torch.as_tensor(list(allowed), dtype=torch.long)] = False
        b[out] = -float("inf")
    for t in list(banned or ()) + list(stop_ids):
        b[int(t)] = -float("inf")
    return b


def processed_scores(logits, seen=None, rep=1.0, temp=1.0, counts=None, presence=0.0, frequency=0.0, bias=None) -> torch.Tensor:
    """bf16/f32 [B, V] -> f32 [B, V], every operation in fp32 in the order above."""
    s = logits.float().clone()
    if bias is not None:
        s = s + bias.float()
    if seen is not None and rep != 1.0:
        s = torch.where(seen.bool(), torch.where(s < 0, s * rep, s / rep), s)
    if counts is not None and (presence != 0.0 or frequency != 0.0):
        c = counts.float()
        pen = torch.tensor(frequency, dtype=torch.float32) * c + torch.tensor(presence, dtype=torch.float32)     # the three lines of step 3
        s = torch.where(c > 0, s - pen, s)
    return s / temp


def rel_e(s: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """e_i = exp(s_i - max s) over the kept tokens (float64), 0 elsewhere."""
    sd = torch.where(keep, s.double(), torch.full_like(s, -float("inf"), dtype=torch.float64))
    return torch.exp(sd - sd.max(dim=-1, keepdim=True).values)


def kept_mask(s: torch.Tensor, top_k=0, top_p=1.0, min_p=0.0) -> torch.Tensor:
    keep = _kept_k_p(s, top_k, top_p) & torch.isfinite(s)
    if min_p > 0.0:
        keep = keep & (rel_e(s, keep) >= float(np.float32(min_p)))
    return keep


def min_p_margin(s: torch.Tensor, top_k, top_p, min_p) -> float:
    """Smallest relative distance |e_i / min_p - 1| over the tokens top-k / top-p keep: the kept-set comparison is exact when no
    token sits within the device's expf error of the threshold."""
    keep = _kept_k_p(s, top_k, top_p) & torch.isfinite(s)
    e = rel_e(s, keep)[keep]
    return float((e / float(np.float32(min_p)) - 1).abs().min())


def logprobs(logits, seen=None, rep=1.0, temp=1.0, top_k=0, top_p=1.0, do_sample=False, min_p=0.0, counts=None, presence=0.0,
             frequency=0.0, bias=None):
    """-> (scores f32 [B, V] with -inf where masked, log-probs f32 [B, V]).  Greedy rows: steps 1-3, temperature 1, no masks beyond
    the -inf edits themselves."""
    if not do_sample:
        temp, top_k, top_p, min_p = 1.0, 0, 1.0, 0.0
    s = processed_scores(logits, seen, rep, temp, counts, presence, frequency, bias)
    keep = kept_mask(s, top_k, top_p, min_p)
    s = torch.where(keep, s, torch.full_like(s, -float("inf")))
    return s, torch.log_softmax(s, dim=-1)
