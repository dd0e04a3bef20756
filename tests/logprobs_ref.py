"""fp32 torch definition of the top-N log-probs (vLLM 0.7.2 V0 sampler semantics as restated in include/o3v.h, o3v_logprob_opts).

Processed scores: repetition penalty over the seen map (TF:logits_process.py:404-414), temperature (:301-303); sampling rows then keep
the top-k scores (ties with the k-th stay, :590-594) and, over the softmax of those, the smallest tail set whose mass exceeds top_p
(:527-539 keeps everything above the ascending prefix of mass <= 1 - top_p; tokens with the same score share one fate).  Log-probs
are log_softmax over the kept tokens, -inf elsewhere.  Order and ranks are taken on the processed scores themselves (the log-prob is
the score minus one normaliser), ties to the lower token id.
"""
from __future__ import annotations

import numpy as np
import torch


def processed_scores(logits: torch.Tensor, seen=None, rep: float = 1.0, temp: float = 1.0) -> torch.Tensor:
    """bf16/f32 [B, V] -> f32 [B, V] with the sampler's fp32 operations (x * rep / x / rep, then / temp)."""
    s = logits.float().clone()
    if seen is not None and rep != 1.0:
        m = seen.bool()
        s = torch.where(m, torch.where(s < 0, s * rep, s / rep), s)
    return s / temp


def kept_mask(s: torch.Tensor, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    keep = torch.ones_like(s, dtype=torch.bool)
    V = s.shape[-1]
    if 0 < top_k < V:
        kth = torch.topk(s, top_k, dim=-1).values[:, -1:]
        keep &= s >= kth
    if top_p < 1.0:
        for b in range(s.shape[0]):
            sb = s[b].double()
            e = torch.where(keep[b], torch.exp(sb - sb[keep[b]].max()), torch.zeros_like(sb))
            z = e.sum()
            vals, inv = torch.unique(e[keep[b]], sorted=True, return_inverse=True)   # ascending distinct values
            mass = torch.zeros_like(vals).index_add_(0, inv, e[keep[b]])
            cum = torch.cumsum(mass, 0)
            idx = int(torch.nonzero(cum > (1.0 - top_p) * z)[0]) if bool((cum > (1.0 - top_p) * z).any()) else len(vals) - 1
            keep[b] &= e >= vals[idx]
    return keep


def logprobs(logits, seen=None, rep=1.0, temp=1.0, top_k=0, top_p=1.0, do_sample=False):
    """-> (scores f32 [B,V] with -inf where masked, log-probs f32 [B,V]).  Greedy rows: penalty only, temperature 1, no masks."""
    if not do_sample:
        temp, top_k, top_p = 1.0, 0, 1.0
    s = processed_scores(logits, seen, rep, temp)
    keep = kept_mask(s, top_k, top_p)
    s = torch.where(keep, s, torch.full_like(s, -float("inf")))
    return s, torch.log_softmax(s, dim=-1)


def top_n(scores: torch.Tensor, lp: torch.Tensor, n: int):
    """(ids i64 [B, n], log-probs f32 [B, n]) in descending score order, ties to the lower id."""
    ids, vals = [], []
    for b in range(scores.shape[0]):
        sb = scores[b].numpy()
        order = np.lexsort((np.arange(sb.shape[0]), -sb.astype(np.float64)))[:n]
        ids.append(order)
        vals.append(lp[b].numpy()[order])
    return np.stack(ids), np.stack(vals)


def rank_of(scores: torch.Tensor, tok) -> np.ndarray:
    """1 + number of tokens whose processed score is strictly greater than the token's."""
    tok = torch.as_tensor(tok).long().view(-1)
    st = scores.gather(1, tok[:, None])
    return (1 + (scores > st).sum(dim=1)).numpy()
