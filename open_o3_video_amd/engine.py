"""O3VEngine: the MI355X generate engine (ViT -> merger -> prefill -> decode) over libo3v_hip.so.

Python only plans (index tables, buffers as torch-ROCm tensors, one ctypes call per stage); every FLOP runs
in the HIP library on the current torch stream.  There is no CPU / eager fallback: without a GPU and the
built library this raises.

Reference behaviour restated: GenerationMixin.generate/_sample on Qwen2_5_VLForConditionalGeneration as
the Open-o3-Video trainer and eval drive it (R:src/r1-v/src/open_r1/trainer/grpo_trainer.py:581-586,
R:eval/models/model_vllm.py:103-126); TF = transformers 5.15.0 models/qwen2_5_vl/modeling_qwen2_5_vl.py.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, guided, indexing
from .continuous import IDLE_BASE, ContinuousScheduler, default_session_columns
from .config import O3VConfig
from .weights import DeviceWeights

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # OPENAI_CLIP_MEAN/STD, TF:models/qwen2_vl/image_processing_qwen2_vl.py:94-101
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def prompt_arrays(input_ids, attention_mask=None, check_left_padding: bool = True):
    """Prompt ids and mask (tensor, array or list; one row may come 1-D) -> (ids i64 [B0, S], mask i64 [B0, S], pad i64 [B0]:
    masked slots per row).  A missing mask is all ones."""
    as_np = lambda a: np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.int64)
    ids = as_np(input_ids)
    if ids.ndim == 1:
        ids = ids[None]
    mask = np.ones_like(ids) if attention_mask is None else as_np(attention_mask)
    if mask.ndim == 1:
        mask = mask[None]
    pad = (mask == 0).sum(axis=1)
    if check_left_padding and not all((mask[b, pad[b]:] == 1).all() for b in range(ids.shape[0])):
        raise ValueError("only left padding is supported (padding_side='left', R:grpo_trainer.py:546)")
    return ids, mask, pad


def visual_identity(pixel_values, grid, frames, vis_embeds, pixel_values_videos, vgrid, video_frames):
    """The visual inputs of a prompt as the named tensors O3VEngine._prompt_key checksums: the group generate stores the hand-over
    under this identity and completion_logps looks it up, so both sides name them here."""
    return (("pv", pixel_values), ("grid", grid), ("frames", frames), ("vis", vis_embeds), ("pvv", pixel_values_videos),
            ("vgrid", vgrid), ("vframes", video_frames))


class DecodePlan(NamedTuple):
    """What one generate call decides about its decode before any buffer exists (plan_decode)."""
    B: int                  # decode rows: B0 prompts x G completions
    own_splits: int         # 128-key chunks of a row's own keys: its generated tokens (and its suffix behind a shared prefix)
    shared_prompt: bool     # the prompt's K/V is kept once per prompt (kc0 / vc0); the rows' caches hold only generated tokens
    Tmax: int               # slots per row of the decode caches
    nsplit: int             # o3v_decode_state.nsplit: context splits of the decode attention, negative = shared-read group kernel
    group: int              # o3v_decode_state.group: rows per shared-prefix (sub-)group, 0 = independent rows
    want_sync: bool         # the ticket / mailbox buffer of the in-launch hand-offs exists


def plan_decode(num_attention_heads: int, num_key_value_heads: int, head_dim: int, B0: int, G: int, S: int, T: int,
                group_attention: bool = True, group_attention_mode: str = "auto", fused: bool = True,
                nsplit_override: Optional[int] = None, suffix: int = 0) -> DecodePlan:
    """The decode attention plan of a generate call: B0 prompts of S slots, G completions each, T new tokens.  Pure arithmetic on
    the model's head geometry and the engine's switches (`fused`: the one-launch decode forms are allowed in this call;
    `nsplit_override`: the O3V_NSPLIT A/B switch).
    `suffix` = Lmax > 0 (generate(shared_prefix_len=S)): the G rows are G different continuations of ONE prefix of S tokens; each row's
    own cache starts with its suffix, left-padded to Lmax slots, and the generated tokens follow.  The group, sub-group and split
    choice is that of G completions of one prompt; only the rows' own key range grows by Lmax."""
    B = B0 * G
    suffix = int(suffix)
    # G completions of a prompt share its K/V (head_dim 128, own keys in <= 32 splits): the prompt's K/V is kept ONCE
    # (kc0 / vc0) and every row's cache holds only its generated tokens -- no G-fold copy of the prompt
    own_splits = (suffix + T + 127) // 128
    shared_prompt = G > 1 and head_dim == 128 and own_splits <= 32 and group_attention
    Tmax = suffix + T if shared_prompt else S + suffix + T
    # context splits of the decode attention: one 128-key chunk per block at 1-4 rows; from 8 rows on fewer, longer chunks
    # so that the grid stays near 640 blocks (measured, 7B: 8 rows 40 -> 20 splits 3.85 -> 3.72 ms/step; 16 independent rows
    # 32 -> 8 splits 2020 -> 2128 tok/s; 2 and 4 rows are best at 40)
    nsplit = max(1, min(64, (S + suffix + T + 127) // 128, max(1, 640 // max(1, B * num_key_value_heads))))
    if nsplit_override is not None:
        nsplit = nsplit_override
    # G completions of a prompt share its K/V: the group kernel reads the prompt keys once per group (head_dim 128,
    # G * n_rep <= 64 query rows per kv head, prefix splits + own-key splits <= 64)
    n_rep = num_attention_heads // num_key_value_heads
    group = G if shared_prompt else 0
    mode = group_attention_mode
    if group:
        # the one-pass kernel holds a sub-group's query rows as MFMA columns (<= 64); sub-groups of 4 rows measured best
        sub = max(d for d in range(1, G + 1) if G % d == 0 and d <= 4 and d * n_rep <= 64)
        if mode == "auto":
            # measured, 7B dims, ms per decode step (tools/measure_configs.py rollout / rollout_eval), per-row kernel reading
            # the leader's prefix through the shared L2 | one-pass kernel in sub-groups of 4 (prefix + own keys, one launch):
            #   S=4.5k: G=4 3.45 | 3.53   G=8 3.71 | 3.79   G=12 4.06 | 4.09   G=16 4.42 | 4.36
            #   S=10k : G=8 4.37 | 3.97
            mode = "kernel" if (S >= 8192 or B >= 16) and sub > 1 else "shared_read"
        if mode == "kernel" and sub > 1:
            group = sub
            # prefix splits: ~320 blocks in all (measured: G=16, S=4.5k 36 -> 18 splits 4.80 -> 4.63 ms/step; G=8, S=10k is
            # best left at its 63)
            nsplit = max(1, min(64 - own_splits, (S + 127) // 128, max(1, 320 // (num_key_value_heads * (B // sub)))))
            if S >= 8192:
                nsplit = max(1, min(64 - own_splits, (S + 127) // 128))
        else:
            nsplit = -nsplit
    # tickets / mailboxes of the one-launch attention block (batch 1 only)
    want_sync = bool(fused and B == 1)
    return DecodePlan(B, own_splits, bool(shared_prompt), Tmax, nsplit, group, want_sync)


def kv_cache_in_effect(kv_cache_dtype: str, head_dim: int, plan: DecodePlan) -> str:
    """The K/V cache format a generate call decodes on: "fp8" iff the engine asks for it (`O3VEngine.kv_cache_dtype`), the kernels
    exist for the head size (128) and every row streams its own context (`not plan.shared_prompt`); else "bf16".  Shared-prompt
    groups keep bf16: their prompt K/V is read once per group, so the step is latency-bound there and halving those bytes buys
    nothing, while the rows' own caches hold only the generated tokens."""
    return "fp8" if kv_cache_dtype == "fp8" and head_dim == 128 and not plan.shared_prompt else "bf16"


def mlp_weights_in_effect(images, plan: DecodePlan) -> str:
    """The weight format gate/up and down_proj of a generate call stream -- decide_regime's rule (csrc/o3v_engine.hip) restated on
    the keys of DeviceWeights.t (`images`): "mxfp4" where the call decodes on fp8 rows (<= 3 independent rows) or fp8 fragments
    (4..32 rows) and BOTH MLP matrices keep the MXFP4 image of that form, "fp8" on those rows / fragments otherwise, else "bf16"."""
    def has(*sfx):
        return all(f"l0.{m}{x}" in images for m in ("gu_w", "down_w") for x in sfx)
    if plan.B <= 3 and plan.group <= 1 and has("8") and all(f"l0.{m}8" in images for m in ("qkv_w", "o_w")):
        return "mxfp4" if has("4", "4s") else "fp8"
    if plan.B >= 4 and has("8p") and "l0.o_w8p" in images:
        return "mxfp4" if has("4p", "4ps") else "fp8"
    return "bf16"


def trimmed_length(gen: np.ndarray, eos_ids, ended: dict, done: int) -> int:
    """Columns of gen i64 [B, done] that HF would have produced: up to and including the step at which the last row finished.
    A row finishes at its first id of `eos_ids`, a row the stop checker ended (`ended`: row -> tokens it keeps) at the column the
    checker named if that comes first, any other row at `done`; at least one column stays."""
    hit = np.isin(gen, list(eos_ids))
    fin_at = np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, done)
    for b, end in ended.items():
        fin_at[b] = min(fin_at[b], end)
    return int(max(1, min(done, fin_at.max())))


@dataclass
class Logprobs:
    """Top-N log-probs of a run of positions (vLLM SamplingParams.logprobs / prompt_logprobs; o3v_logprob_opts in include/o3v.h)."""
    token: torch.Tensor                # f32 [B, T]: log-prob of the emitted (decode) / target (prompt) token
    rank: torch.Tensor                 # i32 [B, T]: 1 + tokens with a strictly larger log-prob
    top_ids: torch.Tensor              # i32 [B, T, N]: descending log-prob, ties to the lower id
    top: torch.Tensor                  # f32 [B, T, N]

    @classmethod
    def zeros(cls, B: int, T: int, n: int, device) -> "Logprobs":
        return cls(token=torch.zeros((B, T), dtype=torch.float32, device=device),
                   rank=torch.zeros((B, T), dtype=torch.int32, device=device),
                   top_ids=torch.zeros((B, T, n), dtype=torch.int32, device=device),
                   top=torch.zeros((B, T, n), dtype=torch.float32, device=device))


@dataclass
class GenerateOutput:
    sequences: torch.Tensor            # i64 [B, S+T]
    margins: Optional[torch.Tensor]    # f32 [B, T]: greedy top1-top2 margin / sampled token log-prob
    n_steps: int
    timings: dict
    # generate(logprobs=N): the processed distribution each token was drawn from, [B, n_steps(, N)]
    logprobs: Optional[Logprobs] = None
    # generate(prompt_logprobs=N): [B0, S-1(, N)] per prompt, column j = prompt token j+1 given the tokens before it (left-padded
    # rows: the columns before the row's first real token carry no meaning)
    prompt_logprobs: Optional[Logprobs] = None


@dataclass
class ContinuousRequest:
    """One request of O3VEngine.generate_continuous: the prompt, its precomputed visual inputs (as generate takes them) and its
    own completion length."""
    ids: object                               # 1-D token ids
    max_new_tokens: int = 16
    vis_embeds: Optional[torch.Tensor] = None
    image_grid_thw: object = None
    video_grid_thw: object = None
    second_per_grid_ts: object = None


@dataclass
class ContinuousOutput:
    tokens: torch.Tensor                      # i64 [n] (host): the generated tokens, trimmed as generate trims a row (first EOS kept)
    margins: Optional[torch.Tensor]           # f32 [n] top1-top2 margins of those tokens
    row: int                                  # where it ran: decode row, first column, session (1-based)
    t0: int
    session: int
    timings: dict                             # of the whole call; filled when it returns
    sequences: torch.Tensor                   # i64 [1, S + n] (host): prompt + tokens


class _DecodeBuffers:
    """The device state of one generate call's decode: every tensor whose address goes into o3v_decode_state / o3v_sampling_opts /
    o3v_logprob_opts, the structs themselves (st; so / lp_opts: None when the call does not use them) and the host_stats array.
    The structs hold bare addresses, so this object lives until the last o3v_llm_decode_ex call and the final check_waits()."""

    def __init__(self, eng: "O3VEngine", plan: DecodePlan, S, T, G, ids_rep, pad_rep, eos_token_ids, row_ids, return_margins, n_lp,
                 sampling, knobs, cosd, sind, logits, kc, vc, kc0, vc0, kv8=None, kv8_emulate=False, own=None, guide=None,
                 ragged=None):
        tc, dev = eng.cfg.text, eng.dev
        B, V = plan.B, tc.vocab_size
        zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        addr = lambda t: 0 if t is None else t.data_ptr()
        # kv8 = (k8, v8, k8s, v8s): the fp8 K/V caches; kc / vc are then the bf16 staging rows [B, Hkv, 1, D] of the new token
        # own = (own_past, own_lo i32 [B]): the rows are suffixes behind ONE shared prefix of S tokens (kc0 / vc0, one entry for all
        # B rows); their own caches already hold own_past slots, the first own_lo[b] of them padding.  ids_rep is then the rows'
        # own left-padded prompts (any width), pad_rep the padding in front of the prefix
        self.caches, self.tables, self.logits = (kc, vc, kc0, vc0, kv8), (cosd, sind), logits
        self.seen = zeros((B, V), torch.uint8)
        if knobs["rep_penalty"] != 1.0:
            ids_dev = torch.from_numpy(ids_rep.astype(np.int32)).to(dev)
            _lib.call("o3v_mark_seen", _ptr(ids_dev), _ptr(self.seen), B, ids_rep.shape[1], V, _stream())
        self.cur_tok, self.finished = zeros(B, torch.int32), zeros(B, torch.int32)
        self.out_ids = torch.full((B, T), knobs["pad_id"], dtype=torch.int32, device=dev)
        self.margins = zeros((B, T), torch.float32) if return_margins else None
        self.eos = torch.tensor(list(eos_token_ids) or [0], dtype=torch.int32, device=dev)
        self.k_lo = torch.from_numpy(pad_rep.astype(np.int32)).to(dev)
        self.rid = torch.tensor(list(row_ids) if row_ids is not None else list(range(B)), dtype=torch.int32, device=dev)
        n_rep_total = B * tc.num_attention_heads
        self.part_o = empty(n_rep_total * 64 * tc.head_dim, torch.float32)
        self.part_ml = empty(n_rep_total * 64 * 2, torch.float32)
        self.scratch = empty((B, _lib.SAMPLE_SCRATCH_FLOATS if knobs["do_sample"] or n_lp or sampling or guide is not None else 256),
                             torch.float32)
        # guided decoding: the rows' automaton states, double-buffered (step s reads half s & 1, its last stage writes the other)
        self.guide = self.go = self.guide_state = None
        if guide is not None:
            self.guide = guide      # keeps the device table alive
            self.guide_state = torch.full((2, B), int(guide.start), dtype=torch.int32, device=dev)
            self.go = _lib.GuidedOpts(next=guide.table.data_ptr(), n_states=int(guide.n_states), ldn=int(guide.ldn),
                                      state=self.guide_state.data_ptr())
        self.so = None
        if sampling:    # the extended sampler kernels: static-edit vectors and (penalties only) the u16 output counts
            self.bias, self.early = (None if v is None else torch.from_numpy(v).to(dev)
                                     for v in (sampling["bias"], sampling["bias_early"]))
            self.counts = zeros((B, V), torch.int16) if sampling["counts"] else None
            self.so = _lib.SamplingOpts(min_p=sampling["min_p"], presence=sampling["presence"], frequency=sampling["frequency"],
                                        min_tokens=sampling["min_tokens"], bias=addr(self.bias), bias_early=addr(self.early),
                                        out_counts=addr(self.counts))
        self.lp = self.lp_opts = None
        if n_lp:
            lp = self.lp = Logprobs.zeros(B, T, n_lp, dev)
            self.lp_opts = _lib.LogprobOpts(n=n_lp, chosen_lp=lp.token.data_ptr(), chosen_rank=lp.rank.data_ptr(),
                                            top_ids=lp.top_ids.data_ptr(), top_lp=lp.top.data_ptr())
        self.x = empty((B, tc.hidden_size), torch.bfloat16)
        nbytes = _lib.load().o3v_llm_workspace_bytes(C.byref(eng.w.llm), B)
        self.ws = empty(nbytes, torch.uint8)
        # tickets / mailboxes of the in-launch hand-offs: zeroed once per call, epochs count the launches
        self.sync = None
        if plan.want_sync:
            self.sync = zeros(_lib.load().o3v_decode_sync_bytes(), torch.uint8)
            if getattr(eng, "_debug_poison_sync", False):     # test hook: tickets that can never reach "last" -> the waits give up
                self.sync[:1024].view(torch.int32).fill_(0x40000000)
        shared = plan.shared_prompt
        # ragged = row_base i32 [B] (or a list to upload): every row has its own context row_base[b] + step + 1 (continuous batching);
        # q/k/v then writes the new token's K/V into staging rows and the attention kernel appends them at the row's own slot
        state_type = _lib.DecodeStateOwn if ragged is None else _lib.DecodeStateRagged
        self.st = state_type(B=B, S=S, Tmax=plan.Tmax, Tnew=T, nsplit=plan.nsplit, x=self.x.data_ptr(), kcache=kc.data_ptr(),
                             vcache=vc.data_ptr(), cosT=cosd.data_ptr(), sinT=sind.data_ptr(), logits=logits.data_ptr(),
                             seen=self.seen.data_ptr(), cur_tok=self.cur_tok.data_ptr(), finished=self.finished.data_ptr(),
                             out_ids=self.out_ids.data_ptr(), margins=addr(self.margins), eos_ids=self.eos.data_ptr(),
                             k_lo=self.k_lo.data_ptr(), row_id=self.rid.data_ptr(), part_o=self.part_o.data_ptr(),
                             part_ml=self.part_ml.data_ptr(), sample_scratch=self.scratch.data_ptr(),
                             workspace=self.ws.data_ptr(), ws_bytes=nbytes, group=plan.group, sync=addr(self.sync),
                             kprefix=kc0.data_ptr() if shared else 0, vprefix=vc0.data_ptr() if shared else 0,
                             prefix_cap=int(kc0.shape[3]) if shared else 0, rows_per_prompt=G if shared else 0, **knobs)
        self.own_lo = None
        if own is not None:
            self.own_lo = torch.from_numpy(np.ascontiguousarray(own[1], dtype=np.int32)).to(dev)
            self.st.own_past, self.st.own_lo = int(own[0]), self.own_lo.data_ptr()
        # decode forwards, launches in their layer loops, fused / stand-alone attention halves
        self.host_stats = (C.c_longlong * 4)(0, 0, 0, 0)
        self.st.host_stats = C.cast(self.host_stats, C.c_void_p)
        self.st.flags = (0 if eng.qkv_fused_norm else _lib.DECODE_NO_QKV_FUSED_NORM) | (_lib.DECODE_KV8_EMULATE if kv8_emulate else 0)
        if kv8 is not None:
            self.st.k8, self.st.v8, self.st.k8s, self.st.v8s = (t.data_ptr() for t in kv8)
        self.row_base = self.stage = None
        if ragged is not None:
            self.row_base = torch.as_tensor(ragged, dtype=torch.int32).to(dev)
            self.stage = tuple(empty((B, tc.num_key_value_heads, 1, tc.head_dim), torch.bfloat16) for _ in range(2))
            self.st.row_base, self.st.kstage, self.st.vstage = self.row_base.data_ptr(), *(t.data_ptr() for t in self.stage)
            self.st.flags |= _lib.DECODE_RAGGED

    def check_waits(self):
        """Reads the sticky time-out word of the in-launch waits (a device-to-host copy); raises if one of them gave up."""
        if self.sync is None:
            return
        code = int(self.sync[_lib.SYNC_TMO_BYTE:_lib.SYNC_TMO_BYTE + 4].view(torch.int32)[0].item())
        if code:
            raise O3VEngine._InLaunchWaitGaveUp(f"decode: an in-launch wait gave up (code {code:#x})")


class O3VEngine:
    MAX_ROWS = 32   # decode rows per call: the skinny MFMA GEMM multiplies 16 weight rows against one or two 16-row blocks of x

    def __init__(self, cfg: O3VConfig, weights: DeviceWeights):
        if not torch.cuda.is_available():
            raise _lib.O3VError("O3VEngine needs a ROCm GPU (no CPU path)")
        _lib.load()
        self.cfg, self.w = cfg, weights
        self.dev = weights.device
        tc = cfg.text
        D = tc.head_dim
        # inv_freq exactly as torch computes it on the host (TF:521)
        inv = 1.0 / (tc.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float) / D))
        self.inv_freq = inv.to(self.dev)
        self.q3 = cfg.arch == "qwen3_vl"
        axis = indexing.mrope_axis_table_interleaved(tc.mrope_section, D // 2) if tc.mrope_interleaved \
            else indexing.mrope_axis_table(tc.mrope_section)
        self.axis_of = torch.from_numpy(axis).to(self.dev)
        # host arrays (read by the launcher, passed by value); Qwen3-VL's processor normalises with mean = std = 0.5
        self.clip_mean = (C.c_float * 3)(*((0.5, 0.5, 0.5) if self.q3 else CLIP_MEAN))
        self.clip_std = (C.c_float * 3)(*((0.5, 0.5, 0.5) if self.q3 else CLIP_STD))
        self._vit_plan_cache = {}
        self._prefix = {}   # prefix_key -> {"ids", "k", "v"}: prompt K/V kept for reuse (see generate(prefix_key=...))
        # The prompt of the last group generate (num_return_sequences > 1): its K/V, kept once anyway, and the hidden row that predicts
        # completion token 0.  The policy's log-prob pass over those completions (completion_logps, R:grpo_trainer.py:612-613) finds the
        # SAME prompt -- ids, mask, grids, positions and visual tensors equal bit for bit (_prompt_key) -- and skips the tower and the
        # prompt prefill; anything else (another model, a video whose second_per_grid_ts the trainer deleted) recomputes.
        self.reuse_prompt_kv = os.environ.get("O3V_REUSE_PROMPT_KV", "1") != "0"
        self._last_prompt = None
        self.timings_last_logps = {}
        # bumped by load_weights: every cache derived from the weights (prefix K/V, the hand-over, the Qwen3-VL position table
        # in _vit_plan_cache, the vLLM facade's visual tokens) belongs to one version
        self.weights_version = 0
        self.group_attention = os.environ.get("O3V_GROUP_ATTENTION", "1") != "0"   # A/B switch for the shared-prefix kernel
        self.fused_decode = os.environ.get("O3V_FUSED_DECODE", "1") != "0"         # A/B switch for the one-launch attention block
        self.group_attention_mode = os.environ.get("O3V_GROUP_MODE", "auto")
        self.qkv_fused_norm = os.environ.get("O3V_QKV_FUSED_NORM", "1") != "0"     # A/B switch for the norm fused into q/k/v at 8 rows
        # video rope arithmetic (indexing.rope_index): "tf5" = transformers 5.15 (goldens G5b / G14 / G15), "pinned" = the
        # libraries the reference installs (transformers @336dc69d, vllm 0.7.2).  The facades choose; images do not depend on it.
        self.position_mode = "tf5"
        # opt-in (BASELINE config #5): the LLM prefill / log-prob linears as fp8 x fp8 on the matrix cores (W8A8: per-token activation
        # scales, the fp8 rows + per-row scales that fp8_decode builds).  Off by default: the bf16 path and its goldens are untouched.
        self.fp8_prefill = False
        # opt-in (vLLM kv_cache_dtype): "fp8" keeps the K/V cache of independent-row decodes as e4m3fn rows with one power-of-two
        # scale per (token, kv head) -- 132 instead of 256 bytes per row; see kv_cache_in_effect for where it applies.  "bf16": off.
        self.kv_cache_dtype = "bf16"

    # ------------------------------------------------------------------------------------------ vision
    def _vit_plan(self, grid_thw):
        key = indexing._grid_key(grid_thw)
        p = self._vit_plan_cache.get(key)
        if p is not None:
            return p
        vc = self.cfg.vision
        if self.q3:
            return self._vit_plan_q3(key)
        widx, cu_win, cu_full, pos = indexing.vision_plan(key, vc.spatial_merge_size, vc.window_size, vc.patch_size)
        unit = vc.merge_unit
        P = int(cu_full[-1])
        # rotary table in window order (TF:125-134, :441-446): fp32, computed as torch does on the host
        rdim = vc.head_dim // 2
        inv = 1.0 / (10000.0 ** (torch.arange(0, rdim, 2, dtype=torch.float) / rdim))
        rot = (torch.from_numpy(pos).unsqueeze(-1) * inv).flatten(1)            # [P, hd/2]
        wi = torch.from_numpy(widx)
        rot = rot.reshape(P // unit, unit, -1)[wi].reshape(P, -1)
        plan = dict(
            P=P,
            win_idx=wi.to(torch.int32).to(self.dev),
            rev_idx=torch.argsort(wi).to(torch.int32).to(self.dev),
            cos=rot.cos().contiguous().to(self.dev), sin=rot.sin().contiguous().to(self.dev),
            tiles_win=torch.from_numpy(indexing.segment_tiles(cu_win)).to(self.dev),
            tiles_full=torch.from_numpy(indexing.segment_tiles(cu_full)).to(self.dev),
        )
        if len(self._vit_plan_cache) > 16:
            self._vit_plan_cache.clear()
        self._vit_plan_cache[key] = plan
        return plan

    def _vit_plan_q3(self, key):
        """Qwen3-VL (TF3:606-737): no windows -- patches stay in merge-block order, one attention segment per temporal patch;
        the rotary table is stored head_dim_pad/2 wide (the padded frequencies rotate zeros); the learned position table is
        resampled to this grid once (TF3:643-710: four taps, table dtype x fp32 weights, summed in fp32 in tap order)."""
        vc = self.cfg.vision
        _, _, cu_full, pos = indexing.vision_plan(key, vc.spatial_merge_size, vc.patch_size * vc.spatial_merge_size, vc.patch_size)
        P = int(cu_full[-1])
        rdim = vc.head_dim // 2
        inv = 1.0 / (10000.0 ** (torch.arange(0, rdim, 2, dtype=torch.float) / rdim))
        rot = (torch.from_numpy(pos).unsqueeze(-1) * inv).flatten(1)            # [P, hd/2]
        halfp = vc.head_dim_pad // 2
        cos, sin = torch.ones((P, halfp)), torch.zeros((P, halfp))
        cos[:, :rot.shape[1]], sin[:, :rot.shape[1]] = rot.cos(), rot.sin()
        side = int(round(vc.num_position_embeddings ** 0.5))
        idx, wt = indexing.pos_embed_taps(key, side, vc.spatial_merge_size)
        table = self.w.t["v.pos_embed"]
        idx, wt = torch.from_numpy(idx).to(self.dev), torch.from_numpy(wt).to(self.dev)
        taps = [table[idx[:, k]] * wt[:, k, None] for k in range(4)]           # bf16 x fp32 -> fp32
        pe = (((taps[0] + taps[1]) + taps[2]) + taps[3]).to(torch.bfloat16).contiguous()
        plan = dict(P=P, cos=cos.contiguous().to(self.dev), sin=sin.contiguous().to(self.dev), pos_embed=pe,
                    tiles_full=torch.from_numpy(indexing.segment_tiles(cu_full)).to(self.dev))
        if len(self._vit_plan_cache) > 16:
            self._vit_plan_cache.clear()
        self._vit_plan_cache[key] = plan
        return plan

    def pixels_from_processor(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """HF-processor pixel_values f32 [P,1176] -> bf16 [P,Kp] (TF:1090 cast, zero pad)."""
        vc = self.cfg.vision
        pv = pixel_values.to(self.dev, torch.float32).contiguous()
        out = torch.empty((pv.shape[0], vc.patch_k_pad), dtype=torch.bfloat16, device=self.dev)
        _lib.call("o3v_cast_pad_f32_bf16", _ptr(pv), _ptr(out), pv.shape[0], pv.shape[1], vc.patch_k_pad, _stream())
        return out

    def frames_grid(self, frames: torch.Tensor) -> np.ndarray:
        """grid_thw [T,3] of frames-as-images [T,3,H,W]: every frame is its own image of one temporal patch."""
        ps = self.cfg.vision.patch_size
        return np.asarray([[1, frames.shape[2] // ps, frames.shape[3] // ps]] * frames.shape[0], dtype=np.int64)

    def pixels_from_frames(self, frames: torch.Tensor):
        """frames [T,3,H,W] uint8 or f32 (0..255, H,W multiples of 28) -> (bf16 [P,Kp], grid_thw [T,3])."""
        vc = self.cfg.vision
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError("frames must be [T,3,H,W]")
        T, _, H, W = frames.shape
        ps = vc.patch_size
        if H % (2 * ps) or W % (2 * ps):
            raise ValueError(f"frame size must be a multiple of {2 * ps} (smart_resize output)")
        is_u8 = frames.dtype == torch.uint8
        fr = frames.to(self.dev).contiguous() if is_u8 else frames.to(self.dev, torch.float32).contiguous()
        P = T * (H // ps) * (W // ps)
        out = torch.empty((P, vc.patch_k_pad), dtype=torch.bfloat16, device=self.dev)
        _lib.call("o3v_patchify_ps", _ptr(fr), int(is_u8), _ptr(out), T, H, W, vc.patch_k_pad, ps, self.clip_mean, self.clip_std,
                  _stream())
        return out, self.frames_grid(frames)

    def pixels_from_video(self, frames: torch.Tensor):
        """ONE native video [T,3,H,W] uint8 or f32 (0..255) -> (bf16 [ceil(T/2)*gh*gw, Kp], grid [[ceil(T/2), gh, gw]]): temporal
        patch k holds frames 2k and 2k+1, an odd count repeats the last frame (TF:models/qwen2_vl/video_processing_qwen2_vl.py:236-274;
        R:src/r1-v/src/open_r1/vision_process.py:319-333 pads frame lists the same way)."""
        vc = self.cfg.vision
        if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] == 0:
            raise ValueError("video frames must be [T,3,H,W] with T >= 1")
        T, _, H, W = frames.shape
        ps = vc.patch_size
        if H % (2 * ps) or W % (2 * ps):
            raise ValueError(f"frame size must be a multiple of {2 * ps} (smart_resize output)")
        is_u8 = frames.dtype == torch.uint8
        fr = frames.to(self.dev).contiguous() if is_u8 else frames.to(self.dev, torch.float32).contiguous()
        gt = (T + 1) // 2
        out = torch.empty((gt * (H // ps) * (W // ps), vc.patch_k_pad), dtype=torch.bfloat16, device=self.dev)
        _lib.call("o3v_patchify_video", _ptr(fr), int(is_u8), _ptr(out), T, H, W, vc.patch_k_pad, ps, self.clip_mean, self.clip_std,
                  _stream())
        return out, np.asarray([[gt, H // ps, W // ps]], dtype=np.int64)

    def vit_forward(self, pixels_bf16: torch.Tensor, grid_thw) -> torch.Tensor:
        """TF:408-471 -> merged visual tokens bf16 [P/4, out_hidden] in original order."""
        vc = self.cfg.vision
        plan = self._vit_plan(grid_thw)
        P = plan["P"]
        if pixels_bf16.shape[0] != P or pixels_bf16.shape[1] != vc.patch_k_pad:
            raise ValueError(f"pixel rows {tuple(pixels_bf16.shape)} do not match grid ({P} patches)")
        if self.q3:
            # [1 + n_deep, P/4, out_hidden]: row block 0 = the merged visual tokens, 1.. = the DeepStack features (TF3:839-862) that
            # prefill adds to the first decoder layers' outputs at the visual positions; every consumer takes this one tensor
            nd = len(vc.deepstack_visual_indexes)
            nbytes = _lib.load().o3v_vit3_workspace_bytes(C.byref(self.w.vit3), P)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            out = torch.empty((1 + nd, P // vc.merge_unit, vc.out_hidden_size), dtype=torch.bfloat16, device=self.dev)
            _lib.call("o3v_vit3_forward", C.byref(self.w.vit3), _ptr(pixels_bf16), P, _ptr(plan["pos_embed"]), _ptr(plan["cos"]),
                      _ptr(plan["sin"]), _ptr(plan["tiles_full"]), plan["tiles_full"].shape[0], _ptr(ws), nbytes, _ptr(out[0]),
                      _ptr(out[1:]) if nd else None, _stream())
            return out
        nbytes = _lib.load().o3v_vit_workspace_bytes(C.byref(self.w.vit), P)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        out = torch.empty((P // vc.merge_unit, vc.out_hidden_size), dtype=torch.bfloat16, device=self.dev)
        _lib.call("o3v_vit_forward", C.byref(self.w.vit), _ptr(pixels_bf16), P, _ptr(plan["win_idx"]), _ptr(plan["rev_idx"]),
                  _ptr(plan["cos"]), _ptr(plan["sin"]), _ptr(plan["tiles_win"]), plan["tiles_win"].shape[0],
                  _ptr(plan["tiles_full"]), plan["tiles_full"].shape[0], _ptr(ws), nbytes, _ptr(out), _stream())
        return out

    # ------------------------------------------------------------------------------------------ text
    def mrope_table(self, pos3: np.ndarray):
        """pos3 int [3, T] -> cos, sin bf16 [T, D] on device."""
        D = self.cfg.text.head_dim
        T = pos3.shape[1]
        p = torch.from_numpy(np.ascontiguousarray(pos3.astype(np.int32))).to(self.dev)
        cos = torch.empty((T, D), dtype=torch.bfloat16, device=self.dev)
        sin = torch.empty_like(cos)
        _lib.call("o3v_mrope_table", _ptr(p), _ptr(self.inv_freq), _ptr(self.axis_of), _ptr(cos), _ptr(sin), T, D, _stream())
        return cos, sin

    def embed(self, input_ids: np.ndarray, vis: Optional[torch.Tensor], first: int = 0, n_image_rows: Optional[int] = None) -> torch.Tensor:
        """inputs_embeds of the (flattened) prompt; `first` > 0 returns only rows first.. (prefix-KV reuse).  `vis` holds the
        image tokens followed by the video tokens (n_image_rows of the former; default: as many as image placeholders)."""
        src, n_img, n_vid = indexing.embed_source_rows(input_ids, self.cfg.image_token_id, self.cfg.video_token_id, n_image_rows)
        if vis is not None and vis.dim() == 3:      # Qwen3-VL: [1 + n_deep, n, H], block 0 = the visual tokens
            vis = vis[0]
        n_rows = 0 if vis is None else vis.shape[0]
        n_img_rows = n_img if n_image_rows is None else int(n_image_rows)
        if n_img != n_img_rows or n_img + n_vid != n_rows:
            what = "Video" if n_img == n_img_rows else "Image"
            raise ValueError(f"{what} features and {what.lower()} tokens do not match, tokens: {n_img} image + {n_vid} video, "
                             f"features: {n_img_rows} image + {n_rows - n_img_rows} video")
        src = src[first:]
        H = self.cfg.text.hidden_size
        T = src.shape[0]
        x = torch.empty((T, H), dtype=torch.bfloat16, device=self.dev)
        s = torch.from_numpy(src).to(self.dev)
        _lib.call("o3v_embed_scatter", _ptr(self.w.t["l.embed"]), _ptr(vis), _ptr(s), _ptr(x), T, H, _stream())
        return x

    def _prompt_key(self, ids, mask, pos, tensors):
        """Identity of a prompt for the generate -> log-prob hand-over: token ids, mask and rope positions as bytes, every visual input
        by shape, dtype and two 64-bit checksums of its bytes (a plain sum and a position-weighted one, computed where the tensor
        lives)."""
        # the weights version: a hand-over never crosses load_weights (getattr: the key is also computed for bare namespaces)
        parts = [ids.tobytes(), mask.tobytes(), pos.tobytes(), self.position_mode, getattr(self, "weights_version", 0)]
        for name, t in tensors:
            if t is None:
                parts.append((name, None))
                continue
            if isinstance(t, (list, tuple)):
                t = torch.cat([torch.as_tensor(u).reshape(-1).view(torch.uint8) for u in t])
            t = torch.as_tensor(t)
            raw = t.detach().contiguous().reshape(-1).view(torch.uint8)
            pad = (-raw.numel()) % 4
            if pad:
                raw = torch.cat([raw, raw.new_zeros(pad)])
            w = raw.view(torch.int32).to(torch.int64)
            wt = (torch.arange(w.numel(), device=w.device, dtype=torch.int64) & 0xFFFF) + 1
            parts.append((name, tuple(t.shape), str(t.dtype), int(w.sum().item()), int((w * wt).sum().item())))
        return tuple(parts)

    def _visual(self, pixel_values, image_grid_thw, frames, vis_embeds, pixel_values_videos, video_grid_thw, video_frames):
        """The visual side of a call -> (vis, image grid, video grid, n_image_rows): image tokens first, video tokens after them
        (each modality is scattered to its own placeholders in order, TF:1206-1215; the tower treats every temporal patch as its
        own attention segment either way, TF:vision_utils.py:60-65, so the two runs are independent)."""
        as_np = lambda g: None if g is None else np.asarray(g.cpu() if torch.is_tensor(g) else g, dtype=np.int64).reshape(-1, 3)
        grid, vgrid = as_np(image_grid_thw), as_np(video_grid_thw)
        if vis_embeds is not None:
            n_img = None if vgrid is None else (0 if grid is None else int((grid.prod(axis=1) // self.cfg.vision.merge_unit).sum()))
            return vis_embeds, grid, vgrid, n_img
        parts = []
        if frames is not None:
            px, grid = self.pixels_from_frames(frames)
            parts.append(self.vit_forward(px, grid))
        elif pixel_values is not None:
            parts.append(self.vit_forward(self.pixels_from_processor(pixel_values), grid))
        n_img = None
        if video_frames is not None or pixel_values_videos is not None:
            n_img = parts[0].shape[-2] if parts else 0
            if video_frames is not None:
                vids = video_frames if isinstance(video_frames, (list, tuple)) else [video_frames]
                px_g = [self.pixels_from_video(v) for v in vids]
                px, vgrid = torch.cat([p for p, _ in px_g]), np.concatenate([g for _, g in px_g])
            else:
                px = self.pixels_from_processor(pixel_values_videos)
            parts.append(self.vit_forward(px, vgrid))
        if not parts:
            return None, None, None, None
        return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=-2)), grid, vgrid, n_img

    def _positions(self, ids, mask, grid, vgrid, second_per_grid_ts):
        cfg = self.cfg
        if grid is None and vgrid is None:
            p1 = np.where(mask == 0, 0, np.cumsum(mask, axis=1) - 1)
            return np.broadcast_to(p1[None], (3,) + ids.shape).copy(), np.zeros(ids.shape[0], dtype=np.int64)
        return indexing.rope_index(ids, mask, grid, cfg.image_token_id, cfg.vision.spatial_merge_size, video_grid_thw=vgrid,
                                   video_token_id=cfg.video_token_id, second_per_grid_ts=second_per_grid_ts,
                                   tokens_per_second=cfg.vision.tokens_per_second, split_video_frames=self.q3,
                                   mode="tf5" if self.q3 else self.position_mode)

    def alloc_cache(self, B, Tmax):
        tc = self.cfg.text
        shape = (tc.num_hidden_layers, B, tc.num_key_value_heads, Tmax, tc.head_dim)
        return (torch.empty(shape, dtype=torch.bfloat16, device=self.dev),
                torch.empty(shape, dtype=torch.bfloat16, device=self.dev))

    def prefill(self, x: torch.Tensor, pos3: np.ndarray, pad: Sequence[int], B: int, S: int, kc, vc, past: int = 0,
                deepstack=None, prefix=None, own_lo=None):
        """Runs the prompt through the LLM (TF:790-872); x [B*S,H] becomes the last layer's residual stream.
        past > 0: `past` tokens per row are already computed (HF `past_key_values` semantics); x / pos3 are the S tokens
        after them.  By default they sit in slots 0..past-1 of kc / vc.  prefix = (kc0, vc0, rows_per_prefix): they sit ONCE
        per prompt in kc0 / vc0 [layers, B/rows_per_prefix, Hkv, >=past, D] instead, and kc / vc hold only the new tokens (the
        G completions of a prompt behind one copy of its K/V).  deepstack = (input_ids, vis [1+n_deep, n, H]) of a Qwen3-VL
        prompt: the DeepStack features are added after the first decoder layers at the visual rows (TF3:839-862).
        own_lo [B] (with prefix): the first own_lo[b] of row b's S tokens are left padding (suffixes of unequal length behind one
        prefix); their keys are masked, their rows of x carry no meaning."""
        Tmax = kc.shape[3]
        cos, sin = self.mrope_table(pos3.reshape(3, B * S))
        if own_lo is not None and prefix is None:
            raise ValueError("own_lo needs a shared prefix entry")
        tiles = torch.from_numpy(indexing.prefill_tiles(B, S, pad, past=past, own_lo=own_lo)).to(self.dev)
        nbytes = _lib.load().o3v_llm_workspace_bytes(C.byref(self.w.llm), B * S)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        opts = _lib.PrefillOpts()
        if self.fp8_prefill:
            if not getattr(self.w, "fp8_decode", False):
                raise _lib.O3VError("fp8_prefill needs the fp8 weight rows (DeviceWeights(fp8_decode=True) / quantization='fp8')")
            opts.w8a8 = 1
        keep = []
        if deepstack is not None and deepstack[1] is not None and deepstack[1].dim() == 3 and deepstack[1].shape[0] > 1:
            ids_all, vis = deepstack
            rows, src = indexing.deepstack_rows(ids_all, self.cfg.image_token_id, first=past, video_token_id=self.cfg.video_token_id)
            rows_d, src_d = torch.from_numpy(rows).to(self.dev), torch.from_numpy(src).to(self.dev)
            feat = vis[1:]
            keep += [rows_d, src_d, feat]
            opts.ds_rows, opts.ds_src, opts.n_ds = rows_d.data_ptr(), src_d.data_ptr(), int(rows.shape[0])
            opts.ds_feat, opts.n_deep, opts.ds_stride = feat.data_ptr(), int(feat.shape[0]), int(feat.stride(0))
        if prefix is not None:
            kc0, vc0, rpp = prefix
            if kc0.shape[3] < past or not kc0.is_contiguous() or not vc0.is_contiguous() or B % rpp or kc0.shape[1] != B // rpp:
                raise ValueError("prefix caches do not match the rows they serve")
            opts.kprefix, opts.vprefix = kc0.data_ptr(), vc0.data_ptr()
            opts.prefix_len, opts.prefix_cap, opts.rows_per_prefix = int(past), int(kc0.shape[3]), int(rpp)
        _lib.call("o3v_llm_prefill_ex", C.byref(self.w.llm), _ptr(x), _ptr(cos), _ptr(sin), _ptr(tiles), tiles.shape[0],
                  indexing.PREFILL_TILE, _ptr(kc), _ptr(vc), B, S, int(past), Tmax, C.byref(opts), _ptr(ws), nbytes, _stream())
        del keep
        return x

    def head(self, x_rows: torch.Tensor) -> torch.Tensor:
        """final norm + lm_head: bf16 [R,H] (row stride may exceed H) -> logits bf16 [R,V]."""
        R = x_rows.shape[0]
        H, V = self.cfg.text.hidden_size, self.cfg.text.vocab_size
        normed = torch.empty((R, H), dtype=torch.bfloat16, device=self.dev)
        logits = torch.empty((R, V), dtype=torch.bfloat16, device=self.dev)
        _lib.call("o3v_llm_head", C.byref(self.w.llm), _ptr(x_rows), x_rows.stride(0), R, _ptr(normed), _ptr(logits), _stream())
        return logits

    # ------------------------------------------------------------------------------------------ generate
    class _InLaunchWaitGaveUp(_lib.O3VError):
        pass

    @torch.no_grad()
    def generate(self, *args, **kw) -> "GenerateOutput":
        """`_generate` with one safety net: if an in-launch wait of the one-launch decode block gives up (its waiting workgroups were
        not all resident -- e.g. another process holds part of the GPU -- and the sticky time-out word is set), the SAME call is
        run again in this process on the stand-alone kernels (`fused_decode=False` for that call), logged once.  The word is read
        after the first chunk of steps and at the end, so a starved run is noticed after milliseconds, not after the completion."""
        try:
            return self._generate(*args, **kw)
        except O3VEngine._InLaunchWaitGaveUp as e:
            if not getattr(self, "_warned_fused_fallback", False):
                import logging
                logging.getLogger(__name__).warning("%s; re-running this generate call on the stand-alone decode kernels", e)
                self._warned_fused_fallback = True
            self.fused_fallbacks = getattr(self, "fused_fallbacks", 0) + 1
            return self._generate(*args, **kw, _fused_ok=False)

    @torch.no_grad()
    def _generate(self, input_ids, attention_mask=None, pixel_values=None, image_grid_thw=None, frames=None,
                 max_new_tokens=16, eos_token_ids: Sequence[int] = (), pad_token_id: Optional[int] = None,
                 repetition_penalty: float = 1.0, do_sample: bool = False, temperature: float = 1.0, top_p: float = 1.0,
                 top_k: int = 0, num_return_sequences: int = 1, seed: int = 0, row_ids: Optional[Sequence[int]] = None,
                 vis_embeds: Optional[torch.Tensor] = None, steps_per_sync: int = 16, return_margins: bool = True,
                 sync_timings: bool = False, prefix_key=None, pixel_values_videos=None, video_grid_thw=None, video_frames=None,
                 second_per_grid_ts=None, logprobs: int = 0, prompt_logprobs: int = 0, min_p: float = 0.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, min_new_tokens: int = 0, token_bias=None,
                 allowed_token_ids=None, banned_token_ids=None, stop_checker=None, shared_prefix_len: Optional[int] = None,
                 guide=None, _fused_ok: bool = True) -> GenerateOutput:
        """HF-semantics generate.  `num_return_sequences=G` shares ONE ViT pass and ONE prefill across the G
        completions of a prompt (the reference recomputes both G times, TF:1493-1579) and fans the KV cache out.

        `prefix_key` (hashable, single un-padded prompt only): identifies the visual content of the prompt.  The
        K/V of the prompt is kept under that key; a later call with the same key prefills only the tokens after
        the longest common token prefix (V-STAR asks 5 questions per video with the frame block first,
        R:eval/test/test_vstar_multi_images.py:205-206,511-544; self-consistency draws N samples of one prompt,
        R:eval/tts.py:47-123).  Causal attention makes the prefix K/V independent of what follows it.

        `logprobs=N` (0..20): per emitted token its log-prob, rank and the N most likely tokens under the processed distribution it
        was drawn from (GenerateOutput.logprobs; o3v_logprob_opts).  `prompt_logprobs=N`: the same for every prompt token after the
        first on the raw logits, from the prefill's hidden rows in chunks (GenerateOutput.prompt_logprobs).  A call asking for prompt
        log-probs does not reuse (or store) prefix K/V under `prefix_key`: reused rows have no hidden state to score.  With both 0
        nothing changes: no extra buffer, the same decode calls.

        Sampling controls beyond HF's (vLLM 0.7.2 SamplingParams, o3v_sampling_opts), all decided inside the
        sampler's own passes: `min_p` (sampling only; greedy ignores it), `presence_penalty` / `frequency_penalty` over the tokens
        the row has emitted, `token_bias` {id: float} added to the logits, `allowed_token_ids` / `banned_token_ids` as -inf masks,
        `min_new_tokens`: no id of `eos_token_ids` before that many tokens.  With all of them at their defaults the decode calls
        and buffers are the plain ones.  `stop_checker(ids)` is called at every chunk boundary (`steps_per_sync` steps) with the
        int64 CPU tensor [rows, done] of what has been emitted; it returns {row: n} (or (row, n) pairs): row ends after its first n
        tokens.  Such a row emits pad from the next step on, what it emitted past n is replaced by pad, and the trailing-pad trim
        counts it as finished at n.

        `shared_prefix_len=P` ("one video, several questions"; needs num_return_sequences == 1): the rows, given left-padded as
        usual, agree in their first P real tokens, every visual placeholder lies inside those, and the visual inputs are those of
        ONE row.  The prefix is prefilled once (looked up and stored under `prefix_key` like a single prompt), the rows' suffixes
        run behind it as one short prefill, and the rows decode as a group that reads the prefix K/V once per step; each row's own
        cache holds its suffix, left-padded to the longest, and its generated tokens (indexing.shared_prefix_layout, plan_decode's
        `suffix`).  A mismatch raises ValueError.  Shapes the group kernels do not serve (head_dim != 128, one row, more than 32
        own-key splits, prompt_logprobs, group_attention off) run as independent rows on the replicated visual inputs;
        timings["shared_prefix_rows"] tells which ran (rows in the group, 0 = independent rows).

        `guide` (guided.Guide; vLLM guided_decoding regex / choice): a token-level automaton on the device,
        i16 [n_states, ldn] with ldn >= vocabulary and ldn % 8 == 0.  Every row starts in `guide.start`; at each step the tokens
        whose entry in the row's state is negative are masked inside the sampler passes, in front of every other control, and the
        sampler's last stage moves the row to the entry of the token it emits -- no host round trip, no added launch, every decode
        regime.  The table is checked against the call's static bias first (guided.check_no_dead_end); `min_new_tokens` > 0 is
        refused with a guide (an accepting state whose only token is EOS would have none).  timings["guide_states"] holds the
        rows' states after the last step."""
        cfg, tc = self.cfg, self.cfg.text
        ids, mask, pad = prompt_arrays(input_ids, attention_mask)
        B0, S = ids.shape
        G = int(num_return_sequences)
        if B0 * G > self.MAX_ROWS:
            raise ValueError(f"at most {self.MAX_ROWS} sequences per engine call (two 16-column MFMA blocks in the decode linears); "
                             "shard larger batches")
        pad_id = cfg.pad_token_id if pad_token_id is None else int(pad_token_id)
        T = int(max_new_tokens)
        if T <= 0:
            raise ValueError(f"`max_new_tokens` must be greater than 0, but is {T}.")   # GenerationConfig.validate's rule
        n_lp, n_plp = int(logprobs or 0), int(prompt_logprobs or 0)
        for what, v in (("logprobs", n_lp), ("prompt_logprobs", n_plp)):
            if not 0 <= v <= _lib.MAX_LOGPROBS:
                raise ValueError(f"`{what}` must be in 0..{_lib.MAX_LOGPROBS}, got {v}")
        sampling = self._sampling_vectors(tc.vocab_size, T, eos_token_ids, bool(do_sample), min_p, presence_penalty, frequency_penalty,
                                          min_new_tokens, token_bias, allowed_token_ids, banned_token_ids)
        if guide is not None:
            self._check_guide(guide, tc.vocab_size, sampling, min_new_tokens)
        nsplit_env = os.environ.get("O3V_NSPLIT")      # A/B switch (tools/probes), read at every call
        if self.kv_cache_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_cache_dtype={self.kv_cache_dtype!r}: 'bf16' or 'fp8'")

        P = Lmax = 0    # shared prefix: its length and the longest suffix behind it; 0 = none, or it runs as independent rows
        if shared_prefix_len is not None:
            if G != 1:
                raise ValueError("shared_prefix_len needs num_return_sequences == 1")
            P, Lmax = int(shared_prefix_len), int(S - pad.min()) - int(shared_prefix_len)

        def make_plan(fused):
            if P:   # the B0 rows as one group behind one prefix of P tokens
                return plan_decode(tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim, 1, B0, P, T, self.group_attention,
                                   self.group_attention_mode, fused, int(nsplit_env) if nsplit_env else None, suffix=Lmax)
            return plan_decode(tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim, B0, G, S, T, self.group_attention,
                               self.group_attention_mode, fused, int(nsplit_env) if nsplit_env else None)

        plan = make_plan(self.fused_decode and _fused_ok)
        replicate = False
        if P and (n_plp or not plan.shared_prompt):     # shapes the group kernels do not serve: independent rows
            P, replicate = 0, True
            plan = make_plan(self.fused_decode and _fused_ok)
        # fp8 K/V (or, test hook, its arithmetic emulated on bf16 caches): the stand-alone attention kernels, so no hand-off buffer
        emulate = bool(getattr(self, "_debug_kv8_emulate", False)) and kv_cache_in_effect("fp8", tc.head_dim, plan) == "fp8"
        kv_dtype = "bf16" if emulate else kv_cache_in_effect(self.kv_cache_dtype, tc.head_dim, plan)
        if kv_dtype == "fp8" or emulate:
            plan = make_plan(False)
        # test hook: the rows decode through the ragged state (row_base = S for every row) -- the kernels of generate_continuous on
        # the inputs of an ordinary call, whose outputs they must reproduce bit for bit
        debug_ragged = bool(getattr(self, "_debug_ragged", False))
        if debug_ragged:
            if P or G != 1 or kv_dtype != "bf16" or emulate or pad.any() or n_lp or sampling or guide is not None or do_sample:
                raise ValueError("_debug_ragged: unpadded prompts of equal length, one greedy completion each, bf16 K/V, no extras")
            plan = make_plan(False)
        B = plan.B
        tm = {}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if sync_timings else None

        def mark(i):
            if ev is not None:
                ev[i].record()

        mark(0)
        # ---- vision (once per prompt batch): images (frames-as-images, R:…/grpo_trainer.py:540-548) and / or native videos
        # (pixel_values_videos + <|video_pad|>, R:…:555-564; R:eval/models/model_vllm.py:72-88)
        vis, grid, vgrid, n_img_rows = self._visual(pixel_values, image_grid_thw, frames, vis_embeds, pixel_values_videos, video_grid_thw,
                                                    video_frames)
        mark(1)
        lay = None
        if shared_prefix_len is not None:   # the rows' layout behind the prefix; checks them whichever way they run
            lay = indexing.shared_prefix_layout(ids, mask, int(shared_prefix_len), T, cfg.image_token_id, cfg.video_token_id, pad_id,
                                                **self._rope_kw(grid, vgrid, second_per_grid_ts))
            tm["shared_prefix_rows"] = B0 if P else 0
        if replicate:   # independent rows: every row gets the one row's visual tokens
            vis, grid, vgrid, n_img_rows, second_per_grid_ts = self._replicate_visual(vis, grid, vgrid, n_img_rows, second_per_grid_ts, B0)
        kv8, plp = None, None
        self._last_prompt = None
        if P:
            # ---- the prefix once, the suffixes behind it; every row's last suffix token gives its first logits
            x, kc, vc, kc0, vc0, past = self._prefill_shared_prefix(lay, vis, n_img_rows, plan, prefix_key)
            tm["prefix_tokens_reused"] = past
            logits = self.head(x.view(B0, Lmax, -1)[:, -1, :])      # [B0, V]
            mark(2)
            dpos, ids_rep = lay.decode_pos, ids
            state = dict(S=P, G=B0, pad_rep=np.zeros(B0, dtype=np.int64), own=(Lmax, lay.own_lo))
        else:
            # ---- positions + prefill (once per prompt); a call asking for prompt log-probs neither reuses nor stores prefix K/V
            pos, deltas = self._positions(ids, mask, grid, vgrid, second_per_grid_ts)
            x, kc, vc, kc0, vc0, past, kv8 = self._prefill_prompt(ids, pad, pos, vis, n_img_rows, G, plan, None if n_plp else prefix_key,
                                                                  kv_dtype == "fp8", emulate)
            tm["prefix_tokens_reused"] = past
            if self.reuse_prompt_kv and plan.shared_prompt and B0 == 1:
                key = self._prompt_key(ids, mask, pos, visual_identity(pixel_values, grid, frames, vis_embeds, pixel_values_videos, vgrid,
                                                                       video_frames))
                self._last_prompt = {"key": key, "kc0": kc0, "vc0": vc0, "x_last": x.view(B0, S - past, -1)[0, -1:, :].clone(),
                                     "deltas": np.array(deltas, copy=True)}
            plp = self._prompt_logprobs(x.view(B0, S, -1), ids, n_plp) if n_plp else None
            last = x.view(B0, S - past, -1)[:, -1, :]               # left padding: every row ends at S-1
            logits0 = self.head(last)                               # [B0, V]
            logits = logits0.repeat_interleave(G, dim=0).contiguous() if G > 1 else logits0
            mark(2)
            dpos = indexing.decode_positions(mask, deltas, T)       # [3,B0,T]
            if G > 1:
                dpos = np.repeat(dpos, G, axis=1)
            ids_rep = np.repeat(ids, G, axis=0) if G > 1 else ids
            state = dict(S=S, G=G, pad_rep=np.repeat(pad, G) if G > 1 else pad, own=None)
        # ---- decode state
        cosd, sind = self.mrope_table(dpos.reshape(3, B * T))
        knobs = dict(pad_id=pad_id, n_eos=len(eos_token_ids), do_sample=int(do_sample), rep_penalty=float(repetition_penalty),
                     temperature=float(temperature), top_p=float(top_p), seed=int(seed) & (2 ** 64 - 1), top_k=max(0, int(top_k or 0)))
        buf = _DecodeBuffers(self, plan, state["S"], T, state["G"], ids_rep, state["pad_rep"], eos_token_ids, row_ids, return_margins,
                             n_lp, sampling, knobs, cosd, sind, logits, kc, vc, kc0, vc0, kv8, emulate, own=state["own"], guide=guide,
                             ragged=[S] * B if debug_ragged else None)
        tm["kv_cache_dtype"] = kv_dtype
        tm["mlp_weights"] = mlp_weights_in_effect(self.w.t, plan)
        tm["kv_cache_bytes"] = int((kc.numel() + vc.numel() + (kc0.numel() + vc0.numel() if plan.shared_prompt else 0)) * 2 +
                                   sum(t.numel() * t.element_size() for t in kv8 or ()))
        use_eos = len(eos_token_ids) > 0
        done, ended = self._decode_loop(buf, T, use_eos, steps_per_sync, stop_checker)
        mark(3)
        stats = buf.host_stats
        layers_run = stats[0] * tc.num_hidden_layers
        tm["decode_forwards"] = int(stats[0])
        tm["launches_per_layer"] = (stats[1] / layers_run) if layers_run else None
        tm["fused_attention_layers"], tm["standalone_attention_layers"] = int(stats[2]), int(stats[3])
        buf.check_waits()
        if guide is not None:       # step `done` would read half done & 1
            tm["guide_states"] = buf.guide_state[done & 1].cpu().tolist()
        if getattr(self, "_debug_keep", False):     # probe hook: the decode's state after the last step
            self._debug_last = {"kc": kc, "vc": vc, "logits": logits, "x": buf.x, "S": state["S"], "cos": cosd, "sin": sind, "k_lo": buf.k_lo,
                                "nsplit": plan.nsplit, "Tmax": plan.Tmax, "out_ids": buf.out_ids,
                                **dict(zip(("k8", "v8", "k8s", "v8s"), kv8 or (None,) * 4))}
        gen = buf.out_ids[:, :done].to(torch.int64)
        if use_eos or ended:
            # HF stops at the step where every row has finished: trim trailing all-pad columns generated past it
            done = trimmed_length(gen.cpu().numpy(), eos_token_ids, ended, done)
            gen = gen[:, :done]
        seqs = torch.cat([torch.from_numpy(ids_rep).to(self.dev), gen], dim=1)
        if ev is not None:
            torch.cuda.synchronize()
            tm.update({"vit_ms": ev[0].elapsed_time(ev[1]), "prefill_ms": ev[1].elapsed_time(ev[2]),
                       "decode_ms": ev[2].elapsed_time(ev[3])})
        lp, margins = buf.lp, buf.margins
        if lp is not None:
            lp = Logprobs(lp.token[:, :done], lp.rank[:, :done], lp.top_ids[:, :done], lp.top[:, :done])
        return GenerateOutput(sequences=seqs, margins=None if margins is None else margins[:, :done], n_steps=done,
                              timings=tm, logprobs=lp, prompt_logprobs=plp)

    # ------------------------------------------------------------------------------------------ continuous batching
    @torch.no_grad()
    def generate_continuous(self, requests, rows: int, eos_token_ids: Sequence[int] = (), repetition_penalty: float = 1.0,
                            pad_token_id: Optional[int] = None, steps_per_sync: int = 16, session_columns: Optional[int] = None,
                            return_margins: bool = True, prefix_keys=None):
        """Greedy decoding of a list of requests over `rows` decode rows that are refilled in flight: a row whose request has ended
        takes the next request at the following chunk boundary instead of decoding pad tokens until the longest row of its batch
        ends ("Ragged rows").  -> one ContinuousOutput per request, in request order.

        A request is a ContinuousRequest (or a dict of its fields): 1-D `ids`, `max_new_tokens`, and its visual inputs as generate
        takes them precomputed (`vis_embeds`, `image_grid_thw`, `video_grid_thw`, `second_per_grid_ts`).  `prefix_keys`: None or one
        `prefix_key` per request (generate's prompt K/V reuse; every request is prefilled alone, so it applies to each).

        State: one set of decode buffers with B = rows; caches [layers][rows][Hkv][Tmax][D] with Tmax = max(len(ids) + max_new) +
        steps_per_sync (a row runs on to the end of the chunk in which it ends); ids, margins and the M-RoPE table hold
        `session_columns` columns (default: continuous.default_session_columns).  A request is admitted into a free row at a chunk
        boundary, column t0, if t0 + max_new <= session_columns: its prompt is prefilled alone, its K/V copied to slots [0, S) of the
        row, and row_base[row] = S - t0 tells the kernels where the row's context ends.  When the next request does not fit, the
        live rows drain and a new session starts at column 0 on the same buffers.  All of it is enqueued on the current stream.

        Rows never depend on one another: with rows, steps_per_sync and the weights fixed, a request's tokens and margins are the
        same bits whichever row it lands in and whenever it is admitted.  Sampling, log-probs, the extended controls, guides, stop
        strings, fp8 K/V and shared-prefix groups are indexed by the decode column or need per-row kernels of their own: they
        keep static batches (generate).  timings of the call: ContinuousOutput.timings (one dict, shared)."""
        cfg, tc = self.cfg, self.cfg.text
        rows = int(rows)
        if not 1 <= rows <= self.MAX_ROWS:
            raise ValueError(f"rows must be in 1..{self.MAX_ROWS}")
        reqs = [r if isinstance(r, ContinuousRequest) else ContinuousRequest(**r) for r in requests]
        if not reqs:
            return []
        keys = list(prefix_keys) if prefix_keys is not None else [None] * len(reqs)
        if len(keys) != len(reqs):
            raise ValueError("prefix_keys: one per request")
        if self.kv_cache_dtype != "bf16":
            raise ValueError("generate_continuous decodes on bf16 K/V (the fp8 K/V cache keeps static batches)")
        ids_all = [np.asarray(r.ids.cpu() if torch.is_tensor(r.ids) else r.ids, dtype=np.int64).reshape(-1) for r in reqs]
        if any(i.size == 0 for i in ids_all):
            raise ValueError("empty prompt")
        sync = max(1, int(steps_per_sync))
        max_new = [int(r.max_new_tokens) for r in reqs]
        columns = default_session_columns(max_new, sync) if session_columns is None else int(session_columns)
        sched = ContinuousScheduler([i.size for i in ids_all], max_new, rows, columns, sync, eos_token_ids)
        ctx_max = max(i.size + m for i, m in zip(ids_all, max_new))
        Tmax = ctx_max + sync
        # the context splits are a constant of the call (a request's bits depend on them): plan_decode's rule on the longest context
        nsplit_env = os.environ.get("O3V_NSPLIT")
        nsplit = int(nsplit_env) if nsplit_env else max(1, min(64, (ctx_max + 127) // 128, max(1, 640 // (rows * tc.num_key_value_heads))))
        plan = DecodePlan(rows, 0, False, Tmax, nsplit, 0, False)
        pad_id = cfg.pad_token_id if pad_token_id is None else int(pad_token_id)
        dev, V, D = self.dev, tc.vocab_size, tc.head_dim
        kc, vc = self.alloc_cache(rows, Tmax)
        cosd = torch.zeros((rows, columns, D), dtype=torch.bfloat16, device=dev)
        sind = torch.zeros_like(cosd)
        logits = torch.zeros((rows, V), dtype=torch.bfloat16, device=dev)
        knobs = dict(pad_id=pad_id, n_eos=len(eos_token_ids), do_sample=0, rep_penalty=float(repetition_penalty), temperature=1.0,
                     top_p=1.0, seed=0, top_k=0)
        buf = _DecodeBuffers(self, plan, 0, columns, 1, np.zeros((rows, 1), dtype=np.int64), np.zeros(rows, dtype=np.int64),
                             eos_token_ids, None, return_margins, 0, None, dict(knobs, rep_penalty=1.0), cosd, sind, logits, kc, vc,
                             None, None, ragged=[IDLE_BASE] * rows)
        buf.st.rep_penalty = float(repetition_penalty)
        buf.finished.fill_(1)
        self._last_prompt = None
        tm = {"prefix_tokens_reused": 0}
        out = [None] * len(reqs)

        def admit(a):
            r, b = reqs[a.request], a.row
            ids = ids_all[a.request][None]
            S, T = ids.shape[1], max_new[a.request]
            mask = np.ones_like(ids)
            vis, grid, vgrid, n_img_rows = self._visual(None, r.image_grid_thw, None, r.vis_embeds, None, r.video_grid_thw, None)
            pos, deltas = self._positions(ids, mask, grid, vgrid, r.second_per_grid_ts)
            x, k1, v1, _, _, past, _ = self._prefill_prompt(ids, np.zeros(1, dtype=np.int64), pos, vis, n_img_rows, 1,
                                                            DecodePlan(1, 0, False, S, 1, 0, False), keys[a.request])
            tm["prefix_tokens_reused"] += int(past)
            kc[:, b, :, :S].copy_(k1[:, 0])
            vc[:, b, :, :S].copy_(v1[:, 0])
            logits[b].copy_(self.head(x[-1:])[0])
            cos, sin = self.mrope_table(indexing.decode_positions(mask, deltas, T).reshape(3, T))
            cosd[b, a.t0:a.t0 + T].copy_(cos)
            sind[b, a.t0:a.t0 + T].copy_(sin)
            buf.seen[b].zero_()
            if repetition_penalty != 1.0:
                ids_dev = torch.from_numpy(ids.astype(np.int32)).to(dev)
                _lib.call("o3v_mark_seen", _ptr(ids_dev), _ptr(buf.seen[b]), 1, S, V, _stream())
            buf.finished[b] = 0
            buf.row_base[b] = a.row_base

        while not sched.done():
            for a in sched.admit():
                admit(a)
            c = sched.chunk()
            _lib.call("o3v_llm_decode_ex", C.byref(self.w.llm), C.byref(buf.st), None, None, c.step0, c.n_steps, int(c.skip_last_forward),
                      _stream())
            # the one device-to-host copy of the chunk: what its columns hold
            got = buf.out_ids[:, c.step0:c.step0 + c.n_steps].cpu().numpy()
            session = sched.sessions
            for r in sched.retire(got):
                buf.finished[r.row] = 1
                buf.row_base[r.row] = IDLE_BASE
                toks = torch.from_numpy(np.asarray(sched.row_toks[r.row][:r.n], dtype=np.int64))
                margins = buf.margins[r.row, r.t0:r.t0 + r.n].clone() if return_margins else None
                out[r.request] = ContinuousOutput(tokens=toks, margins=margins, row=r.row, t0=r.t0, session=session, timings=tm,
                                                  sequences=torch.cat([torch.from_numpy(ids_all[r.request]), toks])[None])
        stats = buf.host_stats
        layers_run = stats[0] * tc.num_hidden_layers
        tm.update(decode_forwards=int(stats[0]), rows_refilled=int(sched.rows_refilled), sessions=int(sched.sessions),
                  launches_per_layer=(stats[1] / layers_run) if layers_run else None,
                  kv_cache_bytes=int((kc.numel() + vc.numel()) * 2), standalone_attention_layers=int(stats[3]), nsplit=nsplit,
                  session_columns=columns, Tmax=Tmax)
        return out

    def _rope_kw(self, grid, vgrid, second_per_grid_ts):
        """indexing.rope_index's keywords for this model (as _positions passes them)."""
        cfg = self.cfg
        return dict(image_grid_thw=grid, merge=cfg.vision.spatial_merge_size, video_grid_thw=vgrid,
                    second_per_grid_ts=second_per_grid_ts, tokens_per_second=cfg.vision.tokens_per_second,
                    split_video_frames=self.q3, mode="tf5" if self.q3 else self.position_mode)

    @staticmethod
    def _replicate_visual(vis, grid, vgrid, n_img_rows, second_per_grid_ts, B):
        """One row's visual tokens for B rows that all hold its placeholders: [image tokens ; video tokens] -> [B x image ; B x video]
        (the order embed_source_rows consumes), grids and seconds-per-grid repeated alike."""
        if vis is None:
            return vis, grid, vgrid, n_img_rows, second_per_grid_ts
        n_img = vis.shape[-2] if n_img_rows is None else int(n_img_rows)
        vis = torch.cat([vis[..., :n_img, :]] * B + [vis[..., n_img:, :]] * B, dim=-2)
        tile = lambda g: None if g is None else np.tile(np.asarray(g).reshape(-1, 3), (B, 1))
        spg = second_per_grid_ts
        if spg is not None:
            spg = np.tile(np.asarray(spg.cpu() if torch.is_tensor(spg) else spg, dtype=np.float64).reshape(-1), B)
        return vis, tile(grid), tile(vgrid), None if n_img_rows is None else n_img * B, spg

    def _prefill_shared_prefix(self, lay, vis, n_img_rows, plan: DecodePlan, prefix_key):
        """The prompt stage of generate(shared_prefix_len=P): the prefix as ONE un-padded row through the route of _prefill_prompt
        (looked up and stored under `prefix_key`; Qwen3-VL DeepStack rows all lie in it), then the B suffixes, left-padded to Lmax,
        behind it into the rows' own caches.
        -> (x: last-layer rows of the suffixes [B * Lmax, H], kc, vc [layers, B, Hkv, plan.Tmax, D], kc0, vc0: the prefix entry,
        past: prefix tokens reused).  A stored entry that covers the whole prefix is used where it lies: nothing here writes it."""
        pids = lay.prefix_ids
        P = pids.shape[1]
        B, Lmax = lay.suffix_ids.shape
        past, ent = 0, self._prefix.get(prefix_key) if prefix_key is not None else None
        if ent is not None:
            n = min(len(ent["ids"]), P)
            neq = np.flatnonzero(ent["ids"][:n] != pids[0, :n])
            past = int(neq[0]) if neq.size else int(n)
        if past == P:
            kc0, vc0 = ent["k"], ent["v"]
        else:
            kc0, vc0 = self.alloc_cache(1, P)
            if past:
                kc0[:, :, :, :past].copy_(ent["k"][:, :, :, :past])
                vc0[:, :, :, :past].copy_(ent["v"][:, :, :, :past])
            x0 = self.embed(pids, vis, first=past, n_image_rows=n_img_rows)
            self.prefill(x0, lay.prefix_pos[:, :, past:], [0], 1, P - past, kc0, vc0, past=past,
                         deepstack=(pids, vis) if self.q3 else None)
            if prefix_key is not None:
                self._prefix_store(prefix_key, pids[0], kc0, vc0)
        kc, vc = self.alloc_cache(B, plan.Tmax)
        x = self.embed(lay.suffix_ids, None)
        self.prefill(x, lay.suffix_pos, np.zeros(B, dtype=np.int64), B, Lmax, kc, vc, past=P, prefix=(kc0, vc0, B), own_lo=lay.own_lo)
        return x, kc, vc, kc0, vc0, past

    def _prefill_prompt(self, ids, pad, pos, vis, n_img_rows, G, plan: DecodePlan, prefix_key, kv8: bool = False,
                        kv8_emulate: bool = False):
        """The prompt stage of generate: the caches, the tokens whose K/V are kept under `prefix_key` (single un-padded prompt)
        copied in, the prefill of the rest, the fan-out to the G rows of each prompt, the prefix store.
        -> (x: last-layer rows of the tokens run [B0 * (S - past), H], kc, vc: the decode caches, kc0, vc0: the prompt's K/V kept
        once (None unless plan.shared_prompt), past: tokens reused, kv8: None or the fp8 caches (k8, v8, k8s, v8s)).
        kv8 (never with plan.shared_prompt): the prompt is prefilled in bf16 into an entry of S slots -- prefill attention itself
        runs on unquantised K/V -- and quantised from there into fp8 caches of plan.Tmax slots; the entry is released (the
        `prefix_key` store keeps its bf16 copy) and kc / vc are the staging rows of the new token [B, Hkv, 1, D].
        kv8_emulate (test hook): bf16 caches whose prompt slots are replaced by dequant(quant(row))."""
        B0, S = ids.shape
        if kv8:
            return self._prefill_prompt_kv8(ids, pad, pos, vis, n_img_rows, G, plan, prefix_key)
        kc, vc = self.alloc_cache(plan.B, plan.Tmax)
        kc0 = vc0 = None
        past = 0
        use_prefix = prefix_key is not None and B0 == 1 and int(pad[0]) == 0
        if use_prefix:
            past = self._prefix_lookup(prefix_key, ids[0])
        x = self.embed(ids, vis, first=past, n_image_rows=n_img_rows)
        ds = (ids, vis) if self.q3 else None
        if G == 1 and not use_prefix:
            self.prefill(x, pos, pad, B0, S, kc, vc, deepstack=ds)
        else:
            kc0, vc0 = self.alloc_cache(B0, S)
            if past:
                ent = self._prefix[prefix_key]
                kc0[:, :, :, :past].copy_(ent["k"][:, :, :, :past])
                vc0[:, :, :, :past].copy_(ent["v"][:, :, :, :past])
            self.prefill(x, pos[:, :, past:], pad, B0, S - past, kc0, vc0, past=past, deepstack=ds)
            if not plan.shared_prompt:
                # KV fan-out: completion g of prompt b is row b*G+g (repeat_interleave order, R:grpo_trainer.py:586)
                # (a broadcast copy into the [layers, B0, G, ...] view of the caches: no G-times temporary)
                shp = (kc.shape[0], B0, G) + tuple(kc.shape[2:])
                kc.view(shp)[:, :, :, :, :S].copy_(kc0[:, :, None])
                vc.view(shp)[:, :, :, :, :S].copy_(vc0[:, :, None])
            if use_prefix:
                self._prefix_store(prefix_key, ids[0], kc0, vc0)
            if not plan.shared_prompt:
                kc0 = vc0 = None
        if kv8_emulate:
            _lib.call("o3v_kv8_roundtrip", _ptr(kc), _ptr(vc), kc.shape[0] * kc.shape[1] * kc.shape[2], plan.Tmax, 0, S, kc.shape[4],
                      _stream())
        return x, kc, vc, kc0, vc0, past, None

    def _prefill_prompt_kv8(self, ids, pad, pos, vis, n_img_rows, G, plan: DecodePlan, prefix_key):
        tc = self.cfg.text
        B0, S = ids.shape
        L, Hkv, D = tc.num_hidden_layers, tc.num_key_value_heads, tc.head_dim
        past = 0
        use_prefix = prefix_key is not None and B0 == 1 and int(pad[0]) == 0
        if use_prefix:
            past = self._prefix_lookup(prefix_key, ids[0])
        x = self.embed(ids, vis, first=past, n_image_rows=n_img_rows)
        kc0, vc0 = self.alloc_cache(B0, S)
        if past:
            ent = self._prefix[prefix_key]
            kc0[:, :, :, :past].copy_(ent["k"][:, :, :, :past])
            vc0[:, :, :, :past].copy_(ent["v"][:, :, :, :past])
        self.prefill(x, pos[:, :, past:], pad, B0, S - past, kc0, vc0, past=past, deepstack=(ids, vis) if self.q3 else None)
        if use_prefix:
            self._prefix_store(prefix_key, ids[0], kc0, vc0)

        def caches(rows, slots):
            return tuple(torch.empty((L, rows, Hkv, slots) + tail, dtype=dt, device=self.dev)
                         for tail, dt in (((D,), torch.uint8), ((D,), torch.uint8), ((), torch.float32), ((), torch.float32)))

        def quantize(dst, slots):
            _lib.call("o3v_kv8_quantize", _ptr(kc0), _ptr(vc0), *(_ptr(t) for t in dst), L * B0 * Hkv, S, slots, D, _stream())

        kv8 = caches(plan.B, plan.Tmax)
        if G == 1:
            quantize(kv8, plan.Tmax)
        else:
            # KV fan-out of the quantised prompt: completion g of prompt b is row b*G+g (the broadcast copy of the bf16 path)
            once = caches(B0, S)
            quantize(once, S)
            for dst, src in zip(kv8, once):
                dst.view((L, B0, G) + tuple(dst.shape[2:]))[:, :, :, :, :S].copy_(src[:, :, None])
        kc, vc = (torch.empty((plan.B, Hkv, 1, D), dtype=torch.bfloat16, device=self.dev) for _ in range(2))
        return x, kc, vc, None, None, past, kv8

    def _decode_loop(self, buf: "_DecodeBuffers", T: int, use_eos: bool, steps_per_sync: int, stop_checker):
        """Chunks of decode steps enqueued from C++, one host check per chunk (TF:utils.py:2936-2937) -> (steps done, ended: rows
        the stop checker ended -> number of tokens they keep)."""
        B, pad_id = buf.st.B, buf.st.pad_id
        lp_opts, so, go = (None if o is None else C.byref(o) for o in (buf.lp_opts, buf.so, buf.go))
        done = 0
        chunk = max(1, int(steps_per_sync)) if (use_eos or stop_checker is not None) else T
        ended = {}
        while done < T:
            # the first chunk is short whenever the one-launch block is in use: its time-out word is read right after it
            n = min(chunk if (done or buf.sync is None) else min(chunk, getattr(self, "_first_chunk", 16)), T - done)
            if go is None:
                _lib.call("o3v_llm_decode_ex", C.byref(self.w.llm), C.byref(buf.st), lp_opts, so, done, n, int(done + n == T), _stream())
            else:
                _lib.call("o3v_llm_decode_guided", C.byref(self.w.llm), C.byref(buf.st), lp_opts, so, go, done, n, int(done + n == T),
                          _stream())
            first = done == 0
            done += n
            if first and done < T:
                buf.check_waits()
            if stop_checker is not None:
                hits = stop_checker(buf.out_ids[:, :done].to(torch.int64).cpu())
                for b, end in (hits.items() if hasattr(hits, "items") else (hits or ())):
                    b, end = int(b), int(end)
                    if not (0 <= b < B and 0 <= end <= done):
                        raise ValueError(f"stop_checker: row {b} / end {end} outside [0, {B}) x [0, {done}]")
                    if b not in ended:
                        ended[b] = end
                        buf.finished[b] = 1
                        buf.out_ids[b, end:] = pad_id
            if (use_eos or ended) and done < T and bool(buf.finished.all().item()):
                break
        return done, ended

    def _check_guide(self, guide, V: int, sampling, min_new_tokens):
        """generate(guide=...): the table's shape and device, min_new_tokens, and no dead end under the call's static bias."""
        t = guide.table
        if not (torch.is_tensor(t) and t.dtype == torch.int16 and t.dim() == 2 and t.is_contiguous() and t.is_cuda):
            raise ValueError("guide.table must be a contiguous int16 tensor [n_states, ldn] on the engine's device")
        n, ldn = int(t.shape[0]), int(t.shape[1])
        if (n, ldn) != (int(guide.n_states), int(guide.ldn)) or ldn < V or ldn % 8 or not 0 <= int(guide.start) < n:
            raise ValueError(f"guide: table {tuple(t.shape)} against n_states={guide.n_states}, ldn={guide.ldn} (>= {V}, a multiple of 8), "
                             f"start={guide.start}")
        if int(min_new_tokens or 0) > 0:
            raise ValueError("a guide cannot be combined with min_new_tokens > 0: an accepting state with only EOS left would have no token")
        host = guide.host_table if guide.host_table is not None else t.cpu().numpy()
        guided.check_no_dead_end(host[:, :V], None if sampling is None else sampling["bias"], int(guide.start))

    @staticmethod
    def _sampling_vectors(V: int, T: int, eos_token_ids, do_sample: bool, min_p, presence_penalty, frequency_penalty,
                          min_new_tokens, token_bias, allowed_token_ids, banned_token_ids):
        """Host side of o3v_sampling_opts: None when every control is at its default (the plain decode calls then), else the
        scalars and the two dense f32 [V] vectors of static edits -- `bias` (token_bias, -inf outside the allowed set and at banned
        ids; None when there is no edit) and `bias_early` (the same with every EOS id at -inf, for the steps before
        min_new_tokens).  Pure numpy: no GPU needed."""
        min_p, pres, freq, min_new = float(min_p or 0.0), float(presence_penalty or 0.0), float(frequency_penalty or 0.0), \
            int(min_new_tokens or 0)
        if not 0.0 <= min_p <= 1.0:
            raise ValueError(f"`min_p` must be in [0, 1], got {min_p}")
        for what, v in (("presence_penalty", pres), ("frequency_penalty", freq)):
            if not -2.0 <= v <= 2.0:
                raise ValueError(f"`{what}` must be in [-2, 2], got {v}")
        if min_new < 0:
            raise ValueError(f"`min_new_tokens` must be >= 0, got {min_new}")
        if not do_sample:
            min_p = 0.0      # greedy ignores top_k / top_p / min_p
        eos = [int(e) for e in eos_token_ids]
        if not eos or min_new == 0:
            min_new = 0      # nothing to hold back
        static = bool(token_bias) or allowed_token_ids is not None or bool(banned_token_ids is not None and len(banned_token_ids))
        if not (min_p or pres or freq or min_new or static):
            return None
        bias = None
        if static:
            bias = np.zeros(V, dtype=np.float32)
            for t, v in dict(token_bias or {}).items():
                if not 0 <= int(t) < V or not np.isfinite(float(v)):
                    raise ValueError(f"token_bias: token id {t} outside the vocabulary or bias {v} not finite")
                bias[int(t)] += np.float32(v)
            if allowed_token_ids is not None:
                allowed = np.asarray(list(allowed_token_ids), dtype=np.int64).reshape(-1)
                if allowed.size == 0 or allowed.min() < 0 or allowed.max() >= V:
                    raise ValueError("allowed_token_ids must be a non-empty list of ids inside the vocabulary")
                outside = np.ones(V, dtype=bool)
                outside[allowed] = False
                bias[outside] = -np.inf
            if banned_token_ids is not None and len(banned_token_ids):
                banned = np.asarray(list(banned_token_ids), dtype=np.int64).reshape(-1)
                if banned.min() < 0 or banned.max() >= V:
                    raise ValueError("banned_token_ids must lie inside the vocabulary")
                bias[banned] = -np.inf
            if not np.isfinite(bias).any():
                raise ValueError("allowed_token_ids minus the banned tokens is empty: no token could be emitted")
        early = None
        if min_new:
            early = np.zeros(V, dtype=np.float32) if bias is None else bias.copy()
            early[[e for e in eos if 0 <= e < V]] = -np.inf
            if not np.isfinite(early).any():
                raise ValueError("every allowed token is a stop id while min_new_tokens > 0: no token could be emitted")
        counts = bool(pres or freq)
        if counts and T > _lib.MAX_COUNT:
            raise ValueError(f"presence / frequency penalties count emitted tokens in 16 bits: max_new_tokens <= {_lib.MAX_COUNT}")
        return {"min_p": min_p, "presence": pres, "frequency": freq, "min_tokens": min_new, "bias": bias, "bias_early": early,
                "counts": counts}

    def _prompt_logprobs(self, xs: torch.Tensor, ids: np.ndarray, n: int, rows_per_chunk: int = 2048) -> Logprobs:
        """Prompt log-probs from the prefill's hidden rows xs [B0, S, H]: row j of prompt b predicts ids[b, j+1].  The head runs on
        `rows_per_chunk` rows at a time (as completion_logps does); no [S, vocab] tensor is ever held."""
        B0, S, H = xs.shape
        V = self.cfg.text.vocab_size
        out = Logprobs.zeros(B0, S - 1, n, self.dev)
        if S < 2:
            return out
        tgt = torch.from_numpy(np.ascontiguousarray(ids[:, 1:].astype(np.int32))).to(self.dev)
        step = max(16, int(rows_per_chunk))
        scratch = torch.empty((min(step, S - 1), _lib.LOGPROB_ROW_SCRATCH_FLOATS), dtype=torch.float32, device=self.dev)
        for b in range(B0):
            for r0 in range(0, S - 1, step):
                r1 = min(S - 1, r0 + step)
                lg = self.head(xs[b, r0:r1])
                _lib.call("o3v_logprobs_rows", _ptr(lg), _ptr(tgt[b, r0:r1]), r1 - r0, V, V, n, _ptr(out.token[b, r0:r1]),
                          _ptr(out.rank[b, r0:r1]), _ptr(out.top_ids[b, r0:r1]), _ptr(out.top[b, r0:r1]), _ptr(scratch), _stream())
                del lg
        return out

    # ------------------------------------------------------------------------------------------ prefix K/V
    PREFIX_ENTRIES = 2   # videos whose prompt K/V stay resident (7B, S=4.5k: 0.26 GB each; 288 GB HBM is not the limit)

    def _prefix_lookup(self, key, ids_row: np.ndarray) -> int:
        """Tokens of `ids_row` whose K/V are cached under `key`: the longest common prefix, capped at S-1 so the
        last prompt token is always run (its hidden state feeds the first logits)."""
        ent = self._prefix.get(key)
        if ent is None:
            return 0
        old = ent["ids"]
        n = min(len(old), len(ids_row) - 1)
        neq = np.flatnonzero(old[:n] != ids_row[:n])
        return int(neq[0]) if neq.size else int(n)

    def _prefix_store(self, key, ids_row: np.ndarray, kc0, vc0):
        self._prefix.pop(key, None)
        while len(self._prefix) >= self.PREFIX_ENTRIES:
            self._prefix.pop(next(iter(self._prefix)))
        self._prefix[key] = {"ids": np.array(ids_row, copy=True), "k": kc0, "v": vc0}

    def drop_prefix_cache(self):
        self._prefix = {}

    def drop_prompt_handover(self):
        """Release the generate -> completion_logps hand-over (the prompt's K/V and x_last).  It otherwise lives until the next
        generate; load_weights drops it because it was computed with the old weights."""
        self._last_prompt = None

    # ------------------------------------------------------------------------------------------ weight update
    def load_weights(self, named_tensors) -> set:
        """New policy weights in place (vLLM's model.load_weights; the trainer calls it after each optimizer step): the packed
        images are rewritten on the device by o3v_repack_rows (DeviceWeights.load_weights: same bytes as a fresh load, same data
        pointers, enqueued on the current stream), then every cache derived from the weights is dropped.  Returns the canonical
        names written."""
        try:
            return self.w.load_weights(named_tensors)
        finally:
            # also when a launch fails part-way: some slots may already hold the new bytes, so nothing derived from the old
            # weights may be served again (the position table is dropped whether or not pos_embed was among the names)
            self.weights_version += 1
            self.drop_prefix_cache()
            self.drop_prompt_handover()
            if self.q3:
                self._vit_plan_cache.clear()   # the resampled position table lives in the plan

    # ------------------------------------------------------------------------------------------ LoRA adapter
    def _adapter_state_changed(self):
        """Nothing computed under one adapter state may be served under another: the same invalidation as load_weights."""
        self.weights_version += 1
        self.drop_prefix_cache()
        self.drop_prompt_handover()
        if self.q3:
            self._vit_plan_cache.clear()

    def load_adapter(self, named_tensors, scale=None, lora_alpha=None, use_rslora=False) -> set:
        """A peft LoRA adapter merged on the device next to the base weights (DeviceWeights.load_adapter) and switched on.  Decoding
        with it costs what decoding without it costs; `with engine.adapter_disabled():` runs the base (the reference log-probs of
        R:grpo_trainer.py:624-630).  A later call with the same targets rewrites the adapter images in place: the per-step push of
        a LoRA trainer moves A and B only."""
        try:
            return self.w.load_adapter(named_tensors, scale=scale, lora_alpha=lora_alpha, use_rslora=use_rslora)
        finally:
            self._adapter_state_changed()

    def unload_adapter(self):
        try:
            self.w.unload_adapter()
        finally:
            self._adapter_state_changed()

    def set_adapter_enabled(self, flag: bool):
        if bool(flag) != self.w.adapter_enabled:
            try:
                self.w.set_adapter_enabled(flag)
            finally:
                self._adapter_state_changed()

    @property
    def adapter_loaded(self) -> bool:
        return self.w.adapter_loaded

    @property
    def adapter_enabled(self) -> bool:
        return self.w.adapter_enabled

    @contextlib.contextmanager
    def adapter_disabled(self):
        """peft's disable_adapter(): the base weights inside the block, the previous state after it (also on an exception)."""
        was = self.w.adapter_enabled
        self.set_adapter_enabled(False)
        try:
            yield self
        finally:
            if was and self.w.adapter_loaded:
                self.set_adapter_enabled(True)

    # ------------------------------------------------------------------------------------------ logits / logps
    @torch.no_grad()
    def forward_logits(self, input_ids, attention_mask=None, pixel_values=None, image_grid_thw=None, frames=None,
                       vis_embeds=None, pixel_values_videos=None, video_grid_thw=None, video_frames=None,
                       second_per_grid_ts=None) -> torch.Tensor:
        """model(input_ids, ...).logits bf16 [B,L,V] (R:grpo_trainer.py:375)."""
        ids, mask, pad = prompt_arrays(input_ids, attention_mask, check_left_padding=False)
        B, S = ids.shape
        vis, grid, vgrid, n_img_rows = self._visual(pixel_values, image_grid_thw, frames, vis_embeds, pixel_values_videos, video_grid_thw,
                                                    video_frames)
        pos, _ = self._positions(ids, mask, grid, vgrid, second_per_grid_ts)
        kc, vc = self.alloc_cache(B, S)
        x = self.embed(ids, vis, n_image_rows=n_img_rows)
        self.prefill(x, pos, pad, B, S, kc, vc, deepstack=(ids, vis) if self.q3 else None)
        return self.head(x).view(B, S, -1)

    @torch.no_grad()
    def completion_logps(self, prompt_ids, completion_ids, attention_mask=None, pixel_values=None, image_grid_thw=None,
                         frames=None, vis_embeds=None, rows_per_chunk: int = 2048, pixel_values_videos=None, video_grid_thw=None,
                         video_frames=None, second_per_grid_ts=None) -> torch.Tensor:
        """log p(completion token | everything before it) for the G completions of ONE prompt -> f32 [G, T].

        What R:grpo_trainer.py:371-384 + :612-613 compute (`_get_per_token_logps(model, prompt_completion_ids, ...)
        [:, prompt_length-1:]`) for the policy and for the reference model, restructured around what the G rows share:
        the ViT runs once (the reference re-encodes the frames per row), the prompt is prefilled once and its K/V fanned
        out, the G x T completion tokens run as one pass behind that prefix, and the lm_head + log-softmax touch only the
        G x T positions that are kept, `rows_per_chunk` rows of logits at a time (the reference materialises
        [G, S+T, vocab]: 12.8 GB at G=8, S+T=5.2k)."""
        tc = self.cfg.text
        comp = torch.as_tensor(completion_ids).to(torch.int64)
        if comp.dim() != 2:
            raise ValueError("completion_ids must be [G, T]")
        G, T = comp.shape
        ids, mask, pad = prompt_arrays(prompt_ids, attention_mask)      # ONE prompt: [S] or [1, S]
        S = ids.shape[1]
        H = tc.hidden_size
        out = torch.empty((G, T), dtype=torch.float32, device=self.dev)
        if T == 0 or G == 0:
            return out
        as_np = lambda g: None if g is None else np.asarray(g.cpu() if torch.is_tensor(g) else g, dtype=np.int64).reshape(-1, 3)
        grid, vgrid = as_np(image_grid_thw), as_np(video_grid_thw)
        if frames is not None:
            grid = self.frames_grid(frames)
        if video_frames is not None:
            vgrid = None      # derived from the frames by the tower's front end: no hand-over for this input form
        memo, self.timings_last_logps = self._last_prompt, {"prompt_kv_reused": False}
        pos = deltas = None
        if memo is not None and (video_frames is None):
            pos, deltas = self._positions(ids, mask, grid, vgrid, second_per_grid_ts)
            key = self._prompt_key(ids, mask, pos, visual_identity(pixel_values, grid, frames, vis_embeds, pixel_values_videos, vgrid,
                                                                   video_frames))
            if key != memo["key"]:
                memo = None
        else:
            memo = None
        if memo is not None:
            # the prompt generate has just prefilled: same bytes in, same kernels -> the K/V and the last hidden row it kept
            kc0, vc0, x_last, deltas = memo["kc0"], memo["vc0"], memo["x_last"], memo["deltas"]
            self.timings_last_logps["prompt_kv_reused"] = True
        else:
            vis, grid, vgrid, n_img_rows = self._visual(pixel_values, image_grid_thw, frames, vis_embeds, pixel_values_videos,
                                                        video_grid_thw, video_frames)
            pos, deltas = self._positions(ids, mask, grid, vgrid, second_per_grid_ts)
            # prompt once
            kc0, vc0 = self.alloc_cache(1, S)
            x = self.embed(ids, vis, n_image_rows=n_img_rows)
            self.prefill(x, pos, pad, 1, S, kc0, vc0, deepstack=(ids, vis) if self.q3 else None)
            x_last = x[S - 1:S].clone()                               # hidden state that predicts completion token 0
            del x
        rows = torch.empty((G, T, H), dtype=torch.bfloat16, device=self.dev)
        rows[:, 0] = x_last
        if T > 1:
            # the first T-1 completion tokens of every row behind the shared prompt K/V
            # (their caches hold only their own T-1 tokens; the prompt's K/V is read from kc0 / vc0, kept once)
            kc, vc = self.alloc_cache(G, T - 1)
            ctok = comp[:, :T - 1].to(self.dev, torch.int32).contiguous().view(-1)
            xc = torch.empty((G * (T - 1), H), dtype=torch.bfloat16, device=self.dev)
            _lib.call("o3v_embed_tokens", _ptr(self.w.t["l.embed"]), _ptr(ctok), _ptr(xc), G * (T - 1), H, _stream())
            dpos = np.repeat(indexing.decode_positions(mask, deltas, T - 1), G, axis=1)      # [3, G, T-1]
            self.prefill(xc, dpos, np.repeat(pad, G), G, T - 1, kc, vc, past=S, prefix=(kc0, vc0, G))
            rows[:, 1:] = xc.view(G, T - 1, H)
            del kc, vc, xc
        del kc0, vc0
        flat = rows.view(G * T, H)
        tgt = comp.to(self.dev, torch.int32).contiguous().view(-1)
        V = tc.vocab_size
        of = out.view(-1)
        step = max(16, int(rows_per_chunk))
        for r0 in range(0, G * T, step):
            r1 = min(G * T, r0 + step)
            lg = self.head(flat[r0:r1])
            _lib.call("o3v_logprob_gather", _ptr(lg), _ptr(tgt[r0:r1]), _ptr(of[r0:r1]), r1 - r0, V, V, _stream())
            del lg
        return out

    @torch.no_grad()
    def per_token_logps(self, logits: torch.Tensor, input_ids) -> torch.Tensor:
        """R:grpo_trainer.py:371-384: log_softmax(logits[:, :-1]) gathered at input_ids[:, 1:] -> f32 [B, L-1]."""
        B, L, V = logits.shape
        ids = torch.as_tensor(input_ids).to(self.dev)
        tgt = ids[:, 1:].to(torch.int32).contiguous().view(-1)
        lg = logits[:, :-1, :].contiguous().view(-1, V)
        out = torch.empty(lg.shape[0], dtype=torch.float32, device=self.dev)
        _lib.call("o3v_logprob_gather", _ptr(lg), _ptr(tgt), _ptr(out), lg.shape[0], V, V, _stream())
        return out.view(B, L - 1)
