"""vLLM-style facade (facade 2): `LLM(...).generate(inputs, sampling_params)` as
R:eval/inference_example.py:15-29,75-82 and R:eval/models/model_vllm.py:18-33,103,117,125 call it.

    llm = LLM(model=path, tensor_parallel_size=1, max_model_len=81920, gpu_memory_utilization=0.7,
              limit_mm_per_prompt={"image": 32})
    out = llm.generate([{"prompt": text, "multi_modal_data": {"image": frames}}], sampling_params=SamplingParams(...))
    out[0].outputs[0].text

The engine tokenises `prompt` itself, expands each <|image_pad|> to gh*gw/4 placeholders
(TF:models/qwen2_5_vl/processing_qwen2_5_vl.py:59-62) and runs the fused GPU frame pipeline on the images
(list of PIL images, a [T,3,H,W] tensor / ndarray as process_vision_info returns it, or a single image).
`multi_modal_data["video"]` (what QwenVL_VLLM.__call__ sends, R:eval/models/model_vllm.py:72-88,99-103: the [T,3,H,W] array of
process_vision_info under a <|vision_start|><|video_pad|><|vision_end|> prompt) is the native video input: temporal patches of two
frames, one <|video_pad|> expanded to T/2*gh*gw/4 placeholders, rope time advancing per temporal patch.
temperature == 0 -> greedy; otherwise temperature / top-p sampling with repetition penalty over prompt + output.
`SamplingParams(logprobs=N, prompt_logprobs=N)` return vLLM's per-token {token_id: Logprob} dicts (V0 sampler semantics: the
processed distribution each token was drawn from).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Any, List, Optional, Sequence

import numpy as np
import torch

from . import guided
from . import vision_process as vp
from .config import O3VConfig
from .engine import O3VEngine
from .weights import DeviceWeights, getter_from_safetensors_dir

MAX_LOGPROBS = 20   # vLLM's default max_logprobs (the kernels' O3V_MAX_LOGPROBS)


@dataclass
class GuidedDecodingParams:
    """vLLM 0.7.2's GuidedDecodingParams.  Built: `regex` and `choice` (exactly one; the subset and semantics of
    open_o3_video_amd.guided).  `json`, `grammar` and `json_object` are refused by name; `backend` and
    `whitespace_pattern` are accepted and ignored (there is one backend, and no JSON guide to put whitespace into)."""
    regex: Optional[str] = None
    choice: Optional[Sequence[str]] = None
    json: Any = None
    grammar: Any = None
    json_object: Any = None
    backend: Optional[str] = None
    whitespace_pattern: Optional[str] = None

    def __post_init__(self):
        for name in ("json", "grammar", "json_object"):
            if getattr(self, name) is not None:
                raise ValueError(f"SamplingParams.guided_decoding: {name} guides are not supported (regex and choice are)")
        if (self.regex is None) == (self.choice is None):
            raise ValueError("SamplingParams.guided_decoding needs exactly one of regex / choice")
        if self.regex is not None and (not isinstance(self.regex, str) or not self.regex):
            raise ValueError("SamplingParams.guided_decoding: regex must be a non-empty string")
        if self.choice is not None:
            self.choice = list(self.choice) if not isinstance(self.choice, str) else self.choice
            guided.choice_regex(self.choice)    # a non-empty list of non-empty strings

    @property
    def pattern(self) -> str:
        return self.regex if self.regex is not None else guided.choice_regex(self.choice)


@dataclass
class SamplingParams:
    temperature: float = 1.0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    max_tokens: int = 16
    stop_token_ids: Optional[Sequence[int]] = None
    n: int = 1
    seed: Optional[int] = None
    logprobs: Optional[int] = None          # per output token: its log-prob + the N most likely (0: the token's only)
    prompt_logprobs: Optional[int] = None   # the same for every prompt token after the first
    # the rest of vLLM 0.7.2's sampling controls (defaults and checks of SamplingParams._verify_args; semantics: INTEGRATION.md a14)
    top_k: int = -1                         # -1: off
    min_p: float = 0.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    min_tokens: int = 0
    stop: Any = None                        # str or list of str
    include_stop_str_in_output: bool = False
    ignore_eos: bool = False
    skip_special_tokens: bool = True
    logit_bias: Optional[dict] = None       # {token id: bias}
    allowed_token_ids: Optional[Sequence[int]] = None
    bad_words: Optional[Sequence[str]] = None
    guided_decoding: Any = None             # GuidedDecodingParams or a dict of its keys: regex / choice
    # vLLM arguments that are not built: anything but None is refused by name
    best_of: Any = None
    logits_processors: Any = None
    truncate_prompt_tokens: Any = None

    def __post_init__(self):
        for name in ("logprobs", "prompt_logprobs"):
            v = getattr(self, name)
            if v is not None and not 0 <= int(v) <= MAX_LOGPROBS:
                raise ValueError(f"Requested {name} of {v}, which is outside the allowed range 0..{MAX_LOGPROBS}")
        for name in ("best_of", "logits_processors", "truncate_prompt_tokens"):
            if getattr(self, name) is not None:
                raise ValueError(f"SamplingParams.{name} is not supported")
        if isinstance(self.guided_decoding, dict):
            unknown = set(self.guided_decoding) - set(GuidedDecodingParams.__dataclass_fields__)
            if unknown:
                raise ValueError(f"SamplingParams.guided_decoding: unknown keys {sorted(unknown)}")
            self.guided_decoding = GuidedDecodingParams(**self.guided_decoding)
        elif self.guided_decoding is not None and not isinstance(self.guided_decoding, GuidedDecodingParams):
            raise ValueError("SamplingParams.guided_decoding must be a GuidedDecodingParams or a dict of its keys")
        if self.guided_decoding is not None and self.min_tokens > 0:
            raise ValueError("SamplingParams.guided_decoding cannot be combined with min_tokens > 0")
        if isinstance(self.seed, (list, tuple)):
            raise ValueError("SamplingParams.seed: a per-request list of seeds is not supported (pass a list of SamplingParams)")
        if isinstance(self.top_k, bool) or int(self.top_k) != self.top_k or self.top_k < -1 or self.top_k == 0:
            raise ValueError(f"top_k must be -1 (disable), or at least 1, got {self.top_k}.")
        self.top_k = int(self.top_k)
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {self.min_p}.")
        for name in ("presence_penalty", "frequency_penalty"):
            if not -2.0 <= getattr(self, name) <= 2.0:
                raise ValueError(f"{name} must be in [-2, 2], got {getattr(self, name)}.")
        if int(self.min_tokens) != self.min_tokens or self.min_tokens < 0:
            raise ValueError(f"min_tokens must be greater than or equal to 0, got {self.min_tokens}.")
        if self.max_tokens is not None and self.min_tokens > self.max_tokens:
            raise ValueError(f"min_tokens must be less than or equal to max_tokens={self.max_tokens}, got {self.min_tokens}.")
        if self.stop is None:
            self.stop = []
        elif isinstance(self.stop, str):
            self.stop = [self.stop]
        else:
            self.stop = list(self.stop)
        if any(not isinstance(t, str) or not t for t in self.stop):
            raise ValueError("stop cannot contain an empty string.")
        if self.logit_bias is not None:
            try:
                self.logit_bias = {int(k): float(v) for k, v in dict(self.logit_bias).items()}
            except (TypeError, ValueError) as e:
                raise ValueError(f"logit_bias must map token ids to floats: {e}") from None
            if any(k < 0 or not np.isfinite(v) for k, v in self.logit_bias.items()):
                raise ValueError("logit_bias: token ids must be >= 0 and biases finite")
        if self.allowed_token_ids is not None:
            self.allowed_token_ids = [int(t) for t in self.allowed_token_ids]
            if not self.allowed_token_ids or min(self.allowed_token_ids) < 0:
                raise ValueError("allowed_token_ids must be a non-empty list of token ids")
        if self.bad_words is not None:
            self.bad_words = list(self.bad_words)
            if any(not isinstance(w, str) or not w for w in self.bad_words):
                raise ValueError("bad_words cannot contain an empty string.")


def continuous_eligible(sp: "SamplingParams", kv_cache_dtype: str = "bf16") -> bool:
    """Whether requests under `sp` may run through O3VEngine.generate_continuous (LLM(continuous_batching=True)): greedy, one
    completion each, nothing that is indexed by the decode column (log-probs, the extended controls, guides, stop strings) and
    bf16 K/V.  Everything else keeps static batches."""
    return bool(sp.temperature == 0.0 and sp.n == 1 and sp.logprobs is None and sp.prompt_logprobs is None and not sp.min_p
                and not sp.presence_penalty and not sp.frequency_penalty and not sp.min_tokens and not sp.logit_bias
                and sp.allowed_token_ids is None and not sp.bad_words and sp.guided_decoding is None and not sp.stop
                and kv_cache_dtype == "bf16")


class _IncrementalDetokenizer:
    """Text of a growing token list, one token at a time (the prefix / read offset scheme of vLLM's detokenize_incrementally and
    HF's TextStreamer: a token's text is what decoding adds behind the text of the tokens before it, held back while it ends in an
    incomplete UTF-8 sequence).  `ends[j]` = len(text) after token j."""

    def __init__(self, decode):
        self.decode, self.toks, self.text, self.ends, self.prefix, self.read = decode, [], "", [], 0, 0

    def push(self, tok: int):
        self.toks.append(int(tok))
        before = self.decode(self.toks[self.prefix:self.read]) if self.read > self.prefix else ""
        now = self.decode(self.toks[self.prefix:])
        if len(now) > len(before) and not now.endswith("\ufffd"):
            self.text += now[len(before):]
            self.prefix, self.read = self.read, len(self.toks)
        self.ends.append(len(self.text))


def find_stop(detok: "_IncrementalDetokenizer", j: int, stop: Sequence[str]):
    """vLLM's StopChecker for stop strings at token j (0-based) of `detok`: the first string of `stop` that the token's text
    completes (an occurrence that ends inside the characters this token added) -> (string, index of its first character)."""
    old = detok.ends[j - 1] if j else 0
    new = detok.ends[j]
    if new == old:
        return None
    text = detok.text[:new]
    for s_ in stop:
        i = text.find(s_, max(0, old - len(s_) + 1))
        if i >= 0:
            return s_, i
    return None


@dataclass
class Logprob:
    logprob: float
    rank: Optional[int] = None
    decoded_token: Optional[str] = None


@dataclass
class CompletionOutput:
    index: int
    text: str
    token_ids: List[int]
    finish_reason: str = "length"
    cumulative_logprob: Optional[float] = None
    logprobs: Optional[List[dict]] = None    # one {token_id: Logprob} per token of token_ids
    stop_reason: Any = None                  # None: EOS or length; the token id of a stop_token_ids hit; the string of a stop hit


@dataclass
class RequestOutput:
    request_id: str
    prompt: str
    prompt_token_ids: List[int]
    outputs: List[CompletionOutput] = field(default_factory=list)
    prompt_logprobs: Optional[List[Optional[dict]]] = None   # None, then one {token_id: Logprob} per prompt token after the first


def logprob_dicts(token_ids, token_lp, rank, top_ids, top_lp, n: int, decode=None) -> List[dict]:
    """vLLM V0's per-position dict (sampler.py _get_sampled_logprob_if_needed / _get_prompt_logprob_if_needed): the position's own
    token with its rank, then the n most likely tokens with ranks 1..n (which win when the token is among them).  Host arrays:
    token_lp / rank [T], top_ids / top_lp [T, >= n]."""
    dec = decode or (lambda t: None)
    out = []
    for j, t in enumerate(token_ids):
        d = {int(t): Logprob(float(token_lp[j]), int(rank[j]), dec(int(t)))}
        for k in range(n):
            tid = int(top_ids[j][k])
            if tid >= 0:
                d[tid] = Logprob(float(top_lp[j][k]), k + 1, dec(tid))
        out.append(d)
    return out


def _host_logprobs(lp):
    """engine.Logprobs (device tensors) -> host arrays (token, rank, top_ids, top)."""
    return None if lp is None else tuple(t.cpu().numpy() for t in (lp.token, lp.rank, lp.top_ids, lp.top))


def _load_tokenizer(path):
    from transformers import AutoTokenizer  # local files only; never downloads
    return AutoTokenizer.from_pretrained(path, local_files_only=True)


def shared_prefix_groups(ids_list, vkeys, visual_ids):
    """Which requests of one generate() call run as shared-prefix groups: -> (groups: [(P, positions)], rest: positions that go
    the ordinary way), both in input order.  Requests with the same visual key form a group when there are at least two of them
    and their longest common token prefix, capped so that every request keeps a token behind it, ends at or after the last visual
    placeholder (P >= 1: everything visual, and whatever text precedes it, is shared)."""
    by_key = {}
    for i, k in enumerate(vkeys):
        by_key.setdefault(k, []).append(i)
    groups, rest = [], []
    for k, at in by_key.items():
        P = 0
        if len(at) >= 2:
            first = ids_list[at[0]]
            P = min(len(ids_list[i]) for i in at) - 1
            for i in at[1:]:
                row = ids_list[i]
                P = next((j for j in range(P) if row[j] != first[j]), P)
            last_visual = max((j for j, t in enumerate(first) if t in visual_ids), default=-1)
            if P <= last_visual or any(t in visual_ids for i in at for t in ids_list[i][P:]):
                P = 0
        if P >= 1:
            groups.append((P, at))
        else:
            rest += at
    return groups, sorted(rest)


def decode_quantization(quantization: Optional[str]) -> dict:
    """vLLM's `quantization` keyword -> the DeviceWeights switches it stands for; any value that is not built is refused by name."""
    if quantization not in (None, "fp8", "mxfp4"):
        raise ValueError(f"quantization={quantization!r}: only None, 'fp8' (decode rows) or 'mxfp4' (MLP decode rows) is built")
    return dict(fp8_decode=quantization in ("fp8", "mxfp4"), mxfp4_decode=quantization == "mxfp4")


class LoRARequest:
    """vllm.lora.request.LoRARequest: a name, a positive id and the local adapter directory (adapter_config.json +
    adapter_model.safetensors).  Two requests name the same adapter when id and path agree."""

    def __init__(self, lora_name: str, lora_int_id: int, lora_path: str = "", **_):
        if int(lora_int_id) < 1:
            raise ValueError(f"id must be > 0, got {lora_int_id}")
        self.lora_name, self.lora_int_id, self.lora_path = lora_name, int(lora_int_id), lora_path

    @property
    def key(self):
        return (self.lora_int_id, self.lora_path)

    def __eq__(self, other):
        return isinstance(other, LoRARequest) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return f"LoRARequest(lora_name={self.lora_name!r}, lora_int_id={self.lora_int_id}, lora_path={self.lora_path!r})"


class LLM:
    IMAGE_PAD = "<|image_pad|>"
    VIDEO_PAD = "<|video_pad|>"
    VISION_START, VISION_END = "<|vision_start|>", "<|vision_end|>"

    def __init__(self, model: str = None, tensor_parallel_size: int = 1, max_model_len: int = 81920,
                 gpu_memory_utilization: float = 0.9, limit_mm_per_prompt: Optional[dict] = None, dtype: str = "bfloat16",
                 max_num_seqs: int = 8, engine: Optional[O3VEngine] = None, tokenizer: Any = None,
                 min_pixels: int = 56 * 56, max_pixels: int = 14 * 14 * 4 * 1280, device="cuda",
                 enable_prefix_caching: bool = True, quantization: Optional[str] = None, mm_processor_kwargs: Optional[dict] = None,
                 position_mode: str = "pinned", fp8_prefill: bool = False, kv_cache_dtype: str = "auto",
                 share_video_prefix: bool = False, enable_lora: bool = False, max_lora_rank: int = 16,
                 continuous_batching: bool = False, **_):
        # vLLM's keyword: "fp8" / "fp8_e4m3" keep the K/V cache of independent-row decodes as e4m3fn rows with one power-of-two scale
        # per (token, kv head) (O3VEngine.kv_cache_dtype; not vLLM's per-tensor k_scale / v_scale: parity unpinned against vLLM)
        kv_dtypes = {"auto": "bf16", "bfloat16": "bf16", "fp8": "fp8", "fp8_e4m3": "fp8"}
        if kv_cache_dtype not in kv_dtypes:
            raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r}: only 'auto', 'bfloat16', 'fp8' or 'fp8_e4m3' is built")
        if tensor_parallel_size != 1:
            raise ValueError("the reference runs tensor_parallel_size=1 (R:eval/models/model_vllm.py:21); data parallelism "
                             "is one engine per GPU (open_o3_video_amd.dist)")
        if dtype not in ("bfloat16", "auto"):
            raise ValueError("bf16 only")
        if engine is None:
            if model is None or not os.path.isdir(model):
                raise OSError(f"{model} is not a local checkpoint directory (this build never downloads)")
            cfg = O3VConfig.from_pretrained(model)
            # vLLM's keyword: quantization="fp8" quantises the bf16 checkpoint's linears on load (here: fp8 e4m3fn decode rows with
            # one power-of-two scale per output row beside the bf16 matrices, which prefill keeps using; BASELINE config #5)
            # "mxfp4": those fp8 rows, and MXFP4 images (OCP MX: e2m1 codes, one e8m0 scale per 32 weights, rounded to nearest on
            # load) of the MLP matrices, which the decode streams instead -- no calibrated checkpoint behind it: parity unpinned
            wq = decode_quantization(quantization)
            engine = O3VEngine(cfg, DeviceWeights(cfg, getter_from_safetensors_dir(model), device, **wq))
            # vLLM's fp8 linears quantise the activations per token as well (W8A8); here that is opt-in for the compute-bound
            # prefill (fp8 x fp8 on the matrix cores), while the decode keeps bf16 activations on the exactly widened fp8 rows
            if fp8_prefill and not wq["fp8_decode"]:
                raise ValueError("fp8_prefill=True needs quantization='fp8' or 'mxfp4'")
            engine.fp8_prefill = bool(fp8_prefill)
            tokenizer = tokenizer or _load_tokenizer(model)
            pp = os.path.join(model, "preprocessor_config.json")
            if os.path.exists(pp):
                import json
                with open(pp) as f:
                    pc = json.load(f)
                # either the flat keys or transformers 5.x's size = {shortest_edge: min pixels, longest_edge: max pixels}
                size = pc.get("size") or {}
                min_pixels = pc.get("min_pixels") or size.get("shortest_edge") or min_pixels
                max_pixels = pc.get("max_pixels") or size.get("longest_edge") or max_pixels
        if tokenizer is None:
            raise ValueError("a tokenizer is required (encode / decode / convert_tokens_to_ids)")
        self.generation_eos_ids = []
        if model is not None and os.path.isdir(model):
            from .hf_api import load_generation_config
            ge = load_generation_config(model).get("eos_token_id")
            self.generation_eos_ids = [] if ge is None else ([int(e) for e in ge] if isinstance(ge, (list, tuple)) else [int(ge)])
        self.engine, self.tokenizer = engine, tokenizer
        engine.kv_cache_dtype = kv_dtypes[kv_cache_dtype]
        self.image_factor = engine.cfg.vision.patch_size * engine.cfg.vision.spatial_merge_size   # 28; Qwen3-VL: 32
        self.max_num_seqs = int(max_num_seqs)   # requests of one generate() call decoded together (<= O3VEngine.MAX_ROWS)
        self.cfg = engine.cfg
        self.max_model_len = max_model_len
        self.limit_mm = dict(limit_mm_per_prompt or {})
        self.min_pixels, self.max_pixels = min_pixels, max_pixels
        self._req = 0
        # cross-prompt visual reuse: the V-STAR harness asks 5 questions per video and the
        # test-time-scaling loop N samples per video (R:eval/test/test_vstar_multi_images.py:511-544), each of which
        # re-encodes identical frames in the reference.  Merged visual tokens are cached per frame-tensor content.
        self._vis_cache = {}
        self.vis_cache_size = 4
        self.vis_cache_hits = 0
        # prompt-prefix K/V reuse per video (same section): only the tokens after the longest common token prefix of two
        # prompts over identical frames are prefilled; vLLM's `enable_prefix_caching` keyword switches it
        self.enable_prefix_caching = bool(enable_prefix_caching)
        self.prefix_tokens_reused = 0
        # opt-in: the requests of one generate() call over the same visual content ("five questions about one video") run as ONE
        # engine call that prefills their common prefix once and decodes them as a group reading its K/V once per step
        # (O3VEngine.generate(shared_prefix_len=...)); counted in shared_prefix_calls / shared_prefix_rows
        self.share_video_prefix = bool(share_video_prefix)
        self.shared_prefix_calls = self.shared_prefix_rows = 0
        # opt-in: a generate() call with more requests than decode rows refills a row as soon as its request ends
        # (O3VEngine.generate_continuous) where continuous_eligible() allows; counted in continuous_sessions / rows_refilled /
        # decode_forwards.  Off, or not eligible: static batches of max_num_seqs rows.
        self.continuous_batching = bool(continuous_batching)
        self.continuous_sessions = self.rows_refilled = self.decode_forwards = 0
        # guided decoding: the token-level automata of the last two (pattern, EOS ids) on the device, and the tokenizer's byte strings
        self._guides = {}
        self._token_bytes = None
        self.guide_cache_hits = 0
        # native video inputs: HF's Qwen2_5_VLProcessor gives every video second_per_grid_ts = temporal_patch_size / fps with
        # fps = 2.0 unless mm_processor_kwargs={"fps": ...} says otherwise (TF:models/qwen2_5_vl/processing_qwen2_5_vl.py:143-153;
        # the reference passes none, R:eval/models/model_vllm.py:18-26)
        self.mm_processor_kwargs = dict(mm_processor_kwargs or {})
        # video rope arithmetic: "pinned" = vllm 0.7.2's MRotaryEmbedding.get_input_positions (R:setup.sh:7; restated, parity
        # unpinned), "tf5" = transformers 5.15 (goldens G5b / G14 / G15); see indexing.rope_index
        self.position_mode = position_mode
        # vLLM's LoRA keywords: generate(lora_request=LoRARequest(...)) runs under that adapter, merged on the device
        # (O3VEngine.load_adapter); ONE adapter is resident, a request for another (id, path) replaces it
        self.enable_lora, self.max_lora_rank = bool(enable_lora), int(max_lora_rank)
        self._lora_resident = None

    def _apply_lora(self, lora_request, n_inputs: int):
        """Bring the engine into the adapter state a generate call asks for.  Without enable_lora and without a request nothing is
        touched."""
        if isinstance(lora_request, (list, tuple)):
            if len(lora_request) != n_inputs:
                raise ValueError(f"The lengths of prompts ({n_inputs}) and lora_request ({len(lora_request)}) must be the same.")
            first = lora_request[0] if lora_request else None
            for r in lora_request:
                if (r.key if r is not None else None) != (first.key if first is not None else None):
                    raise ValueError(f"lora_request: {first!r} and {r!r} in one call; one adapter is resident at a time, so every "
                                     "request of a generate call must name the same adapter (or none)")
            lora_request = first
        if lora_request is None:
            if self.enable_lora and self.engine.adapter_loaded:
                self.engine.set_adapter_enabled(False)
            return
        if not self.enable_lora:
            raise ValueError(f"Got lora_request {lora_request} but LoRA is not enabled!")
        if self._lora_resident != lora_request.key or not self.engine.adapter_loaded:
            from .hf_api import read_adapter_dir
            if not os.path.isdir(lora_request.lora_path):
                raise OSError(f"{lora_request.lora_path} is not a local adapter directory (this build never downloads)")
            tensors, alpha, rslora = read_adapter_dir(lora_request.lora_path)
            rank = max((t.shape[0] for n, t in tensors if ".lora_A." in n), default=0)
            if rank > self.max_lora_rank:
                raise ValueError(f"{lora_request.lora_name}: LoRA rank {rank} is greater than max_lora_rank {self.max_lora_rank}")
            self._lora_resident = None
            self.engine.load_adapter(tensors, lora_alpha=alpha, use_rslora=rslora)
            self._lora_resident = lora_request.key
        else:
            self.engine.set_adapter_enabled(True)

    # ---- new policy weights (GRPO / GSPO: the trainer pushes them after every optimizer step)
    def load_weights(self, weights) -> set:
        """vLLM's model.load_weights(iterable of (HF name, tensor)): packed weights rewritten in place on the GPU, then every
        cache derived from them dropped (O3VEngine.load_weights)."""
        done = self.engine.load_weights(weights)
        self._vis_cache.clear()
        return done

    def reset_prefix_cache(self) -> bool:
        self.engine.drop_prefix_cache()
        self.engine.drop_prompt_handover()
        return True

    @property
    def llm_engine(self):
        """The attribute chain TRL pushes weights through after each step:
        llm.llm_engine.model_executor.driver_worker.model_runner.model.load_weights(model.state_dict().items())."""
        model = SimpleNamespace(load_weights=self.load_weights)
        runner = SimpleNamespace(model=model)
        return SimpleNamespace(model_executor=SimpleNamespace(driver_worker=SimpleNamespace(model_runner=runner)),
                               reset_prefix_cache=self.reset_prefix_cache)

    # ---- multimodal input -> uint8/f32 frames [T,3,H,W] with H,W multiples of 28
    def _frames(self, mm) -> Optional[torch.Tensor]:
        if not mm:
            return None
        data = mm.get("image", None)
        if data is None:
            return None
        if isinstance(data, (list, tuple)):
            lim = self.limit_mm.get("image")
            if lim is not None and len(data) > lim:
                raise ValueError(f"{len(data)} images exceed limit_mm_per_prompt['image']={lim}")
            frames = []
            for im in data:
                arr = np.asarray(im.convert("RGB") if hasattr(im, "convert") else im)
                if arr.ndim == 3 and arr.shape[-1] == 3:
                    arr = arr.transpose(2, 0, 1)
                frames.append(torch.from_numpy(np.ascontiguousarray(arr)))
            sizes = {tuple(f.shape[1:]) for f in frames}
            if len(sizes) != 1:
                raise NotImplementedError("images of different sizes in one request")
            data = torch.stack(frames)
        else:
            data = torch.as_tensor(np.asarray(data)) if not torch.is_tensor(data) else data
            if data.dim() == 3:
                data = data[None]
        if data.shape[1] != 3 and data.shape[-1] == 3:
            data = data.permute(0, 3, 1, 2)
        T, _, H, W = data.shape
        # the HF image processor resizes every image with smart_resize(factor = patch x merge: 28, Qwen3-VL 32; min/max pixels) -- a no-op for frames
        # that process_vision_info already sized
        rh, rw = vp.smart_resize(H, W, self.image_factor, self.min_pixels, self.max_pixels)
        if (rh, rw) != (H, W):
            data = vp.resize_frames_device(data, (rh, rw))   # antialiased bicubic on the GPU; frames stay on the device
        return data

    def _videos(self, mm):
        """multi_modal_data["video"] -> list of (frames [T,3,H,W] sized by smart_resize, metadata dict).  One array / tensor is one
        video (R:eval/models/model_vllm.py:72-88 sends `v_input.numpy()`, f32 0..255 from process_vision_info); a list holds
        several; an (array, metadata) pair carries {"fps", "frames_indices"} for Qwen3-VL's timestamps."""
        data = None if not mm else mm.get("video", None)
        if data is None:
            return []
        if isinstance(data, tuple) and len(data) == 2 and isinstance(data[1], dict):
            data = [data]
        elif not isinstance(data, list):
            data = [data]
        lim = self.limit_mm.get("video")
        if lim is not None and len(data) > lim:
            raise ValueError(f"{len(data)} videos exceed limit_mm_per_prompt['video']={lim}")
        out = []
        for item in data:
            meta = {}
            if isinstance(item, tuple) and len(item) == 2 and isinstance(item[1], dict):
                item, meta = item
            v = item if torch.is_tensor(item) else torch.as_tensor(np.asarray(item))
            if v.dim() != 4:
                raise ValueError("a video is a [T,3,H,W] (or [T,H,W,3]) array of frames")
            if v.shape[1] != 3 and v.shape[-1] == 3:
                v = v.permute(0, 3, 1, 2)
            T, _, H, W = v.shape
            rh, rw = vp.smart_resize(H, W, self.image_factor, self.min_pixels, self.max_pixels)
            if (rh, rw) != (H, W):
                v = vp.resize_frames_device(v, (rh, rw))
            out.append((v, dict(meta)))
        return out

    def _cached_visual(self, fr: torch.Tensor, video: bool):
        """ViT + merger output for image frames / one native video, cached by content: (kind, shape, dtype, 128-bit hash of the
        bytes computed on the device by o3v_content_hash128 -- one pass over the frames, one 16-byte read-back)."""
        import ctypes as C
        from . import _lib
        fr = fr.to(self.engine.dev).contiguous()
        if fr.data_ptr() % 8:       # frames that came in on the device as a view into a larger buffer: the kernel reads 8-byte words
            fr = fr.clone()
        h = torch.zeros(2, dtype=torch.int64, device=fr.device)
        _lib.call("o3v_content_hash128", C.c_void_p(fr.data_ptr()), fr.numel() * fr.element_size(), C.c_void_p(h.data_ptr()),
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        # the weights version keys the entry too: visual tokens computed before load_weights are never served after it
        key = ("video" if video else "image", tuple(fr.shape), str(fr.dtype), self.engine.weights_version) + \
            tuple(int(v) for v in h.tolist())
        hit = self._vis_cache.get(key)
        if hit is not None:
            self.vis_cache_hits += 1
            return hit[0], hit[1], key
        px, grid = self.engine.pixels_from_video(fr) if video else self.engine.pixels_from_frames(fr)
        vis = self.engine.vit_forward(px, grid)
        if len(self._vis_cache) >= self.vis_cache_size:
            self._vis_cache.pop(next(iter(self._vis_cache)))
        self._vis_cache[key] = (vis, grid)
        return vis, grid, key

    def _visual_tokens(self, frames: torch.Tensor):
        vis, _, key = self._cached_visual(frames, video=False)
        return vis, key

    def _video_placeholder(self, grid_row, meta) -> str:
        """What one <|video_pad|> of the prompt becomes.  Qwen2.5-VL (TF:models/qwen2_5_vl/processing_qwen2_5_vl.py:64-67): t*gh*gw/4
        pads.  Qwen3-VL (TF:models/qwen3_vl/processing_qwen3_vl.py:81-107,178-189): per temporal patch "<{t:.1f} seconds>" +
        <|vision_start|> gh*gw/4 pads <|vision_end|>, the time being the mean of the patch's first / last frame index over the
        video fps (fps 24 and indices 0..T-1 when the request carries no metadata, as HF falls back)."""
        t, gh, gw = (int(v) for v in grid_row)
        per = gh * gw // self.cfg.vision.merge_unit
        if self.cfg.arch != "qwen3_vl":
            return self.VIDEO_PAD * (t * per)
        fps = float(meta.get("fps") or 24)
        idx = list(meta.get("frames_indices") if meta.get("frames_indices") is not None else range(int(meta.get("n_frames", 2 * t))))
        idx = [float(i) for i in idx]
        if len(idx) % 2:
            idx.append(idx[-1])
        ts = [i / fps for i in idx]
        ts = [(ts[i] + ts[i + 1]) / 2 for i in range(0, len(ts), 2)]
        return "".join(f"<{ts[k]:.1f} seconds>" + self.VISION_START + self.VIDEO_PAD * per + self.VISION_END for k in range(t))

    def _tokenize(self, prompt: str, n_frames: int, tok_per_frame: int, video_placeholders: Sequence[str] = ()):
        if n_frames:
            n_tags = prompt.count(self.IMAGE_PAD)
            if n_tags != n_frames:
                raise ValueError(f"prompt has {n_tags} image placeholders but {n_frames} images were given")
            prompt = prompt.replace(self.IMAGE_PAD, self.IMAGE_PAD * tok_per_frame)
        n_vtags = prompt.count(self.VIDEO_PAD)
        if n_vtags != len(video_placeholders):
            raise ValueError(f"prompt has {n_vtags} video placeholders but {len(video_placeholders)} videos were given")
        if n_vtags:
            q3 = self.cfg.arch == "qwen3_vl"
            triple = self.VISION_START + self.VIDEO_PAD + self.VISION_END
            parts, rest = [], prompt
            for ph in video_placeholders:
                i = rest.index(self.VIDEO_PAD)
                # Qwen3-VL's expansion carries its own <|vision_start|> / <|vision_end|> per temporal patch: it replaces the whole
                # <|vision_start|><|video_pad|><|vision_end|> of the chat template when the pad stands inside one
                if q3 and rest[max(0, i - len(self.VISION_START)):i + len(self.VIDEO_PAD) + len(self.VISION_END)] == triple:
                    parts.append(rest[:i - len(self.VISION_START)] + ph)
                    rest = rest[i + len(self.VIDEO_PAD) + len(self.VISION_END):]
                else:
                    parts.append(rest[:i] + ph)
                    rest = rest[i + len(self.VIDEO_PAD):]
            prompt = "".join(parts) + rest
        ids = self.tokenizer.encode(prompt, add_special_tokens=False) if hasattr(self.tokenizer, "encode") else self.tokenizer(prompt)
        return list(ids)

    def _banned_ids(self, sp: SamplingParams) -> List[int]:
        """bad_words as vLLM tokenises them (the word, and the word behind a space): single-token results are banned outright,
        anything longer would need per-step host logic and is refused."""
        banned = []
        for w in sp.bad_words or ():
            for text in (w.lstrip(), " " + w.lstrip()):
                ids = list(self.tokenizer.encode(text, add_special_tokens=False))
                if len(ids) > 1:
                    raise ValueError(f"bad_words: {w!r} tokenises to {len(ids)} tokens; only single-token bad words are supported")
                banned += [int(t) for t in ids if int(t) not in banned]
        return banned

    GUIDE_ENTRIES = 2

    def _guide(self, gd: GuidedDecodingParams, eos: Sequence[int]) -> "guided.Guide":
        """The device table of a pattern under the call's EOS ids: compiled once per (pattern, EOS ids, tokenizer), two kept."""
        V = self.cfg.text.vocab_size
        key = (gd.pattern, tuple(eos), id(self.tokenizer))
        g = self._guides.get(key)
        if g is not None:
            self.guide_cache_hits += 1
            self._guides[key] = self._guides.pop(key)      # most recent last
            return g
        if self._token_bytes is None or self._token_bytes[0] != id(self.tokenizer):
            self._token_bytes = (id(self.tokenizer), guided.token_bytes(self.tokenizer, V))
        table = guided.token_table(guided.compile_regex(gd.pattern), self._token_bytes[1], eos, V)
        g = guided.Guide(table=torch.from_numpy(table).to(self.engine.dev), n_states=table.shape[0], ldn=table.shape[1], start=0,
                         host_table=table)
        while len(self._guides) >= self.GUIDE_ENTRIES:
            self._guides.pop(next(iter(self._guides)))
        self._guides[key] = g
        return g

    def generate(self, inputs, sampling_params=None, use_tqdm: bool = False, lora_request=None):
        """`sampling_params`: one SamplingParams for every request, or a list with one per request.  Requests with equal parameters
        run together exactly as a single-parameter call runs them; results come back in input order, and request ids / default
        seeds follow the input position, so a request's samples do not depend on what it was grouped with.
        `lora_request` (needs LLM(enable_lora=True)): the adapter the call runs under, None = the base weights."""
        if isinstance(inputs, dict):
            inputs = [inputs]
        inputs = list(inputs)
        self._apply_lora(lora_request, len(inputs))
        if not isinstance(sampling_params, (list, tuple)):
            return self._generate_group(inputs, sampling_params or SamplingParams(), list(range(len(inputs))))
        if len(sampling_params) != len(inputs):
            raise ValueError(f"The lengths of prompts ({len(inputs)}) and sampling_params ({len(sampling_params)}) must be the same.")
        groups = []     # (SamplingParams, positions) in order of first appearance
        for pos, sp in enumerate(sampling_params):
            sp = sp or SamplingParams()
            for g in groups:
                if g[0] == sp:
                    g[1].append(pos)
                    break
            else:
                groups.append((sp, [pos]))
        base, results = self._req, [None] * len(inputs)
        for sp, positions in groups:
            self._req = base
            for pos, ro in zip(positions, self._generate_group([inputs[p] for p in positions], sp, positions)):
                results[pos] = ro
        self._req = base + len(inputs)
        return results

    def _generate_group(self, inputs, sp: SamplingParams, positions: Sequence[int]):
        """The requests `inputs` (input positions `positions` of the generate call) under one SamplingParams."""
        base = self._req
        greedy = sp.temperature == 0.0
        # vLLM stops on the request's stop ids, the model's eos id and every eos id of the checkpoint's generation_config.json
        stop = list(sp.stop_token_ids) if sp.stop_token_ids else []
        model_eos = [] if sp.ignore_eos else [self.cfg.eos_token_id] + list(self.generation_eos_ids)   # ignore_eos: only the request's own stops
        eos = stop + [e for e in model_eos if e is not None and e not in stop]
        eos = list(dict.fromkeys(int(e) for e in eos))
        common = dict(max_new_tokens=sp.max_tokens, eos_token_ids=eos, pad_token_id=self.cfg.pad_token_id,
                      repetition_penalty=sp.repetition_penalty, do_sample=not greedy,
                      temperature=1.0 if greedy else sp.temperature, top_p=1.0 if greedy else sp.top_p, return_margins=False)
        # the newer controls reach the engine only when they differ from their defaults; greedy ignores top_k / top_p / min_p
        V = self.cfg.text.vocab_size
        if not greedy and sp.top_k > 0:
            common["top_k"] = sp.top_k
        if not greedy and sp.min_p > 0:
            common["min_p"] = sp.min_p
        if sp.presence_penalty:
            common["presence_penalty"] = sp.presence_penalty
        if sp.frequency_penalty:
            common["frequency_penalty"] = sp.frequency_penalty
        if sp.min_tokens > 0:
            common["min_new_tokens"] = sp.min_tokens
        if sp.logit_bias:
            if max(sp.logit_bias) >= V:
                raise ValueError(f"logit_bias: token id {max(sp.logit_bias)} is outside the vocabulary ({V})")
            common["token_bias"] = dict(sp.logit_bias)
        banned = self._banned_ids(sp)
        if banned:
            common["banned_token_ids"] = banned
        if sp.allowed_token_ids is not None:
            if max(sp.allowed_token_ids) >= V:
                raise ValueError(f"allowed_token_ids: token id {max(sp.allowed_token_ids)} is outside the vocabulary ({V})")
            left = set(sp.allowed_token_ids) - set(banned)
            if not left or (sp.min_tokens > 0 and not left - set(eos)):
                raise ValueError("allowed_token_ids leaves no token to emit once the banned tokens"
                                 + (" and, before min_tokens, the stop ids" if left else "") + " are taken out")
            common["allowed_token_ids"] = list(sp.allowed_token_ids)
        if sp.guided_decoding is not None:      # the same guide through every call site below (rows, shared-prefix groups, n samples)
            common["guide"] = self._guide(sp.guided_decoding, eos)
        stop_strs = list(sp.stop)

        def tok_decode(toks):
            return self.tokenizer.decode(toks, skip_special_tokens=sp.skip_special_tokens)

        def row_end(detok, toks):
            """Where vLLM's StopChecker ends a row, checked after every single token: (number of tokens kept, finish_reason,
            stop_reason, text or None).  `detok` holds the text of toks[:len(detok.toks)] and is extended as far as needed."""
            for j, t in enumerate(toks):
                if stop_strs and j >= len(detok.toks):
                    detok.push(t)
                if j + 1 < sp.min_tokens:
                    continue        # nothing stops a row before min_tokens
                if t in eos:        # the stop token is dropped from token_ids and from the text
                    text = detok.text[:detok.ends[j - 1] if j else 0] if stop_strs else None
                    return j, "stop", (t if t in stop else None), text
                hit = find_stop(detok, j, stop_strs) if stop_strs else None
                if hit is not None:
                    cut = hit[1] + (len(hit[0]) if sp.include_stop_str_in_output else 0)
                    return j + 1, "stop", hit[0], detok.text[:cut]
            return len(toks), "length", None, (detok.text[:detok.ends[len(toks) - 1] if toks else 0] if stop_strs else None)

        def make_checker(n_rows):
            """engine.generate's stop_checker for one call: rows that a stop string has ended, at the token that completed it."""
            if not stop_strs:
                return None, None
            detoks = [_IncrementalDetokenizer(tok_decode) for _ in range(n_rows)]

            def checker(ids):
                rows = ids.tolist()
                if rows and len(rows[0]) < len(detoks[0].toks):     # the engine re-ran the call from step 0
                    detoks[:] = [_IncrementalDetokenizer(tok_decode) for _ in range(n_rows)]
                out = {}
                for b, toks in enumerate(rows):
                    n, _, stop_reason, _ = row_end(detoks[b], toks)
                    if isinstance(stop_reason, str):    # (a row that hit a stop id has ended on the GPU already)
                        out[b] = n
                return out
            return checker, detoks
        # logprobs=0 still reports the token's own log-prob: the engine is asked for at least one top entry (0 there means off)
        n_lp = None if sp.logprobs is None else int(sp.logprobs)
        n_plp = None if sp.prompt_logprobs is None else int(sp.prompt_logprobs)
        if n_lp is not None:
            common["logprobs"] = max(1, n_lp)
        decode_memo = {}

        def decode_one(t):
            if t not in decode_memo:
                decode_memo[t] = self.tokenizer.decode([t]) if hasattr(self.tokenizer, "decode") else None
            return decode_memo[t]
        # ---- per request: frames -> (cached) visual tokens, prompt -> ids
        prepared = []
        tps = self.cfg.vision.temporal_patch_size
        fps = float(self.mm_processor_kwargs.get("fps", 2.0))
        self.engine.position_mode = self.position_mode
        for req in inputs:
            prompt = req["prompt"] if isinstance(req, dict) else str(req)
            mm = req.get("multi_modal_data") if isinstance(req, dict) else None
            frames = self._frames(mm)
            videos = self._videos(mm)
            tpf = 0 if frames is None else (frames.shape[2] // self.image_factor) * (frames.shape[3] // self.image_factor)
            vis_i, grid, keys = None, None, []
            if frames is not None:
                vis_i, k = self._visual_tokens(frames)
                keys.append(k)
                ps = self.cfg.vision.patch_size
                grid = np.asarray([[1, frames.shape[2] // ps, frames.shape[3] // ps]] * frames.shape[0], dtype=np.int64)
            vis_v, vgrids, placeholders = [], [], []
            for v, meta in videos:
                vv, vg, k = self._cached_visual(v, video=True)
                vis_v.append(vv)
                vgrids.append(vg)
                placeholders.append(self._video_placeholder(vg[0], dict(meta, n_frames=v.shape[0])))
                keys.append(k)
            ids = self._tokenize(prompt, 0 if frames is None else frames.shape[0], tpf, placeholders)
            if len(ids) + sp.max_tokens > self.max_model_len:
                raise ValueError(f"prompt ({len(ids)}) + max_tokens ({sp.max_tokens}) exceeds max_model_len {self.max_model_len}")
            vgrid = np.concatenate(vgrids) if vgrids else None
            spg = [tps / fps] * len(vgrids) if vgrids else None
            # identifies what the prompt's K/V depend on besides the token ids (prefix-K/V reuse, shared-prefix groups): the visual
            # content and, with a video, the M-RoPE arithmetic its K rows were rotated with (indexing.rope_index: the modes agree on
            # images) -- the engine's store is shared by every facade over it
            vkey = tuple(keys) if keys else ("text-only",)
            if spg:
                vkey += (("positions", self.position_mode, tuple(spg)),)
            prepared.append((prompt, ids, vis_i, grid, vkey, vis_v, vgrid, spg))

        def cat_visual(img_parts, vid_parts):
            """[image tokens of every row ; video tokens of every row] -- the order engine.embed scatters them in."""
            parts = [p for p in img_parts if p is not None] + [p for p in vid_parts if p is not None]
            if not parts:
                return None
            return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-2)

        def finish(ro, index, row, n_prompt, lp=None, i=0):
            toks = row[n_prompt:].tolist()
            n, reason, stop_reason, text = row_end(_IncrementalDetokenizer(tok_decode), toks)
            toks = toks[:n]
            if text is None:
                text = tok_decode(toks)
            co = CompletionOutput(index, text, toks, reason, stop_reason=stop_reason)
            if lp is not None:      # trimmed exactly as token_ids
                tok_lp, rank, top_ids, top_lp = (a[i] for a in lp)
                co.logprobs = logprob_dicts(toks, tok_lp, rank, top_ids, top_lp, n_lp, decode_one)
                co.cumulative_logprob = float(np.sum(tok_lp[:len(toks)], dtype=np.float64))
            ro.outputs.append(co)

        def prompt_dicts(plp, i, ids, first_col):
            """[None] + one dict per prompt token after the first; prompt token k is column first_col + k - 1 of row i."""
            tok_lp, rank, top_ids, top_lp = (a[i, first_col:first_col + len(ids) - 1] for a in plp)
            return [None] + logprob_dicts(ids[1:], tok_lp, rank, top_ids, top_lp, n_plp, decode_one)

        results = []
        if len(prepared) > 1 and sp.n == 1 and self.max_num_seqs > 1:
            # several requests in one call (vLLM batches them, R:eval/models/model_vllm.py:23 max_num_seqs): decode up to
            # max_num_seqs of them together, left padded, every streamed weight byte shared by the rows of the step
            rows_per_call = min(self.max_num_seqs, O3VEngine.MAX_ROWS)
            results = [None] * len(prepared)

            def run_rows(at, shared=None):
                """One engine call over the requests prepared[i], i in `at`.  shared = (P, vkey): they share their first P tokens and
                the visual content `vkey` -- one row's visual inputs, the prefix prefilled once, the rows decoded as a group."""
                chunk = [prepared[i] for i in at]
                L = max(len(p[1]) for p in chunk)
                pad = self.cfg.pad_token_id
                rows = [[pad] * (L - len(p[1])) + p[1] for p in chunk]
                mask = [[0] * (L - len(p[1])) + [1] * len(p[1]) for p in chunk]
                vis_of = chunk[:1] if shared else chunk
                grid_parts = [p[3] for p in vis_of if p[3] is not None]
                vgrid_parts = [p[6] for p in vis_of if p[6] is not None]
                spg_all = [x for p in vis_of if p[7] for x in p[7]]
                if stop_strs:
                    common["stop_checker"] = make_checker(len(chunk))[0]
                extra = {}
                if shared:
                    extra = dict(shared_prefix_len=shared[0], prefix_key=shared[1] if self.enable_prefix_caching else None)
                out = self.engine.generate(rows, mask, vis_embeds=cat_visual([p[2] for p in vis_of], [v for p in vis_of for v in p[5]]),
                                           image_grid_thw=np.concatenate(grid_parts) if grid_parts else None,
                                           video_grid_thw=np.concatenate(vgrid_parts) if vgrid_parts else None,
                                           second_per_grid_ts=spg_all or None,
                                           row_ids=[base + positions[i] for i in at],
                                           seed=0 if sp.seed is None else sp.seed,
                                           prompt_logprobs=0 if n_plp is None else max(1, n_plp), **extra, **common)
                if shared:
                    self.shared_prefix_calls += 1
                    self.shared_prefix_rows += int(out.timings.get("shared_prefix_rows", 0))
                    self.prefix_tokens_reused += int(out.timings.get("prefix_tokens_reused", 0))
                lp, plp = _host_logprobs(out.logprobs), _host_logprobs(out.prompt_logprobs)
                for i, (at_i, p) in enumerate(zip(at, chunk)):
                    ro = RequestOutput(request_id=str(base + positions[at_i]), prompt=p[0], prompt_token_ids=p[1])
                    finish(ro, 0, out.sequences[i], L, lp, i)
                    if plp is not None:     # left padding: the row's first real token sits at column L - len(ids)
                        ro.prompt_logprobs = prompt_dicts(plp, i, p[1], L - len(p[1]))
                    results[at_i] = ro
                    self._req += 1

            rest = list(range(len(prepared)))
            if self.share_video_prefix and n_plp is None:
                visual_ids = (self.cfg.image_token_id, self.cfg.video_token_id)
                groups, rest = shared_prefix_groups([p[1] for p in prepared], [p[4] for p in prepared], visual_ids)
                for P, at in groups:
                    for c0 in range(0, len(at), rows_per_call):
                        run_rows(at[c0:c0 + rows_per_call], shared=(P, prepared[at[0]][4]))
            if (self.continuous_batching and len(prepared) > rows_per_call and rest
                    and continuous_eligible(sp, getattr(self.engine, "kv_cache_dtype", "bf16"))):
                # rows refilled in flight: every request not taken by a shared-prefix group, in input order
                creqs = [dict(ids=prepared[i][1], max_new_tokens=sp.max_tokens,
                              vis_embeds=cat_visual([prepared[i][2]], prepared[i][5]), image_grid_thw=prepared[i][3],
                              video_grid_thw=prepared[i][6], second_per_grid_ts=prepared[i][7]) for i in rest]
                outs = self.engine.generate_continuous(
                    creqs, rows_per_call, eos_token_ids=eos, repetition_penalty=sp.repetition_penalty,
                    pad_token_id=self.cfg.pad_token_id, return_margins=False,
                    prefix_keys=[prepared[i][4] for i in rest] if self.enable_prefix_caching else None)
                tmc = outs[0].timings
                self.continuous_sessions += int(tmc["sessions"])
                self.rows_refilled += int(tmc["rows_refilled"])
                self.decode_forwards += int(tmc["decode_forwards"])
                self.prefix_tokens_reused += int(tmc.get("prefix_tokens_reused", 0))
                for i, o in zip(rest, outs):
                    p = prepared[i]
                    ro = RequestOutput(request_id=str(base + positions[i]), prompt=p[0], prompt_token_ids=p[1])
                    finish(ro, 0, o.sequences[0], len(p[1]))
                    results[i] = ro
                    self._req += 1
                return results
            for c0 in range(0, len(rest), rows_per_call):
                run_rows(rest[c0:c0 + rows_per_call])
            return results
        for pos, (prompt, ids, vis_i, grid, vkey, vis_v, vgrid, spg) in zip(positions, prepared):
            vis = cat_visual([vis_i], vis_v)
            req = base + pos
            ro = RequestOutput(request_id=str(req), prompt=prompt, prompt_token_ids=ids)
            # n samples of one prompt (self-consistency, R:eval/tts.py:47-123) run in groups of <= 16 decode rows; sample i is
            # keyed by (seed, i) whatever group it lands in, and groups after the first reuse the whole prompt K/V
            for i0 in range(0, sp.n, O3VEngine.MAX_ROWS):
                g = min(O3VEngine.MAX_ROWS, sp.n - i0)
                if stop_strs:
                    common["stop_checker"] = make_checker(g)[0]
                out = self.engine.generate([ids], None, vis_embeds=vis, image_grid_thw=grid, video_grid_thw=vgrid,
                                           second_per_grid_ts=spg, num_return_sequences=g,
                                           row_ids=list(range(i0, i0 + g)), seed=req if sp.seed is None else sp.seed,
                                           prefix_key=vkey if self.enable_prefix_caching else None,
                                           prompt_logprobs=0 if n_plp is None or i0 else max(1, n_plp), **common)
                self.prefix_tokens_reused += int(out.timings.get("prefix_tokens_reused", 0))
                lp = _host_logprobs(out.logprobs)
                if out.prompt_logprobs is not None:
                    ro.prompt_logprobs = prompt_dicts(_host_logprobs(out.prompt_logprobs), 0, ids, 0)
                for i in range(g):
                    finish(ro, i0 + i, out.sequences[i], len(ids), lp, i)
            results.append(ro)
            self._req += 1
        return results
