"""ctypes binding of libo3v_hip.so (include/o3v.h).  The library is built in-tree by
``open_o3_video_amd.build``; there is NO fallback: if it is missing or a call fails we raise."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libo3v_hip.so")

OK, ERR_ARG, ERR_SHAPE, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3, -4
_ERR = {ERR_ARG: "bad argument", ERR_SHAPE: "unsupported shape", ERR_LAUNCH: "HIP launch failure",
        ERR_WORKSPACE: "workspace too small"}
EPI_NONE, EPI_RESIDUAL, EPI_GELU, EPI_SWIGLU, EPI_GELU_TANH = 0, 1, 2, 3, 6
MAX_DEEPSTACK = 8

vp, ip, fp, i32, i64, f32, u64, sz = (C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int, C.c_long,
                                      C.c_float, C.c_uint64, C.c_size_t)


class VitBlockW(C.Structure):
    _fields_ = [(n, vp) for n in ("norm1", "norm2", "qkv_w", "qkv_b", "proj_w", "proj_b", "gu_w", "gu_b", "down_w", "down_b")]


class VitDesc(C.Structure):
    _fields_ = [("depth", i32), ("hidden", i32), ("heads", i32), ("inter_pad", i32), ("out_hidden", i32),
                ("patch_k_pad", i32), ("merge_unit", i32), ("fullatt_mask", u64), ("patch_w", vp),
                ("blocks", C.POINTER(VitBlockW)), ("ln_q", vp), ("m0_w", vp), ("m0_b", vp), ("m2_w", vp), ("m2_b", vp), ("gemm_tile", i32)]


class LlmLayerW(C.Structure):
    _fields_ = [(n, vp) for n in ("ln1", "ln2", "qkv_w", "qkv_b", "o_w", "gu_w", "down_w", "qkv_wp", "o_wp", "gu_wp", "down_wp",
                                  "qkv_w8", "o_w8", "gu_w8", "down_w8", "qkv_s", "o_s", "gu_s", "down_s", "q_norm", "k_norm",
                                  "qkv_w8p", "o_w8p", "gu_w8p", "down_w8p", "gu_w4", "down_w4", "gu_s4", "down_s4", "gu_w4p", "down_w4p",
                                  "gu_s4p", "down_s4p")]


class Vit3BlockW(C.Structure):
    _fields_ = [(n, vp) for n in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w", "fc1_b",
                                  "fc2_w", "fc2_b")]


class Vit3MergerW(C.Structure):
    _fields_ = [(n, vp) for n in ("norm_w", "norm_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")] + [("postshuffle", i32)]


class Vit3Desc(C.Structure):
    _fields_ = [("depth", i32), ("hidden", i32), ("heads", i32), ("head_dim", i32), ("head_dim_pad", i32), ("inter_pad", i32),
                ("out_hidden", i32), ("patch_k_pad", i32), ("merge_unit", i32), ("n_deep", i32), ("deep_index", i32 * MAX_DEEPSTACK),
                ("gemm_tile", i32), ("patch_w", vp), ("patch_b", vp), ("blocks", C.POINTER(Vit3BlockW)), ("merger", Vit3MergerW),
                ("deep", Vit3MergerW * MAX_DEEPSTACK)]


class LlmDesc(C.Structure):
    _fields_ = [("hidden", i32), ("layers", i32), ("heads", i32), ("kv_heads", i32), ("head_dim", i32), ("inter", i32),
                ("vocab", i32), ("rms_eps", f32), ("embed", vp), ("layer", C.POINTER(LlmLayerW)), ("final_norm", vp),
                ("lm_head", vp), ("lm_head_p", vp), ("gemm_tile", i32), ("lm_head8", vp), ("lm_head_s", vp), ("lm_head8p", vp)]


class DecodeState(C.Structure):
    _fields_ = [("B", i32), ("S", i32), ("Tmax", i32), ("Tnew", i32), ("nsplit", i32), ("pad_id", i32), ("n_eos", i32),
                ("do_sample", i32), ("rep_penalty", f32), ("temperature", f32), ("top_p", f32), ("seed", u64),
                ("x", vp), ("kcache", vp), ("vcache", vp), ("cosT", vp), ("sinT", vp), ("logits", vp), ("seen", vp),
                ("cur_tok", vp), ("finished", vp), ("out_ids", vp), ("margins", vp), ("eos_ids", vp), ("k_lo", vp),
                ("row_id", vp), ("part_o", vp), ("part_ml", vp), ("sample_scratch", vp), ("workspace", vp),
                ("ws_bytes", sz), ("group", i32), ("sync", vp), ("top_k", i32), ("kprefix", vp), ("vprefix", vp),
                ("prefix_cap", i32), ("rows_per_prompt", i32), ("host_stats", vp), ("flags", i32), ("k8", vp), ("v8", vp),
                ("k8s", vp), ("v8s", vp)]


class DecodeStateOwn(DecodeState):
    """The whole o3v_decode_state: DecodeState (the fields up to `v8s`) followed by the pair of the suffixes behind a shared prefix.
    The decode entry points read the pair, so they take this type only."""
    _fields_ = [("own_past", i32), ("own_lo", vp)]


class DecodeStateRagged(DecodeStateOwn):
    """DecodeStateOwn followed by the ragged regime's three fields (continuous batching).  The library reads them only when `flags`
    has DECODE_RAGGED, so every other caller may keep passing a DecodeStateOwn."""
    _fields_ = [("row_base", vp), ("kstage", vp), ("vstage", vp)]


class LogprobOpts(C.Structure):
    _fields_ = [("n", i32), ("chosen_lp", vp), ("chosen_rank", vp), ("top_ids", vp), ("top_lp", vp)]


class SamplingOpts(C.Structure):
    """o3v_sampling_opts: min_p, presence / frequency penalty, min_tokens, the two static-edit vectors, the output counts."""
    _fields_ = [("min_p", f32), ("presence", f32), ("frequency", f32), ("min_tokens", i32), ("bias", vp), ("bias_early", vp),
                ("out_counts", vp)]


class GuidedOpts(C.Structure):
    """o3v_guided_opts: the token-level automaton of a guide (i16 [n_states, ldn]) and the rows' double-buffered states."""
    _fields_ = [("next", vp), ("n_states", i32), ("ldn", i32), ("state", vp)]


class PrefillOpts(C.Structure):
    _fields_ = [("ds_rows", vp), ("ds_src", vp), ("n_ds", i32), ("ds_feat", vp), ("n_deep", i32), ("ds_stride", i64),
                ("kprefix", vp), ("vprefix", vp), ("prefix_len", i32), ("prefix_cap", i32), ("rows_per_prefix", i32), ("w8a8", i32)]


class RepackDesc(C.Structure):
    _fields_ = [(n, vp) for n in ("src", "row_map", "col_map", "dst", "dst_frag", "dst8", "dst8_scale", "dst8_frag")] + \
               [("src_ld", C.c_int64)] + [(n, i32) for n in ("src_dtype", "src_rows", "src_cols", "rows", "cols", "blk0", "nblk",
                                                          "blk_stride")] + \
               [(n, vp) for n in ("dst4", "dst4_scale", "dst4_frag", "dst4_frag_scale")]


SRC_BF16, SRC_F32 = 0, 1   # O3V_SRC_* in include/o3v.h
LORA_MAX_RANK = 256        # O3V_LORA_MAX_RANK


class LoraDesc(C.Structure):
    """o3v_lora_desc: one o3v_lora_merge launch."""
    _fields_ = [(n, vp) for n in ("base", "A", "B", "out")] + [(n, C.c_int64) for n in ("base_ld", "a_ld", "b_ld", "out_ld")] + \
               [(n, i32) for n in ("ab_dtype", "N", "K", "r", "base_rows", "blk0", "blk_stride")] + [("scale", f32)]


# name -> argtypes (return type int unless listed in _RET)
SIGNATURES = {
    "o3v_abi_version": [],
    "o3v_ctx_create": [C.POINTER(LlmDesc), C.POINTER(VitDesc), C.POINTER(Vit3Desc)],
    "o3v_ctx_destroy": [vp],
    "o3v_ctx_llm": [vp],
    "o3v_ctx_vit": [vp],
    "o3v_ctx_vit3": [vp],
    "o3v_rmsnorm": [vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "o3v_layernorm": [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "o3v_qkv_norm_rope_cache": [vp, vp, vp, f32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_add_rows": [vp, vp, vp, vp, i32, i32, vp],
    "o3v_patchify_ps": [vp, i32, vp, i32, i32, i32, i32, i32, fp, fp, vp],
    "o3v_patchify_video": [vp, i32, vp, i32, i32, i32, i32, i32, fp, fp, vp],
    "o3v_vit_rope": [vp, vp, vp, i32, i32, i32, vp],
    "o3v_mrope_table": [vp, vp, vp, vp, vp, i32, i32, vp],
    "o3v_qkv_rope_cache": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_gather_rows": [vp, vp, vp, i32, i32, vp],
    "o3v_embed_scatter": [vp, vp, vp, vp, i32, i32, vp],
    "o3v_embed_tokens": [vp, vp, vp, i32, i32, vp],
    "o3v_cast_pad_f32_bf16": [vp, vp, i32, i32, i32, vp],
    "o3v_patchify": [vp, i32, vp, i32, i32, i32, i32, fp, fp, vp],
    "o3v_content_hash128": [vp, sz, vp, vp],
    "o3v_gemm_bf16": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_gemv_bf16": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_attn_tiles": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, i64, i64, i64, i64, i64, i64, f32, vp],
    "o3v_attn_decode": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "o3v_gemm_bf16_tile": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_gemm_bf16_phased": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_gemm_bf16_splitk": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp],
    "o3v_resize_bicubic_aa": [vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp],
    "o3v_crop_resize_bilinear": [vp, vp, vp, i32, i32, i32, i32, vp],
    "o3v_attn_decode_ragged": [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "o3v_attn_decode_group": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "o3v_decode_sync_bytes": [],
    "o3v_decode_attn_block_capacity": [i32, i32],
    "o3v_decode_attn_block_fp8": [vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32,
                                  i32, i32, i32, f32, vp, C.c_uint32, vp],
    "o3v_decode_attn_block_qknorm": [vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32,
                                     i32, i32, i32, i32, i32, f32, vp, C.c_uint32, vp],
    "o3v_decode_attn_block": [vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32,
                              i32, f32, vp, C.c_uint32, vp],
    "o3v_quantize_rows_fp8": [vp, vp, vp, i32, i32, i32, i32, vp],
    "o3v_kv8_quantize": [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp],
    "o3v_kv8_roundtrip": [vp, vp, i64, i32, i32, i32, i32, vp],
    "o3v_attn_decode_kv8": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "o3v_rmsnorm_quantize_fp8": [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "o3v_gemm_fp8": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_gemm_fp8_sched": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_sample_greedy": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, i32, vp, vp],
    "o3v_sample_greedy_embed": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, i32, vp, vp, vp, i32, vp],
    "o3v_gemv_norm_qkv_rope": [vp, vp, f32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_qkv_rope_fp8_rows": [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_linear_decode_fp8_rows": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_linear_decode_fp8": [vp, vp, f32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_gemv_norm_qkv_rope_fp8": [vp, vp, f32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_linear_decode": [vp, vp, f32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_linear_decode_mxfp4": [vp, vp, f32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_linear_decode_mxfp4_rows": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_quantize_rows_mxfp4": [vp, vp, vp, i32, i32, i32, vp],
    "o3v_gemv_norm_bf16": [vp, vp, f32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "o3v_sample_top_p": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, f32, u64, vp, i32, i32, vp, vp],
    "o3v_sample_top_k_top_p": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, i32, f32, u64, vp, i32, i32, vp, vp],
    "o3v_mark_seen": [vp, vp, i32, i32, i32, vp],
    "o3v_logprob_gather": [vp, vp, vp, i32, i32, i32, vp],
    "o3v_vit_workspace_bytes": [C.POINTER(VitDesc), i32],
    "o3v_vit_forward": [C.POINTER(VitDesc), vp, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, sz, vp, vp],
    "o3v_llm_workspace_bytes": [C.POINTER(LlmDesc), i32],
    "o3v_llm_prefill": [C.POINTER(LlmDesc), vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, sz, vp],
    "o3v_vit3_workspace_bytes": [C.POINTER(Vit3Desc), i32],
    "o3v_vit3_forward": [C.POINTER(Vit3Desc), vp, i32, vp, vp, vp, vp, i32, vp, sz, vp, vp, vp],
    "o3v_llm_prefill_ex": [C.POINTER(LlmDesc), vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, C.POINTER(PrefillOpts), vp, sz, vp],
    "o3v_attn_tiles_prefix": [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, vp, i32, i32, i32, i32, i32, i64, i64, i64, i64, i64, i64, i64,
                              i64, f32, vp],
    "o3v_attn_decode_group_prefix": [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "o3v_attn_decode_group_prefix_lo": [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                        f32, vp],
    "o3v_llm_head": [C.POINTER(LlmDesc), vp, i32, i32, vp, vp, vp],
    "o3v_llm_decode": [C.POINTER(LlmDesc), C.POINTER(DecodeStateOwn), i32, i32, i32, vp],
    "o3v_sample_logprobs": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, i32, f32, u64, vp, i32, i32, vp,
                            C.POINTER(LogprobOpts), vp],
    "o3v_logprobs_rows": [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp],
    "o3v_llm_decode_lp": [C.POINTER(LlmDesc), C.POINTER(DecodeStateOwn), C.POINTER(LogprobOpts), i32, i32, i32, vp],
    "o3v_repack_rows": [C.POINTER(RepackDesc), vp],
    "o3v_lora_merge": [C.POINTER(LoraDesc), vp],
    "o3v_sample_step_ex": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, i32, f32, u64, vp, i32, i32, vp,
                           C.POINTER(LogprobOpts), C.POINTER(SamplingOpts), vp],
    "o3v_llm_decode_ex": [C.POINTER(LlmDesc), C.POINTER(DecodeStateOwn), C.POINTER(LogprobOpts), C.POINTER(SamplingOpts), i32, i32, i32,
                          vp],
    "o3v_sample_step_guided": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, i32, f32, u64, vp, i32, i32, vp,
                               C.POINTER(LogprobOpts), C.POINTER(SamplingOpts), C.POINTER(GuidedOpts), vp],
    "o3v_llm_decode_guided": [C.POINTER(LlmDesc), C.POINTER(DecodeStateOwn), C.POINTER(LogprobOpts), C.POINTER(SamplingOpts),
                              C.POINTER(GuidedOpts), i32, i32, i32, vp],
}
_RET = {"o3v_ctx_create": vp, "o3v_ctx_destroy": None, "o3v_ctx_llm": C.POINTER(LlmDesc), "o3v_ctx_vit": C.POINTER(VitDesc),
        "o3v_ctx_vit3": C.POINTER(Vit3Desc), "o3v_vit_workspace_bytes": sz, "o3v_vit3_workspace_bytes": sz, "o3v_llm_workspace_bytes": sz, "o3v_decode_sync_bytes": sz}

SYNC_TMO_BYTE = 2048            # O3V_SYNC_TMO_BYTE in include/o3v.h
SAMPLE_SCRATCH_FLOATS = 40960   # O3V_SAMPLE_SCRATCH_FLOATS in include/o3v.h
MAX_LOGPROBS = 20               # O3V_MAX_LOGPROBS
MAX_COUNT = 65535               # the u16 output counts of o3v_sampling_opts saturate here
LOGPROB_ROW_SCRATCH_FLOATS = 384  # O3V_LOGPROB_ROW_SCRATCH_FLOATS
# o3v_decode_state.flags (values 1 and 2 are retired): O3V_DECODE_NO_QKV_FUSED_NORM (switches a form OFF), O3V_DECODE_KV8_EMULATE
# (tests: the fp8 K/V arithmetic on a bf16 cache)
DECODE_NO_QKV_FUSED_NORM, DECODE_KV8_EMULATE = 4, 8
DECODE_RAGGED = 16              # O3V_DECODE_RAGGED: the state is a DecodeStateRagged

_lib = None


class O3VError(RuntimeError):
    code = None  # the O3V_ERR_* value when a call of the library returned one


def load():
    """Load the HIP library (raises if it has not been built: there is no CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise O3VError(f"{LIB_PATH} not found: run `python -m open_o3_video_amd.build` (hipcc, gfx950)")
        # torch-ROCm bundles its own libamdhip64.so.7; import it FIRST so our DT_NEEDED entry resolves to the runtime
        # that owns torch's streams and allocations (two HIP runtimes in one process cannot launch on each other's
        # streams: "HIP launch failure").
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI and this table diverge
            fn.argtypes = args
            fn.restype = _RET.get(name, i32)
        if lib.o3v_abi_version() != 6:
            raise O3VError("libo3v_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != OK:
        err = O3VError(f"{what} failed: {_ERR.get(rc, rc)} ({rc})")
        err.code = rc
        raise err


def call(name: str, *args):
    check(getattr(load(), name)(*args), name)
