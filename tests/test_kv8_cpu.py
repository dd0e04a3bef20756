"""Host side of the opt-in fp8 K/V cache (vLLM kv_cache_dtype): the quantiser restatement against the oracle, where the format is
in effect, the facade keyword, and the argument errors of the three entry points.  No GPU."""
import ctypes

import pytest
import torch

import fixture_models as fm
from kv8_ops import dequant, quant_rows128
from open_o3_video_amd import _lib
from open_o3_video_amd.engine import DecodePlan, kv_cache_in_effect, plan_decode
from oracle import quant_ref


def _rows():
    g = torch.Generator().manual_seed(0)
    base = torch.randn(128, generator=g).clamp(-0.99, 0.99)     # |base| < 1: the planted value below is the row's amax
    rows = []
    for k in (-12, -3, 0, 1, 7):
        for top in (448.0, 448.0 * (1 + 2.0 ** -7), 0.875 - 2.0 ** -8, 0.875, 0.875 + 2.0 ** -7, 0.5, 1.0 - 2.0 ** -8):
            r = base * top * 2.0 ** k * 0.5
            r[5] = -top * 2.0 ** k if len(rows) % 2 else top * 2.0 ** k       # the amax, with either sign
            rows.append(r)
    rows.append(torch.zeros(128))
    mixed = torch.randn(128, generator=g) * 3
    rows.append(mixed)
    rows.append(-mixed.abs())
    return torch.stack(rows).to(torch.bfloat16)


def test_quant_rows128_equals_the_oracle():
    """amax exactly 448 * 2^k, just above it, mantissa on either side of 0.875, a zero row, mixed signs (bf16 inputs)."""
    x = _rows()
    assert (x.float().abs().amax(1)[:35] > 0).all()
    q, s = quant_rows128(x)
    rq, rs = quant_ref.quantize_rows(x)
    assert torch.equal(s, rs) and torch.equal(q, rq.view(torch.uint8))
    assert s[-3].item() == 1.0 and not q[-3].any()                       # the zero row
    top = (x.float().abs().amax(1) / s)
    assert (top <= 448).all() and (top[:35] > 224).all()                 # the SMALLEST such power of two
    d = dequant(q, s)
    assert torch.equal(d.float(), quant_ref.dequantize_rows(rq, rs))
    q2, s2 = quant_rows128(x.view(2, 19, 128))                            # any leading shape
    assert torch.equal(q2.view_as(q), q) and torch.equal(s2.view_as(s), s)


def test_kv_cache_in_effect_table():
    def plan(D, B0, G, heads=(28, 4)):
        return plan_decode(heads[0], heads[1], D, B0, G, 300, 16)

    for B0 in (1, 4, 32):
        assert kv_cache_in_effect("fp8", 128, plan(128, B0, 1)) == "fp8"
        assert kv_cache_in_effect("bf16", 128, plan(128, B0, 1)) == "bf16"
        assert kv_cache_in_effect("fp8", 32, plan(32, B0, 1)) == "bf16"
    shared = plan(128, 2, 4)
    assert shared.shared_prompt and kv_cache_in_effect("fp8", 128, shared) == "bf16"
    fanned = plan_decode(28, 4, 128, 1, 4, 300, 16, group_attention=False)          # G rows, each with its own copy of the prompt
    assert not fanned.shared_prompt and kv_cache_in_effect("fp8", 128, fanned) == "fp8"
    # plan_decode itself is unchanged
    assert DecodePlan._fields == ("B", "own_splits", "shared_prompt", "Tmax", "nsplit", "group", "want_sync")
    assert plan(128, 1, 1).want_sync and not plan_decode(28, 4, 128, 1, 1, 300, 16, fused=False).want_sync


class _Tok:
    def encode(self, text, add_special_tokens=False):
        return [1]

    def decode(self, ids, skip_special_tokens=True):
        return ""


class _Engine:
    MAX_ROWS = 32

    def __init__(self):
        from open_o3_video_amd.config import O3VConfig
        self.cfg = O3VConfig.from_dict(fm.tiny_config())
        self.position_mode = "tf5"
        self.kv_cache_dtype = "bf16"


def test_vllm_facade_kv_cache_dtype_keyword():
    from open_o3_video_amd.vllm_api import LLM
    for value, want in (("auto", "bf16"), ("bfloat16", "bf16"), ("fp8", "fp8"), ("fp8_e4m3", "fp8")):
        eng = _Engine()
        eng.kv_cache_dtype = "fp8" if want == "bf16" else "bf16"       # the keyword decides, also for an engine passed in
        llm = LLM(engine=eng, tokenizer=_Tok(), kv_cache_dtype=value)
        assert llm.engine is eng and eng.kv_cache_dtype == want
    assert LLM(engine=_Engine(), tokenizer=_Tok()).engine.kv_cache_dtype == "bf16"
    for bad in ("fp8_e5m2", "int8", "", None):
        with pytest.raises(ValueError, match=repr(bad).replace("(", r"\(")):
            LLM(engine=_Engine(), tokenizer=_Tok(), kv_cache_dtype=bad)


def test_kv8_entry_points_argument_errors_without_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # o3v_kv8_quantize(Ksrc, Vsrc, K8, V8, Ks, Vs, heads, S, Tmax, D, stream)
    assert lib.o3v_kv8_quantize(p, p, p, None, p, p, 1, 1, 2, 128, None) == _lib.ERR_ARG
    assert lib.o3v_kv8_quantize(p, p, p, p, p, None, 1, 1, 2, 128, None) == _lib.ERR_ARG
    assert lib.o3v_kv8_quantize(p, p, p, p, p, p, 1, 3, 2, 128, None) == _lib.ERR_ARG          # S > Tmax
    assert lib.o3v_kv8_quantize(p, p, p, p, p, p, 1, 1, 2, 64, None) == _lib.ERR_SHAPE
    assert lib.o3v_kv8_quantize(p, p, p, p, p, p, 1, 0, 2, 128, None) == _lib.OK               # nothing to do
    # o3v_kv8_roundtrip(Kc, Vc, heads, Tmax, slot0, n, D, stream)
    assert lib.o3v_kv8_roundtrip(None, p, 1, 4, 0, 1, 128, None) == _lib.ERR_ARG
    assert lib.o3v_kv8_roundtrip(p, p, 1, 4, 3, 2, 128, None) == _lib.ERR_ARG                  # past the capacity
    assert lib.o3v_kv8_roundtrip(p, p, 1, 4, 0, 1, 64, None) == _lib.ERR_SHAPE
    assert lib.o3v_kv8_roundtrip(p, p, 1, 4, 0, 0, 128, None) == _lib.OK
    # o3v_attn_decode_kv8(Q, K8, V8, Ks, Vs, Knew, Vnew, out, part_o, part_ml, k_lo, B, Hq, Hkv, D, ctx, Tmax, nsplit, scale, stream)
    ok = [p] * 10
    for i in range(10):
        args = list(ok)
        args[i] = None
        assert lib.o3v_attn_decode_kv8(*args, None, 1, 8, 2, 128, 4, 8, 2, 0.1, None) == _lib.ERR_ARG, i
    assert lib.o3v_attn_decode_kv8(*ok, None, 1, 8, 2, 128, 9, 8, 2, 0.1, None) == _lib.ERR_ARG      # ctx > Tmax
    assert lib.o3v_attn_decode_kv8(*ok, None, 1, 8, 2, 128, 4, 8, 0, 0.1, None) == _lib.ERR_ARG      # no scalar form: nsplit > 0
    assert lib.o3v_attn_decode_kv8(*ok, None, 1, 8, 2, 64, 4, 8, 2, 0.1, None) == _lib.ERR_SHAPE     # head_dim 64
    assert lib.o3v_attn_decode_kv8(*ok, None, 1, 9, 1, 128, 4, 8, 2, 0.1, None) == _lib.ERR_SHAPE    # n_rep 9
    assert lib.o3v_attn_decode_kv8(*ok, None, 0, 8, 2, 128, 4, 8, 2, 0.1, None) == _lib.OK           # no rows
    # the decode state: the new fields sit behind `flags`, zero = off
    names = [f[0] for f in _lib.DecodeState._fields_]
    assert names[-5:] == ["flags", "k8", "v8", "k8s", "v8s"] and _lib.DECODE_KV8_EMULATE == 8
    st = _lib.DecodeState()
    assert not (st.k8 or st.v8 or st.k8s or st.v8s or st.flags)
