"""Test helpers of the fp8 K/V cache: thin torch-tensor wrappers over its three entry points (in the style of kernel_ops.py) and a
torch restatement of the row quantiser (the rule of o3v_quantize_rows_fp8 / oracle.quant_ref on rows of 128)."""
from __future__ import annotations

import ctypes as C

import torch

from kernel_ops import _buf, _p, _s
from open_o3_video_amd import _lib

F8 = torch.float8_e4m3fn


def quant_rows128(x: torch.Tensor):
    """[..., 128] (bf16 or float) -> (u8 codes [..., 128], f32 scales [...]): scale = the smallest power of two s with
    max|row| / s <= 448 (1.0 for a zero row), code = e4m3fn(x / s), round to nearest even.  Computed on the CPU, returned on x's
    device."""
    xf = x.detach().float().cpu()
    amax = xf.abs().amax(dim=-1)
    m, e = torch.frexp(amax)                      # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    s = torch.ldexp(torch.ones_like(amax), torch.where(m <= 0.875, e - 9, e - 8))
    s = torch.where(amax > 0, s, torch.ones_like(s))
    q = (xf / s[..., None]).to(F8).view(torch.uint8)
    return q.to(x.device), s.to(x.device)


def dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """codes u8 [..., 128], scales f32 [...] -> bf16 (exact: 4 significant bits times a power of two)."""
    v = q.cpu().view(F8).float() * s.cpu().float()[..., None]
    out = v.to(torch.bfloat16)
    assert torch.equal(out.float(), v)
    return out.to(q.device)


def kv8_quantize(ksrc, vsrc, k8, v8, ks, vs):
    """ksrc / vsrc bf16 [..., S, 128] -> slots 0..S-1 of k8 / v8 u8 [..., Tmax, 128] and ks / vs f32 [..., Tmax]."""
    S, D = ksrc.shape[-2], ksrc.shape[-1]
    heads = ksrc.numel() // (S * D) if S else 0
    _lib.call("o3v_kv8_quantize", _p(ksrc), _p(vsrc), _p(k8), _p(v8), _p(ks), _p(vs), heads, S, k8.shape[-2], D, _s())


def kv8_roundtrip_(kc, vc, slot0, n):
    """in place on bf16 [..., Tmax, 128]"""
    Tmax, D = kc.shape[-2], kc.shape[-1]
    _lib.call("o3v_kv8_roundtrip", _p(kc), _p(vc), kc.numel() // (Tmax * D), Tmax, slot0, n, D, _s())


def attn_decode_kv8(q, k8, v8, ks, vs, knew, vnew, k_lo, ctx, nsplit, scale, poison=False):
    """q [B, Hq, 128]; k8 / v8 [B, Hkv, Tmax, 128]; ks / vs [B, Hkv, Tmax]; knew / vnew bf16 [B, Hkv, 128]."""
    B, Hq, D = q.shape
    _, Hkv, Tmax, _ = k8.shape
    out = _buf(q.shape, q.dtype, q.device, poison)
    po = _buf(B * Hq * nsplit * D, torch.float32, q.device, poison)
    pm = _buf(B * Hq * nsplit * 2, torch.float32, q.device, poison)
    _lib.call("o3v_attn_decode_kv8", _p(q), _p(k8), _p(v8), _p(ks), _p(vs), _p(knew), _p(vnew), _p(out), _p(po), _p(pm), _p(k_lo), B, Hq,
              Hkv, D, ctx, Tmax, nsplit, float(scale), _s())
    return out


__all__ = ["quant_rows128", "dequant", "kv8_quantize", "kv8_roundtrip_", "attn_decode_kv8", "C"]
