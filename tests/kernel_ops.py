"""Test helpers: thin torch-tensor wrappers over the per-op entry points of the C ABI (the engine calls the model-level
entry points instead).  Every wrapper launches on the current torch stream.  Used by tests/ and tools/ only."""
from __future__ import annotations

import ctypes as C

import torch

from open_o3_video_amd import _lib
from open_o3_video_amd._lib import EPI_GELU, EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU  # noqa: F401


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- canvases: operands and outputs placed inside a larger buffer the test owns, so that a padded pitch is really padded and a
# stray store or an over-read lands somewhere the test can look at.
NAN = "nan"          # input fill: bf16 / f32 NaN patterns (0x7FC0 and 0xFFFF on alternate rows, as nan_fill_ of test_gpu_kernels.py), 0x7F for bytes
CANARY = 0x5A5A5A5A  # output fill: a fixed non-NaN bit pattern (truncated to the element width)
TILE_ROWS = 256      # the tallest tile any kernel stages; rows past a ragged edge are clamped inside it
_RAW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.uint8: torch.uint8, torch.float32: torch.int32,
        torch.int32: torch.int32}


def guard_rows_for(rows, ld, widest_ld=None):
    """Guard rows on each side of a [rows, ld] view: one full tile at least, and enough that `rows` rounded up by one more tile and
    walked at the WIDEST pitch of the call (a swapped pitch, an over-read of a clamped tile) still ends inside the buffer."""
    widest = max(ld, widest_ld or ld)
    return max(TILE_ROWS, -(-((rows + TILE_ROWS) * widest) // ld) - rows)


class Canvas:
    """guard + rows + guard rows of `ld` elements filled with `fill`; `.view` is the [rows, cols] window of row stride ld in the
    middle.  untouched() raises AssertionError unless every element OUTSIDE the view (padding columns, guard rows) still holds
    the fill, compared as raw integers; untouched(whole=True) includes the view (an entry point that refused the call)."""

    def __init__(self, rows, cols, ld, dtype, fill, guard_rows=None, device="cpu"):
        assert cols <= ld and rows >= 0
        self.rows, self.cols, self.ld = rows, cols, ld
        self.guard = guard_rows_for(rows, ld) if guard_rows is None else guard_rows
        assert self.guard >= TILE_ROWS, "a guard is one full tile at least"
        raw_t = _RAW[dtype]
        self.raw = torch.empty((2 * self.guard + rows, ld), dtype=raw_t, device=device)
        if fill == NAN:
            if raw_t == torch.uint8:
                self.raw.fill_(0x7F)                 # e4m3fn NaN
            elif raw_t == torch.int16:
                self.raw[0::2] = 0x7FC0
                self.raw[1::2] = -1
            else:
                self.raw[0::2] = 0x7FC00000
                self.raw[1::2] = -1
        else:
            bits = raw_t.itemsize * 8
            v = int(fill) & ((1 << bits) - 1)
            self.raw.fill_(v - (1 << bits) if raw_t != torch.uint8 and v >= 1 << (bits - 1) else v)
        self.pristine = self.raw.clone()
        self.buf = self.raw.view(dtype)
        self.view = self.buf[self.guard:self.guard + rows, :cols]

    def load(self, x):
        """Put operand values into the view (an input, or a residual updated in place); they become part of the expected state."""
        self.view.copy_(x)
        self.pristine = self.raw.clone()
        return self.view

    def untouched(self, whole=False):
        diff = self.raw != self.pristine
        if not whole:
            diff[self.guard:self.guard + self.rows, :self.cols] = False
        if diff.any():
            r, c = (int(v) for v in diff.nonzero()[0])
            where = ("guard rows before the view" if r < self.guard else "guard rows after the view" if r >= self.guard + self.rows
                     else "padding columns" if c >= self.cols else "view")
            raise AssertionError(f"{int(diff.sum())} elements outside the view changed; first at buffer row {r} (view row {r - self.guard}), "
                                 f"column {c}: {where}")
        return True


def canvas(rows, cols, ld, dtype, fill, guard_rows=None, device="cpu"):
    return Canvas(rows, cols, ld, dtype, fill, guard_rows, device)


def _buf(shape, dtype, device, poison):
    """Output / split-partial buffer: uninitialised, or all NaN with poison=True (a slot the kernels fail to write then
    reaches the result as NaN)."""
    if poison:
        return torch.full(shape if isinstance(shape, (tuple, torch.Size)) else (shape,), float("nan"), dtype=dtype, device=device)
    return torch.empty(shape, dtype=dtype, device=device)


def rmsnorm(x, w, eps, out=None):
    """x (and a ready-made `out`) may be row-strided views: the pitches passed are their strides."""
    if out is None:
        out = torch.empty_like(x)
    _lib.call("o3v_rmsnorm", _p(x), _p(w), _p(out), x.shape[0], x.shape[1], x.stride(0), out.stride(0), float(eps), _s())
    return out


def gemm(a, w, bias=None, res=None, epi=EPI_NONE, force=None, tile=0, out=None):
    """out = epi(a @ w.T + bias).  force in {None,'gemm','gemv'}; tile 0 / 128 / 256 picks the MFMA GEMM kernel.
    a / w / res / out may be row-strided views (e.g. of a `canvas`): lda / ldw / ldr / ldo are their strides."""
    M, K = a.shape
    N = w.shape[0]
    No = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, No), dtype=torch.bfloat16, device=a.device)
    assert out.shape == (M, No)
    ldr = 0 if res is None else res.stride(0)
    if force == "gemv" or (force is None and M <= 8):
        _lib.call("o3v_gemv_bf16", _p(a), _p(w), _p(bias), _p(res), _p(out), M, N, K, a.stride(0), w.stride(0), out.stride(0), ldr, epi, _s())
    else:
        _lib.call("o3v_gemm_bf16_tile", _p(a), _p(w), _p(bias), _p(res), _p(out), M, N, K, a.stride(0), w.stride(0), out.stride(0), ldr,
                  epi, tile, _s())
    return out


def gemm_splitk(a, w, bias=None, res=None, epi=EPI_NONE, splits=8, out=None, poison=False):
    """Split-K form of `gemm` for few-tile shapes (epilogues NONE / RESIDUAL / GELU).  Views as in `gemm`; poison=True fills the
    workspace of partials with NaN first (a partial nobody writes then reaches the result)."""
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    assert out.shape == (M, N)
    ws = _buf(splits * M * N, torch.float32, a.device, poison)
    _lib.call("o3v_gemm_bf16_splitk", _p(a), _p(w), _p(bias), _p(res), _p(out), M, N, K, a.stride(0), w.stride(0), out.stride(0),
              0 if res is None else res.stride(0), epi, splits, _p(ws), ws.numel() * 4, _s())
    return out


def vit_rope_(qkv, cos, sin, H, D):
    _lib.call("o3v_vit_rope", _p(qkv), _p(cos), _p(sin), qkv.shape[0], H, D, _s())
    return qkv


def attn_tiles(q, k, v, tiles, Hq, n_rep, D, q_ts, k_ts, k_hs, k_bs, v_ts, v_hs, v_bs, out, o_ts, scale, rows_per_tile=64,
               poison=False):
    if poison:
        out.fill_(float("nan"))
    _lib.call("o3v_attn_tiles", _p(q), _p(k), _p(v), _p(out), _p(tiles), tiles.shape[0], rows_per_tile, Hq, n_rep, D, q_ts, k_ts, k_hs,
              k_bs, v_ts, v_hs, v_bs, o_ts, float(scale), _s())
    return out


def attn_decode(q, kc, vc, k_lo, ctx, nsplit, scale, poison=False):
    B, Hq, D = q.shape
    _, Hkv, Tmax, _ = kc.shape
    ns = abs(nsplit)  # negative nsplit selects the scalar (non-MFMA) kernel
    out = _buf(q.shape, q.dtype, q.device, poison)
    po = _buf(B * Hq * ns * D, torch.float32, q.device, poison)
    pm = _buf(B * Hq * ns * 2, torch.float32, q.device, poison)
    _lib.call("o3v_attn_decode", _p(q), _p(kc), _p(vc), _p(out), _p(po), _p(pm), _p(k_lo), B, Hq, Hkv, D, ctx, Tmax, nsplit,
              float(scale), _s())
    return out


def attn_decode_group(q, kc, vc, k_lo, G, prefix_len, ctx, nsplit_prefix, scale, poison=False):
    B, Hq, D = q.shape
    _, Hkv, Tmax, _ = kc.shape
    out = _buf(q.shape, q.dtype, q.device, poison)
    po = _buf(B * Hq * 64 * D, torch.float32, q.device, poison)
    pm = _buf(B * Hq * 64 * 2, torch.float32, q.device, poison)
    _lib.call("o3v_attn_decode_group", _p(q), _p(kc), _p(vc), _p(out), _p(po), _p(pm), _p(k_lo), B, G, Hq, Hkv, D, prefix_len, ctx,
              Tmax, nsplit_prefix, float(scale), _s())
    return out


def attn_decode_group_prefix(q, kc_own, vc_own, kpre, vpre, rows_per_prompt, k_lo, G, prefix_len, ctx, nsplit_prefix, scale, poison=False):
    """kc_own / vc_own [B, Hkv, Tmax_own, D]: generated tokens only; kpre / vpre [B / rows_per_prompt, Hkv, cap, D]."""
    B, Hq, D = q.shape
    _, Hkv, Tmax, _ = kc_own.shape
    out = _buf(q.shape, q.dtype, q.device, poison)
    po = _buf(B * Hq * 64 * D, torch.float32, q.device, poison)
    pm = _buf(B * Hq * 64 * 2, torch.float32, q.device, poison)
    _lib.call("o3v_attn_decode_group_prefix", _p(q), _p(kc_own), _p(vc_own), _p(kpre), _p(vpre), kpre.shape[2], rows_per_prompt, _p(out),
              _p(po), _p(pm), _p(k_lo), B, G, Hq, Hkv, D, prefix_len, ctx, Tmax, nsplit_prefix, float(scale), _s())
    return out


def attn_tiles_prefix(q, k, v, kpre, vpre, p_hs, p_bs, prefix_len, rows_per_prefix, tiles, Hq, n_rep, D, q_ts, k_ts, k_hs, k_bs, v_ts,
                      v_hs, v_bs, out, o_ts, scale, rows_per_tile=64, poison=False):
    if poison:
        out.fill_(float("nan"))
    _lib.call("o3v_attn_tiles_prefix", _p(q), _p(k), _p(v), _p(kpre), _p(vpre), p_hs, p_bs, prefix_len, rows_per_prefix, _p(out),
              _p(tiles), tiles.shape[0], rows_per_tile, Hq, n_rep, D, q_ts, k_ts, k_hs, k_bs, v_ts, v_hs, v_bs, o_ts, float(scale), _s())
    return out


def gather_rows(src, idx):
    out = torch.empty((idx.shape[0], src.shape[1]), dtype=src.dtype, device=src.device)
    _lib.call("o3v_gather_rows", _p(src), _p(idx), _p(out), idx.shape[0], src.shape[1] * src.element_size(), _s())
    return out
