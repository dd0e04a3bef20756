"""Checkpoint -> device weight images for libo3v_hip.so.

Packing done once at load (all bf16, resident in HBM):
  * fused q|k|v weight and bias of every LLM layer (one GEMM / GEMV instead of three);
  * gate/up fused and interleaved in 16-row groups so the SwiGLU epilogue finds gate_j and up_j in one lane
    (csrc/o3v_gemm.hip EPI_SWIGLU); intermediate width zero-padded to a multiple of 64 (ViT 3420 -> 3456);
  * Conv3d patch-embed weight flattened to [hidden, 1176] and zero-padded to K = 1216.
Zero padding adds exact zeros to fp32 sums, so results are unchanged.

Accepts HF 5.x names (model.visual.*, model.language_model.*) and the hub names of Qwen2.5-VL checkpoints
(visual.*, model.layers.*); loads a local safetensors directory (never downloads).
"""
from __future__ import annotations

import ctypes as C
import glob
import json
import math
import os
import re
from typing import Callable, Dict

import torch

from . import _lib
from .config import O3VConfig


def pack_gate_up(gate: torch.Tensor, up: torch.Tensor, ipad: int) -> torch.Tensor:
    """[I,K],[I,K] -> [2*ipad,K]: rows 32g..32g+15 = gate[16g..], rows 32g+16..32g+31 = up[16g..] (zero padded)."""
    I, K = gate.shape[0], (gate.shape[1] if gate.dim() == 2 else 1)
    g = torch.zeros((ipad,) + tuple(gate.shape[1:]), dtype=gate.dtype, device=gate.device)
    u = torch.zeros_like(g)
    g[:I] = gate
    u[:I] = up
    tail = tuple(gate.shape[1:])
    g = g.reshape((ipad // 16, 16) + tail)
    u = u.reshape((ipad // 16, 16) + tail)
    return torch.stack([g, u], dim=1).reshape((2 * ipad,) + tail).contiguous()


def pack_mfma_fragments(w: torch.Tensor) -> torch.Tensor:
    """[N,K] row-major -> MFMA-fragment-major [N/16][K/32][64 lanes][8]: lane l of the A fragment of (row block nb,
    k-step ks) holds W[nb*16 + (l & 15)][ks*32 + (l >> 4)*8 : +8], so one wave-instruction reads one contiguous KiB
    (csrc/o3v_gemm.hip gemv_mfma_kernel<PACKED>).  Requires N % 16 == 0 and K % 32 == 0."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0
    return w.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(N, K)


def pack_mfma_fragments_fp8(w8: torch.Tensor) -> torch.Tensor:
    """uint8 [N,K] (fp8 codes, row-major) -> fragment-major [N/16][K/64][64 lanes][16]: lane l of (row block nb, 64-wide double
    step t) holds W[nb*16 + (l & 15)][t*64 + (l >> 4)*16 : +16] -- the A fragments of two MFMAs, one contiguous KiB per
    wave-instruction (csrc/o3v_gemm.hip gemv_mfma_fp8_kernel).  Requires N % 16 == 0 and K % 64 == 0."""
    N, K = w8.shape
    assert N % 16 == 0 and K % 64 == 0
    return w8.view(N // 16, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(N, K)


FP8_MAX = 448.0   # largest finite OCP e4m3fn value


def quantize_rows_fp8(w: torch.Tensor):
    """[N, K] bf16 -> (uint8 [N, K] holding OCP e4m3fn codes, f32 [N] scales): per output row the scale is the smallest POWER
    OF TWO s with max|w| / s <= 448, q = rne(w / s) (torch's float8_e4m3fn conversion; no overflow); an all-zero row gets
    s = 1.  A power-of-two scale costs no precision (fp8 is floating point: it only shifts the exponent) and makes the
    dequantised weight fp8(q) * s exactly representable in bf16, so the fp8 path can be checked against the bf16 path on the
    very same weight values.  dequantize_rows_fp8 restates what the kernel multiplies."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    s = torch.exp2(torch.ceil(torch.log2(torch.clamp(amax, min=1e-30) / FP8_MAX)))
    s = torch.where(amax > 0, s, torch.ones_like(s))
    s = torch.where(amax / s > FP8_MAX, s * 2, s)          # guard the log2 rounding at exact powers of two
    q = (wf / s[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), s.contiguous()


def dequantize_rows_fp8(q8: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    return q8.view(torch.float8_e4m3fn).float() * s[:, None].float()


MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # OCP e2m1 magnitudes of codes 0..7; bit 3 of a code is the sign


def quantize_rows_mxfp4(w: torch.Tensor):
    """[N, K] bf16 -> (uint8 [N, K/2] codes, uint8 [N, K/32] scales): OCP MX v1.0 MXFP4 over blocks of 32 consecutive k of a row.
    Per block e = floor(log2(amax)) - 2 clamped to [-125, 125] (an all-zero block: e = 0), scale byte e + 127; elements are v / 2^e
    rounded to nearest even on the e2m1 grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6 (amax / 2^e lies in [4, 8): a value
    in (6, 8) * 2^e becomes 6 * 2^e); element 2i is the low nibble of byte i, bit 3 of a code the sign.  The clamp keeps every
    dequantised value a normal, finite bf16, and e2m1 * 2^e is exact in bf16, so the MXFP4 path can be checked against the bf16
    path on the very same weight values.
    Written on bit patterns and exact products so that the device quantiser (csrc/o3v_mxfp4.h) agrees bit for bit: amax is the
    largest magnitude PATTERN of the block, its exponent field gives e, |v| * 2^-e is exact.  Requires K % 32 == 0."""
    N, K = w.shape
    assert K % 32 == 0
    bits = w.to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int32).view(N, K // 32, 32) & 0xFFFF
    mag = bits & 0x7FFF
    amax = mag.amax(dim=2)
    e = torch.clamp((amax >> 7) - 129, -125, 125)          # exponent field - 127 = floor(log2) of a normal; subnormals hit the clamp
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    inv = ((127 - e) << 23).to(torch.int32).view(torch.float32)       # 2^-e
    a = (mag << 16).to(torch.int32).view(torch.float32) * inv[:, :, None]
    # thresholds = midpoints of the grid; a tie goes to the code with an even mantissa bit (0, 1, 2, 4)
    code = ((a > 0.25).to(torch.int32) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0)) | ((bits >> 12) & 8)
    code = code.view(N, K // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    return codes.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_rows_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(uint8 [N, K/2], uint8 [N, K/32]) -> f32 [N, K]: e2m1(code) * 2^(scale - 127), what the kernels multiply (exact in bf16)."""
    N = codes.shape[0]
    c = torch.stack([codes & 15, codes >> 4], dim=-1).view(N, -1).long()
    grid = torch.tensor(MXFP4_GRID + tuple(-v for v in MXFP4_GRID), dtype=torch.float32, device=codes.device)
    s = (scales.to(torch.int32) << 23).view(torch.float32)
    return (grid[c].view(N, -1, 32) * s[:, :, None]).view(N, -1)


def pack_mfma_fragments_mxfp4(codes: torch.Tensor, scales: torch.Tensor):
    """Row-major MXFP4 (codes uint8 [N, K/2], scales uint8 [N, K/32]) -> the fragment-major pair of
    csrc/o3v_mxfp4.hip gemv_mfma_mxfp4_kernel, laid out like pack_mfma_fragments_fp8:
      codes  [N/16][K/128][64 lanes][16 B]: lane l of (row block nb, 128-wide k step t) holds the MX block of row nb*16 + (l & 15),
             k = 128 t + 32 (l >> 4) .. + 32 -- a lane's 16-byte load is one block, a wave-instruction reads one contiguous KiB;
      scales [N/16][ceil(K/512)][64 lanes][4 B]: the same (row block, k step, lane) order with four consecutive k steps of a lane in
             one dword (bytes of steps past K/128 are padding: 127).
    Requires N % 16 == 0 and K % 128 == 0."""
    N, K = codes.shape[0], codes.shape[1] * 2
    assert N % 16 == 0 and K % 128 == 0 and scales.shape == (N, K // 32)
    nt = K // 128
    nt4 = (nt + 3) // 4
    cp = codes.view(N // 16, 16, nt, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(N, K // 2)
    sp = torch.full((N, nt4 * 16), 127, dtype=torch.uint8, device=scales.device)
    sp[:, : nt * 4] = scales
    sp = sp.view(N // 16, 16, nt4, 4, 4).permute(0, 2, 4, 1, 3).contiguous().view(N // 16, nt4 * 256)   # [nb][q][g][row][step in q]
    return cp, sp


def pad_cols(w: torch.Tensor, kpad: int) -> torch.Tensor:
    if w.shape[1] == kpad:
        return w.contiguous()
    out = torch.zeros((w.shape[0], kpad), dtype=w.dtype, device=w.device)
    out[:, : w.shape[1]] = w
    return out


class _RepackWrite:
    """One o3v_repack_rows launch: 16-row blocks row0 + i * stride (i < nblk) of slot `slot` and of its derived images."""

    def __init__(self, slot, row0, nblk, stride, row_map=None, col_map=None, frag=None, q8=None, q8s=None, q8frag=None, q4=None,
                 q4s=None, q4frag=None, q4frags=None):
        self.slot, self.row0, self.nblk, self.stride, self.row_map, self.col_map = slot, row0, nblk, stride, row_map, col_map
        self.frag, self.q8, self.q8s, self.q8frag = frag, q8, q8s, q8frag
        self.q4, self.q4s, self.q4frag, self.q4frags = q4, q4s, q4frag, q4frags      # MXFP4 codes / scales, row-major and fragment-major

    def apply(self, t: Dict[str, torch.Tensor], src: torch.Tensor, stream):
        if src.stride(-1) != 1 or src.data_ptr() % 16:
            src = src.contiguous()
        dst = t[self.slot]

        def ptr(key):
            return t[key].data_ptr() if key else None

        d = _lib.RepackDesc(src=src.data_ptr(), row_map=None if self.row_map is None else self.row_map.data_ptr(),
                            col_map=None if self.col_map is None else self.col_map.data_ptr(), dst=dst.data_ptr(),
                            dst_frag=ptr(self.frag), dst8=ptr(self.q8), dst8_scale=ptr(self.q8s), dst8_frag=ptr(self.q8frag),
                            src_ld=src.stride(0), src_dtype=_lib.SRC_F32 if src.dtype == torch.float32 else _lib.SRC_BF16,
                            src_rows=src.shape[0], src_cols=src.shape[1], rows=dst.shape[0], cols=dst.shape[1], blk0=self.row0,
                            nblk=self.nblk, blk_stride=self.stride, dst4=ptr(self.q4), dst4_scale=ptr(self.q4s),
                            dst4_frag=ptr(self.q4frag), dst4_frag_scale=ptr(self.q4frags))
        _lib.call("o3v_repack_rows", C.byref(d), C.c_void_p(stream.cuda_stream))

    def bytes_written(self, t) -> int:
        rows = min(16 * self.nblk, t[self.slot].shape[0] - 16 * self.row0) if self.stride == 1 else 16 * self.nblk
        cols = t[self.slot].shape[1]
        n = rows * cols * (2 * (1 + (self.frag is not None)) + (self.q8 is not None) + (self.q8frag is not None))
        n += 4 * rows if self.q8s else 0
        return n + rows * cols // 32 * (17 * (self.q4 is not None) + 17 * (self.q4frag is not None))   # 16 code bytes + 1 scale byte per block


class _VectorWrite:
    """A norm / bias vector: slot[dst] = bf16(src) (src_idx: gather, -1 = zero), an in-place device copy."""

    def __init__(self, slot, dst, src_idx=None):
        self.slot, self.dst, self.src_idx = slot, dst, src_idx

    def apply(self, t: Dict[str, torch.Tensor], src: torch.Tensor, stream):
        v = src.to(torch.bfloat16)          # _Getter's conversion
        if self.src_idx is None:
            t[self.slot][self.dst].copy_(v)
        else:
            vals = torch.where(self.src_idx >= 0, v[self.src_idx.clamp(min=0)], torch.zeros((), dtype=v.dtype, device=v.device))
            if isinstance(self.dst, slice):
                t[self.slot][self.dst].copy_(vals)
            else:
                t[self.slot].index_copy_(0, self.dst, vals)

    def bytes_written(self, t) -> int:
        return 2 * (t[self.slot][self.dst].numel() if isinstance(self.dst, slice) else self.dst.numel())


class _LoraTarget:
    """One adapted matrix: A [r, K8] and B [N16, r] as the device keeps them (zero-padded to whole 16-row blocks / 8-column chunks,
    which adds exact zeros), its scale and the plan entry whose write places the merged matrix."""

    def __init__(self, name, entry, A, B, scale):
        self.name, self.entry, self.A, self.B, self.scale = name, entry, A, B, float(scale)
        self.r = A.shape[0]


_LORA_KEY = re.compile(r"^(?:base_model\.model\.)?(?P<mod>.+)\.lora_(?P<ab>[AB])(?:\.(?P<adapter>[^.]+))?\.weight$")
# matrices the update plan could rewrite but that no LoRA linear wraps
_LORA_NOT_LINEAR = (("lm_head.weight", "lm_head"), ("embed_tokens.weight", "embed_tokens (an embedding: lora_embedding_* is not supported)"),
                    ("patch_embed.proj.weight", "the patch-embed convolution"), ("pos_embed.weight", "the position table (an embedding)"))


class UpdateEntry:
    """What load_weights does with one HF name: its expected shape (alt_shapes: other accepted views, the Conv3d patch weight)
    and the writes that put it where DeviceWeights packed it."""

    def __init__(self, name, shape, writes):
        self.name, self.shape, self.writes, self.alt_shapes = name, shape, writes, ()
        self.unsupported = None   # why o3v_repack_rows cannot rewrite this weight's layout (load_weights raises)


class _Getter:
    def __init__(self, fn: Callable[[str], torch.Tensor], device):
        self.fn, self.device = fn, device

    def __call__(self, *names):
        for n in names:
            try:
                t = self.fn(n)
            except KeyError:
                continue
            if t is not None:
                return t.to(device=self.device, dtype=torch.bfloat16)
        raise KeyError(f"weight not found under any of {names}")


class DeviceWeights:
    """Owns the packed tensors and the ctypes descriptors that point at them."""

    def __init__(self, cfg: O3VConfig, get: Callable[[str], torch.Tensor], device="cuda", batched_decode: bool = True,
                 fp8_decode: bool = False, mxfp4_decode: bool = False):
        """batched_decode: also keep MFMA-fragment-major copies of the LLM matrices (+1x their size in HBM) so that
        decoding 2..8 sequences together (group rollout) streams weights at the same rate as batch 1.
        fp8_decode: also keep fp8 (OCP e4m3fn) copies of the LLM matrices and the head with one fp32 scale per output row
        (quantize_rows_fp8); decode at batch <= 3 then streams those -- half the bytes per step (BASELINE config #5).
        mxfp4_decode: implies fp8_decode, and also keeps MXFP4 images (quantize_rows_mxfp4: e2m1 codes, one e8m0 scale per 32 k) of
        the two MLP matrices of every layer -- 85 % of a layer's bytes.  A decode on the fp8 rows then streams gate/up and down_proj
        from those; attention projections and head stay on the fp8 rows, prefill and log-prob passes never use MXFP4."""
        fp8_decode = bool(fp8_decode or mxfp4_decode)
        self.cfg = cfg
        self.device = torch.device(device)
        g = _Getter(get, self.device)
        self.t: Dict[str, torch.Tensor] = {}
        vc, tc = cfg.vision, cfg.text

        def v(name):
            return g("model.visual." + name, "visual." + name)

        def l(name):
            return g("model.language_model." + name, "model." + name, "language_model.model." + name)

        keep = self.t
        self.vit = self.vit3 = None
        if cfg.arch == "qwen3_vl":
            self._pack_vision_q3(v)
        else:
            self._pack_vision(v)
        # ---- text
        keep["l.embed"] = l("embed_tokens.weight").contiguous()
        self.llm_layers = (_lib.LlmLayerW * tc.num_hidden_layers)()
        for i in range(tc.num_hidden_layers):
            b = f"layers.{i}."
            keep[f"l{i}.ln1"] = l(b + "input_layernorm.weight").contiguous()
            keep[f"l{i}.ln2"] = l(b + "post_attention_layernorm.weight").contiguous()
            keep[f"l{i}.qkv_w"] = torch.cat([l(b + "self_attn.q_proj.weight"), l(b + "self_attn.k_proj.weight"),
                                             l(b + "self_attn.v_proj.weight")], dim=0).contiguous()
            fields = ["ln1", "ln2", "qkv_w", "o_w", "gu_w", "down_w"]
            if tc.attention_bias:
                keep[f"l{i}.qkv_b"] = torch.cat([l(b + "self_attn.q_proj.bias"), l(b + "self_attn.k_proj.bias"),
                                                 l(b + "self_attn.v_proj.bias")], dim=0).contiguous()
                fields.append("qkv_b")
            if tc.qk_norm:
                keep[f"l{i}.q_norm"] = l(b + "self_attn.q_norm.weight").contiguous()
                keep[f"l{i}.k_norm"] = l(b + "self_attn.k_norm.weight").contiguous()
                fields += ["q_norm", "k_norm"]
            keep[f"l{i}.o_w"] = l(b + "self_attn.o_proj.weight").contiguous()
            keep[f"l{i}.gu_w"] = pack_gate_up(l(b + "mlp.gate_proj.weight"), l(b + "mlp.up_proj.weight"), tc.inter_pad)
            keep[f"l{i}.down_w"] = pad_cols(l(b + "mlp.down_proj.weight"), tc.inter_pad)
            for f in fields:
                setattr(self.llm_layers[i], f, keep[f"l{i}.{f}"].data_ptr())
            for f in ("qkv_w", "o_w", "gu_w", "down_w"):
                w = keep[f"l{i}.{f}"]
                if batched_decode and w.shape[0] % 16 == 0 and w.shape[1] % 32 == 0:
                    keep[f"l{i}.{f}p"] = pack_mfma_fragments(w)
                    setattr(self.llm_layers[i], f + "p", keep[f"l{i}.{f}p"].data_ptr())
            if fp8_decode:
                for f in ("qkv_w", "o_w", "gu_w", "down_w"):
                    q8, sc = quantize_rows_fp8(keep[f"l{i}.{f}"])
                    keep[f"l{i}.{f}8"], keep[f"l{i}.{f}8s"] = q8, sc
                    setattr(self.llm_layers[i], f[:-1] + "w8", q8.data_ptr())
                    setattr(self.llm_layers[i], f[:-2] + "_s", sc.data_ptr())
                    if batched_decode and q8.shape[0] % 16 == 0 and q8.shape[1] % 64 == 0:
                        keep[f"l{i}.{f}8p"] = pack_mfma_fragments_fp8(q8)       # 4..32 decode rows (config #5's N = 16 chains)
                        setattr(self.llm_layers[i], f[:-1] + "w8p", keep[f"l{i}.{f}8p"].data_ptr())
            if mxfp4_decode:
                for f in ("gu_w", "down_w"):
                    w, n = keep[f"l{i}.{f}"], f[:-2]
                    if w.shape[1] % 32:
                        continue
                    q4, s4 = quantize_rows_mxfp4(w)
                    keep[f"l{i}.{f}4"], keep[f"l{i}.{f}4s"] = q4, s4
                    setattr(self.llm_layers[i], n + "_w4", q4.data_ptr())
                    setattr(self.llm_layers[i], n + "_s4", s4.data_ptr())
                    if batched_decode and w.shape[0] % 16 == 0 and w.shape[1] % 128 == 0:
                        keep[f"l{i}.{f}4p"], keep[f"l{i}.{f}4ps"] = pack_mfma_fragments_mxfp4(q4, s4)
                        setattr(self.llm_layers[i], n + "_w4p", keep[f"l{i}.{f}4p"].data_ptr())
                        setattr(self.llm_layers[i], n + "_s4p", keep[f"l{i}.{f}4ps"].data_ptr())
        keep["l.norm"] = l("norm.weight").contiguous()
        if tc.tie_word_embeddings:
            keep["l.head"] = keep["l.embed"]
        else:
            try:
                keep["l.head"] = g("lm_head.weight").contiguous()
            except KeyError as e:   # an incomplete shard / index or a renamed key must not silently turn into a tied head
                raise KeyError("lm_head.weight is missing from the checkpoint although tie_word_embeddings is false") from e
        head_p = 0
        if batched_decode and keep["l.head"].shape[0] % 16 == 0 and keep["l.head"].shape[1] % 32 == 0:
            keep["l.headp"] = pack_mfma_fragments(keep["l.head"])
            head_p = keep["l.headp"].data_ptr()
        self.llm = _lib.LlmDesc(hidden=tc.hidden_size, layers=tc.num_hidden_layers, heads=tc.num_attention_heads,
                                kv_heads=tc.num_key_value_heads, head_dim=tc.head_dim, inter=tc.inter_pad,
                                vocab=tc.vocab_size, rms_eps=tc.rms_norm_eps, embed=keep["l.embed"].data_ptr(),
                                layer=self.llm_layers, final_norm=keep["l.norm"].data_ptr(),
                                lm_head=keep["l.head"].data_ptr(), lm_head_p=head_p)
        self.fp8_decode = bool(fp8_decode)
        self.mxfp4_decode = bool(mxfp4_decode)
        if fp8_decode:
            keep["l.head8"], keep["l.head8s"] = quantize_rows_fp8(keep["l.head"])
            self.llm.lm_head8, self.llm.lm_head_s = keep["l.head8"].data_ptr(), keep["l.head8s"].data_ptr()
            if batched_decode and keep["l.head8"].shape[0] % 16 == 0 and keep["l.head8"].shape[1] % 64 == 0:
                keep["l.head8p"] = pack_mfma_fragments_fp8(keep["l.head8"])
                self.llm.lm_head8p = keep["l.head8p"].data_ptr()
        self._check_shapes()
        self._record_update_plan()
        # LoRA adapter (load_adapter): canonical name -> _LoraTarget, and the adapter's own copy of every image of the slots it touches
        self._adapter_targets: Dict[str, "_LoraTarget"] = {}
        self.adapter_t: Dict[str, torch.Tensor] = {}
        self._adapter_on = False

    def _pack_vision(self, v):
        """Qwen2.5-VL tower (TF:408-471)."""
        keep, vc = self.t, self.cfg.vision
        pw = v("patch_embed.proj.weight").reshape(vc.hidden_size, -1)
        keep["v.patch_w"] = pad_cols(pw, vc.patch_k_pad)
        self.vit_blocks = (_lib.VitBlockW * vc.depth)()
        for i in range(vc.depth):
            b = f"blocks.{i}."
            keep[f"v{i}.norm1"] = v(b + "norm1.weight").contiguous()
            keep[f"v{i}.norm2"] = v(b + "norm2.weight").contiguous()
            keep[f"v{i}.qkv_w"] = v(b + "attn.qkv.weight").contiguous()
            keep[f"v{i}.qkv_b"] = v(b + "attn.qkv.bias").contiguous()
            keep[f"v{i}.proj_w"] = v(b + "attn.proj.weight").contiguous()
            keep[f"v{i}.proj_b"] = v(b + "attn.proj.bias").contiguous()
            keep[f"v{i}.gu_w"] = pack_gate_up(v(b + "mlp.gate_proj.weight"), v(b + "mlp.up_proj.weight"), vc.inter_pad)
            keep[f"v{i}.gu_b"] = pack_gate_up(v(b + "mlp.gate_proj.bias"), v(b + "mlp.up_proj.bias"), vc.inter_pad)
            keep[f"v{i}.down_w"] = pad_cols(v(b + "mlp.down_proj.weight"), vc.inter_pad)
            keep[f"v{i}.down_b"] = v(b + "mlp.down_proj.bias").contiguous()
            for f in ("norm1", "norm2", "qkv_w", "qkv_b", "proj_w", "proj_b", "gu_w", "gu_b", "down_w", "down_b"):
                setattr(self.vit_blocks[i], f, keep[f"v{i}.{f}"].data_ptr())
        keep["v.ln_q"] = v("merger.ln_q.weight").contiguous()
        keep["v.m0_w"] = v("merger.mlp.0.weight").contiguous()
        keep["v.m0_b"] = v("merger.mlp.0.bias").contiguous()
        keep["v.m2_w"] = v("merger.mlp.2.weight").contiguous()
        keep["v.m2_b"] = v("merger.mlp.2.bias").contiguous()
        mask = 0
        for i in vc.fullatt_block_indexes:
            mask |= 1 << int(i)
        self.vit = _lib.VitDesc(depth=vc.depth, hidden=vc.hidden_size, heads=vc.num_heads, inter_pad=vc.inter_pad,
                                out_hidden=vc.out_hidden_size, patch_k_pad=vc.patch_k_pad, merge_unit=vc.merge_unit,
                                fullatt_mask=mask, patch_w=keep["v.patch_w"].data_ptr(), blocks=self.vit_blocks,
                                ln_q=keep["v.ln_q"].data_ptr(), m0_w=keep["v.m0_w"].data_ptr(),
                                m0_b=keep["v.m0_b"].data_ptr(), m2_w=keep["v.m2_w"].data_ptr(),
                                m2_b=keep["v.m2_b"].data_ptr())

    def _pack_vision_q3(self, v):
        """Qwen3-VL tower (TF3:606-737): LayerNorm + bias, fc1/fc2 MLP, learned position table, main + DeepStack mergers.
        Heads of head_dim 72 are stored head_dim_pad = 80 wide, each rotary half followed by its share of zero rows
        ([36 | 4 zeros | 36 | 4 zeros]): the pairs (j, j + 40) the rotation kernel couples are the model's (j, j + 36), the
        zero dims add nothing to q.k, and the matching zero columns of proj drop the padded outputs."""
        keep, vc = self.t, self.cfg.vision
        hid, heads, hd, Dp, hp, ip = vc.hidden_size, vc.num_heads, vc.head_dim, vc.head_dim_pad, vc.hidden_pad, vc.inter_pad
        dev = self.device
        half, halfp = hd // 2, Dp // 2
        j = torch.arange(Dp, device=dev)
        inner = torch.where(j < halfp, j, j - halfp)
        src_in_head = torch.where(j < halfp, inner, inner + half)
        valid = inner < half
        src = (torch.arange(heads, device=dev)[:, None] * hd + src_in_head[None, :]).reshape(-1)      # [heads*Dp]
        valid = valid[None, :].expand(heads, Dp).reshape(-1)
        src = torch.where(valid, src, torch.zeros_like(src))

        def head_rows(w):      # [heads*hd, ...] -> [heads*Dp, ...]
            out = w[src]
            out[~valid] = 0
            return out

        keep["v.patch_w"] = pad_cols(v("patch_embed.proj.weight").reshape(hid, -1), vc.patch_k_pad)
        keep["v.patch_b"] = v("patch_embed.proj.bias").contiguous()
        keep["v.pos_embed"] = v("pos_embed.weight").contiguous()
        self.vit3_blocks = (_lib.Vit3BlockW * vc.depth)()
        for i in range(vc.depth):
            b = f"blocks.{i}."
            for n in ("norm1", "norm2"):
                keep[f"v{i}.{n}_w"] = v(b + n + ".weight").contiguous()
                keep[f"v{i}.{n}_b"] = v(b + n + ".bias").contiguous()
            qw, qb = v(b + "attn.qkv.weight"), v(b + "attn.qkv.bias")
            keep[f"v{i}.qkv_w"] = pad_cols(torch.cat([head_rows(t) for t in qw.view(3, hid, hid)], dim=0), hp)
            keep[f"v{i}.qkv_b"] = torch.cat([head_rows(t) for t in qb.view(3, hid)], dim=0).contiguous()
            keep[f"v{i}.proj_w"] = head_rows(v(b + "attn.proj.weight").t().contiguous()).t().contiguous()
            keep[f"v{i}.proj_b"] = v(b + "attn.proj.bias").contiguous()
            f1 = torch.zeros((ip, hp), dtype=torch.bfloat16, device=dev)
            f1[: vc.intermediate_size, :hid] = v(b + "mlp.linear_fc1.weight")
            f1b = torch.zeros(ip, dtype=torch.bfloat16, device=dev)
            f1b[: vc.intermediate_size] = v(b + "mlp.linear_fc1.bias")
            keep[f"v{i}.fc1_w"], keep[f"v{i}.fc1_b"] = f1, f1b
            keep[f"v{i}.fc2_w"] = pad_cols(v(b + "mlp.linear_fc2.weight"), ip)
            keep[f"v{i}.fc2_b"] = v(b + "mlp.linear_fc2.bias").contiguous()
            for f in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
                setattr(self.vit3_blocks[i], f, keep[f"v{i}.{f}"].data_ptr())

        def merger(prefix, key, post):
            m = _lib.Vit3MergerW(postshuffle=int(post))
            for f, name in (("norm_w", "norm.weight"), ("norm_b", "norm.bias"), ("fc1_w", "linear_fc1.weight"),
                            ("fc1_b", "linear_fc1.bias"), ("fc2_w", "linear_fc2.weight"), ("fc2_b", "linear_fc2.bias")):
                keep[f"{key}.{f}"] = v(prefix + name).contiguous()
                setattr(m, f, keep[f"{key}.{f}"].data_ptr())
            return m

        deep_idx = [int(i) for i in vc.deepstack_visual_indexes]
        if len(deep_idx) > _lib.MAX_DEEPSTACK or sorted(set(deep_idx)) != deep_idx or any(i >= vc.depth for i in deep_idx):
            raise _lib.O3VError(f"deepstack_visual_indexes {deep_idx}: need <= {_lib.MAX_DEEPSTACK} ascending block indexes")
        self.vit3 = _lib.Vit3Desc(depth=vc.depth, hidden=hid, heads=heads, head_dim=hd, head_dim_pad=Dp, inter_pad=ip,
                                  out_hidden=vc.out_hidden_size, patch_k_pad=vc.patch_k_pad, merge_unit=vc.merge_unit,
                                  n_deep=len(deep_idx), patch_w=keep["v.patch_w"].data_ptr(), patch_b=keep["v.patch_b"].data_ptr(),
                                  blocks=self.vit3_blocks, merger=merger("merger.", "v.m", False))
        for k, idx in enumerate(deep_idx):
            self.vit3.deep_index[k] = idx
            self.vit3.deep[k] = merger(f"deepstack_merger_list.{k}.", f"v.ds{k}", True)

    def _check_shapes(self):
        vc, tc = self.cfg.vision, self.cfg.text
        q3 = self.cfg.arch == "qwen3_vl"
        if (vc.hidden_size % 64 and not q3) or tc.hidden_size % 64 or (tc.num_attention_heads * tc.head_dim) % 64:
            raise _lib.O3VError("hidden sizes must be multiples of 64 for the MFMA GEMM K loop")
        if q3 and ((vc.num_heads * vc.head_dim_pad) % 64 or (vc.hidden_size * vc.merge_unit) % 64 or vc.hidden_size % 8 or vc.head_dim % 4):
            raise _lib.O3VError("qwen3_vl vision widths: heads*pad16(head_dim) and 4*hidden must be multiples of 64")
        if vc.head_dim_pad not in (32, 64, 80, 128) or tc.head_dim not in (32, 64, 128):
            raise _lib.O3VError(f"unsupported head_dim (vision {vc.head_dim}, text {tc.head_dim})")
        if tc.num_attention_heads // tc.num_key_value_heads > 8:
            raise _lib.O3VError("GQA group size > 8 not supported by the decode attention kernel")

    # ------------------------------------------------------------------------------------ in-place update (load_weights)
    def _record_update_plan(self):
        """One UpdateEntry per accepted HF name (canonical spelling: model.language_model.* / model.visual.* / lm_head.weight):
        where the packing above put that tensor's values, restated as o3v_repack_rows launches (matrices) or in-place copies
        (vectors).  Derived images are planned exactly where the packing made them (the keys present in self.t)."""
        keep, vc, tc, dev = self.t, self.cfg.vision, self.cfg.text, self.device
        plan: Dict[str, UpdateEntry] = {}
        self.update_plan, self._update_alias = plan, {}

        def images(slot):
            return {arg: slot + sfx if slot + sfx in keep else None
                    for arg, sfx in (("frag", "p"), ("q8", "8"), ("q8s", "8s"), ("q8frag", "8p"), ("q4", "4"), ("q4s", "4s"),
                                     ("q4frag", "4p"), ("q4frags", "4ps"))}

        def mat(name, shape, slot, row0=0, stride=1, nblk=None, row_map=None, col_map=None, derived=None, llm=False, why=None):
            # a layout the kernel cannot rewrite is recorded as unsupported (load_weights refuses it); loading never fails here
            rows, cols = keep[slot].shape
            if nblk is None:
                nblk = (rows - 16 * row0 + 15) // 16 if stride == 1 else rows // 16 // stride
            if cols % 16:
                why = why or f"{slot} is {cols} columns wide (o3v_repack_rows needs a multiple of 16)"
            if llm and not (row0 * 16 + (nblk - 1) * 16 * stride + 16 <= rows and rows % 16 == 0):
                # every 16-row block of an LLM slot comes from this one source: whole fragment KiB per k-step
                why = why or f"{slot}: {rows} rows are not whole 16-row blocks of one source"
            if row_map is not None and row_map.numel() < 16 * nblk:   # the kernel reads one entry per row of every launched block
                row_map = torch.cat([row_map, row_map.new_full((16 * nblk - row_map.numel(),), -1)])
            w = _RepackWrite(slot, row0, nblk, stride, row_map, col_map, **((derived or images(slot)) if llm else {}))
            plan[name] = UpdateEntry(name, tuple(shape), [] if why else [w])
            plan[name].unsupported = why
            return plan[name]

        def vec(name, n, slot, dst=None, src_idx=None):
            plan[name] = UpdateEntry(name, (n,), [_VectorWrite(slot, slice(0, n) if dst is None else dst, src_idx)])

        def gate_up_idx(n_src, ipad, half):   # pack_gate_up on vectors: destination positions of gate (half 0) / up (half 1)
            g = torch.arange(ipad, device=dev)
            dst = (g // 16) * 32 + half * 16 + g % 16
            return dst, torch.where(g < n_src, g, torch.full_like(g, -1))

        L, V = "model.language_model.", "model.visual."
        H, D, nq, nkv, I = tc.hidden_size, tc.head_dim, tc.num_attention_heads, tc.num_key_value_heads, tc.intermediate_size
        for i in range(tc.num_hidden_layers):
            b, k = f"{L}layers.{i}.", f"l{i}."
            vec(b + "input_layernorm.weight", H, k + "ln1")
            vec(b + "post_attention_layernorm.weight", H, k + "ln2")
            off = 0
            for p, n in (("q", nq * D), ("k", nkv * D), ("v", nkv * D)):
                mat(f"{b}self_attn.{p}_proj.weight", (n, H), k + "qkv_w", row0=off // 16, nblk=max(n // 16, 1), llm=True,
                    why=None if off % 16 == 0 and n % 16 == 0 else "q / k / v rows are not whole 16-row blocks")
                if tc.attention_bias:
                    vec(f"{b}self_attn.{p}_proj.bias", n, k + "qkv_b", dst=slice(off, off + n))
                off += n
            if tc.qk_norm:
                vec(b + "self_attn.q_norm.weight", D, k + "q_norm")
                vec(b + "self_attn.k_norm.weight", D, k + "k_norm")
            mat(b + "self_attn.o_proj.weight", (H, nq * D), k + "o_w", llm=True)
            for half, p in enumerate(("gate", "up")):
                mat(f"{b}mlp.{p}_proj.weight", (I, H), k + "gu_w", row0=half, stride=2, llm=True)
            mat(b + "mlp.down_proj.weight", (H, I), k + "down_w", llm=True)
        vec(L + "norm.weight", H, "l.norm")
        head = dict(frag="l.headp" if "l.headp" in keep else None, q8="l.head8" if "l.head8" in keep else None,
                    q8s="l.head8s" if "l.head8s" in keep else None, q8frag="l.head8p" if "l.head8p" in keep else None)
        none = dict(frag=None, q8=None, q8s=None, q8frag=None)
        if tc.tie_word_embeddings:   # l.head IS l.embed: the embedding refreshes the head's derived images too
            mat(L + "embed_tokens.weight", (tc.vocab_size, H), "l.embed", derived=head, llm=True)
            self._update_alias["lm_head.weight"] = L + "embed_tokens.weight"
        else:
            mat(L + "embed_tokens.weight", (tc.vocab_size, H), "l.embed", derived=none, llm=True)
            mat("lm_head.weight", (tc.vocab_size, H), "l.head", derived=head, llm=True)

        vh, vi = vc.hidden_size, vc.intermediate_size
        pe = mat(V + "patch_embed.proj.weight", (vh, vc.patch_k), "v.patch_w")
        pe.alt_shapes = ((vh, vc.in_channels, vc.temporal_patch_size, vc.patch_size, vc.patch_size),)   # the Conv3d weight
        if self.cfg.arch == "qwen3_vl":
            self._plan_vision_q3(mat, vec)
        else:
            for i in range(vc.depth):
                b, k = f"{V}blocks.{i}.", f"v{i}."
                vec(b + "norm1.weight", vh, k + "norm1")
                vec(b + "norm2.weight", vh, k + "norm2")
                mat(b + "attn.qkv.weight", (3 * vh, vh), k + "qkv_w")
                vec(b + "attn.qkv.bias", 3 * vh, k + "qkv_b")
                mat(b + "attn.proj.weight", (vh, vh), k + "proj_w")
                vec(b + "attn.proj.bias", vh, k + "proj_b")
                for half, p in enumerate(("gate", "up")):
                    mat(f"{b}mlp.{p}_proj.weight", (vi, vh), k + "gu_w", row0=half, stride=2)
                    vec(f"{b}mlp.{p}_proj.bias", vi, k + "gu_b", *gate_up_idx(vi, vc.inter_pad, half))
                mat(b + "mlp.down_proj.weight", (vh, vi), k + "down_w")
                vec(b + "mlp.down_proj.bias", vh, k + "down_b")
            mh = vh * vc.merge_unit
            vec(V + "merger.ln_q.weight", vh, "v.ln_q")
            mat(V + "merger.mlp.0.weight", (mh, mh), "v.m0_w")
            vec(V + "merger.mlp.0.bias", mh, "v.m0_b")
            mat(V + "merger.mlp.2.weight", (vc.out_hidden_size, mh), "v.m2_w")
            vec(V + "merger.mlp.2.bias", vc.out_hidden_size, "v.m2_b")

    def _plan_vision_q3(self, mat, vec):
        """_pack_vision_q3's layout: head_rows as a row map (qkv) or a column map (proj), fc1 zero rows / columns, merger
        norms of DeepStack width."""
        vc, dev, V = self.cfg.vision, self.device, "model.visual."
        hid, heads, hd, Dp, ip = vc.hidden_size, vc.num_heads, vc.head_dim, vc.head_dim_pad, vc.inter_pad
        half, halfp = hd // 2, Dp // 2
        j = torch.arange(Dp)
        inner = torch.where(j < halfp, j, j - halfp)
        src = (torch.arange(heads)[:, None] * hd + torch.where(j < halfp, inner, inner + half)[None, :]).reshape(-1)
        head_map = torch.where((inner < half)[None, :].expand(heads, Dp).reshape(-1), src, torch.full_like(src, -1))
        qkv_map = torch.cat([torch.where(head_map >= 0, head_map + p * hid, head_map) for p in range(3)])
        qkv_map_dev = qkv_map.to(torch.int32).to(dev)
        col_map_dev = head_map.to(torch.int32).to(dev)
        vec(V + "patch_embed.proj.bias", hid, "v.patch_b")
        mat(V + "pos_embed.weight", (vc.num_position_embeddings, hid), "v.pos_embed")
        for i in range(vc.depth):
            b, k = f"{V}blocks.{i}.", f"v{i}."
            for n in ("norm1", "norm2"):
                vec(b + n + ".weight", hid, k + n + "_w")
                vec(b + n + ".bias", hid, k + n + "_b")
            mat(b + "attn.qkv.weight", (3 * hid, hid), k + "qkv_w", nblk=(qkv_map.numel() + 15) // 16, row_map=qkv_map_dev)
            vec(b + "attn.qkv.bias", 3 * hid, k + "qkv_b", slice(0, qkv_map.numel()), qkv_map.to(dev))
            mat(b + "attn.proj.weight", (hid, hid), k + "proj_w", col_map=col_map_dev)
            vec(b + "attn.proj.bias", hid, k + "proj_b")
            mat(b + "mlp.linear_fc1.weight", (vc.intermediate_size, hid), k + "fc1_w")
            vec(b + "mlp.linear_fc1.bias", vc.intermediate_size, k + "fc1_b")
            mat(b + "mlp.linear_fc2.weight", (hid, vc.intermediate_size), k + "fc2_w")
            vec(b + "mlp.linear_fc2.bias", hid, k + "fc2_b")
        mh = hid * vc.merge_unit
        for prefix, key, post in [("merger.", "v.m", False)] + [(f"deepstack_merger_list.{n}.", f"v.ds{n}", True)
                                                               for n in range(len(vc.deepstack_visual_indexes))]:
            nw = mh if post else hid
            vec(V + prefix + "norm.weight", nw, key + ".norm_w")
            vec(V + prefix + "norm.bias", nw, key + ".norm_b")
            mat(V + prefix + "linear_fc1.weight", (mh, mh), key + ".fc1_w")
            vec(V + prefix + "linear_fc1.bias", mh, key + ".fc1_b")
            mat(V + prefix + "linear_fc2.weight", (vc.out_hidden_size, mh), key + ".fc2_w")
            vec(V + prefix + "linear_fc2.bias", vc.out_hidden_size, key + ".fc2_b")

    def resolve_name(self, name: str) -> str:
        """Canonical plan name of an HF name in any spelling _Getter accepts; KeyError if the engine has no such weight."""
        if name in self.update_plan:
            return name
        if name in self._update_alias:
            return self._update_alias[name]
        for alias, canon in (("visual.", "model.visual."), ("language_model.model.", "model.language_model."),
                             ("model.", "model.language_model.")):
            if name.startswith(alias) and canon + name[len(alias):] in self.update_plan:
                return canon + name[len(alias):]
        raise KeyError(name)

    def load_weights(self, named_tensors) -> set:
        """Rewrite the packed images in place from (HF name, tensor) pairs -- vLLM's model.load_weights.  Every image a slot keeps
        (bf16 rows, fragment-major, fp8 codes + scales, fp8 fragment-major, MXFP4 codes + scales in both layouts) gets the bytes a fresh DeviceWeights load of the same
        tensors builds; data pointers do not change; rows a tensor does not own are not touched.  All pairs are validated before
        anything is written (unknown name: KeyError; wrong shape or a dtype other than bf16 / fp32: ValueError; a layout the
        kernel cannot rewrite: O3VError).  Matrices go through o3v_repack_rows, vectors (norms, biases) through in-place device
        copies, all enqueued on torch's current stream.
        Sources on this GPU are used where they are and record_stream'ed on that stream, so freeing one right after the call
        (e.g. leaving a ZeRO-3 GatheredParameters context) is safe: its memory is not reused before the queued work has read it.
        Other sources are staged to this GPU one tensor at a time (transient memory: the largest tensor); a host source's copy
        is a pageable one, so it blocks the host until that tensor has arrived.  Device sources need no host synchronisation.
        Returns the canonical names written.  Derived state outside this object (engine caches) is the caller's:
        O3VEngine.load_weights invalidates it."""
        items = []
        for name, t in named_tensors:
            key = self.resolve_name(name)
            e = self.update_plan[key]
            if not torch.is_tensor(t) or not t.is_floating_point():
                raise ValueError(f"{name}: need a floating-point tensor, got {getattr(t, 'dtype', type(t))}")
            if t.dtype not in (torch.bfloat16, torch.float32):
                raise ValueError(f"{name}: dtype {t.dtype} (bf16 or fp32 sources only)")
            if tuple(t.shape) != e.shape and tuple(t.shape) not in e.alt_shapes:
                raise ValueError(f"{name}: shape {tuple(t.shape)}, the engine expects {e.shape}")
            if e.unsupported:
                raise _lib.O3VError(f"{name}: no in-place update for this layout ({e.unsupported})")
            items.append((key, e, t.detach()))
        if self.device.type != "cuda":
            raise _lib.O3VError("load_weights rewrites the device images: it needs weights on a ROCm GPU")
        target = self.t["l.embed"].device            # the resolved device (self.device may be a bare "cuda")
        stream = torch.cuda.current_stream(target)
        done = set()
        with torch.cuda.device(target):
            for key, e, t in items:
                if t.device != target:
                    t = t.to(target)                  # staged on `stream`: one source tensor alive at a time
                else:
                    t.record_stream(stream)
                for w in e.writes:
                    w.apply(self.t, t.reshape(e.shape), stream)
                    if key not in self._adapter_targets and getattr(w, "slot", None) in self.adapter_t:
                        w.apply(self.adapter_t, t.reshape(e.shape), stream)   # an untargeted matrix of an adapted slot: the base's rows
                done.add(key)
            self._merge_adapter([k for k in self._adapter_targets if k in done], stream)   # adapter images are never stale
        return done

    # ------------------------------------------------------------------------------------ LoRA adapter (merged, switchable)
    def _validate_adapter(self, named_tensors, scale=None, lora_alpha=None, use_rslora=False):
        """peft names -> [(canonical name, plan entry, A, B, scale)], every refusal raised by name before anything is allocated."""
        pairs: Dict[str, dict] = {}
        adapters = set()
        for name, t in named_tensors:
            if "lora_magnitude_vector" in name:
                raise ValueError(f"{name}: DoRA adapters (lora_magnitude_vector) are not supported")
            if "lora_embedding_" in name:
                raise ValueError(f"{name}: LoRA on embeddings (lora_embedding_*) is not supported")
            if "modules_to_save" in name:
                raise ValueError(f"{name}: modules_to_save tensors are full weights, not an adapter: send them through load_weights")
            m = _LORA_KEY.match(name)
            if m is None:
                raise ValueError(f"{name}: not a LoRA tensor name (<module>.lora_A[.<adapter>].weight / lora_B)")
            if not torch.is_tensor(t) or t.dtype not in (torch.bfloat16, torch.float32):
                raise ValueError(f"{name}: dtype {getattr(t, 'dtype', type(t))} (bf16 or fp32 adapters only)")
            if t.dim() != 2:
                raise ValueError(f"{name}: shape {tuple(t.shape)}, a LoRA factor is a matrix")
            adapters.add(m["adapter"])
            if len(adapters) > 1:
                raise ValueError(f"{name}: tensors of several adapters ({sorted(str(a) for a in adapters)}); one adapter is resident at a time")
            slot = pairs.setdefault(m["mod"], {})
            if m["ab"] in slot:
                raise ValueError(f"{name}: lora_{m['ab']} of {m['mod']} given twice")
            slot[m["ab"]] = (name, t.detach())
        if scale is None and lora_alpha is None:
            raise ValueError("load_adapter needs scale or lora_alpha")
        out = []
        for mod, ab in pairs.items():
            if "A" not in ab or "B" not in ab:
                have = ab.get("A") or ab.get("B")
                raise ValueError(f"{have[0]}: {mod} has lora_{'A' if 'A' in ab else 'B'} without lora_{'B' if 'A' in ab else 'A'}")
            key = self.resolve_name(mod + ".weight")     # KeyError: the engine has no such module
            e = self.update_plan[key]
            for suffix, what in _LORA_NOT_LINEAR:
                if key.endswith(suffix):
                    raise ValueError(f"{mod}: no LoRA on {what}")
            if e.unsupported:
                raise ValueError(f"{mod}: no in-place update for this layout ({e.unsupported})")
            w = e.writes[0] if len(e.writes) == 1 else None
            if not isinstance(w, _RepackWrite) or len(e.shape) != 2:
                raise ValueError(f"{mod}: not a linear layer's matrix")
            if w.row_map is not None or w.col_map is not None:
                raise ValueError(f"{mod}: its rows / columns are re-ordered in the packed image (Qwen3-VL tower attention); LoRA on it is "
                                 "not supported")
            (an, A), (bn, B) = ab["A"], ab["B"]
            N, K = e.shape
            r = A.shape[0]
            if r < 1 or tuple(A.shape) != (r, K) or tuple(B.shape) != (N, r):
                raise ValueError(f"{mod}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not factor the engine's {e.shape} at one rank")
            if r > _lib.LORA_MAX_RANK:
                raise ValueError(f"{mod}: rank {r} > {_lib.LORA_MAX_RANK}")
            rows = self.t[w.slot].shape[0]
            n16 = (N + 15) // 16
            if 16 * (w.row0 + (n16 - 1) * w.stride) + 16 > rows:
                raise ValueError(f"{mod}: {w.slot} keeps {rows} rows, not whole 16-row blocks of this matrix")
            sc = float(scale) if scale is not None else float(lora_alpha) / (math.sqrt(r) if use_rslora else r)
            if not math.isfinite(sc):
                raise ValueError(f"{mod}: scale {sc}")
            out.append((key, e, A, B, sc))
        if not out:
            raise ValueError("load_adapter: no LoRA tensors given")
        return out

    def adapter_image_keys(self, target_names) -> list:
        """Keys of self.t an adapter on these plan entries owns a copy of: each touched slot and every image derived from it."""
        keys = []
        for name in target_names:
            w = self.update_plan[self.resolve_name(name)].writes[0]
            for k in (w.slot, w.frag, w.q8, w.q8s, w.q8frag, w.q4, w.q4s, w.q4frag, w.q4frags):
                if k and k not in keys:
                    keys.append(k)
        return keys

    def _descriptor_field(self, key):
        """(ctypes structure, field) the kernels read image `key` through."""
        m = re.fullmatch(r"l(\d+)\.(qkv|o|gu|down)_w(p|8|8s|8p|4|4s|4p|4ps)?", key)
        if m:
            n = m[2]
            field = {None: n + "_w", "p": n + "_wp", "8": n + "_w8", "8s": n + "_s", "8p": n + "_w8p", "4": n + "_w4", "4s": n + "_s4",
                     "4p": n + "_w4p", "4ps": n + "_s4p"}[m[3]]
            return self.llm_layers[int(m[1])], field
        m = re.fullmatch(r"v(\d+)\.(\w+_w)", key)
        if m:
            return (self.vit3_blocks if self.vit3 is not None else self.vit_blocks)[int(m[1])], m[2]
        if key in ("v.m0_w", "v.m2_w"):
            return self.vit, key[2:]
        m = re.fullmatch(r"v\.m\.(fc[12]_w)", key)
        if m:
            return self.vit3.merger, m[1]
        m = re.fullmatch(r"v\.ds(\d+)\.(fc[12]_w)", key)
        if m:
            return self.vit3.deep[int(m[1])], m[2]
        raise KeyError(key)

    @property
    def adapter_loaded(self) -> bool:
        return bool(self._adapter_targets)

    @property
    def adapter_enabled(self) -> bool:
        return self._adapter_on

    def adapter_bytes(self) -> int:
        """HBM the adapter holds: its image copies plus A and B."""
        n = sum(t.numel() * t.element_size() for t in self.adapter_t.values())
        return n + sum(x.numel() * x.element_size() for tg in self._adapter_targets.values() for x in (tg.A, tg.B))

    def load_adapter(self, named_tensors, scale=None, lora_alpha=None, use_rslora=False) -> set:
        """A peft LoRA adapter, applied MERGED next to the base: for every adapted matrix W' = bf16(W + s B A) (o3v_lora_merge: fp32
        accumulation, one rounding) is packed by that matrix's own o3v_repack_rows write into the adapter's copy of every image its
        slot keeps, and the descriptors are pointed at the copies -- every forward kernel runs unchanged and at the base's cost.
        Names: [base_model.model.]<HF module path>.lora_A[.<adapter name>].weight and lora_B; s = scale, or lora_alpha / r
        (lora_alpha / sqrt(r) with use_rslora).  Targets are the linears whose packed rows and columns keep their order (the 7 LLM
        linears, the Qwen2.5-VL tower's linears, the mergers, Qwen3-VL's fc1 / fc2); everything else is refused by name with
        ValueError before anything is allocated or written.  A load with the targets of the resident adapter reuses its images
        (stable data pointers: the trainer's per-step push); the copies start as the base's bytes, so rows of an untargeted matrix
        sharing a slot equal the base.  The base images are never written.  Leaves the adapter enabled; returns the canonical
        names adapted.  Engine caches are the caller's (O3VEngine.load_adapter)."""
        items = self._validate_adapter(named_tensors, scale, lora_alpha, use_rslora)
        if self.device.type != "cuda":
            raise _lib.O3VError("load_adapter merges on the device: it needs weights on a ROCm GPU")
        target = self.t["l.embed"].device
        stream = torch.cuda.current_stream(target)
        names = {key for key, *_ in items}
        with torch.cuda.device(target):
            if names != set(self._adapter_targets):
                self.unload_adapter()
                for k in self.adapter_image_keys(names):
                    self.adapter_t[k] = self.t[k].clone()
            self._adapter_targets = {}
            for key, e, A, B, sc in items:
                N, K = e.shape
                dt = torch.float32 if torch.float32 in (A.dtype, B.dtype) else torch.bfloat16
                if K % 8 == 0 and N % 16 == 0:      # the usual case: one private copy each, no padding
                    Ap = A.to(device=target, dtype=dt, copy=True).contiguous()
                    Bp = B.to(device=target, dtype=dt, copy=True).contiguous()
                else:
                    Ap = torch.zeros((A.shape[0], (K + 7) // 8 * 8), dtype=dt, device=target)
                    Bp = torch.zeros(((N + 15) // 16 * 16, A.shape[0]), dtype=dt, device=target)
                    Ap[:, :K].copy_(A)
                    Bp[:N].copy_(B)
                self._adapter_targets[key] = _LoraTarget(key, e, Ap, Bp, sc)
            self._merge_adapter(list(self._adapter_targets), stream)
        self.set_adapter_enabled(True)
        return names

    def _merge_adapter(self, names, stream):
        """o3v_lora_merge of each named target into one staging tensor (the largest target), then its plan entry's repack into the
        adapter images."""
        if not names:
            return
        tgs = [self._adapter_targets[n] for n in names]
        stage = torch.empty(max(tg.B.shape[0] * tg.A.shape[1] for tg in tgs), dtype=torch.bfloat16, device=tgs[0].A.device)
        for tg in tgs:
            w, (N, K) = tg.entry.writes[0], tg.entry.shape
            base = self.t[w.slot]
            n16, k8 = tg.B.shape[0], tg.A.shape[1]
            out = stage[: n16 * k8].view(n16, k8)
            d = _lib.LoraDesc(base=base.data_ptr(), A=tg.A.data_ptr(), B=tg.B.data_ptr(), out=out.data_ptr(), base_ld=base.stride(0),
                              a_ld=tg.A.stride(0), b_ld=tg.B.stride(0), out_ld=k8,
                              ab_dtype=_lib.SRC_F32 if tg.A.dtype == torch.float32 else _lib.SRC_BF16, N=n16, K=k8, r=tg.r,
                              base_rows=base.shape[0], blk0=w.row0, blk_stride=w.stride, scale=tg.scale)
            _lib.call("o3v_lora_merge", C.byref(d), C.c_void_p(stream.cuda_stream))
            w.apply(self.adapter_t, out[:N, :K], stream)

    def set_adapter_enabled(self, flag: bool):
        """Point the descriptor fields of the adapted slots at the adapter's images (True) or at the base's (False).  Host only:
        launches already queued keep the pointers they were given."""
        flag = bool(flag)
        if flag and not self._adapter_targets:
            raise ValueError("set_adapter_enabled(True): no adapter is loaded")
        src = self.adapter_t if flag else self.t
        for key in self.adapter_t:
            st, field = self._descriptor_field(key)
            setattr(st, field, src[key].data_ptr())
        self._adapter_on = flag

    def unload_adapter(self):
        """Back to the base images; the adapter's memory is released."""
        self.set_adapter_enabled(False)
        self._adapter_targets, self.adapter_t = {}, {}

    def update_bytes(self, names=None):
        """(bytes read, bytes written) of a bf16-source update of `names` (default: every plan entry)."""
        rd = wr = 0
        for name in (self.update_plan if names is None else names):
            e = self.update_plan[name]
            n = 1
            for s in e.shape:
                n *= s
            rd += 2 * n
            for w in e.writes:
                wr += w.bytes_written(self.t)
        return rd, wr

    def nbytes(self):
        seen, n = set(), 0
        for t in self.t.values():
            if t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                n += t.numel() * t.element_size()
        return n


# -------------------------------------------------------------------------------------------- sources of weights
def getter_from_dict(sd: Dict[str, torch.Tensor]):
    def get(name):
        return sd[name]
    return get


def getter_from_safetensors_dir(path: str):
    """Local HF checkpoint directory (model.safetensors or sharded + index).  Never touches the network."""
    from safetensors import safe_open

    index = os.path.join(path, "model.safetensors.index.json")
    if os.path.exists(index):
        with open(index) as f:
            wm = json.load(f)["weight_map"]
    else:
        wm = {}
        for fn in sorted(glob.glob(os.path.join(path, "*.safetensors"))):
            with safe_open(fn, framework="pt") as f:
                for k in f.keys():
                    wm[k] = os.path.basename(fn)
    if not wm:
        raise FileNotFoundError(f"no safetensors weights under {path}")
    handles = {}

    def get(name):
        fn = wm[name]  # KeyError -> next alias
        if fn not in handles:
            handles[fn] = safe_open(os.path.join(path, fn), framework="pt")
        return handles[fn].get_tensor(name)
    return get


def random_getter(cfg: O3VConfig, seed=1234, device="cuda", std=0.02, head_std=None):
    """Seeded random bf16 weights at the model's true dimensions, generated on the device (benchmarks only:
    there are no checkpoints offline; throughput does not depend on weight values)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    vc, tc = cfg.vision, cfg.text
    shapes = {}
    vh, vi = vc.hidden_size, vc.intermediate_size
    shapes["model.visual.patch_embed.proj.weight"] = (vh, vc.patch_k)
    q3 = cfg.arch == "qwen3_vl"
    mh = vh * vc.merge_unit
    if q3:
        shapes["model.visual.patch_embed.proj.bias"] = (vh,)
        shapes["model.visual.pos_embed.weight"] = (vc.num_position_embeddings, vh)
        for i in range(vc.depth):
            b = f"model.visual.blocks.{i}."
            shapes.update({b + "norm1.weight": (vh,), b + "norm1.bias": (vh,), b + "norm2.weight": (vh,), b + "norm2.bias": (vh,),
                           b + "attn.qkv.weight": (3 * vh, vh), b + "attn.qkv.bias": (3 * vh,), b + "attn.proj.weight": (vh, vh),
                           b + "attn.proj.bias": (vh,), b + "mlp.linear_fc1.weight": (vi, vh), b + "mlp.linear_fc1.bias": (vi,),
                           b + "mlp.linear_fc2.weight": (vh, vi), b + "mlp.linear_fc2.bias": (vh,)})
        for m, post in [("model.visual.merger.", False)] + [(f"model.visual.deepstack_merger_list.{k}.", True)
                                                            for k in range(len(vc.deepstack_visual_indexes))]:
            shapes.update({m + "norm.weight": (mh if post else vh,), m + "norm.bias": (mh if post else vh,),
                           m + "linear_fc1.weight": (mh, mh), m + "linear_fc1.bias": (mh,),
                           m + "linear_fc2.weight": (vc.out_hidden_size, mh), m + "linear_fc2.bias": (vc.out_hidden_size,)})
    for i in range(0 if q3 else vc.depth):
        b = f"model.visual.blocks.{i}."
        shapes.update({b + "norm1.weight": (vh,), b + "norm2.weight": (vh,), b + "attn.qkv.weight": (3 * vh, vh),
                       b + "attn.qkv.bias": (3 * vh,), b + "attn.proj.weight": (vh, vh), b + "attn.proj.bias": (vh,),
                       b + "mlp.gate_proj.weight": (vi, vh), b + "mlp.gate_proj.bias": (vi,), b + "mlp.up_proj.weight": (vi, vh),
                       b + "mlp.up_proj.bias": (vi,), b + "mlp.down_proj.weight": (vh, vi), b + "mlp.down_proj.bias": (vh,)})
    m = "model.visual.merger."
    if not q3:
        shapes.update({m + "ln_q.weight": (vh,), m + "mlp.0.weight": (mh, mh), m + "mlp.0.bias": (mh,),
                       m + "mlp.2.weight": (vc.out_hidden_size, mh), m + "mlp.2.bias": (vc.out_hidden_size,)})
    H, nh, nkv, D, I, V = (tc.hidden_size, tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim,
                           tc.intermediate_size, tc.vocab_size)
    shapes["model.language_model.embed_tokens.weight"] = (V, H)
    for i in range(tc.num_hidden_layers):
        b = f"model.language_model.layers.{i}."
        shapes.update({b + "input_layernorm.weight": (H,), b + "post_attention_layernorm.weight": (H,),
                       b + "self_attn.q_proj.weight": (nh * D, H), b + "self_attn.q_proj.bias": (nh * D,),
                       b + "self_attn.k_proj.weight": (nkv * D, H), b + "self_attn.k_proj.bias": (nkv * D,),
                       b + "self_attn.v_proj.weight": (nkv * D, H), b + "self_attn.v_proj.bias": (nkv * D,),
                       b + "self_attn.o_proj.weight": (H, nh * D), b + "mlp.gate_proj.weight": (I, H),
                       b + "mlp.up_proj.weight": (I, H), b + "mlp.down_proj.weight": (H, I)})
        if tc.qk_norm:
            shapes.update({b + "self_attn.q_norm.weight": (D,), b + "self_attn.k_norm.weight": (D,)})
    shapes["model.language_model.norm.weight"] = (H,)
    shapes["lm_head.weight"] = (V, H)

    def get(name):
        shape = shapes[name]
        if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name.endswith("layernorm.weight") \
                or name.endswith("norm.weight") or name.endswith("ln_q.weight"):
            return torch.ones(shape, device=device, dtype=torch.bfloat16)
        if name.endswith("norm1.bias") or name.endswith("norm2.bias") or name.endswith("norm.bias"):
            return torch.zeros(shape, device=device, dtype=torch.bfloat16)
        t = torch.empty(shape, device=device, dtype=torch.bfloat16)
        t.normal_(0.0, head_std if (head_std is not None and name == "lm_head.weight") else std, generator=gen)
        return t
    return get
