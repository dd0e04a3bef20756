"""CPU tests of the MXFP4 weight format (weights.quantize_rows_mxfp4 / dequantize_rows_mxfp4 / pack_mfma_fragments_mxfp4) and of the
switches that turn it on: the scale rule on hand-built blocks, the code table and nibble order, exactness of the dequantised values
in bf16, the per-block error bound, idempotence (the GPU engine tests rely on it), the fragment layouts restated lane by lane, and
the facade keywords."""
import numpy as np
import pytest
import torch

import fixture_models as fm
from open_o3_video_amd.weights import (MXFP4_GRID, DeviceWeights, dequantize_rows_mxfp4, getter_from_dict, pack_mfma_fragments_mxfp4,
                                       quantize_rows_mxfp4)

BF = torch.bfloat16


def _block(vals, fill=0.0):
    b = torch.full((32,), fill, dtype=torch.float32)
    b[: len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return b


def test_scale_rule_on_hand_built_blocks():
    """e = floor(log2(amax)) - 2 clamped to [-125, 125], an all-zero block gets e = 0, the byte is e + 127."""
    rows = torch.stack([
        torch.cat([_block([8.0, 1.0, -2.0]),                # amax exactly a power of two: e = 3 - 2 = 1, 8 / 2 = 4
                   _block([7.0, -0.1]),                      # amax in (6, 8) * 2^0: e = 0, 7 saturates at 6
                   _block([]),                               # all zero: e = 0
                   _block([2.0 ** -130, -(2.0 ** -133)])]),  # tiny (bf16 subnormals): the clamp, e = -125
        torch.cat([_block([-0.75]),                          # e = -1 - 2 = -3
                   _block([3.0e38]),                         # near the top of bf16: floor(log2) = 127, e = 125
                   _block([0.0, 0.0, 5.0]),                  # e = 0
                   _block([2.0 ** -126])])]).to(BF)          # smallest normal: e = -128 -> clamp -125
    codes, scales = quantize_rows_mxfp4(rows)
    assert codes.shape == (2, 64) and codes.dtype == torch.uint8 and scales.shape == (2, 4) and scales.dtype == torch.uint8
    assert (scales.int() - 127).tolist() == [[1, 0, 0, -125], [-3, 125, 0, -125]]
    dq = dequantize_rows_mxfp4(codes, scales)
    assert dq[0, :3].tolist() == [8.0, 1.0, -2.0]
    assert dq[0, 32:34].tolist() == [6.0, 0.0]               # (6, 8) * 2^e -> 6 * 2^e; 0.1 < 0.25 -> 0
    assert (dq[0, 64:96] == 0).all() and (codes[0, 32:48] == 0).all()
    assert (dq[0, 96:128] == 0).all()                         # 2^-130 / 2^-125 = 1/32 < 0.25 -> 0
    assert dq[1, 0].item() == -0.75
    assert dq[1, 32].item() == 6.0 * 2.0 ** 125               # 3e38 / 2^125 = 7.05: saturates
    assert dq[1, 66].item() == 4.0                            # 5 is the tie between 4 and 6: even mantissa, 4
    assert dq[1, 96].item() == 2.0 ** -126                    # 2^-126 / 2^-125 = 0.5: exact
    assert torch.isfinite(dq).all()


def test_code_table_nibble_order_and_rounding():
    """All 16 codes against a hand-written table, element 2i in the low nibble of byte i, ties to the even code."""
    table = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    assert list(MXFP4_GRID) == table[:8]
    codes = torch.arange(16, dtype=torch.uint8)
    packed = torch.zeros((1, 16), dtype=torch.uint8)
    packed[0, :8] = codes[0::2] | (codes[1::2] << 4)           # byte i: element 2i low, element 2i + 1 high
    dq = dequantize_rows_mxfp4(packed, torch.tensor([[127]], dtype=torch.uint8))
    assert dq[0, :16].tolist() == table and (dq[0, 16:] == 0).all()
    assert torch.signbit(dq[0, 8]).item()
    # quantising the table (amax 6: e = 0) gives the codes back, in the same nibbles
    q, s = quantize_rows_mxfp4(dq.to(BF))
    assert s.item() == 127 and torch.equal(q, packed)
    # every midpoint of the grid and a value on each side of it (block amax 6: e = 0)
    vals = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.2490234375, 0.251953125, 0.74609375, 0.75390625, 2.484375, 2.515625, 4.96875, 5.03125,
            -0.25, -0.75, -2.5, -5.0, 6.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 0.0, 0.5, 0.5, 1.0, 2.0, 3.0, 4.0, 6.0, -0.0, -1.0, -2.0, -4.0, 6.0]
    blk = _block(vals).to(BF)
    assert blk.float()[: len(vals)].tolist() == vals          # the probes are bf16 values
    q, s = quantize_rows_mxfp4(blk[None])
    assert dequantize_rows_mxfp4(q, s)[0, : len(vals)].tolist() == want


def _uneven(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    w[:, : K // 3] *= 4.0
    w[::7] *= 0.05
    w[1, :32] = 0
    w[2, 32:64] = 0.01
    w[2, 40] = 7.25                                           # a block holding a value in (6, 8) * 2^e
    return w.to(BF)


@pytest.mark.parametrize("N,K", [(16, 128), (48, 384), (2304, 896)])
def test_dequantised_values_exact_error_bound_idempotence(N, K):
    w = _uneven(N, K, N + K)
    codes, scales = quantize_rows_mxfp4(w)
    dq = dequantize_rows_mxfp4(codes, scales)
    assert torch.equal(dq, dq.to(BF).float())                 # exact in bf16
    assert torch.isfinite(dq).all() and ((dq == 0) | (dq.abs() >= 2.0 ** -126)).all()      # normal or zero
    e = scales.int() - 127
    assert (e >= -125).all() and (e <= 125).all()
    # |w - dq| < 2 * 2^e per block: the grid's widest spacing is 2 (4 -> 6, so rounding errs by <= 1) and saturation cuts < 2 (amax < 8)
    err = (w.float() - dq).abs().view(N, K // 32, 32).amax(dim=2)
    assert (err < 2.0 * torch.exp2(e.float())).all()
    amax = w.float().abs().view(N, K // 32, 32).amax(dim=2)
    nz = amax > 0
    assert ((amax[nz] / torch.exp2(e.float())[nz] >= 4) & (amax[nz] / torch.exp2(e.float())[nz] < 8)).all()
    assert dq[1, :32].abs().sum() == 0 and scales[1, 0] == 127
    assert dq[2, 40] == 6.0 and scales[2, 1] == 127           # 7.25 -> e = 0 -> saturated at 6
    # idempotence: the dequantised matrix quantises to the same codes and scales
    c2, s2 = quantize_rows_mxfp4(dq.to(BF))
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    # fp32 input (what DeviceWeights' getter converts) == its bf16 rounding
    c3, s3 = quantize_rows_mxfp4(dq)
    assert torch.equal(c3, codes) and torch.equal(s3, scales)


@pytest.mark.parametrize("N,K", [(16, 128), (48, 384), (2304, 896)])
def test_fragment_images_unpack_to_the_row_major_arrays(N, K):
    """The layout as the header states it, lane by lane: codes [N/16][K/128][64][16 B] with lane l of (nb, t) holding the MX block of
    row 16 nb + (l & 15), k = 128 t + 32 (l >> 4); scales [N/16][ceil(K/512)][64][4] with byte j of lane l's dword q the scale of
    step t = 4 q + j."""
    codes, scales = quantize_rows_mxfp4(_uneven(N, K, 3 * N + K))
    cp, sp = pack_mfma_fragments_mxfp4(codes, scales)
    nt, nt4 = K // 128, (K // 128 + 3) // 4
    assert cp.numel() == N * K // 2 and sp.numel() == N // 16 * nt4 * 256 and cp.dtype == sp.dtype == torch.uint8
    cpn, spn = cp.reshape(N // 16, nt, 64, 16).numpy(), sp.reshape(N // 16, nt4, 64, 4).numpy()
    nb, t, l = np.meshgrid(np.arange(N // 16), np.arange(nt), np.arange(64), indexing="ij")
    row, blk = 16 * nb + (l & 15), 4 * t + (l >> 4)            # MX block index along the row
    back_c = np.zeros((N, K // 32, 16), dtype=np.uint8)
    back_c[row, blk] = cpn[nb, t, l]
    back_s = np.zeros((N, K // 32), dtype=np.uint8)
    back_s[row, blk] = spn[nb, t >> 2, l, t & 3]
    assert np.array_equal(back_c.reshape(N, K // 2), codes.numpy())
    assert np.array_equal(back_s, scales.numpy())
    pad = np.ones((N // 16, nt4, 64, 4), dtype=bool)
    pad[nb, t >> 2, l, t & 3] = False
    assert (spn[pad] == 127).all()                             # steps past K / 128
    with pytest.raises(AssertionError):
        pack_mfma_fragments_mxfp4(codes[:, : (K - 32) // 2].contiguous(), scales[:, :-1].contiguous())   # K % 128 != 0


def test_facade_keywords():
    from open_o3_video_amd.vllm_api import decode_quantization
    assert decode_quantization("mxfp4") == dict(fp8_decode=True, mxfp4_decode=True)
    assert decode_quantization("fp8") == dict(fp8_decode=True, mxfp4_decode=False)
    assert decode_quantization(None) == dict(fp8_decode=False, mxfp4_decode=False)
    with pytest.raises(ValueError, match="int4"):
        decode_quantization("int4")
    import inspect
    from open_o3_video_amd.hf_api import Qwen2_5_VLForConditionalGeneration
    assert "mxfp4_decode" in inspect.signature(Qwen2_5_VLForConditionalGeneration.from_pretrained).parameters


def test_device_weights_build_fragment_images_only_where_the_shape_allows():
    """tied3b_config has I = 2752 = 21.5 x 128: down_proj (K = I) gets the row-major MXFP4 image and NO fragment image, gate/up
    (K = hidden) gets both; nothing fails, the fp8 images stay, and the update plan names exactly the images that exist."""
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import DecodePlan, mlp_weights_in_effect
    cfg = fm.tied3b_config()
    c = O3VConfig.from_dict(cfg)
    assert c.text.inter_pad % 32 == 0 and c.text.inter_pad % 128 != 0
    W = fm.make_weights(cfg, 4)
    dw = DeviceWeights(c, getter_from_dict(W), "cpu", mxfp4_decode=True)
    assert dw.mxfp4_decode and dw.fp8_decode                   # implied
    t, l0 = dw.t, dw.llm_layers[0]
    for k in ("l0.gu_w4", "l0.gu_w4s", "l0.gu_w4p", "l0.gu_w4ps", "l0.down_w4", "l0.down_w4s", "l0.gu_w8", "l0.down_w8", "l0.down_w8p"):
        assert k in t, k
    assert "l0.down_w4p" not in t and "l0.down_w4ps" not in t
    assert l0.gu_w4 == t["l0.gu_w4"].data_ptr() and l0.gu_s4 == t["l0.gu_w4s"].data_ptr()
    assert l0.gu_w4p == t["l0.gu_w4p"].data_ptr() and l0.gu_s4p == t["l0.gu_w4ps"].data_ptr()
    assert l0.down_w4 == t["l0.down_w4"].data_ptr() and l0.down_s4 == t["l0.down_w4s"].data_ptr()
    assert not l0.down_w4p and not l0.down_s4p
    I, H = c.text.inter_pad, c.text.hidden_size
    assert t["l0.gu_w4"].shape == (2 * I, H // 2) and t["l0.gu_w4s"].shape == (2 * I, H // 32)
    assert t["l0.down_w4"].shape == (H, I // 2) and t["l0.down_w4s"].shape == (H, I // 32)
    q, s = quantize_rows_mxfp4(t["l0.down_w"])
    assert torch.equal(q, t["l0.down_w4"]) and torch.equal(s, t["l0.down_w4s"])
    w = dw.update_plan["model.language_model.layers.0.mlp.down_proj.weight"].writes[0]
    assert (w.q4, w.q4s, w.q4frag, w.q4frags) == ("l0.down_w4", "l0.down_w4s", None, None)
    w = dw.update_plan["model.language_model.layers.0.mlp.gate_proj.weight"].writes[0]
    assert (w.q4, w.q4s, w.q4frag, w.q4frags) == ("l0.gu_w4", "l0.gu_w4s", "l0.gu_w4p", "l0.gu_w4ps")
    w = dw.update_plan["model.language_model.layers.0.self_attn.o_proj.weight"].writes[0]
    assert w.q4 is None and w.q8 == "l0.o_w8"
    # the format a call decodes on: rows at <= 3 independent rows, the fp8 fragments at 4 (no fragment image of down_proj)
    plan = lambda B, group=0: DecodePlan(B, 1, False, 64, 1, group, False)
    assert mlp_weights_in_effect(t, plan(1)) == "mxfp4" and mlp_weights_in_effect(t, plan(3)) == "mxfp4"
    assert mlp_weights_in_effect(t, plan(4)) == "fp8" and mlp_weights_in_effect(t, plan(2, group=2)) == "bf16"
    plain = DeviceWeights(c, getter_from_dict(W), "cpu", fp8_decode=True)
    assert not plain.mxfp4_decode and "l0.gu_w4" not in plain.t and not plain.llm_layers[0].gu_w4
    assert mlp_weights_in_effect(plain.t, plan(1)) == "fp8" and mlp_weights_in_effect(plain.t, plan(8)) == "fp8"
    bf = DeviceWeights(c, getter_from_dict(W), "cpu")
    assert mlp_weights_in_effect(bf.t, plan(1)) == "bf16" and mlp_weights_in_effect(bf.t, plan(8)) == "bf16"
