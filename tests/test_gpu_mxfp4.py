"""GPU tests of the opt-in MXFP4 MLP weights (csrc/o3v_mxfp4.hip, o3v_repack.hip, the engine's mlp_weights regime): the device
quantiser bit-exact against weights.quantize_rows_mxfp4, the two decode linears through the C ABI on weights whose dequantised
values are exact in bf16 (so the reference sees the very same numbers and only the summation order differs), and the engine against
the bf16-row engine on MXFP4-representable weights.  Tolerances are the project's own for "same values, other summation order"."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
import fixture_models_q3 as fq
import kernel_ops as ops
from test_gpu_kernels import _epi_ref, close_bf16, rb
from test_gpu_model import LOGIT_ATOL

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPI = {"none": ops.EPI_NONE, "swiglu": ops.EPI_SWIGLU, "res": ops.EPI_RESIDUAL}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open_o3_video_amd import _lib
    _lib.load()
    return torch.device("cuda")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _uneven_weight(N, K, seed, swiglu):
    """The generator of test_linear_decode_fp8_weights (magnitudes uneven along K and across rows) plus one all-zero block and one
    block holding a value in (6, 8) x its scale."""
    from open_o3_video_amd.weights import pack_gate_up
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    w[:, : K // 3] *= 4.0
    w[::7] *= 0.05
    w[1, :32] = 0
    w[2, 32:64] = 2.0 ** -9
    w[2, 40] = 7.25 * 2.0 ** -6      # amax 7.25 * 2^-6: e = -6, the value saturates at 6 * 2^-6
    if swiglu:
        w = pack_gate_up(w[: N // 2].contiguous(), w[N // 2:].contiguous(), N // 2)
    return w


@functools.lru_cache(maxsize=1)
def _case(N, K, swiglu):
    """One weight matrix and its images, shared by the rows of x the test runs it with."""
    from open_o3_video_amd.weights import dequantize_rows_mxfp4, pack_mfma_fragments_mxfp4, quantize_rows_mxfp4
    w = _uneven_weight(N, K, N + K, swiglu).cuda()
    q4, s4 = quantize_rows_mxfp4(w)
    wd = dequantize_rows_mxfp4(q4, s4)
    wq = wd.to(BF)
    assert torch.equal(wq.float(), wd)                         # exact in bf16
    assert (s4 == 127).any() and (wd.abs().view(N, K // 32, 32).amax(2) == 6 * torch.exp2(s4.float() - 127)).any()
    frag = pack_mfma_fragments_mxfp4(q4, s4) if N % 16 == 0 and K % 128 == 0 else (None, None)
    g = torch.Generator().manual_seed(N * 3 + K)
    bias = (0.1 * torch.randn(N, generator=g)).to(BF).cuda()
    return dict(q4=q4, s4=s4, wq=wq, q4p=frag[0], s4p=frag[1], bias=bias)


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("rows,K", [(16, 128), (37, 896), (64, 18944)])
def test_quantize_rows_mxfp4_bit_exact(dev, rows, K):
    from open_o3_video_amd import _lib
    from open_o3_video_amd.weights import quantize_rows_mxfp4
    g = torch.Generator().manual_seed(rows + K)
    x = (torch.randn(rows, K, generator=g) * torch.logspace(-3, 2, rows)[:, None]).to(BF)
    x[:, : K // 3] *= 4.0
    x[::7] *= 0.05
    x[3] = 0                                                   # all-zero blocks
    x[4, :32] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, 7.0] * 2)  # every tie
    x[5, 32:64] = 2.0 ** -9
    x[5, 40] = 7.25 * 2.0 ** -6                                # a value in (6, 8) x the scale
    x[6, :32] = 2.0 ** -131                                    # bf16 subnormals: the clamp
    x[6, 64:96] = 3.0e38                                       # the top of the range: the other clamp
    x[7, 5] = 8.0                                              # amax exactly a power of two
    x = x.cuda()
    q = torch.full((rows, K // 2), 0xAA, dtype=torch.uint8, device="cuda")
    s = torch.full((rows, K // 32), 0xAA, dtype=torch.uint8, device="cuda")
    _lib.call("o3v_quantize_rows_mxfp4", P(x), P(q), P(s), rows, K, K, _st())
    qr, sr = quantize_rows_mxfp4(x)
    assert torch.equal(s, sr) and torch.equal(q, qr)
    qc, sc = quantize_rows_mxfp4(x.cpu())                      # torch on the CPU and on the GPU agree as well
    assert torch.equal(qc, qr.cpu()) and torch.equal(sc, sr.cpu())
    wide = torch.zeros((rows, K + 64), dtype=BF, device="cuda")   # rows of a wider buffer
    wide[:, :K] = x
    q2, s2 = torch.empty_like(q), torch.empty_like(s)
    _lib.call("o3v_quantize_rows_mxfp4", P(wide), P(q2), P(s2), rows, K, K + 64, _st())
    assert torch.equal(q2, q) and torch.equal(s2, s)
    assert _lib.load().o3v_quantize_rows_mxfp4(P(x), P(q), P(s), rows, 48, K, _st()) == _lib.ERR_SHAPE


# ------------------------------------------------------------------------------------------------ M <= 3
@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("N,K,epi_name,norm", [(512, 128, "none", False), (2304, 896, "swiglu", True), (896, 1152, "res", False),
                                               (37888, 3584, "swiglu", True), (3584, 18944, "res", False)])
def test_linear_decode_mxfp4(dev, M, N, K, epi_name, norm):
    """o3v_linear_decode_mxfp4 against an fp32 matmul over weights.dequantize_rows_mxfp4 (exactly what the kernel multiplies) with the
    bf16 path's rounding points, as test_linear_decode_fp8_weights does for the fp8 rows."""
    from open_o3_video_amd import _lib
    from oracle import model_ref
    c = _case(N, K, epi_name == "swiglu")
    g = torch.Generator().manual_seed(M * 5 + N)
    x = (torch.randn(M, K, generator=g) * 2).to(BF).to(dev)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(dev)
    res = torch.randn(M, N, generator=g).to(BF).to(dev)
    epi = EPI[epi_name]
    No = N // 2 if epi == ops.EPI_SWIGLU else N
    out = torch.full((M, No), float("nan"), dtype=BF, device=dev)
    use_bias = epi != ops.EPI_SWIGLU
    _lib.call("o3v_linear_decode_mxfp4", P(x), P(nw) if norm else None, 1e-6, P(c["q4"]), P(c["s4"]), P(c["bias"]) if use_bias else None,
              P(res) if epi == ops.EPI_RESIDUAL else None, P(out), M, N, K, K, No, N, epi, _st())
    xn = model_ref.rmsnorm(x.cpu(), nw.cpu(), 1e-6).to(dev) if norm else x
    acc = xn.float() @ c["wq"].float().t()
    if epi == ops.EPI_SWIGLU:
        a3 = acc.view(M, N // 32, 2, 16)
        gate, up = rb(a3[:, :, 0].reshape(M, -1)), rb(a3[:, :, 1].reshape(M, -1))
        ref = rb(torch.nn.functional.silu(gate)) * up
    else:
        ref = _epi_ref(acc, c["bias"], res if epi == ops.EPI_RESIDUAL else None, epi)
    close_bf16(out, ref, ulps=1, atol=2e-3, frac=0.999)


def test_linear_decode_mxfp4_rejects(dev):
    from open_o3_video_amd import _lib
    lib = _lib.load()
    c = _case(512, 128, False)
    x = torch.zeros((4, 128), dtype=BF, device=dev)
    out = torch.zeros((4, 512), dtype=BF, device=dev)
    args = lambda M, K: (P(x), None, 0.0, P(c["q4"]), P(c["s4"]), None, None, P(out), M, 512, K, 128, 512, 0, ops.EPI_NONE, _st())
    assert lib.o3v_linear_decode_mxfp4(*args(4, 128)) == _lib.ERR_ARG        # 4 rows: the fragment kernel's
    assert lib.o3v_linear_decode_mxfp4(*args(1, 48)) == _lib.ERR_SHAPE       # K is not whole MX blocks
    assert lib.o3v_linear_decode_mxfp4(P(x), None, 0.0, P(c["q4"]), None, None, None, P(out), 1, 512, 128, 128, 512, 0, 0, _st()) == _lib.ERR_ARG
    assert lib.o3v_linear_decode_mxfp4(*args(1, 128)[:14], ops.EPI_RESIDUAL, _st()) == _lib.ERR_ARG     # residual without res


# ------------------------------------------------------------------------------------------------ 4 <= M <= 32
@pytest.mark.parametrize("M", [4, 8, 21, 32])
@pytest.mark.parametrize("N,K,epi_name", [(128, 128, "none"), (2304, 896, "swiglu"), (896, 1152, "res"), (37888, 3584, "swiglu"),
                                          (3584, 18944, "res")])
def test_linear_decode_mxfp4_rows(dev, M, N, K, epi_name):
    """o3v_linear_decode_mxfp4_rows (fragment-major codes + scale image, widened in registers, bf16 matrix cores) against the bf16
    kernels run on the DEQUANTISED weights, as test_linear_decode_fp8_rows does: same values, another summation order."""
    from open_o3_video_amd import _lib
    c = _case(N, K, epi_name == "swiglu")
    g = torch.Generator().manual_seed(M * 3 + N + K)
    x = (torch.randn(M, K, generator=g) * 2).to(BF).to(dev)
    res = torch.randn(M, N, generator=g).to(BF).to(dev)
    epi = EPI[epi_name]
    No = N // 2 if epi == ops.EPI_SWIGLU else N
    out = torch.full((M, No), float("nan"), dtype=BF, device=dev)
    use_bias = epi != ops.EPI_SWIGLU
    _lib.call("o3v_linear_decode_mxfp4_rows", P(x), P(c["q4p"]), P(c["s4p"]), P(c["bias"]) if use_bias else None,
              P(res) if epi == ops.EPI_RESIDUAL else None, P(out), M, N, K, K, No, N, epi, _st())
    ref = ops.gemm(x, c["wq"], c["bias"] if use_bias else None, res if epi == ops.EPI_RESIDUAL else None, epi, force="gemm")
    if epi == ops.EPI_SWIGLU:
        close_bf16(out, ref.float(), ulps=1, atol=1e-3, frac=0.998)
    else:
        close_bf16(out, ref.float(), ulps=1, atol=2e-3, frac=0.999)
    lib = _lib.load()
    assert lib.o3v_linear_decode_mxfp4_rows(P(x), P(c["q4p"]), P(c["s4p"]), None, None, P(out), 3, N, K, K, No, N, ops.EPI_NONE, _st()) == _lib.ERR_ARG
    assert lib.o3v_linear_decode_mxfp4_rows(P(x), P(c["q4p"]), P(c["s4p"]), None, None, P(out), M, N, K - 64, K, No, N, ops.EPI_NONE, _st()) == _lib.ERR_SHAPE


# ------------------------------------------------------------------------------------------------ engine
def _representable(W):
    """MLP matrices -> their MXFP4-dequantised values, attention projections and head -> their fp8-dequantised values: all exact in
    bf16, so the bf16-row engine and the mxfp4 engine multiply the same numbers (quantising them again changes nothing)."""
    from open_o3_video_amd.weights import dequantize_rows_fp8, dequantize_rows_mxfp4, quantize_rows_fp8, quantize_rows_mxfp4
    W = dict(W)
    for k in list(W):
        if k.startswith("model.language_model.layers.") and ".mlp." in k and k.endswith("_proj.weight"):
            W[k] = dequantize_rows_mxfp4(*quantize_rows_mxfp4(W[k].to(BF)))
            assert torch.equal(W[k], W[k].to(BF).float())
        elif k.startswith("model.language_model.layers.") and k.endswith("_proj.weight") or k == "lm_head.weight":
            W[k] = dequantize_rows_fp8(*quantize_rows_fp8(W[k].to(BF)))
    return W


def _pair(cfg, W, **kw):
    """(engine A on bf16 rows, engine B with mxfp4_decode=True) over the same weights"""
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    c = O3VConfig.from_dict(cfg)
    return (O3VEngine(c, DeviceWeights(c, getter_from_dict(W), "cuda", **kw)),
            O3VEngine(c, DeviceWeights(c, getter_from_dict(W), "cuda", mxfp4_decode=True)))


def _follows(a, b, row, n_new, what):
    """B's greedy ids follow A's until a step where A's margin is < 2 LOGIT_ATOL; margins over the common prefix differ by < LOGIT_ATOL
    (the rules of test_fp8_decode_weights_engine / test_fp8_rows_batched_decode_engine)."""
    ra, rb_ = a.sequences[row, -n_new:].tolist(), b.sequences[row, -n_new:].tolist()
    m = a.margins[row].tolist()
    k = 0
    while k < n_new and ra[k] == rb_[k]:
        k += 1
    d = (a.margins[row, :k] - b.margins[row, :k]).abs().max().item() if k else 0.0
    print(f"{what}: follows the bf16 rows for {k}/{n_new} tokens; margins differ by {d:.4f} over them; A's margins {np.round(m, 3).tolist()}")
    assert k == n_new or m[k] < 2 * LOGIT_ATOL, (what, k, m[k])
    assert d < LOGIT_ATOL, (what, d)


@pytest.fixture(scope="module")
def medium(dev):
    cfg = fm.medium_config()
    W = _representable(fm.make_weights(cfg, 6))
    a, b = _pair(cfg, W)
    frames = fm.make_frames(2, 112, 140, seed=3)
    _, grid = a.pixels_from_frames(frames)
    ids = np.asarray([fm.make_prompt(cfg, [tuple(g) for g in grid.tolist()], seed=3)])
    return dict(cfg=cfg, W=W, a=a, b=b, frames=frames, ids=ids)


def test_engine_descriptors_carry_the_images(medium):
    b, a = medium["b"], medium["a"]
    assert b.w.mxfp4_decode and b.w.fp8_decode and not a.w.mxfp4_decode
    for i in range(b.cfg.text.num_hidden_layers):
        l = b.w.llm.layer[i]
        assert l.gu_w4 and l.down_w4 and l.gu_s4 and l.down_s4 and l.gu_w4p and l.down_w4p and l.gu_s4p and l.down_s4p
        assert l.gu_w8 and l.down_w8 and l.gu_w8p               # the fp8 images of the MLP stay (W8A8 prefill, fall-back)
    l = a.w.llm.layer[0]
    assert not l.gu_w4 and not l.down_w4p


@pytest.mark.parametrize("G", [1, 4, 8, 19])
def test_engine_mxfp4_follows_the_bf16_rows(medium, G):
    n_new = 12 if G == 1 else 10
    kw = dict(frames=medium["frames"], max_new_tokens=n_new, pad_token_id=medium["cfg"]["pad_token_id"])
    if G > 1:
        kw["num_return_sequences"] = G
    a = medium["a"].generate(medium["ids"], None, **kw)
    b = medium["b"].generate(medium["ids"], None, **kw)
    assert a.timings["mlp_weights"] == "bf16" and b.timings["mlp_weights"] == "mxfp4"
    _follows(a, b, G - 1, n_new, f"medium fixture, {G} decode rows")
    # the switch changes the decode only: prefill and the log-prob pass never read MXFP4
    if G == 1:
        la = medium["a"].forward_logits(medium["ids"], None, frames=medium["frames"])
        lb = medium["b"].forward_logits(medium["ids"], None, frames=medium["frames"])
        assert torch.equal(la, lb)


def test_engine_streams_the_images_its_regime_names(medium):
    """What a call reports is what it reads: zeroing the row-major MXFP4 codes of one down_proj changes the 1-row decode and leaves the
    4-row decode alone, zeroing its fragment image does the opposite, and neither touches the prefill (forward_logits)."""
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    c = O3VConfig.from_dict(medium["cfg"])
    eng = O3VEngine(c, DeviceWeights(c, getter_from_dict(medium["W"]), "cuda", mxfp4_decode=True))
    kw = dict(frames=medium["frames"], max_new_tokens=6, pad_token_id=medium["cfg"]["pad_token_id"])
    run = lambda G: eng.generate(medium["ids"], None, num_return_sequences=G, **kw)
    one, four, lg = run(1), run(4), eng.forward_logits(medium["ids"], None, frames=medium["frames"])
    eng.w.t["l1.down_w4"].zero_()
    one_z, four_z = run(1), run(4)
    assert not torch.equal(one_z.margins, one.margins)
    assert torch.equal(four_z.sequences, four.sequences) and torch.equal(four_z.margins, four.margins)
    eng.w.t["l1.down_w4p"].zero_()
    assert not torch.equal(run(4).margins, four.margins)
    assert torch.equal(eng.forward_logits(medium["ids"], None, frames=medium["frames"]), lg)


def test_fallback_without_a_fragment_image_is_the_fp8_call(dev, golden_dir):
    """tied3b_config: I = 2752 is no multiple of 128, so down_proj has no MXFP4 fragment image: at 4 rows the MLP stays on the fp8
    fragments -- the call reports "fp8" and is the fp8_decode=True engine's call, id for id; at one row the row-major images serve."""
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    g = np.load(os.path.join(golden_dir, "g11_tied3b.npz"))
    cfg = fm.tied3b_config()
    W = fm.make_weights(cfg, 4)
    c = O3VConfig.from_dict(cfg)
    e8 = O3VEngine(c, DeviceWeights(c, getter_from_dict(W), "cuda", fp8_decode=True))
    e4 = O3VEngine(c, DeviceWeights(c, getter_from_dict(W), "cuda", mxfp4_decode=True))
    l0 = e4.w.llm.layer[0]
    assert l0.gu_w4p and l0.down_w4 and not l0.down_w4p
    kw = dict(pixel_values=torch.from_numpy(g["pixel_values"]), image_grid_thw=g["grid"], max_new_tokens=10, pad_token_id=cfg["pad_token_id"])
    a = e8.generate(g["input_ids"], None, num_return_sequences=4, **kw)
    b = e4.generate(g["input_ids"], None, num_return_sequences=4, **kw)
    assert a.timings["mlp_weights"] == "fp8" and b.timings["mlp_weights"] == "fp8"
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.margins, b.margins)
    one = e4.generate(g["input_ids"], None, **kw)
    assert one.timings["mlp_weights"] == "mxfp4" and one.timings["fused_attention_layers"] > 0   # the one-launch block keeps running


def test_engine_mxfp4_qwen3vl(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "g12_q3_tiny.npz"))
    cfg = fq.tiny_q3_config()
    a, b = _pair(cfg, _representable(fq.make_weights(cfg, 0)))
    assert b.cfg.arch == "qwen3_vl" and b.w.llm.layer[0].gu_w4 and b.w.llm.layer[0].q_norm
    kw = dict(pixel_values=torch.from_numpy(g["pixel_values"]), image_grid_thw=g["grid"], max_new_tokens=10, pad_token_id=cfg["pad_token_id"])
    oa, ob = a.generate(g["input_ids"], None, **kw), b.generate(g["input_ids"], None, **kw)
    assert ob.timings["mlp_weights"] == "mxfp4"
    _follows(oa, ob, 0, 10, "Qwen3-VL tiny fixture, 1 row")


def test_engine_mxfp4_with_fp8_kv_cache(medium):
    """kv_cache_dtype="fp8" at 4 independent rows on both engines: the K/V format is the same, the MLP weights' is not."""
    from test_gpu_kv8 import batch, run
    args, kw, _ = batch(medium["cfg"], medium["a"], 4)
    a, _ = run(medium["a"], args, kw, "fp8", max_new_tokens=10)
    b, _ = run(medium["b"], args, kw, "fp8", max_new_tokens=10)
    assert a.timings["kv_cache_dtype"] == b.timings["kv_cache_dtype"] == "fp8"
    assert a.timings["mlp_weights"] == "bf16" and b.timings["mlp_weights"] == "mxfp4"
    for row in range(4):
        _follows(a, b, row, 10, f"fp8 K/V, row {row}")


def test_load_weights_keeps_every_mxfp4_image_current(dev):
    """After load_weights with new tensors (bf16 and fp32 sources) every image -- the MXFP4 codes, scales and both fragment images
    among them -- is byte-equal to a fresh DeviceWeights load of those tensors, and generate equals the fresh engine's."""
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    cfg = fm.medium_config()
    c = O3VConfig.from_dict(cfg)
    WA, WB = fm.make_weights(cfg, 6), fm.make_weights(cfg, 7)
    k0 = "model.language_model.layers.0.mlp.down_proj.weight"
    WB[k0] = WB[k0].clone()
    WB[k0][1, :32] = 0                                          # an all-zero block
    WB[k0][2, 32:64] = 0.01
    WB[k0][2, 40] = 7.25                                        # a value in (6, 8) x the scale: saturates
    eng = O3VEngine(c, DeviceWeights(c, getter_from_dict(WA), "cuda", mxfp4_decode=True))
    fresh = O3VEngine(c, DeviceWeights(c, getter_from_dict(WB), "cuda", mxfp4_decode=True))
    ptrs = {k: v.data_ptr() for k, v in eng.w.t.items()}
    names = [n for n in eng.w.update_plan if n.startswith("model.language_model.") or n == "lm_head.weight"]
    eng.load_weights([(n, WB[n].to(BF) if i % 2 else WB[n].float()) for i, n in enumerate(names)])
    torch.cuda.synchronize()
    assert set(eng.w.t) == set(fresh.w.t) and all(eng.w.t[k].data_ptr() == p for k, p in ptrs.items())
    mx = [k for k in fresh.w.t if k.endswith(("4", "4s", "4p", "4ps"))]
    assert len(mx) == 8 * c.text.num_hidden_layers
    for k in fresh.w.t:
        if k.startswith("l"):
            assert torch.equal(eng.w.t[k].view(torch.uint8), fresh.w.t[k].view(torch.uint8)), k
    eng.load_weights([(n, WB[n]) for n in eng.w.update_plan if n.startswith("model.visual.")])
    frames = fm.make_frames(2, 56, 84, seed=5)
    _, grid = eng.pixels_from_frames(frames)
    ids = np.asarray([fm.make_prompt(cfg, [tuple(r) for r in grid.tolist()], seed=5)])
    for G in (1, 4):
        kw = dict(frames=frames, max_new_tokens=8, pad_token_id=cfg["pad_token_id"], num_return_sequences=G)
        x, y = eng.generate(ids, None, **kw), fresh.generate(ids, None, **kw)
        assert x.timings["mlp_weights"] == "mxfp4"
        assert torch.equal(x.sequences, y.sequences) and torch.equal(x.margins, y.margins)


def test_repack_rows_mxfp4_images_with_canary_rows(dev):
    """o3v_repack_rows on the gate/up interleave (row blocks 1, 3, 5 of a slot): the MXFP4 images of the written blocks equal the
    torch packers', every other byte of every image -- the padding bytes of the fragment scale image among them -- keeps its value."""
    from open_o3_video_amd.weights import _RepackWrite, pack_mfma_fragments_mxfp4, quantize_rows_mxfp4
    rows, cols = 96, 384                                        # K / 128 = 3: one padding byte per lane of the scale image
    g = torch.Generator().manual_seed(9)
    rnd = lambda shape, dt: torch.randint(0, 256, (int(np.prod(shape)) * torch.tensor([], dtype=dt).element_size(),), generator=g,
                                          dtype=torch.uint8).view(dt).view(*shape)
    t = {"s": rnd((rows, cols), BF), "s4": rnd((rows, cols // 2), torch.uint8), "s4s": rnd((rows, cols // 32), torch.uint8),
         "s4p": rnd((rows, cols // 2), torch.uint8), "s4ps": rnd((rows // 16, 256), torch.uint8)}
    src = (torch.randn((40, cols), generator=g) * 0.05).to(BF)  # 40 source rows: the third block is half zero rows
    src[0, :32] = 0
    src[1, 40] = 7.25
    dev_t = {k: v.cuda() for k, v in t.items()}
    w = _RepackWrite("s", 1, 3, 2, q4="s4", q4s="s4s", q4frag="s4p", q4frags="s4ps")
    w.apply(dev_t, src.cuda(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    want = t["s"].clone()
    full = torch.zeros((48, cols), dtype=BF)
    full[:40] = src
    for i in range(3):
        want[16 * (1 + 2 * i): 16 * (2 + 2 * i)] = full[16 * i: 16 * i + 16]
    assert torch.equal(dev_t["s"].cpu().view(torch.int16), want.view(torch.int16))
    q, s = quantize_rows_mxfp4(want)
    qp, sp = pack_mfma_fragments_mxfp4(q, s)
    written = torch.zeros(rows, dtype=torch.bool)
    for i in range(3):
        written[16 * (1 + 2 * i): 16 * (2 + 2 * i)] = True
    got = {k: v.cpu() for k, v in dev_t.items()}
    assert torch.equal(got["s4"][written], q[written]) and torch.equal(got["s4"][~written], t["s4"][~written])
    assert torch.equal(got["s4s"][written], s[written]) and torch.equal(got["s4s"][~written], t["s4s"][~written])
    wb = written.view(rows // 16, 16)[:, 0]
    gp, tp = got["s4p"].view(rows // 16, -1), t["s4p"].view(rows // 16, -1)
    assert torch.equal(gp[wb], qp.view(rows // 16, -1)[wb]) and torch.equal(gp[~wb], tp[~wb])
    gs, ts_, ws = got["s4ps"].view(rows // 16, 64, 4), t["s4ps"].view(rows // 16, 64, 4), sp.view(rows // 16, 64, 4)
    assert torch.equal(gs[wb][:, :, :3], ws[wb][:, :, :3]) and torch.equal(gs[wb][:, :, 3], ts_[wb][:, :, 3])   # byte 3: step 3 of 3, padding
    assert torch.equal(gs[~wb], ts_[~wb])


# ------------------------------------------------------------------------------------------------ facade
def test_llm_facade_quantization_mxfp4(dev, tmp_path):
    from safetensors.torch import save_file
    from open_o3_video_amd.vllm_api import LLM, SamplingParams
    from test_gpu_facades import StubTokenizer
    cfg = fm.tiny_config()
    W = fm.make_weights(cfg, 0)
    flat = dict(cfg["text_config"], **{k: v for k, v in cfg.items() if k != "text_config"})
    flat["rope_scaling"] = {"type": "mrope", "mrope_section": flat.pop("mrope_section")}
    (tmp_path / "config.json").write_text(json.dumps(flat))
    save_file({k: v.to(BF).contiguous() for k, v in W.items()}, str(tmp_path / "model.safetensors"))
    llm = LLM(model=str(tmp_path), tokenizer=StubTokenizer(cfg), quantization="mxfp4", fp8_prefill=True)
    w = llm.engine.w
    assert w.mxfp4_decode and w.fp8_decode and w.llm.layer[0].gu_w4 and w.llm.lm_head8 and llm.engine.fp8_prefill
    with pytest.raises(ValueError, match="int4"):
        LLM(model=str(tmp_path), tokenizer=StubTokenizer(cfg), quantization="int4")
    prompt = [15, 16, 17, 18, 19, 20, 21]
    out = llm.generate([{"prompt": " ".join(f"w{t}" for t in prompt)}], SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    ref = llm.engine.generate([prompt], None, max_new_tokens=6, pad_token_id=cfg["pad_token_id"])
    assert ref.timings["mlp_weights"] == "mxfp4"             # the format the call decoded on
    assert out[0].outputs[0].token_ids == ref.sequences[0, len(prompt):].tolist()
    from open_o3_video_amd.hf_api import Qwen2_5_VLForConditionalGeneration
    model = Qwen2_5_VLForConditionalGeneration.from_pretrained(str(tmp_path), torch_dtype=torch.bfloat16, mxfp4_decode=True)
    assert model.engine.w.mxfp4_decode and model.engine.w.llm.layer[0].down_w4
