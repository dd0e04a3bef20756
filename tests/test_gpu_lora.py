"""LoRA adapters on the GPU: o3v_lora_merge against the torch reference (bit for bit on exact probes, a derived bound on general
values), the adapter's images against a fresh load of the merged state dict (every image, byte for byte), the engine with the adapter
on / off against fresh engines (ids and margins bit-identical, no cache crossing an adapter state) and the facades."""
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_models as fm  # noqa: E402
import fixture_models_q3 as fq  # noqa: E402
import lora_ref as lr  # noqa: E402
from test_gpu_weight_update import _assert_images_equal, _prompt, _same_bytes, _same_out  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _random_bytes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape)) * 2
    return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).view(torch.bfloat16).view(*shape)


def _run_merge(W, A, B, scale, blk0=0, stride=1, base_pad=0, out_pad=0, seed=0):
    """o3v_lora_merge on a base image that holds W the way the packed slots do (16-row blocks blk0 + i * stride, base_pad more
    columns), into a canvas of random bytes with one guard row before and after and out_pad guard columns.  Returns (merged [N, K],
    the canvas after the launch, the canvas before it)."""
    from open_o3_video_amd import _lib
    N, K = W.shape
    r = A.shape[0]
    nb = N // 16
    img = lr.probe_base(16 * nb * stride, K + base_pad, seed + 77)      # blk0 < stride: every block read lies inside
    rows = (16 * (blk0 + torch.arange(nb) * stride)[:, None] + torch.arange(16)[None, :]).reshape(-1)
    img[rows, :K] = W
    canvas0 = _random_bytes((N + 2, K + out_pad), seed + 5)
    canvas = canvas0.clone().cuda()
    base, Ad, Bd = img.cuda(), A.cuda(), B.cuda()
    out = canvas[1:]
    d = _lib.LoraDesc(base=base.data_ptr(), A=Ad.data_ptr(), B=Bd.data_ptr(), out=out.data_ptr(), base_ld=base.stride(0),
                      a_ld=Ad.stride(0), b_ld=Bd.stride(0), out_ld=canvas.stride(0),
                      ab_dtype=_lib.SRC_F32 if A.dtype == torch.float32 else _lib.SRC_BF16, N=N, K=K, r=r, base_rows=base.shape[0],
                      blk0=blk0, blk_stride=stride, scale=scale)
    _lib.call("o3v_lora_merge", C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = canvas.cpu()
    return got[1:N + 1, :K], got, canvas0


def _canaries_intact(got, before, N, K):
    return _same_bytes(got[0], before[0]) and _same_bytes(got[N + 1], before[N + 1]) and _same_bytes(got[:, K:], before[:, K:])


LAYOUTS = [dict(), dict(stride=2, blk0=0), dict(stride=2, blk0=1), dict(base_pad=24, out_pad=8), dict(stride=2, blk0=1, base_pad=8, out_pad=16)]


@pytest.mark.parametrize("N,K,r", [(16, 32, 1), (48, 80, 3), (64, 128, 16), (32, 1040, 17), (16, 64, 256)])
def test_kernel_exact_probes_bit_for_bit(need_gpu, N, K, r):
    for dtype in (torch.bfloat16, torch.float32):
        for li, lay in enumerate(LAYOUTS):
            W = lr.probe_base(N, K, seed=N + K + r + li)
            A, B = lr.probe_ab(N, K, r, seed=r + li, dtype=dtype)
            got, canvas, before = _run_merge(W, A, B, lr.PROBE_SCALE, seed=li, **lay)
            assert _same_bytes(got, lr.merge(W, A, B, lr.PROBE_SCALE)), (dtype, lay)
            assert _canaries_intact(canvas, before, N, K), (dtype, lay)


@pytest.mark.parametrize("scale", [0.0, -lr.PROBE_SCALE, -2.0])
def test_kernel_zero_and_negative_scale(need_gpu, scale):
    N, K, r = 48, 80, 3
    W = lr.probe_base(N, K, seed=3)
    A, B = lr.probe_ab(N, K, r, seed=4)
    got, canvas, before = _run_merge(W, A, B, scale, out_pad=8)
    assert _same_bytes(got, lr.merge(W, A, B, scale)) and _canaries_intact(canvas, before, N, K)
    if scale == 0.0:
        assert _same_bytes(got, W)


@pytest.mark.parametrize("N,K,r", [(64, 128, 16), (32, 1040, 64)])
def test_kernel_general_values_within_the_derived_bound(need_gpu, N, K, r):
    """|out - y| <= 0.5 ulp_bf16(y) + (r + 2) 2^-24 (|W| + |s| sum |B||A|), element-wise, no exempted share."""
    W, A, B = lr.general(N, K, r, seed=N + r)
    for scale, dtype in ((2.0, torch.bfloat16), (0.37, torch.float32)):
        got, _, _ = _run_merge(W, A.to(dtype), B.to(dtype), scale)
        y, bnd = lr.bound(W, A, B, scale)
        err = (got.double() - y).abs()
        print(f"N={N} K={K} r={r} scale={scale}: max err / bound = {(err / bnd).max().item():.4f}, differs from torch's merge in "
              f"{(got != lr.merge(W, A, B, scale)).sum().item()} of {N * K}")
        assert (err <= bnd).all()


def test_kernel_fp32_factors_are_rounded_like_a_fresh_load(need_gpu):
    """fp32 A / B that are not bf16 values: the kernel rounds them to bf16 (torch's rule) before the product."""
    N, K, r = 32, 64, 8
    W = lr.probe_base(N, K, seed=1)
    g = torch.Generator().manual_seed(2)
    A, B = torch.randint(-3, 4, (r, K), generator=g) + 2.0 ** -10, torch.randint(-3, 4, (N, r), generator=g) - 2.0 ** -10
    got, _, _ = _run_merge(W, A.float(), B.float(), lr.PROBE_SCALE)
    assert _same_bytes(got, lr.merge(W, A.float().to(torch.bfloat16), B.float().to(torch.bfloat16), lr.PROBE_SCALE))


# ------------------------------------------------------------------------------------------------ 2. the images
def _dw(cfg_dict, W, **kw):
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    return DeviceWeights(O3VConfig.from_dict(cfg_dict), getter_from_dict(W), "cuda", **kw)


def _llm_modules(cfg):
    return [f"model.language_model.layers.{i}.{m}" for i in range(cfg["text_config"]["num_hidden_layers"]) for m in lr.LLM_LINEARS]


V = "model.visual."
TOWER_25 = [V + "blocks.0.attn.qkv", V + "blocks.1.attn.proj", V + "blocks.2.mlp.gate_proj", V + "blocks.2.mlp.up_proj",
            V + "blocks.3.mlp.down_proj", V + "merger.mlp.0", V + "merger.mlp.2"]
TOWER_Q3 = [V + "blocks.0.mlp.linear_fc1", V + "blocks.1.mlp.linear_fc2", V + "merger.linear_fc1", V + "merger.linear_fc2",
            V + "deepstack_merger_list.0.linear_fc1"]
IMAGE_FIXTURES = {"tiny": (fm.tiny_config, fm.make_weights, TOWER_25), "medium": (fm.medium_config, fm.make_weights, TOWER_25),
                  "tiny_q3": (fq.tiny_q3_config, fq.make_weights, TOWER_Q3)}


def _adapter_view(dw):
    """The image set the kernels see with the adapter on."""
    return SimpleNamespace(t={**dw.t, **dw.adapter_t})


@pytest.mark.parametrize("fix", list(IMAGE_FIXTURES))
def test_adapter_images_equal_a_fresh_load_of_the_merged_weights(need_gpu, fix):
    cfg_fn, mk, tower = IMAGE_FIXTURES[fix]
    cfg = cfg_fn()
    W = mk(cfg, 0)
    kw = dict(mxfp4_decode=True)                      # with it: the fp8 and the MXFP4 images of every slot that can have them
    dw = _dw(cfg, W, **kw)
    base = {k: v.clone() for k, v in dw.t.items()}
    mods = _llm_modules(cfg) + tower
    for seed, dtype, r in ((0, torch.bfloat16, 5), (1, torch.float32, 16)):
        ad = lr.probe_adapter(W, mods, r, seed=seed, dtype=dtype)
        done = dw.load_adapter(lr.peft_names(ad, adapter_name="default"), scale=lr.PROBE_SCALE)
        assert done == {m + ".weight" for m in mods} and dw.adapter_loaded and dw.adapter_enabled
        assert set(dw.adapter_t) == set(dw.adapter_image_keys(done))
        if seed == 0:
            ptrs = {k: v.data_ptr() for k, v in dw.adapter_t.items()}
            assert any(k.endswith("4ps") for k in ptrs) and any(k.endswith("8p") for k in ptrs)
        else:
            assert {k: v.data_ptr() for k, v in dw.adapter_t.items()} == ptrs      # same targets: the images are reused
        fresh = _dw(cfg, lr.merge_state_dict(W, ad, lr.PROBE_SCALE), **kw)
        _assert_images_equal(_adapter_view(dw), fresh)
        assert not _same_bytes(dw.adapter_t["l0.qkv_w"], base["l0.qkv_w"])
        assert all(_same_bytes(dw.t[k], base[k]) for k in base)                     # the base is never written
        for k, t in dw.adapter_t.items():                                           # the descriptors point at the adapter's images
            st, field = dw._descriptor_field(k)
            assert getattr(st, field) == t.data_ptr() != dw.t[k].data_ptr(), k
    assert dw.adapter_bytes() >= sum(t.numel() * t.element_size() for t in dw.adapter_t.values())
    dw.set_adapter_enabled(False)
    for k in dw.adapter_t:
        st, field = dw._descriptor_field(k)
        assert getattr(st, field) == dw.t[k].data_ptr(), k
    keys = list(dw.adapter_t)
    dw.unload_adapter()
    assert not dw.adapter_loaded and not dw.adapter_t and dw.adapter_bytes() == 0
    assert all(_same_bytes(dw.t[k], base[k]) for k in base)
    for k in keys:
        st, field = dw._descriptor_field(k)
        assert getattr(st, field) == dw.t[k].data_ptr(), k


def test_zero_b_and_untargeted_neighbours_equal_the_base(need_gpu):
    cfg = fm.medium_config()
    W = fm.make_weights(cfg, 0)
    dw = _dw(cfg, W, mxfp4_decode=True)
    ad = lr.probe_adapter(W, _llm_modules(cfg) + TOWER_25, 8, zero_b=True)
    dw.load_adapter(lr.peft_names(ad), scale=lr.PROBE_SCALE)
    assert dw.adapter_t and all(_same_bytes(t, dw.t[k]) for k, t in dw.adapter_t.items())
    # q_proj and gate_proj only: k / v and up rows of the shared slots are the base's, in every image
    mods = ["model.language_model.layers.1.self_attn.q_proj", "model.language_model.layers.1.mlp.gate_proj"]
    ad = lr.probe_adapter(W, mods, 8, seed=3)
    dw.load_adapter(lr.peft_names(ad), scale=lr.PROBE_SCALE)
    assert set(dw.adapter_t) == {"l1.qkv_w", "l1.qkv_wp", "l1.qkv_w8", "l1.qkv_w8s", "l1.qkv_w8p", "l1.gu_w", "l1.gu_wp", "l1.gu_w8",
                                 "l1.gu_w8s", "l1.gu_w8p", "l1.gu_w4", "l1.gu_w4s", "l1.gu_w4p", "l1.gu_w4ps"}
    _assert_images_equal(_adapter_view(dw), _dw(cfg, lr.merge_state_dict(W, ad, lr.PROBE_SCALE), mxfp4_decode=True))
    nq = 7 * 128
    assert _same_bytes(dw.adapter_t["l1.qkv_w"][nq:], dw.t["l1.qkv_w"][nq:]) and not _same_bytes(dw.adapter_t["l1.qkv_w"][:nq], dw.t["l1.qkv_w"][:nq])


def test_load_weights_under_an_adapter_keeps_its_images_fresh(need_gpu):
    cfg = fm.medium_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    dw = _dw(cfg, WA, fp8_decode=True)
    mods = [m for m in _llm_modules(cfg) if not m.endswith("k_proj")] + TOWER_25[:3]
    ad = lr.probe_adapter(WA, mods, 8, seed=5)
    dw.load_adapter(lr.peft_names(ad), lora_alpha=8 * lr.PROBE_SCALE)              # alpha / r = the probe scale
    ptrs = {k: v.data_ptr() for k, v in dw.adapter_t.items()}
    # a partial push: an adapted matrix and an untargeted one that shares an adapted slot
    part = ["model.language_model.layers.0.self_attn.k_proj.weight", "model.language_model.layers.2.mlp.down_proj.weight"]
    dw.load_weights([(k, WB[k].cuda()) for k in part])
    mixed = {**WA, **{k: WB[k] for k in part}}
    _assert_images_equal(dw, _dw(cfg, mixed, fp8_decode=True))
    _assert_images_equal(_adapter_view(dw), _dw(cfg, lr.merge_state_dict(mixed, ad, lr.PROBE_SCALE), fp8_decode=True))
    dw.load_weights([(k, v.cuda()) for k, v in WB.items()])
    _assert_images_equal(dw, _dw(cfg, WB, fp8_decode=True))
    _assert_images_equal(_adapter_view(dw), _dw(cfg, lr.merge_state_dict(WB, ad, lr.PROBE_SCALE), fp8_decode=True))
    assert {k: v.data_ptr() for k, v in dw.adapter_t.items()} == ptrs and dw.adapter_enabled


# ------------------------------------------------------------------------------------------------ 3. the engine
ENGINE_SCALE = 2.0 ** -7


def _engine(cfg_dict, W, fp8=False):
    from open_o3_video_amd.engine import O3VEngine
    w = _dw(cfg_dict, W, fp8_decode=fp8)
    return O3VEngine(w.cfg, w)


RUNS = [dict(max_new_tokens=12, pad_token_id=4011),                                                                   # 1 row: the one-launch block
        dict(max_new_tokens=10, num_return_sequences=4, do_sample=True, top_p=0.95, top_k=50, temperature=1.0, seed=3),   # 4 rows
        dict(max_new_tokens=10, num_return_sequences=8, do_sample=True, top_p=0.95, top_k=50, temperature=1.0, seed=4)]   # 8 rows


@pytest.fixture(scope="module")
def medium_adapter():
    cfg = fm.medium_config()
    W = fm.make_weights(cfg, 0)
    ad = lr.probe_adapter(W, _llm_modules(cfg) + TOWER_25, 8, seed=11)
    return cfg, W, ad, lr.merge_state_dict(W, ad, ENGINE_SCALE)


@pytest.mark.parametrize("fp8", [False, True])
def test_engine_on_off_on_equals_fresh_engines(need_gpu, medium_adapter, fp8):
    cfg, W, ad, Wm = medium_adapter
    eng, base, merged = _engine(cfg, W, fp8), _engine(cfg, W, fp8), _engine(cfg, Wm, fp8)
    ids, fr = _prompt(eng, cfg)
    v0 = eng.weights_version
    eng.load_adapter(lr.peft_names(ad), scale=ENGINE_SCALE)
    assert eng.weights_version > v0 and eng.adapter_loaded and eng.adapter_enabled
    first = []
    for kw in RUNS:
        got, exp, off = eng.generate([ids], None, frames=fr, **kw), merged.generate([ids], None, frames=fr, **kw), \
            base.generate([ids], None, frames=fr, **kw)
        assert _same_out(got, exp), kw
        assert not torch.equal(exp.sequences, off.sequences), "the adapter must change the decode for the test to mean anything"
        first.append(got)
    with eng.adapter_disabled():
        assert not eng.adapter_enabled
        for kw in RUNS:
            assert _same_out(eng.generate([ids], None, frames=fr, **kw), base.generate([ids], None, frames=fr, **kw)), kw
        assert _same_bytes(eng.forward_logits([ids], None, frames=fr), base.forward_logits([ids], None, frames=fr))
    assert eng.adapter_enabled
    for kw, a in zip(RUNS, first):
        assert _same_out(eng.generate([ids], None, frames=fr, **kw), a), kw
    assert _same_bytes(eng.forward_logits([ids], None, frames=fr), merged.forward_logits([ids], None, frames=fr))
    with pytest.raises(RuntimeError, match="inside"):
        with eng.adapter_disabled():
            raise RuntimeError("inside")
    assert eng.adapter_enabled                                   # restored on an exception too
    comp = first[1].sequences[:, len(ids):]
    assert _same_bytes(eng.completion_logps([ids], comp, frames=fr), merged.completion_logps([ids], comp, frames=fr))
    with eng.adapter_disabled():
        assert _same_bytes(eng.completion_logps([ids], comp, frames=fr), base.completion_logps([ids], comp, frames=fr))
    eng.unload_adapter()
    assert not eng.adapter_loaded
    assert _same_out(eng.generate([ids], None, frames=fr, **RUNS[0]), base.generate([ids], None, frames=fr, **RUNS[0]))


def test_prefix_and_handover_are_not_reused_across_an_adapter_state(need_gpu, medium_adapter):
    cfg, W, ad, Wm = medium_adapter
    eng, base, merged = _engine(cfg, W), _engine(cfg, W), _engine(cfg, Wm)
    ids, fr = _prompt(eng, cfg)
    eng.load_adapter(lr.peft_names(ad), scale=ENGINE_SCALE)
    kw = dict(max_new_tokens=8, pad_token_id=cfg["pad_token_id"])
    eng.generate([ids], None, frames=fr, prefix_key="video", **kw)
    assert eng.generate([ids], None, frames=fr, prefix_key="video", **kw).timings["prefix_tokens_reused"] > 0
    gkw = dict(max_new_tokens=10, num_return_sequences=4, do_sample=True, top_p=0.95, top_k=50, temperature=1.0, seed=3)
    out = eng.generate([ids], None, frames=fr, **gkw)
    assert eng._last_prompt is not None
    comp = out.sequences[:, len(ids):]
    v0 = eng.weights_version
    with eng.adapter_disabled():
        assert eng.weights_version == v0 + 1 and eng._last_prompt is None and not eng._prefix
        lp = eng.completion_logps([ids], comp, frames=fr)
        assert not eng.timings_last_logps["prompt_kv_reused"]
        assert _same_bytes(lp, base.completion_logps([ids], comp, frames=fr))
        warm = eng.generate([ids], None, frames=fr, prefix_key="video", **kw)
        assert warm.timings["prefix_tokens_reused"] == 0
        assert _same_out(warm, base.generate([ids], None, frames=fr, **kw))
        eng.generate([ids], None, frames=fr, **gkw)
        memo = eng._last_prompt
        assert memo is not None and eng._prefix
    assert eng.weights_version == v0 + 2 and eng._last_prompt is None and not eng._prefix
    # a hand-over made with the adapter off is never taken with it on, even if the caller restores the memo by hand
    eng._last_prompt = memo
    lp = eng.completion_logps([ids], comp, frames=fr)
    assert not eng.timings_last_logps["prompt_kv_reused"]
    assert _same_bytes(lp, merged.completion_logps([ids], comp, frames=fr))
    warm = eng.generate([ids], None, frames=fr, prefix_key="video", **kw)
    assert warm.timings["prefix_tokens_reused"] == 0 and _same_out(warm, merged.generate([ids], None, frames=fr, **kw))


def test_qwen3_engine_with_an_adapter(need_gpu):
    cfg = fq.tiny_q3_config()
    W = fq.make_weights(cfg, 0)
    ad = lr.probe_adapter(W, _llm_modules(cfg) + TOWER_Q3, 4, seed=2)
    eng, base, merged = _engine(cfg, W), _engine(cfg, W), _engine(cfg, lr.merge_state_dict(W, ad, ENGINE_SCALE))
    px, grid = eng.pixels_from_frames(fm.make_frames(2, 64, 96, seed=4))
    eng.vit_forward(px, grid)
    assert eng._vit_plan_cache
    eng.load_adapter(lr.peft_names(ad), scale=ENGINE_SCALE)
    assert not eng._vit_plan_cache
    on = eng.vit_forward(px, grid)
    assert _same_bytes(on, merged.vit_forward(px, grid)) and not _same_bytes(on, base.vit_forward(px, grid))
    with eng.adapter_disabled():
        assert _same_bytes(eng.vit_forward(px, grid), base.vit_forward(px, grid))


# ------------------------------------------------------------------------------------------------ 4. the facades
def _write_adapter_dir(path, ad, r, alpha, **cfg_extra):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    save_file({k: v.contiguous() for k, v in lr.peft_names(ad, adapter_name=None)}, os.path.join(path, "adapter_model.safetensors"))
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none", "use_rslora": False, **cfg_extra}, f)
    return str(path)


def test_hf_facade_adapter_directory_and_disable_adapter(need_gpu, tmp_path):
    from open_o3_video_amd.hf_api import GenerationConfigLike, Qwen2_5_VLForConditionalGeneration
    cfg = fm.tiny_config()
    W = fm.make_weights(cfg, 0)
    ad = lr.probe_adapter(W, _llm_modules(cfg), 4, seed=1)
    scale = 2.0 ** -6
    path = _write_adapter_dir(tmp_path / "adapter", ad, r=4, alpha=4 * scale)
    model = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, W)
    base = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, W)
    merged = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, lr.merge_state_dict(W, ad, scale))
    g = np.load(os.path.join(GOLDEN, "g6_tiny.npz"))
    inp = dict(input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.ones_like(torch.from_numpy(g["input_ids"])),
               pixel_values=torch.from_numpy(g["pixel_values"]), image_grid_thw=torch.from_numpy(g["grid"]))
    gc = GenerationConfigLike(max_new_tokens=8, do_sample=False, num_return_sequences=1, pad_token_id=cfg["pad_token_id"], eos_token_id=None)
    assert not model.adapter_loaded
    assert model.load_adapter(path) == {m + ".weight" for m in ad} and model.adapter_loaded
    on, off = merged.generate(**inp, generation_config=gc), base.generate(**inp, generation_config=gc)
    assert not torch.equal(on, off)
    assert torch.equal(model.generate(**inp, generation_config=gc), on)
    with model.disable_adapter():
        assert torch.equal(model.generate(**inp, generation_config=gc), off)
    assert torch.equal(model.generate(**inp, generation_config=gc), on)
    model.unload_adapter()
    assert not model.adapter_loaded and torch.equal(model.generate(**inp, generation_config=gc), off)
    assert model.load_adapter(lr.peft_names(ad), scale=scale) == {m + ".weight" for m in ad}      # named tensors
    assert torch.equal(model.generate(**inp, generation_config=gc), on)
    with pytest.raises(ValueError, match="use_dora"):
        model.load_adapter(_write_adapter_dir(tmp_path / "dora", ad, r=4, alpha=1, use_dora=True))
    assert torch.equal(model.generate(**inp, generation_config=gc), on)                              # a refused load changes nothing


def test_vllm_facade_lora_request(need_gpu, tmp_path):
    from open_o3_video_amd.vllm_api import LLM, LoRARequest, SamplingParams
    from test_gpu_facades import StubTokenizer
    cfg = fm.medium_config()
    W = fm.make_weights(cfg, 0)
    ad = lr.probe_adapter(W, _llm_modules(cfg) + TOWER_25, 8, seed=11)
    path = _write_adapter_dir(tmp_path / "adapter", ad, r=8, alpha=8 * ENGINE_SCALE)
    mk = lambda w, **kw: LLM(engine=_engine(cfg, w), tokenizer=StubTokenizer(cfg), limit_mm_per_prompt={"image": 32}, max_model_len=4096, **kw)
    llm, base, merged = mk(W, enable_lora=True), mk(W), mk(lr.merge_state_dict(W, ad, ENGINE_SCALE))
    g = np.load(os.path.join(GOLDEN, "g7_medium.npz"))
    words, ids, i = [], g["input_ids"][0].tolist(), 0
    while i < len(ids):            # the prompt text with ONE <|image_pad|> per frame, as test_gpu_facades builds it
        if ids[i] == cfg["image_token_id"]:
            words.append("<|image_pad|>")
            while i < len(ids) and ids[i] == cfg["image_token_id"]:
                i += 1
            continue
        words.append({cfg["vision_start_token_id"]: "<|vision_start|>", cfg["vision_end_token_id"]: "<|vision_end|>"}.get(ids[i], f"w{ids[i]}"))
        i += 1
    req = {"prompt": " ".join(words), "multi_modal_data": {"image": torch.from_numpy(g["frames"])}}
    sp = SamplingParams(temperature=0.0, max_tokens=10, stop_token_ids=[])
    lora = LoRARequest("probe", 1, path)
    on, off = merged.generate(req, sp)[0].outputs[0].token_ids, base.generate(req, sp)[0].outputs[0].token_ids
    assert on != off
    assert llm.generate(req, sp, lora_request=lora)[0].outputs[0].token_ids == on
    hits = llm.vis_cache_hits
    assert llm.generate(req, sp, lora_request=None)[0].outputs[0].token_ids == off
    assert llm.vis_cache_hits == hits                        # the tower is adapted too: its tokens were not reused across the switch
    assert llm.generate(req, sp, lora_request=lora)[0].outputs[0].token_ids == on
    with pytest.raises(ValueError, match="LoRA is not enabled"):
        base.generate(req, sp, lora_request=lora)


def test_group_rollout_reference_is_the_base_under_an_adapter(need_gpu):
    from open_o3_video_amd import rewards, rollout
    from open_o3_video_amd.hf_api import Qwen2_5_VLForConditionalGeneration
    from test_gpu_facades import StubTokenizer
    g = np.load(os.path.join(GOLDEN, "g7_medium.npz"))
    cfg = fm.medium_config()
    W = fm.make_weights(cfg, 2)
    ad = lr.probe_adapter(W, _llm_modules(cfg), 8, seed=11)
    model = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, W)
    base = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, W)
    model.load_adapter(lr.peft_names(ad), scale=2.0 ** -9)
    gr = rollout.GroupRollout(model, [rewards.format_reward], StubTokenizer(cfg).batch_decode, eos_token_id=cfg["eos_token_id"],
                              pad_token_id=cfg["pad_token_id"], ref_model=None, num_generations=4, max_completion_length=10)
    ids = torch.from_numpy(g["input_ids"])
    pv, grid = torch.from_numpy(g["pixel_values"]), torch.from_numpy(g["grid"])
    res = gr.step(dict(input_ids=ids, attention_mask=torch.ones_like(ids), pixel_values=pv, image_grid_thw=grid),
                  {"prompt": "p", "task": "temporal-spatial free-form QA"})
    assert model.engine.adapter_enabled
    assert res.ref_per_token_logps is not res.per_token_logps
    exp = base.completion_logps(ids, torch.ones_like(ids), res.completion_ids, pv, grid)
    assert _same_bytes(res.ref_per_token_logps, exp)
    assert (res.per_token_kl != 0).any() and torch.isfinite(res.loss)
