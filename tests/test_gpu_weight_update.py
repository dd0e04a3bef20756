"""In-place weight update on the GPU: o3v_repack_rows against the torch packers byte for byte, a full A -> B update of every fixture
model against a fresh load of B (same bytes in every image, same data pointers), the engine and the facades after an update
(greedy ids and margins bit-identical to a fresh B engine, no stale prefix K/V, hand-over, visual tokens or Qwen3-VL position
table), a partial update, and stream order (generate, load_weights, generate with no host synchronisation in between)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_models as fm  # noqa: E402
import fixture_models_q3 as fq  # noqa: E402
from test_weight_update_cpu import _repack_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dw(cfg_dict, W, fp8=False):
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    c = O3VConfig.from_dict(cfg_dict)
    return DeviceWeights(c, getter_from_dict(W), "cuda", fp8_decode=fp8)


def _engine(cfg_dict, W, fp8=False):
    from open_o3_video_amd.engine import O3VEngine
    w = _dw(cfg_dict, W, fp8)
    return O3VEngine(w.cfg, w)


def _same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _assert_images_equal(dw, fresh):
    assert set(dw.t) == set(fresh.t)
    bad = [k for k in fresh.t if not _same_bytes(dw.t[k], fresh.t[k])]
    assert not bad, bad[:8]


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _run_write(w, slot_tensors, src):
    """Run `w` on the GPU and on the CPU (torch packers) from the same starting images; return both image dicts."""
    from open_o3_video_amd.weights import _RepackWrite
    dev = {k: v.cuda() for k, v in slot_tensors.items()}
    ref = {k: v.clone() for k, v in slot_tensors.items()}
    gw = _RepackWrite(w.slot, w.row0, w.nblk, w.stride,
                      None if w.row_map is None else w.row_map.cuda(), None if w.col_map is None else w.col_map.cuda(),
                      w.frag, w.q8, w.q8s, w.q8frag)
    gw.apply(dev, src.cuda(), torch.cuda.current_stream())
    _repack_ref(w, ref, src)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev.items()}, ref


def _canvas(rows, cols, fp8, frag, seed):
    """Slot images filled with random bytes: whatever the kernel does not write keeps them (canary rows)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(shape, dtype):
        n = int(np.prod(shape)) * torch.tensor([], dtype=dtype).element_size()
        return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).view(dtype).view(*shape)
    t = {"s": rnd((rows, cols), torch.bfloat16)}
    if frag:
        t["sp"] = rnd((rows, cols), torch.bfloat16)
    if fp8:
        t["s8"], t["s8s"] = rnd((rows, cols), torch.uint8), rnd((rows,), torch.float32)
        if frag:
            t["s8p"] = rnd((rows, cols), torch.uint8)
    return t


def _write(t, **kw):
    from open_o3_video_amd.weights import _RepackWrite
    return _RepackWrite("s", frag="sp" if "sp" in t else None, q8="s8" if "s8" in t else None, q8s="s8s" if "s8s" in t else None,
                        q8frag="s8p" if "s8p" in t else None, **kw)


def _check(gpu, ref):
    for k in ref:
        assert _same_bytes(gpu[k], ref[k]), k


def _fp8_edge_rows(src):
    """zero rows, rows whose amax is exactly 448 * 2^k, and rows whose values land on fp8 subnormals after scaling"""
    src[0] = 0
    src[1, 5] = 448.0 * 2.0 ** -6
    src[2, :] = src[2, :].clamp(-1, 1)
    src[2, 0] = 448.0 * 2.0 ** 3
    src[3, :] = torch.linspace(-2.0 ** -9, 2.0 ** -9, src.shape[1])       # with amax 1.0: codes down in the subnormal range
    src[3, 0] = 1.0
    src[4, :] = 0
    src[4, 3] = -448.0
    return src


@pytest.mark.parametrize("src_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,cols,src_rows", [(64, 128, 64), (96, 320, 80), (48, 1024, 48)])
def test_kernel_identity_rows_all_images(need_gpu, src_dtype, rows, cols, src_rows):
    g = torch.Generator().manual_seed(rows + cols)
    src = _fp8_edge_rows(torch.randn((src_rows, cols), generator=g) * 0.05).to(src_dtype)
    t = _canvas(rows, cols, fp8=True, frag=True, seed=1)
    # blocks 1.. of the slot: block 0 is a canary in every image
    w = _write(t, row0=1, nblk=rows // 16 - 1, stride=1)
    gpu, ref = _run_write(w, t, src)
    _check(gpu, ref)
    assert _same_bytes(gpu["s"][:16], t["s"][:16]) and _same_bytes(gpu["s8s"][:16], t["s8s"][:16])


@pytest.mark.parametrize("Ksrc", [180, 179])   # row pitch 8-byte aligned (bf16) / not even 4-byte aligned: the narrower load paths
@pytest.mark.parametrize("src_dtype", [torch.bfloat16, torch.float32])
def test_kernel_gate_up_interleave_and_column_padding(need_gpu, src_dtype, Ksrc):
    from open_o3_video_amd.weights import pack_gate_up, pad_cols
    I, ipad, K = 200, 256, 192                 # zero rows (200 -> 256), zero columns (Ksrc -> 192)
    g = torch.Generator().manual_seed(5)
    gate, up = (torch.randn((I, Ksrc), generator=g) * 0.1).to(src_dtype), (torch.randn((I, Ksrc), generator=g) * 0.1).to(src_dtype)
    t = _canvas(2 * ipad, K, fp8=True, frag=True, seed=2)
    gpu_g, ref_g = _run_write(_write(t, row0=0, nblk=ipad // 16, stride=2), t, gate)
    _check(gpu_g, ref_g)
    gpu, ref = _run_write(_write(t, row0=1, nblk=ipad // 16, stride=2), gpu_g, up)
    _check(gpu, ref)
    # with both halves written the slot is pack_gate_up + pad_cols, the up half never touched the gate rows
    exp = pad_cols(pack_gate_up(gate.to(torch.bfloat16), up.to(torch.bfloat16), ipad), K)
    assert _same_bytes(gpu["s"], exp)


def test_kernel_row_and_column_maps(need_gpu):
    """Qwen3-VL head_rows: a row map with zero rows, and a column gather (proj_w)."""
    g = torch.Generator().manual_seed(7)
    src = torch.randn((72, 72), generator=g).to(torch.bfloat16)
    rm = torch.arange(80, dtype=torch.int32)
    rm = torch.where(rm % 40 < 36, (rm // 40) * 36 + rm % 40, torch.full_like(rm, -1))
    t = _canvas(80, 128, fp8=False, frag=False, seed=3)
    gpu, ref = _run_write(_write(t, row0=0, nblk=5, stride=1, row_map=rm), t, src)
    _check(gpu, ref)
    cm = torch.cat([rm, torch.full((48,), -1, dtype=torch.int32)])
    t = _canvas(72, 128, fp8=False, frag=False, seed=4)
    gpu, ref = _run_write(_write(t, row0=0, nblk=5, stride=1, col_map=cm), t, src)
    _check(gpu, ref)


def test_kernel_fp32_specials_round_like_torch(need_gpu):
    """+-inf, NaN (any payload) and bf16 rounding ties in an fp32 source: the bf16 images equal torch's conversion on the device
    (what a fresh load of a device fp32 tensor does; every NaN becomes 0x7FC0)."""
    from open_o3_video_amd.weights import pack_mfma_fragments
    rows, cols = 32, 256
    x = torch.randn((rows, cols), generator=torch.Generator().manual_seed(9))
    bits = x.view(torch.int32)
    bits[:, ::4] = (bits[:, ::4] & ~0xFFFF) | 0x8000           # exact ties, both parities of the kept bit
    bits[1, 1] = 0x7F800000                                      # +inf
    bits[1, 2] = -8388608                                        # 0xFF800000 -inf
    bits[2, 3] = 0x7FC00001                                      # quiet NaN with a payload
    bits[2, 5] = -1                                              # 0xFFFFFFFF NaN with the sign set
    bits[3, 7] = 0x7F7FFFFF                                      # max float: rounds to +inf
    bits[3, 9] = 0x00000001                                      # a denormal
    t = _canvas(rows, cols, fp8=False, frag=True, seed=5)
    gpu, _ = _run_write(_write(t, row0=0, nblk=2, stride=1), t, x)
    exp = x.cuda().to(torch.bfloat16).cpu()
    assert _same_bytes(gpu["s"], exp) and _same_bytes(gpu["sp"], pack_mfma_fragments(exp))
    finite = torch.isfinite(x).all(dim=1)
    assert _same_bytes(exp[finite], x[finite].to(torch.bfloat16))   # the host conversion agrees wherever there is no NaN / inf


# ------------------------------------------------------------------------------------------------ 2. full update A -> B
FIXTURES = {"tiny": (fm.tiny_config, fm.make_weights), "medium": (fm.medium_config, fm.make_weights),
            "tied3b": (fm.tied3b_config, fm.make_weights), "tiny_q3": (fq.tiny_q3_config, fq.make_weights)}


def _spelled(W, hub):
    """HF 5.x names, or the hub spelling of Qwen2.5-VL checkpoints (visual.*, model.layers.*)."""
    if not hub:
        return list(W.items())
    out = []
    for k, v in W.items():
        if k.startswith("model.visual."):
            k = "visual." + k[len("model.visual."):]
        elif k.startswith("model.language_model."):
            k = "model." + k[len("model.language_model."):]
        out.append((k, v))
    return out


@pytest.mark.parametrize("fix", list(FIXTURES))
def test_full_update_gives_the_bytes_of_a_fresh_load(need_gpu, fix):
    cfg_fn, mk = FIXTURES[fix]
    cfg = cfg_fn()
    WA, WB = mk(cfg, 0), mk(cfg, 1)
    dw = _dw(cfg, WA, fp8=True)
    ptrs = {k: v.data_ptr() for k, v in dw.t.items()}
    fresh = {"A": _dw(cfg, WA, fp8=True), "B": _dw(cfg, WB, fp8=True)}
    assert not _same_bytes(fresh["A"].t["l0.qkv_w"], fresh["B"].t["l0.qkv_w"])
    combos = [("B", "cpu", torch.float32, True), ("A", "cuda", torch.bfloat16, False), ("B", "cuda", torch.float32, False),
              ("A", "cpu", torch.bfloat16, True)]
    for which, where, dtype, hub in combos:
        W = WB if which == "B" else WA
        src = [(k, v.to(device=where, dtype=dtype)) for k, v in _spelled(W, hub)]
        done = dw.load_weights(src)
        assert done == set(dw.update_plan)
        del src                                  # the sources may go right away
        _assert_images_equal(dw, fresh[which])
        assert {k: v.data_ptr() for k, v in dw.t.items()} == ptrs
    if fresh["A"].cfg.text.tie_word_embeddings:  # lm_head of a tied model lands in the shared embedding and the head images
        dw.load_weights([("lm_head.weight", WB["model.language_model.embed_tokens.weight"])])
        for k in ("l.embed", "l.headp", "l.head8", "l.head8s", "l.head8p"):
            assert _same_bytes(dw.t[k], fresh["B"].t[k]), k


def test_partial_update_touches_only_its_images(need_gpu):
    cfg = fm.medium_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    name = "model.language_model.layers.1.mlp.up_proj.weight"
    dw = _dw(cfg, WA, fp8=True)
    before = {k: v.clone() for k, v in dw.t.items()}
    assert dw.load_weights([(name, WB[name].cuda())]) == {name}
    fresh = _dw(cfg, {**WA, name: WB[name]}, fp8=True)
    _assert_images_equal(dw, fresh)
    changed = {k for k in dw.t if not _same_bytes(dw.t[k], before[k])}
    assert changed == {"l1.gu_w", "l1.gu_wp", "l1.gu_w8", "l1.gu_w8s", "l1.gu_w8p"}
    gate_rows = dw.t["l1.gu_w"].view(-1, 2, 16, dw.t["l1.gu_w"].shape[1])[:, 0]
    assert _same_bytes(gate_rows, before["l1.gu_w"].view(-1, 2, 16, dw.t["l1.gu_w"].shape[1])[:, 0])


# ------------------------------------------------------------------------------------------------ 3. behaviour
def _prompt(eng, cfg, seed=9):
    fr = fm.make_frames(2, 56, 84, seed=seed)
    _, grid = eng.pixels_from_frames(fr)
    return fm.make_prompt(cfg, [tuple(r) for r in grid.tolist()], seed=seed), fr


def _same_out(a, b):
    return torch.equal(a.sequences, b.sequences) and (a.margins is None) == (b.margins is None) and \
        (a.margins is None or _same_bytes(a.margins, b.margins))


@pytest.mark.parametrize("fp8", [False, True])
def test_generate_after_update_equals_a_fresh_engine(need_gpu, fp8):
    cfg = fm.medium_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    eng = _engine(cfg, WA, fp8)
    fresh = _engine(cfg, WB, fp8)
    ids, fr = _prompt(eng, cfg)
    runs = [dict(max_new_tokens=12, pad_token_id=cfg["pad_token_id"]),                                  # B = 1
            dict(max_new_tokens=10, num_return_sequences=8, do_sample=True, top_p=0.95, top_k=50, temperature=1.0, seed=3)]   # G = 8
    before = [eng.generate([ids], None, frames=fr, **kw) for kw in runs]
    eng.load_weights([(k, v.cuda()) for k, v in WB.items()])
    for kw, a in zip(runs, before):
        got, exp = eng.generate([ids], None, frames=fr, **kw), fresh.generate([ids], None, frames=fr, **kw)
        assert _same_out(got, exp), kw
        assert not torch.equal(a.sequences, exp.sequences), "A and B must decode differently for the test to mean anything"
    assert _same_bytes(eng.forward_logits([ids], None, frames=fr), fresh.forward_logits([ids], None, frames=fr))


# ------------------------------------------------------------------------------------------------ 5. caches
def test_prefix_and_handover_are_not_reused_across_an_update(need_gpu):
    cfg = fm.medium_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    eng, fresh = _engine(cfg, WA), _engine(cfg, WB)
    ids, fr = _prompt(eng, cfg)
    kw = dict(max_new_tokens=8, pad_token_id=cfg["pad_token_id"])
    eng.generate([ids], None, frames=fr, prefix_key="video", **kw)
    assert eng.generate([ids], None, frames=fr, prefix_key="video", **kw).timings["prefix_tokens_reused"] > 0
    gkw = dict(max_new_tokens=10, num_return_sequences=4, do_sample=True, top_p=0.95, top_k=50, temperature=1.0, seed=3)
    out = eng.generate([ids], None, frames=fr, **gkw)
    assert eng._last_prompt is not None
    v0 = eng.weights_version
    eng.load_weights([(k, v.cuda()) for k, v in WB.items()])
    assert eng.weights_version == v0 + 1 and eng._last_prompt is None and not eng._prefix
    comp = out.sequences[:, len(ids):]
    lp = eng.completion_logps([ids], comp, frames=fr)
    assert not eng.timings_last_logps["prompt_kv_reused"]
    assert _same_bytes(lp, fresh.completion_logps([ids], comp, frames=fr))
    warm = eng.generate([ids], None, frames=fr, prefix_key="video", **kw)
    assert warm.timings["prefix_tokens_reused"] == 0
    assert _same_out(warm, fresh.generate([ids], None, frames=fr, **kw))
    # a hand-over made BEFORE an update is never taken after it, even if the caller restores the memo by hand
    out = eng.generate([ids], None, frames=fr, **gkw)
    memo = eng._last_prompt
    eng.load_weights([(k, v.cuda()) for k, v in WB.items()])
    eng._last_prompt = memo
    eng.completion_logps([ids], out.sequences[:, len(ids):], frames=fr)
    assert not eng.timings_last_logps["prompt_kv_reused"]


def test_qwen3_pos_embed_update_refreshes_the_tower(need_gpu):
    cfg = fq.tiny_q3_config()
    WA, WB = fq.make_weights(cfg, 0), fq.make_weights(cfg, 1)
    name = "model.visual.pos_embed.weight"
    eng = _engine(cfg, WA)
    fresh = _engine(cfg, {**WA, name: WB[name]})
    px, grid = eng.pixels_from_frames(fm.make_frames(2, 64, 96, seed=4))
    old = eng.vit_forward(px, grid)
    assert eng._vit_plan_cache
    eng.load_weights([("visual.pos_embed.weight", WB[name])])
    new = eng.vit_forward(px, grid)
    assert _same_bytes(new, fresh.vit_forward(px, grid))
    assert not _same_bytes(new, old)


# ------------------------------------------------------------------------------------------------ 5/6. facades
def test_vllm_facade_update_and_trl_chain(need_gpu):
    from open_o3_video_amd.vllm_api import LLM, SamplingParams
    from test_gpu_facades import StubTokenizer
    cfg = fm.medium_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    llm = LLM(engine=_engine(cfg, WA), tokenizer=StubTokenizer(cfg), limit_mm_per_prompt={"image": 32}, max_model_len=4096)
    ref = LLM(engine=_engine(cfg, WB), tokenizer=StubTokenizer(cfg), limit_mm_per_prompt={"image": 32}, max_model_len=4096)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_medium.npz"))
    words, ids, i = [], g["input_ids"][0].tolist(), 0
    while i < len(ids):            # the prompt text with ONE <|image_pad|> per frame, as test_gpu_facades builds it
        if ids[i] == cfg["image_token_id"]:
            words.append("<|image_pad|>")
            while i < len(ids) and ids[i] == cfg["image_token_id"]:
                i += 1
            continue
        words.append({cfg["vision_start_token_id"]: "<|vision_start|>", cfg["vision_end_token_id"]: "<|vision_end|>"}.get(ids[i], f"w{ids[i]}"))
        i += 1
    prompt, frames = " ".join(words), torch.from_numpy(g["frames"])
    sp = SamplingParams(temperature=0.0, max_tokens=10, stop_token_ids=[])
    req = {"prompt": prompt, "multi_modal_data": {"image": frames}}
    a = llm.generate(req, sp)[0].outputs[0].token_ids
    assert llm.generate(req, sp)[0].outputs[0].token_ids == a
    hits = llm.vis_cache_hits
    assert hits >= 1
    model = llm.llm_engine.model_executor.driver_worker.model_runner.model
    model.load_weights(((k, v.cuda()) for k, v in WB.items()))
    b = llm.generate(req, sp)[0].outputs[0].token_ids
    assert llm.vis_cache_hits == hits                       # the visual tokens were recomputed with B's tower
    assert b == ref.generate(req, sp)[0].outputs[0].token_ids and b != a
    assert llm.reset_prefix_cache() is True
    llm.load_weights(WA.items())
    assert llm.generate(req, sp)[0].outputs[0].token_ids == a


def test_hf_facade_load_state_dict(need_gpu):
    from open_o3_video_amd.hf_api import GenerationConfigLike, Qwen2_5_VLForConditionalGeneration
    cfg = fm.tiny_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    model = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, WA)
    ref = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, WB)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g6_tiny.npz"))
    inp = dict(input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.ones_like(torch.from_numpy(g["input_ids"])),
               pixel_values=torch.from_numpy(g["pixel_values"]),
               image_grid_thw=torch.from_numpy(g["grid"]))
    gc = GenerationConfigLike(max_new_tokens=8, do_sample=False, num_return_sequences=1, pad_token_id=cfg["pad_token_id"],
                              eos_token_id=None)
    a = model.generate(**inp, generation_config=gc)
    r = model.load_state_dict(WB)
    assert r.missing_keys == [] and r.unexpected_keys == []
    out = model.generate(**inp, generation_config=gc)
    assert torch.equal(out, ref.generate(**inp, generation_config=gc)) and not torch.equal(out, a)
    with pytest.raises(RuntimeError):
        model.load_state_dict({**WA, "extra.weight": torch.zeros(3)})
    with pytest.raises(RuntimeError):
        model.load_state_dict({"model.language_model.norm.weight": WA["model.language_model.norm.weight"]})
    name = "model.language_model.layers.1.mlp.up_proj.weight"
    r = model.load_state_dict({name: WA[name], "extra.weight": torch.zeros(3)}, strict=False)
    assert r.unexpected_keys == ["extra.weight"] and name not in r.missing_keys
    assert len(r.missing_keys) == len(model.engine.w.update_plan) - 1
    assert model.load_weights(WA.items()) == set(model.engine.w.update_plan)
    assert torch.equal(model.generate(**inp, generation_config=gc), a)


# ------------------------------------------------------------------------------------------------ 7. stream order
def _spin(ms):
    """Keep the current stream busy for about `ms` milliseconds (a bounded spin kernel, calibrated here); returns an event recorded
    right after the spin -- not yet complete means nothing queued behind the spin has started."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(10_000_000)
    b.record()
    b.synchronize()
    torch.cuda._sleep(int(10_000_000 * ms / max(a.elapsed_time(b), 1e-3)))
    done = torch.cuda.Event()
    done.record()
    return done


def test_update_is_ordered_on_the_stream(need_gpu):
    """generate -> load_weights -> generate with no synchronisation in between gives A's then B's output.  (generate reads its
    ids back, so this alone cannot tell stream order from a host synchronisation: the next test can.)"""
    cfg = fm.medium_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    eng, fa, fb = _engine(cfg, WA), _engine(cfg, WA), _engine(cfg, WB)
    ids, fr = _prompt(eng, cfg)
    kw = dict(max_new_tokens=8, num_return_sequences=8, do_sample=True, top_p=0.95, top_k=50, temperature=1.0, seed=5)
    WBd = [(k, v.to("cuda", torch.bfloat16)) for k, v in WB.items()]
    torch.cuda.synchronize()
    o1 = eng.generate([ids], None, frames=fr, **kw)
    eng.load_weights(WBd)
    del WBd
    o2 = eng.generate([ids], None, frames=fr, **kw)
    assert _same_out(o1, fa.generate([ids], None, frames=fr, **kw))
    assert _same_out(o2, fb.generate([ids], None, frames=fr, **kw))


def test_update_is_enqueued_on_the_current_stream_without_a_host_sync(need_gpu):
    """On a side stream held busy by a spin kernel, load_weights returns while nothing has been written yet (a read on another
    stream still sees A), and after that stream drains every image is B's."""
    cfg = fm.tiny_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    dw, fresh_a, fresh_b = _dw(cfg, WA, fp8=True), _dw(cfg, WA, fp8=True), _dw(cfg, WB, fp8=True)
    src = [(k, v.to("cuda", torch.bfloat16)) for k, v in WB.items()]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        side.wait_stream(torch.cuda.default_stream())
        spun = _spin(1000)
        dw.load_weights(src)
    snap = {k: v.clone() for k, v in dw.t.items()}            # default stream, while `side` still spins
    torch.cuda.default_stream().synchronize()
    assert not spun.query(), "the spin ended before the snapshot: the check did not run"
    _assert_images_equal(SimpleNamespace(t=snap), fresh_a)
    side.synchronize()
    _assert_images_equal(dw, fresh_b)


def test_device_sources_freed_right_after_the_call_stay_safe(need_gpu):
    """Sources allocated on another stream and freed as soon as load_weights returns (a ZeRO-3 gather context closing): their
    memory must not be handed out again before the queued update has read it (record_stream on the resolved device)."""
    cfg = fm.medium_config()
    WA, WB = fm.make_weights(cfg, 0), fm.make_weights(cfg, 1)
    dw, fresh_b = _dw(cfg, WA, fp8=True), _dw(cfg, WB, fp8=True)
    assert dw.device == torch.device("cuda")                  # the bare device string the facades pass
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        src = [(k, v.to("cuda", torch.bfloat16)) for k, v in WB.items()]
    torch.cuda.current_stream().wait_stream(other)
    spun = _spin(1000)                                         # the update stays queued behind this
    dw.load_weights(src)
    shapes = [(v.shape, v.dtype) for _, v in src]
    del src
    with torch.cuda.stream(other):                             # `other` is idle: without record_stream this reuses the blocks now
        junk = [torch.full(sh, 3.0, dtype=dt, device="cuda") for sh, dt in shapes]
    other.synchronize()
    assert not spun.query(), "the spin ended before the sources were overwritten: the check did not run"
    torch.cuda.synchronize()
    del junk
    _assert_images_equal(dw, fresh_b)
