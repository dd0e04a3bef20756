"""LoRA adapters, host side: the exact probes stay exact, every peft spelling finds its plan entry, every refusal names the module
and allocates nothing, scales from adapter_config.json, the adapter's image list, the C ABI's argument errors, the vLLM keywords
over a recording engine, and the rollout's reference pass under disable_adapter()."""
import contextlib
import ctypes as C
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_models as fm  # noqa: E402
import fixture_models_q3 as fq  # noqa: E402
import lora_ref as lr  # noqa: E402

from open_o3_video_amd import _lib, hf_api, rollout  # noqa: E402
from open_o3_video_amd.config import O3VConfig  # noqa: E402
from open_o3_video_amd.weights import DeviceWeights, getter_from_dict  # noqa: E402

SHAPES = [(16, 32, 1), (48, 80, 3), (64, 128, 16), (32, 1040, 17), (16, 64, 256)]
L0 = "model.language_model.layers.0."


def _cpu(cfg_dict, W, **kw):
    c = O3VConfig.from_dict(cfg_dict)
    return DeviceWeights(c, getter_from_dict(W), "cpu", **kw)


@pytest.fixture(scope="module")
def tiny():
    cfg = fm.tiny_config()
    W = fm.make_weights(cfg, 0)
    return cfg, W, _cpu(cfg, W, fp8_decode=True)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("N,K,r", SHAPES)
@pytest.mark.parametrize("scale", [lr.PROBE_SCALE, -lr.PROBE_SCALE, 0.0])
def test_exact_probes_are_exact(N, K, r, scale):
    """fp32 and fp64 agree before the final rounding, so no summation order can change the bf16 result."""
    W = lr.probe_base(N, K, seed=N + K + r)
    A, B = lr.probe_ab(N, K, r, seed=r)
    assert W.float().abs().max() <= 2 and torch.equal(W.float() * 64, (W.float() * 64).round())
    f32 = W.float() + scale * (B.float() @ A.float())
    f64 = lr.merge64(W, A, B, scale)
    assert torch.equal(f32.double(), f64)
    assert torch.equal(lr.merge(W, A, B, scale), f64.to(torch.bfloat16))
    # a different summation order (reversed j) gives the same fp32 values
    assert torch.equal(W.float() + scale * (B.float().flip(1) @ A.float().flip(0)), f32)
    if r > 1 and scale:
        assert not torch.equal(lr.merge(W, A, B, scale), W)


def test_general_bound_holds_for_the_reference():
    W, A, B = lr.general(64, 128, 16, seed=1)
    y, bnd = lr.bound(W, A, B, 0.5)
    assert ((lr.merge(W, A, B, 0.5).double() - y).abs() <= bnd).all()
    assert lr.ulp_bf16(torch.tensor([1.0, 1.5, 0.02], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -13]


# ------------------------------------------------------------------------------------------------ names
@pytest.mark.parametrize("fmt", ["base_model.model.{m}.lora_{x}.weight", "base_model.model.{m}.lora_{x}.default.weight", "{m}.lora_{x}.weight",
                                 "{m}.lora_{x}.policy.weight"])
@pytest.mark.parametrize("mod,canon", [
    ("model.language_model.layers.1.self_attn.q_proj", "model.language_model.layers.1.self_attn.q_proj.weight"),
    ("model.layers.1.mlp.up_proj", "model.language_model.layers.1.mlp.up_proj.weight"),
    ("language_model.model.layers.0.mlp.down_proj", "model.language_model.layers.0.mlp.down_proj.weight"),
    ("visual.blocks.2.attn.qkv", "model.visual.blocks.2.attn.qkv.weight"),
    ("model.visual.merger.mlp.0", "model.visual.merger.mlp.0.weight")])
def test_every_peft_spelling_maps_to_its_plan_entry(tiny, fmt, mod, canon):
    cfg, W, dw = tiny
    N, K = dw.update_plan[canon].shape
    A, B = lr.probe_ab(N, K, 4, 0)
    items = dw._validate_adapter([(fmt.format(m=mod, x="A"), A), (fmt.format(m=mod, x="B"), B)], lora_alpha=8)
    assert [(k, sc) for k, e, a, b, sc in items] == [(canon, 2.0)]


def test_scale_rules(tiny):
    cfg, W, dw = tiny
    mod = L0 + "self_attn.q_proj"
    A, B = lr.probe_ab(128, 128, 16, 0)
    named = lr.peft_names({mod: (A, B)})
    assert dw._validate_adapter(named, lora_alpha=32)[0][4] == 2.0
    assert dw._validate_adapter(named, lora_alpha=32, use_rslora=True)[0][4] == 8.0
    assert dw._validate_adapter(named, scale=0.25, lora_alpha=32)[0][4] == 0.25
    with pytest.raises(ValueError, match="scale or lora_alpha"):
        dw._validate_adapter(named)


@pytest.mark.parametrize("rslora,expect", [(False, 32 / 16), (True, 32 / 4)])
def test_scale_from_adapter_config(tmp_path, rslora, expect):
    from safetensors.torch import save_file
    A, B = lr.probe_ab(128, 128, 16, 0)
    mod = L0 + "self_attn.q_proj"
    save_file(dict(lr.peft_names({mod: (A, B)})), str(tmp_path / "adapter_model.safetensors"))
    (tmp_path / "adapter_config.json").write_text(json.dumps({"peft_type": "LORA", "r": 16, "lora_alpha": 32, "use_rslora": rslora,
                                                               "bias": "none", "target_modules": ["q_proj"]}))
    tensors, alpha, rs = hf_api.read_adapter_dir(str(tmp_path))
    assert (alpha, rs) == (32.0, rslora) and {n for n, _ in tensors} == {n for n, _ in lr.peft_names({mod: (A, B)})}
    cfg = fm.tiny_config()
    dw = _cpu(cfg, fm.make_weights(cfg, 0))
    assert dw._validate_adapter(tensors, lora_alpha=alpha, use_rslora=rs)[0][4] == expect


@pytest.mark.parametrize("field,value,word", [("bias", "all", "bias"), ("use_dora", True, "use_dora"), ("rank_pattern", {"q_proj": 4}, "rank_pattern"),
                                              ("alpha_pattern", {"q_proj": 4}, "alpha_pattern"), ("modules_to_save", ["lm_head"], "modules_to_save"),
                                              ("fan_in_fan_out", True, "fan_in_fan_out"), ("peft_type", "IA3", "peft_type")])
def test_adapter_config_refusals(field, value, word):
    with pytest.raises(ValueError, match=word):
        hf_api.read_adapter_config({"r": 8, "lora_alpha": 16, field: value})
    assert hf_api.read_adapter_config({"r": 8, "lora_alpha": 16, "bias": "none", "rank_pattern": {}, "modules_to_save": None}) == (16.0, False)


# ------------------------------------------------------------------------------------------------ refusals
def _q(dw, r=4, dtype=torch.bfloat16, mod=L0 + "self_attn.q_proj"):
    N, K = dw.update_plan[dw.resolve_name(mod + ".weight")].shape
    return lr.probe_ab(N, K, r, 0, dtype)


def test_every_refusal_names_the_module_and_allocates_nothing(tiny):
    cfg, W, dw = tiny
    A, B = _q(dw)
    q = L0 + "self_attn.q_proj"
    ok = lr.peft_names({q: (A, B)})
    cases = [
        ([(f"base_model.model.{q}.lora_A.weight", A)], "q_proj"),                                              # A without B
        ([(f"base_model.model.{q}.lora_B.weight", B)], "q_proj"),
        (lr.peft_names({q: (A[:3], B)}), "q_proj"),                                                            # rank mismatch
        (lr.peft_names({q: (A[:, :64], B)}), "q_proj"),                                                        # shape mismatch
        (lr.peft_names({q: lr.probe_ab(128, 128, 257, 0)}), "rank 257"),
        (lr.peft_names({q: (A.half(), B.half())}), "dtype"),
        (lr.peft_names({q: (A.double(), B.double())}), "dtype"),
        (ok + [(f"base_model.model.{q}.lora_magnitude_vector.default.weight", torch.ones(128))], "DoRA"),
        ([("base_model.model.model.language_model.embed_tokens.lora_embedding_A.default", A)], "lora_embedding"),
        (ok + [("base_model.model.lm_head.modules_to_save.default.weight", W["lm_head.weight"])], "modules_to_save"),
        (lr.peft_names({"lm_head": lr.probe_ab(512, 128, 4, 0)}), "lm_head"),
        (lr.peft_names({"model.language_model.embed_tokens": lr.probe_ab(512, 128, 4, 0)}), "embed_tokens"),
        (lr.peft_names({"model.visual.patch_embed.proj": lr.probe_ab(64, 1176, 4, 0)}), "patch-embed"),
        (lr.peft_names({q: (A, B)}, adapter_name="a") + lr.peft_names({L0 + "self_attn.k_proj": _q(dw, mod=L0 + "self_attn.k_proj")},
                                                                       adapter_name="b"), "several adapters"),
        ([], "no LoRA tensors"),
    ]
    for named, word in cases:
        with pytest.raises(ValueError, match=word):
            dw.load_adapter(named, lora_alpha=8)
        assert not dw.adapter_loaded and not dw.adapter_t and not dw.adapter_enabled, word
    with pytest.raises(KeyError):
        dw.load_adapter(lr.peft_names({"model.language_model.layers.7.self_attn.q_proj": (A, B)}), lora_alpha=8)
    # a valid adapter passes validation; without a GPU the merge itself is refused, still with nothing allocated
    with pytest.raises(_lib.O3VError, match="ROCm GPU"):
        dw.load_adapter(ok, lora_alpha=8)
    assert not dw.adapter_loaded and not dw.adapter_t


def test_unsupported_plan_entries_and_mapped_tower_matrices_are_refused():
    cfg = fq.tiny_q3_config()
    dw = _cpu(cfg, fq.make_weights(cfg, 0))
    for mod in ("model.visual.blocks.0.attn.qkv", "model.visual.blocks.1.attn.proj"):
        N, K = dw.update_plan[mod + ".weight"].shape
        with pytest.raises(ValueError, match=mod.rsplit(".", 1)[1]):
            dw.load_adapter(lr.peft_names({mod: lr.probe_ab(N, K, 4, 0)}), lora_alpha=8)
    for mod in ("model.visual.blocks.0.mlp.linear_fc1", "model.visual.merger.linear_fc2", "model.visual.deepstack_merger_list.0.linear_fc1"):
        N, K = dw.update_plan[mod + ".weight"].shape
        assert dw._validate_adapter(lr.peft_names({mod: lr.probe_ab(N, K, 4, 0)}), lora_alpha=8)[0][0] == mod + ".weight"
    e = dw.update_plan[L0 + "self_attn.o_proj.weight"]
    e.unsupported, keep = "made up for the test", e.unsupported
    try:
        with pytest.raises(ValueError, match="made up for the test"):
            dw.load_adapter(lr.peft_names({L0 + "self_attn.o_proj": lr.probe_ab(*e.shape, 4, 0)}), lora_alpha=8)
    finally:
        e.unsupported = keep


# ------------------------------------------------------------------------------------------------ the image set
def test_image_keys_q_proj_only_and_all_linears():
    cfg = fm.tiny_config()
    dw = _cpu(cfg, fm.make_weights(cfg, 0), mxfp4_decode=True)
    assert dw.adapter_image_keys([L0 + "self_attn.q_proj.weight"]) == ["l0.qkv_w", "l0.qkv_wp", "l0.qkv_w8", "l0.qkv_w8s", "l0.qkv_w8p"]
    names = [f"model.language_model.layers.{i}.{m}.weight" for i in range(2) for m in lr.LLM_LINEARS]
    keys = dw.adapter_image_keys(names)
    expect = {k for k in dw.t if k[0] == "l" and k[1].isdigit() and "_w" in k}
    assert set(keys) == expect and len(keys) == len(set(keys))
    assert {"l1.gu_w4", "l1.gu_w4s", "l1.gu_w4p", "l1.gu_w4ps", "l1.down_w4", "l0.o_w8p"} <= expect
    # every key has a descriptor field that currently points at the base image
    for k in keys:
        st, field = dw._descriptor_field(k)
        assert getattr(st, field) == dw.t[k].data_ptr(), k
    # the tower: plain bf16 slots
    assert dw.adapter_image_keys(["visual.blocks.1.mlp.gate_proj.weight", "visual.merger.mlp.2.weight"]) == ["v1.gu_w", "v.m2_w"]
    for k in ("v1.gu_w", "v.m2_w", "v0.qkv_w", "v3.down_w", "v.m0_w"):
        st, field = dw._descriptor_field(k)
        assert getattr(st, field) == dw.t[k].data_ptr(), k


def test_descriptor_fields_of_the_qwen3_tower():
    cfg = fq.tiny_q3_config()
    dw = _cpu(cfg, fq.make_weights(cfg, 0))
    keys = dw.adapter_image_keys(["model.visual.blocks.0.mlp.linear_fc1.weight", "model.visual.merger.linear_fc2.weight",
                                  "model.visual.deepstack_merger_list.0.linear_fc1.weight"])
    assert keys == ["v0.fc1_w", "v.m.fc2_w", "v.ds0.fc1_w"]
    for k in keys:
        st, field = dw._descriptor_field(k)
        assert getattr(st, field) == dw.t[k].data_ptr(), k


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _desc(**kw):
    buf = torch.zeros(64 * 64, dtype=torch.bfloat16)
    p = buf.data_ptr()
    assert p % 16 == 0
    d = dict(base=p, A=p, B=p, out=p, base_ld=64, a_ld=64, b_ld=16, out_ld=64, ab_dtype=_lib.SRC_BF16, N=32, K=64, r=16, base_rows=32,
             blk0=0, blk_stride=1, scale=1.0)
    d.update(kw)
    return _lib.LoraDesc(**d), buf


@pytest.mark.parametrize("kw,rc", [
    (dict(base=None), _lib.ERR_ARG), (dict(A=None), _lib.ERR_ARG), (dict(B=None), _lib.ERR_ARG), (dict(out=None), _lib.ERR_ARG),
    (dict(ab_dtype=2), _lib.ERR_ARG), (dict(N=0), _lib.ERR_ARG), (dict(K=-8), _lib.ERR_ARG), (dict(r=0), _lib.ERR_ARG),
    (dict(base_ld=56), _lib.ERR_ARG), (dict(out_ld=56), _lib.ERR_ARG), (dict(a_ld=56), _lib.ERR_ARG), (dict(b_ld=8), _lib.ERR_ARG),
    (dict(blk0=-1), _lib.ERR_ARG), (dict(blk_stride=0), _lib.ERR_ARG), (dict(blk0=1), _lib.ERR_ARG), (dict(blk_stride=2), _lib.ERR_ARG),
    (dict(base_rows=31), _lib.ERR_ARG), (dict(scale=float("nan")), _lib.ERR_ARG), (dict(scale=float("inf")), _lib.ERR_ARG),
    (dict(r=257, b_ld=264), _lib.ERR_SHAPE), (dict(N=24), _lib.ERR_SHAPE), (dict(K=60), _lib.ERR_SHAPE),
    (dict(base_ld=68), _lib.ERR_SHAPE), (dict(out_ld=68), _lib.ERR_SHAPE), (dict(a_ld=68), _lib.ERR_SHAPE)])
def test_c_abi_argument_errors(kw, rc):
    d, keep = _desc(**kw)
    assert _lib.load().o3v_lora_merge(C.byref(d), None) == rc


def test_c_abi_misaligned_pointers_and_null_descriptor():
    lib = _lib.load()
    assert lib.o3v_lora_merge(None, None) == _lib.ERR_ARG
    for f in ("base", "A", "B", "out"):
        d, keep = _desc()
        setattr(d, f, getattr(d, f) + 2)
        assert lib.o3v_lora_merge(C.byref(d), None) == _lib.ERR_ARG, f


# ------------------------------------------------------------------------------------------------ vLLM keywords
class _RecordingEngine:
    """What LLM touches of an engine when only the adapter state is driven."""

    def __init__(self):
        self.cfg = O3VConfig.from_dict(fm.tiny_config())
        self.calls, self.adapter_loaded, self.adapter_enabled = [], False, False

    def load_adapter(self, tensors, scale=None, lora_alpha=None, use_rslora=False):
        self.calls.append(("load", sorted(n for n, _ in tensors), lora_alpha, use_rslora))
        self.adapter_loaded = self.adapter_enabled = True

    def set_adapter_enabled(self, flag):
        self.calls.append(("enable", bool(flag)))
        self.adapter_enabled = bool(flag)


def _adapter_dir(path, r=4, alpha=8, mod=L0 + "self_attn.q_proj"):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    A, B = lr.probe_ab(128, 128, r, r)
    save_file(dict(lr.peft_names({mod: (A, B)})), os.path.join(path, "adapter_model.safetensors"))
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none"}, f)
    return str(path)


def test_lora_request_and_enable_lora_checks(tmp_path):
    from open_o3_video_amd.vllm_api import LLM, LoRARequest
    one, two, big = _adapter_dir(tmp_path / "one"), _adapter_dir(tmp_path / "two"), _adapter_dir(tmp_path / "big", r=32)
    eng = _RecordingEngine()
    off = LLM(engine=eng, tokenizer=object())
    with pytest.raises(ValueError, match="LoRA is not enabled"):
        off.generate([], lora_request=LoRARequest("a", 1, one))
    off.generate([])
    assert eng.calls == []                                   # without enable_lora and without a request nothing is touched
    with pytest.raises(ValueError):
        LoRARequest("a", 0, one)

    llm = LLM(engine=eng, tokenizer=object(), enable_lora=True, max_lora_rank=16)
    r1, r2 = LoRARequest("a", 1, one), LoRARequest("b", 2, two)
    assert llm.generate([], lora_request=r1) == [] and eng.calls[-1][0] == "load" and eng.calls[-1][2:] == (8.0, False)
    n = len(eng.calls)
    llm.generate([], lora_request=LoRARequest("same adapter, other name", 1, one))
    assert eng.calls[n:] == [("enable", True)]              # resident: no reload
    llm.generate([], lora_request=None)
    assert eng.calls[-1] == ("enable", False) and not eng.adapter_enabled
    llm.generate([], lora_request=r1)
    assert eng.calls[-1] == ("enable", True)
    llm.generate([], lora_request=r2)
    assert eng.calls[-1][0] == "load"                        # another (id, path): loaded in its place
    with pytest.raises(ValueError, match="max_lora_rank"):
        llm.generate([], lora_request=LoRARequest("big", 3, big))
    with pytest.raises(ValueError, match="'a'.*'b'|same adapter"):
        llm._apply_lora([r1, r2], 2)
    with pytest.raises(ValueError, match="same adapter"):
        llm._apply_lora([r1, None], 2)
    with pytest.raises(ValueError, match="lengths"):
        llm._apply_lora([r1], 2)
    n = len(eng.calls)
    llm._apply_lora([r2, LoRARequest("b again", 2, two)], 2)
    assert eng.calls[n:] == [("enable", True)]
    with pytest.raises(OSError):
        llm.generate([], lora_request=LoRARequest("missing", 9, str(tmp_path / "nowhere")))


# ------------------------------------------------------------------------------------------------ the rollout's reference pass
class _StubModel:
    EOS, PAD = 9, 0

    def __init__(self, adapter_loaded):
        self.adapter_loaded, self.enabled, self.log = adapter_loaded, adapter_loaded, []

    def generate(self, input_ids, attention_mask, pixel_values, image_grid_thw, generation_config):
        G = generation_config.num_return_sequences
        comp = torch.tensor([[11 + g, 12, self.EOS] for g in range(G)])
        return torch.cat([torch.as_tensor(input_ids).expand(G, -1), comp], dim=1)

    def completion_logps(self, prompt_ids, prompt_mask, completion_ids, pixel_values=None, image_grid_thw=None):
        self.log.append(self.enabled)
        return -(0.05 if self.enabled else 0.07) * completion_ids.float()

    @contextlib.contextmanager
    def disable_adapter(self):
        was, self.enabled = self.enabled, False
        try:
            yield
        finally:
            self.enabled = was


def _step(model):
    gr = rollout.GroupRollout(model, [lambda prompts, completions, **kw: [1.0] * len(completions)], lambda ids: ["x"] * len(ids),
                              eos_token_id=model.EOS, pad_token_id=model.PAD, num_generations=3, max_completion_length=4)
    return gr.step({"input_ids": torch.tensor([[5, 6, 7]]), "attention_mask": torch.ones(1, 3, dtype=torch.int64)}, {"prompt": "p"})


def test_rollout_reference_pass_runs_with_the_adapter_disabled():
    m = _StubModel(adapter_loaded=True)
    res = _step(m)
    assert m.log == [True, False] and m.enabled            # policy pass, then the reference pass inside disable_adapter()
    assert res.ref_per_token_logps is not res.per_token_logps
    assert torch.equal(res.ref_per_token_logps, -0.07 * res.completion_ids.float())
    assert (res.per_token_kl != 0).any()


def test_rollout_without_an_adapter_keeps_the_policy_as_its_reference():
    m = _StubModel(adapter_loaded=False)
    res = _step(m)
    assert m.log == [False] and res.ref_per_token_logps is res.per_token_logps
    assert (res.per_token_kl == 0).all()
