"""In-place weight update (DeviceWeights.load_weights), host side: the update plan recorded at load covers every weight of the
fixture models under every accepted spelling, rejects bad input before writing anything, keeps each 16-row block of an LLM slot
to one source, and -- replayed on the CPU with a torch restatement of o3v_repack_rows -- turns a model loaded from seed A into
the bytes of a fresh load of seed B."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_models as fm  # noqa: E402
import fixture_models_q3 as fq  # noqa: E402

from open_o3_video_amd.config import O3VConfig  # noqa: E402
from open_o3_video_amd.weights import (DeviceWeights, _RepackWrite, getter_from_dict, pack_mfma_fragments,  # noqa: E402
                                       pack_mfma_fragments_fp8, quantize_rows_fp8)

FIXTURES = {"tiny": (fm.tiny_config, fm.make_weights), "medium": (fm.medium_config, fm.make_weights),
            "tied3b": (fm.tied3b_config, fm.make_weights), "tiny_q3": (fq.tiny_q3_config, fq.make_weights)}


def _load(fix, seed, fp8=False):
    cfg_fn, mk = FIXTURES[fix]
    cfg = cfg_fn()
    W = mk(cfg, seed)
    c = O3VConfig.from_dict(cfg)
    return c, W, DeviceWeights(c, getter_from_dict(W), "cpu", fp8_decode=fp8)


def _repack_ref(w: _RepackWrite, t, src):
    """What o3v_repack_rows writes, restated with the torch packers."""
    dst = t[w.slot]
    rows, cols = dst.shape
    src = src.to(torch.bfloat16)
    for i in range(w.nblk):
        b = w.row0 + i * w.stride
        r0, r1 = 16 * b, min(16 * b + 16, rows)
        img = torch.zeros((r1 - r0, cols), dtype=torch.bfloat16)
        for r in range(r1 - r0):
            s = int(w.row_map[16 * i + r]) if w.row_map is not None else 16 * i + r
            if s < 0 or s >= src.shape[0]:
                continue
            if w.col_map is None:
                img[r, : src.shape[1]] = src[s]
            else:
                cm = w.col_map.long()
                img[r] = torch.where(cm >= 0, src[s][cm.clamp(min=0)], torch.zeros((), dtype=torch.bfloat16))
        dst[r0:r1] = img
        if w.frag:
            t[w.frag].view(-1)[r0 * cols: r1 * cols] = pack_mfma_fragments(img).view(-1)
        if w.q8:
            q8, sc = quantize_rows_fp8(img)
            t[w.q8][r0:r1], t[w.q8s][r0:r1] = q8, sc
            if w.q8frag:
                t[w.q8frag].view(-1)[r0 * cols: r1 * cols] = pack_mfma_fragments_fp8(q8).view(-1)


def _replay(dw: DeviceWeights, named):
    for name, src in named:
        e = dw.update_plan[dw.resolve_name(name)]
        for w in e.writes:
            if isinstance(w, _RepackWrite):
                _repack_ref(w, dw.t, src.reshape(e.shape))
            else:
                w.apply(dw.t, src, None)


@pytest.mark.parametrize("fix", list(FIXTURES))
def test_every_fixture_weight_has_a_plan_entry(fix):
    c, W, dw = _load(fix, 0, fp8=True)
    canon = {dw.resolve_name(k) for k in W}
    assert canon == set(dw.update_plan)
    for k, t in W.items():
        e = dw.update_plan[dw.resolve_name(k)]
        assert tuple(t.shape) in (e.shape,) + tuple(e.alt_shapes), k


@pytest.mark.parametrize("fix", list(FIXTURES))
def test_llm_slots_take_whole_16_row_blocks_from_one_source(fix):
    c, W, dw = _load(fix, 0, fp8=True)
    owner = {}
    for name, e in dw.update_plan.items():
        for w in e.writes:
            if not isinstance(w, _RepackWrite):
                continue
            rows, cols = dw.t[w.slot].shape
            assert cols % 16 == 0, (name, w.slot)
            if not w.slot.startswith("l"):
                continue
            assert rows % 16 == 0 and w.row_map is None and w.col_map is None
            for i in range(w.nblk):
                b = w.row0 + i * w.stride
                assert 16 * b + 16 <= rows
                assert owner.setdefault((w.slot, b), name) == name, (w.slot, b)
            assert (w.frag is not None) == (w.slot + "p" in dw.t or (w.slot == "l.embed" and "l.headp" in dw.t
                                                                       and c.text.tie_word_embeddings))
    for key, t in dw.t.items():   # every block of every LLM matrix has exactly one owner
        if key.startswith("l") and t.dim() == 2 and key in {w.slot for e in dw.update_plan.values() for w in e.writes}:
            assert {b for (s, b) in owner if s == key} == set(range(t.shape[0] // 16)), key


def test_alternative_spellings_resolve_to_the_same_slot():
    c, W, dw = _load("tiny", 0)
    assert dw.resolve_name("model.layers.1.mlp.up_proj.weight") == "model.language_model.layers.1.mlp.up_proj.weight"
    assert dw.resolve_name("language_model.model.layers.1.mlp.up_proj.weight") == "model.language_model.layers.1.mlp.up_proj.weight"
    assert dw.resolve_name("model.embed_tokens.weight") == "model.language_model.embed_tokens.weight"
    assert dw.resolve_name("visual.blocks.0.attn.qkv.weight") == "model.visual.blocks.0.attn.qkv.weight"
    assert dw.resolve_name("model.visual.merger.mlp.0.weight") == "model.visual.merger.mlp.0.weight"
    assert dw.resolve_name("lm_head.weight") == "lm_head.weight"
    c, W, dw = _load("tied3b", 0)
    assert dw.resolve_name("lm_head.weight") == "model.language_model.embed_tokens.weight"
    c, W, dw = _load("tiny_q3", 0)
    assert dw.resolve_name("visual.pos_embed.weight") == "model.visual.pos_embed.weight"
    assert dw.resolve_name("model.layers.0.self_attn.q_norm.weight") == "model.language_model.layers.0.self_attn.q_norm.weight"


def test_bad_input_raises_before_anything_is_written():
    c, W, dw = _load("tiny", 0)
    before = {k: v.clone() for k, v in dw.t.items()}
    good = ("model.language_model.layers.0.mlp.up_proj.weight", W["model.language_model.layers.0.mlp.up_proj.weight"] + 1)
    with pytest.raises(KeyError, match="no_such.weight"):
        dw.load_weights([good, ("model.language_model.no_such.weight", torch.zeros(4))])
    with pytest.raises(ValueError, match="shape"):
        dw.load_weights([good, ("model.language_model.layers.0.mlp.down_proj.weight", torch.zeros(3, 3))])
    with pytest.raises(ValueError):
        dw.load_weights([good, ("model.language_model.norm.weight", torch.zeros(128, dtype=torch.int32))])
    with pytest.raises(ValueError):
        dw.load_weights([good, ("model.language_model.norm.weight", torch.zeros(128, dtype=torch.float16))])
    with pytest.raises(KeyError):
        _load("tied3b", 0)[2].resolve_name("lm_head.bias")
    for k, v in dw.t.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k


@pytest.mark.parametrize("fix", list(FIXTURES))
def test_plan_replayed_on_cpu_gives_a_fresh_load(fix):
    """The plan's launches, restated with the torch packers, turn seed A into the bytes of a fresh load of seed B."""
    c, WA, dw = _load(fix, 0, fp8=True)
    _, WB, fresh = _load(fix, 1, fp8=True)
    _replay(dw, [(("visual." + k[len("model.visual."):]) if k.startswith("model.visual.") else k, v) for k, v in WB.items()])
    for k, v in fresh.t.items():
        assert torch.equal(dw.t[k].view(torch.uint8), v.view(torch.uint8)), k


def test_partial_replay_touches_only_its_rows():
    c, WA, dw = _load("medium", 0, fp8=True)
    before = {k: v.clone() for k, v in dw.t.items()}
    name = "model.language_model.layers.1.mlp.up_proj.weight"
    new = fm.make_weights(fm.medium_config(), 1)[name]
    _replay(dw, [(name, new)])
    WA[name] = new
    fresh = DeviceWeights(c, getter_from_dict(WA), "cpu", fp8_decode=True)
    changed = set()
    for k, v in fresh.t.items():
        assert torch.equal(dw.t[k].view(torch.uint8), v.view(torch.uint8)), k
        if not torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)):
            changed.add(k)
    assert changed == {"l1.gu_w", "l1.gu_wp", "l1.gu_w8", "l1.gu_w8s", "l1.gu_w8p"}


def test_layout_the_kernel_cannot_rewrite_still_loads_and_is_refused_by_name():
    """A vocabulary that is not a multiple of 16 loads as before (no fragment image of the head); its embedding and head are
    recorded as unsupported for in-place update and refused before anything is written, the other weights stay updatable."""
    from open_o3_video_amd._lib import O3VError
    cfg = fm.tiny_config()
    cfg["text_config"] = dict(cfg["text_config"], vocab_size=500)
    W = fm.make_weights(cfg, 0)
    c = O3VConfig.from_dict(cfg)
    dw = DeviceWeights(c, getter_from_dict(W), "cpu", fp8_decode=True)
    assert dw.update_plan["lm_head.weight"].unsupported and dw.update_plan["model.language_model.embed_tokens.weight"].unsupported
    assert not dw.update_plan["model.language_model.layers.0.mlp.up_proj.weight"].unsupported
    with pytest.raises(O3VError, match="lm_head"):
        dw.load_weights([("lm_head.weight", W["lm_head.weight"])])
