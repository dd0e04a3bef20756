"""Host side of the shared-prefix group ("several questions about one video" as ONE engine call): the layout helper against
rope_index / decode_positions of every un-padded row, plan_decode's `suffix`, descriptor word 7 of prefill_tiles, the façade's
grouping over an engine that records its calls, and the argument checks of the C entry points.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import fixture_models as fm
from open_o3_video_amd import _lib, indexing
from open_o3_video_amd.engine import plan_decode

IMG, VID, PAD = 500, 501, 511     # placeholder / pad ids of the fixture configs


def _rect(rows, pad=PAD):
    L = max(len(r) for r in rows)
    ids = np.asarray([[pad] * (L - len(r)) + list(r) for r in rows], dtype=np.int64)
    mask = np.asarray([[0] * (L - len(r)) + [1] * len(r) for r in rows], dtype=np.int64)
    return ids, mask


def _check_against_rows(rows, P, n_new, rope_kw):
    """the layout of `rows` (lists of ids) equals rope_index / decode_positions of every row taken alone"""
    ids, mask = _rect(rows)
    lay = indexing.shared_prefix_layout(ids, mask, P, n_new, IMG, VID, PAD, **rope_kw)
    lens = [len(r) - P for r in rows]
    Lmax = max(lens)
    assert lay.own_lo.dtype == np.int32 and lay.own_lo.tolist() == [Lmax - n for n in lens]
    assert lay.prefix_ids.tolist() == [list(rows[0][:P])]
    assert lay.suffix_ids.shape == (len(rows), Lmax) and lay.suffix_pos.shape == (3, len(rows), Lmax)
    kw = {k: v for k, v in rope_kw.items() if k != "image_grid_thw"}
    for b, r in enumerate(rows):
        pos, dl = indexing.rope_index(np.asarray([r]), None, rope_kw.get("image_grid_thw"), IMG, video_token_id=VID, **kw)
        lo = int(lay.own_lo[b])
        assert lay.suffix_ids[b, lo:].tolist() == list(r[P:]) and (lay.suffix_ids[b, :lo] == PAD).all()
        assert np.array_equal(lay.prefix_pos[:, 0], pos[:, 0, :P])
        assert np.array_equal(lay.suffix_pos[:, b, lo:], pos[:, 0, P:]) and (lay.suffix_pos[:, b, :lo] == 0).all()
        assert np.array_equal(lay.decode_pos[:, b], indexing.decode_positions(np.ones((1, len(r))), dl, n_new)[:, 0])
        assert lay.deltas[b] == dl[0]
    return lay


def test_layout_hand_worked_image_prefix():
    # one image of grid (1, 4, 6): 2 x 3 merged tokens at positions t = 2, h = 2..3, w = 2..4; the text behind it starts at 2 + 3 = 5
    pre = [7, 8] + [IMG] * 6 + [9]
    rows = [pre + [20, 21, 22], pre + [30], pre + [40, 41]]
    lay = _check_against_rows(rows, len(pre), 4, dict(image_grid_thw=[[1, 4, 6]]))
    assert lay.own_lo.tolist() == [0, 2, 1]
    assert lay.suffix_ids.tolist() == [[20, 21, 22], [PAD, PAD, 30], [PAD, 40, 41]]
    assert lay.prefix_pos[:, 0].tolist() == [[0, 1, 2, 2, 2, 2, 2, 2, 5], [0, 1, 2, 2, 2, 3, 3, 3, 5], [0, 1, 2, 3, 4, 2, 3, 4, 5]]
    assert lay.suffix_pos[0].tolist() == [[6, 7, 8], [0, 0, 6], [0, 6, 7]]
    # 12 / 10 / 11 tokens, delta = 9 - 12 = -3 (the image's 6 tokens advance the position by 3): first new tokens at 9, 7, 8
    assert lay.deltas.tolist() == [-3, -3, -3]
    assert lay.decode_pos[0].tolist() == [[9, 10, 11, 12], [7, 8, 9, 10], [8, 9, 10, 11]]
    assert (lay.decode_pos[1] == lay.decode_pos[0]).all() and (lay.decode_pos[2] == lay.decode_pos[0]).all()


@pytest.mark.parametrize("mode", ["tf5", "pinned"])
def test_layout_video_prefix(mode):
    # a video of 3 temporal patches at 2 seconds each (tokens_per_second 2): the t axis runs ahead of the text that follows
    pre = [3] + [VID] * (3 * 2 * 2) + [4, 5]
    rows = [pre + [60], pre + [61, 62, 63, 64, 65], pre + [66, 67]]
    _check_against_rows(rows, len(pre), 3, dict(video_grid_thw=[[3, 4, 4]], second_per_grid_ts=[2.0], tokens_per_second=2, mode=mode))
    # P may end right behind the last visual token as well
    _check_against_rows(rows, len(pre) - 2, 3, dict(video_grid_thw=[[3, 4, 4]], second_per_grid_ts=[2.0], tokens_per_second=2,
                                                    mode=mode))


def test_layout_qwen3vl_split_frames_and_image_plus_video():
    # Qwen3-VL: every temporal patch is a block of its own with timestamp text between them
    pre = [1, 70] + [VID] * 4 + [71] + [VID] * 4 + [2]
    rows = [pre + [80, 81], pre + [82], pre + [83, 84, 85, 86]]
    _check_against_rows(rows, len(pre), 5, dict(video_grid_thw=[[2, 4, 4]], split_video_frames=True))
    pre = [1] + [IMG] * 2 + [5] + [VID] * 8 + [6]
    rows = [pre + [90], pre + [91, 92]]
    _check_against_rows(rows, len(pre), 2, dict(image_grid_thw=[[1, 2, 4]], video_grid_thw=[[2, 4, 4]], second_per_grid_ts=[1.0]))


def test_layout_left_padded_batch_of_one_and_padded_rows():
    pre = [7] + [IMG] * 4 + [9]
    row = pre + [20, 21]
    ids = np.asarray([[PAD, PAD, PAD] + row])
    mask = np.asarray([[0, 0, 0] + [1] * len(row)])
    lay = indexing.shared_prefix_layout(ids, mask, len(pre), 3, IMG, VID, PAD, image_grid_thw=[[1, 4, 4]])
    assert lay.own_lo.tolist() == [0] and lay.suffix_ids.tolist() == [[20, 21]] and lay.prefix_ids.tolist() == [pre]
    pos, dl = indexing.rope_index(np.asarray([row]), None, [[1, 4, 4]], IMG)
    assert np.array_equal(lay.prefix_pos, pos[:, :, :len(pre)]) and np.array_equal(lay.suffix_pos, pos[:, :, len(pre):])
    assert np.array_equal(lay.decode_pos, indexing.decode_positions(mask, dl, 3))
    # a missing mask is all ones; 1-D ids are one row
    lay1 = indexing.shared_prefix_layout(np.asarray(row), None, len(pre), 3, IMG, VID, PAD, image_grid_thw=[[1, 4, 4]])
    assert all(np.array_equal(a, b) for a, b in zip(lay, lay1))


def test_layout_refusals():
    pre = [7] + [IMG] * 4 + [9]
    kw = dict(image_grid_thw=[[1, 4, 4]])
    ok = _rect([pre + [20], pre + [21, 22]])
    indexing.shared_prefix_layout(*ok, len(pre), 2, IMG, VID, PAD, **kw)
    with pytest.raises(ValueError, match="differs from row 0"):
        indexing.shared_prefix_layout(*_rect([pre + [20], [8] + pre[1:] + [21]]), len(pre), 2, IMG, VID, PAD, **kw)
    with pytest.raises(ValueError, match="differs from row 0"):       # P reaches into the differing text
        indexing.shared_prefix_layout(*_rect([pre + [20, 5], pre + [21, 5]]), len(pre) + 1, 2, IMG, VID, PAD, **kw)
    with pytest.raises(ValueError, match="placeholder behind"):
        indexing.shared_prefix_layout(*ok, 3, 2, IMG, VID, PAD, **kw)
    with pytest.raises(ValueError, match="placeholder behind"):
        indexing.shared_prefix_layout(*_rect([pre + [20], pre + [VID]]), len(pre), 2, IMG, VID, PAD, **kw)
    for P in (0, -1):
        with pytest.raises(ValueError, match="at least 1"):
            indexing.shared_prefix_layout(*ok, P, 2, IMG, VID, PAD, **kw)
    with pytest.raises(ValueError, match="nothing behind"):           # a row that IS the prefix has no token for its first logits
        indexing.shared_prefix_layout(*_rect([pre + [20], pre]), len(pre), 2, IMG, VID, PAD, **kw)


# ------------------------------------------------------------------------------------------------------------------ plan_decode
GEOM = (28, 4, 128)     # 7B: heads, kv heads, head_dim


@pytest.mark.parametrize("B", [2, 3, 5, 8, 32])
@pytest.mark.parametrize("S,mode", [(4490, "auto"), (20394, "auto"), (4490, "kernel"), (4490, "shared_read")])
def test_plan_decode_suffix(B, S, mode):
    T, Lmax = 128, 37
    base = plan_decode(*GEOM, 1, B, S, T, group_attention_mode=mode)
    plan = plan_decode(*GEOM, 1, B, S, T, group_attention_mode=mode, suffix=Lmax)
    assert plan.B == B and plan.shared_prompt and plan.Tmax == Lmax + T and plan.own_splits == (Lmax + T + 127) // 128 == 2
    # the group, sub-group and form are those of B completions of one prompt
    assert plan.group == base.group and (plan.nsplit < 0) == (base.nsplit < 0) and plan.want_sync == base.want_sync
    sub = max(d for d in range(1, B + 1) if B % d == 0 and d <= 4 and d * 7 <= 64)
    kernel = sub > 1 and (mode == "kernel" or (mode == "auto" and (S >= 8192 or B >= 16)))
    assert plan.group == (sub if kernel else B) and (plan.nsplit > 0) == kernel
    if kernel:
        assert 1 <= plan.nsplit <= 64 - plan.own_splits
    else:
        assert 1 <= -plan.nsplit <= 64


def test_plan_decode_suffix_zero_is_todays_plan_and_fallbacks():
    for args in ((28, 4, 128, 1, 8, 4490, 128), (28, 4, 128, 4, 1, 300, 64), (16, 2, 64, 1, 4, 100, 16), (28, 4, 128, 2, 16, 9000, 200)):
        for mode in ("auto", "kernel", "shared_read"):
            a, b = plan_decode(*args, group_attention_mode=mode), plan_decode(*args, group_attention_mode=mode, suffix=0)
            assert a == b and a._fields == b._fields
    assert plan_decode(*GEOM, 1, 8, 4490, 128) == plan_decode(*GEOM, 1, 8, 4490, 128, suffix=0)
    # not a group: head_dim 64, one row, own keys past 32 splits, group attention off -- independent rows with room for everything
    for plan in (plan_decode(16, 2, 64, 1, 5, 300, 16, suffix=9), plan_decode(*GEOM, 1, 1, 300, 16, suffix=9),
                 plan_decode(*GEOM, 1, 5, 300, 4000, suffix=97), plan_decode(*GEOM, 1, 5, 300, 16, group_attention=False, suffix=9)):
        assert not plan.shared_prompt and plan.group == 0 and plan.nsplit > 0
    assert plan_decode(*GEOM, 1, 5, 300, 4000, suffix=96).shared_prompt        # exactly 32 splits still runs as a group
    assert plan_decode(*GEOM, 1, 5, 300, 4000, suffix=96).own_splits == 32


# ------------------------------------------------------------------------------------------------------------------ prefill_tiles
@pytest.mark.parametrize("tile", [64, 128])
def test_prefill_tiles_word7(tile):
    B, S, past = 3, 150, 200
    own_lo = [0, 7, 149]
    base = indexing.prefill_tiles(B, S, [0, 0, 0], tile, past=past)
    zero = indexing.prefill_tiles(B, S, [0, 0, 0], tile, past=past, own_lo=[0, 0, 0])
    assert zero.dtype == base.dtype and zero.tobytes() == base.tobytes()
    assert indexing.prefill_tiles(2, 70, [5, 0], tile).tobytes() == indexing.prefill_tiles(2, 70, [5, 0], tile, own_lo=None).tobytes()
    t = indexing.prefill_tiles(B, S, [0, 0, 0], tile, past=past, own_lo=own_lo)
    assert t.shape == base.shape and np.array_equal(t[:, :7], base[:, :7])
    assert [int(w) for w in t[:, 7]] == [own_lo[int(b)] for b in t[:, 6]]
    assert (base[:, 7] == 0).all() and (indexing.segment_tiles([0, 70, 200])[:, 7] == 0).all()
    with pytest.raises(ValueError):
        indexing.prefill_tiles(B, S, [0, 0, 0], tile, past=0, own_lo=own_lo)        # a gap needs a prefix in front of it
    with pytest.raises(ValueError):
        indexing.prefill_tiles(B, S, [0, 0, 0], tile, past=past, own_lo=[0, 150, 0])  # a row needs one real token


# ------------------------------------------------------------------------------------------------------------------ façade
class _Tok:
    def encode(self, text, add_special_tokens=False):
        return [int(w) for w in text.replace("<|image_pad|>", " 500 ").split()]

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(i)) for i in ids)


class _Engine:
    """Records every generate call; row b of a call emits (last prompt token + 1 + step), so the outputs tell the rows apart."""
    MAX_ROWS = 32

    def __init__(self, cfg):
        self.cfg, self.calls, self.position_mode, self.dev, self.weights_version = cfg, [], "tf5", torch.device("cpu"), 0

    def generate(self, input_ids, attention_mask=None, max_new_tokens=16, **kw):
        from open_o3_video_amd.engine import GenerateOutput
        ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.int64)
        self.calls.append(dict(kw, ids=ids.tolist(), mask=np.asarray(attention_mask).tolist()))
        gen = ids[:, -1:] + 1 + torch.arange(max_new_tokens)[None]
        tm = {"shared_prefix_rows": ids.shape[0]} if kw.get("shared_prefix_len") else {}
        return GenerateOutput(sequences=torch.cat([ids, gen], 1), margins=None, n_steps=max_new_tokens, timings=tm)


def _llm(**kw):
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.vllm_api import LLM
    eng = _Engine(O3VConfig.from_dict(fm.tiny_config()))
    llm = LLM(engine=eng, tokenizer=_Tok(), **kw)
    # visual tokens without a GPU: one merged token per image, keyed by the frame's first pixel
    llm._frames = lambda mm: None if not mm else mm["image"]
    llm._visual_tokens = lambda fr: (torch.full((fr.shape[0], 4), float(fr[0, 0, 0, 0])), ("image", float(fr[0, 0, 0, 0])))
    llm.image_factor = 1
    return llm, eng


def _req(video, tail):
    frames = torch.full((1, 3, 1, 1), float(video))
    return {"prompt": f"1 2 <|image_pad|> 3 {tail}", "multi_modal_data": {"image": frames}}


def test_shared_prefix_groups_function():
    from open_o3_video_amd.vllm_api import shared_prefix_groups
    pre = [1, 2, 500, 500, 3]
    ids = [pre + [10, 11], pre + [10, 12, 13], [1, 2, 500, 500, 4, 9], pre + [14], [5, 6, 7], [5, 6, 8], pre + [10]]
    keys = ["a", "a", "b", "a", "t", "t", "c"]
    groups, rest = shared_prefix_groups(ids, keys, (500, 501))
    assert groups == [(5, [0, 1, 3]), (2, [4, 5])] and rest == [2, 6]
    # the common prefix is capped so that every request keeps a token: [.., 10] against [.., 10, 11]
    assert shared_prefix_groups([pre + [10], pre + [10, 11]], ["a", "a"], (500, 501)) == ([(5, [0, 1])], [])
    # it must cover every visual token: rows over one key that differ inside the frame block go the ordinary way
    assert shared_prefix_groups([[1, 500, 500, 9], [1, 500, 7, 9]], ["a", "a"], (500, 501)) == ([], [0, 1])
    assert shared_prefix_groups([[500, 500, 9], [500, 500]], ["a", "a"], (500, 501)) == ([], [0, 1])


def test_facade_groups_requests_over_one_video():
    from open_o3_video_amd.vllm_api import SamplingParams
    sp = SamplingParams(temperature=0.0, max_tokens=3)
    reqs = [_req(1, "10 11"), _req(2, "20"), _req(1, "12"), _req(1, "13 14 15"), _req(3, "30"), _req(1, "16"), _req(1, "17 18")]
    llm, eng = _llm(share_video_prefix=True)
    outs = llm.generate(reqs, sp)
    assert llm.shared_prefix_calls == 1 and llm.shared_prefix_rows == 5
    shared = [c for c in eng.calls if c.get("shared_prefix_len")]
    assert len(shared) == 1 and len(eng.calls) == 2
    c = shared[0]
    assert c["shared_prefix_len"] == 4 and c["prefix_key"] == (("image", 1.0),)       # "1 2 <pad> 3": everything up to the question
    assert [r[-1] for r in c["ids"]] == [11, 12, 15, 16, 18] and c["row_ids"] == [0, 2, 3, 5, 6]
    assert c["vis_embeds"].shape[0] == 1 and c["image_grid_thw"].shape == (1, 3)     # ONE row's visual inputs
    other = [c for c in eng.calls if not c.get("shared_prefix_len")][0]
    assert [r[-1] for r in other["ids"]] == [20, 30] and other["row_ids"] == [1, 4] and other["vis_embeds"].shape[0] == 2
    # input order, the old path's request ids, every row's own continuation
    assert [o.request_id for o in outs] == [str(i) for i in range(7)]
    assert [o.outputs[0].token_ids[0] for o in outs] == [12, 21, 13, 16, 31, 17, 19]
    # flag off: the untouched path -- one call, the rows in input order, no shared keyword
    llm0, eng0 = _llm()
    outs0 = llm0.generate(reqs, sp)
    assert len(eng0.calls) == 1 and "shared_prefix_len" not in eng0.calls[0] and eng0.calls[0]["row_ids"] == list(range(7))
    assert llm0.shared_prefix_calls == 0 and llm0.shared_prefix_rows == 0
    assert [(o.request_id, o.outputs[0].token_ids, o.prompt_token_ids) for o in outs0] == \
        [(o.request_id, o.outputs[0].token_ids, o.prompt_token_ids) for o in outs]


def test_facade_grouping_conditions():
    from open_o3_video_amd.vllm_api import SamplingParams
    reqs = [_req(1, "10"), _req(1, "11"), _req(1, "12")]
    # n > 1 and prompt_logprobs keep the old paths
    for sp in (SamplingParams(temperature=0.0, max_tokens=2, prompt_logprobs=1), ):
        llm, eng = _llm(share_video_prefix=True)
        eng_generate = eng.generate
        eng.generate = lambda *a, **k: eng_generate(*a, **{x: y for x, y in k.items() if x != "prompt_logprobs"})
        llm.generate(reqs, sp)
        assert llm.shared_prefix_calls == 0 and all("shared_prefix_len" not in c for c in eng.calls)
    # groups larger than max_num_seqs run max_num_seqs rows at a time
    llm, eng = _llm(share_video_prefix=True, max_num_seqs=2)
    outs = llm.generate(reqs, SamplingParams(temperature=0.0, max_tokens=2))
    assert [len(c["ids"]) for c in eng.calls] == [2, 1] and llm.shared_prefix_calls == 2
    assert [o.outputs[0].token_ids[0] for o in outs] == [11, 12, 13]
    # a single request, and requests over different videos, form no group
    llm, eng = _llm(share_video_prefix=True)
    llm.generate([_req(1, "10"), _req(2, "11")], SamplingParams(temperature=0.0, max_tokens=2))
    assert llm.shared_prefix_calls == 0 and len(eng.calls) == 1


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_without_gpu():
    lib = _lib.load()
    assert hasattr(lib, "o3v_attn_decode_group_prefix_lo") and "o3v_attn_decode_group_prefix_lo" in _lib.SIGNATURES
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # o3v_attn_decode_group_prefix_lo(Q, Kc, Vc, Kpre, Vpre, cap, rpp, out, part_o, part_ml, k_lo, own_lo, B, G, Hq, Hkv, D, P, ctx,
    #                                 Tmax, nsp, scale, stream): own_lo needs the prompt entry; G = 1 only in the shared-read form
    f = lib.o3v_attn_decode_group_prefix_lo
    assert f(p, p, p, None, None, 0, 1, p, p, p, None, p, 4, 2, 8, 2, 128, 64, 70, 80, 2, 0.1, None) == _lib.ERR_ARG
    assert f(p, p, p, p, p, 64, 4, p, p, p, None, p, 4, 1, 8, 2, 128, 64, 70, 80, 2, 0.1, None) == _lib.ERR_ARG
    assert f(p, p, p, p, p, 64, 4, p, p, p, None, p, 4, 2, 8, 2, 64, 64, 70, 80, 2, 0.1, None) == _lib.ERR_SHAPE
    assert lib.o3v_attn_decode_group_prefix(p, p, p, p, p, 64, 4, p, p, p, None, 4, 1, 8, 2, 128, 64, 70, 80, 2, 0.1, None) == _lib.ERR_ARG
    # the decode state: the pair sits behind v8s, zero = off, and is refused without a group on a prompt entry or with fp8 K/V
    assert [n for n, _ in _lib.DecodeStateOwn._fields_] == ["own_past", "own_lo"]
    assert _lib.DecodeStateOwn.own_past.offset == ctypes.sizeof(_lib.DecodeState)
    assert _lib.DecodeStateOwn.own_lo.offset == ctypes.sizeof(_lib.DecodeState) + 8
    layer = _lib.LlmLayerW()
    desc = _lib.LlmDesc(hidden=64, layers=1, heads=8, kv_heads=2, head_dim=128, inter=64, vocab=32,
                        layer=ctypes.pointer(layer))

    def state(**kw):
        st = _lib.DecodeStateOwn(B=4, S=64, Tmax=32, Tnew=8, nsplit=-2, group=4, rows_per_prompt=4, prefix_cap=64, ws_bytes=0)
        for n in ("x", "kcache", "vcache", "cosT", "sinT", "logits", "seen", "cur_tok", "finished", "out_ids", "part_o", "part_ml",
                  "workspace", "sample_scratch", "kprefix", "vprefix"):
            setattr(st, n, p.value)
        for n, v in kw.items():
            setattr(st, n, v)
        return st

    def rc(st):
        return lib.o3v_llm_decode(ctypes.byref(desc), ctypes.byref(st), 0, 1, 0, None)

    # a valid state gets as far as the workspace check (no launch: ws_bytes = 0), with and without the pair
    assert not (state().own_past or state().own_lo)
    assert rc(state()) == _lib.ERR_WORKSPACE
    assert rc(state(own_past=9, own_lo=p.value)) == _lib.ERR_WORKSPACE
    assert rc(state(own_past=9)) == _lib.ERR_WORKSPACE
    assert rc(state(own_lo=p.value, kprefix=None, vprefix=None, Tmax=100)) == _lib.ERR_ARG     # no prompt entry
    assert rc(state(own_past=9, kprefix=None, vprefix=None, Tmax=100)) == _lib.ERR_ARG
    assert rc(state(own_past=9, own_lo=p.value, group=1)) == _lib.ERR_ARG                      # not a group
    assert rc(state(own_past=-1, own_lo=p.value)) == _lib.ERR_ARG
    assert rc(state(own_past=26, own_lo=p.value)) == _lib.ERR_ARG                              # own_past + Tnew > Tmax + 1
    assert rc(state(own_past=25, own_lo=p.value)) == _lib.ERR_WORKSPACE
    assert rc(state(own_past=9, own_lo=p.value, k8=p.value, v8=p.value, k8s=p.value, v8s=p.value)) == _lib.ERR_ARG   # fp8 K/V
