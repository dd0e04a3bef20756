"""Several continuations of ONE shared prefix ("one video, several questions") as a single engine call.

Kernel probes: the gap mask of o3v_attn_decode_group_prefix_lo (both forms) and of o3v_attn_tiles_prefix's descriptor word 7 with the
probe families of test_gpu_attention_edges (A key sets, B needles and decoys, C peaked inputs with that file's rounding bounds, D
poisoned memory).  Row b's logical keys are [0, P) in the prompt entry and [P, ctx) in its own cache, whose first own_lo[b] slots are
padding: visible are [k_lo, P) and [P + own_lo[b], ctx).  The gap slots and the slots below k_lo hold finite decoys (the suffix
prefill writes them; the kernels may read them and must mask them); NaN sits where that file places it.

Engine: generate(shared_prefix_len=P) on the medium fixtures (head_dim 128) against the HF goldens, the CPU oracle run row by row and
the independent-row batch; the façade's share_video_prefix."""
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
import fixture_models_q3 as fq
from test_gpu_attention_edges import (BF, FAMS, Probe, _causal_bands, _causal_edges, _group_edges, dev)  # noqa: F401 (dev: fixture)
from test_gpu_model import LOGIT_ATOL, build_engine

pytestmark = pytest.mark.gpu


def _p(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def decode_group_prefix_lo(q, kc_own, vc_own, kpre, vpre, rpp, k_lo, own_lo, G, prefix_len, ctx, nsp, scale):
    """o3v_attn_decode_group_prefix_lo on poisoned out / part_o / part_ml"""
    from open_o3_video_amd import _lib
    B, Hq, D = q.shape
    _, Hkv, Tmax, _ = kc_own.shape
    nan = lambda n, dt: torch.full((n,), float("nan"), dtype=dt, device=q.device)
    out, po, pm = nan(q.numel(), q.dtype).view(q.shape), nan(B * Hq * 64 * D, torch.float32), nan(B * Hq * 64 * 2, torch.float32)
    _lib.call("o3v_attn_decode_group_prefix_lo", _p(q), _p(kc_own), _p(vc_own), _p(kpre), _p(vpre), kpre.shape[2], rpp, _p(out), _p(po),
              _p(pm), _p(k_lo), _p(own_lo), B, G, Hq, Hkv, D, prefix_len, ctx, Tmax, nsp, float(scale), _stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# decode: o3v_attn_decode_group_prefix_lo, one-pass form (nsp > 0) and shared-read form (nsp < 0)
# ---------------------------------------------------------------------------------------------------------------------------
DECODE_LO_CASES = [
    # B, G, Hq, Hkv, P, own, own_lo per row, pad, nsp, rows_per_prompt
    (4, 4, 8, 2, 128, 40, [0, 1, 31, 39], 0, 2, 4),                    # the last row sees only its newest own key
    (3, 3, 4, 1, 32, 33, [32, 0, 17], 31, 1, 3),                       # k_lo = P - 1, a gap of exactly one tile
    (4, 2, 16, 2, 129, 300, [260, 0, 128, 255], 0, 3, 4),              # a whole own split and whole waves inside the gap
    (8, 8, 28, 4, 333, 70, [0, 5, 64, 63, 65, 1, 33, 69], 5, -3, 8),   # shared-read form
    (5, 1, 28, 4, 97, 130, [0, 129, 96, 32, 2], 40, -5, 5),            # sub-group 1
]


def _decode_lo_inputs(fam, B, G, Hq, Hkv, P, own, own_lo, pad, nsp, rpp, rnd, gap=True):
    """-> (probe, q, ko, vo, kpre, vpre): the prompt-entry layout of test_gpu_attention_edges with the rows' gaps"""
    D, ctx = 128, P + own
    scale = D ** -0.5
    lo = own_lo if gap else [0] * B
    mask = torch.zeros(B, 1, ctx, dtype=torch.bool)
    mask[:, 0, pad:] = True
    for b in range(B):
        mask[b, 0, P:P + lo[b]] = False
    edges = [[k for k in set(_group_edges(P, ctx, nsp, pad) + [P + lo[b] - 1, P + lo[b], P + lo[b] + 1]) if pad - 1 <= k < ctx and k >= 0]
             for b in range(B)]
    edges = [sorted(e) for e in edges]
    # family B: every query sees DECOY on the keys of its row's gap (one more dimension), as below k_lo
    gap_keys = [(b, j) for b in range(B) for j in range(P, P + lo[b])]
    bands = [([(b, 0) for b in range(B)], gap_keys)] if fam == "B" and gap_keys else ()
    pr = Probe(fam, B, 1, Hq, Hkv, ctx, D, mask, scale, seed=ctx * 5 + B + rnd, edges=edges, always=[[pad]] * B, lo=[pad] * B,
               sink=[[pad]] * B, bands=bands, rot=rnd * Hq + 3)
    for b in range(B):                                       # rows sharing a prompt share its K / V
        lead = (b // rpp) * rpp
        pr.K[b, :, :P], pr.V[b, :, :P] = pr.K[lead, :, :P], pr.V[lead, :, :P]
    g = torch.Generator().manual_seed(100 + rnd)
    cap, T_own = P + 3, own + 4
    kpre = torch.zeros(B // rpp, Hkv, cap, D, dtype=BF)
    vpre = torch.zeros_like(kpre)
    kpre[:, :, :P], vpre[:, :, :P] = pr.K[::rpp, :, :P], pr.V[::rpp, :, :P]
    pr.decoy_rows_(kpre[:, :, P:], vpre[:, :, P:], g)
    ko = torch.zeros(B, Hkv, T_own, D, dtype=BF)
    vo = torch.zeros_like(ko)
    ko[:, :, :own], vo[:, :, :own] = pr.K[:, :, P:], pr.V[:, :, P:]
    pr.decoy_rows_(ko[:, :, own:], vo[:, :, own:], g)
    for t in (pr.K, pr.V):                                   # the contract: what a kernel may read and must mask is finite
        for b in range(B):
            assert torch.isfinite(t[b, :, :pad].float()).all() and torch.isfinite(t[b, :, P:P + lo[b]].float()).all()
    return pr, ko, vo, kpre, vpre


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("B,G,Hq,Hkv,P,own,own_lo,pad,nsp,rpp", DECODE_LO_CASES)
def test_decode_gap_probes(dev, fam, B, G, Hq, Hkv, P, own, own_lo, pad, nsp, rpp):
    scale = 128 ** -0.5
    k_lo = torch.full((B,), pad, dtype=torch.int32, device=dev)
    lo_d = torch.tensor(own_lo, dtype=torch.int32, device=dev)
    n_edges = len(_group_edges(P, P + own, nsp, pad)) + 3
    rounds = 1 if fam != "B" else min(6, -(-n_edges // Hq))
    for rnd in range(rounds):
        pr, ko, vo, kpre, vpre = _decode_lo_inputs(fam, B, G, Hq, Hkv, P, own, own_lo, pad, nsp, rpp, rnd)
        out = decode_group_prefix_lo(pr.q[:, 0].to(dev), ko.to(dev), vo.to(dev), kpre.to(dev), vpre.to(dev), rpp, k_lo, lo_d, G, P,
                                     P + own, nsp, scale)
        pr.check(out[:, None], f"group gap P={P} own={own} own_lo={own_lo} pad={pad} nsp={nsp} G={G} round {rnd}", dev)


@pytest.mark.parametrize("B,G,Hq,Hkv,P,own,own_lo,pad,nsp,rpp", DECODE_LO_CASES)
def test_decode_zero_gap_equals_the_old_entry(dev, B, G, Hq, Hkv, P, own, own_lo, pad, nsp, rpp):
    """own_lo all zero, or NULL: bit for bit the output of o3v_attn_decode_group_prefix"""
    import kernel_ops as ops
    scale = 128 ** -0.5
    k_lo = torch.full((B,), pad, dtype=torch.int32, device=dev)
    pr, ko, vo, kpre, vpre = _decode_lo_inputs("C", B, G, Hq, Hkv, P, own, own_lo, pad, nsp, rpp, 0, gap=False)
    args = (pr.q[:, 0].to(dev), ko.to(dev), vo.to(dev), kpre.to(dev), vpre.to(dev), rpp, k_lo)
    old = ops.attn_decode_group_prefix(*args, G, P, P + own, nsp, scale, poison=True)
    zero = decode_group_prefix_lo(*args, torch.zeros(B, dtype=torch.int32, device=dev), G, P, P + own, nsp, scale)
    null = decode_group_prefix_lo(*args, None, G, P, P + own, nsp, scale)
    assert not torch.isnan(old.float()).any()
    assert torch.equal(old.view(torch.int16), zero.view(torch.int16)) and torch.equal(old.view(torch.int16), null.view(torch.int16))
    pr.check(old[:, None], f"group zero gap P={P} own={own} nsp={nsp} G={G}", dev)


# ---------------------------------------------------------------------------------------------------------------------------
# prefill: o3v_attn_tiles_prefix with descriptor word 7
# ---------------------------------------------------------------------------------------------------------------------------
PREFILL_LO_CASES = [
    # D, Hq, Hkv, G, P, L, own_lo per row, pad, rows_per_prefix
    (128, 7, 1, 3, 150, 20, [0, 7, 19], 0, 3),
    (128, 8, 2, 4, 64, 130, [0, 64, 65, 129], 13, 4),
    (128, 28, 4, 2, 4400, 90, [0, 50], 0, 2),
]


def _prefill_lo_inputs(fam, D, Hq, Hkv, G, P, L, own_lo, pad, rpp):
    T = P + L
    pads = [pad] * G
    mask = torch.zeros(G, L, T, dtype=torch.bool)
    for b in range(G):
        for i in range(L):
            mask[b, i, pad:P + i + 1] = True
        mask[b, :, P:P + own_lo[b]] = False
    edges = [sorted(set(e + [k for k in (P + own_lo[b] - 1, P + own_lo[b], P + own_lo[b] + 1) if 0 <= k < T]))
             for b, e in enumerate(_causal_edges(G, L, P, pads, T))]
    bands = ()
    if fam == "B":
        gap_keys = [(b, j) for b in range(G) for j in range(P, P + own_lo[b])]
        bands = _causal_bands(G, L, P, pads, T, mask) + ([([(b, i) for b in range(G) for i in range(L)], gap_keys)] if gap_keys else [])
    pr = Probe(fam, G, L, Hq, Hkv, T, D, mask, D ** -0.5, seed=P + L + D, edges=edges, always=[[pad]] * G, bands=bands, lo=pads,
               sink=[[pad]] * G, needle_extra=lambda b, i: [P + i, P + i - 1], unrounded_sum=True)
    for b in range(G):
        lead = (b // rpp) * rpp
        pr.K[b, :, :P], pr.V[b, :, :P] = pr.K[lead, :, :P], pr.V[lead, :, :P]
        assert torch.isfinite(pr.K[b, :, P:P + own_lo[b]].float()).all() and torch.isfinite(pr.V[b, :, P:P + own_lo[b]].float()).all()
    return pr


def _run_tiles_prefix(pr, dev, D, Hq, Hkv, G, P, L, own_lo, pad, rpp, rpt):
    import kernel_ops as ops
    from open_o3_video_amd import indexing
    cap, T2, QD = P + 3, L + 5, Hq * D
    g = torch.Generator().manual_seed(P)
    kp = torch.zeros(G // rpp, Hkv, cap, D, dtype=BF)
    vp = torch.zeros_like(kp)
    kp[:, :, :P], vp[:, :, :P] = pr.K[::rpp, :, :P], pr.V[::rpp, :, :P]
    pr.decoy_rows_(kp[:, :, P:], vp[:, :, P:], g)
    ko = torch.zeros(G, Hkv, T2, D, dtype=BF)
    vo = torch.zeros_like(ko)
    ko[:, :, :L], vo[:, :, :L] = pr.K[:, :, P:], pr.V[:, :, P:]
    pr.decoy_rows_(ko[:, :, L:], vo[:, :, L:], g)
    tiles = torch.from_numpy(indexing.prefill_tiles(G, L, [pad] * G, rpt, past=P, own_lo=own_lo)).to(dev)
    out = torch.empty(G * L + 16, QD, dtype=BF, device=dev)
    ops.attn_tiles_prefix(pr.q.reshape(G * L, QD).to(dev), ko.to(dev), vo.to(dev), kp.to(dev), vp.to(dev), cap * D, Hkv * cap * D, P, rpp,
                          tiles, Hq, Hq // Hkv, D, QD, D, T2 * D, Hkv * T2 * D, D, T2 * D, Hkv * T2 * D, out, QD, D ** -0.5,
                          rows_per_tile=rpt, poison=True)
    assert torch.isnan(out[G * L:].float()).all(), "rows past the batch were written"
    return out[:G * L].view(G, L, Hq, D)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("rpt", [64, 128])
@pytest.mark.parametrize("D,Hq,Hkv,G,P,L,own_lo,pad,rpp", PREFILL_LO_CASES)
def test_prefill_gap_probes(dev, fam, rpt, D, Hq, Hkv, G, P, L, own_lo, pad, rpp):
    pr = _prefill_lo_inputs(fam, D, Hq, Hkv, G, P, L, own_lo, pad, rpp)
    out = _run_tiles_prefix(pr, dev, D, Hq, Hkv, G, P, L, own_lo, pad, rpp, rpt)
    # query rows below own_lo are padding: they carry no meaning and must only be finite
    for b in range(G):
        assert torch.isfinite(out[b, :own_lo[b]].float()).all(), f"row {b}: padding query rows not finite"
        pr.qvalid[b, :own_lo[b]] = False
    pr.check(out, f"prefix gap P={P} L={L} own_lo={own_lo} pad={pad} D={D} tile={rpt}", dev)


@pytest.mark.parametrize("rpt", [64, 128])
@pytest.mark.parametrize("D,Hq,Hkv,G,P,L,own_lo,pad,rpp", PREFILL_LO_CASES)
def test_prefill_zero_word7_is_the_kernel_without_a_gap(dev, rpt, D, Hq, Hkv, G, P, L, own_lo, pad, rpp):
    """word 7 all zero: the bits of the same attention through o3v_attn_tiles on one contiguous cache per row (the instantiation
    that never reads the word), and within the bound of family C"""
    import kernel_ops as ops
    from open_o3_video_amd import indexing
    zero = [0] * G
    pr = _prefill_lo_inputs("C", D, Hq, Hkv, G, P, L, zero, pad, rpp)
    out = _run_tiles_prefix(pr, dev, D, Hq, Hkv, G, P, L, zero, pad, rpp, rpt)
    out_none = _run_tiles_prefix(pr, dev, D, Hq, Hkv, G, P, L, None, pad, rpp, rpt)
    T, QD = P + L, Hq * D
    tiles = torch.from_numpy(indexing.prefill_tiles(G, L, [pad] * G, rpt, past=P)).to(dev)
    flat = torch.empty(G * L, QD, dtype=BF, device=dev)
    ops.attn_tiles(pr.q.reshape(G * L, QD).to(dev), pr.K.to(dev), pr.V.to(dev), tiles, Hq, Hq // Hkv, D, QD, D, T * D, Hkv * T * D, D, T * D,
                   Hkv * T * D, flat, QD, D ** -0.5, rows_per_tile=rpt, poison=True)
    assert torch.equal(out.reshape(G * L, QD).view(torch.int16), flat.view(torch.int16))
    assert torch.equal(out.view(torch.int16), out_none.view(torch.int16))
    pr.check(out, f"prefix zero word 7 P={P} L={L} tile={rpt}", dev)


# ---------------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------------
N_NEW = 16
# Altered text tails of the medium golden prompt behind its frame block (its own tail: the 6 tokens 55..60), rows 1..3: (length,
# seed) of np.random.RandomState(seed).randint(10, 3990, size=length).  Chosen by a seeded search on the CPU oracle (fp32,
# repetition penalty 1.05): per length the first seed from 0 whose top-1 / top-2 margin of the processed scores exceeds
# 2 * LOGIT_ATOL at every one of the 16 steps -- as tools/make_golden.py:search_case picks the golden cases (the `medium` fixture
# re-checks the margins).  Shorter and longer than the golden's tail: Lmax = 8, own_lo = [2, 4, 5, 0].  (No single-token tail has
# such margins: all 3980 were tried.)  OTHER_TAIL: the same search for the golden prompt's frames in reverse order (another video).
TAILS = [(4, 1522), (3, 23254), (8, 924)]
OTHER_TAIL = (6, 3153)


def _tail(n, seed):
    return np.random.RandomState(seed).randint(10, 3990, size=n).tolist()


def _rect(rows, pad):
    L = max(len(r) for r in rows)
    return (np.asarray([[pad] * (L - len(r)) + r for r in rows], dtype=np.int64),
            np.asarray([[0] * (L - len(r)) + [1] * len(r) for r in rows], dtype=np.int64))


@pytest.fixture(scope="module")
def medium(dev, golden_dir):
    """engine, golden, the four rows (row 0 = the golden prompt), P, and the oracle's ids / first logits of rows 1..3 run one by one
    on the CPU (computed once)"""
    from oracle import model_ref
    g = np.load(os.path.join(golden_dir, "g7_medium.npz"))
    cfg = fm.medium_config()
    W = fm.make_weights(cfg, 2)
    ids = g["input_ids"][0].tolist()
    P = max(i for i, t in enumerate(ids) if t == cfg["vision_end_token_id"]) + 1          # right behind the frame block
    rows = [ids] + [ids[:P] + _tail(n, s) for n, s in TAILS]
    pv = torch.from_numpy(g["pixel_values"])
    ref_ids, ref_first = [g["bf16_ids_rp105"][0, len(ids):].tolist()], [torch.from_numpy(g["f32_step_logits"][0, 0])]
    for row in rows[1:]:
        seq, lg = model_ref.generate(W, cfg, [row], None, pv, g["grid"], N_NEW, dtype=torch.float32, pad_token_id=cfg["pad_token_id"],
                                     rep_penalty=1.05, return_logits=True)
        margins = []
        for t in range(N_NEW):
            top = model_ref.repetition_penalty(lg[:, t], seq[:, :len(row) + t], 1.05).topk(2, -1).values[0]
            margins.append(float(top[0] - top[1]))
        assert min(margins) > 2 * LOGIT_ATOL, f"tail {row[P:]}: oracle margin {min(margins):.3f}: not a robust case"
        ref_ids.append(seq[0, len(row):].tolist())
        ref_first.append(lg[0, 0])
    eng = build_engine(cfg, W)
    kw = dict(pixel_values=pv, image_grid_thw=g["grid"], max_new_tokens=N_NEW, repetition_penalty=1.05, pad_token_id=cfg["pad_token_id"])
    return dict(eng=eng, g=g, cfg=cfg, W=W, rows=rows, P=P, ref_ids=ref_ids, ref_first=ref_first, kw=kw)


def _new_ids(out, n_rows):
    return [out.sequences[b, -out.n_steps:].tolist() for b in range(n_rows)]


@pytest.mark.parametrize("mode", ["kernel", "shared_read"])
def test_engine_group_equals_golden_and_oracle(medium, mode):
    """row 0 reproduces the HF golden exactly, rows 1..3 the CPU oracle's ids, in both forms of the group attention"""
    eng, cfg = medium["eng"], medium["cfg"]
    ids, mask = _rect(medium["rows"], cfg["pad_token_id"])
    eng.group_attention_mode = mode
    try:
        out = eng.generate(ids, mask, shared_prefix_len=medium["P"], **medium["kw"])
    finally:
        eng.group_attention_mode = "auto"
    assert out.timings["shared_prefix_rows"] == 4 and out.timings["prefix_tokens_reused"] == 0
    assert out.sequences.shape == (4, ids.shape[1] + N_NEW) and np.array_equal(out.sequences[:, :ids.shape[1]].cpu().numpy(), ids)
    got = _new_ids(out, 4)
    assert got[0] == medium["ref_ids"][0], "row 0 is the golden prompt: bf16_ids_rp105"
    for b in range(1, 4):
        assert got[b] == medium["ref_ids"][b], (b, got[b], medium["ref_ids"][b])


def test_engine_first_step_logits(medium):
    eng, cfg = medium["eng"], medium["cfg"]
    ids, mask = _rect(medium["rows"], cfg["pad_token_id"])
    eng._debug_keep = True
    try:
        eng.generate(ids, mask, shared_prefix_len=medium["P"], **dict(medium["kw"], max_new_tokens=1))
        logits = eng._debug_last["logits"].float().cpu()        # one step: the buffer still holds the logits it sampled from
    finally:
        eng._debug_keep = False
        eng._debug_last = None
    for b in range(4):
        err = (logits[b] - medium["ref_first"][b]).abs().max().item()
        print(f"row {b}: first-step logits max|err| vs oracle fp32: {err:.4f}")
        assert err < LOGIT_ATOL, (b, err)


def test_engine_group_against_independent_batch_and_prefix_reuse(medium):
    eng, cfg, g, P = medium["eng"], medium["cfg"], medium["g"], medium["P"]
    tc = cfg["text_config"]
    ids, mask = _rect(medium["rows"], cfg["pad_token_id"])
    grp = eng.generate(ids, mask, shared_prefix_len=P, **medium["kw"])
    kw4 = dict(medium["kw"], pixel_values=torch.cat([medium["kw"]["pixel_values"]] * 4), image_grid_thw=np.tile(g["grid"], (4, 1)))
    ind = eng.generate(ids, mask, **kw4)
    assert "shared_prefix_rows" not in ind.timings and torch.equal(grp.sequences, ind.sequences)
    Lmax = max(len(r) for r in medium["rows"]) - P
    per_slot = tc["num_hidden_layers"] * tc["num_key_value_heads"] * 128 * 2 * 2      # K and V, bf16, every layer
    assert grp.timings["kv_cache_bytes"] == per_slot * (P + 4 * (Lmax + N_NEW))        # ONE prefix + the rows' own slots
    assert ind.timings["kv_cache_bytes"] == per_slot * 4 * (ids.shape[1] + N_NEW) > grp.timings["kv_cache_bytes"]
    # a second call over the same video reuses the stored prefix, also when the first one stored it
    eng.drop_prefix_cache()
    try:
        a = eng.generate(ids, mask, shared_prefix_len=P, prefix_key="video-1", **medium["kw"])
        b = eng.generate(ids[1:], mask[1:], shared_prefix_len=P, prefix_key="video-1", **medium["kw"])
        assert a.timings["prefix_tokens_reused"] == 0 and b.timings["prefix_tokens_reused"] == P
        assert torch.equal(a.sequences, grp.sequences) and torch.equal(b.sequences, grp.sequences[1:])
        assert b.timings["shared_prefix_rows"] == 3 and eng._last_prompt is None
    finally:
        eng.drop_prefix_cache()


def test_engine_refuses_rows_that_do_not_share(medium):
    eng, cfg, P = medium["eng"], medium["cfg"], medium["P"]
    rows = medium["rows"]
    bad = [rows[0], rows[1][:3] + [rows[1][3] + 1] + rows[1][4:]]
    with pytest.raises(ValueError):
        eng.generate(*_rect(bad, cfg["pad_token_id"]), shared_prefix_len=P, **medium["kw"])
    with pytest.raises(ValueError):
        eng.generate(*_rect(rows[:2], cfg["pad_token_id"]), shared_prefix_len=P - 3, **medium["kw"])       # a placeholder behind P
    with pytest.raises(ValueError):
        eng.generate(*_rect(rows[:2], cfg["pad_token_id"]), shared_prefix_len=P, num_return_sequences=2, **medium["kw"])


def test_engine_fallbacks(medium, golden_dir):
    # fp8 K/V asked for: a group call still decodes on bf16 K/V
    eng, cfg, P = medium["eng"], medium["cfg"], medium["P"]
    ids, mask = _rect(medium["rows"], cfg["pad_token_id"])
    eng.kv_cache_dtype = "fp8"
    try:
        out = eng.generate(ids, mask, shared_prefix_len=P, **medium["kw"])
    finally:
        eng.kv_cache_dtype = "bf16"
    assert out.timings["kv_cache_dtype"] == "bf16" and out.timings["shared_prefix_rows"] == 4
    assert _new_ids(out, 4) == medium["ref_ids"]
    # group attention off, one row, prompt log-probs: independent rows on the one row's visual inputs, replicated
    eng.group_attention = False
    try:
        off = eng.generate(ids, mask, shared_prefix_len=P, **medium["kw"])
    finally:
        eng.group_attention = True
    assert off.timings["shared_prefix_rows"] == 0 and _new_ids(off, 4) == medium["ref_ids"]
    one = eng.generate(ids[:1, -len(medium["rows"][0]):], None, shared_prefix_len=P, **medium["kw"])
    assert one.timings["shared_prefix_rows"] == 0 and _new_ids(one, 1) == medium["ref_ids"][:1]
    plp = eng.generate(ids, mask, shared_prefix_len=P, prompt_logprobs=1, **medium["kw"])
    assert plp.timings["shared_prefix_rows"] == 0 and plp.prompt_logprobs is not None and _new_ids(plp, 4) == medium["ref_ids"]
    # head_dim != 128 (tiny fixture): the same ids as the old path
    g = np.load(os.path.join(golden_dir, "g6_tiny.npz"))
    tcfg = fm.tiny_config()
    teng = build_engine(tcfg, fm.make_weights(tcfg, 0))
    tids = g["input_ids"][0].tolist()
    tP = max(i for i, t in enumerate(tids) if t == tcfg["vision_end_token_id"]) + 1
    trows = [tids, tids[:tP] + [33, 44], tids[:tP] + [55, 66, 77, 88, 99, 111, 122, 133]]
    tkw = dict(max_new_tokens=8, pad_token_id=tcfg["pad_token_id"])
    pv = torch.from_numpy(g["pixel_values"])
    a = teng.generate(*_rect(trows, tcfg["pad_token_id"]), shared_prefix_len=tP, pixel_values=pv, image_grid_thw=g["grid"], **tkw)
    b = teng.generate(*_rect(trows, tcfg["pad_token_id"]), pixel_values=torch.cat([pv] * 3), image_grid_thw=np.tile(g["grid"], (3, 1)), **tkw)
    assert a.timings["shared_prefix_rows"] == 0 and torch.equal(a.sequences, b.sequences)


def test_engine_options(medium):
    """sampling (reproducible per (seed, row_ids)), logprobs, and the fp8 decode weight rows at 4 rows"""
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    eng, cfg, P = medium["eng"], medium["cfg"], medium["P"]
    ids, mask = _rect(medium["rows"], cfg["pad_token_id"])
    skw = dict(medium["kw"], do_sample=True, temperature=1.0, top_p=0.9, max_new_tokens=8)
    a = eng.generate(ids, mask, shared_prefix_len=P, seed=7, row_ids=[10, 11, 12, 13], **skw)
    b = eng.generate(ids, mask, shared_prefix_len=P, seed=7, row_ids=[10, 11, 12, 13], **skw)
    c = eng.generate(ids, mask, shared_prefix_len=P, seed=8, row_ids=[10, 11, 12, 13], **skw)
    d = eng.generate(ids, mask, shared_prefix_len=P, seed=7, row_ids=[20, 21, 22, 23], **skw)
    assert torch.equal(a.sequences, b.sequences), "the same (seed, row_ids) draw the same tokens"
    assert not torch.equal(a.sequences, c.sequences) and not torch.equal(a.sequences, d.sequences)
    assert a.timings["shared_prefix_rows"] == 4
    lp = eng.generate(ids, mask, shared_prefix_len=P, logprobs=2, **medium["kw"])
    assert _new_ids(lp, 4) == medium["ref_ids"]
    assert lp.logprobs.token.shape == (4, N_NEW) and lp.logprobs.top.shape == (4, N_NEW, 2) and lp.logprobs.top_ids.shape == (4, N_NEW, 2)
    assert torch.isfinite(lp.logprobs.token).all() and (lp.logprobs.token <= 0).all()
    assert torch.equal(lp.logprobs.top_ids[:, :, 0].cpu().long(), lp.sequences[:, -N_NEW:].cpu()), "greedy: the token is the top-1"
    # fp8 decode rows: the group against the independent rows of the same engine, up to the first step the margin leaves open
    c8 = O3VConfig.from_dict(cfg)
    e8 = O3VEngine(c8, DeviceWeights(c8, getter_from_dict(medium["W"]), "cuda", fp8_decode=True))
    g8 = e8.generate(ids, mask, shared_prefix_len=P, **medium["kw"])
    kw4 = dict(medium["kw"], pixel_values=torch.cat([medium["kw"]["pixel_values"]] * 4), image_grid_thw=np.tile(medium["g"]["grid"], (4, 1)))
    i8 = e8.generate(ids, mask, **kw4)
    assert g8.timings["shared_prefix_rows"] == 4
    for r in range(4):
        x, y, m = g8.sequences[r, -N_NEW:].tolist(), i8.sequences[r, -N_NEW:].tolist(), i8.margins[r].tolist()
        k = 0
        while k < N_NEW and x[k] == y[k]:
            k += 1
        assert k == N_NEW or m[k] < 2 * LOGIT_ATOL, (r, k, m[k])


def test_engine_qwen3vl_group(dev, golden_dir):
    """Qwen3-VL medium (head_dim 128): DeepStack rows in the prefix, q/k norm in the suffix prefill; row 0 is the golden prompt"""
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    g = np.load(os.path.join(golden_dir, "g13_q3_medium.npz"))
    cfg = fq.medium_q3_config()
    c = O3VConfig.from_dict(cfg)
    eng = O3VEngine(c, DeviceWeights(c, getter_from_dict(fq.make_weights(cfg, 2)), "cuda"))
    ids = g["input_ids"][0].tolist()
    P = max(i for i, t in enumerate(ids) if t == cfg["vision_end_token_id"]) + 1
    rows = [ids, ids[:P] + _tail(2, 0), ids[:P] + _tail(len(ids) - P + 3, 1)]        # one shorter, one longer than the golden's tail
    n_new = g["bf16_ids"].shape[1] - len(ids)
    kw = dict(pixel_values=torch.from_numpy(g["pixel_values"]), image_grid_thw=g["grid"], max_new_tokens=n_new,
              pad_token_id=cfg["pad_token_id"])
    for mode in ("kernel", "shared_read"):
        eng.group_attention_mode = mode
        out = eng.generate(*_rect(rows, cfg["pad_token_id"]), shared_prefix_len=P, **kw)
        assert out.timings["shared_prefix_rows"] == 3
        assert out.sequences[0, -n_new:].tolist() == g["bf16_ids"][0, len(ids):].tolist(), mode


# ---------------------------------------------------------------------------------------------------------------------------
# façade
# ---------------------------------------------------------------------------------------------------------------------------
def _prompt_text(cfg, ids):
    """the prompt text of token ids with ONE <|image_pad|> per frame, as the eval scripts write it"""
    words, i = [], 0
    while i < len(ids):
        if ids[i] == cfg["image_token_id"]:
            words.append("<|image_pad|>")
            while i < len(ids) and ids[i] == cfg["image_token_id"]:
                i += 1
            continue
        words.append({cfg["vision_start_token_id"]: "<|vision_start|>", cfg["vision_end_token_id"]: "<|vision_end|>"}.get(ids[i], f"w{ids[i]}"))
        i += 1
    return " ".join(words)


def test_facade_share_video_prefix(medium):
    """five prompts over one video and one over another: outputs in input order, ids equal to the flag-off run"""
    from open_o3_video_amd.vllm_api import LLM, SamplingParams
    from test_gpu_facades import StubTokenizer
    eng, cfg, g, rows, P = medium["eng"], medium["cfg"], medium["g"], medium["rows"], medium["P"]
    frames = torch.from_numpy(g["frames"])
    other = torch.flip(frames, dims=[0])                                 # another video: the frames in reverse order
    other_row = rows[0][:P] + _tail(*OTHER_TAIL)
    reqs = [{"prompt": _prompt_text(cfg, r), "multi_modal_data": {"image": frames}} for r in rows + [rows[0]]]
    reqs.insert(2, {"prompt": _prompt_text(cfg, other_row), "multi_modal_data": {"image": other}})
    sp = SamplingParams(temperature=0.0, repetition_penalty=1.05, max_tokens=N_NEW, stop_token_ids=[])
    mk = lambda **kw: LLM(engine=eng, tokenizer=StubTokenizer(cfg), limit_mm_per_prompt={"image": 32}, max_model_len=4096, **kw)
    eng.drop_prefix_cache()
    try:
        on, off = mk(share_video_prefix=True), mk()
        a, b = on.generate(reqs, sp), off.generate(reqs, sp)
    finally:
        eng.drop_prefix_cache()
    assert on.shared_prefix_calls == 1 and on.shared_prefix_rows == 5 and off.shared_prefix_calls == 0 and off.shared_prefix_rows == 0
    assert [o.request_id for o in a] == [str(i) for i in range(6)] == [o.request_id for o in b]
    assert [o.prompt_token_ids for o in a] == [rows[0], rows[1], other_row, rows[2], rows[3], rows[0]]
    assert [o.outputs[0].token_ids for o in a] == [o.outputs[0].token_ids for o in b], "ids equal to the flag-off run"
    for i, k in ((0, 0), (1, 1), (3, 2), (4, 3), (5, 0)):      # the rows over the shared video: the golden / oracle ids
        assert a[i].outputs[0].token_ids == medium["ref_ids"][k], (i, k)
