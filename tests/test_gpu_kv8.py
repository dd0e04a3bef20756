"""The opt-in fp8 K/V cache of the independent-row decode (vLLM kv_cache_dtype="fp8") on the GPU: the quantise kernel against the
torch restatement of its rule, o3v_attn_decode_kv8 bit for bit against o3v_attn_decode on the dequantised cache, its accuracy
against fp64, what it appends and what it must never read, and the engine / facade against the emulation mode
(`_debug_kv8_emulate`: bf16 caches whose rows are dequant(quant(row)), the ordinary bf16 kernels)."""
import math
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
import kernel_ops as ko
import kv8_ops as k8o
from kv8_ops import dequant, quant_rows128

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CANARY = 0xA5
U = 2.0 ** -8          # bf16 unit round-off: the coefficient of the decode kernels' bound in include/o3v.h


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open_o3_video_amd import _lib
    _lib.load()
    return torch.device("cuda")


def normals(shape, gen, lo=-20, hi=10):
    """bf16 normals with magnitudes spread log-uniformly over [2^lo, 2^hi), either sign"""
    e = torch.randint(lo, hi, shape, generator=gen).float()
    m = 1.0 + torch.rand(shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return (sign * m * torch.exp2(e)).to(BF)


# ------------------------------------------------------------------------------------------------ 1. the quantise kernel
@pytest.mark.parametrize("S", [1, 33])
def test_quantize_kernel_equals_the_rule(dev, S):
    gen = torch.Generator().manual_seed(S)
    L, B, Hkv, Tmax = 2, 3, 2, S + 5
    k, v = normals((L, B, Hkv, S, 128), gen), normals((L, B, Hkv, S, 128), gen)
    k[0, 1, 0, 0] = 0                         # zero rows: scale 1, codes 0
    v[1, 2, 1, S - 1] = 0
    k[1, 0, 1, S // 2] = normals((128,), gen, 3, 4)        # a row in one binade, and rows whose amax sits on 448 * 2^k
    v[0, 0, 0, 0, 7] = 448.0
    v[0, 0, 0, 0, :7] = normals((7,), gen, 0, 8)
    v[0, 0, 0, 0, 8:] = normals((120,), gen, 0, 8)
    k8, v8 = (torch.full((L, B, Hkv, Tmax, 128), CANARY, dtype=torch.uint8, device=dev) for _ in range(2))
    ks, vs = (torch.full((L, B, Hkv, Tmax), -7.0, dtype=torch.float32, device=dev) for _ in range(2))
    k8o.kv8_quantize(k.to(dev), v.to(dev), k8, v8, ks, vs)
    for src, c8, cs, name in ((k, k8, ks, "K"), (v, v8, vs, "V")):
        q, s = quant_rows128(src)
        assert torch.equal(cs[..., :S].cpu(), s), name
        assert torch.equal(c8[..., :S, :].cpu(), q), name
        assert (c8[..., S:, :] == CANARY).all() and (cs[..., S:] == -7.0).all(), f"{name}: slots past S were written"


# ------------------------------------------------------------------------------------------------ 2. attention, bit-identity
def _case(dev, B, Hq, Hkv, ctx, seed, k_lo_mode="mixed"):
    """Random K/V quantised by the rule; the newest key's rows as bf16 staging rows; the bf16 cache the kv8 kernel must agree with."""
    gen = torch.Generator().manual_seed(seed)
    Tmax = ctx + 3
    kfull = (torch.randn(B, Hkv, Tmax, 128, generator=gen) * torch.exp2(torch.randint(-3, 3, (B, Hkv, Tmax, 1), generator=gen).float())).to(BF)
    vfull = (torch.randn(B, Hkv, Tmax, 128, generator=gen) * torch.exp2(torch.randint(-6, 4, (B, Hkv, Tmax, 1), generator=gen).float())).to(BF)
    if ctx > 3:
        vfull[:, :, 2] = 0                                     # a zero row inside the context
    k8, ks = quant_rows128(kfull)
    v8, vs = quant_rows128(vfull)
    knew, vnew = kfull[:, :, ctx - 1].contiguous(), vfull[:, :, ctx - 1].contiguous()
    kd, vd = dequant(k8, ks), dequant(v8, vs)                  # slot ctx-1 holds dequant(quant(staging)) by construction
    q = (torch.randn(B, Hq, 128, generator=gen) * 0.7).to(BF)
    if k_lo_mode == "mixed":
        opts = [0, min(7, ctx - 1), ctx - 1]
        k_lo = torch.tensor([opts[(b + seed) % 3] for b in range(B)], dtype=torch.int32)
    else:
        k_lo = None
    # slot ctx-1 of the fp8 cache is what an earlier call left there: stale bytes, here the canary
    for t in (k8, v8):
        t[:, :, ctx - 1:] = CANARY
    for t in (ks, vs):
        t[:, :, ctx - 1:] = -7.0
    to = lambda t: None if t is None else t.to(dev)
    return dict(q=to(q), k8=to(k8), v8=to(v8), ks=to(ks), vs=to(vs), knew=to(knew), vnew=to(vnew), kd=to(kd), vd=to(vd), k_lo=to(k_lo),
                ctx=ctx, Tmax=Tmax, scale=1.0 / math.sqrt(128))


def _run_kv8(c, nsplit, poison=False):
    k8, v8, ks, vs = (c[n].clone() for n in ("k8", "v8", "ks", "vs"))
    out = k8o.attn_decode_kv8(c["q"], k8, v8, ks, vs, c["knew"], c["vnew"], c["k_lo"], c["ctx"], nsplit, c["scale"], poison=poison)
    return out, (k8, v8, ks, vs)


@pytest.mark.parametrize("ctx", [1, 31, 32, 33, 129, 513])
@pytest.mark.parametrize("B", [1, 4, 5])
@pytest.mark.parametrize("Hq,Hkv", [(7, 1), (16, 2), (8, 8), (28, 4)])
def test_attention_bit_identical_to_the_bf16_kernel(dev, Hq, Hkv, B, ctx):
    c = _case(dev, B, Hq, Hkv, ctx, seed=ctx * 7 + B)
    for nsplit in (1, 3, 8):                                   # 8 splits: more splits than 32-key tiles up to ctx = 129
        ref = ko.attn_decode(c["q"], c["kd"], c["vd"], c["k_lo"], ctx, nsplit, c["scale"], poison=True)
        out, _ = _run_kv8(c, nsplit, poison=True)
        assert torch.isfinite(ref.float()).all()
        assert torch.equal(out, ref), (nsplit, (out.float() - ref.float()).abs().max().item())
    c = _case(dev, B, Hq, Hkv, ctx, seed=ctx + B, k_lo_mode=None)                    # no k_lo array at all
    assert torch.equal(_run_kv8(c, 3, poison=True)[0], ko.attn_decode(c["q"], c["kd"], c["vd"], None, ctx, 3, c["scale"]))


# ------------------------------------------------------------------------------------------------ 3. attention, accuracy
def _ref64(q, K, V, k_lo, ctx, scale):
    """fp64 softmax attention of one decode step on the dequantised values -> ref, spread = sum_j p_j |v_j - ref|  [B, Hq, D]"""
    B, Hq, D = q.shape
    rep = Hq // K.shape[1]
    ref = torch.empty(B, Hq, D, dtype=torch.float64)
    spr = torch.empty_like(ref)
    for b in range(B):
        lo = int(k_lo[b]) if k_lo is not None else 0
        for h in range(Hq):
            k, v = K[b, h // rep, lo:ctx].double(), V[b, h // rep, lo:ctx].double()
            p = torch.softmax((k @ q[b, h].double()) * scale, dim=0)
            o = p @ v
            ref[b, h] = o
            spr[b, h] = (p[:, None] * (v - o[None]).abs()).sum(0)
    return ref, spr


@pytest.mark.parametrize("ctx,nsplit", [(33, 1), (300, 3), (513, 8)])
def test_attention_accuracy_peaked_inputs(dev, ctx, nsplit):
    """Scores of std 10 nats and a sink key at k_lo (~30 nats): |out - ref| <= u sum_j p_j |v_j - ref| + u |ref| + 1e-6 per element,
    the bound include/o3v.h derives for the decode kernels, on the dequantised K/V."""
    gen = torch.Generator().manual_seed(ctx)
    B, Hq, Hkv, Tmax = 3, 8, 2, ctx + 3
    q = torch.randn(B, Hq, 128, generator=gen).to(BF)
    K = (torch.randn(B, Hkv, Tmax, 128, generator=gen) * 10.0).to(BF)
    V = torch.randn(B, Hkv, Tmax, 128, generator=gen).to(BF)
    k_lo = torch.tensor([0, min(7, ctx - 1), min(40, ctx - 1)], dtype=torch.int32)
    scale = 1.0 / math.sqrt(128)
    for b in range(B):                                             # the sink: aligned with the mean query of each kv head
        for hk in range(Hkv):
            qm = q[b, hk * 4:(hk + 1) * 4].float().mean(0)
            K[b, hk, int(k_lo[b])] = (qm / qm.norm() * 30.0 / (scale * qm.norm())).to(BF)
    k8, ks = quant_rows128(K)
    v8, vs = quant_rows128(V)
    kd, vd = dequant(k8, ks), dequant(v8, vs)
    ref, spr = _ref64(q, kd, vd, k_lo, ctx, scale)
    knew, vnew = K[:, :, ctx - 1].contiguous(), V[:, :, ctx - 1].contiguous()
    out = k8o.attn_decode_kv8(q.to(dev), k8.to(dev), v8.to(dev), ks.to(dev), vs.to(dev), knew.to(dev), vnew.to(dev), k_lo.to(dev), ctx,
                              nsplit, scale, poison=True).cpu().double()
    err, tol = (out - ref).abs(), U * spr + U * ref.abs() + 1e-6
    print(f"kv8 peaked ctx={ctx}: max err/tol {float((err / tol).max()):.3f}")
    assert torch.isfinite(out).all() and (err <= tol).all(), float((err / tol).max())


@pytest.mark.parametrize("ctx,nsplit", [(33, 1), (129, 3), (513, 8)])
def test_attention_accuracy_needles(dev, ctx, nsplit):
    """q and K carry a +-16 binary code of the key position, so the needle key beats every other visible key by >= 45 nats: the
    output is the needle's dequantised V row within 1 bf16 ulp.  Needles sit on the edges: k_lo, the tile ends, the newest key."""
    gen = torch.Generator().manual_seed(ctx + 1)
    B, Hq, Hkv, Tmax = 2, 8, 2, ctx + 3
    nb = max(1, (Tmax - 1).bit_length())
    code = ((torch.arange(Tmax)[:, None] >> torch.arange(nb)) & 1).float() * 2 - 1          # [Tmax, nb]
    K = torch.zeros(B, Hkv, Tmax, 128)
    K[..., :nb] = code * 16.0
    K[..., nb:] = torch.randn(B, Hkv, Tmax, 128 - nb, generator=gen)                         # q is zero on these dimensions
    V = torch.randn(B, Hkv, Tmax, 128, generator=gen)
    k_lo = torch.tensor([0, min(5, ctx - 1)], dtype=torch.int32)
    edges = [ctx - 1, 0, 31, 32, ctx - 2, 63, 64, ctx // 2]
    needle = torch.empty(B, Hq, dtype=torch.long)
    q = torch.zeros(B, Hq, 128)
    for b in range(B):
        for h in range(Hq):
            n = min(max(edges[h], int(k_lo[b])), ctx - 1)
            needle[b, h] = n
            q[b, h, :nb] = code[n] * 16.0
    K, V, q = K.to(BF), V.to(BF), q.to(BF)
    k8, ks = quant_rows128(K)
    v8, vs = quant_rows128(V)
    vd = dequant(v8, vs).double()
    knew, vnew = K[:, :, ctx - 1].contiguous(), V[:, :, ctx - 1].contiguous()
    out = k8o.attn_decode_kv8(q.to(dev), k8.to(dev), v8.to(dev), ks.to(dev), vs.to(dev), knew.to(dev), vnew.to(dev), k_lo.to(dev), ctx,
                              nsplit, 1.0 / math.sqrt(128), poison=True).cpu().double()
    for b in range(B):
        for h in range(Hq):
            want = vd[b, h // 4, needle[b, h]]
            ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 7)
            assert ((out[b, h] - want).abs() <= ulp).all(), (b, h, int(needle[b, h]))


# ------------------------------------------------------------------------------------------------ 4. append and isolation
@pytest.mark.parametrize("ctx,nsplit", [(1, 1), (32, 3), (33, 1), (200, 8)])
def test_attention_appends_the_newest_key_and_reads_nothing_else(dev, ctx, nsplit):
    B, Hq, Hkv = 4, 8, 2
    c = _case(dev, B, Hq, Hkv, ctx, seed=11 + ctx)
    out, after = _run_kv8(c, nsplit)
    for name, src, c8, cs, i in (("K", c["knew"], after[0], after[2], "k"), ("V", c["vnew"], after[1], after[3], "v")):
        q, s = quant_rows128(src.cpu())
        assert torch.equal(c8[:, :, ctx - 1].cpu(), q) and torch.equal(cs[:, :, ctx - 1].cpu(), s), name
        before8, befores = c[i + "8"], c[i + "s"]
        keep = torch.ones(c["Tmax"], dtype=torch.bool, device=dev)
        keep[ctx - 1] = False
        assert torch.equal(c8[:, :, keep], before8[:, :, keep]) and torch.equal(cs[:, :, keep], befores[:, :, keep]), name
    # poison: every slot >= ctx-1 as found on entry (0x7F = e4m3fn NaN, NaN / Inf scales), every key below k_lo, out and partials
    p = dict(c)
    for n in ("k8", "v8"):
        p[n] = c[n].clone()
        p[n][:, :, ctx - 1:] = 0x7F
    for n, bad in (("ks", float("nan")), ("vs", float("inf"))):
        p[n] = c[n].clone()
        p[n][:, :, ctx - 1:] = bad
    for b in range(B):
        lo = int(c["k_lo"][b])
        p["k8"][b, :, :lo] = 0x7F
        p["v8"][b, :, :lo] = 0xFF
        p["ks"][b, :, :lo] = float("inf")
        p["vs"][b, :, :lo] = float("nan")
    out_p, _ = _run_kv8(p, nsplit, poison=True)
    assert torch.isfinite(out_p.float()).all() and torch.equal(out_p, out)


# ------------------------------------------------------------------------------------------------ engine
def _engine(cfg, wseed, **wkw):
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    c = O3VConfig.from_dict(cfg)
    return O3VEngine(c, DeviceWeights(c, getter_from_dict(fm.make_weights(cfg, wseed)), "cuda", **wkw))


_ENGINES = {}


def engine_of(name):
    if name not in _ENGINES:
        cfg = getattr(fm, name)()
        _ENGINES[name] = (cfg, _engine(cfg, {"medium_config": 6, "tied3b_config": 4}[name]))
    return _ENGINES[name]


def batch(cfg, eng, B0, seed=3):
    """B0 prompts of different lengths over their own frames, left-padded -> generate's positional and keyword arguments"""
    frs, prompts = [], []
    for i in range(B0):
        fr = fm.make_frames(1 + i % 2, 56, 84, seed=seed + i)
        _, grid = eng.pixels_from_frames(fr)
        prompts.append(fm.make_prompt(cfg, [tuple(g) for g in grid.tolist()], n_text_post=4 + 3 * (i % 4), seed=seed + i))
        frs.append(fr)
    S = max(len(p) for p in prompts)
    pad = cfg["pad_token_id"]
    rows = [[pad] * (S - len(p)) + p for p in prompts]
    mask = [[0] * (S - len(p)) + [1] * len(p) for p in prompts]
    return (rows, mask if B0 > 1 else None), dict(frames=torch.cat(frs), pad_token_id=pad), [S - len(p) for p in prompts]


def run(eng, args, kw, mode, keep=False, **more):
    """mode: 'fp8' | 'emulate' | 'bf16'; the engine is left at its defaults"""
    eng.kv_cache_dtype = "fp8" if mode == "fp8" else "bf16"
    eng._debug_kv8_emulate = mode == "emulate"
    eng._debug_keep = keep
    try:
        out = eng.generate(*args, **kw, **more)
        last = eng._debug_last if keep else None
    finally:
        eng.kv_cache_dtype, eng._debug_kv8_emulate, eng._debug_keep = "bf16", False, False
        eng._debug_last = None
    return out, last


def assert_same(a, b):
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.margins, b.margins)


@pytest.mark.parametrize("B0", [1, 4, 9])
@pytest.mark.parametrize("name", ["medium_config", "tied3b_config"])
def test_engine_fp8_kv_equals_the_emulation(dev, name, B0):
    """kv_cache_dtype="fp8" against the same engine on bf16 caches holding dequant(quant(row)) of every K/V row: bit-identical ids
    and margins, and the caches themselves: prompt slots = quant(the bf16 run's prompt K/V) (prefill is untouched), generated slots
    = the emulation's rows.  (Generated slots are compared dequantised: quantising a dequantised row whose largest code is 224
    picks the next smaller scale, other codes for the same values.)"""
    cfg, eng = engine_of(name)
    args, kw, pads = batch(cfg, eng, B0)
    T = 10
    a, ka = run(eng, args, kw, "fp8", keep=True, max_new_tokens=T)
    b, kb = run(eng, args, kw, "emulate", keep=True, max_new_tokens=T)
    eng.fused_decode = False
    try:
        c, kc = run(eng, args, kw, "bf16", keep=True, max_new_tokens=T)
    finally:
        eng.fused_decode = True
    assert_same(a, b)
    S = ka["S"]
    for r, p in enumerate(pads):                # the row's own prompt tokens (pad slots hold whatever prefill wrote for pad tokens)
        for c8, cs, src in ((ka["k8"], ka["k8s"], kc["kc"]), (ka["v8"], ka["v8s"], kc["vc"])):
            q, s = quant_rows128(src[:, r, :, p:S].cpu())
            assert torch.equal(c8[:, r, :, p:S].cpu(), q) and torch.equal(cs[:, r, :, p:S].cpu(), s), (r, p)
    gen = slice(S, S + T - 1)                   # the last token is sampled, never run
    for c8, cs, emu in ((ka["k8"], ka["k8s"], kb["kc"]), (ka["v8"], ka["v8s"], kb["vc"])):
        assert torch.equal(dequant(c8[:, :, :, gen].cpu(), cs[:, :, :, gen].cpu()), emu[:, :, :, gen].cpu())
    ta, tb, tc_ = a.timings, b.timings, c.timings
    assert ta["kv_cache_dtype"] == "fp8" and tb["kv_cache_dtype"] == "bf16" and tc_["kv_cache_dtype"] == "bf16"
    assert ta["standalone_attention_layers"] > 0 and ta["fused_attention_layers"] == 0
    assert ta["launches_per_layer"] == tc_["launches_per_layer"]
    t = eng.cfg.text
    staging = 2 * B0 * t.num_key_value_heads * 128 * 2
    assert ta["kv_cache_bytes"] * 256 == tc_["kv_cache_bytes"] * 132 + staging * 256


@pytest.mark.parametrize("fname,name,key", [("g7_medium.npz", "medium_config", 2), ("g11_tied3b.npz", "tied3b_config", 4)])
def test_engine_default_is_untouched(dev, golden_dir, fname, name, key):
    g = np.load(os.path.join(golden_dir, fname))
    cfg = getattr(fm, name)()
    eng = _engine(cfg, key)
    assert eng.kv_cache_dtype == "bf16"
    n_new = 12
    out = eng.generate(g["input_ids"], None, pixel_values=torch.from_numpy(g["pixel_values"]), image_grid_thw=g["grid"],
                       max_new_tokens=n_new, pad_token_id=cfg["pad_token_id"])
    S = g["input_ids"].shape[1]
    assert np.array_equal(out.sequences.cpu().numpy(), g["bf16_ids"][:, :S + n_new])
    assert out.timings["kv_cache_dtype"] == "bf16"
    if name == "tied3b_config":     # 16 query heads of 128: a shape the one-launch block is built for; it still runs at B = 1
        assert out.timings["fused_attention_layers"] > 0 and out.timings["standalone_attention_layers"] == 0
        assert abs(out.timings["launches_per_layer"] - 3.0) < 1e-9        # attention block, gate/up, down


def test_engine_fp8_kv_with_fp8_weight_rows(dev):
    cfg = fm.medium_config()
    eng = _engine(cfg, 6, fp8_decode=True)
    args, kw, _ = batch(cfg, eng, 4)
    a, _ = run(eng, args, kw, "fp8", max_new_tokens=10)
    b, _ = run(eng, args, kw, "emulate", max_new_tokens=10)
    assert_same(a, b)
    assert a.timings["kv_cache_dtype"] == "fp8" and eng.w.llm.layer[0].qkv_w8p


@pytest.mark.parametrize("fname,cfgname,wseed,in_effect", [("g12_q3_tiny.npz", "tiny_q3_config", 0, "bf16"),
                                                           ("g13_q3_medium.npz", "medium_q3_config", 2, "fp8")])
def test_engine_fp8_kv_qwen3vl(dev, golden_dir, fname, cfgname, wseed, in_effect):
    """Qwen3-VL (q/k norm between the linear and the rotation: o3v_qkv_norm_rope_cache writes the staging rows) at 1 and 4 rows.
    The G12 fixture has head_dim 32, where the format is not in effect (the call must simply be the bf16 call); G13 has 128."""
    import fixture_models_q3 as fq
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    g = np.load(os.path.join(golden_dir, fname))
    cfg = getattr(fq, cfgname)()
    c = O3VConfig.from_dict(cfg)
    eng = O3VEngine(c, DeviceWeights(c, getter_from_dict(fq.make_weights(cfg, wseed)), "cuda"))
    pv = torch.from_numpy(g["pixel_values"])
    for rows in (1, 4):
        args = (np.repeat(g["input_ids"], rows, axis=0), None)
        kw = dict(pixel_values=torch.cat([pv] * rows), image_grid_thw=np.concatenate([g["grid"]] * rows), max_new_tokens=8,
                  pad_token_id=cfg["pad_token_id"])
        a, _ = run(eng, args, kw, "fp8")
        b, _ = run(eng, args, kw, "emulate")
        assert_same(a, b)
        assert a.timings["kv_cache_dtype"] == in_effect
        assert all(torch.equal(a.sequences[i], a.sequences[0]) for i in range(rows))


def test_engine_fp8_kv_logprobs_and_repetition_penalty(dev):
    cfg, eng = engine_of("medium_config")
    args, kw, _ = batch(cfg, eng, 4)
    more = dict(max_new_tokens=8, logprobs=3, repetition_penalty=1.05)
    a, _ = run(eng, args, kw, "fp8", **more)
    b, _ = run(eng, args, kw, "emulate", **more)
    assert_same(a, b)
    for f in ("token", "rank", "top_ids", "top"):
        assert torch.equal(getattr(a.logprobs, f), getattr(b.logprobs, f)), f
    assert torch.isfinite(a.logprobs.token).all()


def test_engine_fp8_kv_prefix_reuse(dev, golden_dir):
    """`prefix_key`: the store keeps the prompt's bf16 K/V, a second call prefills only the tokens behind the common prefix (as
    test_prefix_kv_reuse states it: the reused count is the cut, the ids those of the cold run) and quantises the whole prompt."""
    g = np.load(os.path.join(golden_dir, "g7_medium.npz"))
    cfg = fm.medium_config()
    eng = _engine(cfg, 2)
    ids = g["input_ids"][0].copy()
    S = len(ids)
    special = {cfg["image_token_id"], cfg["vision_start_token_id"], cfg["vision_end_token_id"]}
    cut = [i for i in range(S) if int(ids[i]) not in special][-3]
    other = ids.copy()
    other[cut] = ids[cut] + 1 if int(ids[cut]) + 1 not in special else ids[cut] + 2
    kw = dict(pixel_values=torch.from_numpy(g["pixel_values"]), image_grid_thw=g["grid"], repetition_penalty=1.05,
              pad_token_id=cfg["pad_token_id"])
    res = {}
    for mode in ("fp8", "emulate"):
        cold, _ = run(eng, ([ids], None), kw, mode, max_new_tokens=12)
        run(eng, ([other], None), kw, mode, max_new_tokens=2, prefix_key=("vid", mode))
        warm, _ = run(eng, ([ids], None), kw, mode, max_new_tokens=12, prefix_key=("vid", mode))
        assert cold.timings["prefix_tokens_reused"] == 0 and warm.timings["prefix_tokens_reused"] == cut
        assert torch.equal(warm.sequences, cold.sequences), mode
        res[mode] = (cold, warm)
    assert res["fp8"][1].timings["kv_cache_dtype"] == "fp8"
    assert eng._prefix[("vid", "fp8")]["k"].dtype == BF                    # the store keeps bf16
    assert_same(res["fp8"][0], res["emulate"][0])
    assert_same(res["fp8"][1], res["emulate"][1])


def test_engine_groups_keep_bf16(dev):
    cfg, eng = engine_of("medium_config")
    args, kw, _ = batch(cfg, eng, 1)
    a, _ = run(eng, args, kw, "fp8", max_new_tokens=8, num_return_sequences=4)
    b, _ = run(eng, args, kw, "bf16", max_new_tokens=8, num_return_sequences=4)
    assert a.timings["kv_cache_dtype"] == "bf16" and torch.equal(a.sequences, b.sequences)
    # G rows that each hold their own copy of the prompt (no shared entry): fp8 is in effect, the quantised prompt is fanned out
    eng.group_attention = False
    try:
        c, _ = run(eng, args, kw, "fp8", max_new_tokens=8, num_return_sequences=4)
        d, _ = run(eng, args, kw, "emulate", max_new_tokens=8, num_return_sequences=4)
    finally:
        eng.group_attention = True
    assert c.timings["kv_cache_dtype"] == "fp8"
    assert_same(c, d)


# The drift gate.  Measured once on the MI355X (medium_config fixture, 3 layers, 4 left-padded rows, first decode step) against the
# bf16-K/V engine: the largest |logit(fp8 K/V) - logit(bf16 K/V)| is 0.498 on logits of magnitude up to 17.5 (4 bf16 ulps there), and
# all four rows follow the bf16-K/V run for 10/10 greedy tokens.  A misapplied scale moves logits by O(1..10); the factor 2 covers
# box-to-box summation-order noise.
DRIFT_MEASURED = 0.498


def test_engine_drift_against_bf16_kv(dev):
    cfg, eng = engine_of("medium_config")
    args, kw, _ = batch(cfg, eng, 4)
    T = 10
    a, _ = run(eng, args, kw, "fp8", max_new_tokens=T)
    b, _ = run(eng, args, kw, "bf16", max_new_tokens=T)
    S = len(args[0][0])
    for r in range(4):
        ga, gb = a.sequences[r, S:].tolist(), b.sequences[r, S:].tolist()
        k = next((i for i in range(T) if ga[i] != gb[i]), T)
        print(f"fp8 K/V drift: row {r} follows the bf16-K/V run for {k}/{T} greedy tokens")
    _, la = run(eng, args, kw, "fp8", keep=True, max_new_tokens=2)
    _, lb = run(eng, args, kw, "bf16", keep=True, max_new_tokens=2)
    d = (la["logits"].float() - lb["logits"].float()).abs().max().item()
    print(f"fp8 K/V drift: first decode step, max |logit diff| vs bf16 K/V = {d:.4f} (logit magnitude {lb['logits'].float().abs().max().item():.2f})")
    assert d < 2 * DRIFT_MEASURED


# ------------------------------------------------------------------------------------------------ facade
def test_vllm_facade_kv_cache_dtype_fp8(dev):
    from test_gpu_facades import StubTokenizer
    from open_o3_video_amd.vllm_api import LLM, SamplingParams
    cfg = fm.medium_config()
    eng = _engine(cfg, 6)
    llm = LLM(engine=eng, tokenizer=StubTokenizer(cfg), max_model_len=4096, kv_cache_dtype="fp8")
    assert llm.engine.kv_cache_dtype == "fp8"
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(10, 400, (L,), generator=g).tolist() for L in (14, 9)]
    sp = SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True)
    outs = llm.generate([{"prompt": " ".join(f"w{t}" for t in p)} for p in prompts], sp)
    L = max(len(p) for p in prompts)
    pad = cfg["pad_token_id"]
    rows = [[pad] * (L - len(p)) + p for p in prompts]
    mask = [[0] * (L - len(p)) + [1] * len(p) for p in prompts]
    ref = eng.generate(rows, mask, max_new_tokens=10, pad_token_id=pad)
    assert ref.timings["kv_cache_dtype"] == "fp8"
    for i in range(2):
        assert outs[i].outputs[0].token_ids == ref.sequences[i, L:].tolist()
    eng.kv_cache_dtype = "bf16"
