"""The one-launch decode attention block hands its payloads over in 16-byte accesses (partials, merge slice on the 8-element grid,
merged output) and packs the q/k/v publish per workgroup: it must still equal the stand-alone launches BYTE FOR BYTE -- q, the
appended K/V row, the attention output, the residual stream -- over three consecutive epochs on the same buffers with fresh inputs
(a stale line would show).  Contexts are chosen so that every branch of the slice code runs; the split count is the engine's own
rule (plan_decode), and each case checks that it is in the regime it is meant for through o3v_attn_merge_slice."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D, TNEW, STEP = 128, 7, 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open_o3_video_amd import _lib
    _lib.load()
    return torch.device("cuda")


def nan_fill_(x):
    i = x.view(torch.int16)
    i[..., 0::2, :] = 0x7FC0
    i[..., 1::2, :] = -1


_weights = {}


def weights(dev, Hq, Hkv, H, form):
    """Random layer weights of one head geometry, made once per module (the cases of a geometry share them)."""
    key = (Hq, Hkv, H, form)
    if key not in _weights:
        from open_o3_video_amd.weights import quantize_rows_fp8
        g = torch.Generator().manual_seed(Hq * 1000 + H)
        N, QD = (Hq + 2 * Hkv) * D, Hq * D
        w = dict(nw=(1 + 0.1 * torch.randn(H, generator=g)).to(BF).to(dev),
                 wqkv=(torch.randn(N, H, generator=g) / math.sqrt(H)).to(BF).to(dev),
                 bqkv=(0.5 * torch.randn(N, generator=g)).to(BF).to(dev),
                 wo=(torch.randn(H, QD, generator=g) / math.sqrt(QD)).to(BF).to(dev),
                 qn=(1 + 0.2 * torch.randn(D, generator=g)).to(BF).to(dev),
                 kn=(1 + 0.2 * torch.randn(D, generator=g)).to(BF).to(dev))
        ang = torch.rand(1, TNEW, D // 2, generator=g) * 30
        w["cos"] = torch.cat([ang.cos(), ang.cos()], -1).to(BF).to(dev).contiguous()
        w["sin"] = torch.cat([ang.sin(), ang.sin()], -1).to(BF).to(dev).contiguous()
        if form == "fp8":
            w["q8"], w["qs"] = quantize_rows_fp8(w["wqkv"])
            w["o8"], w["os"] = quantize_rows_fp8(w["wo"])
        _weights[key] = w
    return _weights[key]


def slices(lib, n_out, nsplit):
    fn = lib.o3v_attn_merge_slice
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    fn.restype = C.c_int
    out = []
    b, c = C.c_int(), C.c_int()
    for s in range(nsplit):
        assert fn(n_out, nsplit, s, C.byref(b), C.byref(c)) == 0
        out.append((b.value, c.value))
    return out


# (form, Hq, Hkv, H, ctx, T new tokens the call was planned for, left pad, regime the case is there for)
CASES = [
    ("bf16", 28, 4, 3584, 1, 16, 0, "whole"),         # 7B: one key, one split: the slice is the whole head group (896 > 256: several trips)
    ("bf16", 28, 4, 3584, 40, 512, 3, "multi"),       # 7B: 5 splits (184 / 160 elements), all keys in the first: four workgroups publish neutral partials
    ("bf16", 28, 4, 3584, 7200, 64, 0, "empty"),      # 7B: nsplit * 8 > n_rep * D / 2: trailing workgroups merge nothing, still take ticket 2
    ("bf16", 28, 4, 3584, 4490, 200, 0, "n37"),       # 7B: the bench prompt, 37 splits of 32 / 0 elements
    ("bf16", 16, 2, 2048, 3, 16, 0, "whole"),         # 3B (n_rep 8): the largest whole-head slice, 1024 elements
    ("bf16", 16, 2, 2048, 1500, 232, 5, "ragged"),    # 3B: 14 splits of 80 elements, a shorter last slice and an empty one
    ("fp8", 28, 4, 3584, 4490, 200, 0, "n37"),        # fp8 weight rows, once
    ("qkn", 32, 8, 4096, 300, 212, 5, "multi"),       # q/k norm (raw scratch + head-group finish), once
]


@pytest.mark.parametrize("form,Hq,Hkv,H,ctx,T,pad,regime", CASES)
def test_block_equals_stand_alone_launches_bytewise(dev, form, Hq, Hkv, H, ctx, T, pad, regime):
    from open_o3_video_amd import _lib
    from open_o3_video_amd.engine import plan_decode
    lib = _lib.load()
    plan = plan_decode(Hq, Hkv, D, 1, 1, ctx, T)
    Tmax, nsplit = plan.Tmax, plan.nsplit
    n_rep, N, QD = Hq // Hkv, (Hq + 2 * Hkv) * D, Hq * D
    cap = lib.o3v_decode_attn_block_capacity(QD, 1 if form == "fp8" else 2)
    if form != "qkn":   # (the capacity query has no q/k-norm form; the launcher checks its own)
        assert nsplit * Hkv + (H + 7) // 8 < cap, "the one-launch form does not apply to this context"
    sl = slices(lib, n_rep * D, nsplit)
    if regime == "whole":
        assert nsplit == 1 and sl == [(0, n_rep * D)]
    elif regime == "empty":
        assert nsplit * 8 > n_rep * D // 2 and sl[-1][1] == 0 and sl[0][1] > 0
    elif regime == "n37":
        assert nsplit == 37 and sl[0][1] == 32 and sl[-1][1] == 0
    elif regime == "ragged":
        assert 0 < sl[-2][1] < sl[0][1] and sl[-1][1] == 0 and sl[0][1] % D != 0
    else:
        assert nsplit > 1 and all(c > 0 for _, c in sl)

    w = weights(dev, Hq, Hkv, H, form)
    slot = ctx - 1
    g = torch.Generator().manual_seed(Hq * 1000 + ctx)
    kc0 = torch.randn(1, Hkv, Tmax, D, generator=g).to(BF).to(dev)
    vc0 = torch.randn(1, Hkv, Tmax, D, generator=g).to(BF).to(dev)
    kc0[:, :, slot] = float("nan")     # the slot of the new token holds garbage until the q/k/v role fills it
    vc0[:, :, slot] = float("nan")
    nan_fill_(kc0[:, :, ctx:])         # slots past the context are never read
    nan_fill_(vc0[:, :, ctx:])
    k_lo = torch.tensor([pad], dtype=torch.int32, device=dev)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    scale = 1.0 / math.sqrt(D)
    sync = torch.zeros(lib.o3v_decode_sync_bytes(), dtype=torch.uint8, device=dev)   # zeroed once; epochs 1, 2, 3 below
    part_o = torch.empty(Hq * 64 * D, dtype=torch.float32, device=dev)
    part_ml = torch.empty(Hq * 64 * 2, dtype=torch.float32, device=dev)
    zq = lambda: torch.zeros(1, Hq, D, dtype=BF, device=dev)
    q2, att2, raw2 = zq(), zq(), torch.zeros(N, dtype=BF, device=dev)
    k2, v2 = kc0.clone(), vc0.clone()
    nw, cos, sin = w["nw"], w["cos"], w["sin"]
    for rep in range(3):
        x0 = (torch.randn(1, H, generator=g) * 2).to(BF).to(dev)
        # ---- the stand-alone launches
        x1, q1, att1, k1, v1 = x0.clone(), zq(), zq(), kc0.clone(), vc0.clone()
        po1, pm1 = torch.empty_like(part_o), torch.empty_like(part_ml)
        if form == "bf16":
            _lib.call("o3v_gemv_norm_qkv_rope", P(x1), P(nw), 1e-6, P(w["wqkv"]), None, P(w["bqkv"]), 1, H, H, P(cos), P(sin), P(q1),
                      P(k1), P(v1), slot, Hq, Hkv, D, Tmax, TNEW, STEP, st)
        elif form == "fp8":
            _lib.call("o3v_gemv_norm_qkv_rope_fp8", P(x1), P(nw), 1e-6, P(w["q8"]), P(w["qs"]), P(w["bqkv"]), 1, H, H, P(cos), P(sin),
                      P(q1), P(k1), P(v1), slot, Hq, Hkv, D, Tmax, TNEW, STEP, st)
        else:
            qkv1 = torch.zeros(1, N, dtype=BF, device=dev)
            _lib.call("o3v_linear_decode", P(x1), P(nw), 1e-6, P(w["wqkv"]), None, None, None, P(qkv1), 1, N, H, H, N, 0, _lib.EPI_NONE, st)
            _lib.call("o3v_qkv_norm_rope_cache", P(qkv1), P(w["qn"]), P(w["kn"]), 1e-6, P(cos), P(sin), P(q1), P(k1), P(v1), slot, 1, 1,
                      Hq, Hkv, D, Tmax, TNEW, STEP, st)
        _lib.call("o3v_attn_decode", P(q1), P(k1), P(v1), P(att1), P(po1), P(pm1), P(k_lo), 1, Hq, Hkv, D, ctx, Tmax, nsplit, scale, st)
        if form == "fp8":
            _lib.call("o3v_linear_decode_fp8", P(att1), None, 0.0, P(w["o8"]), P(w["os"]), None, P(x1), P(x1), 1, H, QD, QD, H, H,
                      _lib.EPI_RESIDUAL, st)
        else:
            _lib.call("o3v_linear_decode", P(att1), None, 0.0, P(w["wo"]), None, None, P(x1), P(x1), 1, H, QD, QD, H, H,
                      _lib.EPI_RESIDUAL, st)
        # ---- one launch, the same buffers every epoch
        x2 = x0.clone()
        k2[:, :, slot] = float("nan")
        v2[:, :, slot] = float("nan")
        if form == "bf16":
            rc = lib.o3v_decode_attn_block(P(x2), P(nw), 1e-6, P(w["wqkv"]), P(w["bqkv"]), P(w["wo"]), P(cos), P(sin), P(q2), P(att2),
                                           P(k2), P(v2), P(part_o), P(part_ml), P(k_lo), H, Hq, Hkv, D, slot, Tmax, TNEW, STEP, nsplit,
                                           scale, P(sync), rep + 1, st)
        elif form == "fp8":
            rc = lib.o3v_decode_attn_block_fp8(P(x2), P(nw), 1e-6, P(w["q8"]), P(w["qs"]), P(w["bqkv"]), P(w["o8"]), P(w["os"]), P(cos),
                                               P(sin), P(q2), P(att2), P(k2), P(v2), P(part_o), P(part_ml), P(k_lo), H, Hq, Hkv, D, slot,
                                               Tmax, TNEW, STEP, nsplit, scale, P(sync), rep + 1, st)
        else:
            rc = lib.o3v_decode_attn_block_qknorm(P(x2), P(nw), 1e-6, P(w["wqkv"]), None, P(w["wo"]), None, P(w["qn"]), P(w["kn"]),
                                                  P(raw2), P(cos), P(sin), P(q2), P(att2), P(k2), P(v2), P(part_o), P(part_ml), P(k_lo),
                                                  H, Hq, Hkv, D, slot, Tmax, TNEW, STEP, nsplit, scale, P(sync), rep + 1, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        tmo = int(sync[_lib.SYNC_TMO_BYTE:_lib.SYNC_TMO_BYTE + 4].view(torch.int32)[0].item())
        assert tmo == 0, f"an in-launch wait timed out (code {tmo:#x})"
        assert not torch.isnan(x1.float()).any() and not torch.isnan(att1.float()).any()
        for name, a, b in (("q", q2, q1), ("k", k2, k1), ("v", v2, v1), ("att", att2, att1), ("xout", x2, x1)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name} differs in epoch {rep + 1}"
