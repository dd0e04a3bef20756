"""The memory contract of the linear, norm and row-quantise entry points of include/o3v.h: padded pitches, odd N, ragged tile edges
and what a kernel may touch.  Every case runs its entry point twice on the same operand values -- contiguous, the way the other GPU
tests call it, and on canvases (kernel_ops.canvas): inputs inside NaN-filled buffers at a padded pitch, outputs inside canary-filled
ones, each with at least one full tile of guard rows on both sides.  Asserted per case (`run`):
  1. both calls return what the header documents (O3V_OK, or the O3V_ERR_* of a shape it rules out; a pitch it rules out is
     refused by the canvas call alone) -- after a refusal every canvas is wholly untouched;
  2. the canvas output is BIT-EQUAL to the contiguous one (same kernel, same decomposition, same arithmetic per element -- also
     where the pitch forces the MFMA GEMMs' scalar epilogue);
  3. the contiguous output passes the reference check the neighbouring test of that entry point uses (same close_bf16 arguments);
  4. nothing outside the output view changed (padding columns, guard rows), no input canvas changed, no NaN reached the output;
  5. a residual updated in place (res aliases out, both padded) gives the same bits, where the entry point takes a residual.
Shapes are the smallest at which each path can still go wrong; the table below is the whole test."""
import ctypes as C
import functools
import math

import pytest
import torch

import kernel_ops as ops
from test_gpu_kernels import _epi_ref, close_bf16, rb

pytestmark = pytest.mark.gpu

BF, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
OK, ERR_ARG, ERR_SHAPE = 0, -1, -2
from open_o3_video_amd._lib import EPI_GELU_TANH  # noqa: E402
EPI = {"none": ops.EPI_NONE, "res": ops.EPI_RESIDUAL, "gelu": ops.EPI_GELU, "swiglu": ops.EPI_SWIGLU, "gelu_tanh": EPI_GELU_TANH}
CANARY16 = ops.CANARY & 0xFFFF


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open_o3_video_amd import _lib
    _lib.load()
    return torch.device("cuda")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    from open_o3_video_amd import _lib
    return _lib.load()


def status(fn, *a, **kw):
    """O3V status of a kernel_ops wrapper call (the wrappers raise on a non-zero one)"""
    from open_o3_video_amd import _lib
    try:
        fn(*a, **kw)
    except _lib.O3VError as e:
        return e.code
    return OK


def r8(n):
    return (n + 7) // 8 * 8


def ld(t):
    return 0 if t is None else t.stride(0)


def raw(t):
    return t.view(ops._RAW[t.dtype])


# ------------------------------------------------------------------------------------------------ the harness
class Spec:
    """One call of one entry point.
    call(t) -> status; t maps operand names to tensors (contiguous, or canvas views: the pitches passed are their strides)
    ins    name -> (contiguous 2-D device tensor, padded pitch)          outs   name -> (rows, cols, padded pitch, dtype)
    ref(t) reference check of the contiguous run                         expect the documented status
    alias  (input, output): that input is updated in place -- one buffer at the output's pitch
    dense  name -> (shape, dtype): outputs without a pitch (q, the K/V cache), canary-filled in both runs and compared bit for bit
    after(t) checks the dense outputs of a call that ran
    expect_canvas: the documented status of the canvas call where it differs from the contiguous one's (a pitch the header rules
    out: the contiguous call, whose pitches are the widths, still runs)"""

    def __init__(self, call, ins, outs, ref=None, expect=OK, alias=None, dense=None, after=None, expect_canvas=None):
        self.call, self.ins, self.outs, self.ref, self.expect, self.alias = call, ins, outs, ref, expect, alias
        self.dense, self.after = dense or {}, after
        self.expect_canvas = expect if expect_canvas is None else expect_canvas


def _dense(spec, t, dev):
    for name, (shape, dt) in spec.dense.items():
        t[name] = torch.empty(shape, dtype=dt, device=dev)
        raw(t[name]).fill_(CANARY16 if dt == BF else ops.CANARY & 0xFF)


def run(dev, spec):
    src, dst = spec.alias or (None, None)
    # ---- contiguous, as the other tests call it
    t1 = {k: v for k, (v, _) in spec.ins.items()}
    for name, (rows, cols, _, dt) in spec.outs.items():
        t1[name] = torch.empty((rows, cols), dtype=dt, device=dev)
    if src:
        t1[dst] = t1[src].clone()
        t1[src] = t1[dst]
    _dense(spec, t1, dev)
    rc1 = spec.call(t1)
    torch.cuda.synchronize()
    expect = spec.expect
    assert rc1 == expect, f"contiguous call returned {rc1}, the header documents {expect}"
    if expect == OK:
        if spec.after:
            spec.after(t1)
        if spec.ref:
            spec.ref(t1)
    expect = spec.expect_canvas
    # ---- the same values on canvases
    widest = max([p for _, p in spec.ins.values()] + [o[2] for o in spec.outs.values()])
    cv, t2 = {}, {}
    for name, (rows, cols, pitch, dt) in spec.outs.items():
        cv[name] = ops.canvas(rows, cols, pitch, dt, ops.CANARY, ops.guard_rows_for(rows, pitch, widest), dev)
        t2[name] = cv[name].view
    for name, (v, pitch) in spec.ins.items():
        if name == src:
            t2[name] = t2[dst] = cv[dst].load(v)
            continue
        assert pitch > v.shape[1], "an input canvas has padding columns"
        cv[name] = ops.canvas(v.shape[0], v.shape[1], pitch, v.dtype, ops.NAN, ops.guard_rows_for(v.shape[0], pitch, widest), dev)
        t2[name] = cv[name].load(v)
    _dense(spec, t2, dev)
    rc2 = spec.call(t2)
    torch.cuda.synchronize()
    assert rc2 == expect, f"canvas call returned {rc2}, the header documents {expect} (contiguous: {rc1})"
    for name in spec.ins:
        if name != src:
            cv[name].untouched(whole=True)          # an input (a separate residual buffer too) is never written
    for name, (_, _, _, dt) in spec.outs.items():
        if expect != OK:
            cv[name].untouched(whole=True)          # refused before any launch
            continue
        cv[name].untouched()
        assert rc1 == OK
        assert torch.equal(raw(t2[name]), raw(t1[name])), \
            f"{name}: {int((raw(t2[name]) != raw(t1[name])).sum())} elements differ between the canvas and the contiguous call"
        if dt.is_floating_point:
            assert not t2[name].isnan().any(), f"{name}: NaN in the output view"
    for name in spec.dense:
        if expect == rc1:
            assert torch.equal(raw(t2[name]), raw(t1[name])), f"{name} differs between the padded and the contiguous call"
        if expect != OK:
            assert (raw(t2[name]) == (CANARY16 if t2[name].dtype == BF else ops.CANARY & 0xFF)).all(), f"{name} written by a refused call"
    if expect == OK and spec.after:
        spec.after(t2)


# ------------------------------------------------------------------------------------------------ operands, shared by the cases of a shape
@functools.lru_cache(maxsize=None)
def _lin(M, N, K, xscale=1.0):
    """x [M,K], W [N,K] (read as the 16-row interleaved gate/up matrix by the SWIGLU cases), bias, residual, norm weights and the
    fp32 product, on the GPU"""
    g = torch.Generator().manual_seed(M * 131 + N * 7 + K)
    d = dict(x=(torch.randn(M, K, generator=g) * xscale).to(BF), w=(torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF),
             bias=(0.1 * torch.randn(N, generator=g)).to(BF), res=torch.randn(M, N, generator=g).to(BF),
             nw=(1 + 0.1 * torch.randn(K, generator=g)).to(BF), nw_out=(1 + 0.1 * torch.randn(N, generator=g)).to(BF))
    d = {k: v.cuda() for k, v in d.items()}
    d["acc"] = d["x"].float() @ d["w"].float().t()
    return d


@functools.lru_cache(maxsize=None)
def _normed(M, N, K, xscale):
    """(rmsnorm(x) as the oracle rounds it, its fp32 product with W)"""
    from oracle import model_ref
    d = _lin(M, N, K, xscale)
    xn = model_ref.rmsnorm(d["x"].cpu(), d["nw"].cpu(), 1e-6).cuda()
    return xn, xn.float() @ d["w"].float().t()


def swiglu_ref(acc, bias):
    """out[:, 16 b + j] = bf16(bf16(silu(bf16(row 32 b + j))) * bf16(row 32 b + 16 + j)) of the packed gate/up product"""
    v = rb(acc + (bias.float() if bias is not None else 0)).view(acc.shape[0], -1, 2, 16)
    return rb(rb(torch.nn.functional.silu(v[:, :, 0])) * v[:, :, 1]).reshape(acc.shape[0], -1)


def check_linear(out, acc, bias, res, epi):
    if epi == "swiglu":
        close_bf16(out, swiglu_ref(acc, bias))                                  # test_swiglu_gemm_and_gemv
    elif epi == "gelu_tanh":
        lin = rb(acc + bias.float())
        close_bf16(out, torch.nn.functional.gelu(lin, approximate="tanh"), ulps=1, atol=1e-3, frac=0.999)   # test_gemm_gelu_tanh_epilogue
    else:
        close_bf16(out, _epi_ref(acc, bias, res, EPI[epi]))                     # test_gemm_epilogues / test_gemv / test_gemm_splitk


def _res_ins(ins, d, epi, ldr):
    if epi == "res":
        ins["res"] = (d["res"], ldr)


# ------------------------------------------------------------------------------------------------ MFMA GEMM, split-K
def gemm_spec(entry, M, N, K, epi, ldo, ldr=0, bias=True, inplace=False):
    d = _lin(M, N, K)
    b, E, No = (d["bias"] if bias else None), EPI[epi], (N // 2 if epi == "swiglu" else N)
    ins = {"a": (d["x"], K + 8), "w": (d["w"], K + 24)}
    _res_ins(ins, d, epi, ldr or ldo)

    def call(t):
        a, w, res, out = t["a"], t["w"], t.get("res"), t["out"]
        if entry in ("tile128", "tile256"):
            return status(ops.gemm, a, w, b, res, E, force="gemm", tile=int(entry[4:]), out=out)
        fn = lib().o3v_gemm_bf16_phased if entry == "phased" else lib().o3v_gemm_bf16
        return fn(P(a), P(w), P(b), P(res), P(out), M, N, K, ld(a), ld(w), ld(out), ld(res), E, st())

    return Spec(call, ins, {"out": (M, No, ldo, BF)}, lambda t: check_linear(t["out"], d["acc"], b, d["res"], epi),
                expect=ERR_SHAPE if entry == "phased" and K < 256 else OK,     # o3v.h: K % 128 == 0, K >= 256
                alias=("res", "out") if inplace else None)


def splitk_spec(M, N, K, splits, epi, ldo, ldr=0, inplace=False):
    d = _lin(M, N, K)
    ins = {"a": (d["x"], K + 8), "w": (d["w"], K + 24)}
    _res_ins(ins, d, epi, ldr or ldo)

    def call(t):   # workspace of partials NaN-filled: a partial nobody writes (a split without k-steps) would surface
        return status(ops.gemm_splitk, t["a"], t["w"], d["bias"], t.get("res"), EPI[epi], splits, out=t["out"], poison=True)

    return Spec(call, ins, {"out": (M, N, ldo, BF)}, lambda t: check_linear(t["out"], d["acc"], d["bias"], d["res"], epi),
                alias=("res", "out") if inplace else None)


# ------------------------------------------------------------------------------------------------ GEMV, skinny GEMM, decode linears
@functools.lru_cache(maxsize=None)
def _images(M, N, K, kind):
    """the weight images of the decode linears for _lin(M, N, K, 2.0)'s W, and the bf16 matrix holding exactly what they multiply"""
    from open_o3_video_amd import weights as W
    w = _lin(M, N, K, 2.0)["w"]
    if kind == "frag":
        return dict(wp=W.pack_mfma_fragments(w), wq=w)
    if kind == "fp8":
        q8, sc = W.quantize_rows_fp8(w)
        wd = W.dequantize_rows_fp8(q8, sc)
        assert torch.equal(wd.to(BF).float(), wd)
        return dict(q8=q8, sc=sc, wq=wd.to(BF), q8p=W.pack_mfma_fragments_fp8(q8) if N % 16 == 0 and K % 64 == 0 else None)
    q4, s4 = W.quantize_rows_mxfp4(w)
    wd = W.dequantize_rows_mxfp4(q4, s4)
    assert torch.equal(wd.to(BF).float(), wd)
    q4p, s4p = W.pack_mfma_fragments_mxfp4(q4, s4) if N % 16 == 0 and K % 128 == 0 else (None, None)
    return dict(q4=q4, s4=s4, wq=wd.to(BF), q4p=q4p, s4p=s4p)


def decode_spec(entry, M, N, K, epi, ldo, ldr=0, norm=False, bias=True, inplace=False):
    """entry: gemv (o3v_gemv_bf16 / o3v_gemv_norm_bf16 on row-major W at a padded ldw), decode (o3v_linear_decode with the
    fragment-major image), fp8 / fp8_rows / mxfp4 / mxfp4_rows"""
    d = _lin(M, N, K, 2.0)
    E, No = EPI[epi], (N // 2 if epi == "swiglu" else N)
    b = d["bias"] if bias else None
    nw = d["nw"] if norm else None
    ins = {"x": (d["x"], K + 8)}
    if entry == "gemv":
        ins["w"] = (d["w"], K + 16)
    _res_ins(ins, d, epi, ldr or ldo)
    im = _images(M, N, K, {"gemv": "frag", "decode": "frag", "fp8": "fp8", "fp8_rows": "fp8"}.get(entry, "mxfp4")) if entry != "gemv" else None

    def call(t):
        x, res, out = t["x"], t.get("res"), t["out"]
        tail = (P(b), P(res), P(out), M, N, K, ld(x), ld(out), ld(res), E, st())
        if entry == "gemv" and not norm:
            return status(ops.gemm, x, t["w"], b, res, E, force="gemv", out=out)
        if entry == "gemv":
            return lib().o3v_gemv_norm_bf16(P(x), P(nw), 1e-6, P(t["w"]), P(b), P(res), P(out), M, N, K, ld(x), ld(t["w"]), ld(out), ld(res),
                                            E, st())
        if entry == "decode":
            return lib().o3v_linear_decode(P(x), P(nw), 1e-6, P(d["w"]), P(im["wp"]), *tail)
        if entry == "fp8":
            return lib().o3v_linear_decode_fp8(P(x), P(nw), 1e-6, P(im["q8"]), P(im["sc"]), *tail)
        if entry == "fp8_rows":
            return lib().o3v_linear_decode_fp8_rows(P(x), P(im["q8p"]), P(im["sc"]), *tail)
        if entry == "mxfp4":
            return lib().o3v_linear_decode_mxfp4(P(x), P(nw), 1e-6, P(im["q4"]), P(im["s4"]), *tail)
        return lib().o3v_linear_decode_mxfp4_rows(P(x), P(im["q4p"]), P(im["s4p"]), *tail)

    def ref(t):
        out, r = t["out"], (d["res"] if epi == "res" else None)
        if entry in ("gemv", "decode"):
            check_linear(out, _normed(M, N, K, 2.0)[1] if norm else d["acc"], b, r, epi)
            return
        wq = im["wq"]
        xn = _normed(M, N, K, 2.0)[0] if norm else d["x"]
        acc = xn.float() @ wq.float().t()
        want = swiglu_ref(acc, b) if epi == "swiglu" else _epi_ref(acc, b, r, E)
        if entry in ("fp8", "mxfp4"):
            close_bf16(out, want, ulps=1, atol=2e-3, frac=0.999)          # test_linear_decode_fp8_weights / test_linear_decode_mxfp4
        elif entry == "fp8_rows" and epi != "swiglu":
            close_bf16(out, want)                                         # test_linear_decode_fp8_rows
        else:                                                             # ... and test_linear_decode_mxfp4_rows: the bf16 GEMM on wq
            g = ops.gemm(d["x"], wq, b, r, E, force="gemm").float()
            if epi == "swiglu":
                close_bf16(out, g, ulps=1, atol=1e-3, frac=0.998)
            else:
                close_bf16(out, g, ulps=1, atol=2e-3, frac=0.999)

    return Spec(call, ins, {"out": (M, No, ldo, BF)}, ref, alias=("res", "out") if inplace else None)


def bad_pitch_spec(make, name, pitch, code, *a, **kw):
    """`make`'s case with ONE pitch the header rules out (not a multiple of 8 elements / 16 bytes): the contiguous call runs and is
    checked as usual, the canvas call returns the documented code and leaves every canvas wholly untouched"""
    spec = make(*a, **kw)
    if name in spec.ins:
        spec.ins[name] = (spec.ins[name][0], pitch)
    else:
        o = spec.outs[name]
        spec.outs[name] = (o[0], o[1], pitch, o[3])
    spec.expect_canvas = code
    return spec


# ------------------------------------------------------------------------------------------------ fused q/k/v
def qkv_spec(entry, M, Hq=4, Hkv=2, D=32, K=128):
    """Padded ldx only; q and the written cache slot bit-equal to the contiguous call (the dense outputs of `run`), every other
    cache slot keeps its canary.  Reference: the check of test_gemv_fused_norm_qkv_rope_cache (the unfused chain) for the bf16
    entry, of test_qkv_rope_fp8_rows (the bf16 entry on the dequantised weights) for the fp8 ones."""
    from open_o3_video_amd import _lib
    from open_o3_video_amd.weights import pack_mfma_fragments
    from oracle import model_ref
    N, Tmax, Tnew, step, slot = (Hq + 2 * Hkv) * D, 40, 6, 4, 33
    d = _lin(M, N, K, 2.0)
    g = torch.Generator().manual_seed(M + Hq)
    bias = (0.5 * torch.randn(N, generator=g)).to(BF).cuda()
    ang = torch.rand(M, Tnew, D // 2, generator=g) * 30
    cos = torch.cat([ang.cos(), ang.cos()], -1).to(BF).cuda().contiguous()
    sin = torch.cat([ang.sin(), ang.sin()], -1).to(BF).cuda().contiguous()
    tail = lambda t: (P(cos), P(sin), P(t["q"]), P(t["kc"]), P(t["vc"]), slot, Hq, Hkv, D, Tmax, Tnew, step, st())
    fp8 = entry != "bf16"
    im = _images(M, N, K, "fp8") if fp8 else None
    w = im["wq"] if fp8 else d["w"]
    wp = pack_mfma_fragments(w) if M >= 4 else None
    xin = _normed(M, N, K, 2.0)[0] if entry == "fp8_rows" else d["x"]      # the rows form takes x already normalised

    def call(t):
        x = t["x"]
        if entry == "bf16":
            return lib().o3v_gemv_norm_qkv_rope(P(x), P(d["nw"]), 1e-6, P(w), P(wp), P(bias), M, K, ld(x), *tail(t))
        if entry == "fp8":
            return lib().o3v_gemv_norm_qkv_rope_fp8(P(x), P(d["nw"]), 1e-6, P(im["q8"]), P(im["sc"]), P(bias), M, K, ld(x), *tail(t))
        return lib().o3v_qkv_rope_fp8_rows(P(x), P(im["q8p"]), P(im["sc"]), P(bias), M, K, ld(x), *tail(t))

    def after(t):
        for c in (t["kc"], t["vc"]):
            r = raw(c)
            assert (r[:, :, :slot] == CANARY16).all() and (r[:, :, slot + 1:] == CANARY16).all(), "a cache slot other than `slot` was written"
            assert not c[:, :, slot].isnan().any()
        assert not t["q"].isnan().any()

    def ref(t):
        q1 = torch.zeros(M, Hq, D, dtype=BF, device="cuda")
        k1 = torch.zeros(M, Hkv, Tmax, D, dtype=BF, device="cuda")
        v1 = torch.zeros_like(k1)
        if fp8:   # the bf16 kernel on the dequantised weights (exact in bf16)
            xr, nwr = (xin, None) if entry == "fp8_rows" else (d["x"], d["nw"])
            _lib.call("o3v_gemv_norm_qkv_rope", P(xr), P(nwr), 1e-6, P(w), P(wp), P(bias), M, K, K, P(cos), P(sin), P(q1), P(k1), P(v1), slot,
                      Hq, Hkv, D, Tmax, Tnew, step, st())
            frac = 0.998
        else:     # the unfused chain
            qkv = torch.empty(M, N, dtype=BF, device="cuda")
            _lib.call("o3v_gemv_norm_bf16", P(d["x"]), P(d["nw"]), 1e-6, P(w), P(bias), None, P(qkv), M, N, K, K, K, N, 0, ops.EPI_NONE, st())
            _lib.call("o3v_qkv_rope_cache", P(qkv), P(cos), P(sin), P(q1), P(k1), P(v1), slot, M, 1, Hq, Hkv, D, Tmax, Tnew, step, st())
            frac = 0.999
        close_bf16(t["q"], q1.float(), ulps=1, atol=2e-3, frac=frac)
        close_bf16(t["kc"][:, :, slot], k1[:, :, slot].float(), ulps=1, atol=2e-3, frac=frac)
        close_bf16(t["vc"][:, :, slot], v1[:, :, slot].float(), ulps=1, atol=2e-3, frac=frac)

    # o3v.h: the fp8 row form streams up to 3 rows (O3V_ERR_SHAPE above), the fragment form 4..32 (O3V_ERR_ARG below)
    expect = ERR_SHAPE if entry == "fp8" and M > 3 else ERR_ARG if entry == "fp8_rows" and M < 4 else OK
    cache = ((M, Hkv, Tmax, D), BF)
    return Spec(call, {"x": (xin, K + 8)}, {}, ref, expect, dense={"q": ((M, Hq, D), BF), "kc": cache, "vc": cache}, after=after)


# ------------------------------------------------------------------------------------------------ W8A8 GEMM
@functools.lru_cache(maxsize=None)
def _w8(M, N, K):
    """the operands and exact products of test_gemm_fp8_against_exact_products"""
    from open_o3_video_amd.weights import quantize_rows_fp8
    from oracle import quant_ref
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * torch.rand(M, 1, generator=g) * 3).to(BF)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
    qx, sx = quant_ref.quantize_rows(x)
    w8, sw = quantize_rows_fp8(w)
    bias = (0.1 * torch.randn(N, generator=g)).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    f8 = w8.view(torch.float8_e4m3fn).double()
    sc = sx.double()[:, None] * sw.double()[None, :]
    return dict(a8=qx.view(U8).cuda(), sa=sx.cuda(), w8=w8.cuda(), sw=sw.cuda(), bias=bias.cuda(), res=res.cuda(), bias_c=bias, res_c=res,
                prod=(qx.double() @ f8.t()) * sc, mag=(qx.double().abs() @ f8.abs().t()) * sc)


def w8a8_spec(sched, M, N, K, epi, ldo, ldr=0, inplace=False):
    from test_gpu_fp8 import _ulp_bf16
    d = _w8(M, N, K)
    E, No = EPI[epi], (N // 2 if epi == "swiglu" else N)
    b = d["bias"] if epi == "none" else None
    ins = {"a8": (d["a8"], K + 16), "w8": (d["w8"], K + 32)}     # pitches in bytes: multiples of 16
    _res_ins(ins, d, epi, ldr or ldo)

    def call(t):
        a, w, res, out = t["a8"], t["w8"], t.get("res"), t["out"]
        return lib().o3v_gemm_fp8_sched(P(a), P(d["sa"]), P(w), P(d["sw"]), P(b), P(res), P(out), M, N, K, ld(a), ld(w), ld(out), ld(res), E,
                                        sched, st())

    def ref(t):   # the bounds of test_gemm_fp8_against_exact_products, as written there
        got, prod, mag = t["out"].float().cpu(), d["prod"], d["mag"]
        acc_tol = (mag * K * 2.0 ** -24).float()
        if epi == "none":
            want = (prod + d["bias_c"].double()).float()
            assert ((got - want).abs() <= _ulp_bf16(want) + acc_tol).all()
            assert (got == want.to(BF).float()).float().mean() > 0.97
        elif epi == "res":
            want = prod.float().to(BF).float() + d["res_c"].float()
            assert ((got - want).abs() <= 2 * _ulp_bf16(want) + _ulp_bf16(prod.float()) + acc_tol).all()
            assert (got == want.to(BF).float()).float().mean() > 0.95
        else:
            p = prod.float().to(BF).float().view(M, N // 32, 2, 16)
            want = (torch.nn.functional.silu(p[:, :, 0]).to(BF).float() * p[:, :, 1]).reshape(M, N // 2)
            assert ((got - want).abs() <= 4 * _ulp_bf16(want) + 0.02 * want.abs() + 1e-3).all()
            assert (got == want.to(BF).float()).float().mean() > 0.9

    return Spec(call, ins, {"out": (M, No, ldo, BF)}, ref, alias=("res", "out") if inplace else None,
                expect=ERR_SHAPE if sched == 2 and K < 512 else OK)   # o3v.h: schedule 2 needs an even number >= 4 of K-tiles


# ------------------------------------------------------------------------------------------------ row kernels
def rows_spec(kind, rows, cols):
    """ld_in = cols + 8, ld_out / ld_q = cols + 16; the dense scale / code outputs sit in canvases (guards only) too"""
    from oracle import model_ref, quant_ref
    from open_o3_video_amd import weights as W
    g = torch.Generator().manual_seed(rows * 7 + cols)
    x = torch.randn(rows, cols, generator=g) * 3
    if "quant" in kind:
        x = x * torch.logspace(-3, 2, rows)[:, None]
    x = (x + (0.5 if kind == "layernorm" else 0)).to(BF).cuda()
    w = (1 + 0.1 * torch.randn(cols, generator=g)).to(BF).cuda()
    b = (0.2 * torch.randn(cols, generator=g)).to(BF).cuda()
    ins, L = {"x": (x, cols + 8)}, lib()
    if kind in ("rmsnorm", "layernorm"):
        outs = {"out": (rows, cols, cols + 16, BF)}
        if kind == "rmsnorm":
            call = lambda t: status(ops.rmsnorm, t["x"], w, 1e-6, out=t["out"])
            ref = lambda t: close_bf16(t["out"], model_ref.rmsnorm(x.cpu(), w.cpu(), 1e-6), ulps=1, atol=0, frac=1.0)       # test_rmsnorm
        else:
            call = lambda t: L.o3v_layernorm(P(t["x"]), P(w), P(b), P(t["out"]), rows, cols, ld(t["x"]), ld(t["out"]), 1e-6, st())
            ref = lambda t: close_bf16(t["out"], torch.nn.functional.layer_norm(x.float().cpu(), (cols,), w.float().cpu(), b.float().cpu(), 1e-6),
                                       ulps=1, atol=1e-3, frac=0.999)                                                      # test_layernorm
        return Spec(call, ins, outs, ref, expect=ERR_SHAPE if cols > 8192 else OK)   # o3v.h: at most 8192 columns
    if kind in ("quant_fp8", "rmsnorm_quant_fp8"):
        outs = {"q": (rows, cols, cols + 16, U8), "scale": (rows, 1, 1, F32)}
        if kind == "quant_fp8":
            call = lambda t: L.o3v_quantize_rows_fp8(P(t["x"]), P(t["q"]), P(t["scale"]), rows, cols, ld(t["x"]), ld(t["q"]), st())
            y = lambda: x
        else:
            call = lambda t: L.o3v_rmsnorm_quantize_fp8(P(t["x"]), P(w), P(t["q"]), P(t["scale"]), rows, cols, ld(t["x"]), ld(t["q"]), 1e-6, st())
            y = lambda: ops.rmsnorm(x, w, 1e-6)         # the bf16 rows o3v_rmsnorm would have written (test_rmsnorm_quantize_fp8)

        def ref(t):                                     # bit for bit against oracle/quant_ref.py
            if kind == "rmsnorm_quant_fp8" and cols > 8192:
                return ref_wide(t)
            qr, sr = quant_ref.quantize_rows(y().cpu())
            assert torch.equal(t["scale"].cpu()[:, 0], sr) and torch.equal(t["q"].cpu(), qr.view(U8))

        def ref_wide(t):
            """Past o3v_rmsnorm's 8192 columns the rows it would have written do not exist; the oracle's rmsnorm stands in.  Its sum of
            squares runs in another order, so its rows may differ from the kernel's by one bf16 ulp (test_rmsnorm allows exactly
            that) and a code may then sit one step away: no bit-for-bit claim.  Bound per element, from the number formats alone, with
            s the kernel's scale: |fp8(q) * s - y| <= 2^-8 |y| (one bf16 ulp of y) + 2^-4 |y'| (half an e4m3 step, 3 mantissa bits;
            y' = y moved by that ulp) + 2^-10 s (half the subnormal step 2^-9 s); s is the power of two that puts the row maximum,
            give or take that ulp, into (224, 448]."""
            yr = model_ref.rmsnorm(x.cpu(), w.cpu(), 1e-6).float()
            sc = t["scale"].cpu()[:, 0]
            got = t["q"].cpu().view(torch.float8_e4m3fn).float() * sc[:, None]
            u = 2.0 ** -8
            assert ((got - yr).abs() <= u * yr.abs() + 2.0 ** -4 * (1 + u) * yr.abs() + 2.0 ** -10 * sc[:, None]).all()
            amax = yr.abs().amax(dim=1)
            assert (torch.log2(sc) == torch.log2(sc).round()).all() and (amax * (1 - u) <= 448 * sc).all() and (amax * (1 + u) > 224 * sc).all()
        return Spec(call, ins, outs, ref)
    outs = {"codes": (rows, cols // 2, cols // 2, U8), "scales": (rows, cols // 32, cols // 32, U8)}
    call = lambda t: L.o3v_quantize_rows_mxfp4(P(t["x"]), P(t["codes"]), P(t["scales"]), rows, cols, ld(t["x"]), st())

    def ref(t):                                         # bit for bit against weights.py (test_quantize_rows_mxfp4_bit_exact)
        qr, sr = W.quantize_rows_mxfp4(x)
        assert torch.equal(t["codes"], qr) and torch.equal(t["scales"], sr)
        assert torch.equal(W.dequantize_rows_mxfp4(t["codes"], t["scales"]), W.dequantize_rows_mxfp4(qr, sr))
    return Spec(call, ins, outs, ref)


# ------------------------------------------------------------------------------------------------ the table
CASES = []


def add(make, *a, **kw):
    name = lambda v: v.__name__[:-5] if callable(v) else str(v)
    CASES.append(pytest.param(make, a, kw, id="-".join([name(make)] + [name(v) for v in a] + [f"{k}{v}" for k, v in kw.items()])))


def ldo_pair(n):
    return (r8(n) + 8, n + 3)            # a multiple of 8 (vector stores stay possible) and an odd pitch


def ldr_other(n, ldo):
    return n + 5 if ldo % 8 == 0 else r8(n) + 16      # a residual pitch that differs from ldo, odd or even the other way round


for _entry in ("tile128", "tile256", "phased", "auto"):
    # ragged M and N on the 128 tile; odd N (scalar epilogue, last column in a partly filled fragment); second tile row and column
    # of the 256 tile at the smallest K the phased kernel takes
    for _M, _N, _K in ((130, 200, 128), (130, 197, 128), (260, 264, 256), (300, 197, 256)):
        for _ldo in ldo_pair(_N):
            add(gemm_spec, _entry, _M, _N, _K, "none", _ldo, bias=False)
            for _epi in ("none", "gelu", "gelu_tanh"):
                add(gemm_spec, _entry, _M, _N, _K, _epi, _ldo)
            for _ldr in (_ldo + 8, _N + 5):
                add(gemm_spec, _entry, _M, _N, _K, "res", _ldo, _ldr)
            add(gemm_spec, _entry, _M, _N, _K, "res", _ldo, inplace=True)
    for _M, _N, _K in ((130, 192, 128), (260, 320, 256)):
        for _ldo in (_N // 2 + 8, _N // 2 + 1):          # the second reaches the scalar SWIGLU branch
            add(gemm_spec, _entry, _M, _N, _K, "swiglu", _ldo)

# splits clamped to 1 at K = 64; at (576, 6) the last split gets no k-steps
for _M, _N, _K, _S in ((40, 197, 448, 3), (17, 200, 64, 4), (100, 264, 576, 6)):
    for _ldo in ldo_pair(_N):
        for _epi in ("none", "gelu"):
            add(splitk_spec, _M, _N, _K, _S, _epi, _ldo)
        for _ldr in (_ldo + 8, _N + 5):
            add(splitk_spec, _M, _N, _K, _S, "res", _ldo, _ldr)
        add(splitk_spec, _M, _N, _K, _S, "res", _ldo, inplace=True)

# scalar GEMV (K % 32 != 0 keeps 4..8 rows off the matrix cores): odd N, not a multiple of the wave's row group; K = 1096 runs more
# than one 512-wide k-trip with a tail
for _norm in (False, True):
    for _M, _N, _K in [(m, n, 136) for m in (1, 3, 5, 8) for n in (197, 1001)] + [(1, 197, 1096)]:
        for _ldo in (r8(_N + 8), _N + 3):
            for _epi in ("none", "gelu"):
                add(decode_spec, "gemv", _M, _N, _K, _epi, _ldo, norm=_norm)
            add(decode_spec, "gemv", _M, _N, _K, "res", _ldo, ldr_other(_N, _ldo), norm=_norm, bias=False)
        add(decode_spec, "gemv", _M, _N, _K, "res", r8(_N + 8), norm=_norm, bias=False, inplace=True)
    for _M in (1, 3, 5, 8):                              # N / 2 = 112 is not a multiple of 16 rows per group
        for _ldo in (120, 115):
            add(decode_spec, "gemv", _M, 224, 136, "swiglu", _ldo, norm=_norm)

# skinny matrix-core GEMM: row-major W through o3v_gemv_bf16, the fragment-major image through o3v_linear_decode
for _entry in ("gemv", "decode"):
    for _M in (4, 9, 16, 17, 32):
        for _N, _K in ((208, 160), (48, 96)):
            for _ldo in (_N + 8, _N + 3):
                add(decode_spec, _entry, _M, _N, _K, "none", _ldo)
                add(decode_spec, _entry, _M, _N, _K, "res", _ldo, ldr_other(_N, _ldo))
                add(decode_spec, _entry, _M, _N, _K, "res", _ldo, inplace=True)
            if _M <= 16:                                 # a fused norm is not offered above 16 rows
                add(decode_spec, _entry, _M, _N, _K, "none", _N + 8, norm=True)
        for _N, _K in ((224, 160), (64, 96)):
            for _ldo in (_N // 2 + 8, _N // 2 + 1):
                add(decode_spec, _entry, _M, _N, _K, "swiglu", _ldo)

# fp8 / MXFP4 decode linears at the smallest legal (N, K); N = 197 where the header allows it (the row forms)
for _entry, _Ms in (("fp8", (1, 2, 3)), ("mxfp4", (1, 2, 3)), ("fp8_rows", (4, 21)), ("mxfp4_rows", (4, 21))):
    for _M in _Ms:
        for _N in (48, 197) if _entry in ("fp8", "mxfp4") else (48,):
            for _ldo in ldo_pair(_N):
                add(decode_spec, _entry, _M, _N, 128, "none", _ldo, norm=_entry in ("fp8", "mxfp4"))
                add(decode_spec, _entry, _M, _N, 128, "res", _ldo, ldr_other(_N, _ldo))
        add(decode_spec, _entry, _M, 48, 128, "res", 56, inplace=True)
        for _ldo in (40, 35):
            add(decode_spec, _entry, _M, 64, 128, "swiglu", _ldo, bias=False)

for _entry in ("bf16", "fp8", "fp8_rows"):
    for _M in (1, 9):
        add(qkv_spec, _entry, _M)

for _sched in (1, 2):
    for _M, _N, _K in ((130, 200, 256), (130, 200, 512), (130, 197, 256)):
        for _ldo in ldo_pair(_N):
            add(w8a8_spec, _sched, _M, _N, _K, "none", _ldo)
            add(w8a8_spec, _sched, _M, _N, _K, "res", _ldo, ldr_other(_N, _ldo))
        add(w8a8_spec, _sched, _M, _N, _K, "res", r8(_N) + 8, inplace=True)
    for _K in (256, 512):
        for _ldo in (96 + 8, 96 + 1):
            add(w8a8_spec, _sched, 130, 192, _K, "swiglu", _ldo)

# rows {1, 5}: five rows give the second workgroup a single live wave; columns on and just past each template boundary
for _kind in ("rmsnorm", "layernorm", "quant_fp8", "rmsnorm_quant_fp8", "quant_mxfp4"):
    for _rows in (1, 5):
        for _cols in (2048, 2080, 4096, 4128, 8192) if _kind == "quant_mxfp4" else (2048, 2056, 4096, 4104, 8192, 8200):
            add(rows_spec, _kind, _rows, _cols)


# one pitch the header rules out per family: the documented code, every canvas wholly untouched
add(bad_pitch_spec, gemm_spec, "a", 128 + 4, ERR_SHAPE, "tile128", 130, 200, 128, "none", 208)
add(bad_pitch_spec, gemm_spec, "w", 256 + 4, ERR_SHAPE, "phased", 260, 264, 256, "none", 272)
add(bad_pitch_spec, gemm_spec, "a", 256 + 12, ERR_SHAPE, "auto", 260, 264, 256, "res", 272, 280)
add(bad_pitch_spec, splitk_spec, "w", 448 + 4, ERR_SHAPE, 40, 197, 448, 3, "none", 208)
add(bad_pitch_spec, decode_spec, "x", 136 + 4, ERR_SHAPE, "gemv", 3, 197, 136, "none", 208)
add(bad_pitch_spec, decode_spec, "w", 136 + 4, ERR_SHAPE, "gemv", 3, 197, 136, "none", 208, norm=True)
add(bad_pitch_spec, decode_spec, "x", 160 + 4, ERR_SHAPE, "decode", 9, 208, 160, "none", 216)
for _entry, _M in (("fp8", 2), ("mxfp4", 2), ("fp8_rows", 4), ("mxfp4_rows", 4)):
    add(bad_pitch_spec, decode_spec, "x", 128 + 4, ERR_SHAPE, _entry, _M, 48, 128, "none", 56)
add(bad_pitch_spec, qkv_spec, "x", 128 + 4, ERR_SHAPE, "bf16", 1)
add(bad_pitch_spec, qkv_spec, "x", 128 + 4, ERR_SHAPE, "fp8_rows", 9)
add(bad_pitch_spec, w8a8_spec, "a8", 256 + 8, ERR_SHAPE, 1, 130, 200, 256, "none", 208)
add(bad_pitch_spec, w8a8_spec, "w8", 512 + 8, ERR_SHAPE, 2, 130, 200, 512, "none", 208)
for _kind in ("rmsnorm", "layernorm"):
    add(bad_pitch_spec, rows_spec, "x", 2048 + 4, ERR_ARG, _kind, 5, 2048)
    add(bad_pitch_spec, rows_spec, "out", 2048 + 4, ERR_ARG, _kind, 5, 2048)
for _kind in ("quant_fp8", "rmsnorm_quant_fp8"):
    add(bad_pitch_spec, rows_spec, "x", 2048 + 4, ERR_ARG, _kind, 5, 2048)
    add(bad_pitch_spec, rows_spec, "q", 2048 + 4, ERR_ARG, _kind, 5, 2048)


@pytest.mark.parametrize("make,args,kw", CASES)
def test_pitches(dev, make, args, kw):
    run(dev, make(*args, **kw))
