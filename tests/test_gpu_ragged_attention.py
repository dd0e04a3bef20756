"""o3v_attn_decode_ragged on the GPU: a decode attention whose context is per row (continuous batching).  Every live row must be
bit-identical to o3v_attn_decode run on that row alone, append exactly its staging row and read nothing at or behind it; idle rows
touch nothing and give +0; the bound of include/o3v.h against fp64; the argument refusals launch nothing."""
import math

import pytest
import torch

import kernel_ops as ko
import ragged_ops as ro
from ragged_ops import raw

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U = 2.0 ** -8          # bf16 unit round-off: the coefficient of the decode kernels' bound in include/o3v.h
CTXS = [1, 31, 32, 33, 128, 129, 513]
MIX5 = {0: [1, 32, 129, 513, 31], 1: [33, 128, 513, 1, 129]}     # both mixes together hold every context of CTXS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open_o3_video_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _ctxs(B, k):
    return MIX5[k % 2] if B == 5 else [CTXS[k % len(CTXS)]]


def _reference_row(c, b, nsplit):
    """o3v_attn_decode with B = 1 on row b's cache, which already holds the staging row at slot ctx_b - 1"""
    return ko.attn_decode(c["q"][b:b + 1], c["kfull"][b:b + 1].contiguous(), c["vfull"][b:b + 1].contiguous(), None, c["ctxs"][b], nsplit,
                          c["scale"], poison=True)[0]


def _check(c, nsplit):
    kc, vc = c["kc"].clone(), c["vc"].clone()
    out = ro.attn_decode_ragged(c["q"], kc, vc, c["knew"], c["vnew"], c["row_base"], c["step"], nsplit, c["scale"], poison=True)
    assert torch.isfinite(out.float()).all(), nsplit
    for b, ctx in enumerate(c["ctxs"]):
        if not c["live"][b]:
            assert (raw(out[b]) == 0).all(), (nsplit, b, "an idle row's output must be +0")
            assert torch.equal(raw(kc[b]), raw(c["kc"][b])) and torch.equal(raw(vc[b]), raw(c["vc"][b])), (nsplit, b, "idle row's cache")
            continue
        ref = _reference_row(c, b, nsplit)
        assert torch.equal(out[b], ref), (nsplit, b, ctx, (out[b].float() - ref.float()).abs().max().item())
        for name, cache, before, new in (("K", kc, c["kc"], c["knew"]), ("V", vc, c["vc"], c["vnew"])):
            assert torch.equal(raw(cache[b, :, ctx - 1]), raw(new[b])), (name, nsplit, b, "slot ctx-1 must hold the staging row")
            assert torch.equal(raw(cache[b, :, :ctx - 1]), raw(before[b, :, :ctx - 1])), (name, nsplit, b, "slots below were written")
            assert torch.equal(raw(cache[b, :, ctx:]), raw(before[b, :, ctx:])), (name, nsplit, b, "slots behind were written")
    return out


# ------------------------------------------------------------------------------------------------ bit-identity and canaries
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Hq,Hkv", [(7, 1), (16, 2), (8, 8), (28, 4)])
def test_rows_bit_identical_to_the_single_row_kernel_d128(dev, Hq, Hkv, B):
    """Mixed contexts in one call; slots >= ctx_b - 1 arrive holding NaN (0xFFFF), part_o / part_ml / out arrive holding NaN."""
    for k, nsplit in enumerate((1, 3, 8, -1, -3, -8)):        # 8 splits: more splits than 32-key tiles up to ctx = 129
        c = ro.ragged_case(dev, _ctxs(B, k + Hq), Hq, Hkv, 128, seed=Hq * 31 + B * 7 + k)
        _check(c, nsplit)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D,Hq,Hkv", [(32, 4, 2), (64, 4, 1)])
def test_rows_bit_identical_scalar_form_small_heads(dev, D, Hq, Hkv, B):
    for k, nsplit in enumerate((-1, -3, -8, 3)):              # either sign is the scalar form at these head sizes
        c = ro.ragged_case(dev, _ctxs(B, k + D), Hq, Hkv, D, seed=D + B * 5 + k)
        _check(c, nsplit)


@pytest.mark.parametrize("B", [1, 5])
def test_every_context_of_the_list_alone_and_mixed(dev, B):
    """Each context of the list at least once per form (the mixes above rotate; this one walks the whole list)."""
    for k in range(len(CTXS) if B == 1 else 2):
        c = ro.ragged_case(dev, _ctxs(B, k), 8, 2, 128, seed=900 + k + B)
        _check(c, 3)
        _check(c, -3)


# ------------------------------------------------------------------------------------------------ idle rows
@pytest.mark.parametrize("nsplit", [1, 3, -3])
def test_idle_rows_touch_nothing_and_give_zero(dev, nsplit):
    Tmax = 140
    # contexts <= 0 (an empty slot; a retired row: a large negative base) and Tmax + 1 (a row past its capacity) between live rows
    ctxs = [33, 0, -(1 << 30) + 6, Tmax + 1, 129, -7, Tmax]
    c = ro.ragged_case(dev, ctxs, 8, 2, 128, seed=5 + abs(nsplit), Tmax=Tmax)
    assert c["live"] == [True, False, False, False, True, False, True]
    _check(c, nsplit)
    c = ro.ragged_case(dev, [0, 20, 70], 4, 2, 32, seed=8, Tmax=64)      # the 32-wide form of the tiny fixtures
    assert c["live"] == [False, True, False]
    _check(c, nsplit)


# ------------------------------------------------------------------------------------------------ accuracy
def test_accuracy_against_fp64(dev):
    """|out - ref| <= u sum_j p_j |v_j - ref| + u |ref| (+ 1e-6) per element: the bound include/o3v.h derives for o3v_attn_decode."""
    ctxs = [513, 33, 129, 1, 300]
    c = ro.ragged_case(dev, ctxs, 8, 2, 128, seed=77)
    for nsplit in (3, -3):
        out = _check(c, nsplit).cpu().double()
        q, K, V = c["q"].cpu(), c["kfull"].cpu(), c["vfull"].cpu()
        worst = 0.0
        for b, ctx in enumerate(ctxs):
            for h in range(8):
                k, v = K[b, h // 4, :ctx].double(), V[b, h // 4, :ctx].double()
                p = torch.softmax((k @ q[b, h].double()) * c["scale"], dim=0)
                ref = p @ v
                spr = (p[:, None] * (v - ref[None]).abs()).sum(0)
                err, tol = (out[b, h] - ref).abs(), U * spr + U * ref.abs() + 1e-6
                worst = max(worst, float((err / tol).max()))
                assert (err <= tol).all(), (nsplit, b, h, float((err / tol).max()))
        print(f"ragged nsplit={nsplit}: max err/tol {worst:.3f}")


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(dev):
    from open_o3_video_amd import _lib
    c = ro.ragged_case(dev, [33, 40], 8, 2, 128, seed=3)

    def refused(code, q=None, nsplit=2, **kw):
        q = c["q"] if q is None else q
        args = dict(knew=c["knew"], vnew=c["vnew"], row_base=c["row_base"], kc=c["kc"].clone(), vc=c["vc"].clone())
        args.update({k: v for k, v in kw.items() if k in args})
        extra = {k: v for k, v in kw.items() if k not in args}
        out = torch.full(q.shape, float("nan"), dtype=BF, device=dev)
        with pytest.raises(_lib.O3VError) as e:
            ro.attn_decode_ragged(q, args["kc"], args["vc"], args["knew"], args["vnew"], args["row_base"], c["step"], nsplit, c["scale"],
                                  poison=True, out=out, **extra)
        assert e.value.code == code, (e.value.code, code, kw)
        torch.cuda.synchronize()
        assert torch.isnan(out.float()).all(), "a refused call must not launch"
        assert torch.equal(raw(args["kc"]), raw(c["kc"])) and torch.equal(raw(args["vc"]), raw(c["vc"]))

    refused(_lib.ERR_ARG, knew=None)
    refused(_lib.ERR_ARG, vnew=None)
    refused(_lib.ERR_ARG, row_base=None)
    refused(_lib.ERR_ARG, Hkv=3)                                     # Hq % Hkv != 0
    for ns in (0, 65, -65):
        refused(_lib.ERR_ARG, nsplit=ns)
    refused(_lib.ERR_SHAPE, q=torch.zeros(2, 18, 128, dtype=BF, device=dev))    # 9 query heads per kv head
    refused(_lib.ERR_SHAPE, D=80)
    refused(_lib.ERR_SHAPE, D=256)
