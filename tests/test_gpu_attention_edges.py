"""Edge probes of the attention kernels against fp64 references: every entry point (o3v_attn_tiles for the ViT segments and the
causal prefill, o3v_attn_tiles_prefix, o3v_attn_decode on the MFMA and the scalar kernels, o3v_attn_decode_group,
o3v_attn_decode_group_prefix) with four families of inputs.

  A  key-set probes: q = 0, so every visible key scores 0, p = exp2(0) = 1 and the merge weights are 1.  V holds {0, 1}: column 0
     is 1 on every key (output 1: the normalisation), column 1 marks one key every query sees (output 1/n: the key count), the
     other columns mark at most three keys each, placed on the edges of the kernels (k_lo - 1, k_lo, ctx - 1, multiples of 32 /
     64 / 128 and their neighbours, the first and last key of every split and wave, P - 1 and P, segment ends, the causal
     diagonal).  The output is c / n exactly in fp32; it must sit within 1 bf16 ulp of the fp64 value.
  B  needles and decoys: q and K carry a +-1 binary code of the key position (16 * 16 per bit), so the code of the needle key
     beats every other visible key by >= 30 nats; the output must be the needle's V row within 1 bf16 ulp.  Decoys score
     another >= 30 nats above the needle at keys the query must not see: below k_lo, past ctx, a non-leader row's prefix slots,
     prompt slots past prefix_len, above the causal diagonal, in another ViT segment.
  C  peaked random inputs: scores of std 10 nats and a sink key at k_lo (~30 nats), compared per element with the bound the
     kernels' rounding points imply (P rounded to bf16, fp32 accumulation, bf16 output; derived in include/o3v.h):
        decode kernels (the row sum adds the rounded P):    |out - ref| <= 2^-8 * sum_j p_j |v_j - ref| + 2^-8 |ref| + 1e-6,
        attn_tiles (the row sum adds the unrounded p):      |out - ref| <= 2^-8 * sum_j p_j |v_j - ref| + 2^-7 |ref| + 1e-6,
     and over the whole tensor ||out - ref||_2 <= 2^-7 ||ref||_2.
  D  poisoned memory, in every probe: what the call must never read holds NaN (bf16 0x7FC0 and 0xFFFF): K/V slots from ctx (or
     k_len) up to Tmax, prompt-entry slots from prefix_len up to its capacity, own-cache slots past the generated tokens, the
     prefix slots of non-leader rows in the group layout.  out, part_o and part_ml start as NaN, so a slot a kernel fails to
     write shows up.  (Family B puts its decoys on every other row of those regions and NaN on the rest.)

Contract kept by the engine and by these tests: slots below k_lo (left padding) are written by the prefill, so they hold finite
values; the kernels may read them and must mask them.  They are finite here (decoys in B) and never NaN."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
NAN_BITS = (0x7FC0, -1)   # int16 views of the bf16 NaNs 0x7FC0 and 0xFFFF
AMP = 16.0                # code amplitude of q and K (family B)
DECOY = 512.0             # K value on a decoy dimension: > 2 * bits * AMP, so a decoy beats any needle
SIGMA_C = 10.0            # family C: std of the scores in nats


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from open_o3_video_amd import _lib
    _lib.load()
    return torch.device("cuda")


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def nan_rows_(x, start=0, step=1):
    """NaN into rows start, start + step, ... of a bf16 view (token axis -2), alternating the two bit patterns."""
    i = x.view(torch.int16)
    i[..., start::2 * step, :] = NAN_BITS[0]
    i[..., start + step::2 * step, :] = NAN_BITS[1]


def ulp_bf16(x):
    """one bf16 ulp at |x| (the normal spacing below 2^-126)"""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def assert_within_ulp(out, ref, what):
    """out bf16, ref fp64: no NaN, |out - ref| <= 1 bf16 ulp of ref"""
    o = out.to(F64)
    assert not torch.isnan(o).any(), f"{what}: {int(torch.isnan(o).sum())} NaN outputs (unwritten or read a poisoned slot)"
    err = (o - ref).abs()
    bad = err > ulp_bf16(ref)
    if bad.any():
        idx = tuple(int(t) for t in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} outputs off by more than 1 bf16 ulp; first at {idx}: "
                             f"got {o[idx].item():.8g}, want {ref[idx].item():.8g}")


def assert_rounding_bound(out, ref, spread, what, ref_coef=2.0 ** -8):
    """Family C: per element |out - ref| <= 2^-8 spread + ref_coef |ref| + 1e-6 (spread = sum_j p_j |v_j - ref|; ref_coef 2^-8
    for the decode kernels, 2^-7 for attn_tiles, whose row sum adds the unrounded p), and the relative RMS over the whole
    tensor <= 2^-7."""
    o = out.to(F64)
    assert not torch.isnan(o).any(), f"{what}: {int(torch.isnan(o).sum())} NaN outputs"
    err = (o - ref).abs()
    tol = 2.0 ** -8 * spread + ref_coef * ref.abs() + 1e-6
    bad = err > tol
    if bad.any():
        idx = tuple(int(t) for t in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} outputs outside the rounding bound; first at {idx}: got "
                             f"{o[idx].item():.6g}, want {ref[idx].item():.6g} +- {tol[idx].item():.3g}")
    rel = ((o - ref).norm() / ref.norm()).item()
    assert rel <= 2.0 ** -7, f"{what}: relative RMS error {rel:.3g} > 2^-7"


def ref64(q, K, V, mask, scale, spread=False):
    """fp64 softmax attention.  q [B, Sq, Hq, D], K / V [B, Hkv, T, D] (finite wherever mask is set), mask [B, Sq, T].
    Returns ref [B, Sq, Hq, D] and, with spread, sum_j p_j |v_j - ref| of the same shape (rows without a key: NaN)."""
    B, Sq, Hq, D = q.shape
    rep = Hq // K.shape[1]
    ref = torch.empty(B, Sq, Hq, D, dtype=F64, device=q.device)
    spr = torch.empty_like(ref) if spread else None
    for b in range(B):
        for hk in range(K.shape[1]):
            k = torch.nan_to_num(K[b, hk].to(F64))   # NaN only where masked (checked by the callers' builders)
            v = torch.nan_to_num(V[b, hk].to(F64))
            for r in range(rep):
                h = hk * rep + r
                s = (q[b, :, h].to(F64) @ k.T) * scale
                p = torch.softmax(s.masked_fill(~mask[b], -math.inf), dim=-1)
                o = p @ v
                ref[b, :, h] = o
                if spread:
                    for i in range(0, Sq, 32):
                        spr[b, i:i + 32, h] = (p[i:i + 32, :, None] * (v[None] - o[i:i + 32, None]).abs()).sum(1)
    return ref, spr


def code_bits(T):
    return max(1, (T - 1).bit_length())


def codes(pos, nb):
    """+-1 binary code of each position: [len(pos), nb]"""
    pos = torch.as_tensor(pos, dtype=torch.long)
    return ((pos[:, None] >> torch.arange(nb)) & 1).to(torch.float32) * 2 - 1


def mfma_splits(ctx, nsplit, kbeg=0):
    """(split, wave) key ranges of attn_decode_mfma_body: chunk rounded up to 128 keys, four waves of chunk / 4"""
    chunk = -(-(ctx - kbeg) // nsplit)
    chunk = -(-chunk // 128) * 128
    out = []
    for s in range(nsplit):
        for w in range(4):
            a = kbeg + s * chunk + w * (chunk // 4)
            out.append((a, min(a + chunk // 4, ctx)))
    return out


def scalar_splits(ctx, nsplit, D):
    """split ranges of attn_decode_kernel (chunk rounded to 16 * KPW keys) and the first / last key of each wave"""
    kpw = 64 // (D // 8)
    chunk = -(-ctx // nsplit)
    chunk = -(-chunk // (16 * kpw)) * (16 * kpw)
    out = []
    for s in range(nsplit):
        a, e = s * chunk, min(s * chunk + chunk, ctx)
        out.append((a, e))
        for w in range(4):
            out.append((a + w * kpw, a + w * kpw + kpw))
    return out


def edge_keys(lo, hi, extra=(), ranges=()):
    """Edge keys inside [lo - 1, hi): the ends, multiples of 32 / 64 / 128 and their neighbours, the given extra keys, the first
    and last key of each (a, e) range."""
    ks = {lo - 1, lo, lo + 1, hi - 2, hi - 1, *extra}
    for m in range(32, hi + 1, 32):
        ks.update((m - 1, m, m + 1))
    for a, e in ranges:
        if a < e:
            ks.update((a, e - 1))
    return sorted(k for k in ks if lo - 1 <= k < hi and k >= 0)


class Probe:
    """Logical inputs of one call: q [B, Sq, Hq, D], K / V [B, Hkv, T, D] (bf16, CPU), mask [B, Sq, T] (visible keys), and
    the family's expectations.  The builders of the entry points map K / V into their physical buffers."""

    def __init__(self, fam, B, Sq, Hq, Hkv, T, D, mask, scale, seed, edges, always, bands=(), lo=None, sink=None,
                 needle_extra=None, rot=0, unrounded_sum=False):
        g = torch.Generator().manual_seed(seed)
        self.fam, self.mask, self.scale, self.D = fam, mask, scale, D
        self.ref_coef = 2.0 ** -7 if unrounded_sum else 2.0 ** -8   # family C bound (include/o3v.h)
        self.qvalid = mask.any(-1)                               # [B, Sq]: rows with at least one key
        lo = lo if lo is not None else [0] * B
        q = torch.zeros(B, Sq, Hq, D)
        K = torch.randn(B, Hkv, T, D, generator=g)
        V = torch.randn(B, Hkv, T, D, generator=g)
        self.needle = None
        self.decoy_k = None
        if fam == "A":
            V.zero_()
            V[..., 0] = 1.0
            for b in range(B):
                for j in always[b]:
                    V[b, :, j, 1] = 1.0
                E = edges[b]
                for h in range(Hkv):
                    sub = E if len(E) <= 3 * (D - 2) else E[h::Hkv]
                    assert len(sub) <= 3 * (D - 2), "too many probe keys for the columns"
                    for i, j in enumerate(sub):
                        V[b, h, j, 2 + (i + 7 * h) % (D - 2)] = 1.0
        elif fam == "B":
            nb = code_bits(T)
            gd = nb                                              # global decoy dimension
            assert nb + 1 + len(bands) + 2 <= D, "no room for the code"
            K[..., :nb] = AMP * codes(range(T), nb)
            K[..., nb:nb + 1 + len(bands)] = 0.0
            q[..., nb + 1 + len(bands):] = torch.randn(B, Sq, Hq, D - nb - 1 - len(bands), generator=g)
            q[..., gd] = AMP
            for b in range(B):
                K[b, :, :lo[b], gd] = DECOY                     # invisible to every query of the row
            for m, (rows, keys) in enumerate(bands):            # rows of band m must not see keys; they see DECOY there
                x = nb + 1 + m
                for b, i in rows:
                    q[b, i, :, x] = AMP
                for b, j in keys:
                    K[b, :, j, x] = DECOY
            self.needle = torch.full((B, Sq, Hq), -1, dtype=torch.long)
            for b in range(B):
                for i in range(Sq):
                    if not self.qvalid[b, i]:
                        continue
                    vis = [j for j in (edges[b] + (needle_extra(b, i) if needle_extra else [])) if mask[b, i, j]]
                    for h in range(Hq):
                        n = vis[(rot + i * Hq + h) % len(vis)]
                        self.needle[b, i, h] = n
                        q[b, i, h, :nb] = AMP * codes([n], nb)[0]
            dk = torch.zeros(D)                                 # K row of the physical decoys (NaN-free half of the unread slots)
            dk[:nb] = AMP * codes([0], nb)[0]
            dk[gd] = DECOY
            self.decoy_k = dk.to(BF)
        else:
            q = SIGMA_C * torch.randn(B, Sq, Hq, D, generator=g)
            xs = D - 1                                          # sink dimension: every query 8, the sink key ~30 nats / 8
            q[..., xs] = 8.0
            K[..., xs] = 0.0
            for b in range(B):
                for j in sink[b]:
                    K[b, :, j, xs] = round(30.0 / (8.0 * scale))
        self.q, self.K, self.V = q.to(BF), K.to(BF), V.to(BF)
        if fam == "B":
            self.check_margins()

    def decoy_rows_(self, xk, xv, g):
        """Family B: decoys on the even rows of an unread region, NaN on the odd ones; A / C: NaN everywhere."""
        if self.fam == "B":
            xk[..., 0::2, :] = self.decoy_k
            xv[..., 0::2, :] = torch.randn(xv[..., 0::2, :].shape, generator=g).to(BF)
            nan_rows_(xk, 1, 2)
            nan_rows_(xv, 1, 2)
        else:
            nan_rows_(xk)
            nan_rows_(xv)

    def check_margins(self):
        """the needle beats every other visible key, and every decoy beats the needle, by >= 30 nats (fp64 on the bf16 values)"""
        B, Sq, Hq, D = self.q.shape
        rep = Hq // self.K.shape[1]
        dk = self.decoy_k.double()
        for b in range(B):
            for h in range(Hq):
                s = (self.q[b, :, h].double() @ self.K[b, h // rep].double().T) * self.scale   # [Sq, T]
                for i in range(Sq):
                    if not self.qvalid[b, i]:
                        continue
                    n = int(self.needle[b, i, h])
                    vis = self.mask[b, i].clone()
                    sn = s[i, n].item()
                    vis[n] = False
                    if vis.any():
                        assert sn - s[i][vis].max().item() >= 30.0, (b, i, h, n)
                    dec = ~self.mask[b, i] & (s[i] > sn)
                    assert (s[i][dec] - sn >= 30.0).all(), (b, i, h)
                    assert (self.q[b, i, h].double() @ dk).item() * self.scale - sn >= 30.0

    def check(self, out, what, dev):
        """out [B, Sq, Hq, D] (bf16, device), rows without a key are not checked"""
        qv = self.qvalid.to(dev)
        if self.fam == "B":
            B, Sq, Hq, D = self.q.shape
            rep = Hq // self.K.shape[1]
            want = torch.zeros(B, Sq, Hq, D, dtype=F64)
            for b in range(B):
                for i in range(Sq):
                    for h in range(Hq):
                        n = int(self.needle[b, i, h])
                        if n >= 0:
                            want[b, i, h] = self.V[b, h // rep, n].double()
            assert_within_ulp(out[qv], want.to(dev)[qv], f"{what} [B: needle]")
            return
        ref, spr = ref64(self.q.to(dev), self.K.to(dev), self.V.to(dev), self.mask.to(dev), self.scale, spread=self.fam == "C")
        if self.fam == "A":
            assert_within_ulp(out[qv], ref[qv], f"{what} [A: key set]")
        else:
            assert_rounding_bound(out[qv], ref[qv], spr[qv], f"{what} [C: peaked]", self.ref_coef)


FAMS = ["A", "B", "C"]


# ---------------------------------------------------------------------------------------------------------------------------
# o3v_attn_decode: MFMA body (head_dim 128, nsplit > 0) and the scalar kernel (nsplit < 0, head_dim 32 / 64)
# ---------------------------------------------------------------------------------------------------------------------------
DECODE_CASES = [
    # B, Hq, Hkv, D, ctx, Tmax, pads, nsplit
    (1, 28, 4, 128, 4700, 4733, [0], 64),                  # 7B bench length, 37 of 64 splits hold keys
    (2, 28, 4, 128, 4490, 4500, [1024, 4489], 37),         # k_lo a 128 multiple / a single valid key
    (3, 8, 1, 128, 129, 160, [0, 64, 128], 5),
    (4, 14, 2, 128, 33, 48, [0, 1, 31, 32], 8),            # ctx << 128 * nsplit: empty splits and waves
    (2, 16, 2, 128, 31, 40, [0, 30], 2), (2, 16, 2, 128, 32, 40, [0, 31], 1), (2, 16, 2, 128, 127, 130, [0, 126], 3),
    (2, 16, 2, 128, 128, 129, [0, 127], 4),
    (2, 7, 1, 128, 1, 8, [0, 0], 3),                       # one key
    (1, 28, 4, 128, 4490, 4500, [0], -36),                 # scalar kernel, head_dim 128
    (2, 8, 2, 128, 129, 140, [0, 128], -3), (2, 8, 1, 128, 1, 4, [0, 0], -2),
    (2, 8, 2, 64, 300, 320, [0, 127], 4), (3, 4, 2, 32, 127, 130, [0, 64, 126], 2), (2, 4, 1, 32, 33, 40, [0, 32], -3),
]


def _decode_edges(ctx, nsplit, D, pad):
    rng = mfma_splits(ctx, nsplit) if (nsplit > 0 and D == 128) else scalar_splits(ctx, abs(nsplit), D)
    return edge_keys(pad, ctx, ranges=rng)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("B,Hq,Hkv,D,ctx,Tmax,pads,nsplit", DECODE_CASES)
def test_decode_probes(dev, fam, B, Hq, Hkv, D, ctx, Tmax, pads, nsplit):
    import kernel_ops as ops
    scale = D ** -0.5
    mask = torch.zeros(B, 1, ctx, dtype=torch.bool)
    for b, p in enumerate(pads):
        mask[b, 0, p:] = True
    edges = [_decode_edges(ctx, nsplit, D, p) for p in pads]
    rounds = 1 if fam != "B" else min(24, -(-max(len(e) for e in edges) // Hq))
    k_lo = torch.tensor(pads, dtype=torch.int32, device=dev)
    for rnd in range(rounds):
        pr = Probe(fam, B, 1, Hq, Hkv, ctx, D, mask, scale, seed=ctx * 7 + D + rnd, edges=edges, always=[[p] for p in pads],
                   lo=pads, sink=[[p] for p in pads], rot=rnd * Hq)
        g = torch.Generator().manual_seed(rnd)
        kc = torch.zeros(B, Hkv, Tmax, D, dtype=BF)
        vc = torch.zeros_like(kc)
        kc[:, :, :ctx], vc[:, :, :ctx] = pr.K, pr.V
        if Tmax > ctx:
            pr.decoy_rows_(kc[:, :, ctx:], vc[:, :, ctx:], g)
        out = ops.attn_decode(pr.q[:, 0].to(dev), kc.to(dev), vc.to(dev), k_lo, ctx, nsplit, scale, poison=True)
        pr.check(out[:, None], f"decode ctx={ctx} nsplit={nsplit} D={D} pads={pads} round {rnd}", dev)


# ---------------------------------------------------------------------------------------------------------------------------
# o3v_attn_decode_group (prefix in the leader row's cache) and o3v_attn_decode_group_prefix (prefix in a prompt entry)
# ---------------------------------------------------------------------------------------------------------------------------
GROUP_CASES = [
    # B, G, Hq, Hkv, P, own, pad, nsp, rows_per_prompt (prompt-entry layout)
    (6, 6, 28, 4, 4490, 33, 0, 36, 6),      # 7B bench prompt, one long case
    (4, 4, 8, 2, 128, 1, 64, 2, 4),         # k_lo a 64 multiple, one own key
    (4, 2, 16, 2, 129, 130, 0, 3, 4),       # sub-groups of 2 inside a prompt's 4 rows
    (8, 8, 28, 4, 333, 64, 5, -3, 8),       # shared-read form (per-row kernel, prefix from the group's first row)
    (3, 3, 4, 1, 32, 31, 31, 1, 3),         # k_lo = P - 1
    (4, 2, 28, 4, 97, 300, 40, -5, 2),
]


def _group_edges(P, ctx, nsp, pad):
    if nsp > 0:
        rng = mfma_splits(P, nsp) + mfma_splits(ctx, -(-(ctx - P) // 128), kbeg=P)
    else:
        rng = mfma_splits(ctx, -nsp)
    return edge_keys(pad, ctx, extra=(P - 1, P, P + 1), ranges=rng)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("layout", ["leader", "prompt"])
@pytest.mark.parametrize("B,G,Hq,Hkv,P,own,pad,nsp,rpp", GROUP_CASES)
def test_decode_group_probes(dev, fam, layout, B, G, Hq, Hkv, P, own, pad, nsp, rpp):
    import kernel_ops as ops
    D, ctx = 128, P + own
    scale = D ** -0.5
    mask = torch.zeros(B, 1, ctx, dtype=torch.bool)
    mask[:, 0, pad:] = True
    edges = [_group_edges(P, ctx, nsp, pad)] * B
    share = G if layout == "leader" else rpp               # rows that hold identical prefix keys
    rounds = 1 if fam != "B" else min(6, -(-len(edges[0]) // Hq))
    k_lo = torch.full((B,), pad, dtype=torch.int32, device=dev)
    for rnd in range(rounds):
        pr = Probe(fam, B, 1, Hq, Hkv, ctx, D, mask, scale, seed=ctx * 5 + B + rnd, edges=edges, always=[[pad]] * B, lo=[pad] * B,
                   sink=[[pad]] * B, rot=rnd * Hq + 3)
        for b in range(B):                                   # rows sharing a prompt share its K / V
            lead = (b // share) * share
            pr.K[b, :, :P], pr.V[b, :, :P] = pr.K[lead, :, :P], pr.V[lead, :, :P]
        g = torch.Generator().manual_seed(100 + rnd)
        what = f"group {layout} P={P} own={own} pad={pad} nsp={nsp} G={G} round {rnd}"
        if layout == "leader":
            Tmax = ctx + 5
            kc = torch.zeros(B, Hkv, Tmax, D, dtype=BF)
            vc = torch.zeros_like(kc)
            kc[:, :, :ctx], vc[:, :, :ctx] = pr.K, pr.V
            pr.decoy_rows_(kc[:, :, ctx:], vc[:, :, ctx:], g)
            for b in range(B):
                if b % G:
                    pr.decoy_rows_(kc[b, :, :P], vc[b, :, :P], g)     # never read: the group's first row holds the prefix
            out = ops.attn_decode_group(pr.q[:, 0].to(dev), kc.to(dev), vc.to(dev), k_lo, G, P, ctx, nsp, scale, poison=True)
        else:
            cap, T_own = P + 3, own + 4
            kpre = torch.zeros(B // rpp, Hkv, cap, D, dtype=BF)
            vpre = torch.zeros_like(kpre)
            kpre[:, :, :P], vpre[:, :, :P] = pr.K[::rpp, :, :P], pr.V[::rpp, :, :P]
            pr.decoy_rows_(kpre[:, :, P:], vpre[:, :, P:], g)
            ko = torch.zeros(B, Hkv, T_own, D, dtype=BF)
            vo = torch.zeros_like(ko)
            ko[:, :, :own], vo[:, :, :own] = pr.K[:, :, P:], pr.V[:, :, P:]
            pr.decoy_rows_(ko[:, :, own:], vo[:, :, own:], g)
            out = ops.attn_decode_group_prefix(pr.q[:, 0].to(dev), ko.to(dev), vo.to(dev), kpre.to(dev), vpre.to(dev), rpp, k_lo, G, P,
                                               ctx, nsp, scale, poison=True)
        pr.check(out[:, None], what, dev)


# ---------------------------------------------------------------------------------------------------------------------------
# o3v_attn_tiles: causal GQA prefill (cache layout, left padding, past > 0) and o3v_attn_tiles_prefix
# ---------------------------------------------------------------------------------------------------------------------------
def _causal_setup(B, S, past, pads, T):
    mask = torch.zeros(B, S, T, dtype=torch.bool)
    for b, pad in enumerate(pads):
        for i in range(S):
            mask[b, i, pad:past + i + 1] = True
    return mask


def _causal_bands(B, S, past, pads, T, mask):
    """Decoy bands above the causal diagonal, one per band top (row `top`, whose diagonal is J = past + top): the rows of a batch
    row between its previous band top and this one see DECOY on every key above J, and the rows above J see those keys
    normally.  Band m uses one dimension for all batch rows."""
    bands = []
    prev = [-1] * B
    for top in (15, 16, 31, 32, 63, 64, 127, 128):
        rows, keys = [], []
        J = past + top
        for b in range(B):
            if top >= S or J + 1 >= T or not mask[b, top].any():
                continue
            rows += [(b, i) for i in range(S) if prev[b] < past + i <= J and mask[b, i].any()]
            keys += [(b, j) for j in range(J + 1, T)]
            prev[b] = J
        if rows:
            bands.append((rows, keys))
    return bands


def _causal_edges(B, S, past, pads, T):
    out = []
    for pad in pads:
        diag = [past + i + d for i in (0, 15, 16, 31, 32, 63, 64, 127, 128, S - 1) for d in (0, 1) if i < S]
        out.append(edge_keys(pad, T, extra=diag + [past - 1, past]))
    return out


PREFILL_CASES = [
    # Hq, Hkv, D, S, past, pads
    (7, 1, 128, 150, 0, [0, 13]), (4, 2, 32, 70, 0, [5]), (16, 2, 128, 333, 0, [0]), (4, 4, 64, 129, 0, [64, 0, 127]),
    (8, 2, 128, 100, 200, [0, 70]),                        # past > 0: padding inside the computed prefix
    (28, 4, 128, 90, 4400, [0]),                           # long context: the chunk behind the 7B bench prompt
]


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("rpt", [64, 128])
@pytest.mark.parametrize("Hq,Hkv,D,S,past,pads", PREFILL_CASES)
def test_prefill_probes(dev, fam, rpt, Hq, Hkv, D, S, past, pads):
    import kernel_ops as ops
    from open_o3_video_amd import indexing
    B, T = len(pads), past + S
    Tmax, scale, QD = T + 9, D ** -0.5, Hq * D
    mask = _causal_setup(B, S, past, pads, T)
    pr = Probe(fam, B, S, Hq, Hkv, T, D, mask, scale, seed=S * 3 + D + past, edges=_causal_edges(B, S, past, pads, T),
               always=[[p] for p in pads], bands=_causal_bands(B, S, past, pads, T, mask) if fam == "B" else (), lo=pads,
               sink=[[p] for p in pads], needle_extra=lambda b, i: [past + i, past + i - 1], unrounded_sum=True)
    g = torch.Generator().manual_seed(S)
    kc = torch.zeros(B, Hkv, Tmax, D, dtype=BF)
    vc = torch.zeros_like(kc)
    kc[:, :, :T], vc[:, :, :T] = pr.K, pr.V
    pr.decoy_rows_(kc[:, :, T:], vc[:, :, T:], g)
    tiles = torch.from_numpy(indexing.prefill_tiles(B, S, pads, rpt, past=past)).to(dev)
    out = torch.empty(B * S + 16, QD, dtype=BF, device=dev)
    ops.attn_tiles(pr.q.reshape(B * S, QD).to(dev), kc.to(dev), vc.to(dev), tiles, Hq, Hq // Hkv, D, QD, D, Tmax * D, Hkv * Tmax * D,
                   D, Tmax * D, Hkv * Tmax * D, out, QD, scale, rows_per_tile=rpt, poison=True)
    assert torch.isnan(out[B * S:].float()).all(), "rows past the batch were written"
    pr.check(out[:B * S].view(B, S, Hq, D), f"prefill S={S} past={past} pads={pads} D={D} tile={rpt}", dev)


PREFIX_CASES = [
    # D, Hq, Hkv, G, P, L, pad, rows_per_prefix
    (128, 8, 2, 3, 200, 70, 0, 3), (128, 4, 4, 2, 129, 100, 5, 1), (64, 4, 2, 2, 64, 64, 63, 2), (32, 4, 2, 4, 77, 40, 0, 2),
    (128, 28, 4, 2, 4400, 90, 0, 2),                       # long prompt
]


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("rpt", [64, 128])
@pytest.mark.parametrize("D,Hq,Hkv,G,P,L,pad,rpp", PREFIX_CASES)
def test_prefill_prefix_probes(dev, fam, rpt, D, Hq, Hkv, G, P, L, pad, rpp):
    """o3v_attn_tiles_prefix: the G rows' L new tokens behind prompt entries shared by rpp rows each"""
    import kernel_ops as ops
    from open_o3_video_amd import indexing
    T, cap, T2 = P + L, P + 3, L + 5
    scale, QD = D ** -0.5, Hq * D
    pads = [pad] * G
    mask = _causal_setup(G, L, P, pads, T)
    pr = Probe(fam, G, L, Hq, Hkv, T, D, mask, scale, seed=P + L + D, edges=_causal_edges(G, L, P, pads, T), always=[[pad]] * G,
               bands=_causal_bands(G, L, P, pads, T, mask) if fam == "B" else (), lo=pads, sink=[[pad]] * G,
               needle_extra=lambda b, i: [P + i, P + i - 1], unrounded_sum=True)
    for b in range(G):
        lead = (b // rpp) * rpp
        pr.K[b, :, :P], pr.V[b, :, :P] = pr.K[lead, :, :P], pr.V[lead, :, :P]
    g = torch.Generator().manual_seed(P)
    kp = torch.zeros(G // rpp, Hkv, cap, D, dtype=BF)
    vp = torch.zeros_like(kp)
    kp[:, :, :P], vp[:, :, :P] = pr.K[::rpp, :, :P], pr.V[::rpp, :, :P]
    pr.decoy_rows_(kp[:, :, P:], vp[:, :, P:], g)
    ko = torch.zeros(G, Hkv, T2, D, dtype=BF)
    vo = torch.zeros_like(ko)
    ko[:, :, :L], vo[:, :, :L] = pr.K[:, :, P:], pr.V[:, :, P:]
    pr.decoy_rows_(ko[:, :, L:], vo[:, :, L:], g)
    tiles = torch.from_numpy(indexing.prefill_tiles(G, L, pads, rpt, past=P)).to(dev)
    out = torch.empty(G * L + 16, QD, dtype=BF, device=dev)
    ops.attn_tiles_prefix(pr.q.reshape(G * L, QD).to(dev), ko.to(dev), vo.to(dev), kp.to(dev), vp.to(dev), cap * D, Hkv * cap * D, P, rpp,
                          tiles, Hq, Hq // Hkv, D, QD, D, T2 * D, Hkv * T2 * D, D, T2 * D, Hkv * T2 * D, out, QD, scale, rows_per_tile=rpt,
                          poison=True)
    assert torch.isnan(out[G * L:].float()).all(), "rows past the batch were written"
    pr.check(out[:G * L].view(G, L, Hq, D), f"prefix P={P} L={L} pad={pad} rpp={rpp} D={D} tile={rpt}", dev)


# ---------------------------------------------------------------------------------------------------------------------------
# o3v_attn_tiles: ViT segments (non-causal, q / k / v in place in the fused qkv rows)
# ---------------------------------------------------------------------------------------------------------------------------
def _segment_tiles(cu, rpt):
    out = []
    for a, e in zip(cu[:-1], cu[1:]):
        for q0 in range(a, e, rpt):
            out.append((q0, min(rpt, e - q0), a, e - a, -1, 0, 0, 0))
    return np.asarray(out, dtype=np.int32).reshape(-1, 8)


VARLEN_CASES = [
    # H, D, lens, rows_per_tile
    (4, 80, [12, 16, 48, 64, 100, 480, 1], 64), (2, 32, [24, 64, 65, 7, 129], 128), (3, 64, [130, 64, 1], 64),
    (2, 128, [200, 33, 128], 128), (2, 128, [31, 32, 33, 127], 64),
]


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("H,D,lens,rpt", VARLEN_CASES)
def test_vit_varlen_probes(dev, fam, H, D, lens, rpt):
    import kernel_ops as ops
    P, hid, scale = sum(lens), H * D, D ** -0.5
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seg = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    mask = (seg[:, None] == seg[None, :])[None]              # [1, P, P]
    edges = set()
    for a, e in zip(cu[:-1], cu[1:]):
        edges.update(k for k in edge_keys(int(a), int(e), extra=[int(e)]) if 0 <= k < P)
        edges.update(int(a) + m + d for m in (32, 64, 128) for d in (-1, 0, 1) if int(a) <= int(a) + m + d < min(int(e), P))
    bands = [([(0, i) for i in range(int(a), int(e))], [(0, j) for j in range(P) if not (a <= j < e)])
             for a, e in zip(cu[:-1], cu[1:])] if fam == "B" else ()
    pr = Probe(fam, 1, P, H, H, P, D, mask, scale, seed=P + D, edges=[sorted(edges)], always=[[int(a) for a in cu[:-1]]],
               bands=bands, sink=[[int(a) for a in cu[:-1]]], unrounded_sum=True)
    g = torch.Generator().manual_seed(P)
    qkv = torch.zeros(P + 8, 3, H, D, dtype=BF)
    qkv[:P, 0] = pr.q[0]
    qkv[:P, 1] = pr.K[0].transpose(0, 1)
    qkv[:P, 2] = pr.V[0].transpose(0, 1)
    pr.decoy_rows_(qkv[P:, 1].transpose(0, 1), qkv[P:, 2].transpose(0, 1), g)
    nan_rows_(qkv[P:, 0].transpose(0, 1))
    qd = qkv.reshape(P + 8, 3 * hid).to(dev)
    tiles = torch.from_numpy(_segment_tiles(cu, rpt)).to(dev)
    out = torch.empty(P + 8, hid, dtype=BF, device=dev)
    ops.attn_tiles(qd, qd[:, hid:], qd[:, 2 * hid:], tiles, H, 1, D, 3 * hid, 3 * hid, D, 0, 3 * hid, D, 0, out, hid, scale,
                   rows_per_tile=rpt, poison=True)
    assert torch.isnan(out[P:].float()).all(), "rows past the segments were written"
    pr.check(out[:P].view(1, P, H, D), f"vit lens={lens} D={D} tile={rpt}", dev)
