"""vLLM sampling controls on the GPU: one decode step through o3v_sample_step_ex against the fp32 torch definition of
tests/sampling_ref.py (options off bit-identical to the plain samplers; greedy arg-max; every draw inside the reference's kept set;
log-probs, ranks and top-N; draw frequencies; the output counts), then the engine and the façades on the fixture models."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
import sampling_ref as sr
from logprobs_ref import kept_mask as kept_k_p, rank_of, top_n

pytestmark = pytest.mark.gpu

LP_ATOL = 2e-3      # as tests/test_gpu_logprobs.py


@pytest.fixture(scope="module")
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------- inputs
ROW_SEEDS = (13, 20, 63)


def _row(V, seed):
    """One row as test_sample_top_k_top_p builds it (hot set + a plateau among the largest scores, bf16) with a count table: counts
    1, 2, 3, 7, 40 on hot tokens and ~300 singletons, seen = counted tokens + 200 prompt tokens."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(V, generator=g) * 2.5
    hot = torch.randint(0, V, (30,), generator=g)
    base[hot] += 8.0
    base[hot[10:18]] = float(base[hot[10]])
    cnt = torch.zeros(V)
    cnt.index_add_(0, torch.randint(0, V, (300,), generator=g), torch.ones(300))
    cnt[hot[:5]] += torch.tensor([1., 2., 3., 7., 40.])
    seen = cnt > 0
    seen[torch.randint(0, V, (200,), generator=g)] = True
    return base.to(torch.bfloat16), cnt.to(torch.int32), seen.to(torch.uint8), hot


def _rows(B, V):
    rows = [_row(V, ROW_SEEDS[b % 3] + 1000 * (b // 3)) for b in range(B)]
    return (torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows]), torch.stack([r[2] for r in rows]),
            torch.stack([r[3] for r in rows]))


def _bias(V, hot):
    """+/- values, bans and an allowed set of a few hundred ids (the hot set of row 0 and 400 others)."""
    g = torch.Generator().manual_seed(5)
    allowed = torch.unique(torch.cat([hot[0], torch.randint(0, V, (400,), generator=g)])).tolist()
    lb = {int(hot[0, 0]): -6.0, int(hot[0, 3]): 2.5, int(hot[0, 7]): -1.25, allowed[5]: 3.0, allowed[-3]: 9.5}
    return sr.static_bias(V, lb, allowed, banned=[int(hot[0, 1]), int(hot[0, 12]), allowed[9]])


# name -> sampler settings; "bias": None | "static" | "early" (the static vector with three stop ids at -inf, used while step < min_tokens)
SETS = {
    "min_p": dict(rep=1.0, temp=1.0, top_k=0, top_p=1.0, min_p=0.05, pres=0.0, freq=0.0, bias=None),
    "all": dict(rep=1.1, temp=0.8, top_k=50, top_p=0.95, min_p=0.02, pres=0.5, freq=0.3, bias=None),
    "neg_freq": dict(rep=1.05, temp=1.3, top_k=0, top_p=0.9, min_p=0.2, pres=1.5, freq=-0.2, bias=None),
    "bias": dict(rep=1.0, temp=0.7, top_k=0, top_p=1.0, min_p=0.002, pres=2.0, freq=2.0, bias="static"),
    "early": dict(rep=1.1, temp=0.9, top_k=40, top_p=1.0, min_p=0.01, pres=0.0, freq=0.0, bias="early"),
}


def _case(B, V, name, clear_winner=False):
    """(logits bf16, counts i32, seen u8, settings, bias vector, early vector, min_tokens) on the CPU.  clear_winner (the greedy
    test): where the plateau leaves two processed scores tied for the first place, the first of them gets +0.5 on its logit."""
    m = SETS[name]
    lg, cnt, seen, hot = _rows(B, V)
    bias = early = None
    min_tokens = 0
    if m["bias"] == "static":
        bias = _bias(V, hot)
    elif m["bias"] == "early":
        stops = [int(torch.argmax(lg[0].float())), int(hot[0, 2]), int(hot[0, 20])]     # row 0's most likely token among them
        bias = sr.static_bias(V, {int(hot[0, 4]): 1.0})
        early = sr.static_bias(V, {int(hot[0, 4]): 1.0}, stop_ids=stops)
        min_tokens = 3
    if clear_winner:
        raw = sr.processed_scores(lg, seen, m["rep"], 1.0, cnt, m["pres"], m["freq"], early if early is not None else bias)
        top2 = torch.topk(raw, 2, dim=1)
        for b in torch.nonzero(top2.values[:, 0] - top2.values[:, 1] < 0.01)[:, 0].tolist():
            i = int(raw[b].argmax())
            lg[b, i] = (lg[b, i].float() + 0.5).to(torch.bfloat16)
    return lg, cnt, seen, m, bias, early, min_tokens


class _Step:
    """One decode step (column `step` of a 3-column output) through o3v_sample_step_ex or one of the plain entries."""

    def __init__(self, lg, seen, counts=None, bias=None, early=None):
        from open_o3_video_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.lg, self.B, self.V = lg.cuda(), lg.shape[0], lg.shape[1]
        self.seen0 = seen.cuda()
        self.counts0 = None if counts is None else counts.to(torch.int16).cuda()
        self.bias = None if bias is None else bias.cuda()
        self.early = None if early is None else early.cuda()
        self.rid = torch.arange(self.B, dtype=torch.int32, device="cuda") * 3 + 1
        self.scratch = torch.zeros((self.B, _lib.SAMPLE_SCRATCH_FLOATS), dtype=torch.float32, device="cuda")

    def run(self, do_sample, m, n=None, seed=11, step=1, entry="ex", min_tokens=0, fin=None, eos=None, keep_state=None, T=3):
        """entry: "ex" | "plain" (o3v_sample_greedy / o3v_sample_top_k_top_p) | "lp" (o3v_sample_logprobs).  keep_state: (seen,
        counts) tensors to go on from instead of fresh copies."""
        _lib, lib, B, V = self._lib, self.lib, self.B, self.V
        sn, cn = keep_state if keep_state is not None else (self.seen0.clone(), None if self.counts0 is None else self.counts0.clone())
        cur = torch.zeros(B, dtype=torch.int32, device="cuda")
        fin = torch.zeros(B, dtype=torch.int32, device="cuda") if fin is None else fin
        out_ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
        marg = torch.zeros((B, T), dtype=torch.float32, device="cuda")
        eos_t = torch.tensor(eos or [0x7fffffff], dtype=torch.int32, device="cuda")
        args = (_p(self.lg), _p(sn), _p(cur), _p(fin), _p(out_ids), _p(marg), _p(eos_t), eos_t.numel(), -1, B, V, V)
        temp, top_k, top_p = (m["temp"], m["top_k"], m["top_p"]) if do_sample else (1.0, 0, 1.0)
        lp = opts = None
        if n is not None:
            lp = (torch.zeros((B, T), dtype=torch.float32, device="cuda"), torch.zeros((B, T), dtype=torch.int32, device="cuda"),
                  torch.full((B, T, max(n, 1)), -9, dtype=torch.int32, device="cuda"),
                  torch.zeros((B, T, max(n, 1)), dtype=torch.float32, device="cuda"))
            opts = _lib.LogprobOpts(n=n, chosen_lp=lp[0].data_ptr(), chosen_rank=lp[1].data_ptr(), top_ids=lp[2].data_ptr(),
                                    top_lp=lp[3].data_ptr())
        if entry == "plain":
            assert n is None
            if do_sample:
                _lib.check(lib.o3v_sample_top_k_top_p(*args, m["rep"], temp, top_k, top_p, seed, _p(self.rid), step, T, _p(self.scratch),
                                                      _stream()), "o3v_sample_top_k_top_p")
            else:
                _lib.check(lib.o3v_sample_greedy(*args, m["rep"], step, T, _p(self.scratch), _stream()), "o3v_sample_greedy")
        elif entry == "lp":
            _lib.check(lib.o3v_sample_logprobs(*args, int(do_sample), m["rep"], temp, top_k, top_p, seed, _p(self.rid), step, T,
                                               _p(self.scratch), C.byref(opts), _stream()), "o3v_sample_logprobs")
        else:
            so = _lib.SamplingOpts(min_p=m.get("min_p", 0.0) if do_sample else 0.0, presence=m.get("pres", 0.0), frequency=m.get("freq", 0.0),
                                   min_tokens=min_tokens, bias=0 if self.bias is None else self.bias.data_ptr(),
                                   bias_early=0 if self.early is None else self.early.data_ptr(),
                                   out_counts=0 if cn is None else cn.data_ptr())
            _lib.check(lib.o3v_sample_step_ex(*args, int(do_sample), m["rep"], temp, top_k, top_p, seed, _p(self.rid), step, T,
                                              _p(self.scratch), None if opts is None else C.byref(opts), C.byref(so), _stream()),
                       "o3v_sample_step_ex")
        torch.cuda.synchronize()
        res = dict(ids=out_ids[:, step].cpu(), marg=marg[:, step].cpu(), seen=sn, counts=cn, fin=fin, cur=cur.cpu())
        if lp is not None:
            res["lp"] = (lp[0][:, step].cpu(), lp[1][:, step].cpu(), lp[2][:, step, :n].cpu(), lp[3][:, step, :n].cpu())
        return res


def _reference(lg, cnt, seen, m, bias, do_sample):
    """(scores with -inf where masked, log-probs, unmasked processed scores) of tests/sampling_ref.py for one case."""
    kw = dict(counts=cnt, presence=m["pres"], frequency=m["freq"], bias=bias)
    s, lp = sr.logprobs(lg, seen, m["rep"], m["temp"], m["top_k"], m["top_p"], do_sample, min_p=m["min_p"], **kw)
    temp = m["temp"] if do_sample else 1.0
    return s, lp, sr.processed_scores(lg, seen, m["rep"], temp, **kw)


def _kept_with_ties(raw, m):
    """The reference's kept set with a tie group at the top-k / top-p boundary kept whole (as test_sample_top_k_top_p treats it),
    then min_p; asserts the condition under which the comparison leaves nothing out: no token's e_i within a relative 1e-3 of min_p
    (device expf and the CPU differ by ulps, 1e-7 relative)."""
    kp = kept_k_p(raw, m["top_k"], m["top_p"]) & torch.isfinite(raw)
    smallest = torch.where(kp, raw, torch.full_like(raw, float("inf"))).min(dim=1, keepdim=True).values
    kp = raw >= smallest
    e = sr.rel_e(raw, kp)
    if m["min_p"] > 0:
        mp = float(np.float32(m["min_p"]))
        assert float((e[kp] / mp - 1).abs().min()) > 1e-3, "a token sits at the min_p threshold"
        kp = kp & (e >= mp)
    return kp


# ---------------------------------------------------------------------------------------------------------- 5. options off
@pytest.mark.parametrize("V", [152064, 1001])
@pytest.mark.parametrize("B", [1, 8, 32])
@pytest.mark.parametrize("do_sample", [0, 1])
def test_options_off_is_the_plain_sampler(need_gpu, V, B, do_sample):
    lg, cnt, seen, _ = _rows(B, V)
    m = dict(rep=1.05, temp=0.7, top_k=50, top_p=0.95)
    st = _Step(lg, seen)
    a = st.run(do_sample, m, entry="plain")
    b = st.run(do_sample, m, entry="ex")
    for k in ("ids", "marg", "cur"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["seen"], b["seen"]) and torch.equal(a["fin"], b["fin"])
    a = st.run(do_sample, m, n=5, entry="lp")
    b = st.run(do_sample, m, n=5, entry="ex")
    assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["marg"], b["marg"]) and torch.equal(a["seen"], b["seen"])
    for x, y in zip(a["lp"], b["lp"]):
        assert torch.equal(x, y)            # chosen log-prob, rank, top ids and top log-probs, bit for bit


# ---------------------------------------------------------------------------------------------------------- 6. greedy
@pytest.mark.parametrize("V", [152064, 1001])
@pytest.mark.parametrize("B", [1, 8, 32])
@pytest.mark.parametrize("name", list(SETS))
def test_greedy_is_the_reference_argmax(need_gpu, V, B, name):
    lg, cnt, seen, m, bias, early, min_tokens = _case(B, V, name, clear_winner=True)
    step = 1
    act = early if step < min_tokens else bias
    s, lp_ref, raw = _reference(lg, cnt, seen, m, act, False)
    top2 = torch.topk(raw, 2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-4, "reference top-1 / top-2 gap (kernel and torch may differ by one fp32 ulp)"
    st = _Step(lg, seen, cnt, bias, early)
    r = st.run(0, m, n=20, step=step, min_tokens=min_tokens)
    print(name, V, B, "min gap", float((top2[:, 0] - top2[:, 1]).min()))
    assert torch.equal(r["ids"].long(), raw.argmax(dim=1))
    assert (r["marg"] - (top2[:, 0] - top2[:, 1])).abs().max().item() < 1e-4
    tok_lp, rank, top_ids, top_lp = r["lp"]
    assert (rank == 1).all() and torch.equal(top_ids[:, 0], r["ids"])
    ref_ids, ref_top = top_n(s, lp_ref, 20)
    assert np.array_equal(top_ids.numpy(), ref_ids)
    assert np.abs(top_lp.numpy() - ref_top).max() < LP_ATOL
    assert (tok_lp - lp_ref.gather(1, r["ids"].long()[:, None])[:, 0]).abs().max().item() < LP_ATOL
    # bookkeeping of the last stage: the emitted token is counted once and marked seen
    want = cnt.clone()
    want[torch.arange(B), r["ids"].long()] += 1
    assert torch.equal(r["counts"].cpu().to(torch.int32), want)
    assert bool(r["seen"].cpu()[torch.arange(B), r["ids"].long()].all())


# ---------------------------------------------------------------------------------------------------------- 7. sampled
@pytest.mark.parametrize("V", [152064, 1001])
@pytest.mark.parametrize("B", [1, 8, 32])
@pytest.mark.parametrize("name", list(SETS))
def test_draws_lie_in_the_reference_kept_set_with_logprobs(need_gpu, V, B, name):
    lg, cnt, seen, m, bias, early, min_tokens = _case(B, V, name)
    step = 1
    act = early if step < min_tokens else bias
    s, lp_ref, raw = _reference(lg, cnt, seen, m, act, True)
    kept = _kept_with_ties(raw, m)
    print(name, V, B, "kept per row", kept.sum(1).tolist()[:8], "reference (ties split)", torch.isfinite(s).sum(1).tolist()[:8])
    st = _Step(lg, seen, cnt, bias, early)
    exact = torch.equal(kept, torch.isfinite(s))        # no tie group at a boundary: the reference set is THE set
    for seed in (11, 12, 13):
        r = st.run(1, m, n=20, seed=seed, step=step, min_tokens=min_tokens)
        ids = r["ids"].long()
        assert kept[torch.arange(B), ids].all(), "drawn outside the reference's kept set"
        tok_lp, rank, top_ids, top_lp = r["lp"]
        # the kernel keeps a boundary tie group whole: its distribution is the softmax over `kept`
        s_k = torch.where(kept, raw, torch.full_like(raw, -float("inf")))
        lp_k = torch.log_softmax(s_k, dim=-1)
        ref_ids, ref_top = top_n(s_k, lp_k, 20)
        assert np.array_equal(top_ids.numpy(), ref_ids), (name, seed)
        fin = np.isfinite(ref_top)
        assert np.array_equal(np.isfinite(top_lp.numpy()), fin)              # masked tokens at -inf
        assert np.abs(top_lp.numpy()[fin] - ref_top[fin]).max() < LP_ATOL
        assert np.array_equal(rank.numpy(), rank_of(s_k, ids))
        assert (tok_lp - lp_k.gather(1, ids[:, None])[:, 0]).abs().max().item() < LP_ATOL
        if exact:
            assert (tok_lp - lp_ref.gather(1, ids[:, None])[:, 0]).abs().max().item() < LP_ATOL
        want = cnt.clone()
        want[torch.arange(B), ids] += 1
        assert torch.equal(r["counts"].cpu().to(torch.int32), want)
    assert abs(float(torch.exp(lp_k.double()).sum(1).max()) - 1) < 1e-4 and abs(float(torch.exp(lp_k.double()).sum(1).min()) - 1) < 1e-4


def test_kept_logprobs_sum_to_one(need_gpu):
    """Every kept token's log-prob as the kernel reports it (V = 1001 rows whose kept set fits in 20 entries): the sum is 1."""
    V, B = 1001, 8
    lg, cnt, seen, m, bias, early, _ = _case(B, V, "all")
    m = dict(m, top_k=12)
    r = _Step(lg, seen, cnt).run(1, m, n=20)
    top_lp = r["lp"][3].double()
    n_kept = torch.isfinite(top_lp).sum(1)
    assert (n_kept >= 1).all() and (n_kept < 20).all()          # at most 12 + the 7 other plateau tokens: the whole kept set is listed
    assert (torch.exp(top_lp).sum(1) - 1).abs().max().item() < 1e-4


# ---------------------------------------------------------------------------------------------------------- 8. frequencies
# a flatter distribution than SETS give on this row (dozens of kept tokens), so that the frequencies have something to show
WIDE = dict(rep=1.05, temp=3.0, top_k=0, top_p=1.0, min_p=0.05, pres=0.5, freq=0.1, bias=None)


@pytest.mark.parametrize("name", ["min_p", "all", "neg_freq", "bias", "wide"])
def test_draw_frequencies(need_gpu, name):
    """V = 997, the same row in all B = 32 rows, 64 steps with seen and counts held fixed: n = 2048 draws.  max |freq - p| stays
    below 2.5 / sqrt(n): each freq_i is a binomial mean with sigma <= 0.5 / sqrt(n), so this is the 5 sigma bound."""
    V, B, N = 997, 32, 64
    lg1, cnt1, seen1, hot = _row(V, 13)
    lg, cnt, seen = lg1[None].repeat(B, 1), cnt1[None].repeat(B, 1), seen1[None].repeat(B, 1)
    m = WIDE if name == "wide" else SETS[name]
    bias = _bias(V, hot[None]) if m["bias"] == "static" else None
    _, _, raw = _reference(lg[:1], cnt[:1], seen[:1], m, bias, True)
    kept = _kept_with_ties(raw, m)
    p = torch.softmax(torch.where(kept, raw, torch.full_like(raw, -float("inf"))).double(), dim=-1)[0]
    st = _Step(lg, seen, cnt, bias)
    draws = []
    for step in range(N):
        draws.append(st.run(1, m, seed=99, step=step, T=N)["ids"].long())
    o = torch.cat(draws)
    n = o.numel()
    assert n >= 1600 and kept[0][o].all()
    freq = torch.bincount(o, minlength=V).double() / n
    err = float((freq - p).abs().max())
    print(name, "kept", int(kept.sum()), "max |freq - p|", err, "bound", 2.5 / math.sqrt(n))
    assert err < 2.5 / math.sqrt(n)


# ---------------------------------------------------------------------------------------------------------- 9. counts
@pytest.mark.parametrize("do_sample", [0, 1])
def test_counts_equal_the_bincount_of_the_emitted_ids(need_gpu, do_sample):
    V, B, N = 1001, 8, 64
    lg, _, seen, hot = _rows(B, V)
    m = dict(rep=1.1, temp=1.2, top_k=0, top_p=1.0, min_p=0.0, pres=0.3, freq=0.4)
    # rows 0..3 will finish: the EOS id is among their likeliest tokens (greedy: the penalties walk down the hot set and reach it);
    # rows 4..7 never emit it
    eos = [7]
    lg[:4, 7] = 13.0
    lg[4:, 7] = -30.0
    st = _Step(lg, seen, torch.zeros((B, V), dtype=torch.int32))
    fin = torch.zeros(B, dtype=torch.int32, device="cuda")
    state = (st.seen0.clone(), st.counts0.clone())
    out = []
    for step in range(N):
        r = st.run(do_sample, m, seed=5, step=step, T=N, fin=fin, eos=eos, keep_state=state)
        out.append(r["ids"].long())
    ids = torch.stack(out, 1)                       # [B, N]
    counts = state[1].cpu().to(torch.int32)
    finished = fin.cpu().bool()
    assert finished.any() and not finished.all(), "the case needs rows that finish and rows that do not"
    for b in range(B):
        row = ids[b]
        hit = torch.nonzero(torch.isin(row, torch.tensor(eos)))
        end = int(hit[0]) + 1 if hit.numel() else N         # the EOS token itself is emitted by an unfinished row: counted
        assert bool(finished[b]) == (hit.numel() > 0)
        assert (row[end:] == -1).all()                      # pad afterwards, not counted
        assert torch.equal(counts[b], torch.bincount(row[:end], minlength=V).to(torch.int32)), b
    if not do_sample:
        assert int(counts.max()) >= 2                       # tokens did repeat: the penalties saw counts above one


# ---------------------------------------------------------------------------------------------------------- engine fixtures
def _medium(seed=6):
    from test_gpu_model import build_engine
    cfg = fm.medium_config()
    eng = build_engine(cfg, fm.make_weights(cfg, seed))
    frames = fm.make_frames(2, 56, 84, seed=9)
    _, grid = eng.pixels_from_frames(frames)
    ids = fm.make_prompt(cfg, [tuple(r) for r in grid.tolist()], seed=9)
    return cfg, eng, frames, ids


DEFAULTS = dict(min_p=0.0, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0, token_bias=None, allowed_token_ids=None,
                banned_token_ids=None, stop_checker=None)


# ---------------------------------------------------------------------------------------------------------- 10. defaults
def test_defaults_change_nothing(need_gpu, golden_dir):
    from test_gpu_model import build_engine
    g = np.load(os.path.join(golden_dir, "g6_tiny.npz"))
    cfg = fm.tiny_config()
    eng = build_engine(cfg, fm.make_weights(cfg, 0))
    kw = dict(frames=torch.from_numpy(g["frames"]), max_new_tokens=16, pad_token_id=cfg["pad_token_id"])
    a = eng.generate(g["input_ids"], None, **kw)
    assert np.array_equal(a.sequences.cpu().numpy(), g["bf16_ids"][:, :a.sequences.shape[1]])       # the HF golden, as before
    b = eng.generate(g["input_ids"], None, **kw, **DEFAULTS)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.margins, b.margins)
    assert a.timings["launches_per_layer"] == b.timings["launches_per_layer"]
    kw = dict(kw, do_sample=True, temperature=0.8, top_k=50, top_p=0.95, seed=3, num_return_sequences=4, repetition_penalty=1.05)
    a = eng.generate(g["input_ids"], None, **kw)
    b = eng.generate(g["input_ids"], None, **kw, **DEFAULTS)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.margins, b.margins)
    assert a.timings["launches_per_layer"] == b.timings["launches_per_layer"]


# ---------------------------------------------------------------------------------------------------------- 11. teacher-forced replay
def _replay_rows(eng, ids, gen_row, frames):
    """bf16 logits [T, V] that predicted each emitted token: forward_logits over prompt + emitted tokens."""
    S = len(ids)
    full = eng.forward_logits(np.asarray([list(ids) + gen_row.tolist()]), None, frames=frames)[0]
    return full[S - 1:S - 1 + len(gen_row)].cpu()


def _state_before(ids, gen_row, j, V):
    seen = torch.zeros(V, dtype=torch.uint8)
    seen[torch.as_tensor(list(ids))] = 1
    seen[gen_row[:j]] = 1
    cnt = torch.bincount(gen_row[:j], minlength=V).to(torch.int32)
    return seen[None], cnt[None]


def test_engine_greedy_replay_with_penalties_bias_and_logprobs(need_gpu):
    from test_gpu_model import LOGIT_ATOL
    cfg, eng, frames, ids = _medium()
    V, pad, S, T = cfg["text_config"]["vocab_size"], cfg["pad_token_id"], len(ids), 24
    plain = eng.generate([ids], None, frames=frames, max_new_tokens=T, pad_token_id=pad).sequences[0, S:].cpu()
    tb = {int(plain[0]): -3.0, int(plain[1]): 2.0, 17: 4.0, 23: -1.5}
    m = dict(rep=1.1, pres=0.6, freq=0.4)
    out = eng.generate([ids], None, frames=frames, max_new_tokens=T, pad_token_id=pad, repetition_penalty=m["rep"],
                       presence_penalty=m["pres"], frequency_penalty=m["freq"], token_bias=tb, logprobs=5)
    gen = out.sequences[0, S:].cpu()
    assert not torch.equal(gen, plain)
    rows = _replay_rows(eng, ids, gen, frames)
    bias = sr.static_bias(V, tb)
    checked = 0
    for j in range(T):
        seen, cnt = _state_before(ids, gen, j, V)
        s, lp = sr.logprobs(rows[j][None], seen, m["rep"], counts=cnt, presence=m["pres"], frequency=m["freq"], bias=bias)
        top2 = torch.topk(s[0], 2).values
        if float(top2[0] - top2[1]) > LOGIT_ATOL:
            assert int(gen[j]) == int(s[0].argmax()), j
            checked += 1
        assert abs(float(out.logprobs.token[0, j]) - float(lp[0, gen[j]])) < LOGIT_ATOL, j
    print("greedy replay: steps with a reference gap above LOGIT_ATOL:", checked, "of", T, "; max count", int(torch.bincount(gen).max()))
    assert checked >= T // 2


def test_engine_sampled_group_replay(need_gpu):
    from test_gpu_model import LOGIT_ATOL
    cfg, eng, frames, ids = _medium()
    V, pad, S, T, G = cfg["text_config"]["vocab_size"], cfg["pad_token_id"], len(ids), 12, 4
    m = dict(rep=1.05, temp=0.8, top_k=50, top_p=0.95, min_p=0.05, pres=0.3, freq=0.2)
    kw = dict(frames=frames, max_new_tokens=T, pad_token_id=pad, do_sample=True, temperature=m["temp"], top_k=m["top_k"], top_p=m["top_p"],
              seed=4, num_return_sequences=G, repetition_penalty=m["rep"])
    off = eng.generate([ids], None, **kw)
    on = eng.generate([ids], None, min_p=m["min_p"], presence_penalty=m["pres"], frequency_penalty=m["freq"], logprobs=5, **kw)
    assert on.timings["launches_per_layer"] == off.timings["launches_per_layer"]
    assert torch.isfinite(on.logprobs.token).all() and (on.logprobs.rank >= 1).all()
    worst = 0.0
    for g in range(G):
        gen = on.sequences[g, S:].cpu()
        rows = _replay_rows(eng, ids, gen, frames)
        for j in range(T):
            seen, cnt = _state_before(ids, gen, j, V)
            raw = sr.processed_scores(rows[j][None], seen, m["rep"], m["temp"], cnt, m["pres"], m["freq"])
            keep = sr.kept_mask(raw, m["top_k"], m["top_p"], m["min_p"])
            short = float(raw[0][keep[0]].min() - raw[0, gen[j]])
            worst = max(worst, short)
            assert short <= 2 * LOGIT_ATOL / m["temp"], (g, j, short)
    print("sampled replay: largest shortfall below the reference's smallest kept score", worst)


# ---------------------------------------------------------------------------------------------------------- 12. min_tokens, masks
def test_engine_min_tokens_allowed_and_banned(need_gpu):
    cfg, eng, frames, ids = _medium()
    pad, S = cfg["pad_token_id"], len(ids)
    base = dict(frames=frames, max_new_tokens=10, pad_token_id=pad)
    first = int(eng.generate([ids], None, **base).sequences[0, S])
    a = eng.generate([ids], None, eos_token_ids=[first], **base)
    assert a.sequences.shape[1] == S + 1                                        # the plain run stops after one token
    b = eng.generate([ids], None, eos_token_ids=[first], min_new_tokens=4, **base)
    gen = b.sequences[0, S:].tolist()
    assert len(gen) >= 4 and first not in gen[:4]
    allowed = list(range(40, 140))
    banned = [first, 41, 42]
    c = eng.generate([ids], None, allowed_token_ids=allowed + [first], banned_token_ids=banned, **base)
    gen = c.sequences[0, S:].tolist()
    assert all(t in allowed and t not in banned for t in gen)
    with pytest.raises(ValueError):
        eng.generate([ids], None, allowed_token_ids=[41, 42], banned_token_ids=banned, **base)
    with pytest.raises(ValueError):
        eng.generate([ids], None, allowed_token_ids=[first], eos_token_ids=[first], min_new_tokens=2, **base)
    # n = 4 samples of the prompt (shared prompt K/V) under the same masks and a held-back EOS
    d = eng.generate([ids], None, allowed_token_ids=allowed + [first], banned_token_ids=[41, 42], eos_token_ids=[first], min_new_tokens=3,
                     do_sample=True, temperature=1.5, seed=2, num_return_sequences=4, token_bias={first: 30.0}, **base)
    for row in d.sequences[:, S:].tolist():
        assert first not in row[:3] and row[3] == first                        # +30 on the EOS id: emitted as soon as it may be
        assert all(t in allowed for t in row[:3])
    # left-padded batch of 3 text prompts
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(10, 400, (L,), generator=g).tolist() for L in (9, 14, 5)]
    L = max(len(p) for p in prompts)
    rows = [[pad] * (L - len(p)) + p for p in prompts]
    mask = [[0] * (L - len(p)) + [1] * len(p) for p in prompts]
    plain = eng.generate(rows, mask, max_new_tokens=8, pad_token_id=pad)
    firsts = plain.sequences[:, L].tolist()
    e = eng.generate(rows, mask, max_new_tokens=8, pad_token_id=pad, eos_token_ids=firsts, min_new_tokens=4, banned_token_ids=[55],
                     presence_penalty=0.4)
    for row in e.sequences[:, L:].tolist():
        assert len(row) >= 4 and not set(row[:4]) & set(firsts) and 55 not in row


def test_engine_stop_checker_ends_rows_at_the_named_column(need_gpu):
    cfg, eng, frames, ids = _medium()
    pad, S, T = cfg["pad_token_id"], len(ids), 12
    kw = dict(frames=frames, max_new_tokens=T, pad_token_id=pad, do_sample=True, temperature=1.0, seed=7, num_return_sequences=4,
              steps_per_sync=4)
    plain = eng.generate([ids], None, **kw).sequences[:, S:]
    calls = []

    def checker(out_ids):
        calls.append(tuple(out_ids.shape))
        return {0: 2, 2: 5} if out_ids.shape[1] >= 8 else ({0: 2} if out_ids.shape[1] >= 4 else {})
    got = eng.generate([ids], None, stop_checker=checker, **kw)
    gen = got.sequences[:, S:]
    assert calls[0] == (4, 4) and calls[1] == (4, 8)
    assert torch.equal(gen[0, :2], plain[0, :2]) and (gen[0, 2:] == pad).all()
    assert torch.equal(gen[2, :5], plain[2, :5]) and (gen[2, 5:] == pad).all()
    assert torch.equal(gen[1], plain[1, :gen.shape[1]]) and torch.equal(gen[3], plain[3, :gen.shape[1]])   # the other rows go on untouched
    # every row ended by the checker: the call stops early and trims to the longest row
    short = eng.generate([ids], None, stop_checker=lambda o: {b: 3 for b in range(4)}, **kw)
    assert short.sequences.shape[1] == S + 3 and short.n_steps == 3


def test_engine_controls_qwen3vl_and_fp8_rows(need_gpu, golden_dir):
    import fixture_models_q3 as fq
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    gd = np.load(os.path.join(golden_dir, "g12_q3_tiny.npz"))
    cfg = fq.tiny_q3_config()
    c = O3VConfig.from_dict(cfg)
    eng = O3VEngine(c, DeviceWeights(c, getter_from_dict(fq.make_weights(cfg, 0)), "cuda"))
    ids = gd["input_ids"]
    S = ids.shape[1]
    kw = dict(pixel_values=torch.from_numpy(gd["pixel_values"]), image_grid_thw=gd["grid"], max_new_tokens=8,
              pad_token_id=cfg["pad_token_id"])
    plain = eng.generate(ids, None, **kw)
    same = eng.generate(ids, None, **kw, **DEFAULTS)
    assert torch.equal(plain.sequences, same.sequences)
    first = int(plain.sequences[0, S])
    allowed = list(range(30, 90))
    out = eng.generate(ids, None, allowed_token_ids=allowed, banned_token_ids=[31], frequency_penalty=0.5, do_sample=True, top_p=0.9,
                       min_p=0.05, num_return_sequences=4, seed=5, logprobs=3, **kw)
    gen = out.sequences[:, S:]
    assert ((gen >= 30) & (gen < 90) & (gen != 31)).all() and torch.isfinite(out.logprobs.token).all()
    held = eng.generate(ids, None, eos_token_ids=[first], min_new_tokens=3, **kw).sequences[0, S:].tolist()
    assert len(held) >= 3 and first not in held[:3]
    # fp8 decode rows (8 rows of one prompt): masks and penalties reach the same sampler stage
    mcfg = fm.medium_config()
    mc = O3VConfig.from_dict(mcfg)
    e8 = O3VEngine(mc, DeviceWeights(mc, getter_from_dict(fm.make_weights(mcfg, 6)), "cuda", fp8_decode=True))
    prompt = torch.randint(10, 400, (14,), generator=torch.Generator().manual_seed(1)).tolist()
    kw = dict(max_new_tokens=6, pad_token_id=mcfg["pad_token_id"], num_return_sequences=8, do_sample=True, top_p=0.95, seed=2)
    a = e8.generate([prompt], None, **kw)
    b = e8.generate([prompt], None, **kw, **DEFAULTS)
    assert torch.equal(a.sequences, b.sequences)
    d = e8.generate([prompt], None, allowed_token_ids=list(range(100, 164)), presence_penalty=1.0, min_p=0.1, logprobs=2, **kw)
    gen = d.sequences[:, 14:]
    assert ((gen >= 100) & (gen < 164)).all() and torch.isfinite(d.logprobs.token).all()


# ---------------------------------------------------------------------------------------------------------- 13. façades
def test_vllm_facade_stop_string_and_mixed_sampling_params(need_gpu):
    from test_gpu_facades import StubTokenizer
    from test_gpu_model import build_engine
    from open_o3_video_amd.vllm_api import LLM, SamplingParams
    cfg = fm.medium_config()
    eng = build_engine(cfg, fm.make_weights(cfg, 6))
    llm = LLM(engine=eng, tokenizer=StubTokenizer(cfg), max_model_len=4096)
    g = torch.Generator().manual_seed(7)
    prompts = [" ".join(f"w{t}" for t in torch.randint(10, 400, (L,), generator=g).tolist()) for L in (7, 12)]
    greedy = SamplingParams(temperature=0.0, max_tokens=12, repetition_penalty=1.05, ignore_eos=True)
    full = llm.generate({"prompt": prompts[0]}, greedy)[0].outputs[0]
    assert full.finish_reason == "length" and full.stop_reason is None and len(full.token_ids) == 12
    # a stop string made of the 4th and 5th token's text: found although it spans two tokens
    stop = f"w{full.token_ids[3]} w{full.token_ids[4]}"
    assert stop not in " ".join(f"w{t}" for t in full.token_ids[:4])
    sp = SamplingParams(temperature=0.0, max_tokens=12, repetition_penalty=1.05, ignore_eos=True, stop=["never", stop])
    co = llm.generate({"prompt": prompts[0]}, sp)[0].outputs[0]
    assert (co.finish_reason, co.stop_reason) == ("stop", stop) and co.token_ids == full.token_ids[:5]
    assert co.text == " ".join(f"w{t}" for t in full.token_ids[:3]) + " " and len(co.token_ids) < 12
    sp.include_stop_str_in_output = True
    co = llm.generate({"prompt": prompts[0]}, sp)[0].outputs[0]
    assert co.text == " ".join(f"w{t}" for t in full.token_ids[:5])
    # a list mixing a greedy and a sampled SamplingParams equals the two separate calls, token for token
    sampled = SamplingParams(temperature=0.8, top_k=40, top_p=0.95, min_p=0.05, presence_penalty=0.4, frequency_penalty=0.2,
                             max_tokens=10, seed=3, n=2)
    llm._req = 0
    mixed = llm.generate([{"prompt": prompts[0]}, {"prompt": prompts[1]}], [greedy, sampled])
    llm._req = 0
    one = llm.generate({"prompt": prompts[0]}, greedy) + llm.generate({"prompt": prompts[1]}, sampled)
    assert [ro.request_id for ro in mixed] == ["0", "1"] == [ro.request_id for ro in one]
    assert [[o.token_ids for o in ro.outputs] for ro in mixed] == [[o.token_ids for o in ro.outputs] for ro in one]
    assert len(mixed[1].outputs) == 2 and mixed[0].outputs[0].token_ids == full.token_ids
    banned = llm.generate({"prompt": prompts[0]}, SamplingParams(temperature=0.0, max_tokens=12, repetition_penalty=1.05, ignore_eos=True,
                                                                bad_words=[f"w{full.token_ids[0]}"]))[0].outputs[0]
    assert full.token_ids[0] not in banned.token_ids


def test_hf_facade_controls_equal_the_engine_call(need_gpu, golden_dir):
    from open_o3_video_amd.hf_api import GenerationConfigLike, Qwen2_5_VLForConditionalGeneration
    g = np.load(os.path.join(golden_dir, "g7_medium.npz"))
    cfg = fm.medium_config()
    model = Qwen2_5_VLForConditionalGeneration.from_state_dict(cfg, fm.make_weights(cfg, 2))
    ids = torch.from_numpy(g["input_ids"])
    S = ids.shape[1]
    inputs = dict(input_ids=ids, pixel_values=torch.from_numpy(g["pixel_values"]), image_grid_thw=torch.from_numpy(g["grid"]))
    first = int(g["bf16_ids"][0, S])
    gc = GenerationConfigLike(max_new_tokens=8, do_sample=True, temperature=0.9, top_k=30, top_p=0.9, num_return_sequences=2,
                              pad_token_id=cfg["pad_token_id"], eos_token_id=first, min_new_tokens=3)
    model.manual_seed(5)
    out = model.generate(**inputs, generation_config=gc, min_p=0.1, suppress_tokens=[40, 41], bad_words_ids=[[42]])
    eng = model.engine.generate(g["input_ids"], None, pixel_values=inputs["pixel_values"], image_grid_thw=g["grid"], max_new_tokens=8,
                                eos_token_ids=[first], pad_token_id=cfg["pad_token_id"], do_sample=True, temperature=0.9, top_k=30,
                                top_p=0.9, seed=5, num_return_sequences=2, row_ids=[0, 1], return_margins=False, min_p=0.1,
                                min_new_tokens=3, banned_token_ids=[40, 41, 42])
    assert torch.equal(out, eng.sequences)
    gen = out[:, S:]
    assert (gen[:, :3] != first).all() and not torch.isin(gen, torch.tensor([40, 41, 42], device=gen.device)).any()
    with pytest.raises(NotImplementedError):
        model.generate(**inputs, generation_config=gc, bad_words_ids=[[42, 43]])
