"""Guided decoding on the GPU: one decode step through o3v_sample_step_guided against the fp32 torch definition of
tests/sampling_ref.py with the guide's -inf added to the bias (greedy arg-max, every draw inside allowed AND kept, log-probs, ranks,
top-N, the written state, finished rows), identity with o3v_sample_step_ex, three chained steps over the double buffer, the argument
checks, then the engine on the fixture models in every decode regime and the vLLM façade on a byte vocabulary."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fixture_models as fm
import sampling_ref as sr
from logprobs_ref import kept_mask as kept_k_p, rank_of, top_n

pytestmark = pytest.mark.gpu

LP_ATOL = 2e-3      # as tests/test_gpu_logprobs.py
N_STATES = 5
ALL = dict(rep=1.1, temp=0.8, top_k=50, top_p=0.95, min_p=0.02, pres=0.5, freq=0.3)      # test_gpu_sampling_params' "all"
SHAPES = [(4096, 4096), (1003, 1008)]       # (V, ldn): 16-byte loads; the scalar tail


@pytest.fixture(scope="module")
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------- inputs
def _row(V, seed):
    """One row in the style of test_gpu_sampling_params: a hot set and a plateau among the largest scores (bf16), a count table
    (1, 2, 3, 7, 40 on hot tokens, ~300 singletons), seen = counted tokens + 200 prompt tokens."""
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
    return base.to(torch.bfloat16), cnt.to(torch.int32), seen.to(torch.uint8)


def _table(V, ldn, n_states=N_STATES, frac=0.3, seed=3):
    """i16 [n_states, ldn]: ~30 % of the tokens allowed per state, each with a random next state; -1 elsewhere and in the padding."""
    g = torch.Generator().manual_seed(seed)
    nxt = torch.randint(0, n_states, (n_states, ldn), generator=g)
    allowed = torch.rand((n_states, ldn), generator=g) < frac
    allowed[:, V:] = False
    return torch.where(allowed, nxt, torch.full_like(nxt, -1)).to(torch.int16)


_CASES = {}


def _case(B, V, ldn):
    """(logits, counts, seen, table, start states, guide bias [B, V]) on the CPU, built once per shape and never modified."""
    key = (B, V)
    if key not in _CASES:
        rows = [_row(V, (13, 20, 63)[b % 3] + 1000 * (b // 3)) for b in range(B)]
        lg, cnt, seen = (torch.stack([r[i] for r in rows]) for i in range(3))
        table = _table(V, ldn)
        q = (torch.arange(B) * 2 + 1) % N_STATES         # rows start in different states
        gbias = torch.where(table[q.long(), :V] < 0, torch.tensor(-float("inf")), torch.tensor(0.0))
        _CASES[key] = (lg, cnt, seen, table, q.to(torch.int32), gbias)
    return _CASES[key]


class _Step:
    """One decode step (column `step` of a T-column output) through o3v_sample_step_guided / o3v_sample_step_ex."""

    def __init__(self, lg, seen, counts, table):
        from open_o3_video_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.lg, self.B, self.V = lg.cuda(), lg.shape[0], lg.shape[1]
        self.seen0, self.counts0 = seen.cuda(), counts.to(torch.int16).cuda()
        self.table = None if table is None else table.cuda().contiguous()
        self.rid = torch.arange(self.B, dtype=torch.int32, device="cuda") * 3 + 1
        self.scratch = torch.zeros((self.B, _lib.SAMPLE_SCRATCH_FLOATS), dtype=torch.float32, device="cuda")

    def run(self, do_sample, m, q0=None, n=None, seed=11, step=1, entry="guided", fin=None, state=None, keep=None, so=True, T=3):
        """entry: "guided" | "guided_null" (go == NULL) | "ex".  q0: i32 [B] start states (both halves); state: a [2, B] device
        tensor to go on from.  keep: (seen, counts) to go on from.  so False: NULL options."""
        _lib, lib, B, V = self._lib, self.lib, self.B, self.V
        sn, cn = keep if keep is not None else (self.seen0.clone(), self.counts0.clone())
        cur = torch.zeros(B, dtype=torch.int32, device="cuda")
        fin = torch.zeros(B, dtype=torch.int32, device="cuda") if fin is None else fin.cuda()
        out_ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
        marg = torch.zeros((B, T), dtype=torch.float32, device="cuda")
        eos_t = torch.tensor([0x7fffffff], dtype=torch.int32, device="cuda")
        temp, top_k, top_p = (m["temp"], m["top_k"], m["top_p"]) if do_sample else (1.0, 0, 1.0)
        lp = opts = None
        if n is not None:
            lp = (torch.zeros((B, T), dtype=torch.float32, device="cuda"), torch.zeros((B, T), dtype=torch.int32, device="cuda"),
                  torch.full((B, T, max(n, 1)), -9, dtype=torch.int32, device="cuda"),
                  torch.zeros((B, T, max(n, 1)), dtype=torch.float32, device="cuda"))
            opts = _lib.LogprobOpts(n=n, chosen_lp=lp[0].data_ptr(), chosen_rank=lp[1].data_ptr(), top_ids=lp[2].data_ptr(),
                                    top_lp=lp[3].data_ptr())
        sopt = _lib.SamplingOpts(min_p=m.get("min_p", 0.0) if do_sample else 0.0, presence=m.get("pres", 0.0), frequency=m.get("freq", 0.0),
                                 out_counts=cn.data_ptr())
        args = (_p(self.lg), _p(sn), _p(cur), _p(fin), _p(out_ids), _p(marg), _p(eos_t), 1, -1, B, V, V, int(do_sample), m["rep"], temp,
                top_k, top_p, seed, _p(self.rid), step, T, _p(self.scratch), None if opts is None else C.byref(opts),
                C.byref(sopt) if so else None)
        if entry == "ex":
            _lib.check(lib.o3v_sample_step_ex(*args, _stream()), "o3v_sample_step_ex")
        elif entry == "guided_null":
            _lib.check(lib.o3v_sample_step_guided(*args, None, _stream()), "o3v_sample_step_guided")
        else:
            if state is None:
                state = torch.stack([q0, q0]).to(torch.int32).cuda().contiguous()
            go = _lib.GuidedOpts(next=self.table.data_ptr(), n_states=self.table.shape[0], ldn=self.table.shape[1], state=state.data_ptr())
            _lib.check(lib.o3v_sample_step_guided(*args, C.byref(go), _stream()), "o3v_sample_step_guided")
        torch.cuda.synchronize()
        res = dict(ids=out_ids[:, step].cpu(), marg=marg[:, step].cpu(), seen=sn, counts=cn, fin=fin.cpu(), cur=cur.cpu(), state=state)
        if lp is not None:
            res["lp"] = (lp[0][:, step].cpu(), lp[1][:, step].cpu(), lp[2][:, step, :n].cpu(), lp[3][:, step, :n].cpu())
        return res


def _kept_with_ties(raw, m):
    """The reference's kept set with a tie group at the top-k / top-p boundary kept whole, then min_p (as test_gpu_sampling_params);
    asserts that no token sits within a relative 1e-3 of the min_p threshold, where device expf and the CPU could disagree."""
    kp = kept_k_p(raw, m["top_k"], m["top_p"]) & torch.isfinite(raw)
    smallest = torch.where(kp, raw, torch.full_like(raw, float("inf"))).min(dim=1, keepdim=True).values
    kp = raw >= smallest
    e = sr.rel_e(raw, kp)
    mp = float(np.float32(m["min_p"]))
    assert float((e[kp] / mp - 1).abs().min()) > 1e-3, "a token sits at the min_p threshold"
    return kp & (e >= mp)


# ---------------------------------------------------------------------------------------------------------- 1. one step
@pytest.mark.parametrize("V,ldn", SHAPES)
@pytest.mark.parametrize("B", [1, 3, 32])
def test_greedy_step_is_the_masked_reference_argmax(need_gpu, V, ldn, B):
    lg, cnt, seen, table, q, gbias = _case(B, V, ldn)
    m = ALL
    lg = lg.clone()
    raw = sr.processed_scores(lg, seen, m["rep"], 1.0, cnt, m["pres"], m["freq"], gbias)
    top2 = torch.topk(raw, 2, dim=1)
    for b in torch.nonzero(top2.values[:, 0] - top2.values[:, 1] < 0.01)[:, 0].tolist():      # clear_winner: no tie for the first place
        i = int(raw[b].argmax())
        lg[b, i] = (lg[b, i].float() + 0.5).to(torch.bfloat16)
    s, lp_ref = sr.logprobs(lg, seen, m["rep"], counts=cnt, presence=m["pres"], frequency=m["freq"], bias=gbias)
    raw = sr.processed_scores(lg, seen, m["rep"], 1.0, cnt, m["pres"], m["freq"], gbias)
    top2 = torch.topk(raw, 2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-4
    allowed = table[q.long(), :V] >= 0
    assert (raw.argmax(1) != sr.processed_scores(lg, seen, m["rep"], 1.0, cnt, m["pres"], m["freq"]).argmax(1)).any() or B == 1, \
        "the guide changes at least one row's arg-max"
    r = _Step(lg, seen, cnt, table).run(0, m, q, n=20)
    ids = r["ids"].long()
    assert torch.equal(ids, raw.argmax(dim=1)) and allowed[torch.arange(B), ids].all()
    assert (r["marg"] - (top2[:, 0] - top2[:, 1])).abs().max().item() < 1e-4
    tok_lp, rank, top_ids, top_lp = r["lp"]
    assert (rank == 1).all() and torch.equal(top_ids[:, 0], r["ids"])
    ref_ids, ref_top = top_n(s, lp_ref, 20)
    assert int(allowed.sum(1).min()) >= 20 and np.array_equal(top_ids.numpy(), ref_ids)
    assert allowed.gather(1, top_ids.long()).all(), "a disallowed id among the top-N although more than N tokens are allowed"
    assert np.abs(top_lp.numpy() - ref_top).max() < LP_ATOL
    assert (tok_lp - lp_ref.gather(1, ids[:, None])[:, 0]).abs().max().item() < LP_ATOL
    # the last stage: the next state in the other half, the read half untouched, the token counted and marked seen
    st = r["state"].cpu()
    assert torch.equal(st[1], q) and torch.equal(st[0].long(), table[q.long(), ids].long())
    want = cnt.clone()
    want[torch.arange(B), ids] += 1
    assert torch.equal(r["counts"].cpu().to(torch.int32), want) and bool(r["seen"].cpu()[torch.arange(B), ids].all())


@pytest.mark.parametrize("V,ldn", SHAPES)
@pytest.mark.parametrize("B", [1, 3, 32])
def test_sampled_step_draws_inside_allowed_and_kept(need_gpu, V, ldn, B):
    lg, cnt, seen, table, q, gbias = _case(B, V, ldn)
    m = ALL
    raw = sr.processed_scores(lg, seen, m["rep"], m["temp"], cnt, m["pres"], m["freq"], gbias)
    kept = _kept_with_ties(raw, m)
    allowed = table[q.long(), :V] >= 0
    assert not (kept & ~allowed).any()
    st = _Step(lg, seen, cnt, table)
    s_k = torch.where(kept, raw, torch.full_like(raw, -float("inf")))
    lp_k = torch.log_softmax(s_k, dim=-1)
    ref_ids, ref_top = top_n(s_k, lp_k, 20)
    for seed in (11, 12, 13):
        r = st.run(1, m, q, n=20, seed=seed)
        ids = r["ids"].long()
        assert (allowed & kept)[torch.arange(B), ids].all(), "drawn outside allowed AND the reference's kept set"
        tok_lp, rank, top_ids, top_lp = r["lp"]
        assert np.array_equal(top_ids.numpy(), ref_ids), seed
        fin = np.isfinite(ref_top)
        assert np.array_equal(np.isfinite(top_lp.numpy()), fin)              # masked tokens at -inf
        assert np.abs(top_lp.numpy()[fin] - ref_top[fin]).max() < LP_ATOL
        assert allowed.gather(1, top_ids.long())[torch.from_numpy(fin)].all()
        assert np.array_equal(rank.numpy(), rank_of(s_k, ids))
        assert (tok_lp - lp_k.gather(1, ids[:, None])[:, 0]).abs().max().item() < LP_ATOL
        state = r["state"].cpu()
        assert torch.equal(state[1], q) and torch.equal(state[0].long(), table[q.long(), ids].long())


def test_fewer_than_n_allowed_and_finished_rows(need_gpu):
    V, ldn, B = 1003, 1008, 3
    lg, cnt, seen, table, q, _ = _case(B, V, ldn)
    table = table.clone()
    table[int(q[0])] = -1
    few = [5, 400, 1002]                                            # row 0's state allows three tokens, one in the scalar tail's last group
    table[int(q[0]), few] = torch.tensor([2, 2, 0], dtype=torch.int16)
    m = dict(rep=1.0, temp=1.0, top_k=0, top_p=1.0, pres=0.0, freq=0.0)
    fin = torch.tensor([0, 1, 0], dtype=torch.int32)
    for do_sample in (0, 1):
        r = _Step(lg, seen, cnt, table).run(do_sample, m, q, n=5, fin=fin)
        ids = r["ids"].tolist()
        assert ids[0] in few and ids[1] == -1                       # the finished row emits pad ...
        st = r["state"].cpu()
        assert int(st[0, 1]) == int(q[1]) and int(st[0, 0]) == int(table[int(q[0]), ids[0]])      # ... and keeps its state
        assert int(st[0, 2]) == int(table[int(q[2]), ids[2]]) >= 0
        tok_lp, rank, top_ids, top_lp = r["lp"]
        assert sorted(top_ids[0, :3].tolist()) == few and torch.isfinite(top_lp[0, :3]).all()
        assert top_ids[0, 3:].tolist() == [0, 1] and torch.isinf(top_lp[0, 3:]).all()              # masked ids follow at -inf, lowest first
        ref = torch.log_softmax(lg[0, few].float(), dim=0)
        got = {int(i): float(v) for i, v in zip(top_ids[0, :3], top_lp[0, :3])}
        assert max(abs(got[t] - float(ref[j])) for j, t in enumerate(few)) < LP_ATOL
        assert torch.equal(r["counts"].cpu()[1], cnt[1].to(torch.int16))                            # a finished row counts nothing


# ---------------------------------------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("V,ldn", SHAPES)
@pytest.mark.parametrize("do_sample", [0, 1])
def test_an_all_allowing_table_is_sample_step_ex(need_gpu, V, ldn, do_sample):
    B = 3
    lg, cnt, seen, table, q, _ = _case(B, V, ldn)
    free = torch.where(table < 0, torch.zeros_like(table), table)      # every entry >= 0, the padding included
    st = _Step(lg, seen, cnt, free)
    a = st.run(do_sample, ALL, n=5, entry="ex")
    for entry in ("guided", "guided_null"):
        b = st.run(do_sample, ALL, q, n=5, entry=entry)
        for k in ("ids", "marg", "cur", "fin"):
            assert torch.equal(a[k], b[k]), (entry, k)
        assert torch.equal(a["seen"], b["seen"]) and torch.equal(a["counts"], b["counts"])
        for x, y in zip(a["lp"], b["lp"]):
            assert torch.equal(x, y), entry         # chosen log-prob, rank, top ids and top log-probs, bit for bit
    # `so` NULL with a guide: a zeroed control set, i.e. the plain sampler's ids
    plain = dict(rep=1.05, temp=0.7, top_k=50, top_p=0.95)
    c = st.run(do_sample, plain, q, so=False)
    d = st.run(do_sample, plain, entry="ex")
    assert torch.equal(c["ids"], d["ids"]) and torch.equal(c["marg"], d["marg"])


# ---------------------------------------------------------------------------------------------------------- 3. three chained steps
def test_three_chained_steps_over_the_double_buffer(need_gpu):
    V, ldn, B = 4096, 4096, 3
    lg, cnt, seen, table, q0, _ = _case(B, V, ldn)
    m = dict(ALL)
    st = _Step(lg, seen, cnt, table)
    state = torch.stack([q0, q0]).to(torch.int32).cuda().contiguous()
    keep = (st.seen0.clone(), st.counts0.clone())
    q, seen_h, cnt_h = q0.long(), seen.clone(), cnt.clone()
    states, changed = [q0.long()], 0
    for step in range(3):
        r = st.run(0, m, n=3, step=step, state=state, keep=keep)
        ids = r["ids"].long()
        # the token obeys the state the previous step wrote; its log-prob is that of the state BEFORE this step
        assert (table[q, ids] >= 0).all(), step
        gb = torch.where(table[q, :V] < 0, torch.tensor(-float("inf")), torch.tensor(0.0))
        s, lp_ref = sr.logprobs(lg, seen_h, m["rep"], counts=cnt_h, presence=m["pres"], frequency=m["freq"], bias=gb)
        top2 = torch.topk(s, 2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-3
        assert torch.equal(ids[clear], s.argmax(1)[clear])
        assert (r["lp"][0] - lp_ref.gather(1, ids[:, None])[:, 0]).abs().max().item() < LP_ATOL, step
        nq = table[q, ids].long()
        assert torch.equal(state.cpu()[(step + 1) & 1].long(), nq) and torch.equal(state.cpu()[step & 1].long(), q)
        changed += int((nq != q).sum())
        seen_h[torch.arange(B), ids] = 1
        cnt_h[torch.arange(B), ids] += 1
        q = nq
        states.append(q)
    assert changed > 0, "no row ever changed its state: the chain shows nothing"


# ---------------------------------------------------------------------------------------------------------- 4. argument checks
def test_rejected_guides_return_err_arg_without_launching(need_gpu):
    from open_o3_video_amd import _lib
    lib = _lib.load()
    B, V, ldn = 3, 1003, 1008
    lg, cnt, seen, table, q, _ = _case(B, V, ldn)
    lgd, sn, tab = lg.cuda(), seen.cuda(), table.cuda().contiguous()
    state = torch.stack([q, q]).to(torch.int32).cuda().contiguous()
    cur, fin = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    out_ids = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    eos_t = torch.tensor([0x7fffffff], dtype=torch.int32, device="cuda")
    scratch = torch.zeros((B, _lib.SAMPLE_SCRATCH_FLOATS), dtype=torch.float32, device="cuda")
    ok = dict(next=tab.data_ptr(), n_states=N_STATES, ldn=ldn, state=state.data_ptr())
    bad = [dict(ok, next=0), dict(ok, state=0), dict(ok, next=tab.data_ptr() + 2), dict(ok, next=tab.data_ptr() + 8),
           dict(ok, state=state.data_ptr() + 2), dict(ok, n_states=0), dict(ok, n_states=-3), dict(ok, ldn=1000), dict(ok, ldn=1003),
           dict(ok, ldn=1004)]
    for kw in bad:
        for do_sample in (0, 1):
            for so in (None, _lib.SamplingOpts()):
                go = _lib.GuidedOpts(**kw)
                rc = lib.o3v_sample_step_guided(_p(lgd), _p(sn), _p(cur), _p(fin), _p(out_ids), None, _p(eos_t), 1, -1, B, V, V, do_sample,
                                                1.0, 1.0, 0, 1.0, 5, None, 1, 3, _p(scratch), None, None if so is None else C.byref(so),
                                                C.byref(go), _stream())
                assert rc == _lib.ERR_ARG, kw
    torch.cuda.synchronize()
    assert (out_ids == -7).all() and (cur == 0).all() and torch.equal(sn.cpu(), seen) and torch.equal(state.cpu()[0], q)


# ---------------------------------------------------------------------------------------------------------- 5. engine
def _guide(table, start=0):
    from open_o3_video_amd.guided import Guide
    t = table.contiguous()
    return Guide(table=t.cuda(), n_states=t.shape[0], ldn=t.shape[1], start=start, host_table=t.numpy())


def _walk(table, ids, start=0):
    q = start
    for t in ids:
        q = int(table[q, int(t)])
        assert q >= 0, f"token {t} is not allowed"
    return q


def _rect(rows, pad):
    L = max(len(r) for r in rows)
    return (np.asarray([[pad] * (L - len(r)) + list(r) for r in rows], dtype=np.int64),
            np.asarray([[0] * (L - len(r)) + [1] * len(r) for r in rows], dtype=np.int64))


def _engine_table(V, forbid_first, seed=4):
    """Four states, about half the vocabulary allowed in each; the start state forbids the tokens `forbid_first`."""
    t = _table(V, (V + 7) // 8 * 8, n_states=4, frac=0.5, seed=seed)
    t[0, list(forbid_first)] = -1
    return t


@pytest.fixture(scope="module")
def tiny(need_gpu, golden_dir):
    from test_gpu_model import build_engine
    g = np.load(os.path.join(golden_dir, "g6_tiny.npz"))
    cfg = fm.tiny_config()
    return dict(g=g, cfg=cfg, eng=build_engine(cfg, fm.make_weights(cfg, 0)), S=g["input_ids"].shape[1], T=12)


def test_engine_tiny_greedy_leaves_the_golden_and_obeys_the_table(tiny):
    g, cfg, eng, S, T = (tiny[k] for k in ("g", "cfg", "eng", "S", "T"))
    golden = g["bf16_ids"][0, S:S + T]
    kw = dict(frames=torch.from_numpy(g["frames"]), max_new_tokens=T, pad_token_id=cfg["pad_token_id"])
    plain = eng.generate(g["input_ids"], None, **kw)
    assert np.array_equal(plain.sequences.cpu().numpy()[0, S:], golden)
    table = _engine_table(cfg["text_config"]["vocab_size"], [int(golden[0])])
    out = eng.generate(g["input_ids"], None, guide=_guide(table), **kw)
    gen = out.sequences[0, S:].cpu().numpy()
    assert len(gen) == T and gen[0] != golden[0] and not np.array_equal(gen, golden)
    assert _walk(table, gen) == out.timings["guide_states"][0]
    assert out.timings["launches_per_layer"] == plain.timings["launches_per_layer"]          # B = 1: the one-launch block as before
    assert out.timings["fused_attention_layers"] == plain.timings["fused_attention_layers"]
    with pytest.raises(ValueError):
        eng.generate(g["input_ids"], None, guide=_guide(table), eos_token_ids=[3], min_new_tokens=2, **kw)
    dead = table.clone()
    dead[2] = -1                                # a reachable state without a token
    with pytest.raises(ValueError) as e:
        eng.generate(g["input_ids"], None, guide=_guide(dead), **kw)
    assert "state 2 " in str(e.value)
    with pytest.raises(ValueError):             # ... or with every one of its tokens banned by the call's static bias
        eng.generate(g["input_ids"], None, guide=_guide(table), banned_token_ids=np.flatnonzero(table[1].numpy() >= 0).tolist(), **kw)


def test_engine_tiny_every_decode_regime(tiny):
    g, cfg, eng, S, T = (tiny[k] for k in ("g", "cfg", "eng", "S", "T"))
    pad, V = cfg["pad_token_id"], cfg["text_config"]["vocab_size"]
    tids = g["input_ids"][0].tolist()
    tP = max(i for i, t in enumerate(tids) if t == cfg["vision_end_token_id"]) + 1
    trows = [tids, tids[:tP] + [33, 44], tids[:tP] + [55, 66, 77, 88, 99, 111, 122, 133], tids[:tP] + [21]]
    ids, mask = _rect(trows, pad)
    L = ids.shape[1]
    pv = torch.from_numpy(g["pixel_values"])
    ind = dict(pixel_values=torch.cat([pv] * 4), image_grid_thw=np.tile(g["grid"], (4, 1)), max_new_tokens=T, pad_token_id=pad)
    one = dict(pixel_values=pv, image_grid_thw=g["grid"], max_new_tokens=T, pad_token_id=pad)
    plain = eng.generate(ids, mask, **ind).sequences[:, L:].cpu().numpy()
    table = _engine_table(V, set(plain[:, 0].tolist()) | {int(g["bf16_ids"][0, S])})
    guide = _guide(table)

    def check(out, first_col, plain_rows=None):
        gen = out.sequences[:, first_col:].cpu().numpy()
        assert gen.shape[1] == T
        for b in range(gen.shape[0]):
            assert _walk(table, gen[b]) == out.timings["guide_states"][b], b
            if plain_rows is not None:
                assert gen[b, 0] != plain_rows[b, 0]
        return gen

    a = check(eng.generate(ids, mask, guide=guide, **ind), L, plain)                           # 4 independent rows
    samp = dict(do_sample=True, temperature=1.0, top_p=0.95, seed=3, num_return_sequences=4)
    s = check(eng.generate(g["input_ids"], None, guide=guide, **one, **samp), S)               # n = 4 samples of one prompt
    assert len({tuple(r) for r in s.tolist()}) > 1
    sp = eng.generate(ids, mask, guide=guide, shared_prefix_len=tP, **one)                     # shared prefix (head_dim 32: independent rows)
    assert np.array_equal(check(sp, L, plain), a)
    eng.kv_cache_dtype = "fp8"
    try:
        check(eng.generate(ids, mask, guide=guide, **ind), L, plain)                           # fp8 K/V asked for
    finally:
        eng.kv_cache_dtype = "bf16"
    lp = eng.generate(ids, mask, guide=guide, logprobs=3, **ind)                               # log-probs: never a masked token
    gen = check(lp, L, plain)
    assert np.array_equal(gen, a) and torch.isfinite(lp.logprobs.token).all()
    top = lp.logprobs.top_ids.cpu().numpy()
    for b in range(4):
        q = 0
        for j in range(T):
            assert (table[q, top[b, j]] >= 0).all(), (b, j)
            q = int(table[q, gen[b, j]])


def test_engine_medium_group_and_fp8_kv_regimes(need_gpu):
    """head_dim 128: the shared-prefix group kernels and the fp8 K/V cache really run"""
    from test_gpu_model import build_engine
    cfg = fm.medium_config()
    eng = build_engine(cfg, fm.make_weights(cfg, 6))
    pad, V, T = cfg["pad_token_id"], cfg["text_config"]["vocab_size"], 8
    g = torch.Generator().manual_seed(1)
    pre = torch.randint(10, 400, (14,), generator=g).tolist()
    rows = [pre + torch.randint(10, 400, (n,), generator=g).tolist() for n in (3, 1, 6, 4)]
    ids, mask = _rect(rows, pad)
    L = ids.shape[1]
    kw = dict(max_new_tokens=T, pad_token_id=pad)
    plain = eng.generate(ids, mask, **kw).sequences[:, L:].cpu().numpy()
    table = _engine_table(V, set(plain[:, 0].tolist()), seed=8)
    guide = _guide(table)

    def check(out):
        gen = out.sequences[:, L:].cpu().numpy()
        for b in range(4):
            assert gen[b, 0] != plain[b, 0] and _walk(table, gen[b]) == out.timings["guide_states"][b]
        return gen

    a = check(eng.generate(ids, mask, guide=guide, **kw))
    grp = eng.generate(ids, mask, guide=guide, shared_prefix_len=len(pre), **kw)
    assert grp.timings["shared_prefix_rows"] == 4
    check(grp)
    eng.kv_cache_dtype = "fp8"
    try:
        k8 = eng.generate(ids, mask, guide=guide, **kw)
    finally:
        eng.kv_cache_dtype = "bf16"
    assert k8.timings["kv_cache_dtype"] == "fp8"
    check(k8)
    one = eng.generate([rows[0]], None, guide=guide, do_sample=True, temperature=1.2, seed=5, num_return_sequences=8, **kw)
    gen = one.sequences[:, len(rows[0]):].cpu().numpy()
    for b in range(8):
        assert _walk(table, gen[b]) == one.timings["guide_states"][b]
    assert a.shape == (4, T)


# ---------------------------------------------------------------------------------------------------------- 6. façade
class ByteTokenizer:
    """A byte-level vocabulary of the tiny fixture's size: ids 0..255 are the single bytes (spelled in GPT-2's alphabet, as a
    byte-level BPE tokenizer exposes them), then a few merges; everything else, the model's special ids included, is unknown."""
    MERGES = ["<answer>", "</answer>", "<ans", "wer>", "</", "yes", "no", "unclear", "un", "clear", "ye", "r>A", "AB", "B</a", "swer", " the"]

    def __init__(self, V):
        from open_o3_video_amd.guided import _gpt2_unicode_to_byte
        b2u = {b: u for u, b in _gpt2_unicode_to_byte().items()}
        self.raw = [bytes([b]) for b in range(256)] + [m.encode() for m in self.MERGES]
        self.spelled = ["".join(b2u[b] for b in r) for r in self.raw]
        self.V = V
        self.all_special_ids = []

    def convert_ids_to_tokens(self, i):
        return self.spelled[i] if i < len(self.raw) else None

    def encode(self, text, add_special_tokens=False):
        return list(text.encode())

    def decode(self, ids, skip_special_tokens=True):
        return b"".join(self.raw[int(i)] for i in ids if int(i) < len(self.raw)).decode("utf-8", errors="replace")


def test_vllm_facade_regex_choice_length_logprobs_and_cache(tiny):
    from open_o3_video_amd.vllm_api import GuidedDecodingParams, LLM, SamplingParams
    cfg, eng = tiny["cfg"], tiny["eng"]
    V = cfg["text_config"]["vocab_size"]
    tok = ByteTokenizer(V)
    llm = LLM(engine=eng, tokenizer=tok, max_model_len=4096)
    pattern = "<answer>[ABCD]</answer>"
    words = ["<answer>" + c + "</answer>" for c in "ABCD"]
    prompts = [{"prompt": "Which one?"}, {"prompt": "And this, which?"}, {"prompt": "Q"}]
    greedy = SamplingParams(temperature=0.0, max_tokens=24, guided_decoding=GuidedDecodingParams(regex=pattern))
    outs = llm.generate(prompts, greedy)                                            # batched rows
    assert llm.guide_cache_hits == 0 and len(llm._guides) == 1
    for ro in outs:
        co = ro.outputs[0]
        assert re.fullmatch(pattern, co.text) and co.finish_reason == "stop", co.text
    sampled = SamplingParams(temperature=1.0, top_p=0.95, max_tokens=24, n=4, seed=2, guided_decoding={"regex": pattern})
    ro = llm.generate(prompts[0], sampled)[0]                                       # n samples of one prompt
    assert llm.guide_cache_hits == 1 and len(llm._guides) == 1                      # the same pattern: the table is reused
    assert len(ro.outputs) == 4 and all(re.fullmatch(pattern, co.text) and co.finish_reason == "stop" for co in ro.outputs)
    assert len({co.text for co in ro.outputs} | {tuple(co.token_ids) for co in ro.outputs}) > 2
    choice = SamplingParams(temperature=0.8, max_tokens=12, n=3, seed=1, guided_decoding={"choice": ["yes", "no", "unclear"]})
    for co in llm.generate(prompts[1], choice)[0].outputs:
        assert co.text in ("yes", "no", "unclear") and co.finish_reason == "stop"
    short = SamplingParams(temperature=0.0, max_tokens=3, guided_decoding={"regex": pattern})
    co = llm.generate(prompts[0], short)[0].outputs[0]
    assert co.finish_reason == "length" and len(co.token_ids) == 3 and any(w.startswith(co.text) for w in words) and co.text not in words
    # logprobs=3: while at least three tokens are allowed, no dict holds a disallowed one
    with_lp = SamplingParams(temperature=0.0, max_tokens=24, logprobs=3, guided_decoding={"regex": pattern})
    co = llm.generate(prompts[0], with_lp)[0].outputs[0]
    table = next(g for k, g in llm._guides.items() if k[0] == pattern).host_table
    q, wide = 0, 0
    for t, d in zip(co.token_ids, co.logprobs):
        ok = table[q, :V] >= 0
        if int(ok.sum()) >= 3:
            wide += 1
            assert all(ok[i] for i in d), (t, sorted(d))
        assert ok[t] and t in d
        q = int(table[q, t])
    assert wide >= 1 and re.fullmatch(pattern, co.text)
    # two more patterns: only the last two tables are kept
    llm.generate(prompts[2], SamplingParams(temperature=0.0, max_tokens=4, guided_decoding={"regex": "[ABCD]"}))
    assert len(llm._guides) == 2 and pattern in [k[0] for k in llm._guides]
