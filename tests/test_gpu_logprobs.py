"""Top-N log-probs on the GPU: the decode-step kernels (o3v_sample_logprobs) and the prompt-side entry (o3v_logprobs_rows) against
the fp32 torch definition of tests/logprobs_ref.py on the same bf16 logits, then the engine and the vLLM façade on the fixture
models (Qwen2.5-VL and Qwen3-VL): same ids with log-probs on and off, greedy ranks, decode log-probs against the teacher-forced
completion_logps, prompt log-probs against log_softmax(forward_logits)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
from logprobs_ref import logprobs as ref_logprobs, rank_of, top_n

pytestmark = pytest.mark.gpu

LP_ATOL = 2e-3


@pytest.fixture(scope="module")
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _logits(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn((B, V), generator=g) * 2.5
    hot = torch.randint(0, V, (B, 8), generator=g)
    lg.scatter_(1, hot, torch.rand((B, 8), generator=g) * 4 + 9)      # a few likely tokens per row
    return lg.to(torch.bfloat16)


def _seen(lg, seed):
    """~300 seen tokens per row, and the runner-up of every even row (so the penalty changes its order), never the argmax: the
    argmax is what greedy emits, and its log-prob must be taken BEFORE the step marks it seen."""
    B, V = lg.shape
    g = torch.Generator().manual_seed(seed)
    seen = torch.zeros((B, V), dtype=torch.uint8)
    seen.scatter_(1, torch.randint(0, V, (B, 300), generator=g), 1)
    order = torch.argsort(lg.float(), dim=1, descending=True)
    for b in range(B):
        seen[b, order[b, 0]] = 0
        if b % 2 == 0:
            seen[b, order[b, 1]] = 1
    return seen


MODES = {
    "greedy": dict(do_sample=0, rep=1.05, temp=1.0, top_k=0, top_p=1.0),
    "sample_k_p": dict(do_sample=1, rep=1.05, temp=0.7, top_k=50, top_p=0.95),
    "sample_p": dict(do_sample=1, rep=1.05, temp=1.0, top_k=0, top_p=0.95),
    "sample_narrow": dict(do_sample=1, rep=1.0, temp=0.7, top_k=0, top_p=0.02),   # fewer kept tokens than N: -inf entries
}


def _run_sampler(lib, _lib, lg, seen, m, n, seed, with_lp=True):
    B, V = lg.shape
    dev = lg.device
    sn = seen.clone()
    cur = torch.zeros(B, dtype=torch.int32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev)
    T, step = 3, 1
    out_ids = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    marg = torch.zeros((B, T), dtype=torch.float32, device=dev)
    eos = torch.tensor([0x7fffffff], dtype=torch.int32, device=dev)
    scratch = torch.zeros((B, _lib.SAMPLE_SCRATCH_FLOATS), dtype=torch.float32, device=dev)
    rid = torch.arange(B, dtype=torch.int32, device=dev) * 3 + 1
    args = (_p(lg), _p(sn), _p(cur), _p(fin), _p(out_ids), _p(marg), _p(eos), 1, -1, B, V, V)
    if not with_lp:
        if m["do_sample"]:
            _lib.check(lib.o3v_sample_top_k_top_p(*args, m["rep"], m["temp"], m["top_k"], m["top_p"], seed, _p(rid), step, T,
                                                  _p(scratch), _stream()), "sample")
        else:
            _lib.check(lib.o3v_sample_greedy(*args, m["rep"], step, T, _p(scratch), _stream()), "greedy")
        return out_ids[:, step].cpu(), marg[:, step].cpu(), sn.cpu(), None
    lp_tok = torch.zeros((B, T), dtype=torch.float32, device=dev)
    rank = torch.zeros((B, T), dtype=torch.int32, device=dev)
    tid = torch.full((B, T, max(n, 1)), -9, dtype=torch.int32, device=dev)
    tlp = torch.zeros((B, T, max(n, 1)), dtype=torch.float32, device=dev)
    opts = _lib.LogprobOpts(n=n, chosen_lp=lp_tok.data_ptr(), chosen_rank=rank.data_ptr(), top_ids=tid.data_ptr(), top_lp=tlp.data_ptr())
    _lib.check(lib.o3v_sample_logprobs(*args, m["do_sample"], m["rep"], m["temp"], m["top_k"], m["top_p"], seed, _p(rid), step, T,
                                       _p(scratch), C.byref(opts), _stream()), "o3v_sample_logprobs")
    torch.cuda.synchronize()
    return (out_ids[:, step].cpu(), marg[:, step].cpu(), sn.cpu(),
            (lp_tok[:, step].cpu(), rank[:, step].cpu(), tid[:, step, :n].cpu(), tlp[:, step, :n].cpu()))


@pytest.mark.parametrize("V", [152064, 1001])
@pytest.mark.parametrize("B", [1, 8, 32])
@pytest.mark.parametrize("mode", list(MODES))
def test_decode_step_logprobs_against_torch(need_gpu, V, B, mode):
    from open_o3_video_amd import _lib
    lib = _lib.load()
    m = MODES[mode]
    lg_cpu = _logits(B, V, seed=V + B)
    seen_cpu = _seen(lg_cpu, seed=B)
    lg, seen = lg_cpu.cuda(), seen_cpu.cuda()
    s_ref, lp_ref = ref_logprobs(lg_cpu, seen_cpu, m["rep"], m["temp"], m["top_k"], m["top_p"], bool(m["do_sample"]))
    ids0, marg0, seen0, _ = _run_sampler(lib, _lib, lg, seen, m, 0, seed=11, with_lp=False)
    for n in (1, 5, 20):
        ids, marg, seen1, (tok_lp, rank, top_ids, top_lp) = _run_sampler(lib, _lib, lg, seen, m, n, seed=11)
        # the sampler is untouched: same ids, margins and seen map as without log-probs
        assert torch.equal(ids, ids0) and torch.equal(marg, marg0) and torch.equal(seen1, seen0), (mode, n)
        assert torch.isfinite(s_ref.gather(1, ids.long()[:, None])).all(), "the drawn token is in the kept set"
        ref_ids, ref_top = top_n(s_ref, lp_ref, n)
        assert np.array_equal(top_ids.numpy(), ref_ids), (mode, n)
        fin = np.isfinite(ref_top)
        assert np.array_equal(np.isfinite(top_lp.numpy()), fin)
        assert np.abs(top_lp.numpy()[fin] - ref_top[fin]).max() < LP_ATOL
        assert np.array_equal(rank.numpy(), rank_of(s_ref, ids)), (mode, n)
        ref_tok = lp_ref.gather(1, ids.long()[:, None])[:, 0]
        assert (tok_lp - ref_tok).abs().max().item() < LP_ATOL
        if not m["do_sample"]:
            assert (rank == 1).all() and torch.equal(top_ids[:, 0], ids)


@pytest.mark.parametrize("V", [152064, 1001])
def test_prompt_rows_logprobs(need_gpu, V):
    from open_o3_video_amd import _lib
    lib = _lib.load()
    R, n = 37, 20
    lg_cpu = _logits(R, V, seed=5)
    tgt_cpu = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    lg, tgt = lg_cpu.cuda(), tgt_cpu.cuda()
    tok = torch.zeros(R, dtype=torch.float32, device="cuda")
    rank = torch.zeros(R, dtype=torch.int32, device="cuda")
    tid = torch.zeros((R, n), dtype=torch.int32, device="cuda")
    tlp = torch.zeros((R, n), dtype=torch.float32, device="cuda")
    scratch = torch.empty((R, _lib.LOGPROB_ROW_SCRATCH_FLOATS), dtype=torch.float32, device="cuda")
    _lib.check(lib.o3v_logprobs_rows(_p(lg), _p(tgt), R, V, V, n, _p(tok), _p(rank), _p(tid), _p(tlp), _p(scratch), _stream()), "rows")
    gather = torch.empty(R, dtype=torch.float32, device="cuda")
    _lib.check(lib.o3v_logprob_gather(_p(lg), _p(tgt), _p(gather), R, V, V, _stream()), "gather")
    torch.cuda.synchronize()
    s_ref, lp_ref = ref_logprobs(lg_cpu)
    ref_ids, ref_top = top_n(s_ref, lp_ref, n)
    assert np.array_equal(tid.cpu().numpy(), ref_ids)
    assert np.abs(tlp.cpu().numpy() - ref_top).max() < LP_ATOL
    assert np.array_equal(rank.cpu().numpy(), rank_of(s_ref, tgt_cpu))
    assert (tok.cpu() - lp_ref.gather(1, tgt_cpu.long()[:, None])[:, 0]).abs().max().item() < LP_ATOL
    assert (tok - gather).abs().max().item() < 1e-4                      # the same target log-prob as o3v_logprob_gather


# ---------------------------------------------------------------------------------------------------------- engine
def _medium():
    from test_gpu_model import build_engine
    cfg = fm.medium_config()
    W = fm.make_weights(cfg, 6)
    eng = build_engine(cfg, W)
    frames = fm.make_frames(2, 56, 84, seed=9)
    _, grid = eng.pixels_from_frames(frames)
    ids = fm.make_prompt(cfg, [tuple(r) for r in grid.tolist()], seed=9)
    return cfg, eng, frames, ids


def _check_prompt_lp(eng, plp_row, seq_ids, logits_row, n, atol):
    """plp_row: engine Logprobs row slices [S-1(, n)]; logits_row bf16 [S, V] of forward_logits.  atol: the suite's logit tolerance
    where the two heads may run on different kernels (<= 8 rows stream the GEMV, more the MFMA GEMM)."""
    ref = torch.log_softmax(logits_row[:-1].float(), dim=-1)
    tgt = torch.as_tensor(seq_ids[1:], device=ref.device).long()
    assert (plp_row[0] - ref.gather(1, tgt[:, None])[:, 0]).abs().max().item() < atol
    # every reported top entry carries its own log-prob, and they are the n largest (up to ties at the rounding level)
    assert (ref.gather(1, plp_row[2].long()) - plp_row[3]).abs().max().item() < atol
    assert (ref.topk(n, dim=-1).values - plp_row[3]).abs().max().item() < atol


def test_engine_logprobs_greedy_sampled_and_teacher_forced(need_gpu):
    from test_gpu_model import LOGIT_ATOL
    cfg, eng, frames, ids = _medium()
    pad = cfg["pad_token_id"]
    S, T = len(ids), 10
    # greedy with repetition penalty: same ids, rank 1, the token first among the top entries
    kw = dict(frames=frames, max_new_tokens=T, pad_token_id=pad, repetition_penalty=1.05, sync_timings=False)
    off = eng.generate([ids], None, **kw)
    on = eng.generate([ids], None, logprobs=5, prompt_logprobs=4, **kw)
    assert torch.equal(off.sequences, on.sequences) and off.logprobs is None and off.prompt_logprobs is None
    assert on.timings["launches_per_layer"] == off.timings["launches_per_layer"]
    gen = on.sequences[:, S:]
    lp = on.logprobs
    assert lp.token.shape == (1, T) and lp.top_ids.shape == (1, T, 5)
    assert (lp.rank == 1).all() and torch.equal(lp.top_ids[:, :, 0].long(), gen)
    assert (lp.token <= 0).all() and torch.equal(lp.token, lp.top[:, :, 0])
    # prompt log-probs: log_softmax of forward_logits at the prompt tokens
    lg = eng.forward_logits(np.asarray([ids]), None, frames=frames)
    _check_prompt_lp(eng, [t[0] for t in (on.prompt_logprobs.token, on.prompt_logprobs.rank, on.prompt_logprobs.top_ids,
                                          on.prompt_logprobs.top)], ids, lg[0], 4, LOGIT_ATOL)
    # penalty 1: decode log-probs are the teacher-forced ones of the same completion
    g1 = eng.generate([ids], None, frames=frames, max_new_tokens=T, pad_token_id=pad, logprobs=1)
    tf = eng.completion_logps(ids, g1.sequences[:, S:], frames=frames)
    assert (g1.logprobs.token - tf).abs().max().item() < LOGIT_ATOL
    # sampled, G = 4 completions of one prompt, top-k + top-p: same ids (seeded), ranks >= 1, the drawn token kept (finite)
    kw = dict(frames=frames, max_new_tokens=T, pad_token_id=pad, do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=4,
              num_return_sequences=4, repetition_penalty=1.05)
    off = eng.generate([ids], None, **kw)
    on = eng.generate([ids], None, logprobs=20, **kw)
    assert torch.equal(off.sequences, on.sequences) and torch.equal(off.margins, on.margins)
    assert on.logprobs.top_ids.shape == (4, T, 20)
    assert torch.isfinite(on.logprobs.token).all() and (on.logprobs.token <= 1e-6).all() and (on.logprobs.rank >= 1).all()
    top = on.logprobs.top
    assert (top[:, :, :-1] >= top[:, :, 1:]).all()
    # the drawn token sits at its rank among the top entries when that rank is within them
    r = on.logprobs.rank.long()
    inside = r <= 20
    at = torch.gather(on.logprobs.top, 2, (r.clamp(max=20) - 1)[..., None])[..., 0]
    assert ((at - on.logprobs.token).abs()[inside] < 1e-5).all()


def test_engine_logprobs_batched_left_padded_and_fp8_rows(need_gpu):
    from test_gpu_model import LOGIT_ATOL, build_engine
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    cfg = fm.medium_config()
    W = fm.make_weights(cfg, 6)
    eng = build_engine(cfg, W)
    pad = cfg["pad_token_id"]
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(10, 400, (L,), generator=g).tolist() for L in (9, 14, 5)]
    L = max(len(p) for p in prompts)
    rows = [[pad] * (L - len(p)) + p for p in prompts]
    mask = [[0] * (L - len(p)) + [1] * len(p) for p in prompts]
    kw = dict(max_new_tokens=6, pad_token_id=pad, repetition_penalty=1.05)
    off = eng.generate(rows, mask, **kw)
    on = eng.generate(rows, mask, logprobs=3, prompt_logprobs=3, **kw)
    assert torch.equal(off.sequences, on.sequences)
    assert (on.logprobs.rank == 1).all() and torch.equal(on.logprobs.top_ids[:, :, 0].long(), on.sequences[:, L:])
    for i, p in enumerate(prompts):
        lg = eng.forward_logits(np.asarray([p]), None)
        c0 = L - len(p)
        pl = on.prompt_logprobs
        _check_prompt_lp(eng, [t[i, c0:] for t in (pl.token, pl.rank, pl.top_ids, pl.top)], p, lg[0], 3, LOGIT_ATOL)
    # fp8 decode rows (4+ rows of one prompt): the same ids with log-probs on and off
    c = O3VConfig.from_dict(cfg)
    e8 = O3VEngine(c, DeviceWeights(c, getter_from_dict(W), "cuda", fp8_decode=True))
    kw = dict(max_new_tokens=6, pad_token_id=pad, num_return_sequences=8, do_sample=True, top_p=0.95, seed=2)
    a = e8.generate([prompts[1]], None, **kw)
    b = e8.generate([prompts[1]], None, logprobs=5, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.isfinite(b.logprobs.token).all()


def test_engine_logprobs_qwen3vl(need_gpu, golden_dir):
    import fixture_models_q3 as fq
    from test_gpu_model import LOGIT_ATOL
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.weights import DeviceWeights, getter_from_dict
    gd = np.load(os.path.join(golden_dir, "g12_q3_tiny.npz"))
    cfg = fq.tiny_q3_config()
    c = O3VConfig.from_dict(cfg)
    eng = O3VEngine(c, DeviceWeights(c, getter_from_dict(fq.make_weights(cfg, 0)), "cuda"))
    pv = torch.from_numpy(gd["pixel_values"])
    ids = gd["input_ids"]
    S = ids.shape[1]
    kw = dict(pixel_values=pv, image_grid_thw=gd["grid"], max_new_tokens=8, pad_token_id=cfg["pad_token_id"])
    off = eng.generate(ids, None, **kw)
    on = eng.generate(ids, None, logprobs=5, prompt_logprobs=5, **kw)
    assert torch.equal(off.sequences, on.sequences)
    assert (on.logprobs.rank == 1).all() and torch.equal(on.logprobs.top_ids[:, :, 0].long(), on.sequences[:, S:])
    lg = eng.forward_logits(ids, None, pixel_values=pv, image_grid_thw=gd["grid"])
    pl = on.prompt_logprobs
    _check_prompt_lp(eng, [t[0] for t in (pl.token, pl.rank, pl.top_ids, pl.top)], ids[0].tolist(), lg[0], 5, LOGIT_ATOL)
    # grouped sampling on the qk-norm decode path
    kw = dict(kw, do_sample=True, top_p=0.9, num_return_sequences=4, seed=5)
    a = eng.generate(ids, None, **kw)
    b = eng.generate(ids, None, logprobs=3, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.isfinite(b.logprobs.token).all()


# ---------------------------------------------------------------------------------------------------------- façade
def test_vllm_facade_logprobs(need_gpu):
    from test_gpu_facades import StubTokenizer
    from test_gpu_model import LOGIT_ATOL, build_engine
    from open_o3_video_amd.vllm_api import LLM, SamplingParams
    cfg = fm.medium_config()
    eng = build_engine(cfg, fm.make_weights(cfg, 6))
    llm = LLM(engine=eng, tokenizer=StubTokenizer(cfg), max_model_len=4096)
    g = torch.Generator().manual_seed(7)
    prompts = [" ".join(f"w{t}" for t in torch.randint(10, 400, (L,), generator=g).tolist()) for L in (7, 12, 4)]
    # n = 4 seeded samples of one prompt: same tokens with and without log-probs
    base = dict(temperature=0.8, top_p=0.95, max_tokens=8, n=4, seed=3, repetition_penalty=1.05)
    a = llm.generate({"prompt": prompts[1]}, SamplingParams(**base))
    b = llm.generate({"prompt": prompts[1]}, SamplingParams(**base, logprobs=5, prompt_logprobs=3))
    assert [o.token_ids for o in a[0].outputs] == [o.token_ids for o in b[0].outputs]
    ids = b[0].prompt_token_ids
    assert b[0].prompt_logprobs[0] is None and len(b[0].prompt_logprobs) == len(ids)
    lg = eng.forward_logits(np.asarray([ids]), None)
    ref = torch.log_softmax(lg[0].float(), dim=-1).cpu()
    for k in range(1, len(ids)):
        d = b[0].prompt_logprobs[k]
        assert ids[k] in d and abs(d[ids[k]].logprob - ref[k - 1, ids[k]].item()) < LOGIT_ATOL
        assert len(d) in (3, 4)
    for o in b[0].outputs:
        assert len(o.logprobs) == len(o.token_ids)
        assert all(t in d and d[t].rank >= 1 for t, d in zip(o.token_ids, o.logprobs))
        assert o.cumulative_logprob == pytest.approx(sum(d[t].logprob for t, d in zip(o.token_ids, o.logprobs)), abs=1e-4)
    # three requests decoded together (left-padded batch): same tokens, greedy ranks 1, prompt log-probs per request
    sp = dict(temperature=0.0, max_tokens=6, repetition_penalty=1.05)
    reqs = [{"prompt": p} for p in prompts]
    a = llm.generate(reqs, SamplingParams(**sp))
    b = llm.generate(reqs, SamplingParams(**sp, logprobs=2, prompt_logprobs=2))
    for ra, rb in zip(a, b):
        assert ra.outputs[0].token_ids == rb.outputs[0].token_ids
        o = rb.outputs[0]
        assert all(d[t].rank == 1 for t, d in zip(o.token_ids, o.logprobs))
        ids = rb.prompt_token_ids
        ref = torch.log_softmax(eng.forward_logits(np.asarray([ids]), None)[0].float(), dim=-1).cpu()
        assert rb.prompt_logprobs[0] is None and len(rb.prompt_logprobs) == len(ids)
        for k in range(1, len(ids)):
            assert abs(rb.prompt_logprobs[k][ids[k]].logprob - ref[k - 1, ids[k]].item()) < LOGIT_ATOL
