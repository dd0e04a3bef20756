"""Top-N log-probs without a GPU: the vLLM SamplingParams options, the façade's {token_id: Logprob} assembly from fixed engine
outputs (trimming at a stop id, cumulative_logprob, prompt_logprobs), the C ABI entries and their argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
from logprobs_ref import logprobs as ref_logprobs, rank_of, top_n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sampling_params_logprobs_range():
    from open_o3_video_amd.vllm_api import SamplingParams
    sp = SamplingParams(logprobs=5, prompt_logprobs=3)
    assert sp.logprobs == 5 and sp.prompt_logprobs == 3
    assert SamplingParams().logprobs is None and SamplingParams().prompt_logprobs is None
    SamplingParams(logprobs=0, prompt_logprobs=20)
    for kw in ({"logprobs": 21}, {"prompt_logprobs": 21}, {"logprobs": -1}):
        with pytest.raises(ValueError):
            SamplingParams(**kw)


class _Tok:
    def encode(self, text, add_special_tokens=False):
        return [int(w[1:]) for w in text.split()]

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"w{int(i)}" for i in ids)


class _FakeEngine:
    """Stands in for O3VEngine: returns fixed sequences and log-prob tensors (CPU) and records the calls."""
    MAX_ROWS = 32

    def __init__(self, cfg, T=5, N=3):
        self.cfg, self.T, self.N, self.calls = cfg, T, N, []
        self.position_mode = "tf5"

    def generate(self, input_ids, attention_mask=None, num_return_sequences=1, logprobs=0, prompt_logprobs=0, **kw):
        from open_o3_video_amd.engine import GenerateOutput, Logprobs
        self.calls.append(dict(logprobs=logprobs, prompt_logprobs=prompt_logprobs, G=num_return_sequences, **kw))
        ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.int64)
        B0, S = ids.shape
        G, T = num_return_sequences, self.T
        B = B0 * G
        gen = torch.arange(B * T, dtype=torch.int64).view(B, T) % 50 + 100
        gen[0, 2] = 510                                   # row 0 stops at its third token (eos of the fixture config)
        seqs = torch.cat([ids.repeat_interleave(G, 0), gen], 1)

        def lp_of(rows, cols, tgt, n):
            tok = -0.1 * (1 + torch.arange(rows * cols, dtype=torch.float32).view(rows, cols))
            rank = torch.full((rows, cols), 2, dtype=torch.int32)
            top_ids = torch.stack([torch.full((rows, cols), 7 + k, dtype=torch.int32) for k in range(n)], -1)
            top_ids[..., 0] = tgt.to(torch.int32)         # the token itself is the most likely one ...
            top_ids[0, 0, 0] = 3                          # ... except at one position, where it must still appear
            top = torch.stack([torch.full((rows, cols), -0.5 * (k + 1)) for k in range(n)], -1)
            return Logprobs(tok, rank, top_ids, top)

        lp = lp_of(B, T, gen, logprobs) if logprobs else None
        plp = lp_of(B0, S - 1, ids[:, 1:], prompt_logprobs) if prompt_logprobs else None
        return GenerateOutput(sequences=seqs, margins=None, n_steps=T, timings={}, logprobs=lp, prompt_logprobs=plp)


def _llm():
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.vllm_api import LLM
    eng = _FakeEngine(O3VConfig.from_dict(fm.tiny_config()))
    return LLM(engine=eng, tokenizer=_Tok()), eng


def test_facade_assembles_logprob_dicts():
    from open_o3_video_amd.vllm_api import Logprob, SamplingParams
    llm, eng = _llm()
    out = llm.generate({"prompt": "w1 w2 w3 w4"}, SamplingParams(temperature=0.0, max_tokens=5, logprobs=3, prompt_logprobs=2))
    assert eng.calls[-1]["logprobs"] == 3 and eng.calls[-1]["prompt_logprobs"] == 2
    ro = out[0]
    co = ro.outputs[0]
    # row 0 stops at its third token: token_ids and logprobs are trimmed alike
    assert co.finish_reason == "stop" and len(co.token_ids) == 2 and len(co.logprobs) == 2
    for j, (t, d) in enumerate(zip(co.token_ids, co.logprobs)):
        assert t in d and isinstance(d[t], Logprob)
        assert d[t].decoded_token == f"w{t}"
    d0 = co.logprobs[0]
    t0 = co.token_ids[0]
    # position 0: the token is not among the top entries -> its own rank, plus the 3 top entries with ranks 1..3
    assert d0[t0].rank == 2 and abs(d0[t0].logprob - (-0.1)) < 1e-6 and len(d0) == 4
    assert [d0[i].rank for i in (3, 8, 9)] == [1, 2, 3]
    # position 1: the token is the top entry -> rank 1 (the top entry wins), 3 entries in all
    d1 = co.logprobs[1]
    assert d1[co.token_ids[1]].rank == 1 and len(d1) == 3
    assert co.cumulative_logprob == pytest.approx(-0.1 + -0.2, abs=1e-6)
    # prompt: None first, then one dict per prompt token with that token in it
    assert ro.prompt_logprobs[0] is None and len(ro.prompt_logprobs) == len(ro.prompt_token_ids) == 4
    for t, d in zip(ro.prompt_token_ids[1:], ro.prompt_logprobs[1:]):
        assert t in d and len(d) <= 3


def test_facade_logprobs_zero_and_off():
    from open_o3_video_amd.vllm_api import SamplingParams
    llm, eng = _llm()
    out = llm.generate({"prompt": "w1 w2"}, SamplingParams(temperature=0.0, max_tokens=5))
    assert eng.calls[-1]["logprobs"] == 0 and eng.calls[-1]["prompt_logprobs"] == 0
    assert out[0].outputs[0].logprobs is None and out[0].outputs[0].cumulative_logprob is None and out[0].prompt_logprobs is None
    # logprobs=0: the token's own entry only (the engine is asked for one top entry)
    out = llm.generate({"prompt": "w1 w2"}, SamplingParams(temperature=0.0, max_tokens=5, logprobs=0))
    assert eng.calls[-1]["logprobs"] == 1
    co = out[0].outputs[0]
    assert all(list(d) == [t] for t, d in zip(co.token_ids, co.logprobs))


def test_facade_batched_requests_and_n_samples():
    from open_o3_video_amd.vllm_api import SamplingParams
    llm, eng = _llm()
    reqs = [{"prompt": "w1 w2 w3"}, {"prompt": "w4 w5 w6 w7 w8"}, {"prompt": "w9 w10"}]
    out = llm.generate(reqs, SamplingParams(temperature=0.0, max_tokens=5, logprobs=2, prompt_logprobs=1))
    assert len(eng.calls) == 1                       # one left-padded batch
    for ro in out:
        co = ro.outputs[0]
        assert len(co.logprobs) == len(co.token_ids)
        assert ro.prompt_logprobs[0] is None and len(ro.prompt_logprobs) == len(ro.prompt_token_ids)
        for t, d in zip(ro.prompt_token_ids[1:], ro.prompt_logprobs[1:]):
            assert t in d
    out = llm.generate({"prompt": "w1 w2 w3"}, SamplingParams(temperature=1.0, max_tokens=5, n=4, seed=3, logprobs=2,
                                                             prompt_logprobs=2))
    assert len(out[0].outputs) == 4 and len(out[0].prompt_logprobs) == 3
    for co in out[0].outputs:
        assert len(co.logprobs) == len(co.token_ids) and all(t in d for t, d in zip(co.token_ids, co.logprobs))


def test_reference_definition_orders_and_masks():
    """The torch definition the GPU tests compare against: ties to the lower id, masked tokens at -inf, greedy ignores the masks."""
    lg = torch.tensor([[1.0, 3.0, 3.0, 0.5, -2.0, 2.0]])
    seen = torch.tensor([[0, 0, 1, 0, 0, 0]], dtype=torch.uint8)
    s, lp = ref_logprobs(lg, seen, rep=1.5)
    ids, vals = top_n(s, lp, 3)
    assert ids.tolist() == [[1, 2, 5]] and rank_of(s, [2]).tolist() == [2]      # 3/1.5 = 2.0 ties with id 5: lower id first
    assert abs(np.exp(lp.numpy()).sum() - 1) < 1e-6
    s, lp = ref_logprobs(lg, None, temp=0.5, top_k=2, do_sample=True)
    ids, vals = top_n(s, lp, 4)
    assert ids[0, :2].tolist() == [1, 2] and np.isinf(vals[0, 2:]).all() and ids[0, 2:].tolist() == [0, 3]
    s, lp = ref_logprobs(lg, None, top_p=0.01, do_sample=True)
    assert torch.isfinite(lp).sum().item() == 2                                 # the tied maxima share one fate


def test_c_abi_logprob_entries_reject_bad_arguments():
    from open_o3_video_amd import _lib
    lib = _lib.load()
    assert lib.o3v_abi_version() == 6
    for name in ("o3v_sample_logprobs", "o3v_logprobs_rows", "o3v_llm_decode_lp"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    hdr = open(os.path.join(ROOT, "include", "o3v.h")).read()
    assert "#define O3V_MAX_LOGPROBS 20" in hdr and "#define O3V_LOGPROB_ROW_SCRATCH_FLOATS 384" in hdr
    assert _lib.MAX_LOGPROBS == 20 and _lib.LOGPROB_ROW_SCRATCH_FLOATS == 384
    fake = ctypes.c_void_p(0x1000)
    # n above the maximum, and a missing scratch, are refused before any launch
    assert lib.o3v_logprobs_rows(fake, fake, 4, 100, 100, 21, fake, fake, fake, fake, fake, None) == _lib.ERR_ARG
    assert lib.o3v_logprobs_rows(fake, fake, 4, 100, 100, 5, fake, fake, fake, fake, None, None) == _lib.ERR_ARG
    assert lib.o3v_logprobs_rows(fake, fake, 4, 100, 50, 5, fake, fake, fake, fake, fake, None) == _lib.ERR_ARG   # ldl < V
    opts = _lib.LogprobOpts(n=21, chosen_lp=0x1000, chosen_rank=0x1000, top_ids=0x1000, top_lp=0x1000)
    assert lib.o3v_sample_logprobs(fake, fake, fake, fake, fake, None, fake, 1, 0, 2, 100, 100, 0, 1.0, 1.0, 0, 1.0, 0, None, 0, 4,
                                   fake, ctypes.byref(opts), None) == _lib.ERR_ARG
    assert lib.o3v_sample_logprobs(fake, fake, fake, fake, fake, None, fake, 1, 0, 2, 100, 100, 0, 1.0, 1.0, 0, 1.0, 0, None, 0, 4,
                                   fake, None, None) == _lib.ERR_ARG
    assert lib.o3v_llm_decode_lp(None, None, None, 0, 1, 0, None) == _lib.ERR_ARG
