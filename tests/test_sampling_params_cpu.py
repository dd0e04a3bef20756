"""vLLM sampling controls without a GPU: SamplingParams fields and validation, the torch definition (tests/sampling_ref.py) pinned
against transformers' processors where it has the same operation, the façade's stop conditions over a fake engine, the engine's host
side (static-edit vectors) and the new C ABI entries with their argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- 1. SamplingParams
def test_sampling_params_defaults_and_validation():
    from open_o3_video_amd.vllm_api import SamplingParams
    sp = SamplingParams()
    assert (sp.top_k, sp.min_p, sp.presence_penalty, sp.frequency_penalty, sp.min_tokens) == (-1, 0.0, 0.0, 0.0, 0)
    assert sp.stop == [] and sp.include_stop_str_in_output is False and sp.ignore_eos is False and sp.skip_special_tokens is True
    assert sp.logit_bias is None and sp.allowed_token_ids is None and sp.bad_words is None
    # the nine fields that were there keep their defaults and take what they took
    assert (sp.temperature, sp.top_p, sp.repetition_penalty, sp.max_tokens, sp.stop_token_ids, sp.n, sp.seed, sp.logprobs,
            sp.prompt_logprobs) == (1.0, 1.0, 1.0, 16, None, 1, None, None, None)
    SamplingParams(temperature=0.0, top_p=0.3, repetition_penalty=1.3, max_tokens=1, stop_token_ids=[3], n=7, seed=5)
    ok = SamplingParams(temperature=0.7, top_k=50, min_p=0.05, presence_penalty=0.5, frequency_penalty=-2.0, stop="</answer>",
                        min_tokens=8, logit_bias={"7": 1.5, 9: -3}, allowed_token_ids=[1, 2, 3], bad_words=["no"])
    assert ok.stop == ["</answer>"] and ok.logit_bias == {7: 1.5, 9: -3.0} and ok.top_k == 50
    assert SamplingParams(stop=["a", "bc"]).stop == ["a", "bc"] and SamplingParams(min_tokens=16).min_tokens == 16
    bad = [dict(top_k=0), dict(top_k=-2), dict(min_p=-0.1), dict(min_p=1.5), dict(presence_penalty=2.5), dict(presence_penalty=-2.1),
           dict(frequency_penalty=2.01), dict(frequency_penalty=-3), dict(min_tokens=-1), dict(min_tokens=17), dict(stop=""),
           dict(stop=["x", ""]), dict(logit_bias={3: float("nan")}), dict(logit_bias={3: float("inf")}), dict(logit_bias={-1: 1.0}),
           dict(allowed_token_ids=[]), dict(allowed_token_ids=[-4]), dict(bad_words=[""]),
           dict(best_of=2), dict(logits_processors=[print]), dict(guided_decoding={"json": {}}), dict(truncate_prompt_tokens=5),
           dict(seed=[1, 2])]
    for kw in bad:
        with pytest.raises(ValueError) as e:
            SamplingParams(**kw)
        if next(iter(kw)) in ("best_of", "logits_processors", "guided_decoding", "truncate_prompt_tokens", "seed"):
            assert next(iter(kw)) in str(e.value)       # refused by name


# ---------------------------------------------------------------------------------------------------------- 2. the reference, pinned
def _row(V, seed):
    """Seeded fp32 logits with a hot set (as test_sample_top_k_top_p builds them, but left in fp32 and without its plateau: no two
    scores are equal, which is what exact set equality with transformers needs), output counts 1, 2, 3, 7, 40 on hot tokens plus
    a few hundred singletons, and a seen map covering them and 200 prompt tokens."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(V, generator=g) * 2.5
    hot = torch.randint(0, V, (30,), generator=g)
    base[hot] += 8.0
    lg = base
    cnt = torch.zeros(V)
    cnt.index_add_(0, torch.randint(0, V, (300,), generator=g), torch.ones(300))
    cnt[hot[:5]] += torch.tensor([1., 2., 3., 7., 40.])
    seen = cnt > 0
    prompt = torch.randint(0, V, (200,), generator=g)
    seen[prompt] = True
    return lg, cnt, seen, hot


@pytest.mark.parametrize("V", [997, 152064])
@pytest.mark.parametrize("seed", [13, 20, 63])
@pytest.mark.parametrize("rep,temp,top_k,top_p,min_p", [(1.0, 1.0, 0, 1.0, 0.05), (1.1, 0.8, 50, 0.95, 0.02), (1.05, 1.3, 0, 0.9, 0.2),
                                                       (1.3, 0.7, 20, 1.0, 0.001)])
def test_reference_equals_transformers_processors(V, seed, rep, temp, top_k, top_p, min_p):
    from transformers.generation import logits_process as lp_
    lg, _, seen, hot = _row(V, seed)
    eos = [int(hot[0]), int(hot[1])]            # two likely tokens as EOS ids: min-new-tokens has something to remove
    suppress = [int(hot[2]), 5, 6]
    input_ids = torch.nonzero(seen)[:, 0][None]         # what the repetition penalty gathers: every seen id
    prompt_len = input_ids.shape[1]                     # no new token yet -> min_new_tokens is active
    chain = []
    if rep != 1.0:
        chain.append(lp_.RepetitionPenaltyLogitsProcessor(penalty=rep))
    chain += [lp_.MinNewTokensLengthLogitsProcessor(prompt_len, 4, eos, device="cpu"),
              lp_.SuppressTokensLogitsProcessor(suppress, device="cpu")]
    if temp != 1.0:
        chain.append(lp_.TemperatureLogitsWarper(temp))
    if top_k:
        chain.append(lp_.TopKLogitsWarper(top_k))
    if top_p < 1.0:
        chain.append(lp_.TopPLogitsWarper(top_p))
    chain.append(lp_.MinPLogitsWarper(min_p))
    hf = lg[None].clone()
    for p in chain:
        hf = p(input_ids, hf)
    bias = sr.static_bias(V, banned=suppress, stop_ids=eos)
    ours, _ = sr.logprobs(lg[None], seen[None], rep, temp, top_k, top_p, True, min_p=min_p, bias=bias)
    # the property of the inputs that makes set equality exact: no tie at the top-k / top-p boundary, nothing at the min_p threshold
    s = sr.processed_scores(lg[None], seen[None], rep, temp, bias=bias)
    kept = torch.isfinite(ours[0])
    if top_k or top_p < 1.0:        # (min_p treats equal scores alike: a tie at ITS threshold is no ambiguity)
        from logprobs_ref import kept_mask as kept_k_p
        smallest = s[0][kept_k_p(s, top_k, top_p)[0] & torch.isfinite(s[0])].min()
        assert int((s[0] == smallest).sum()) == 1, "tie at the top-k / top-p boundary"
    # transformers takes the softmax in fp32, the reference e_i in float64: they differ by a few fp32 ulps (6e-8 relative), so a
    # token at least 1e-5 (relative) away from the threshold falls on the same side in both
    assert sr.min_p_margin(s, top_k, top_p, min_p) > 1e-5
    assert torch.equal(torch.isfinite(hf[0]), kept)
    assert torch.equal(hf[0][kept], ours[0][kept])                  # and the kept scores are the same fp32 numbers
    assert 1 <= int(kept.sum()) < V and not kept[suppress].any() and not kept[eos].any()


def test_reference_presence_frequency_unpinned():
    """Step 3 has no counterpart in transformers: the reference IS the definition (x -= f * c + p * [c > 0], fp32), checked on values
    that can be computed by hand."""
    lg = torch.tensor([[2.0, -1.0, 0.5, 3.0]])
    cnt = torch.tensor([[0, 2, 1, 40]])
    s = sr.processed_scores(lg, counts=cnt, presence=0.5, frequency=0.25)
    assert s.tolist() == [[2.0, -1.0 - 1.0, 0.5 - 0.75, 3.0 - 10.5]]
    s = sr.processed_scores(lg, seen=cnt > 0, rep=2.0, counts=cnt, presence=0.0, frequency=-0.5, temp=0.5)
    assert s.tolist() == [[4.0, (-2.0 + 1.0) * 2, (0.25 + 0.5) * 2, (1.5 + 20.0) * 2]]
    b = sr.static_bias(4, logit_bias={0: -1.0}, allowed=[0, 1, 3], banned=[1])
    assert b.tolist() == [-1.0, -math.inf, -math.inf, 0.0]
    s, lp = sr.logprobs(lg, bias=b)
    assert torch.isfinite(s).tolist() == [[True, False, False, True]] and abs(float(lp.exp().sum()) - 1) < 1e-6


# ---------------------------------------------------------------------------------------------------------- 3. façade over a fake engine
class _Tok:
    """'w<ID>' words joined WITHOUT a separator, so a stop string can straddle two tokens ('w1' + 'w23' contains '1w2')."""

    def encode(self, text, add_special_tokens=False):
        text = text.strip()
        return [int(w) for w in text.split("w") if w]

    def decode(self, ids, skip_special_tokens=True):
        return "".join(f"w{int(i)}" for i in ids)


class _FakeEngine:
    """Stands in for O3VEngine: every row emits `script` (or script[row]), honours eos ids and the stop checker per chunk of
    `chunk` steps exactly as the engine documents it, and records the keyword arguments of every call."""
    MAX_ROWS = 32

    def __init__(self, cfg, script, chunk=4):
        self.cfg, self.script, self.chunk, self.calls = cfg, script, chunk, []
        self.position_mode = "tf5"

    def generate(self, input_ids, attention_mask=None, num_return_sequences=1, max_new_tokens=16, eos_token_ids=(), pad_token_id=0,
                 stop_checker=None, **kw):
        from open_o3_video_amd.engine import GenerateOutput
        self.calls.append(dict(kw, eos_token_ids=list(eos_token_ids), max_new_tokens=max_new_tokens, G=num_return_sequences,
                               stop_checker=stop_checker))
        ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.int64)
        B = ids.shape[0] * num_return_sequences
        T = max_new_tokens
        per_row = isinstance(self.script[0], (list, tuple))
        gen = torch.full((B, T), pad_token_id, dtype=torch.int64)
        fin = [False] * B
        done = 0
        while done < T and not all(fin):
            for j in range(done, min(T, done + self.chunk)):
                for b in range(B):
                    sc = self.script[b % len(self.script)] if per_row else self.script
                    if not fin[b]:
                        gen[b, j] = sc[j % len(sc)]
                        fin[b] = int(gen[b, j]) in eos_token_ids
            done = min(T, done + self.chunk)
            if stop_checker is not None:
                for b, end in stop_checker(gen[:, :done].clone()).items():
                    fin[b] = True
                    gen[b, end:] = pad_token_id
        seqs = torch.cat([ids.repeat_interleave(num_return_sequences, 0), gen[:, :done]], 1)
        return GenerateOutput(sequences=seqs, margins=None, n_steps=done, timings={}, logprobs=None, prompt_logprobs=None)


def _llm(script, chunk=4):
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.vllm_api import LLM
    eng = _FakeEngine(O3VConfig.from_dict(fm.tiny_config()), script, chunk)
    return LLM(engine=eng, tokenizer=_Tok()), eng


def _token_by_token(toks, stop, min_tokens, include):
    """The definition: check after every single token; the first string in list order that the token's text completes."""
    dec = _Tok().decode
    for j in range(len(toks)):
        if j + 1 < min_tokens:
            continue
        text, before = dec(toks[:j + 1]), dec(toks[:j])
        for s_ in stop:
            i = text.find(s_, max(0, len(before) - len(s_) + 1))
            if i >= 0:
                return toks[:j + 1], text[:i + len(s_)] if include else text[:i], s_
    return toks, dec(toks), None


SCRIPT = [11, 12, 1, 23, 45, 6, 1, 23, 77, 78, 79, 80]


@pytest.mark.parametrize("chunk", [1, 4, 16])
@pytest.mark.parametrize("stop,min_tokens,include", [(["1w2"], 0, False),             # split across two tokens
                                                     (["1w2"], 0, True),
                                                     (["zz", "3w45", "w45"], 0, False),  # two complete at the same token: list order
                                                     (["w45", "3w45"], 0, False),
                                                     (["1w2"], 5, False),                 # the match inside the first 5 tokens is ignored
                                                     (["w23"], 4, True),                  # ... and one completing exactly at min_tokens counts
                                                     (["nothing"], 0, False)])
def test_stop_strings_equal_token_by_token_check(chunk, stop, min_tokens, include):
    from open_o3_video_amd.vllm_api import SamplingParams
    llm, eng = _llm(SCRIPT, chunk)
    sp = SamplingParams(temperature=0.0, max_tokens=12, stop=stop, min_tokens=min_tokens, include_stop_str_in_output=include)
    co = llm.generate({"prompt": "w1 w2"}, sp)[0].outputs[0]
    toks, text, why = _token_by_token(SCRIPT, stop, min_tokens, include)
    assert (co.token_ids, co.text, co.stop_reason) == (toks, text, why)
    assert co.finish_reason == ("stop" if why else "length")
    assert eng.calls[-1]["stop_checker"] is not None
    if why and chunk == 1:
        assert eng.calls[-1]["max_new_tokens"] == 12 and len(co.token_ids) < 12


def test_stop_reason_ignore_eos_and_min_tokens_on_stop_ids():
    from open_o3_video_amd.vllm_api import SamplingParams
    eos = fm.tiny_config()["eos_token_id"]
    script = [11, 12, eos, 13, 14, 99, 15, 16]
    llm, eng = _llm(script)
    g = lambda **kw: llm.generate({"prompt": "w1"}, SamplingParams(temperature=0.0, max_tokens=8, **kw))[0].outputs[0]
    co = g()
    assert (co.token_ids, co.finish_reason, co.stop_reason) == ([11, 12], "stop", None)               # EOS
    assert eos in eng.calls[-1]["eos_token_ids"]
    co = g(ignore_eos=True)
    assert (co.token_ids, co.finish_reason, co.stop_reason) == (script, "length", None)               # length
    assert eng.calls[-1]["eos_token_ids"] == []
    co = g(ignore_eos=True, stop_token_ids=[99])
    assert (co.token_ids, co.finish_reason, co.stop_reason) == ([11, 12, eos, 13, 14], "stop", 99)    # the stop token id
    assert eng.calls[-1]["eos_token_ids"] == [99]
    co = g(stop=["w14"])
    assert (co.token_ids, co.stop_reason, co.text) == ([11, 12], None, "w11w12")                      # EOS comes first
    co = g(ignore_eos=True, stop=["w14"], include_stop_str_in_output=True)
    assert (co.token_ids, co.stop_reason) == ([11, 12, eos, 13, 14], "w14") and co.text.endswith("w14")
    g(min_tokens=4)
    assert eng.calls[-1]["min_new_tokens"] == 4


def test_default_parameters_add_no_keyword():
    from open_o3_video_amd.vllm_api import SamplingParams
    llm, eng = _llm(SCRIPT)
    llm.generate({"prompt": "w1 w2"}, SamplingParams(temperature=0.7, top_p=0.9, max_tokens=4))
    plain = set(eng.calls[-1])
    new = {"min_p", "presence_penalty", "frequency_penalty", "min_new_tokens", "token_bias", "allowed_token_ids", "banned_token_ids",
           "top_k"}
    assert not plain & new and eng.calls[-1]["stop_checker"] is None
    # explicit defaults are defaults; greedy drops top_k / min_p as vLLM does
    llm.generate({"prompt": "w1 w2"}, SamplingParams(temperature=0.0, top_k=40, min_p=0.3, presence_penalty=0.0, max_tokens=4))
    assert set(eng.calls[-1]) == plain
    llm.generate({"prompt": "w1 w2"}, SamplingParams(temperature=0.7, top_k=40, min_p=0.3, presence_penalty=0.5, frequency_penalty=-0.25,
                                                     logit_bias={3: 2.0}, allowed_token_ids=[3, 4, 5], bad_words=["w4"], max_tokens=4))
    c = eng.calls[-1]
    assert (c["top_k"], c["min_p"], c["presence_penalty"], c["frequency_penalty"]) == (40, 0.3, 0.5, -0.25)
    assert c["token_bias"] == {3: 2.0} and c["allowed_token_ids"] == [3, 4, 5] and c["banned_token_ids"] == [4]


def test_list_of_sampling_params_groups_and_keeps_input_order():
    from open_o3_video_amd.vllm_api import SamplingParams
    llm, eng = _llm([[11, 12, 13, 14], [21, 22, 23, 24]])
    a = SamplingParams(temperature=0.0, max_tokens=3)
    b = SamplingParams(temperature=0.8, max_tokens=4, seed=None)
    reqs = [{"prompt": f"w{i}"} for i in range(1, 6)]
    out = llm.generate(reqs, [a, b, SamplingParams(temperature=0.0, max_tokens=3), b, a])
    assert len(eng.calls) == 2                                         # two groups: positions (0, 2, 4) and (1, 3)
    assert [c["row_ids"] for c in eng.calls] == [[0, 2, 4], [1, 3]]    # sampler keys follow the input position
    assert [ro.request_id for ro in out] == ["0", "1", "2", "3", "4"]
    assert [ro.prompt_token_ids for ro in out] == [[1], [2], [3], [4], [5]]
    assert [len(ro.outputs[0].token_ids) for ro in out] == [3, 4, 3, 4, 3]
    nxt = llm.generate({"prompt": "w9"}, a)
    assert nxt[0].request_id == "5"
    with pytest.raises(ValueError):
        llm.generate(reqs, [a, b])


def test_refused_bad_words_and_emptied_allowed_set():
    from open_o3_video_amd.engine import O3VEngine
    from open_o3_video_amd.vllm_api import SamplingParams
    llm, _ = _llm(SCRIPT)
    with pytest.raises(ValueError, match="bad_words"):
        llm.generate({"prompt": "w1"}, SamplingParams(bad_words=["w4w5"]))
    with pytest.raises(ValueError, match="allowed_token_ids"):
        llm.generate({"prompt": "w1"}, SamplingParams(allowed_token_ids=[4, 5], bad_words=["w4", "w5"]))
    eos = fm.tiny_config()["eos_token_id"]
    with pytest.raises(ValueError, match="allowed_token_ids"):
        llm.generate({"prompt": "w1"}, SamplingParams(allowed_token_ids=[eos], min_tokens=2))
    with pytest.raises(ValueError, match="vocabulary"):
        llm.generate({"prompt": "w1"}, SamplingParams(allowed_token_ids=[10 ** 7]))
    # the engine's own host side: the two dense vectors, and the same refusals
    V = 64
    assert O3VEngine._sampling_vectors(V, 8, [3], True, 0.0, 0.0, 0.0, 0, None, None, None) is None
    assert O3VEngine._sampling_vectors(V, 8, [], True, 0.0, 0.0, 0.0, 5, None, None, None) is None        # no stop id to hold back
    assert O3VEngine._sampling_vectors(V, 8, [3], False, 0.4, 0.0, 0.0, 0, None, None, None) is None      # greedy ignores min_p
    sv = O3VEngine._sampling_vectors(V, 8, [3, 9], True, 0.1, 0.5, 0.0, 2, {7: 1.5}, [3, 7, 8, 9], [8])
    want = sr.static_bias(V, {7: 1.5}, [3, 7, 8, 9], [8])
    assert torch.equal(torch.from_numpy(sv["bias"]), want)
    assert torch.equal(torch.from_numpy(sv["bias_early"]), sr.static_bias(V, {7: 1.5}, [3, 7, 8, 9], [8], stop_ids=[3, 9]))
    assert sv["counts"] and sv["min_tokens"] == 2 and sv["min_p"] == pytest.approx(0.1)
    for kw in (dict(allowed=[8], banned=[8]), dict(allowed=[3, 9], min_new=1), dict(allowed=[V]), dict(banned=[-1]),
               dict(bias={V: 1.0}), dict(bias={1: float("nan")}), dict(min_p=1.5), dict(pres=3.0), dict(pres=0.5, T=70000)):
        with pytest.raises(ValueError):
            O3VEngine._sampling_vectors(V, kw.get("T", 8), [3, 9], True, kw.get("min_p", 0.0), kw.get("pres", 0.0), 0.0,
                                        kw.get("min_new", 0), kw.get("bias"), kw.get("allowed"), kw.get("banned"))


def test_hf_facade_maps_controls():
    from types import SimpleNamespace
    from open_o3_video_amd.hf_api import GenerationConfigLike, Qwen2_5_VLForConditionalGeneration as M
    m = M.__new__(M)
    m.generation_config = GenerationConfigLike(min_new_tokens=3)
    out = m._extra_controls(SimpleNamespace(min_p=0.1, suppress_tokens=[4, 5]), {"bad_words_ids": [[9], [4]]}, True)
    assert out == {"min_p": 0.1, "min_new_tokens": 3, "banned_token_ids": [4, 5, 9]}
    assert m._extra_controls(None, {"min_p": 0.1}, False) == {"min_new_tokens": 3}        # greedy: no warper
    m.generation_config = GenerationConfigLike()
    assert m._extra_controls(None, {}, True) == {}
    with pytest.raises(NotImplementedError):
        m._extra_controls(None, {"bad_words_ids": [[1, 2]]}, True)
    with pytest.raises(ValueError):
        m._extra_controls(None, {"min_p": 1.5}, True)


# ---------------------------------------------------------------------------------------------------------- 4. C ABI
def test_c_abi_sampling_entries_reject_bad_arguments():
    from open_o3_video_amd import _lib
    lib = _lib.load()
    assert lib.o3v_abi_version() == 6
    for name in ("o3v_sample_step_ex", "o3v_llm_decode_ex"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "o3v.h")).read()
    assert "o3v_sampling_opts" in hdr and "_apply_min_p" in hdr and "apply_penalties" in hdr and "_apply_min_tokens_penalty" in hdr
    assert ctypes.sizeof(_lib.SamplingOpts) == 40 and _lib.SamplingOpts.bias.offset == 16
    fake = ctypes.c_void_p(0x1000)

    def step(so, lp=None):
        return lib.o3v_sample_step_ex(fake, fake, fake, fake, fake, None, fake, 1, 0, 2, 100, 100, 1, 1.0, 1.0, 0, 1.0, 0, None, 0, 4,
                                      fake, lp, so, None)

    O = _lib.SamplingOpts
    bad = [O(min_p=float("nan")), O(min_p=-0.1), O(min_p=1.5), O(presence=0.5), O(frequency=-0.5), O(presence=float("nan"), out_counts=0x1000),
           O(frequency=2.5, out_counts=0x1000), O(min_tokens=3), O(min_tokens=-1), O(bias=0x1004), O(min_tokens=1, bias_early=0x1008),
           O(presence=0.5, out_counts=0x1002)]
    for so in bad:
        assert step(ctypes.byref(so)) == _lib.ERR_ARG
        assert lib.o3v_llm_decode_ex(None, None, None, ctypes.byref(so), 0, 1, 0, None) == _lib.ERR_ARG
    assert step(None) == _lib.ERR_ARG                                   # the step entry needs its options
    opts = _lib.LogprobOpts(n=21, chosen_lp=0x1000, chosen_rank=0x1000, top_ids=0x1000, top_lp=0x1000)
    assert step(ctypes.byref(O()), ctypes.byref(opts)) == _lib.ERR_ARG  # log-prob options are checked as before
    assert lib.o3v_llm_decode_ex(None, None, None, None, 0, 1, 0, None) == _lib.ERR_ARG
