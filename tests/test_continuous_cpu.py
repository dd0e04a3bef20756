"""Continuous batching without a GPU: the admit / retire / roll-over bookkeeping (open_o3_video_amd.continuous) driven by a fake
decode, the facade's eligibility predicate and routing over a fake engine, and the C ABI of the ragged regime."""
import ctypes

import numpy as np
import pytest
import torch

import fixture_models as fm
from open_o3_video_amd import _lib
from open_o3_video_amd.continuous import IDLE_BASE, ContinuousScheduler, default_session_columns

EOS = 7


def _drive(prompt_lens, max_new, ends, rows, columns, sync):
    """Runs the scheduler against a fake decode: request r emits 100 + r at every column, and EOS as its ends[r]-th token (None:
    never).  Rows without a request emit -1.  Checks the invariants at every boundary -> (scheduler, admissions, results)."""
    s = ContinuousScheduler(prompt_lens, max_new, rows, columns, sync, [EOS])
    emitted = {}                # request -> tokens emitted so far (the fake device keeps going until the host retires the row)
    admissions, results, chunks = [], {}, []
    base = [IDLE_BASE] * rows
    owner = [None] * rows
    while not s.done():
        t_before = s.t if s.live() else None
        for a in s.admit():
            assert owner[a.row] is None, "admitted into a live row"
            assert a.t0 + max_new[a.request] <= columns
            assert a.row_base == prompt_lens[a.request] - a.t0
            assert t_before is None or a.t0 == t_before
            owner[a.row], base[a.row] = a.request, a.row_base
            emitted[a.request] = 0
            admissions.append(a)
        assert s.row_base() == base
        c = s.chunk()
        assert c.step0 == s.t and 1 <= c.n_steps <= sync and c.step0 + c.n_steps <= columns
        chunks.append(c)
        ids = np.full((rows, c.n_steps), -1, dtype=np.int64)
        for b in range(rows):
            r = owner[b]
            if r is None:
                continue
            for j in range(c.n_steps):
                emitted[r] += 1
                ids[b, j] = EOS if ends[r] is not None and emitted[r] >= ends[r] else 100 + r
            # every live row's context stays inside the cache the engine sizes: S + max_new + steps_per_sync
            assert base[b] + c.step0 + c.n_steps <= prompt_lens[r] + max_new[r] + sync - 1
        if c.skip_last_forward:     # nobody may need the logits of the last forward
            assert all(owner[b] is None or s.row_t0[b] + max_new[owner[b]] <= c.step0 + c.n_steps for b in range(rows))
        for r in s.retire(ids):
            assert owner[r.row] == r.request and r.request not in results
            toks = s.row_toks[r.row][:r.n]
            results[r.request] = (r.t0, r.n, toks)
            owner[r.row], base[r.row] = None, IDLE_BASE
        assert s.row_base() == base, "retired rows are idle"
    return s, admissions, results


def _expected_tokens(r, max_new, ends):
    n = max_new[r] if ends[r] is None or ends[r] > max_new[r] else ends[r]
    return [EOS if ends[r] is not None and j + 1 >= ends[r] else 100 + r for j in range(n)]


def test_every_request_is_admitted_once_and_sliced_at_its_columns():
    lens = [9, 12, 9, 17, 12, 9, 17, 9, 12, 17, 9]
    max_new = [3, 9, 20, 9, 3, 20, 3, 9, 20, 3, 9]
    ends = [None, 4, None, 1, None, 13, 3, None, 20, None, 2]
    s, adm, res = _drive(lens, max_new, ends, rows=4, columns=64, sync=4)
    assert sorted(a.request for a in adm) == list(range(11)) and [a.request for a in adm] == list(range(11))   # once, in order
    assert s.sessions == 1 and s.rows_refilled == 7 and sum(a.refill for a in adm) == 7
    for r in range(11):
        t0, n, toks = res[r]
        assert toks == _expected_tokens(r, max_new, ends), r
        assert n == len(toks) and t0 % 4 == 0
    assert [a.t0 for a in adm[:4]] == [0, 0, 0, 0] and all(a.t0 > 0 for a in adm[4:])
    # steps_per_sync = 1: the same tokens, rows refilled at once
    s1, adm1, res1 = _drive(lens, max_new, ends, rows=4, columns=64, sync=1)
    assert {r: v[2] for r, v in res1.items()} == {r: v[2] for r, v in res.items()}
    assert s1.decode_steps <= s.decode_steps


def test_roll_over_when_the_next_request_does_not_fit():
    lens = [5] * 9
    max_new = [20, 3, 9, 20, 9, 3, 20, 9, 3]
    ends = [None] * 9
    s, adm, res = _drive(lens, max_new, ends, rows=4, columns=24, sync=4)
    assert s.sessions >= 2
    assert all(a.t0 + max_new[a.request] <= 24 for a in adm)
    assert sorted(res) == list(range(9)) and all(res[r][1] == max_new[r] for r in range(9))
    # a session opens at column 0 and only once every row has drained
    opens = [i for i, a in enumerate(adm) if a.t0 == 0]
    assert opens[0] == 0 and len(opens) > 4
    with pytest.raises(ValueError):
        ContinuousScheduler([5], [25], 4, 24, 4)          # longer than a session
    with pytest.raises(ValueError):
        ContinuousScheduler([5], [0], 4, 24, 4)


def test_skewed_workload_needs_fewer_steps_than_static_batches():
    max_new = [40, 5, 4, 3, 5, 2, 4, 5]
    s, _, _ = _drive([6] * 8, max_new, [None] * 8, rows=4, columns=64, sync=4)
    static = sum(max(max_new[i:i + 4]) for i in (0, 4))
    assert s.decode_steps < static
    assert default_session_columns([40, 5], 16) == 1024 and default_session_columns([500], 16) == 2000
    assert default_session_columns([300], 7) % 7 == 0


# ------------------------------------------------------------------------------------------------ facade
def test_eligibility_predicate():
    from open_o3_video_amd.vllm_api import SamplingParams, continuous_eligible
    ok = dict(temperature=0.0, max_tokens=8, repetition_penalty=1.05, stop_token_ids=[3])
    assert continuous_eligible(SamplingParams(**ok))
    assert continuous_eligible(SamplingParams(**ok), "bf16") and not continuous_eligible(SamplingParams(**ok), "fp8")
    for kw in (dict(temperature=0.8), dict(n=2), dict(logprobs=1), dict(logprobs=0), dict(prompt_logprobs=1), dict(min_p=0.1),
               dict(presence_penalty=0.5), dict(frequency_penalty=-0.5), dict(min_tokens=2), dict(logit_bias={5: 1.0}),
               dict(allowed_token_ids=[1, 2, 3]), dict(bad_words=["x"]), dict(guided_decoding=dict(regex="a+")), dict(stop="END"),
               dict(stop=["a", "b"])):
        assert not continuous_eligible(SamplingParams(**{**ok, **kw})), kw


class _Tok:
    def encode(self, text, add_special_tokens=False):
        return [500 if w == "<|image_pad|>" else int(w) for w in text.split()]

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(i)) for i in ids)

    def convert_tokens_to_ids(self, tok):
        return {"<|image_pad|>": 500, "<|video_pad|>": 501}.get(tok, 0)


class _Engine:
    """Records what the facade calls: row b of a static call emits last prompt token + 1 + step, a continuous request likewise."""
    MAX_ROWS = 32

    def __init__(self, cfg):
        self.cfg, self.calls, self.ccalls, self.position_mode, self.dev, self.weights_version = cfg, [], [], "tf5", torch.device("cpu"), 0
        self.kv_cache_dtype = "bf16"

    def generate(self, input_ids, attention_mask=None, max_new_tokens=16, **kw):
        from open_o3_video_amd.engine import GenerateOutput
        ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.int64)
        self.calls.append(dict(kw, ids=ids.tolist()))
        gen = ids[:, -1:] + 1 + torch.arange(max_new_tokens)[None]
        return GenerateOutput(sequences=torch.cat([ids, gen], 1), margins=None, n_steps=max_new_tokens, timings={})

    def generate_continuous(self, requests, rows, **kw):
        from open_o3_video_amd.engine import ContinuousOutput
        self.ccalls.append(dict(kw, rows=rows, requests=requests))
        tm = dict(sessions=1, rows_refilled=len(requests) - rows, decode_forwards=17)
        out = []
        for r in requests:
            ids = torch.as_tensor(np.asarray(r["ids"]), dtype=torch.int64)
            toks = ids[-1] + 1 + torch.arange(r["max_new_tokens"])
            out.append(ContinuousOutput(tokens=toks, margins=None, row=0, t0=0, session=1, timings=tm, sequences=torch.cat([ids, toks])[None]))
        return out


def _llm(**kw):
    from open_o3_video_amd.config import O3VConfig
    from open_o3_video_amd.vllm_api import LLM
    eng = _Engine(O3VConfig.from_dict(fm.tiny_config()))
    llm = LLM(engine=eng, tokenizer=_Tok(), **kw)
    llm._frames = lambda mm: None if not mm else mm["image"]
    llm._visual_tokens = lambda fr: (torch.full((fr.shape[0], 4), float(fr[0, 0, 0, 0])), ("image", float(fr[0, 0, 0, 0])))
    llm.image_factor = 1
    return llm, eng


def _req(video, tail):
    return {"prompt": f"1 2 <|image_pad|> 3 {tail}", "multi_modal_data": {"image": torch.full((1, 3, 1, 1), float(video))}}


def test_facade_routes_eligible_calls_only():
    from open_o3_video_amd.vllm_api import SamplingParams
    reqs = [_req(i % 3, f"{10 + i} {20 + i}") for i in range(9)]
    sp = SamplingParams(temperature=0.0, max_tokens=3, repetition_penalty=1.05)
    llm, eng = _llm(continuous_batching=True, max_num_seqs=4)
    outs = llm.generate(reqs, sp)
    assert len(eng.ccalls) == 1 and not eng.calls
    c = eng.ccalls[0]
    assert c["rows"] == 4 and len(c["requests"]) == 9 and c["repetition_penalty"] == 1.05 and len(c["prefix_keys"]) == 9
    assert [r["max_new_tokens"] for r in c["requests"]] == [3] * 9 and c["requests"][4]["vis_embeds"].shape[0] == 1
    assert (llm.continuous_sessions, llm.rows_refilled, llm.decode_forwards) == (1, 5, 17)
    assert [o.request_id for o in outs] == [str(i) for i in range(9)]
    assert [o.outputs[0].token_ids for o in outs] == [[21 + i, 22 + i, 23 + i] for i in range(9)]
    # the static path gives the same outputs and ids; flag off, few requests, or an ineligible call: nothing is routed
    llm0, eng0 = _llm(max_num_seqs=4)
    outs0 = llm0.generate(reqs, sp)
    assert not eng0.ccalls and len(eng0.calls) == 3 and llm0.continuous_sessions == 0
    assert [(o.request_id, o.outputs[0].token_ids, o.prompt_token_ids) for o in outs0] == \
        [(o.request_id, o.outputs[0].token_ids, o.prompt_token_ids) for o in outs]
    llm1, eng1 = _llm(continuous_batching=True, max_num_seqs=4)
    llm1.generate(reqs[:4], sp)                                          # no more requests than rows
    llm1.generate(reqs, SamplingParams(temperature=0.8, max_tokens=3))
    llm1.generate(reqs, SamplingParams(temperature=0.0, max_tokens=3, stop="22"))
    assert not eng1.ccalls and (llm1.continuous_sessions, llm1.rows_refilled, llm1.decode_forwards) == (0, 0, 0)
    eng1.kv_cache_dtype = "fp8"
    llm1.generate(reqs, sp)
    assert not eng1.ccalls
    # request ids go on counting behind a routed call
    assert [o.request_id for o in llm.generate(reqs[:2], sp)] == ["9", "10"]


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_of_the_ragged_regime():
    lib = _lib.load()
    assert lib.o3v_abi_version() == 6
    assert hasattr(lib, "o3v_attn_decode_ragged") and len(_lib.SIGNATURES["o3v_attn_decode_ragged"]) == 18
    R, O = _lib.DecodeStateRagged, _lib.DecodeStateOwn
    assert issubclass(R, O) and [n for n, _ in R._fields_] == ["row_base", "kstage", "vstage"]
    own_end = O.own_lo.offset + 8
    assert (R.row_base.offset, R.kstage.offset, R.vstage.offset) == (own_end, own_end + 8, own_end + 16)
    assert ctypes.sizeof(R) == own_end + 24 and ctypes.sizeof(O) == own_end
    assert _lib.DECODE_RAGGED == 16
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    layer = _lib.LlmLayerW()
    desc = _lib.LlmDesc(hidden=64, layers=1, heads=8, kv_heads=2, head_dim=128, inter=64, vocab=32, layer=ctypes.pointer(layer))

    def state(**kw):
        st = R(B=4, S=0, Tmax=32, Tnew=64, nsplit=2, ws_bytes=0, flags=_lib.DECODE_RAGGED, row_base=p.value, kstage=p.value,
               vstage=p.value)
        for n in ("x", "kcache", "vcache", "cosT", "sinT", "logits", "seen", "cur_tok", "finished", "out_ids", "part_o", "part_ml",
                  "workspace", "sample_scratch"):
            setattr(st, n, p.value)
        for n, v in kw.items():
            setattr(st, n, v)
        return st

    def rc(st, step0=0, n=1):
        return lib.o3v_llm_decode_ex(ctypes.byref(desc), ctypes.byref(st), None, None, step0, n, 0, None)

    # a valid state gets as far as the workspace check (no launch: ws_bytes = 0); Tnew > Tmax is fine (rows guard themselves)
    assert rc(state()) == _lib.ERR_WORKSPACE and rc(state(), 40, 8) == _lib.ERR_WORKSPACE
    assert rc(state(S=100)) == _lib.ERR_WORKSPACE                                  # S is not read
    assert rc(state(row_base=None, Tnew=8)) == _lib.ERR_WORKSPACE                  # a zeroed set: the behaviour of before ...
    assert rc(state(row_base=None)) == _lib.ERR_ARG                                # ... whose S + Tnew must fit the cache
    assert rc(state(flags=0)) == _lib.ERR_ARG                                      # without the flag the three fields are not read
    for bad in (dict(kstage=None), dict(vstage=None), dict(group=2), dict(kprefix=p.value, vprefix=p.value), dict(own_past=3),
                dict(own_lo=p.value), dict(flags=_lib.DECODE_RAGGED | _lib.DECODE_KV8_EMULATE),
                dict(k8=p.value, v8=p.value, k8s=p.value, v8s=p.value)):
        assert rc(state(**bad)) == _lib.ERR_ARG, bad
    # the kernel entry: argument checks come before any launch
    f = lib.o3v_attn_decode_ragged
    a = lambda **kw: f(*[kw.get(k, d) for k, d in (("Q", p), ("Kc", p), ("Vc", p), ("Knew", p), ("Vnew", p), ("out", p), ("po", p),
                                                   ("pm", p), ("rb", p), ("step", 0), ("B", 2), ("Hq", 8), ("Hkv", 2), ("D", 128),
                                                   ("Tmax", 64), ("nsplit", 2), ("scale", 0.1), ("stream", None))])
    for name in ("Q", "Kc", "Vc", "Knew", "Vnew", "out", "po", "pm", "rb"):
        assert a(**{name: None}) == _lib.ERR_ARG, name
    assert a(Hkv=3) == _lib.ERR_ARG and a(nsplit=0) == _lib.ERR_ARG and a(nsplit=65) == _lib.ERR_ARG and a(nsplit=-65) == _lib.ERR_ARG
    assert a(Hq=18) == _lib.ERR_SHAPE and a(D=80) == _lib.ERR_SHAPE and a(D=256) == _lib.ERR_SHAPE
    assert a(B=0) == _lib.OK and a(B=0, D=32, nsplit=-64) == _lib.OK
