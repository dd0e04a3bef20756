"""Guided decoding, host side (open_o3_video_amd/guided.py): the regex compiler against `re.fullmatch`, pruning, the token table
against an oracle that never sees the compiler, token_bytes, check_no_dead_end, the façade's validation and the C struct.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from open_o3_video_amd import guided

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EVIDENCE = r"<obj>[^<]{1,6}</obj><box>\[\d\]</box>at<t>\d+\.?\d*</t>s"

# (pattern, 6-character alphabet, hand-picked longer strings)
PATTERNS = [
    (r"<answer>[ABCD]</answer>", "<a>ADE", ["<answer>A</answer>", "<answer>D</answer>", "<answer>E</answer>", "<answer>AB</answer>",
                                            "<answer>A</answer", "answer>A</answer>"]),
    (EVIDENCE, "<o>1.s", ["<obj>cat</obj><box>[3]</box>at<t>12.5</t>s", "<obj>a dog!</obj><box>[0]</box>at<t>7</t>s",
                          "<obj>toolong</obj><box>[3]</box>at<t>1</t>s", "<obj></obj><box>[3]</box>at<t>1</t>s",
                          "<obj>x</obj><box>[33]</box>at<t>1</t>s", "<obj>x</obj><box>[3]</box>at<t>.5</t>s",
                          "<obj>x</obj><box>[3]</box>at<t>1.</t>s", "<obj>x</obj><box>[3]</box>at<t>1.2.3</t>s"]),
    (r"<think>(.*?)</think>", "<th>/\n", ["<think>abc</think>", "<think></think>", "<think>a</think>b</think>", "<think>a\nb</think>"]),
    (r"[ABCD]", "ABCDEa", ["AB"]),
    (r"a*b+c?", "abcd \n", ["aaaaaaabbbbbbbc", "aaaaaaabbbbbbbcc"]),
    (r"(ab|c)*d", "abcd|e", ["ababcabccd", "ababcabacd"]),
    (r"[^<]{1,6}", "ab<> \n", ["abcdef", "abcdefg", "a\nb"]),
    (r"\d+\.?\d*", "01.9a-", ["3.14159265", "3..14", "1234567890."]),
    (r"(a(b|c){2,3})+", "abcd()", ["abcabbacbc", "abcabbbbacbc"]),
    (r"((a|b)(c|(d|e)f))+", "abcdef", ["acbdfaefbc", "acbdaefbc"]),
    (r".*", "a\n. éb", ["anything goes here", "but not\nnewlines"]),
    (r"a.c", "abc\n.é", ["a日c", "aéc", "a日日c"]),
    (r"[a-c]+?d", "abcde-", ["abcabcabcd", "abcabcabce"]),
    (r"(?:ab){2}", "ab(?:)", ["ababab"]),
    (r"a{2,}", "ab{2,}", ["aaaaaaaaaa"]),
    (r"x{,2}a", "xa{,2}", ["xxxa"]),
    (r"a{3}b{0}c", "abc{3}", ["aaabc"]),
    (r"^ab$", "ab^$ c", ["abab"]),
    (r"[\d<]+", "0<9a\\d", ["0<1<2<3<4<5"]),
    (r"\w+\s\W", "a_ \t-1", ["hello_World42 !", "hello world"]),
    (r"\D\S", "1a \n-é", ["é日"]),
    (r"a|", "a|b c\n", ["aa"]),
    (r"[]a]+", "]a[b^-", ["]a]a]a]a"]),
    (r"[a\-c]+", "a-cb\\d", ["a-c-a-c-"]),
    (r"\(a\)\.\*\\", "(a).*\\", ["(a).*\\\\"]),
    (r"a{", "a{}b1,", ["a{{"]),
    (r"[^\d\s]x", "1 ax\né", ["日x"]),
    (r"\n\t\r", "\n\t\rnt\\", []),
    (r"(?P<tag>ab)+c", "abc<>P", ["ababababc"]),
]


def _accepts(dfa, strings):
    """Acceptance of every string, walked with one numpy gather per byte position (independent of ByteDFA.walk)."""
    data = [s.encode() for s in strings]
    L = max(1, max(len(d) for d in data))
    mat = np.zeros((len(data), L), dtype=np.uint8)
    lens = np.array([len(d) for d in data])
    for i, d in enumerate(data):
        mat[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    trans = np.vstack([dfa.trans, np.full((1, 256), -1, dtype=np.int32)])
    q = np.zeros(len(data), dtype=np.int64)
    for j in range(L):
        q = np.where(j < lens, trans[q, mat[:, j]], q)
    return (q >= 0) & np.append(dfa.accepting, False)[q]


# ---------------------------------------------------------------------------------------------------------- 1. the compiler
@pytest.mark.parametrize("case", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_dfa_equals_re_fullmatch(case):
    pattern, alphabet, longer = case
    assert len(alphabet) == 6
    dfa = guided.compile_regex(pattern)
    assert dfa.trans.dtype == np.int32 and dfa.trans.shape == (dfa.n_states, 256) and dfa.accepting.dtype == bool
    strings = ["".join(t) for n in range(7) for t in itertools.product(alphabet, repeat=n)] + list(longer)
    want = np.array([re.fullmatch(pattern, s) is not None for s in strings])
    got = _accepts(dfa, strings)
    bad = np.flatnonzero(want != got)
    assert bad.size == 0, [(strings[i], bool(want[i])) for i in bad[:5]]
    assert want.any(), "the alphabet reaches no word of the language"
    for s in longer:
        assert dfa.fullmatch(s) == (re.fullmatch(pattern, s) is not None)


def test_multi_byte_code_points_are_one_unit():
    dot = guided.compile_regex(".")
    for ch in ("é", "日", "😀", "a", "\x7f", "\u0080", "߿", "ࠀ", "￿", "\U00010000", "\U0010ffff"):
        assert dot.fullmatch(ch), ch
    assert not dot.fullmatch("\n") and not dot.fullmatch("éé")
    for raw in (b"\xa9", b"\x80", b"\xc3", b"\xe6\x97", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xff"):
        assert not dot.fullmatch(raw), raw      # lone continuation / truncated / overlong / surrogate / past U+10FFFF
    neg = guided.compile_regex("[^a]b")
    assert neg.fullmatch("日b") and neg.fullmatch("éb") and not neg.fullmatch("ab") and not neg.fullmatch(b"\x97b")
    assert neg.fullmatch("\nb")                 # a negated class takes the newline, as in `re`
    lit = guided.compile_regex("[é日]+x")
    assert lit.fullmatch("é日éx") and not lit.fullmatch(b"\xc3x") and not lit.fullmatch("ex")
    rng = guided.compile_regex("[α-ω]")         # a range of two-byte code points
    assert rng.fullmatch("λ") and not rng.fullmatch("a") and not rng.fullmatch("Ω")
    assert re.fullmatch("[α-ω]", "λ") and not re.fullmatch("[α-ω]", "Ω")
    # ASCII-only classes (a documented difference from `re` on str)
    assert not guided.compile_regex(r"\d").fullmatch("٣") and not guided.compile_regex(r"\w").fullmatch("é")
    assert guided.compile_regex(r"\W").fullmatch("é") and guided.compile_regex(r"\D").fullmatch("٣")


@pytest.mark.parametrize("pattern,construct", [
    (r"(a)\1", "back-reference"), (r"(?P<x>a)(?P=x)", "back-reference"), (r"(?=a)a", "look-around"), (r"(?!a)b", "look-around"),
    (r"(?<=a)b", "look-around"), (r"(?<!a)b", "look-around"), (r"(?i)a", "inline flags"), (r"(?s:a)", "inline flags"),
    (r"a^b", "anchor"), (r"a$b", "anchor"), (r"\bword", r"\b"), (r"\Aab", r"\A"), (r"a\Z", r"\Z"), (r"a**", "multiple repeat"),
    (r"*a", "nothing to repeat"), (r"(a", "unterminated"), (r"a)", "unbalanced"), (r"[a", "unterminated"), (r"a++", "possessive"),
    (r"a{3,2}", "min repeat"), (r"[z-a]", "bad character range"), ("a\\", "bad escape"),
])
def test_unsupported_constructs_are_named(pattern, construct):
    with pytest.raises(ValueError) as e:
        guided.compile_regex(pattern)
    assert construct in str(e.value)


def test_state_limit_and_empty_language():
    with pytest.raises(ValueError) as e:
        guided.compile_regex(r"(a|b)*a(a|b){12}")       # 2^13 subsets
    assert "2048" in str(e.value)
    empty = "[^" + chr(0) + "-" + chr(0x10FFFF) + "]"
    assert re.fullmatch(empty, "a") is None
    with pytest.raises(ValueError) as e:
        guided.compile_regex("a" + empty)
    assert "matches nothing" in str(e.value)


# ---------------------------------------------------------------------------------------------------------- 2. pruning
def _coreachable(dfa):
    live = dfa.accepting.copy()
    for _ in range(dfa.n_states):
        live = live | np.where(dfa.trans >= 0, live[np.maximum(dfa.trans, 0)], False).any(axis=1)
    return live


def test_no_state_without_a_path_to_acceptance():
    empty = "[^" + chr(0) + "-" + chr(0x10FFFF) + "]"
    cases = [p[0] for p in PATTERNS] + ["a" + empty + "|b", "(x" + empty + "y|xz)w"]
    for pattern in cases:
        dfa = guided.compile_regex(pattern)
        reach, stack = {0}, [0]
        while stack:
            for t in np.unique(dfa.trans[stack.pop()]):
                if t >= 0 and int(t) not in reach:
                    reach.add(int(t))
                    stack.append(int(t))
        assert reach == set(range(dfa.n_states)), pattern          # no unreachable state is kept either
        assert _coreachable(dfa).all(), pattern
        assert int(dfa.trans.max()) < dfa.n_states and int(dfa.trans.min()) >= -1
    d = guided.compile_regex("a" + empty + "|b")
    assert d.n_states == 2 and d.trans[0, ord("a")] == -1 and d.trans[0, ord("b")] == 1      # the dead branch's in-edge is gone
    assert d.fullmatch("b") and not d.fullmatch("a")


# ---------------------------------------------------------------------------------------------------------- 3. the token table
EOS = (298, 301)


def _vocabulary():
    """~300 tokens: every printable ASCII byte, merges (some straddling two pattern elements), fillers, two None tokens, two EOS ids."""
    toks = [bytes([b]) for b in range(32, 127)]
    toks += [s.encode() for s in ("<ans", "wer>", "</", "AB", "r>A", "r>E", "D</answer", "<answer>", "answer>", "</answer>", "A<", "B</a", "yes", "no",
                                  "unc", "lear", "ye", "s", "nou", "uncl", "o", "<t>", "</t>", "t>1", "2.", ".5", "5</", "12", "123", "1.", ">s", "BA",
                                  "ABx", "Bx", "AAA", "ab", "bc", "abc", "bcd", "ac", "cd", "é", "日")]
    toks += ["é".encode()[:1], "日".encode()[1:]]       # halves of multi-byte characters
    i = 0
    while len(toks) < 296:
        toks.append(f"~f{i}".encode())
        i += 1
    toks = list(toks)
    toks[290] = None
    toks[295] = None
    V = 302
    toks += [None] * (V - len(toks))
    toks[EOS[0]] = b"<eos>"      # EOS ids carry text: the table must still treat them as EOS only
    toks[EOS[1]] = None
    return toks, V


def _language(pattern, candidates):
    return sorted(c for c in candidates if re.fullmatch(pattern, c) is not None)


FINITE = [
    (r"<answer>[ABCD]</answer>", ["<answer>" + c + "</answer>" for c in "ABCDEa<"] + ["<answer></answer>", "<answer>AB</answer>"]),
    (r"(yes|no|unclear)", ["yes", "no", "unclear", "ye", "nou", "yesno", "unc", "", "n"]),
    (r"<t>[125]{1,2}\.?5?</t>", ["<t>" + "".join(p) + "</t>" for n in range(5) for p in itertools.product("125.", repeat=n)]),
    (r"[AB]{2,3}x?", ["".join(p) for n in range(6) for p in itertools.product("ABx", repeat=n)]),
    (r"(ab|a)(c|bcd)?", ["".join(p) for n in range(7) for p in itertools.product("abcd", repeat=n)]),
    (r"[é日]A?", ["é", "日", "éA", "日A", "A", "é日", "e"]),
]


@pytest.mark.parametrize("pattern,candidates", FINITE, ids=[f[0] for f in FINITE])
def test_token_table_against_the_prefix_oracle(pattern, candidates):
    toks, V = _vocabulary()
    L = [w.encode() for w in _language(pattern, candidates)]
    assert len(L) >= 2 and len(L) < len(candidates)
    dfa = guided.compile_regex(pattern)
    table = guided.token_table(dfa, toks, EOS, V)
    ldn = (V + 7) // 8 * 8
    assert table.dtype == np.int16 and table.shape == (dfa.n_states, ldn) and ldn == 304
    assert (table[:, V:] == -1).all() and int(table.max()) < dfa.n_states and int(table.min()) == -1
    # walk every text that tokens can spell and that is a prefix of a word: the allowed set at each step is the oracle's
    state_of, frontier, steps = {b"": 0}, [b""], 0
    while frontier:
        x = frontier.pop()
        q = state_of[x]
        allowed = set(np.flatnonzero(table[q, :V] >= 0).tolist())
        want = {t for t, tb in enumerate(toks) if tb is not None and t not in EOS and any(w.startswith(x + tb) for w in L)}
        if x in L:
            want |= set(EOS)
            assert all(table[q, e] == q for e in EOS)       # EOS keeps the state
        assert allowed == want, (x, sorted(allowed ^ want))
        steps += 1
        for t in allowed - set(EOS):
            y, n = x + toks[t], int(table[q, t])
            if y in state_of:
                assert state_of[y] == n, y                  # the state depends on the text, not on how it was tokenised
            else:
                state_of[y] = n
                frontier.append(y)
    assert set(L) <= set(state_of), "every word can be spelled from the vocabulary"
    assert steps == len(state_of) >= len(L)


def test_token_table_limits_and_short_vocabulary():
    dfa = guided.compile_regex("ab")
    t = guided.token_table(dfa, [b"a", b"b", b"ab"], [], 9)         # a vocabulary list shorter than V: the rest is never allowed
    assert t.shape == (3, 16) and t[0, :3].tolist() == [1, -1, 2] and (t[:, 3:] == -1).all()
    big = guided.ByteDFA(trans=np.full((40000, 256), -1, dtype=np.int32), accepting=np.ones(40000, dtype=bool))
    with pytest.raises(ValueError) as e:
        guided.token_table(big, [b"a"], [], 1)
    assert "32767" in str(e.value)
    wide = guided.ByteDFA(trans=np.full((2000, 256), -1, dtype=np.int32), accepting=np.ones(2000, dtype=bool))
    with pytest.raises(ValueError) as e:
        guided.token_table(wide, [b"a"], [], 152064)
    assert "512" in str(e.value)


# ---------------------------------------------------------------------------------------------------------- 4. token_bytes
def _bytes_to_unicode():
    """GPT-2's table, written out independently of guided.py (openai/gpt-2 encoder.py)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(2 ** 8):
        if b not in bs:
            bs.append(b)
            cs.append(2 ** 8 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


class _ByteLevelStub:
    """A byte-level BPE tokenizer as transformers exposes Qwen's: tokens spelled in the GPT-2 alphabet, specials added on top."""

    def __init__(self):
        b2u = _bytes_to_unicode()
        spell = lambda raw: "".join(b2u[b] for b in raw)
        self.raw = [b"a", b" the", "é".encode(), "日".encode()[:2], "日".encode()[2:], b"\n\n", b"<", b"answer", bytes([0xFF]), b""]
        self.tokens = [spell(r) for r in self.raw] + ["<|im_end|>", "<|endoftext|>"]
        self.all_special_ids = [11]

    def get_added_vocab(self):
        return {"<|im_end|>": 10, "<|endoftext|>": 11}

    def convert_ids_to_tokens(self, i):
        return self.tokens[i] if i < len(self.tokens) else None

    def decode(self, ids):
        raise AssertionError("a byte-level vocabulary is never decoded token by token")


class _PlainStub:
    all_special_ids = [3]

    def decode(self, ids):
        return ["hello", " world", "", "<eos>", "�", "é"][ids[0]] if ids[0] < 6 else ""


def test_token_bytes():
    st = _ByteLevelStub()
    got = guided.token_bytes(st, 15)
    assert got[:9] == st.raw[:9]
    assert got[1] == b" the" and got[3] == b"\xe6\x97" and got[4] == b"\xa5" and got[8] == b"\xff"     # half characters keep their bytes
    assert got[9] is None                        # the empty string
    assert got[10] is None and got[11] is None   # added / special tokens
    assert got[12:] == [None, None, None]        # ids the tokenizer does not know
    plain = guided.token_bytes(_PlainStub(), 8)
    assert plain == [b"hello", b" world", None, None, None, "é".encode(), None, None]


# ---------------------------------------------------------------------------------------------------------- 5. dead ends
def test_check_no_dead_end():
    toks, V = _vocabulary()
    dfa = guided.compile_regex(r"<answer>[AB]</answer>")
    table = guided.token_table(dfa, toks, EOS, V)
    guided.check_no_dead_end(table, None, 0)
    harmless = np.zeros(V, dtype=np.float32)
    harmless[toks.index(b"~f0")] = -np.inf          # never allowed anyway
    harmless[toks.index(b"<ans")] = -np.inf         # the single bytes still spell it
    harmless[toks.index(b"A")] = 2.5
    guided.check_no_dead_end(table, harmless, 0)
    ban = np.zeros(V, dtype=np.float32)
    for t, tb in enumerate(toks):
        if tb is not None and b"/" in tb:           # nothing can spell the closing tag's "/": the state behind its "<" is a dead end
            ban[t] = -np.inf
    with pytest.raises(ValueError) as e:
        guided.check_no_dead_end(table, ban, 0)
    q = dfa.walk(b"<answer>A<")
    assert f"state {q} " in str(e.value)
    # without an EOS id the accepting state has no token
    with pytest.raises(ValueError) as e:
        guided.check_no_dead_end(guided.token_table(dfa, toks, [], V), None, 0)
    assert f"state {dfa.walk(b'<answer>A</answer>')} " in str(e.value)
    # a start state that is not 0: only what is reachable from it counts
    guided.check_no_dead_end(table, ban, dfa.walk(b"<answer>A</"))
    with pytest.raises(ValueError):
        guided.check_no_dead_end(table, None, dfa.n_states)


def test_choice_regex():
    pat = guided.choice_regex(["yes", "no (maybe)", "a|b", "1.5"])
    for c in ("yes", "no (maybe)", "a|b", "1.5"):
        assert re.fullmatch(pat, c) and guided.compile_regex(pat).fullmatch(c)
    d = guided.compile_regex(pat)
    assert not d.fullmatch("a") and not d.fullmatch("1x5") and not d.fullmatch("yesno")
    for bad in ([], [""], ["a", ""], None, ["a", 3], "abc"):
        with pytest.raises(ValueError):
            guided.choice_regex(bad)


# ---------------------------------------------------------------------------------------------------------- 6. the façade's arguments
def test_sampling_params_guided_decoding():
    from open_o3_video_amd.vllm_api import GuidedDecodingParams, SamplingParams
    sp = SamplingParams(guided_decoding={"regex": "[ABCD]"})
    assert isinstance(sp.guided_decoding, GuidedDecodingParams) and sp.guided_decoding.pattern == "[ABCD]"
    sp2 = SamplingParams(guided_decoding=GuidedDecodingParams(choice=["yes", "no"], backend="outlines", whitespace_pattern=r"\s"))
    assert re.fullmatch(sp2.guided_decoding.pattern, "no") and not re.fullmatch(sp2.guided_decoding.pattern, "yesno")
    assert SamplingParams(guided_decoding={"regex": "[ABCD]"}) == sp and sp != sp2        # requests group by equal parameters
    assert SamplingParams().guided_decoding is None
    for key, val in (("json", {}), ("json", {"type": "object"}), ("grammar", "root ::= 'a'"), ("json_object", True)):
        for form in ({key: val}, {key: val, "regex": "a"}):
            with pytest.raises(ValueError) as e:
                SamplingParams(guided_decoding=form)
            assert "guided_decoding" in str(e.value) and key in str(e.value)
        with pytest.raises(ValueError) as e:
            GuidedDecodingParams(**{key: val})
        assert key in str(e.value)
    for bad in ({}, {"regex": "a", "choice": ["a"]}, {"choice": []}, {"choice": ["a", ""]}, {"regex": ""}, {"backend": "outlines"},
                {"regexp": "a"}, "[ABCD]", ["a"]):
        with pytest.raises(ValueError) as e:
            SamplingParams(guided_decoding=bad)
        assert "guided_decoding" in str(e.value) or "choice" in str(e.value)
    with pytest.raises(ValueError):
        SamplingParams(guided_decoding={"regex": "a"}, min_tokens=2, max_tokens=8)
    for kw in (dict(best_of=2), dict(logits_processors=[print]), dict(truncate_prompt_tokens=5)):      # still refused by name
        with pytest.raises(ValueError) as e:
            SamplingParams(**kw)
        assert next(iter(kw)) in str(e.value)


# ---------------------------------------------------------------------------------------------------------- 7. C ABI
def test_c_abi_guided_struct_and_entries():
    from open_o3_video_amd import _lib
    G = _lib.GuidedOpts
    hdr = open(os.path.join(ROOT, "include", "o3v.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} o3v_guided_opts;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["const int16_t* next", "int n_states, ldn", "int* state"]
    # LP64 layout of those declarations: pointer 8, two ints 4 + 4, pointer 8
    assert [n for n, _ in G._fields_] == ["next", "n_states", "ldn", "state"]
    assert (G.next.offset, G.n_states.offset, G.ldn.offset, G.state.offset) == (0, 8, 12, 16) and ctypes.sizeof(G) == 24
    assert ctypes.sizeof(_lib.SamplingOpts) == 40       # untouched
    for name in ("o3v_sample_step_guided", "o3v_llm_decode_guided"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    lib = _lib.load()
    assert lib.o3v_abi_version() == 6
    fake = ctypes.c_void_p(0x1000)

    def step(go, so=None, V=100):
        return lib.o3v_sample_step_guided(fake, fake, fake, fake, fake, None, fake, 1, 0, 2, V, V, 1, 1.0, 1.0, 0, 1.0, 0, None, 0, 4,
                                          fake, None, so, go, None)

    ok = dict(next=0x2000, n_states=3, ldn=104, state=0x3000)
    bad = [dict(ok, next=0), dict(ok, state=0), dict(ok, next=0x2008), dict(ok, state=0x3002), dict(ok, n_states=0), dict(ok, n_states=-1),
           dict(ok, n_states=40000), dict(ok, ldn=96), dict(ok, ldn=101), dict(ok, ldn=0)]
    for kw in bad:
        go = G(**kw)
        assert step(ctypes.byref(go)) == _lib.ERR_ARG, kw
        assert step(ctypes.byref(go), ctypes.byref(_lib.SamplingOpts())) == _lib.ERR_ARG, kw
        assert lib.o3v_llm_decode_guided(None, None, None, None, ctypes.byref(go), 0, 1, 0, None) == _lib.ERR_ARG
    assert step(ctypes.byref(G(**ok)), ctypes.byref(_lib.SamplingOpts(min_p=2.0))) == _lib.ERR_ARG     # `so` is checked as before
    assert step(None, None) == _lib.ERR_ARG                 # go == NULL is o3v_sample_step_ex, which needs its options
    assert lib.o3v_llm_decode_guided(None, None, None, None, ctypes.byref(G(**ok)), 0, 1, 0, None) == _lib.ERR_ARG    # no model
