"""Guided decoding, host side: a regular expression (or a list of choices) -> byte-level DFA -> token-level automaton.

vLLM 0.7.2 `SamplingParams(guided_decoding=GuidedDecodingParams(regex= | choice=))` (outlines' RegexGuide: an FSM over the
tokenizer's vocabulary whose allowed-token set masks the logits, EOS allowed only in a final state).  The decode loop enqueues
chunks of steps without seeing a token, so the automaton runs on the GPU (o3v_guided_opts in include/o3v.h): this module only
builds its table, `next[q][t]` i16 = state after token t in state q, -1 = not allowed.  Pure Python + numpy.

Semantics: Python `re.fullmatch` without flags, except that `\\d \\w \\s` are ASCII only, the pattern is taken as UTF-8, and `.` and
negated classes match exactly one well-formed UTF-8 code point (never a lone byte of one).  Lazy quantifiers are accepted (they
define the same language).  Back-references, look-around, inline flags and anchors inside the pattern are refused by name.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

MAX_DFA_STATES = 2048
MAX_NFA_STATES = 200_000
MAX_TABLE_STATES = 32767              # next-state entries are i16
MAX_TABLE_BYTES = 512 << 20
MAX_CP = 0x10FFFF

_DIGIT = [(0x30, 0x39)]
_WORD = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_SPACE = [(0x09, 0x0D), (0x20, 0x20)]   # " \t\n\r\f\v"
_ESC_LIT = {"n": "\n", "t": "\t", "r": "\r", "f": "\f", "v": "\v"}


@dataclass
class ByteDFA:
    trans: np.ndarray       # i32 [n, 256], -1 = no edge
    accepting: np.ndarray   # bool [n]; the start state is 0

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    def walk(self, data: bytes, q: int = 0) -> int:
        """State after `data` from q, -1 once a byte has no edge."""
        for b in data:
            q = int(self.trans[q, b])
            if q < 0:
                return -1
        return q

    def fullmatch(self, data) -> bool:
        q = self.walk(data.encode() if isinstance(data, str) else bytes(data))
        return q >= 0 and bool(self.accepting[q])


# ------------------------------------------------------------------------------------------------ code point sets
def _norm(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def _negate(ranges):
    out, at = [], 0
    for lo, hi in _norm(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= MAX_CP:
        out.append((at, MAX_CP))
    return out


def _utf8_sequences(lo: int, hi: int):
    """The code points lo..hi as sequences of byte ranges [(b_lo, b_hi), ...], one sequence per shape of well-formed UTF-8
    (no surrogates, no overlong forms: every range is cut at the encoding-length and continuation-byte boundaries)."""
    if lo > hi:
        return
    if lo <= 0xDFFF and hi >= 0xD800:          # surrogates are not encodable
        yield from _utf8_sequences(lo, 0xD7FF)
        yield from _utf8_sequences(max(lo, 0xE000), hi)
        return
    for top in (0x7F, 0x7FF, 0xFFFF):
        if lo <= top < hi:
            yield from _utf8_sequences(lo, top)
            yield from _utf8_sequences(top + 1, hi)
            return
    if hi < 0x80:
        yield [(lo, hi)]
        return
    for i in (1, 2, 3):
        m = (1 << (6 * i)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                yield from _utf8_sequences(lo, lo | m)
                yield from _utf8_sequences((lo | m) + 1, hi)
                return
            if (hi & m) != m:
                yield from _utf8_sequences(lo, (hi & ~m) - 1)
                yield from _utf8_sequences(hi & ~m, hi)
                return
    yield list(zip(chr(lo).encode(), chr(hi).encode()))


# ------------------------------------------------------------------------------------------------ parser -> AST
# nodes: ("set", ranges) one code point of the set; ("cat", [nodes]); ("alt", [nodes]); ("rep", node, m, n or None)
class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("the pattern must be a str")
        self.p, self.i = pattern, 0
        if self.p.startswith("^"):
            self.i = 1
        self.end = len(self.p)
        if self.p.endswith("$") and not self._escaped_at(len(self.p) - 1) and self.end > self.i:
            self.end -= 1

    def _escaped_at(self, k: int) -> bool:
        n = 0
        while k - 1 - n >= 0 and self.p[k - 1 - n] == "\\":
            n += 1
        return n % 2 == 1

    def peek(self) -> Optional[str]:
        return self.p[self.i] if self.i < self.end else None

    def take(self) -> str:
        c = self.p[self.i]
        self.i += 1
        return c

    def parse(self):
        node = self.alt()
        if self.i < self.end:
            raise ValueError(f"unbalanced parenthesis ')' at position {self.i}")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.take()
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            atom = self.atom()
            items.append(self.quantified(atom))
        return ("cat", items)

    def quantified(self, atom):
        c = self.peek()
        m = n = None
        if c == "*":
            m, n = 0, None
        elif c == "+":
            m, n = 1, None
        elif c == "?":
            m, n = 0, 1
        elif c == "{":
            g = re.compile(r"\{(\d*)(?:(,)(\d*))?\}").match(self.p, self.i, self.end)
            if g is None or g.group(0) == "{}":
                return atom          # a literal brace, as in `re`
            m = int(g.group(1) or 0)
            n = m if g.group(2) is None else (int(g.group(3)) if g.group(3) else None)
            if n is not None and n < m:
                raise ValueError(f"quantifier {g.group(0)}: min repeat greater than max repeat")
            self.i = g.end() - 1
        else:
            return atom
        self.take()
        if self.peek() == "?":       # lazy: the same language
            self.take()
        elif self.peek() == "+":
            raise ValueError("possessive quantifier is not supported")
        if self.peek() is not None and self.peek() in "*+?":
            raise ValueError(f"multiple repeat at position {self.i}")
        return ("rep", atom, m, n)

    def atom(self):
        c = self.take()
        if c == "(":
            if self.peek() == "?":
                self.take()
                k = self.peek()
                if k == ":":
                    self.take()
                elif k in ("=", "!"):
                    raise ValueError("look-around (?= / (?! is not supported")
                elif k == "<" and self.p[self.i + 1:self.i + 2] in ("=", "!"):
                    raise ValueError("look-around (?<= / (?<! is not supported")
                elif k == "P" and self.p[self.i + 1:self.i + 2] == "=":
                    raise ValueError("back-reference (?P=name) is not supported")
                elif k == "P" and self.p[self.i + 1:self.i + 2] == "<":
                    close = self.p.find(">", self.i)
                    if close < 0 or close >= self.end:
                        raise ValueError("unterminated group name")
                    self.i = close + 1
                else:
                    raise ValueError(f"inline flags / group extension (?{k or ''} is not supported")
            node = self.alt()
            if self.peek() != ")":
                raise ValueError("missing ), unterminated group")
            self.take()
            return node
        if c == "[":
            return ("set", self.char_class())
        if c == ".":
            return ("set", _negate([(10, 10)]))
        if c == "\\":
            kind, val = self.escape(in_class=False)
            return ("set", val) if kind == "set" else ("set", [(ord(val), ord(val))])
        if c in "*+?":
            raise ValueError(f"nothing to repeat at position {self.i - 1}")
        if c in "^$":
            raise ValueError(f"anchor {c!r} inside the pattern is not supported (matching is full-match)")
        return ("set", [(ord(c), ord(c))])

    def escape(self, in_class: bool):
        if self.i >= self.end:
            raise ValueError("bad escape (end of pattern)")
        c = self.take()
        sets = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
        if c in sets:
            return "set", list(sets[c])
        if c.lower() in sets and c.isupper():
            return "set", _negate(sets[c.lower()])
        if c in _ESC_LIT:
            return "lit", _ESC_LIT[c]
        if c.isdigit() and c != "0":
            raise ValueError(f"back-reference \\{c} is not supported")
        if c.isascii() and (c.isalnum()):
            raise ValueError(f"escape \\{c} is not supported")
        return "lit", c          # an escaped metacharacter (or any other non-alphanumeric character)

    def char_class(self):
        neg = self.peek() == "^"
        if neg:
            self.take()
        ranges, first = [], True
        while True:
            if self.i >= self.end:
                raise ValueError("unterminated character set")
            c = self.take()
            if c == "]" and not first:
                break
            first = False
            if c == "\\":
                kind, val = self.escape(in_class=True)
                if kind == "set":
                    ranges += val
                    continue
                c = val
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.take()
                d = self.take()
                if d == "\\":
                    kind, d = self.escape(in_class=True)
                    if kind == "set":
                        raise ValueError("bad character range: a class escape cannot end a range")
                if ord(d) < ord(c):
                    raise ValueError(f"bad character range {c}-{d}")
                ranges.append((ord(c), ord(d)))
            else:
                ranges.append((ord(c), ord(c)))
        ranges = _norm(ranges)
        return _negate(ranges) if neg else ranges


# ------------------------------------------------------------------------------------------------ Thompson NFA
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[tuple]] = []     # per state: (byte lo, byte hi, target)

    def new(self) -> int:
        if len(self.eps) >= MAX_NFA_STATES:
            raise ValueError(f"the pattern needs more than {MAX_NFA_STATES} NFA states")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """-> (start, end) of the fragment of `node`."""
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            for lo, hi in node[1]:
                for seq in _utf8_sequences(lo, hi):
                    at = s
                    for j, (blo, bhi) in enumerate(seq):
                        to = e if j == len(seq) - 1 else self.new()
                        self.edges[at].append((blo, bhi, to))
                        at = to
            return s, e
        if kind == "cat":
            s = e = self.new()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.new(), self.new()
            for br in node[1]:
                a, b = self.build(br)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, m, n = node
        s = e = self.new()
        for _ in range(m):
            a, b = self.build(sub)
            self.eps[e].append(a)
            e = b
        if n is None:                      # sub*
            a, b = self.build(sub)
            hub = self.new()
            self.eps[e].append(hub)
            self.eps[hub].append(a)
            self.eps[b].append(hub)
            e = hub
        else:                              # up to n - m more, each one skippable to the end
            end = self.new()
            for _ in range(n - m):
                a, b = self.build(sub)
                self.eps[e].append(end)
                self.eps[e].append(a)
                e = b
            self.eps[e].append(end)
            e = end
        return s, e


def _closure(nfa: _NFA, states) -> frozenset:
    seen, stack = set(states), list(states)
    while stack:
        for t in nfa.eps[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    return frozenset(seen)


def compile_regex(pattern: str) -> ByteDFA:
    """Pattern -> minimal byte DFA without dead ends: Thompson construction, subset construction over bytes, pruning of every state
    that cannot reach an accepting one (the model can never be steered into a dead end), Moore minimisation (the token table costs
    2 * vocabulary bytes per state).  ValueError names any construct outside the supported subset (module docstring)."""
    nfa = _NFA()
    start, end = nfa.build(_Parser(pattern).parse())
    s0 = _closure(nfa, [start])
    index, order, rows = {s0: 0}, [s0], []
    memo = {}
    while len(rows) < len(order):
        cover = [[] for _ in range(256)]
        for q in order[len(rows)]:
            for lo, hi, to in nfa.edges[q]:
                for b in range(lo, hi + 1):
                    cover[b].append(to)
        row = np.full(256, -1, dtype=np.int32)
        for b in range(256):
            if not cover[b]:
                continue
            key = tuple(sorted(set(cover[b])))
            tgt = memo.get(key)
            if tgt is None:
                tgt = memo[key] = _closure(nfa, key)
            j = index.get(tgt)
            if j is None:
                if len(order) >= MAX_DFA_STATES:
                    raise ValueError(f"the pattern needs more than {MAX_DFA_STATES} DFA states")
                j = index[tgt] = len(order)
                order.append(tgt)
            row[b] = j
        rows.append(row)
    trans = np.stack(rows)
    accepting = np.array([end in s for s in order], dtype=bool)
    # prune: keep the states from which an accepting state is reachable
    n = trans.shape[0]
    live = accepting.copy()
    while True:
        grown = live | (np.where(trans >= 0, live[np.maximum(trans, 0)], False)).any(axis=1)
        if (grown == live).all():
            break
        live = grown
    if not live[0]:
        raise ValueError("the pattern matches nothing")
    trans = np.where((trans >= 0) & live[np.maximum(trans, 0)], trans, -1)
    # minimise (Moore): refine {accepting, not} by the classes of the 256 successors
    part = accepting.astype(np.int64)
    part[~live] = 2
    while True:
        sig = np.concatenate([part[:, None], np.where(trans >= 0, part[np.maximum(trans, 0)], -1)], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        if len(np.unique(new)) == len(np.unique(part)):
            break
        part = new
    # renumber: classes of live states in order of first appearance, so that the start state stays 0
    rename, reps = {}, []
    for q in range(n):
        if live[q] and int(part[q]) not in rename:
            rename[int(part[q])] = len(reps)
            reps.append(q)
    cls = np.array([rename.get(int(part[q]), -1) for q in range(n)], dtype=np.int32)
    out = np.where(trans[reps] >= 0, cls[np.maximum(trans[reps], 0)], -1).astype(np.int32)
    return ByteDFA(trans=np.ascontiguousarray(out), accepting=accepting[reps].copy())


def choice_regex(choices: Sequence[str]) -> str:
    """The alternation of the escaped choices (vLLM: guided_decoding.choice)."""
    choices = list(choices) if isinstance(choices, (list, tuple)) else None
    if not choices or any(not isinstance(c, str) or not c for c in choices):
        raise ValueError("choice must be a non-empty list of non-empty strings")
    return "(" + "|".join(re.escape(c) for c in choices) + ")"


# ------------------------------------------------------------------------------------------------ vocabulary
def _gpt2_unicode_to_byte() -> dict:
    """Inverse of GPT-2's bytes_to_unicode: the printable characters the byte-level BPE vocabularies spell their bytes with."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def token_bytes(tokenizer, V: int) -> List[Optional[bytes]]:
    """The byte string of each token id 0..V-1; None = never allowed under a guide (special and added tokens, ids the tokenizer does
    not know, empty strings, and -- on the `decode` route -- tokens whose text is not valid on its own).
    Byte-level BPE tokenizers (Qwen's; whatever spells every token in GPT-2's bytes_to_unicode alphabet) are decoded from
    `convert_ids_to_tokens`, so a token that is half of a multi-byte character keeps its exact bytes; any other tokenizer goes
    through `decode([i]).encode()`."""
    special = set(int(i) for i in (getattr(tokenizer, "all_special_ids", None) or ()))
    added = getattr(tokenizer, "get_added_vocab", None)
    if callable(added):
        special |= set(int(i) for i in added().values())
    toks = None
    conv = getattr(tokenizer, "convert_ids_to_tokens", None)
    if callable(conv):
        toks = []
        for i in range(V):
            try:
                t = conv(i)
            except (IndexError, KeyError, OverflowError, ValueError):
                t = None
            toks.append(t if isinstance(t, str) else None)
        u2b = _gpt2_unicode_to_byte()
        if not all(c in u2b for i, t in enumerate(toks) if t is not None and i not in special for c in t):
            toks = None     # not a byte-level alphabet
    out: List[Optional[bytes]] = []
    for i in range(V):
        if i in special:
            out.append(None)
        elif toks is not None:
            out.append(bytes(u2b[c] for c in toks[i]) if toks[i] else None)
        else:
            try:
                text = tokenizer.decode([i])
            except (IndexError, KeyError, OverflowError, ValueError):
                text = None
            out.append(text.encode() if text and "\ufffd" not in text else None)
    return out


def token_table(dfa: ByteDFA, tok_bytes: Sequence[Optional[bytes]], eos_ids: Sequence[int], V: int) -> np.ndarray:
    """i16 [n_states, ldn], ldn = V rounded up to a multiple of 8: next[q][t] = the state after walking token t's bytes from q, -1
    if a byte has no edge (or the token is None, or t >= V).  next[q][e] = q for every EOS id e when q is accepting, else -1: a
    completion may end only where the pattern is matched.
    Vectorised over the vocabulary: one gather per byte position over the tokens that are that long, 64 states at a time.  The
    7B model's vocabulary (152064 ids, tokens of 1..8 bytes) against the 86-state automaton of the evidence-span pattern takes
    about 0.9 s on one CPU core, 10 ms per state."""
    n = dfa.n_states
    V = int(V)
    ldn = (V + 7) // 8 * 8
    if n > MAX_TABLE_STATES:
        raise ValueError(f"{n} states do not fit the 16-bit table (at most {MAX_TABLE_STATES})")
    if n * ldn * 2 > MAX_TABLE_BYTES:
        raise ValueError(f"the token table would take {n * ldn * 2 >> 20} MiB (at most {MAX_TABLE_BYTES >> 20}): simplify the pattern")
    if len(tok_bytes) < V:
        tok_bytes = list(tok_bytes) + [None] * (V - len(tok_bytes))
    lens = np.array([len(t) if t else 0 for t in tok_bytes[:V]], dtype=np.int64)
    order = np.argsort(-lens, kind="stable")          # longest first: byte position j concerns a leading run of tokens
    lens_sorted = lens[order]
    Lmax = int(lens_sorted[0]) if V else 0
    data = np.zeros((V, max(Lmax, 1)), dtype=np.uint8)
    for row, t in enumerate(order):
        if lens_sorted[row] == 0:
            break
        data[row, :lens_sorted[row]] = np.frombuffer(tok_bytes[t], dtype=np.uint8)
    trans = np.vstack([dfa.trans, np.full((1, 256), -1, dtype=np.int32)])      # row -1: the sink
    table = np.full((n, ldn), -1, dtype=np.int16)
    n_real = int((lens_sorted > 0).sum())
    for q0 in range(0, n, 64):
        q1 = min(n, q0 + 64)
        cur = np.repeat(np.arange(q0, q1, dtype=np.int32)[:, None], n_real, axis=1)
        for j in range(Lmax):
            k = int((lens_sorted > j).sum())
            cur[:, :k] = trans[cur[:, :k], data[None, :k, j]]
        table[q0:q1, order[:n_real]] = cur.astype(np.int16)
    acc = np.flatnonzero(dfa.accepting)
    for e in eos_ids:
        if 0 <= int(e) < V:
            table[:, int(e)] = -1
            table[acc, int(e)] = acc.astype(np.int16)
    return table


def check_no_dead_end(table: np.ndarray, bias: Optional[np.ndarray], start: int = 0) -> None:
    """Every state reachable from `start` through tokens with next >= 0 and a finite static bias must itself have such a token:
    what keeps an all -inf row from ever reaching the sampler.  ValueError names the first state that has none."""
    n, ldn = table.shape
    ok = np.ones(ldn, dtype=bool)
    if bias is not None:
        b = np.asarray(bias)
        ok[:] = False
        ok[:min(ldn, b.shape[0])] = np.isfinite(b[:ldn])
    if not 0 <= int(start) < n:
        raise ValueError(f"start state {start} outside the table ({n} states)")
    seen, stack = {int(start)}, [int(start)]
    while stack:
        q = stack.pop()
        row = table[q]
        nxt = row[(row >= 0) & ok]
        if nxt.size == 0:
            raise ValueError(f"guided decoding: state {q} has no token left (no token of the vocabulary continues the pattern there, "
                             "or the logit bias / allowed / banned ids remove every one that does, or no EOS id ends it)")
        for t in np.unique(nxt):
            if int(t) not in seen:
                seen.add(int(t))
                stack.append(int(t))


@dataclass
class Guide:
    """What O3VEngine.generate(guide=...) takes: the device table and its shape."""
    table: "object"          # torch i16 [n_states, ldn] on the engine's device, contiguous
    n_states: int
    ldn: int
    start: int = 0
    host_table: Optional[np.ndarray] = None    # the same table on the host (check_no_dead_end against the call's bias)
