"""Continuous batching: the host bookkeeping of O3VEngine.generate_continuous, free of any device code.

A session is a run of decode columns 0 .. session_columns over `rows` decode rows that share one set of buffers.  A request
admitted into row b at column t0 has its prompt's K/V in slots [0, S) of the row's cache and its generated token of column t in
slot S + (t - t0): the decode kernels compute a row's context as row_base[b] + t + 1, so row_base[b] = S - t0.  A row without a
request carries IDLE_BASE, for which no column gives a context in [1, Tmax]: the attention kernel touches nothing of it."""
from __future__ import annotations

from collections import deque
from typing import NamedTuple, Optional, Sequence

import numpy as np

IDLE_BASE = -(1 << 30)      # row_base of a row without a request


class Admission(NamedTuple):
    row: int
    request: int
    t0: int         # column of the request's first generated token
    row_base: int   # S - t0
    refill: bool    # the row has served another request of this call before


class Retired(NamedTuple):
    row: int
    request: int
    t0: int
    n: int          # tokens kept: columns [t0, t0 + n) of the row


class Chunk(NamedTuple):
    step0: int
    n_steps: int
    skip_last_forward: bool     # no live row needs the logits of the chunk's last forward


def default_session_columns(max_new: Sequence[int], steps_per_sync: int) -> int:
    """Columns of a session when the caller names none: four times the longest completion (so a row serves a handful of requests
    before the session rolls over), at least 1024, rounded up to whole chunks.  Costs rows x columns x (8 + 4 head_dim) bytes of
    output ids, margins and M-RoPE table."""
    c = max(1024, 4 * max(int(m) for m in max_new))
    return -(-c // steps_per_sync) * steps_per_sync


class ContinuousScheduler:
    """Admit / retire / roll-over for one generate_continuous call.  Drive it as

        while not s.done():
            for a in s.admit(): ...prefill request a.request into row a.row, row_base[a.row] = a.row_base...
            c = s.chunk();      ...decode columns [c.step0, c.step0 + c.n_steps)...
            for r in s.retire(ids of those columns [rows, n_steps]): ...finished[r.row] = 1, row_base[r.row] = IDLE_BASE...

    Requests are admitted in input order, each exactly once, only at a chunk boundary and only if t0 + max_new <= session_columns;
    when the next one does not fit, admission stops, the live rows drain and a new session opens at column 0."""

    def __init__(self, prompt_lens: Sequence[int], max_new: Sequence[int], rows: int, session_columns: int, steps_per_sync: int,
                 eos_token_ids: Sequence[int] = ()):
        self.S = [int(s) for s in prompt_lens]
        self.max_new = [int(m) for m in max_new]
        if len(self.S) != len(self.max_new):
            raise ValueError("one max_new_tokens per request")
        if rows <= 0 or steps_per_sync <= 0:
            raise ValueError("rows and steps_per_sync must be positive")
        if any(m <= 0 for m in self.max_new):
            raise ValueError("`max_new_tokens` must be greater than 0")
        if self.max_new and max(self.max_new) > session_columns:
            raise ValueError(f"session_columns={session_columns} is shorter than the longest completion ({max(self.max_new)})")
        self.rows, self.columns, self.sync = int(rows), int(session_columns), int(steps_per_sync)
        self.eos = frozenset(int(e) for e in eos_token_ids)
        self.pending = deque(range(len(self.S)))
        self.row_req = [None] * self.rows        # request of a live row
        self.row_t0 = [0] * self.rows
        self.row_toks = [[] for _ in range(self.rows)]
        self.row_used = [False] * self.rows
        self.t = 0
        self.sessions = 0
        self.rows_refilled = 0
        self.decode_steps = 0

    def done(self) -> bool:
        return not self.pending and all(r is None for r in self.row_req)

    def live(self):
        return [b for b in range(self.rows) if self.row_req[b] is not None]

    def admit(self):
        """The admissions of this chunk boundary.  Opens a session (column 0) when every row is idle and requests are left."""
        out = []
        if self.pending and not self.live() and (self.sessions == 0 or self.t + self.max_new[self.pending[0]] > self.columns):
            self.t = 0
            self.sessions += 1
        for b in range(self.rows):
            if not self.pending:
                break
            if self.row_req[b] is not None:
                continue
            r = self.pending[0]
            if self.t + self.max_new[r] > self.columns:
                break       # the next request does not fit: the live rows drain, then a new session
            self.pending.popleft()
            self.row_req[b], self.row_t0[b], self.row_toks[b] = r, self.t, []
            out.append(Admission(b, r, self.t, self.S[r] - self.t, self.row_used[b]))
            self.rows_refilled += int(self.row_used[b])
            self.row_used[b] = True
        return out

    def chunk(self) -> Chunk:
        live = self.live()
        if not live:
            raise RuntimeError("chunk() without a live row")
        n = min(self.sync, self.columns - self.t)
        end = self.t + n
        skip = all(self.row_t0[b] + self.max_new[self.row_req[b]] <= end for b in live)
        return Chunk(self.t, n, skip)

    def row_base(self):
        return [IDLE_BASE if self.row_req[b] is None else self.S[self.row_req[b]] - self.row_t0[b] for b in range(self.rows)]

    def retire(self, ids: np.ndarray):
        """ids i [rows, n_steps]: what the chunk just decoded wrote.  -> the rows that ended: at their first id of eos_token_ids
        (kept) or after max_new tokens; what a row wrote behind its end is dropped."""
        ids = np.asarray(ids)
        n = ids.shape[1]
        out = []
        for b in self.live():
            r = self.row_req[b]
            toks = self.row_toks[b]
            toks.extend(int(x) for x in ids[b])
            keep: Optional[int] = None
            for j, tok in enumerate(toks[:self.max_new[r]]):
                if tok in self.eos:
                    keep = j + 1
                    break
            if keep is None and len(toks) >= self.max_new[r]:
                keep = self.max_new[r]
            if keep is not None:
                out.append(Retired(b, r, self.row_t0[b], keep))
                self.row_req[b] = None
        self.t += n
        self.decode_steps += n
        return out
