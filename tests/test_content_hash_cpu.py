"""The reference of the content hash (tests/hash_ref.py) on its own, without a GPU: its mix is splitmix64's, its case list tells
buffers apart that a cache key must tell apart, and the list is discriminating -- a reference with any one of five defects a
kernel could have gives another value on at least one case, so a kernel with that defect fails the exact comparison of
test_gpu_content_cache.py."""
import time

import numpy as np
import pytest

import hash_ref as hr
from hash_ref import C1, C2, C3, L1, L2, M64, U, W, mix


def test_mix_is_splitmix64():
    """splitmix64 seeded with 0: state += C1, output mix(state).  Its first three outputs are published (Vigna's splitmix64.c;
    the values every port's test suite quotes)."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 487617019471545679]
    assert [mix(k * C1) for k in (1, 2, 3)] == want
    assert mix(np.asarray([C1, (2 * C1) & M64, (3 * C1) & M64], dtype=U)).tolist() == want      # the vectorised form agrees
    assert mix(0) == 0


def test_reference_by_hand_on_small_buffers():
    """the vectorised sums against the formula written out word by word in Python ints"""
    def by_hand(b):
        n = len(b) // 8
        words = [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(n)] + [int.from_bytes(b[8 * n:], "little")]
        h1 = sum(mix(w + C1 * (i + 1)) for i, w in enumerate(words)) + mix(len(b) ^ L1)
        h2 = sum(mix((w * C2) ^ ((i + C3) & M64)) for i, w in enumerate(words)) + mix(len(b) * L2)
        return h1 & M64, h2 & M64
    for c in hr.CASES:
        buf = c.make()
        if buf.size <= 3 * 2048 + 5:
            assert hr.content_hash128(buf) == by_hand(buf.tobytes()), c.name
    assert hr.content_hash128(b"") == ((mix(C1) + mix(L1)) & M64, (mix(C3) + mix(0)) & M64)
    assert hr.content_hash128(b"abc") == hr.content_hash128(np.frombuffer(b"abc", dtype=np.uint8))


def test_reference_is_fast_enough():
    buf = hr.BY_NAME["random big"].make()
    assert buf.size > 5 * 2 ** 20 and buf.size % 8 == 1
    t = time.perf_counter()
    hr.content_hash128(buf)
    assert time.perf_counter() - t < 1.0


@pytest.fixture(scope="module")
def true_values():
    return {c.name: hr.content_hash128(c.make()) for c in hr.CASES}


def test_case_list_covers_what_it_says():
    sizes = {c.make().size for c in hr.CASES}
    assert sizes >= {0, 1, 7, 8, 9, 15, 16, 2047, 2048, 2049, 3 * 2048 + 5, 8 * W - 8, 8 * W, 8 * W + 8 * 257 + 3, hr.BIG}
    for c in hr.CASES:      # deterministic builders
        a = c.make()
        assert a.dtype == np.uint8 and a.ndim == 1 and np.array_equal(a, c.make()), c.name
    zeros = [c for c in hr.CASES if c.name.startswith("zeros")]
    assert len({c.make().size for c in zeros}) == 2 and not any(c.make().any() for c in zeros)
    for p in hr.PAIRS:
        a, b = hr.BY_NAME[p.a].make(), hr.BY_NAME[p.b].make()
        assert a.size != b.size or (a != b).any(), p.name
    flips = [p for p in hr.PAIRS if p.name.startswith("lowest bit")]
    assert len(flips) == 4 + 7 + 4
    for p in flips:         # exactly one bit apart
        a, b = hr.BY_NAME[p.a].make(), hr.BY_NAME[p.b].make()
        d = np.flatnonzero(a != b)
        assert d.size == 1 and (a[d[0]] ^ b[d[0]]) == 1, p.name


def test_every_pair_differs_in_both_words(true_values):
    for p in hr.PAIRS:
        a, b = true_values[p.a], true_values[p.b]
        assert a[0] != b[0] and a[1] != b[1], p.name
    assert len(set(true_values.values())) == len(hr.CASES)      # no two cases share a key at all


# ----------------------------------------------------------------------------------------------------------------------------
# five deliberately broken references: what a kernel could get wrong and still serve every cache-hit test
# ----------------------------------------------------------------------------------------------------------------------------
def _sums(w, index=True):
    i = np.arange(w.size, dtype=U) if index else np.zeros(w.size, dtype=U)
    return (int(mix(w + U(C1) * (i + U(1))).sum(dtype=U)) if w.size else 0,
            int(mix((w * U(C2)) ^ (i + U(C3))).sum(dtype=U)) if w.size else 0)


def _tail_terms(t, n):
    return mix(t + C1 * (n + 1)), mix((t * C2) ^ ((n + C3) & M64))


def _length_terms(nbytes):
    return mix(nbytes ^ L1), mix(nbytes * L2)


def _combine(*terms):
    return sum(t[0] for t in terms) & M64, sum(t[1] for t in terms) & M64


def no_tail_word(buf):
    b = hr.as_bytes(buf)
    w, _ = hr.words_and_tail(b)
    return _combine(_sums(w), _length_terms(b.size))


def no_length_terms(buf):
    b = hr.as_bytes(buf)
    w, t = hr.words_and_tail(b)
    return _combine(_sums(w), _tail_terms(t, w.size))


def no_word_index(buf):
    b = hr.as_bytes(buf)
    w, t = hr.words_and_tail(b)
    return _combine(_sums(w, index=False), _tail_terms(t, 0), _length_terms(b.size))


def first_lap_only(buf):
    b = hr.as_bytes(buf)
    w, t = hr.words_and_tail(b)
    return _combine(_sums(w[:W]), _tail_terms(t, w.size), _length_terms(b.size))


def constant(buf):
    return hr.content_hash128(b"")


def test_the_helpers_of_the_broken_references_rebuild_the_true_one(true_values):
    """the pieces the broken variants are put together from, put together in full, ARE the reference"""
    for c in hr.CASES:
        b = c.make()
        w, t = hr.words_and_tail(b)
        assert _combine(_sums(w), _tail_terms(t, w.size), _length_terms(b.size)) == true_values[c.name], c.name


@pytest.mark.parametrize("broken", [no_tail_word, no_length_terms, no_word_index, first_lap_only, constant], ids=lambda f: f.__name__)
def test_case_list_catches_a_broken_hash(true_values, broken):
    """at least one case's value differs from the true one (the GPU test compares every case exactly), and at least one pair that
    must differ collides or the value check alone carries it -- printed, so the log shows which cases catch which defect"""
    wrong = [c.name for c in hr.CASES if broken(c.make()) != true_values[c.name]]
    collide = [p.name for p in hr.PAIRS if any(x == y for x, y in zip(broken(hr.BY_NAME[p.a].make()), broken(hr.BY_NAME[p.b].make())))]
    print(f"{broken.__name__}: {len(wrong)} of {len(hr.CASES)} values wrong; colliding pairs: {collide}")
    assert wrong, f"{broken.__name__} passes every case"
    # the defect each variant stands for also shows as a collision of a pair built for it
    expect = {"no_tail_word": "lowest bit of tail byte 3", "no_length_terms": "one zero byte appended to 16 bytes",
              "no_word_index": "two words of one lap exchanged", "first_lap_only": "lowest bit in word W of the big buffer",
              "constant": "lowest bit of byte 0"}[broken.__name__]
    assert expect in collide, (broken.__name__, collide)
