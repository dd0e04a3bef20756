"""Reference of o3v_content_hash128 (csrc/o3v_elem.hip) and the case list that the CPU and the GPU test share.

The formula, restated from the comment above content_hash_kernel, in unsigned 64-bit wrap-around arithmetic over the
little-endian 8-byte words w_0 .. w_{n-1} of the buffer (n = bytes // 8) and the tail word t (the bytes behind the last full
word, zero-extended; 0 when there are none), which enters as word n:

    h1 = sum_{i<=n} mix(w_i + C1 * (i + 1))       + mix(bytes ^ L1)
    h2 = sum_{i<=n} mix((w_i * C2) ^ (i + C3))    + mix(bytes * L2)

mix = splitmix64's finaliser (Steele, Lea, Flood: "Fast splittable pseudorandom number generators", OOPSLA 2014; Vigna's
splitmix64.c).  The test anchors mix on the generator's published first outputs, not on the kernel."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

M64 = (1 << 64) - 1
C1, C2, C3 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x2545F4914F6CDD1D
L1, L2 = 0xA0761D6478BD642F, 0xE7037ED1A0B428DB
W = 1024 * 256      # words of one grid-stride lap: the launch is capped at 1024 blocks of 256 threads
U = np.uint64


def mix(x):
    """splitmix64's finaliser; a Python int or a uint64 array (array arithmetic wraps, ints are masked)."""
    if isinstance(x, np.ndarray):
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
        return x ^ (x >> U(31))
    x &= M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def as_bytes(buf) -> np.ndarray:
    """bytes / any array -> its bytes as a flat uint8 array"""
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(buf), dtype=np.uint8)
    return np.ascontiguousarray(buf).reshape(-1).view(np.uint8)


def words_and_tail(b: np.ndarray):
    """-> (the full little-endian words as a uint64 array, the zero-extended tail word as an int)"""
    n = b.size // 8
    w = np.frombuffer(b[:n * 8].tobytes(), dtype="<u8").astype(U)
    return w, int.from_bytes(b[n * 8:].tobytes(), "little")


def content_hash128(buf):
    """-> (h1, h2) of the buffer's bytes, as Python ints in [0, 2^64)"""
    b = as_bytes(buf)
    w, t = words_and_tail(b)
    n = w.size
    i = np.arange(n, dtype=U)
    h1 = int(mix(w + U(C1) * (i + U(1))).sum(dtype=U)) if n else 0
    h2 = int(mix((w * U(C2)) ^ (i + U(C3))).sum(dtype=U)) if n else 0
    h1 += mix(t + C1 * (n + 1)) + mix(b.size ^ L1)
    h2 += mix((t * C2) ^ ((n + C3) & M64)) + mix(b.size * L2)
    return h1 & M64, h2 & M64


# ----------------------------------------------------------------------------------------------------------------------------
# the shared case list
# ----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name make")      # make() -> uint8 array, built deterministically from a seed
Pair = namedtuple("Pair", "name a b")       # names of two cases whose keys must differ in BOTH words

BIG = 5 * (1 << 20) + 9                     # a little over 5 MiB, 1 mod 8: 2.5 laps of words and one tail byte
FRAME = 512 * 1024                          # the big buffer read as ten "frames" of 512 KiB (and 9 bytes)


@lru_cache(maxsize=4)
def _random(n: int, seed: int) -> np.ndarray:
    a = np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8)
    a.setflags(write=False)
    return a


def _flip(n, seed, byte):
    def make():
        a = _random(n, seed).copy()
        a[byte] ^= 1
        return a
    return make


def _swap_words(n, seed, i, j, count=1):
    """words [i, i + count) exchanged with words [j, j + count); every exchanged pair of words unequal"""
    def make():
        a = _random(n, seed).copy()
        w = a[:n // 8 * 8].view("<u8")
        x, y = w[i:i + count].copy(), w[j:j + count].copy()
        assert (x != y).all() and i + count <= j and j + count <= w.size
        w[i:i + count], w[j:j + count] = y, x
        return a
    return make


def _build():
    cases, pairs = [], []

    def add(name, make):
        assert name not in {c.name for c in cases}
        cases.append(Case(name, make))
        return name

    def rnd(n, seed):
        return add(f"random {n}", lambda: _random(n, seed))

    # ---- byte lengths: nothing, less than a word, around one word / two words / one block of 256 words, a few blocks with a
    # tail, around the cap of 1024 blocks (W words), 2.5 laps
    for k, n in enumerate([0, 1, 7, 8, 9, 15, 16, 2047, 2048, 2049, 3 * 2048 + 5, 8 * W - 8, 8 * W, 8 * W + 8 * 257 + 3]):
        rnd(n, 100 + k)
    big = add("random big", lambda: _random(BIG, 7))
    z = [add(f"zeros {n}", (lambda n: lambda: np.zeros(n, dtype=np.uint8))(n)) for n in (4096, 4099)]
    pairs.append(Pair("all-zero buffers of two lengths", z[0], z[1]))

    # ---- one bit: in the first word's two end bytes, the second word, the last full word, every tail byte
    n, seed = 2047, 107                                             # = "random 2047": 255 words and 7 tail bytes
    for what, byte in [("byte 0", 0), ("byte 7", 7), ("byte 8", 8), ("the last byte of the last full word", 2039)] + \
                      [(f"tail byte {k}", 2040 + k) for k in range(7)]:
        pairs.append(Pair(f"lowest bit of {what}", "random 2047", add(f"random 2047, {what} flipped", _flip(n, seed, byte))))
    # ---- one bit at the lap boundary and in the third lap; the big buffer's single tail byte
    for what, byte in [("word W-1", 8 * (W - 1) + 3), ("word W", 8 * W), ("word 2W+12345 (third lap)", 8 * (2 * W + 12345) + 5),
                       ("the tail byte", BIG - 1)]:
        pairs.append(Pair(f"lowest bit in {what} of the big buffer", big, add(f"random big, {what} flipped", _flip(BIG, 7, byte))))
    # ---- the same words elsewhere: the word index must count
    pairs.append(Pair("two words of one lap exchanged", big, add("random big, words 5 / 70000 exchanged", _swap_words(BIG, 7, 5, 70000))))
    pairs.append(Pair("two words one lap apart exchanged (one thread reads both)", big,
                      add("random big, words 1000 / 1000+W exchanged", _swap_words(BIG, 7, 1000, 1000 + W))))
    pairs.append(Pair("two whole frames exchanged", big,
                      add("random big, frames 1 / 8 exchanged", _swap_words(BIG, 7, FRAME // 8, 8 * FRAME // 8, FRAME // 8))))
    # ---- zero bytes at the end: only the length tells these apart
    for base_n, seed in ((16, 106), (2047, 107)):
        pairs.append(Pair(f"one zero byte appended to {base_n} bytes", f"random {base_n}",
                          add(f"random {base_n} + a zero byte",
                              (lambda n, s: lambda: np.concatenate([_random(n, s), np.zeros(1, dtype=np.uint8)]))(base_n, seed))))

    def zero_tail():
        a = _random(2049, 109).copy()
        a[-1] = 0
        return a
    pairs.append(Pair("a zero tail byte taken away", add("random 2049, tail byte zero", zero_tail),
                      add("random 2049, tail byte dropped", lambda: _random(2049, 109)[:2048])))
    return cases, pairs


CASES, PAIRS = _build()
BY_NAME = {c.name: c for c in CASES}
