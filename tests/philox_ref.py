"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library) in
plain numpy, and the three ways the library maps its words to outputs.  Nothing here looks at the kernels' code: the round is
restated from the paper, the mappings from the comments of csrc/common.h, csrc/embedding.hip and csrc/elementwise.hip.
tests/test_philox_ref.py pins the generator to the published known-answer vectors; the GPU tests compare the kernels with it.

  words(seed, ctr)   counter = {lo32(ctr), hi32(ctr), 0, 0}, key = {lo32(seed), hi32(seed)}
  normals            block k of four outputs <- counter offset + k:  (v0, v1) = BoxMuller(r0, r1), (v2, v3) = BoxMuller(r2, r3)
  randint            element i = (word i & 3 of counter offset + (i >> 2)) * high >> 32
  dropout            element e kept iff word e & 3 of counter off + (e >> 2) >= uint32((double)(float32)p * 2^32)
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key schedule (Weyl) increments: golden ratio, sqrt(3) - 1
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
U64 = (1 << 64) - 1


def philox4x32_10(counter_words, key_words):
    """Ten rounds on counters (c0, c1, c2, c3) under keys (k0, k1): each an integer or an array of values < 2^32 (broadcast
    against each other).  Returns the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK32 for c in counter_words)
    k0, k1 = (np.atleast_1d(np.asarray(k, dtype=np.uint64)) & MASK32 for k in key_words)
    for _ in range(10):
        p0 = np.uint64(M0) * c0                      # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(seed: int, ctr):
    """(counter_words, key_words) of the library's 64-bit (seed, counter) pair; ``ctr`` an integer or a uint64 array."""
    seed = int(seed) & U64
    ctr = np.asarray(ctr, dtype=np.uint64)
    return (ctr & MASK32, ctr >> S32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32)


def counters(base: int, count: int) -> np.ndarray:
    """base, base + 1, ... as uint64, wrapping mod 2^64 like the device's unsigned addition."""
    with np.errstate(over="ignore"):
        return np.uint64(int(base) & U64) + np.arange(count, dtype=np.uint64)


def stream_words(seed: int, offset: int, n: int) -> np.ndarray:
    """The first n words of the stream (seed, offset): word i is word i & 3 of counter offset + (i >> 2).  uint32 [n]."""
    blocks = (n + 3) // 4
    w = np.stack(philox4x32_10(*words(seed, counters(offset, blocks))), axis=1)      # [blocks, 4]
    return w.reshape(-1)[:n].copy()


def unit_float(u) -> np.ndarray:
    """uint32 word -> float32 in (0, 1]: ((float32)(u >> 8) + 0.5f) * 2^-24, every step in float32.  For u >> 8 >= 2^23 the sum
    k + 0.5 is a tie between two float32 values and rounds to the even one (so u >> 8 = 2^24 - 1 gives exactly 1.0): that rounding
    is part of the definition."""
    k = (np.asarray(u, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)          # exact: < 2^24
    return (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def box_muller(u0, u1):
    """(r cos theta, r sin theta) in float64 with r = sqrt(-2 ln f0), theta = 2 pi f1 of the float32 unit floats."""
    f0 = unit_float(u0).astype(np.float64)
    f1 = unit_float(u1).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(f0))
    th = 2.0 * np.pi * f1
    return r * np.cos(th), r * np.sin(th)


MAX_RADIUS = float(np.sqrt(50.0 * np.log(2.0)))      # f0 = 2^-25, the smallest unit float (u >> 8 == 0)


def normals(seed: int, offset: int, n: int) -> np.ndarray:
    """float64 [n]: the values rho_philox_normal(out[n], seed, offset) approximates in float32."""
    blocks = (n + 3) // 4
    r0, r1, r2, r3 = philox4x32_10(*words(seed, counters(offset, blocks)))
    v0, v1 = box_muller(r0, r1)
    v2, v3 = box_muller(r2, r3)
    return np.stack([v0, v1, v2, v3], axis=1).reshape(-1)[:n].copy()


def randint(seed: int, offset: int, n: int, high: int) -> np.ndarray:
    """int64 [n]: rho_randint's floor(word * high / 2^32), exact (word < 2^32, high < 2^31)."""
    assert 0 < high < (1 << 31)
    return ((stream_words(seed, offset, n).astype(np.uint64) * np.uint64(high)) >> S32).astype(np.int64)


def dropout_threshold(p) -> int:
    """uint32((double)(float32)p * 2^32), truncated."""
    return int(float(np.float32(p)) * 4294967296.0)


def dropout_keep(seed: int, offset: int, n: int, p) -> np.ndarray:
    """uint8 [n]: 1 where element e keeps its value."""
    return (stream_words(seed, offset, n) >= np.uint32(dropout_threshold(p))).astype(np.uint8)
