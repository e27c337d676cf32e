"""CPU: tests/philox_ref.py against the published Random123 Philox4x32-10 known-answer vectors, and the corner points of the
library's three mappings that no (seed, counter) reachable through the C ABI can be aimed at.  The GPU tests
(test_gpu_philox.py) then compare the kernels with this reference."""
import numpy as np
import pytest

import philox_ref as P

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, expected)
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    # digits of pi: the only vector that exercises c[2], c[3] and k1 together (the library always passes c[2] = c[3] = 0)
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = P.philox4x32_10(ctr, key)
    assert all(g.dtype == np.uint32 and g.shape == (1,) for g in got)
    assert tuple(int(g[0]) for g in got) == want


def test_philox4x32_10_is_elementwise_over_arrays():
    """All three vectors in one vectorised call give the same words as one call each."""
    ctr = [np.array([k[0][j] for k in KAT], dtype=np.uint64) for j in range(4)]
    key = [np.array([k[1][j] for k in KAT], dtype=np.uint64) for j in range(2)]
    got = np.stack(P.philox4x32_10(ctr, key), axis=1)
    assert got.tolist() == [list(k[2]) for k in KAT]


def test_words_split_seed_and_counter():
    (c0, c1, c2, c3), (k0, k1) = P.words(0x9E3779B97F4A7C15 + 777, (1 << 40) + 1)
    assert (int(c0), int(c1), c2, c3) == (1, 0x100, 0, 0)
    assert (k0, k1) == (0x7F4A7C15 + 777, 0x9E3779B9)
    # base + i carries into the high word inside one run of counters, and wraps mod 2^64 at the top
    c = P.counters((1 << 32) - 3, 5)
    assert [int(v) for v in c] == [(1 << 32) - 3 + i for i in range(5)]
    (c0, c1, _, _), _ = P.words(0, c)
    assert c0.tolist() == [0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF, 0, 1] and c1.tolist() == [0, 0, 0, 1, 1]
    assert [int(v) for v in P.counters((1 << 64) - 1, 2)] == [(1 << 64) - 1, 0]
    # (seed, ctr) is Philox of those words: the stream of (0, 0) starts with the first known-answer vector
    assert P.stream_words(0, 0, 4).tolist() == list(KAT[0][2])
    assert P.stream_words(0, 0, 7)[4:].tolist() == [int(w[0]) for w in P.philox4x32_10((1, 0, 0, 0), (0, 0))][:3]


def test_unit_float_and_box_muller_at_the_extreme_words():
    """u >> 8 == 0 and u >> 8 == 2^24 - 1: the two ends of the 24-bit mapping, evaluated here because no test can steer a kernel's
    Philox output onto them."""
    f = P.unit_float(np.array([0x00000000, 0x000000FF, 0x00000100, 0x7FFFFFFF, 0x80000000, 0x800001FF, 0xFFFFFEFF, 0xFFFFFFFF], dtype=np.uint32))
    assert f.dtype == np.float32
    assert f[0] == f[1] == np.float32(2.0 ** -25)                     # the low 8 bits are dropped
    assert f[2] == np.float32(1.5 * 2.0 ** -24)
    assert f[3] == np.float32((2 ** 23 - 1 + 0.5) * 2.0 ** -24)       # last k whose k + 0.5 is exact
    assert f[4] == np.float32(0.5)                                    # 2^23 + 0.5 ties to even: 2^23
    assert f[5] == np.float32((2 ** 23 + 2) * 2.0 ** -24)             # 2^23 + 1.5 ties to even: 2^23 + 2
    assert f[6] == np.float32((2 ** 24 - 2) * 2.0 ** -24)             # 2^24 - 1.5 ties to even: 2^24 - 2
    assert f[7] == np.float32(1.0)                                    # 2^24 - 0.5 ties to even: 2^24
    assert (f > 0).all() and (f <= 1).all()
    # smallest f0: the largest radius the mapping can produce; largest f0: radius 0 (ln 1 = 0), never a NaN
    a, b = P.box_muller(np.uint32(0), np.uint32(0))
    assert np.isclose(np.hypot(a, b), P.MAX_RADIUS, rtol=1e-15) and np.isclose(P.MAX_RADIUS, 5.887050112577373, rtol=1e-15)
    a, b = P.box_muller(np.uint32(0xFFFFFFFF), np.uint32(0x12345678))
    assert a == 0.0 and b == 0.0
    a, b = P.box_muller(np.uint32(0x12345678), np.uint32(0xFFFFFFFF))     # theta = 2 pi exactly: (r, ~0)
    r = np.sqrt(-2.0 * np.log(float(P.unit_float(np.uint32(0x12345678)))))
    assert np.isfinite([a, b]).all() and abs(a - r) < 1e-15 and abs(b) < 1e-14


def test_randint_and_dropout_mappings():
    w = P.stream_words(777, 5, 11)
    assert P.randint(777, 5, 11, 1).tolist() == [0] * 11
    assert P.randint(777, 5, 11, 2).tolist() == (w >> 31).tolist()
    hi = (1 << 31) - 1
    assert P.randint(777, 5, 11, hi).tolist() == [(int(v) * hi) >> 32 for v in w]
    assert P.dropout_threshold(0.5) == 1 << 31 and P.dropout_threshold(0.25) == 1 << 30
    assert P.dropout_threshold(0.001) == int(float(np.float32(0.001)) * 2.0 ** 32) == 4294967        # float32(0.001) = 0.0010000000475
    assert P.dropout_keep(777, 5, 11, 0.5).tolist() == (w >> 31).tolist()
    # normals: block k of four outputs comes from counter offset + k, in (cos, sin) pairs
    v = P.normals(777, 5, 7)
    a, b = P.box_muller(w[4], w[5])
    assert v.shape == (7,) and v[4] == a[()] and v[5] == b[()]
    assert np.array_equal(P.normals(777, 6, 3), v[4:7])
