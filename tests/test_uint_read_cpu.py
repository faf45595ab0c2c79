"""Encrypted tables read at encrypted indices (csgn_uint_read*) on a box without a GPU: the term count E, the argument
checks, the dispatch names and knob, the loud failure without a device, the term order the kernel decodes (the walk
over the index bits and the mixed-radix digits, restated here), and the DEFINITION -- the left-nested sum over rows r
of csgn_uint_plain's EQ(x, r) times row r, a composition of the reference's operator+ / operator* with ONE -- pinned
against the compiled reference and the oracle, with decryptions under random keys equal to table[x] (0 past the
table).  The device side is tests/test_uint_read_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, c_E, compose_read, const_term, decrypt_value, encrypt_planes, lib, np_add, np_read,
                         np_read_fast, oracle_ops, rand_terms, read_terms, ref_ops, u64s)


# -- the term order the kernel decodes (csgn_uint_read.hip): no table of terms, a walk from the top bit ----------------
def decode(q, s, rows):
    """Entry q of the E stream: (r, digits d_k), include/csgn_hip.h's term order, by the walk and the digits."""
    v = len(s)
    F = [1] * v
    for k in range(1, v):
        F[k] = F[k - 1] * (2 * s[k - 1] + 1)
    last, r, H, tight = rows - 1, 0, 1, True
    for k in reversed(range(v)):
        if tight and not (last >> k) & 1:
            H *= s[k] + 1
            continue
        c0 = H * (s[k] + 1) * F[k]
        if q < c0:
            H *= s[k] + 1
            tight = False
        else:
            q -= c0
            r |= 1 << k
            H *= s[k]
    assert q < H
    digits = [0] * v
    for k in reversed(range(v)):
        R = s[k] if (r >> k) & 1 else s[k] + 1
        digits[k] = q % R
        q //= R
    return r, digits


def np_read_decoded(n, index, table):
    """The same words term by term from the decode: term q * t_j + c = AND over k of (digit < s_k ? x_k[digit] : ONE)
    AND term c of row r."""
    batch, _, dl = index[0].shape
    s = [p.shape[1] for p in index]
    rows = table[0].shape[0]
    E = read_terms(s, rows)
    one = const_term(n, 1)
    outs = []
    for d in table:
        t = d.shape[1]
        o = np.empty((batch, E * t, dl), dtype=np.uint64)
        for q in range(E):
            r, digits = decode(q, s, rows)
            v = np.broadcast_to(one, (batch, dl)).copy()
            for k, dg in enumerate(digits):
                if dg < s[k]:
                    v &= index[k][:, dg, :]
            for c in range(t):
                o[:, q * t + c, :] = v & d[r, c, :]
        outs.append(o)
    return outs


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_fresh_full_tables(lib):
    for v in range(1, 17):
        assert c_E(lib, v, [1] * v, 1 << v) == 3 ** v, v
    assert c_E(lib, 8, [1] * 8, 256) == 6561


def test_terms_formula(lib):
    rng = np.random.default_rng(5)
    for v in range(1, 9):
        for s in ([1] * v, [2] * v, [int(x) for x in rng.integers(1, 5, v)]):
            for rows in sorted({1, 2, (1 << v) - 1, 1 << v, int(rng.integers(1, (1 << v) + 1)),
                                int(rng.integers(1, (1 << v) + 1))}):
                if rows < 1 or rows > 1 << v:
                    continue
                assert c_E(lib, v, s, rows) == read_terms(s, rows), (v, s, rows)
        full = int(np.prod([2 * x + 1 for x in s], dtype=object))
        assert c_E(lib, v, s, 1 << v) == full
    # one row: only x == 0 matches, every bit a zero: prod (s_k + 1)
    assert c_E(lib, 5, [1, 2, 3, 1, 1], 1) == 2 * 3 * 4 * 2 * 2
    # fresh, partial: 200 of 256 rows
    assert c_E(lib, 8, [1] * 8, 200) == sum(2 ** (8 - bin(r).count("1")) for r in range(200))
    assert c_E(lib, 16, [1] * 16, 65535) == 3 ** 16 - 1


def test_terms_invalid(lib):
    one = [1] * 17
    assert c_E(lib, 0, one, 1) == 0                                   # index width outside 1..16
    assert c_E(lib, 17, one, 1) == 0
    assert c_E(lib, 4, one, 0) == 0                                   # rows outside 1..2^v
    assert c_E(lib, 4, one, 17) == 0
    assert c_E(lib, 4, one, 16) == 81
    assert c_E(lib, 4, None, 16) == 0                                 # null pointer
    assert c_E(lib, 3, [1, 0, 1], 8) == 0                             # a plane of no terms
    # 2^62 or more: (2s + 1)^4 with s = 2^14 - 1 is below 2^60, with s = 2^16 far past 2^62
    assert c_E(lib, 4, [1 << 16] * 4, 16) == 0
    assert c_E(lib, 4, [(1 << 14) - 1] * 4, 16) == (2 ** 15 - 1) ** 4
    assert c_E(lib, 2, [1 << 61, 1], 4) == 0
    assert c_E(lib, 1, [LIMIT - 1], 2) == 0
    assert c_E(lib, 1, [LIMIT // 2 - 1], 2) == LIMIT - 1
    assert c_E(lib, 1, [LIMIT], 1) == 0


def test_dispatch_names(lib, knobs):
    knobs.unset("uint_read_fused")
    from csgn_amd import capi
    assert "uint_read_fused" in capi.tuning_names()

    def name(n, v, s, rows, w, t):
        return lib.csgn_uint_read_kernel(n, 256, v, u64s(s), rows, w, u64s(t)).decode()

    assert name(1247, 8, [1] * 8, 256, 8, [1] * 8) == "k_uint_read"
    assert name(1247, 1, [2], 1, 1, [3]) == "k_uint_read"
    assert name(0, 8, [1] * 8, 256, 8, [1] * 8) == ""                 # n_bits 0
    assert name(1247, 17, [1] * 17, 256, 8, [1] * 8) == ""            # bad index width
    assert name(1247, 4, [1] * 4, 17, 8, [1] * 8) == ""               # rows past 2^v
    assert name(1247, 4, [1] * 4, 0, 8, [1] * 8) == ""
    assert name(1247, 4, [1] * 4, 16, 0, [1] * 8) == ""               # table width outside 1..64
    assert name(1247, 4, [1] * 4, 16, 65, [1] * 65) == ""
    assert name(1247, 4, [1, 0, 1, 1], 16, 2, [1, 1]) == ""           # a plane of no terms
    assert name(1247, 4, [1] * 4, 16, 2, [1, 0]) == ""
    knobs.set("uint_read_fused", 0)
    assert capi.get_tuning("uint_read_fused") == 0
    assert name(1247, 8, [1] * 8, 256, 8, [1] * 8) == "composed"
    knobs.set("uint_read_fused", 1)
    assert name(1247, 8, [1] * 8, 256, 8, [1] * 8) == "k_uint_read"


def test_fails_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_uint_read_gpu.py covers the device")
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 64)(*([p] * 64))
    one = u64s([1] * 64)
    rc = lib.csgn_uint_read(1247, 4, 8, ptrs, one, 256, 8, ptrs, one, ptrs, None)
    assert rc == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    # argument errors are reported before the device is looked for
    assert lib.csgn_uint_read(0, 4, 8, ptrs, one, 256, 8, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 0, ptrs, one, 1, 8, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 17, ptrs, one, 1, 8, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 8, ptrs, one, 0, 8, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 8, ptrs, one, 257, 8, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 8, ptrs, one, 256, 0, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 8, ptrs, one, 256, 65, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 8, None, one, 256, 8, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 8, ptrs, one, 256, 8, ptrs, one, None, None) == -1
    assert lib.csgn_uint_read(1247, 4, 3, ptrs, u64s([1, 0, 1]), 8, 8, ptrs, one, ptrs, None) == -1
    assert lib.csgn_uint_read(1247, 4, 3, ptrs, one, 8, 2, ptrs, u64s([1, 0]), ptrs, None) == -1
    # too large: 3^16 terms * 20 words = 8.6e8 < 2^31, but 3 table terms pass it; 4^16 * 1 does too
    assert lib.csgn_uint_read(1247, 4, 16, ptrs, one, 1 << 16, 1, ptrs, u64s([3]), ptrs, None) == -2
    assert lib.csgn_uint_read(1247, 4, 16, ptrs, one, 1 << 16, 1, ptrs, u64s([2]), ptrs, None) == -3
    assert lib.csgn_uint_read(1247, 4, 16, ptrs, u64s([2] * 16), 1 << 16, 1, ptrs, one, ptrs, None) == -2
    assert lib.csgn_uint_read(1247, 1 << 44, 8, ptrs, one, 256, 8, ptrs, one, ptrs, None) == -2     # batch


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
CASES = [  # (v, rows, index terms, table terms)
    (1, 1, [1], [1]),
    (1, 2, [1], [1, 1]),
    (1, 2, [2], [3]),
    (2, 3, [1, 1], [1, 2]),
    (2, 4, [2, 1], [1]),
    (3, 8, [1, 1, 1], [1, 1, 1]),
    (3, 5, [1, 2, 1], [2, 1]),
    (4, 16, [1, 1, 1, 1], [1, 1]),
    (4, 11, [2, 1, 3, 1], [1, 2, 1]),
    (4, 9, [2, 2, 2, 2], [2]),
]


@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_definition_matches_reference(oracle, ref, n, d, case):
    v, rows, s, t = CASES[case]
    seed = 1000 * case + n
    index = [rand_terms(n, 1, sk, seed + k)[0].ravel() for k, sk in enumerate(s)]
    table = [rand_terms(n, rows, tj, seed + 50 + j) for j, tj in enumerate(t)]
    row_words = [[table[j][r].ravel() for j in range(len(t))] for r in range(rows)]
    one, zero = const_term(n, 1), const_term(n, 0)
    add, mul = ref_ops(ref, n, d)
    want = compose_read(index, row_words, add, mul, one, zero)
    add, mul = oracle_ops(oracle, n)
    got = compose_read(index, row_words, add, mul, one, zero)
    words = np_read(n, [x.reshape(1, sk, -1) for x, sk in zip(index, s)], table)
    dl = (n + 63) // 64
    E = read_terms(s, rows)
    for j in range(len(t)):
        assert np.array_equal(got[j], want[j]), j
        assert got[j].size == t[j] * E * dl
        assert np.array_equal(words[j].ravel(), got[j]), j


@pytest.mark.parametrize("n", [64, 63, 1247])
def test_definition_matches_oracle_batched(oracle, n):
    s, t, rows, batch = [2, 1, 3], [1, 2], 6, 3
    index = [rand_terms(n, batch, sk, 60 + k) for k, sk in enumerate(s)]
    table = [rand_terms(n, rows, tj, 70 + j) for j, tj in enumerate(t)]
    add, mul = oracle_ops(oracle, n)
    words = np_read(n, index, table)
    for e in range(batch):
        rows_e = [[table[j][r].ravel() for j in range(len(t))] for r in range(rows)]
        want = compose_read([x[e].ravel() for x in index], rows_e, add, mul, const_term(n, 1), const_term(n, 0))
        for j in range(len(t)):
            assert np.array_equal(words[j][e].ravel(), want[j]), (e, j)


@pytest.mark.parametrize("v,rows,s,t", [(1, 2, [1], [1]), (2, 3, [1, 1], [2, 1]), (3, 8, [1, 2, 1], [1]),
                                        (4, 16, [1] * 4, [1, 3]), (4, 13, [2, 1, 1, 3], [2]), (5, 20, [1] * 5, [1]),
                                        (5, 32, [1, 1, 2, 1, 1], [1])])
def test_decode_gives_the_definition(v, rows, s, t):
    """The walk and digits csgn_uint_read.hip decodes reproduce the definition's words term for term."""
    n, batch = 129, 2
    index = [rand_terms(n, batch, sk, 80 + k) for k, sk in enumerate(s)]
    table = [rand_terms(n, rows, tj, 90 + j) for j, tj in enumerate(t)]
    want = np_read(n, index, table)
    got = np_read_decoded(n, index, table)
    for j in range(len(t)):
        assert np.array_equal(got[j], want[j]), j


def test_fast_numpy_form_is_the_definition():
    n = 65
    for v, rows, s, t in [(1, 1, [1], [2]), (3, 7, [1, 2, 1], [1, 3]), (4, 16, [1] * 4, [1] * 5)]:
        index = [rand_terms(n, 3, sk, 110 + k) for k, sk in enumerate(s)]
        table = [rand_terms(n, rows, tj, 120 + j) for j, tj in enumerate(t)]
        for a, b in zip(np_read(n, index, table), np_read_fast(n, index, table)):
            assert np.array_equal(a, b)


def test_decode_fresh_subsets():
    """Fresh planes: entry q is P[S] & row r, S = ones(r) plus the zero bits whose digit is 0."""
    v = 4
    s = [1] * v
    E = 3 ** v
    seen = set()
    for q in range(E):
        r, digits = decode(q, s, 1 << v)
        S = sum(1 << k for k in range(v) if digits[k] == 0)
        assert S & r == r
        seen.add((r, S))
    assert len(seen) == E                               # every (row, superset of its ones) once
    assert [decode(q, s, 1 << v)[0] for q in range(E)] == sorted(decode(q, s, 1 << v)[0] for q in range(E))


# -- decryptions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2, 3, 4])
def test_truth_tables_decrypt(oracle, v):
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(270 + v, 64 * d + 64))
    xs = np.arange(1 << v, dtype=np.uint64)
    index = encrypt_planes(oracle, n, key, xs, v, 280 + v)
    rng = np.random.default_rng(v)
    for rows in sorted({1, (1 << v) - 1, 1 << v, int(rng.integers(1, (1 << v) + 1))}):
        if rows < 1:
            continue
        w = 1 + (rows + v) % 4
        values = rng.integers(0, 1 << w, rows).astype(np.uint64)
        table = encrypt_planes(oracle, n, key, values, w, 290 + 10 * v + rows)
        table = [x.reshape(rows, 1, -1) for x in table]
        got = decrypt_value(oracle, n, key, np_read(n, index, table))
        want = [int(values[x]) if x < rows else 0 for x in range(1 << v)]
        assert [int(g) for g in got] == want, (v, rows)


def test_multi_term_planes_decrypt(oracle):
    """Index planes that are sums (x + ZERO + ZERO ...: more terms, the same bit) read the same values."""
    n, d, v, rows = 127, 8, 3, 6
    key, _ = oracle.keygen(n, d, glibc_draws(301, 64 * d + 64))
    xs = np.arange(1 << v, dtype=np.uint64)
    index = encrypt_planes(oracle, n, key, xs, v, 302)
    zero = encrypt_planes(oracle, n, key, np.zeros(1 << v, dtype=np.uint64), 1, 303)[0]
    index = [index[0], np_add(index[1], zero), np_add(np_add(index[2], zero), zero)]
    values = np.array([5, 0, 7, 3, 6, 1], dtype=np.uint64)
    table = [x.reshape(rows, 1, -1) for x in encrypt_planes(oracle, n, key, values, 3, 304)]
    zt = encrypt_planes(oracle, n, key, np.zeros(rows, dtype=np.uint64), 1, 305)[0].reshape(rows, 1, -1)
    table[1] = np_add(table[1], zt)
    outs = np_read(n, index, table)
    assert outs[1].shape[1] == 2 * read_terms([1, 2, 3], rows)
    got = decrypt_value(oracle, n, key, outs)
    assert [int(g) for g in got] == [int(values[x]) if x < rows else 0 for x in range(1 << v)]
