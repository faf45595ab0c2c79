"""The sizes and the definition of the read that follows csgn_uint_write -- arrays whose rows differ in size read at
encrypted indices -- on a box without a GPU: the three restatements of the definition in tests/model_pick_rows.py against
one another, the DEFINITION -- output j is the left-nested sum over r of EQ(index, r) * (row r, plane j) -- pinned
against the compiled reference and the oracle, the offsets of the rows and of their blocks (csgn_uint_pick_rows_offsets)
against the model, a constant T against csgn_uint_pick_terms, the refused arguments, no wrap at 2^62, and the
decryptions of a read after a write."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, const_term, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms, read_terms,  # noqa: F401
                         ref_ops, u64s)
from tests.model_pick import EACH, c_pick_terms, np_pick
from tests.model_pick_rows import (c_offsets, clear_pick_rows, compose_pick_rows, np_pick_rows, np_pick_rows_decoded,
                                   np_pick_rows_fast, out_terms, rows_offsets, write_shaped)
from tests.model_write import array_terms, np_write, row_terms

INDEX_TERMS = ([1], [1, 1], [1, 1, 1], [2, 1, 3], [3, 2], [1, 1, 1, 1], [1, 2, 1, 1])


def row_counts(v):
    """partial and full arrays"""
    return sorted({1, (1 << v) - 1, 1 << v, max(1, (1 << v) - 3)})


def row_tables(s, n, seed):
    """One table per plane: write-shaped, random 1..5, constant, one row of 1 term beside one of 40."""
    rng = np.random.default_rng(seed)
    lone = [1] * n
    lone[n // 2] = 40
    return [write_shaped(s, n), [int(x) for x in rng.integers(1, 6, n)], [3] * n, lone]


def operands(n_bits, s, T, batch, seed):
    index = [rand_terms(n_bits, batch, sk, seed + k) for k, sk in enumerate(s)]
    arrays = [rand_terms(n_bits, batch, sum(t), seed + 80 + j) for j, t in enumerate(T)]
    return index, arrays


# -- the model's three forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", INDEX_TERMS, ids=str)
def test_the_three_model_forms_agree(s):
    n_bits, batch = 129, 2
    v = len(s)
    for n in row_counts(v):
        T = row_tables(s, n, 10 * v + n)
        index, arrays = operands(n_bits, s, T, batch, 10 * v + n)
        want = np_pick_rows(n_bits, index, arrays, T)
        fast = np_pick_rows_fast(n_bits, index, arrays, T)
        got = np_pick_rows_decoded(n_bits, index, arrays, T)
        for j, t in enumerate(T):
            assert want[j].shape[1] == out_terms(s, t) == sum(row_terms(s, r) * t[r] for r in range(n)), (n, j)
            assert np.array_equal(fast[j], want[j]), (n, j)
            assert np.array_equal(got[j], want[j]), (n, j)


def test_sizes_of_the_issue():
    """Fresh v = 3, n = 8 over a table written once from one-term planes: T = 17, 9, 9, 5, 9, 5, 5, 3 (A = 62), Tout =
    277; in general 2 * 5^v + 3^v."""
    T = write_shaped([1] * 3, 8)
    assert T == [17, 9, 9, 5, 9, 5, 5, 3] and sum(T) == 62 == array_terms([1] * 3, 8, 1, 1)
    assert out_terms([1] * 3, T) == 277
    for v in range(1, 9):
        assert out_terms([1] * v, write_shaped([1] * v, 1 << v)) == 2 * 5 ** v + 3 ** v


def test_constant_rows_are_each(lib):
    """T[r] = t for every row: Tout is t * csgn_uint_pick_terms, and the words are csgn_uint_pick EACH's."""
    for s in INDEX_TERMS:
        v = len(s)
        for n in row_counts(v):
            for t in (1, 3):
                rc, src, out = c_offsets(lib, v, s, n, [t] * n)
                assert rc == 0 and out[n] == t * c_pick_terms(lib, EACH, v, s, 1, n, 0), (s, n, t)
                assert src == [t * r for r in range(n + 1)]
    n_bits, s, n, t, batch = 65, [2, 1], 3, 2, 3
    index, arrays = operands(n_bits, s, [[t] * n] * 2, batch, 5)
    dl = arrays[0].shape[2]
    each = np_pick(n_bits, EACH, index, [a.reshape(batch * n, t, dl) for a in arrays], n)
    rows = np_pick_rows(n_bits, index, arrays, [[t] * n] * 2)
    for j in range(2):
        assert np.array_equal(each[j], rows[j]), j


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_offsets_agree_with_the_model(lib):
    """Every n for v <= 4, fresh and mixed index planes, the four kinds of table."""
    sweeps = [[1] * v for v in (1, 2, 3, 4)] + [[2], [3, 2], [2, 1, 3], [1, 2, 1, 1], [3, 1, 2, 2]]
    for s in sweeps:
        v = len(s)
        for n in range(1, (1 << v) + 1):
            for T in row_tables(s, n, 31 * v + n) + [write_shaped(s, n, 2, 3)]:
                rc, src, out = c_offsets(lib, v, s, n, T)
                assert rc == 0 and (src, out) == rows_offsets(s, T), (s, n, T)
    rc, src, out = c_offsets(lib, 3, [1] * 3, 8, write_shaped([1] * 3, 8))
    assert (rc, src[8], out[8]) == (0, 62, 277)
    rc, src, out = c_offsets(lib, 8, [1] * 8, 256, write_shaped([1] * 8, 256))
    assert (rc, src[256], out[256]) == (0, 13378, 2 * 5 ** 8 + 3 ** 8)


def test_offsets_invalid_and_not_wrapping(lib):
    one = [1] * 17
    assert c_offsets(lib, 3, one, 8, [1] * 8)[0] == 0
    assert c_offsets(lib, 0, one, 1, [1])[0] == -1                      # index width outside 1..16
    assert c_offsets(lib, 17, one, 8, [1] * 8)[0] == -1
    assert c_offsets(lib, 3, one, 0, [1])[0] == -1                      # rows outside 1..2^v
    assert c_offsets(lib, 3, one, 9, [1] * 9)[0] == -1
    assert c_offsets(lib, 3, None, 8, [1] * 8)[0] == -1                 # null pointers
    assert c_offsets(lib, 3, one, 8, None)[0] == -1
    assert lib.csgn_uint_pick_rows_offsets(3, u64s(one), 8, u64s([1] * 8), None, (C.c_uint64 * 9)()) == -1
    assert lib.csgn_uint_pick_rows_offsets(3, u64s(one), 8, u64s([1] * 8), (C.c_uint64 * 9)(), None) == -1
    assert c_offsets(lib, 3, [1, 0, 1], 8, [1] * 8)[0] == -1            # a plane of no terms
    assert c_offsets(lib, 3, one, 8, [1, 1, 0, 1, 1, 1, 1, 1])[0] == -1  # a row of no terms
    assert c_offsets(lib, 3, one, 8, [1] * 7 + [LIMIT])[0] == -1        # counts at 2^62
    assert c_offsets(lib, 1, [LIMIT], 2, [1, 1])[0] == -1
    assert c_offsets(lib, 4, [1 << 16] * 4, 16, [1] * 16)[0] == -1      # E saturates
    # v = 1, fresh: P = 2, 1.  2^60 terms a row: Tout = 3 * 2^60 fits; 2^61 in row 0: 2 * 2^61 = 2^62 does not
    rc, src, out = c_offsets(lib, 1, [1], 2, [1 << 60, 1 << 60])
    assert (rc, src[2], out[2]) == (0, 1 << 61, 3 << 60)
    assert c_offsets(lib, 1, [1], 2, [1 << 61, 1])[0] == -1
    assert c_offsets(lib, 1, [1], 2, [1, (1 << 62) - 2])[0] == -1       # the sum reaches 2^62: 2 + 2^62 - 2
    rc, src, out = c_offsets(lib, 1, [1], 2, [1, (1 << 62) - 3])
    assert (rc, out[2]) == (0, (1 << 62) - 1)
    assert c_offsets(lib, 1, [1], 2, [(1 << 63) + 1, 1])[0] == -1       # a product that would wrap to 2
    # E = 3^16: every row of 2^37 terms passes 2^62 in all (5.9e18), though no block (2^53 at most) does
    assert c_offsets(lib, 16, [1] * 16, 1 << 16, [1 << 37] * (1 << 16))[0] == -1
    rc, src, out = c_offsets(lib, 16, [1] * 16, 1 << 16, [1 << 30] * (1 << 16))
    assert (rc, src[-1], out[-1]) == (0, 1 << 46, 3 ** 16 << 30)


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
def element_operands(index, arrays, T, e=0):
    """One element's operands as flat words (compose_pick_rows' arguments)."""
    offs = [rows_offsets([], t)[0] for t in T]
    return ([x[e].ravel() for x in index],
            [[a[e, o[r]:o[r + 1]].ravel() for a, o in zip(arrays, offs)] for r in range(len(T[0]))])


@pytest.mark.parametrize("s", [x for x in INDEX_TERMS if len(x) <= 3], ids=str)
def test_definition_matches_reference(oracle, ref, s):
    n_bits, d = 65, 4
    v = len(s)
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    for n in row_counts(v):
        T = row_tables(s, n, 7 * v + n)
        index, arrays = operands(n_bits, s, T, 1, 1000 * v + n)
        x, rows = element_operands(index, arrays, T)
        add, mul = ref_ops(ref, n_bits, d)
        want = compose_pick_rows(x, rows, add, mul, one, zero)
        add, mul = oracle_ops(oracle, n_bits)
        got = compose_pick_rows(x, rows, add, mul, one, zero)
        words = np_pick_rows(n_bits, index, arrays, T)
        for j in range(len(T)):
            assert np.array_equal(got[j], want[j]), (n, j)
            assert np.array_equal(words[j][0].ravel(), want[j]), (n, j)


@pytest.mark.parametrize("n_bits,d", [(63, 4), (129, 8), (1247, 16)])
def test_definition_matches_reference_at_other_sizes(ref, n_bits, d):
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    s, T = [2, 1], [[3, 1, 4], [1, 5, 2]]
    index, arrays = operands(n_bits, s, T, 1, 77)
    x, rows = element_operands(index, arrays, T)
    add, mul = ref_ops(ref, n_bits, d)
    want = compose_pick_rows(x, rows, add, mul, one, zero)
    words = np_pick_rows(n_bits, index, arrays, T)
    for j in range(2):
        assert np.array_equal(words[j][0].ravel(), want[j]), j


@pytest.mark.parametrize("n_bits", [64, 63, 1247])
def test_definition_matches_oracle_batched(oracle, n_bits):
    """Element e with element e: every element of a batch against the oracle's operators on its own words."""
    s, n, batch = [2, 1, 3], 6, 3
    T = row_tables(s, n, 3)[:2]
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    add, mul = oracle_ops(oracle, n_bits)
    index, arrays = operands(n_bits, s, T, batch, 60)
    words = np_pick_rows(n_bits, index, arrays, T)
    for e in range(batch):
        x, rows = element_operands(index, arrays, T, e)
        want = compose_pick_rows(x, rows, add, mul, one, zero)
        for j in range(2):
            assert np.array_equal(words[j][e].ravel(), want[j]), (e, j)


# -- decryptions: the read that follows the write ----------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2, 3])
def test_read_after_write_decrypts(oracle, v):
    """np_write's planes go into np_pick_rows unmoved: reading at the written index gives the value, at another index
    the array's own row, and 0 where the read index is >= n."""
    n_bits, d, w = 127, 8, 3
    key, _ = oracle.keygen(n_bits, d, glibc_draws(570 + v, 64 * d + 64))
    rng = np.random.default_rng(v)
    for n in sorted({1, (1 << v) - 1, 1 << v}):
        wr = np.repeat(np.arange(1 << v, dtype=np.uint64), 1 << v)      # every (write index, read index)
        rd = np.tile(np.arange(1 << v, dtype=np.uint64), 1 << v)
        table = rng.integers(0, 1 << w, (len(wr), n)).astype(np.uint64)
        vals = rng.integers(0, 1 << w, len(wr)).astype(np.uint64)
        wi = encrypt_planes(oracle, n_bits, key, wr, v, 580 + v)
        ri = encrypt_planes(oracle, n_bits, key, rd, v, 583 + v)
        value = encrypt_planes(oracle, n_bits, key, vals, w, 585 + v)
        a = encrypt_planes(oracle, n_bits, key, table.ravel(), w, 590 + w + n)
        written = np_write(n_bits, wi, value, a, n)
        T = [write_shaped([1] * v, n)] * w
        got = decrypt_value(oracle, n_bits, key, np_pick_rows_fast(n_bits, ri, written, T))
        for e in range(len(wr)):
            after = [int(x) for x in table[e]]
            if wr[e] < n:
                after[int(wr[e])] = int(vals[e])
            assert int(got[e]) == clear_pick_rows(n, after, int(rd[e])), (v, n, e)
