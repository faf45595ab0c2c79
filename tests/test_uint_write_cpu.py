"""Encrypted arrays written at encrypted indices (csgn_uint_write*) on a box without a GPU: the three restatements of the
definition in tests/model_write.py against one another, the DEFINITION -- row r of plane j becomes (EQ(index, r) *
(value_j + d_{r,j})) + d_{r,j} -- pinned against the compiled reference and the oracle, the closed-form offsets of the
ragged rows against the C ABI, the argument checks in csgn_uint_read's order, the dispatch names and knob, the loud
failure without a device, and decryptions of every index.  The device side is tests/test_uint_write_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, const_term, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms, read_terms,  # noqa: F401
                         ref_ops, u64s)
from tests.model_write import (array_terms, c_write_offset, clear_write, compose_write, np_write, np_write_decoded,
                               np_write_fast, row_terms, write_offset, write_offset_by_rows, write_row_terms)

INDEX_TERMS = ([1], [1, 1], [1, 1, 1], [2, 1, 3], [3, 2], [1, 1, 1, 1], [1, 2, 1, 1])
VALUE_ARRAY_TERMS = ((1, 1), (2, 3), (3, 1))


def row_counts(v):
    """partial and full arrays"""
    return sorted({1, (1 << v) - 1, 1 << v, max(1, (1 << v) - 3)})


def operands(n_bits, s, n, tv, td, batch, seed):
    """w planes, one per entry of the lists tv / td"""
    index = [rand_terms(n_bits, batch, sk, seed + k) for k, sk in enumerate(s)]
    value = [rand_terms(n_bits, batch, t, seed + 40 + j) for j, t in enumerate(tv)]
    arrays = [rand_terms(n_bits, batch * n, t, seed + 80 + j) for j, t in enumerate(td)]
    return index, value, arrays


# -- the model's three forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", INDEX_TERMS, ids=str)
def test_the_three_model_forms_agree(s):
    n_bits, batch = 129, 2
    v = len(s)
    for n in row_counts(v):
        index, value, arrays = operands(n_bits, s, n, [1, 2, 3], [1, 3, 1], batch, 10 * v + n)
        want = np_write(n_bits, index, value, arrays, n)
        fast = np_write_fast(n_bits, index, value, arrays, n)
        got = np_write_decoded(n_bits, index, value, arrays, n)
        for j, (tv, td) in enumerate(VALUE_ARRAY_TERMS):
            assert want[j].shape[1] == array_terms(s, n, tv, td), (n, j)
            assert np.array_equal(fast[j], want[j]), (n, j)
            assert np.array_equal(got[j], want[j]), (n, j)


def test_sizes_of_the_issue():
    """Fresh planes: 2^zeros(r) * (tv + td) + td terms in row r; 62 terms per array at v = 3, n = 8 and 13 378 at v = 8,
    n = 256; the rows of an array add up to A; the offsets by rows equal the closed form."""
    for v in (1, 2, 3, 4):
        for r in range(1 << v):
            zeros = v - bin(r).count("1")
            assert write_row_terms([1] * v, r, 2, 3) == (1 << zeros) * 5 + 3
    assert array_terms([1] * 3, 8, 1, 1) == 62
    assert array_terms([1] * 8, 256, 1, 1) == 13378
    for s in INDEX_TERMS:
        for n in row_counts(len(s)):
            for tv, td in VALUE_ARRAY_TERMS:
                assert write_offset(s, 0, tv, td) == 0
                for r in range(n + 1):
                    assert write_offset(s, r, tv, td) == write_offset_by_rows(s, r, tv, td), (s, n, r)
                assert write_offset(s, n, tv, td) == array_terms(s, n, tv, td)
                assert sum(row_terms(s, r) for r in range(n)) == read_terms(s, n)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_offsets_agree_with_the_model(lib):
    """Every r of every n for v <= 4, fresh and mixed index planes."""
    sweeps = [[1] * v for v in (1, 2, 3, 4)] + [[2], [3, 2], [2, 1, 3], [1, 2, 1, 1], [3, 1, 2, 2]]
    for s in sweeps:
        v = len(s)
        for n in range(1, (1 << v) + 1):
            for tv, td in VALUE_ARRAY_TERMS + ((5, 7),):
                for r in range(n + 1):
                    assert c_write_offset(lib, v, s, n, r, tv, td) == write_offset(s, r, tv, td), (s, n, r, tv, td)
    assert c_write_offset(lib, 3, [1] * 3, 8, 8, 1, 1) == 62
    assert c_write_offset(lib, 8, [1] * 8, 256, 256, 1, 1) == 13378


def test_offsets_invalid_and_saturating(lib):
    one = [1] * 17
    assert c_write_offset(lib, 3, one, 8, 8, 1, 1) == 62
    assert c_write_offset(lib, 0, one, 1, 1, 1, 1) == 0                 # index width outside 1..16
    assert c_write_offset(lib, 17, one, 8, 8, 1, 1) == 0
    assert c_write_offset(lib, 3, one, 0, 0, 1, 1) == 0                 # rows outside 1..2^v
    assert c_write_offset(lib, 3, one, 9, 9, 1, 1) == 0
    assert c_write_offset(lib, 3, one, 8, 9, 1, 1) == 0                 # r past the rows
    assert c_write_offset(lib, 3, None, 8, 8, 1, 1) == 0                # null pointer
    assert c_write_offset(lib, 3, [1, 0, 1], 8, 8, 1, 1) == 0           # a plane of no terms
    assert c_write_offset(lib, 3, one, 8, 8, 0, 1) == 0
    assert c_write_offset(lib, 3, one, 8, 8, 1, 0) == 0
    assert c_write_offset(lib, 3, one, 8, 8, LIMIT, 1) == 0             # counts at 2^62
    assert c_write_offset(lib, 3, one, 8, 8, 1, LIMIT) == 0
    assert c_write_offset(lib, 1, [LIMIT], 2, 2, 1, 1) == 0
    assert c_write_offset(lib, 4, [1 << 16] * 4, 16, 16, 1, 1) == 0     # E saturates
    # E = 3^16 = 43 046 721 entries: times 2^36 terms a side the product passes 2^62, one entry below it does not
    E = 3 ** 16
    assert c_write_offset(lib, 16, [1] * 16, 1 << 16, 1 << 16, 1, 1) == 2 * E + (1 << 16)
    big = (LIMIT // E) // 2
    assert c_write_offset(lib, 16, [1] * 16, 1 << 16, 1 << 16, big, big) == 0
    small = (LIMIT - 1) // (2 * E + (1 << 16)) - 1
    assert c_write_offset(lib, 16, [1] * 16, 1 << 16, 1 << 16, small, small) == 2 * E * small + (1 << 16) * small
    assert c_write_offset(lib, 16, [1] * 16, 1 << 16, 1, big, big) == 2 * big * (1 << 16) + big   # row 0's 2^16 entries


def name(lib, n, v, s, rows, w, tv, td, batch=256):
    return lib.csgn_uint_write_kernel(n, batch, v, u64s(s), rows, w, u64s(tv) if tv is not None else None,
                                      u64s(td) if td is not None else None).decode()


def test_dispatch_names(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert "uint_write_fused" in names and names.index("uint_write_fused") < names.index("launch_blocks")
    knobs.unset("uint_write_fused")
    assert capi.get_tuning("uint_write_fused") == -1
    assert name(lib, 1247, 3, [1] * 3, 8, 2, [1, 2], [1, 3]) == "k_uint_write"      # per shape: fused for every shape
    assert name(lib, 1247, 3, [2, 1, 3], 5, 64, [2] * 64, [3] * 64, batch=1) == "k_uint_write"
    assert name(lib, 0, 3, [1] * 3, 8, 1, [1], [1]) == ""                # n_bits 0
    assert name(lib, 1247, 17, [1] * 17, 8, 1, [1], [1]) == ""           # bad index width
    assert name(lib, 1247, 3, [1] * 3, 8, 0, [1], [1]) == ""             # bad width
    assert name(lib, 1247, 3, [1] * 3, 8, 65, [1] * 65, [1] * 65) == ""
    assert name(lib, 1247, 3, [1] * 3, 0, 1, [1], [1]) == ""             # rows outside 1..2^v
    assert name(lib, 1247, 3, [1] * 3, 9, 1, [1], [1]) == ""
    assert name(lib, 1247, 3, [1, 0, 1], 8, 1, [1], [1]) == ""           # a plane of no terms
    assert name(lib, 1247, 3, [1] * 3, 8, 1, [0], [1]) == ""
    assert name(lib, 1247, 3, [1] * 3, 8, 1, [1], [0]) == ""
    assert name(lib, 1247, 3, [1] * 3, 8, 1, None, [1]) == ""
    knobs.set("uint_write_fused", 0)
    assert capi.get_tuning("uint_write_fused") == 0
    assert name(lib, 1247, 3, [1] * 3, 8, 2, [1, 2], [1, 3]) == "composed"
    assert name(lib, 1247, 3, [1] * 3, 8, 1, [1], [1], batch=1 << 29) == "k_uint_write"      # past the gather's counts
    assert name(lib, 1247, 3, [1] * 3, 8, 1, [1], [1], batch=(1 << 29) - 1) == "composed"
    knobs.set("uint_write_fused", 1)
    assert capi.get_tuning("uint_write_fused") == 1
    assert name(lib, 1247, 3, [1] * 3, 8, 2, [1, 2], [1, 3]) == "k_uint_write"


def test_the_knob_is_spelt_as_the_library_stores_it():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    assert '{"uint_write_fused", -1}' in source


def test_plan_figures(lib):
    """csgn_uint_write_plan: the tile of the fused form; the parts of QP entries cover the stream."""
    plan = (C.c_uint64 * 4)()
    one = u64s([1] * 8)
    assert lib.csgn_uint_write_plan(4096, 2, 3, one, 8, 2, one, one, 1, plan) == 0
    G, KC, QP, parts = (int(x) for x in plan)
    assert G >= 1 and KC == 32 and (parts - 1) * QP < 27 <= parts * QP
    assert lib.csgn_uint_write_plan(4096, 0, 3, one, 8, 2, one, one, 1, plan) == -1      # empty batch
    assert lib.csgn_uint_write_plan(4096, 2, 3, one, 9, 2, one, one, 1, plan) == -1      # rows
    assert lib.csgn_uint_write_plan(4096, 2, 3, one, 8, 2, one, one, 1, None) == -1


def host_pointers():
    buf = np.zeros(4096, dtype=np.uint64)
    ptrs = (C.c_void_p * 64)(*([buf.ctypes.data] * 64))
    return buf, ptrs, u64s([1] * 64)


def test_arguments_are_rejected_in_reads_order(lib):
    """Each call breaks TWO rules; the one csgn_uint_read reports for the same pair is the one csgn_uint_write reports:
    n_bits, index width, width, rows, host arrays, index terms, plane terms, sizes, then the device."""
    _, ptrs, one = host_pointers()

    def both(n_bits, batch, v, h_index, s, rows, w, h_planes, t):
        rd = lib.csgn_uint_read(n_bits, batch, v, h_index, s, rows, w, h_planes, t, ptrs, None)
        rd_text = lib.csgn_last_error().decode()
        wr = lib.csgn_uint_write(n_bits, batch, v, h_index, s, rows, w, h_planes, t, ptrs, t, ptrs, None)
        wr_text = lib.csgn_last_error().decode()
        assert rd == wr and rd in (-1, -2), (rd, wr, rd_text, wr_text)
        return rd_text, wr_text

    zero_s = u64s([1, 0, 1])
    zero_t = u64s([0] * 64)
    for args, word in (
            ((0, 4, 0, ptrs, one, 8, 8, ptrs, one), "n_bits"),                  # n_bits before the index width
            ((1 << 21, 4, 3, ptrs, one, 8, 8, ptrs, one), "16384 bytes"),
            ((1247, 4, 17, ptrs, one, 8, 0, ptrs, one), "index width"),         # index width before the width
            ((1247, 4, 3, ptrs, one, 9, 65, ptrs, one), "outside 1..64"),       # width before the rows
            ((1247, 4, 3, None, one, 9, 8, ptrs, one), "rows outside"),         # rows before the host arrays
            ((1247, 4, 3, None, zero_s, 8, 8, ptrs, one), "null host pointer"),  # host arrays before the index terms
            ((1247, 4, 3, ptrs, None, 8, 8, ptrs, zero_t), "null host pointer"),
            ((1247, 4, 3, ptrs, zero_s, 8, 8, ptrs, zero_t), "an index plane has no terms"),   # ... before plane terms
            ((1247, 1 << 52, 3, ptrs, one, 8, 8, ptrs, zero_t), "no terms"),    # plane terms before the sizes
            ((1247, 1 << 52, 3, ptrs, one, 8, 8, ptrs, one), "size overflows"),  # sizes before the device
    ):
        rd_text, wr_text = both(*args)
        assert word in rd_text or word.replace("no terms", "terms") in rd_text, (word, rd_text)
        assert word in wr_text or word.replace("no terms", "of 0 terms") in wr_text, (word, wr_text)
        assert rd_text.startswith("read:") == wr_text.startswith("write:"), (rd_text, wr_text)


def test_argument_errors(lib):
    _, ptrs, one = host_pointers()

    def write(n_bits=1247, batch=4, v=3, h_index=ptrs, s=one, rows=8, w=8, h_value=ptrs, tv=one, h_arrays=ptrs, td=one,
              h_out=ptrs):
        return lib.csgn_uint_write(n_bits, batch, v, h_index, s, rows, w, h_value, tv, h_arrays, td, h_out, None)

    assert write(n_bits=0) == -1
    assert write(v=0) == -1 and write(v=17) == -1
    assert write(w=0) == -1 and write(w=65) == -1
    assert write(rows=0) == -1 and write(rows=9) == -1
    for which in ("h_index", "s", "h_value", "tv", "h_arrays", "td", "h_out"):
        assert write(**{which: None}) == -1, which
    assert write(s=u64s([1, 0, 1])) == -1 and write(s=u64s([1, LIMIT, 1])) == -1
    assert write(tv=u64s([1, 0] + [1] * 6)) == -1 and write(td=u64s([1, 0] + [1] * 6)) == -1
    assert write(tv=u64s([LIMIT] * 8)) == -1 and write(td=u64s([LIMIT] * 8)) == -1
    # an array of 2^31 words or more: 3^16 entries * 2 terms * 20 words = 1.7e9 fits, 3 terms do not
    assert write(v=16, rows=1 << 16, w=1, tv=u64s([2])) == -2
    assert b"2^31" in lib.csgn_last_error()
    assert write(v=16, rows=1 << 16, w=1, td=u64s([2])) == -2
    assert write(batch=1 << 50) == -2                                    # batch times an array: 2^60 words
    assert write(tv=u64s([1 << 61] * 8), td=u64s([1 << 61] * 8)) == -2   # a sum that wraps is past every limit


def test_fails_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_uint_write_gpu.py covers the device")
    _, ptrs, one = host_pointers()
    rc = lib.csgn_uint_write(1247, 4, 3, ptrs, one, 8, 8, ptrs, one, ptrs, one, ptrs, None)
    assert rc == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert lib.csgn_uint_write(1247, 4, 3, ptrs, u64s([2, 1, 3]), 5, 2, ptrs, u64s([2, 3]), ptrs, u64s([3, 1]), ptrs,
                               None) == -3
    assert lib.csgn_uint_write(1247, 0, 3, ptrs, one, 8, 8, ptrs, one, ptrs, one, ptrs, None) == -3   # ... an empty batch too
    # v = 16, n = 2^16: (2 * 3^16 + 2^16) * 20 words = 1.72e9 < 2^31: the device is looked for
    assert lib.csgn_uint_write(1247, 4, 16, ptrs, one, 1 << 16, 1, ptrs, one, ptrs, one, ptrs, None) == -3


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
def element_operands(index, value, arrays, n, e=0):
    """One element's operands as flat words (compose_write's arguments)."""
    return ([x[e].ravel() for x in index], [x[e].ravel() for x in value],
            [[a[e * n + r].ravel() for a in arrays] for r in range(n)])


@pytest.mark.parametrize("s", [x for x in INDEX_TERMS if len(x) <= 3], ids=str)
def test_definition_matches_reference(oracle, ref, s):
    n_bits, d = 65, 4
    v = len(s)
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    dl = (n_bits + 63) // 64
    tv, td = [t[0] for t in VALUE_ARRAY_TERMS], [t[1] for t in VALUE_ARRAY_TERMS]
    for n in row_counts(v):
        index, value, arrays = operands(n_bits, s, n, tv, td, 1, 1000 * v + n)
        x, val, rows = element_operands(index, value, arrays, n)
        add, mul = ref_ops(ref, n_bits, d)
        want = compose_write(x, val, rows, add, mul, one, zero)
        add, mul = oracle_ops(oracle, n_bits)
        got = compose_write(x, val, rows, add, mul, one, zero)
        words = np_write(n_bits, index, value, arrays, n)
        for j in range(len(tv)):
            for r in range(n):
                assert np.array_equal(got[r][j], want[r][j]), (n, r, j)
                assert got[r][j].size == write_row_terms(s, r, tv[j], td[j]) * dl, (n, r, j)
                at = write_offset(s, r, tv[j], td[j])
                assert np.array_equal(words[j][0, at:at + got[r][j].size // dl].ravel(), got[r][j]), (n, r, j)


@pytest.mark.parametrize("n_bits,d", [(63, 4), (129, 8), (1247, 16)])
def test_definition_matches_reference_at_other_sizes(ref, n_bits, d):
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    s, n, tv, td = [2, 1], 3, [2, 1], [3, 1]
    index, value, arrays = operands(n_bits, s, n, tv, td, 1, 77)
    x, val, rows = element_operands(index, value, arrays, n)
    add, mul = ref_ops(ref, n_bits, d)
    want = compose_write(x, val, rows, add, mul, one, zero)
    words = np_write(n_bits, index, value, arrays, n)
    for j in range(2):
        assert np.array_equal(words[j][0].ravel(), np.concatenate([want[r][j] for r in range(n)])), j


@pytest.mark.parametrize("n_bits", [64, 63, 1247])
def test_definition_matches_oracle_batched(oracle, n_bits):
    """Element e with element e: every element of a batch against the oracle's operators on its own words."""
    s, n, tv, td, batch = [2, 1, 3], 6, [2, 1], [3, 1], 3
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    add, mul = oracle_ops(oracle, n_bits)
    index, value, arrays = operands(n_bits, s, n, tv, td, batch, 60)
    words = np_write(n_bits, index, value, arrays, n)
    for e in range(batch):
        x, val, rows = element_operands(index, value, arrays, n, e)
        want = compose_write(x, val, rows, add, mul, one, zero)
        for j in range(2):
            assert np.array_equal(words[j][e].ravel(), np.concatenate([want[r][j] for r in range(n)])), (e, j)


# -- decryptions -------------------------------------------------------------------------------------------------------
def decrypt_arrays(oracle, n_bits, key, outs, s, n, tv, td):
    """Output planes words[batch, A, dL] -> integers[batch, n], row by row through the offsets."""
    got = np.zeros((outs[0].shape[0], n), dtype=np.uint64)
    for r in range(n):
        lo, hi = write_offset(s, r, tv, td), write_offset(s, r + 1, tv, td)
        got[:, r] = decrypt_value(oracle, n_bits, key, [o[:, lo:hi, :] for o in outs])
    return got


@pytest.mark.parametrize("v", [1, 2, 3])
def test_every_index_decrypts(oracle, v):
    n_bits, d, w = 127, 8, 3
    key, _ = oracle.keygen(n_bits, d, glibc_draws(470 + v, 64 * d + 64))
    rng = np.random.default_rng(v)
    for n in sorted({1, (1 << v) - 1, 1 << v}):
        ds = np.arange(1 << v, dtype=np.uint64)                         # every index, past n too
        arrays = rng.integers(0, 1 << w, (len(ds), n)).astype(np.uint64)
        vals = rng.integers(0, 1 << w, len(ds)).astype(np.uint64)
        index = encrypt_planes(oracle, n_bits, key, ds, v, 480 + v)
        value = encrypt_planes(oracle, n_bits, key, vals, w, 485 + v)
        a = encrypt_planes(oracle, n_bits, key, arrays.ravel(), w, 490 + w + n)
        got = decrypt_arrays(oracle, n_bits, key, np_write(n_bits, index, value, a, n), [1] * v, n, 1, 1)
        for e in range(len(ds)):
            assert [int(x) for x in got[e]] == clear_write(n, arrays[e], int(ds[e]), vals[e]), (v, n, e)
