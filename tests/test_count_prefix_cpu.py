"""Running counts of encrypted bits (csgn_count_prefix*) on a box without a GPU: the row offsets against their sums and
their zeros, the argument checks and their order, the loud failure without a device, and the DEFINITION -- row r of
plane j the count of the group's first r + 1 - exclusive inputs, word for word, or the zero term -- pinned against the
oracle and the compiled reference, with decryptions under random keys.  The device side is
tests/test_count_prefix_gpu.py."""
import ctypes as C
from math import comb

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import INVALID, LIMIT, NO_DEVICE, UNSUPPORTED, decrypt_bits, lib, oracle_ops, rand_terms, ref_ops  # noqa: F401
from tests.model_count import compose_count
from tests.model_count_prefix import np_count_prefix, prefix_offset, row_inputs


def js_array(js):
    return (C.c_uint64 * max(len(js), 1))(*js)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_offsets_against_their_sums(lib):
    for g in range(1, 41):
        for t in (1, 2, 3):
            for j in range(8):
                for ex in (0, 1):
                    for r in range(g + 2):
                        assert lib.csgn_count_prefix_offset(g, t, j, ex, r) == prefix_offset(g, t, j, ex, r), (g, t, j, ex, r)
    # the term counts the header names
    assert [lib.csgn_count_prefix_offset(16, 1, j, 0, 16) for j in range(5)] == [136, 681, 6191, 24317, 16]
    assert [lib.csgn_count_prefix_offset(64, 1, j, 0, 64) for j in (0, 1)] == [2080, 43681]
    # the closed forms: inclusive min(r, m - 1) + C(r + 1, m + 1) t^m, exclusive min(r, m) + C(r, m + 1) t^m
    assert lib.csgn_count_prefix_offset(12, 3, 2, 0, 9) == 3 + comb(10, 5) * 81
    assert lib.csgn_count_prefix_offset(12, 3, 2, 1, 9) == 4 + comb(9, 5) * 81


def test_offset_zeros(lib):
    off = lib.csgn_count_prefix_offset
    # bad shapes
    for bad in [(0, 1, 0, 0, 0), (5, 0, 0, 0, 5), (5, 1, 0, 2, 5), (5, 1, 0, 0, 6), (5, LIMIT, 0, 0, 5), (LIMIT, 1, 0, 0, 1),
                ((1 << 64) - 1, 1, 0, 0, (1 << 64) - 1)]:
        assert off(*bad) == 0 == prefix_offset(*bad), bad
    # j > 6, 2^j > group - exclusive
    assert off(200, 1, 7, 0, 200) == 0 and off(64, 1, 6, 0, 64) == 64 and off(64, 1, 6, 1, 64) == 0
    assert off(4, 1, 2, 0, 4) == 4 and off(4, 1, 2, 1, 4) == 0 and off(1, 1, 0, 1, 1) == 0 and off(1, 1, 0, 0, 1) == 1
    # r = 0: the offset is 0
    assert off(8, 1, 1, 0, 0) == 0 and off(8, 1, 1, 1, 0) == 0
    # saturation: t^2 = 2^62; the rows before the first pair are still one term each
    assert off(4, 1 << 31, 1, 0, 4) == 0 == prefix_offset(4, 1 << 31, 1, 0, 4)
    assert off(4, 1 << 31, 1, 0, 1) == 1 == prefix_offset(4, 1 << 31, 1, 0, 1)
    assert off(4, (1 << 31) - 1, 1, 0, 2) == 1 + ((1 << 31) - 1) ** 2
    assert off(4, 1 << 31, 0, 0, 4) == 10 << 31
    # g = 64 at plane 5: C(65, 33) lies below 2^62 and comes out exact; with two terms an input nothing fits
    assert 31 + comb(65, 33) < LIMIT
    assert off(64, 1, 5, 0, 64) == 31 + comb(65, 33) == prefix_offset(64, 1, 5, 0, 64)
    assert off(64, 1, 5, 1, 64) == 32 + comb(64, 33) == prefix_offset(64, 1, 5, 1, 64)
    assert off(64, 2, 5, 0, 64) == 0 == prefix_offset(64, 2, 5, 0, 64)
    assert off(66, 1, 5, 0, 66) == 0 == prefix_offset(66, 1, 5, 0, 66)
    assert off(66, 1, 5, 0, 40) == 31 + comb(41, 33)


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits; count, group, t, exclusive, n_in, n_out, the host
    pointers and the planes (INVALID); 2^31 words per row element and 2^60 per plane (UNSUPPORTED, computed without
    wrap-around); null device pointers (INVALID); and only then the device (NO_DEVICE on a box without one; with one,
    the calls that pass every check are not made: their pointers are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(8, dtype=np.uint64)
    p = buf.ctypes.data

    def ptrs(n, null_at=None):
        return (C.c_void_p * max(n, 1))(*[None if i == null_at else p for i in range(max(n, 1))])

    def cnt(n=1247, count=2, g=8, t=1, ex=0, n_in=1, js=(1, 2), ins=0, outs=0, h_js=0, null_in=None, null_out=None):
        h_in = ptrs(n_in if 0 < n_in <= 64 else 1, null_in) if ins == 0 else ins
        h_out = ptrs(len(js), null_out) if outs == 0 else outs
        return lib.csgn_count_prefix(n, count, g, t, ex, h_in, n_in, len(js), js_array(js) if h_js == 0 else h_js, h_out,
                                     None)

    # each failing check wins over every later one
    assert cnt(n=0, count=0, null_in=0) == INVALID                     # n_bits
    assert b"n_bits" in lib.csgn_last_error()
    assert cnt(n=131073, count=0) == UNSUPPORTED
    for bad in [dict(count=0), dict(g=0), dict(t=0), dict(t=LIMIT), dict(t=(1 << 64) - 1), dict(ex=2), dict(ex=1 << 63),
                dict(n_in=0), dict(n_in=3), dict(g=65, n_in=65), dict(g=1, n_in=1, js=(1,)), dict(g=1, ex=1, js=(0,)),
                dict(js=()), dict(js=(2, 1)), dict(js=(1, 1)), dict(js=(4,)), dict(js=(7,)), dict(js=(64,)),
                dict(g=4, js=(2,), ex=1), dict(g=64, n_in=64, js=(6,), ex=1), dict(ins=None), dict(outs=None),
                dict(h_js=None)]:
        # ... over the sizes and the device pointers
        assert cnt(**dict(dict(null_in=0, null_out=0), **bad)) == INVALID, bad
    assert cnt(g=66, js=(2, 1, 5), null_in=0) == INVALID
    # sizes, before the device pointers: 2^31 words per element of the last row ...
    dl = 20
    assert cnt(g=64, js=(1, 3), null_in=0) == UNSUPPORTED              # C(64, 8) * 20 words
    assert b"per element" in lib.csgn_last_error()
    assert cnt(g=66, js=(5,), null_out=0) == UNSUPPORTED               # C(66, 32) is past 2^62
    assert cnt(g=66, js=(5,), ex=1, n=64, null_out=0) == UNSUPPORTED   # C(65, 32) is not, but past 2^31
    assert cnt(g=2, t=LIMIT - 1, js=(0,), null_in=0) == UNSUPPORTED
    assert cnt(g=2, t=1 << 31, js=(1,), n=64, null_in=0) == UNSUPPORTED            # t^2 = 2^62
    assert cnt(g=8, t=1 << 16, js=(2,), n=64, null_in=0) == UNSUPPORTED            # t^4 wraps to 0
    edge = (1 << 31) // dl                                             # the last row's g * dL >= 2^31 from here on
    assert cnt(g=edge + 1, js=(0,), null_in=0) == UNSUPPORTED
    assert cnt(g=edge + 2, js=(0,), ex=1, null_in=0) == UNSUPPORTED
    assert cnt(g=65537, js=(1,), n=64, null_in=0) == UNSUPPORTED       # C(65537, 2) = 2^31 + 32768
    # ... and 2^60 words per plane: A_0 of g = 2 is 3 terms, inclusive
    assert cnt(count=1 << 56, g=2, js=(0, 1), null_in=0) == UNSUPPORTED            # 2^56 * 3 * 20
    assert b"size overflows" in lib.csgn_last_error()
    assert cnt(count=1 << 59, g=2, js=(0,), n=64, null_in=0) == UNSUPPORTED        # 3 * 2^59
    assert cnt(count=1 << 59, g=2, js=(0,), ex=1, n=64, null_in=0) == UNSUPPORTED  # 2 * 2^59 = 2^60 exactly
    assert cnt(count=1 << 63, g=2, js=(0,), n=64, null_in=0) == UNSUPPORTED        # count * A wraps
    # null device pointers, before the device
    assert cnt(null_in=0) == INVALID
    assert b"null device pointer" in lib.csgn_last_error()
    assert cnt(null_out=1) == INVALID and cnt(n_in=8, null_in=7) == INVALID
    assert cnt(count=1 << 58, g=2, js=(0,), ex=1, n=64, null_in=0) == INVALID      # 2^59 words pass the size check
    assert cnt(g=65536, js=(1,), n=64, null_out=0) == INVALID                      # C(65536, 2) = 2^31 - 32768
    assert cnt(g=65537, js=(1,), ex=1, n=64, null_out=0) == INVALID
    if gpu:
        return
    # no device: every call that passes the checks above
    assert cnt() == NO_DEVICE
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert cnt(ex=1) == NO_DEVICE and cnt(n_in=8) == NO_DEVICE and cnt(g=64, n_in=64, js=(0, 1, 6)) == NO_DEVICE
    assert cnt(g=65, js=(1, 6)) == NO_DEVICE and cnt(g=65, ex=1, js=(1, 6)) == NO_DEVICE
    assert cnt(g=65536, js=(1,), n=64) == NO_DEVICE


# -- the definition against the oracle and the genuine reference -----------------------------------------------------
SHAPES = [(g, t) for g in range(1, 6) for t in (1, 2)]
SHAPE_IDS = ["g%d_t%d" % s for s in SHAPES]


def check_definition(ops, n, g, t):
    """Every row and plane of the model is the composition over the prefix: the left-nested sum over the subsets, in the
    nested loops' order, of the left-nested products -- and the zero term where the prefix is shorter than 2^j."""
    count = 2
    dl = (n + 63) // 64
    x = rand_terms(n, count * g, t, 2000 * n + 10 * g + t)
    planes = [np.ascontiguousarray(x.reshape(count, g, t, -1)[:, i]) for i in range(g)]
    for ex in (0, 1):
        js = [j for j in range(7) if (1 << j) <= g - ex]
        words = np_count_prefix(x, g, js, ex)
        by_planes = np_count_prefix(planes, g, js, ex, "planes")
        for j, rows, rows_p in zip(js, words, by_planes):
            assert len(rows) == g
            for r in range(g):
                assert np.array_equal(rows[r], rows_p[r]), (ex, j, r)             # both layouts: the same words
                nr = row_inputs(r, ex)
                if (1 << j) > nr:
                    assert rows[r].shape == (count, 1, dl) and not rows[r].any(), (ex, j, r)
                    continue
                for q in range(count):
                    got = compose_count(ops, [x[q * g + i].ravel() for i in range(nr)], j)
                    assert got.size == rows[r][q].size and np.array_equal(rows[r][q].ravel(), got), (ex, j, r, q)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_rows_are_the_composition_by_the_oracle(oracle, shape):
    check_definition(oracle_ops(oracle, 63), 63, *shape)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_rows_are_the_composition_by_the_reference(ref, shape):
    check_definition(ref_ops(ref, 129, 8), 129, *shape)


# -- decryptions -------------------------------------------------------------------------------------------------------
def encrypt_bits(oracle, n, key, bits, seed):
    flat = np.asarray(bits, dtype=np.uint8).ravel()
    dl = (n + 63) // 64
    return oracle.encrypt_seq(n, key, flat, glibc_draws(seed, flat.size * (n + 2)))[0].reshape(flat.size, 1, dl)


@pytest.mark.parametrize("g", range(1, 7))
def test_rows_decrypt_to_the_prefix_popcount(oracle, g):
    """Every mask of g bits, both scans: row r decrypts to the number of ones among its prefix, modulo 2^planes."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(800 + g, 64 * d + 64))
    values = np.arange(1 << g, dtype=np.uint64)
    bits = ((values[:, None] >> np.arange(g, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)   # [count, g]
    x = encrypt_bits(oracle, n, key, bits, 810 + g)
    for ex in (0, 1):
        js = [j for j in range(7) if (1 << j) <= g - ex]
        if not js:
            continue
        outs = np_count_prefix(x, g, js, ex)
        for r in range(g):
            got = np.zeros(len(values), dtype=np.uint64)
            for j, rows in zip(js, outs):
                got |= decrypt_bits(oracle, n, key, rows[r]).astype(np.uint64) << np.uint64(j)
            want = bits[:, :row_inputs(r, ex)].sum(axis=1).astype(np.uint64) & np.uint64((1 << len(js)) - 1)
            assert np.array_equal(got, want), (ex, r)
