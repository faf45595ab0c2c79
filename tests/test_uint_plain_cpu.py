"""Comparisons of bit-sliced integers against a PUBLIC constant (csgn_uint_plain_*) on a box without a GPU: the term
counts, the dispatch names and knob, the loud failure without a device, the DEFINITION of all six comparisons -- a
composition of the reference's operator+ / operator* with ONE and ZERO -- pinned against the compiled reference and the
oracle, and decryptions under random keys, which equal clear comparisons and today's route through constant(k).  The
device side is tests/test_uint_plain_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (CLEAR, CMPS, EQ, GE, GT, LE, LT, NE, compose_plain, const_term, decrypt_bits, encrypt_planes,
                         full_width_cases, lib, np_plain, np_uint_eq, np_uint_lt, oracle_ops, plain_terms, rand_terms,
                         ref_ops, u64s)


def edge_ks(w, rng):
    top = (1 << w) - 1
    ks = {0, 1, top, 1 << (w - 1), top ^ 1, 0x5555555555555555 & top, 0xAAAAAAAAAAAAAAAA & top}
    ks.update(int(rng.integers(0, 1 << min(w, 63))) for _ in range(3))
    return sorted(x for x in ks if x <= top)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_plain_terms_formulas(lib):
    rng = np.random.default_rng(5)
    for w in range(1, 65):
        for ts in ([1] * w, [int(x) for x in rng.integers(1, 4, w)], [2] * w):
            for k in edge_ks(w, rng):
                for cmp in CMPS.values():
                    want = plain_terms(cmp, w, k, ts)
                    assert lib.csgn_uint_plain_terms(cmp, w, k, u64s(ts)) == want, (cmp, w, k, ts)


def test_plain_terms_fresh_planes():
    """The sizes of the issue for fresh 1-term planes."""
    for w in range(1, 11):
        for k in range(1 << w):
            zeros = w - bin(k).count("1")
            assert plain_terms(EQ, w, k, [1] * w) == 2 ** zeros
            assert plain_terms(NE, w, k, [1] * w) == 2 ** zeros + 1
            assert plain_terms(LT, w, k, [1] * w) <= 2 ** w
            assert plain_terms(GT, w, k, [1] * w) <= 2 ** w - 1
    assert plain_terms(LT, 8, 1, [1] * 8) == 256 and plain_terms(LT, 8, 255, [1] * 8) == 16 and plain_terms(EQ, 16, 0, [1] * 16) == 65536


def test_plain_terms_invalid(lib):
    one = u64s([1] * 64)
    for bad in (0, 7, -1, 100):
        assert lib.csgn_uint_plain_terms(bad, 4, 3, one) == 0
    assert lib.csgn_uint_plain_terms(EQ, 0, 0, one) == 0                  # width outside 1..64
    assert lib.csgn_uint_plain_terms(EQ, 65, 0, one) == 0
    assert lib.csgn_uint_plain_terms(EQ, 4, 16, one) == 0                 # k >= 2^w
    assert lib.csgn_uint_plain_terms(LT, 8, 1 << 40, one) == 0
    assert lib.csgn_uint_plain_terms(EQ, 64, (1 << 64) - 1, one) == 1     # every k fits 64 bits
    assert lib.csgn_uint_plain_terms(EQ, 3, 0, u64s([1, 0, 1])) == 0       # a plane of no terms
    assert lib.csgn_uint_plain_terms(EQ, 2, 0, None) == 0
    # overflow: 2^62 or more terms
    assert lib.csgn_uint_plain_terms(EQ, 62, 0, one) == 0
    assert lib.csgn_uint_plain_terms(EQ, 61, 0, one) == 1 << 61
    assert lib.csgn_uint_plain_terms(LT, 64, 1, one) == 0 and lib.csgn_uint_plain_terms(LT, 64, (1 << 64) - 1, one) == 128
    assert lib.csgn_uint_plain_terms(GT, 2, 0, u64s([1 << 40, 1 << 40])) == 0
    assert lib.csgn_uint_plain_terms(EQ, 1, 1, u64s([(1 << 64) - 1])) == 0


def sweep_term_vectors(w, rng):
    """Term vectors of 65 counts (the first w are read): small ones, a plane of no terms, counts at 2^62 and next to it,
    and counts whose products cross 2^62 part of the way up the chain."""
    j = int(rng.integers(0, max(w, 1)))
    out = [[1] * 65, [2] * 65, [int(x) for x in rng.integers(1, 4, 65)], [1 << 31] * 65, [(1 << 64) - 1] * 65]
    for special in (0, (1 << 62) - 1, 1 << 62, (1 << 62) + 1, 1 << 40):
        ts = [int(x) for x in rng.integers(1, 3, 65)]
        ts[j] = special
        out.append(ts)
    return out


def sweep_constants(w, rng):
    """Constants of the sweep, all below 2^64: the ends, mixed bits, and, below 64 bits, some that do not fit."""
    top = (1 << min(max(w, 1), 64)) - 1
    ks = {0, 1, top, top - 1, top >> 1, 0x5555555555555555 & top, 0xAAAAAAAAAAAAAAAA & top,
          int(rng.integers(0, 1 << 62)) & top}
    if w < 64:
        ks.update({top + 1, (top + 1) | 1, 1 << 63})
    return sorted(ks)


SWEEP_WIDTHS = (0, 1, 2, 3, 5, 8, 16, 31, 32, 33, 62, 63, 64, 65)


def test_plain_terms_sweep(lib):
    """csgn_uint_plain_terms over widths 0..65, constants that fit and do not, and term vectors with a 0, counts at
    2^62 and overflowing products: the model's count, and 0 for whatever include/csgn_hip.h calls invalid."""
    rng = np.random.default_rng(17)
    for w in SWEEP_WIDTHS:
        for ts in sweep_term_vectors(w, rng):
            for k in sweep_constants(w, rng):
                valid = 1 <= w <= 64 and k >> w == 0 and all(0 < t < (1 << 62) for t in ts[:w])
                for cmp in CMPS.values():
                    want = plain_terms(cmp, w, k, ts[:w]) if valid else 0
                    assert lib.csgn_uint_plain_terms(cmp, w, k, u64s(ts)) == want, (cmp, w, k, ts[:w])


def test_plain_dispatch_names(lib, knobs):
    knobs.unset("uint_plain_fused")

    def name(cmp, w, k, ts=None):
        return lib.csgn_uint_plain_kernel(1247, cmp, 1 << 16, w, k, u64s(ts or [1] * w)).decode()

    for cmp in CMPS.values():
        assert name(cmp, 8, 77) == "k_uint_plain", cmp
        assert name(cmp, 16, 4711) == "k_uint_plain", cmp
        assert name(cmp, 1, 1) == "composed", cmp                          # one copy and a constant
    assert name(LT, 8, 0) == "composed" and name(GE, 8, 0) == "composed"  # ZERO (then ONE)
    assert name(GT, 8, 255) == "composed" and name(LE, 8, 255) == "composed"
    assert name(EQ, 4, 16) == "" and name(9, 4, 1) == ""
    knobs.set("uint_plain_fused", 1)
    assert name(EQ, 1, 1) == "k_uint_plain" and name(LT, 8, 0) == "k_uint_plain"
    knobs.set("uint_plain_fused", 0)
    assert name(EQ, 8, 77) == "composed" and name(GT, 16, 4711, [2] * 16) == "composed"


def test_plain_fails_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_uint_plain_gpu.py covers the device")
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    planes = (C.c_void_p * 64)(*([p] * 64))
    one = u64s([1] * 64)
    rc = lib.csgn_uint_plain(1247, EQ, 4, 8, 77, planes, one, p, None)
    assert rc == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert lib.csgn_uint_plain(1247, LT, 4, 8, 0, planes, one, p, None) == -3
    # argument errors are reported before the device is looked for
    assert lib.csgn_uint_plain(1247, 0, 4, 8, 77, planes, one, p, None) == -1
    assert lib.csgn_uint_plain(0, EQ, 4, 8, 77, planes, one, p, None) == -1
    assert lib.csgn_uint_plain(1247, EQ, 4, 8, 256, planes, one, p, None) == -1
    assert lib.csgn_uint_plain(1247, EQ, 4, 65, 0, planes, one, p, None) == -1
    assert lib.csgn_uint_plain(1247, EQ, 4, 3, 0, planes, u64s([1, 0, 1]), p, None) == -1
    assert lib.csgn_uint_plain(1247, EQ, 4, 3, 0, None, one, p, None) == -1
    # too large: 2^27 terms * 20 words per element exceed 2^31 words
    assert lib.csgn_uint_plain(1247, EQ, 4, 27, 0, planes, one, p, None) == -2
    assert lib.csgn_uint_plain(1247, EQ, 4, 26, 0, planes, one, p, None) == -3
    assert lib.csgn_uint_plain(1247, EQ, 1 << 56, 8, 0, planes, one, p, None) == -2     # batch


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("cmp", sorted(CMPS.values()))
@pytest.mark.parametrize("w,k,ts", [(1, 0, [1]), (1, 1, [2]), (3, 5, [1, 2, 1]), (4, 0, [1, 1, 2, 1]),
                                    (4, 15, [2, 1, 1, 1]), (4, 6, [1, 1, 1, 1]), (5, 18, [1, 2, 1, 1, 2])])
def test_plain_definition_matches_reference(oracle, ref, n, d, cmp, w, k, ts):
    planes = [rand_terms(n, 1, t, 40 + j)[0].ravel() for j, t in enumerate(ts)]
    add, mul = ref_ops(ref, n, d)
    want = compose_plain(cmp, planes, k, add, mul, const_term(n, 1), const_term(n, 0))
    add, mul = oracle_ops(oracle, n)
    got = compose_plain(cmp, planes, k, add, mul, const_term(n, 1), const_term(n, 0))
    words = np_plain(n, cmp, [p.reshape(1, t, -1) for p, t in zip(planes, ts)], k)
    dl = (n + 63) // 64
    assert np.array_equal(got, want)
    assert got.size == plain_terms(cmp, w, k, ts) * dl
    assert np.array_equal(words.ravel(), got)


@pytest.mark.parametrize("n", [64, 4096, 63, 1247])
@pytest.mark.parametrize("cmp", sorted(CMPS.values()))
def test_plain_definition_matches_oracle(oracle, n, cmp):
    ts, batch = [2, 1, 3, 1, 2, 1], 3
    planes = [rand_terms(n, batch, t, 60 + j) for j, t in enumerate(ts)]
    add, mul = oracle_ops(oracle, n)
    for k in (0, 1, 37, 63, 32, 21):
        words = np_plain(n, cmp, planes, k)
        for e in range(batch):
            want = compose_plain(cmp, [p[e].ravel() for p in planes], k, add, mul, const_term(n, 1), const_term(n, 0))
            assert np.array_equal(words[e].ravel(), want), (k, e)


# -- decryptions: clear comparisons, and today's route through constant(k) ------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_plain_truth_tables(oracle, w):
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(70 + w, 64 * d + 64))
    values = np.arange(1 << w, dtype=np.uint64)
    planes = encrypt_planes(oracle, n, key, values, w, 80 + w)
    for k in range(1 << w):
        const = [np.broadcast_to(const_term(n, (k >> j) & 1), (len(values), 1, planes[0].shape[2])) for j in range(w)]
        eq_today = decrypt_bits(oracle, n, key, np_uint_eq(n, planes, const))
        lt_today = decrypt_bits(oracle, n, key, np_uint_lt(n, planes, const))
        gt_today = decrypt_bits(oracle, n, key, np_uint_lt(n, const, planes))
        for cmp, f in CLEAR.items():
            got = decrypt_bits(oracle, n, key, np_plain(n, cmp, planes, k))
            assert np.array_equal(got, f(values, np.uint64(k))), (cmp, k)
        # the same bits as today's route (whose words differ: 3^w terms against at most 2^w)
        assert np.array_equal(decrypt_bits(oracle, n, key, np_plain(n, EQ, planes, k)), eq_today)
        assert np.array_equal(decrypt_bits(oracle, n, key, np_plain(n, LT, planes, k)), lt_today)
        assert np.array_equal(decrypt_bits(oracle, n, key, np_plain(n, GT, planes, k)), gt_today)
        assert np_plain(n, EQ, planes, k).shape[1] < 3 ** w or w == 1


@pytest.mark.parametrize("w,count", [(8, 40), (16, 3)])
def test_plain_random_pairs(oracle, w, count):
    n, d = 127, 8
    rng = np.random.default_rng(w)
    key, _ = oracle.keygen(n, d, glibc_draws(90 + w, 64 * d + 64))
    values = rng.integers(0, 1 << w, count).astype(np.uint64)
    planes = encrypt_planes(oracle, n, key, values, w, 95 + w)
    ks = [int(rng.integers(0, 1 << w)), int(values[0]), (1 << w) - 1 - 0x10, 1 << (w - 1)]
    for k in ks:
        for cmp, f in CLEAR.items():
            if w == 16 and cmp in (EQ, NE) and bin(k).count("1") < 6:
                continue                                              # 2^(zeros of k) terms: kept to 2^10 here
            got = decrypt_bits(oracle, n, key, np_plain(n, cmp, planes, k))
            assert np.array_equal(got, f(values, np.uint64(k))), (cmp, k)


@pytest.mark.parametrize("n", [65, 1247])
def test_plain_definition_at_64_bits(lib, oracle, n):
    """np_plain at w = 64 (k and values at and above 2^63 are Python / uint64 integers throughout): as many terms as
    csgn_uint_plain_terms says, the words of the composition through the oracle's operators, and decryptions equal to
    clear uint64 comparisons."""
    w, batch = 64, 2
    planes = [rand_terms(n, batch, 1, 900 + j) for j in range(w)]
    add, mul = oracle_ops(oracle, n)
    for cmp, k in full_width_cases(w):
        words = np_plain(n, cmp, planes, k)
        assert words.shape[1] == lib.csgn_uint_plain_terms(cmp, w, k, u64s([1] * w)) == plain_terms(cmp, w, k, [1] * w)
        if words.shape[1] <= 256:
            want = compose_plain(cmp, [p[1].ravel() for p in planes], k, add, mul, const_term(n, 1), const_term(n, 0))
            assert np.array_equal(words[1].ravel(), want), (cmp, k)
    d = 8
    key, _ = oracle.keygen(n, d, glibc_draws(64, 64 * d + 64))
    values = np.array([0, 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 2, (1 << 63) - 1, (1 << 63) + 1, 0x0123456789ABCDEF],
                      dtype=np.uint64)
    planes = encrypt_planes(oracle, n, key, values, w, 640)
    for k in (0, 1, 1 << 63, (1 << 63) - 1, (1 << 64) - 1, (1 << 64) - 2):
        for cmp, f in CLEAR.items():
            if 0 < plain_terms(cmp, w, k, [1] * w) <= 4096:
                got = decrypt_bits(oracle, n, key, np_plain(n, cmp, planes, k))
                assert np.array_equal(got, f(values, np.uint64(k))), (cmp, k)
