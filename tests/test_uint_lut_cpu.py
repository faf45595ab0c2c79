"""Public lookup tables on bit-sliced integers (csgn_uint_lut_*) on a box without a GPU: the ANF, the term counts, the
argument checks, the dispatch names and knob, the loud failure without a device, and the DEFINITION -- the table's
algebraic normal form, a composition of the reference's operator+ / operator* with ONE and ZERO -- pinned against the
compiled reference and the oracle, with decryptions under random keys equal to the table.  The device side is
tests/test_uint_lut_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (EQ, aes_sbox, c_terms, compose_lut, const_term, decrypt_bits, decrypt_value, encrypt_planes,
                         lib, lut_terms, np_add, np_anf, np_lut, np_plain, oracle_ops, rand_terms, random_table,
                         ref_ops, u64s)


# -- the definition, over any (add, mul, one, zero) ---------------------------------------------------------------------
def monomials(table, w, j):
    anf = np_anf(table, w)
    return [S for S in range(1 << w) if (anf[S] >> j) & 1]


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,m", [(1, 1), (3, 2), (4, 4), (8, 8), (8, 64), (12, 3), (16, 1)])
def test_anf_is_the_mobius_transform(lib, w, m):
    table = random_table(w, m, w * 100 + m)
    anf = (C.c_uint64 * (1 << w))()
    assert lib.csgn_uint_lut_anf(w, m, u64s(table), anf) == 0
    got = [int(v) for v in anf]
    # a direct numpy transform: butterflies over the whole uint64 word
    a = np.array(table, dtype=np.uint64)
    for i in range(w):
        a = a.reshape(-1, 2, 1 << i)
        a[:, 1, :] ^= a[:, 0, :]
        a = a.reshape(-1)
    assert got == [int(v) for v in a]
    # the transform is its own inverse: evaluating the ANF gives the table back
    back = [0] * (1 << w)
    for x in range(1 << w):
        for S in range(1 << w):
            if S & x == S:
                back[x] ^= got[S]
        if w > 8:
            break
    if w <= 8:
        assert back == table
    assert np_anf(got, w) == table


def test_anf_of_known_tables(lib):
    w = 8
    ident = list(range(256))
    anf = np_anf(ident, w)
    assert all(anf[S] == (S if S & (S - 1) == 0 and S else 0) for S in range(256))   # out_j = a_j
    assert np_anf([0] * 16, 4) == [0] * 16
    assert np_anf([15] * 16, 4) == [15] + [0] * 15                                     # out_j = ONE
    sbox = aes_sbox()
    assert sbox[0] == 0x63 and sbox[1] == 0x7C and sbox[0x53] == 0xED and len(set(sbox)) == 256
    counts = [len(monomials(sbox, 8, j)) for j in range(8)]
    assert all(100 <= c <= 160 for c in counts), counts


def test_terms_formulas(lib):
    rng = np.random.default_rng(7)
    for w, m in [(1, 1), (2, 3), (4, 4), (5, 8), (8, 8), (8, 64)]:
        table = random_table(w, m, w + m)
        for t in ([1] * w, [int(x) for x in rng.integers(1, 4, w)], [2] * w, [3] + [1] * (w - 1)):
            rc, got = c_terms(lib, table, w, m, t)
            assert rc == 0
            assert got == lut_terms(table, w, m, t), (w, m, t)
            if t == [1] * w:
                assert got == [max(1, len(monomials(table, w, j))) for j in range(m)]
    # fresh planes: at most 2^w; the identity is one term, the constants one term
    assert c_terms(lib, list(range(16)), 4, 4, [1] * 4) == (0, [1, 1, 1, 1])
    assert c_terms(lib, list(range(16)), 4, 4, [3, 1, 2, 5]) == (0, [3, 1, 2, 5])
    assert c_terms(lib, [0] * 16, 4, 4, [2] * 4) == (0, [1] * 4)
    assert c_terms(lib, [15] * 16, 4, 4, [2] * 4) == (0, [1] * 4)
    assert c_terms(lib, [1] + [0] * 65535, 16, 1, [1] * 16)[1] == [1 << 16]      # x == 0: every monomial


def test_terms_invalid(lib):
    one = [1] * 16
    assert c_terms(lib, [0, 1], 0, 1, one)[0] == -1                     # in_width outside 1..16
    assert c_terms(lib, [0] * (1 << 17), 17, 1, one)[0] == -1
    assert c_terms(lib, [0, 1], 1, 0, one)[0] == -1                     # out_width outside 1..64
    assert c_terms(lib, [0, 1], 1, 65, one)[0] == -1
    assert c_terms(lib, [0, 2], 1, 1, one)[0] == -1                     # a value >= 2^out_width
    assert c_terms(lib, [0, (1 << 64) - 1], 1, 64, one)[0] == 0
    assert c_terms(lib, [0, 1, 2, 3], 2, 2, [1, 0])[0] == -1            # a plane of no terms
    out = (C.c_uint64 * 1)()
    assert lib.csgn_uint_lut_terms(1, 1, None, u64s(one), out) == -1
    assert lib.csgn_uint_lut_terms(1, 1, u64s([0, 1]), None, out) == -1
    assert lib.csgn_uint_lut_anf(1, 1, u64s([0, 2]), (C.c_uint64 * 2)()) == -1
    # overflow: 2^62 terms or more
    top = [0] * 15 + [1]                                                 # out = a0 a1 a2 a3: t^4 terms
    assert c_terms(lib, top, 4, 1, [1 << 16] * 4)[0] == -1
    assert c_terms(lib, top, 4, 1, [1 << 15, 1 << 15, 1 << 15, 1 << 17])[0] == -1
    assert c_terms(lib, top, 4, 1, [1 << 15, 1 << 15, 1 << 15, (1 << 17) - 1]) == (0, [(1 << 62) - (1 << 45)])


def test_dispatch_names(lib, knobs):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_uint_lut_gpu.py names the forms of a compiled table")
    knobs.unset("uint_lut_fused")
    assert lib.csgn_uint_lut_kernel(1247, None, 1) == b""
    from csgn_amd import capi
    assert "uint_lut_fused" in capi.tuning_names()
    knobs.set("uint_lut_fused", 0)
    assert capi.get_tuning("uint_lut_fused") == 0


def test_fails_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_uint_lut_gpu.py covers the device")
    handle = C.c_void_p()
    rc = lib.csgn_uint_lut_create(8, 8, u64s(aes_sbox()), u64s([1] * 8), C.byref(handle))
    assert rc == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert handle.value is None
    # argument errors are reported before the device is looked for
    assert lib.csgn_uint_lut_create(8, 7, u64s(aes_sbox()), u64s([1] * 8), C.byref(handle)) == -1
    assert lib.csgn_uint_lut_create(8, 8, u64s(aes_sbox()), u64s([1] * 8), None) == -1
    # an output of 2^31 terms or more
    assert lib.csgn_uint_lut_create(4, 1, u64s([0] * 15 + [1]), u64s([216] * 4), C.byref(handle)) == -2
    buf = np.zeros(64, dtype=np.uint64)
    ptrs = (C.c_void_p * 64)(*([buf.ctypes.data] * 64))
    assert lib.csgn_uint_lut_apply(None, 1247, 4, ptrs, ptrs, None) == -1
    assert lib.csgn_uint_lut_apply(None, 0, 4, ptrs, ptrs, None) == -1
    lib.csgn_uint_lut_destroy(None)


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
TABLES = {
    "identity": (4, 4, list(range(16))),
    "zero": (3, 2, [0] * 8),
    "ones": (3, 3, [7] * 8),
    "times3": (4, 4, [(3 * x) % 16 for x in range(16)]),
    "popcount": (4, 3, [bin(x).count("1") for x in range(16)]),
    "random": (5, 6, random_table(5, 6, 55)),
    "wide_out": (3, 64, random_table(3, 64, 56)),
}


@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_definition_matches_reference(oracle, ref, n, d, name, tmode):
    w, m, table = TABLES[name]
    ts = [1] * w if tmode == "1" else [1 + (i * 5 + len(name)) % 3 for i in range(w)]
    planes = [rand_terms(n, 1, t, 40 + i)[0].ravel() for i, t in enumerate(ts)]
    add, mul = ref_ops(ref, n, d)
    want = compose_lut(planes, table, w, m, add, mul, const_term(n, 1), const_term(n, 0))
    add, mul = oracle_ops(oracle, n)
    got = compose_lut(planes, table, w, m, add, mul, const_term(n, 1), const_term(n, 0))
    words = np_lut(n, [p.reshape(1, t, -1) for p, t in zip(planes, ts)], table, m)
    dl = (n + 63) // 64
    sizes = lut_terms(table, w, m, ts)
    for j in range(m):
        assert np.array_equal(got[j], want[j]), j
        assert got[j].size == sizes[j] * dl
        assert np.array_equal(words[j].ravel(), got[j]), j
    if name == "identity":
        for j in range(m):
            assert np.array_equal(words[j].ravel(), planes[j])
    if name in ("zero", "ones"):
        bit = 1 if name == "ones" else 0
        for j in range(m):
            assert np.array_equal(words[j].ravel(), const_term(n, bit))


def test_definition_sbox_matches_reference(oracle, ref):
    n, d = 1247, 16
    table = aes_sbox()
    planes = [rand_terms(n, 1, 1, 70 + i)[0].ravel() for i in range(8)]
    add, mul = ref_ops(ref, n, d)
    want = compose_lut(planes, table, 8, 8, add, mul, const_term(n, 1), const_term(n, 0))
    words = np_lut(n, [p.reshape(1, 1, -1) for p in planes], table, 8)
    for j in range(8):
        assert np.array_equal(words[j].ravel(), want[j]), j


@pytest.mark.parametrize("n", [64, 63, 1247])
def test_definition_matches_oracle_batched(oracle, n):
    w, m = 4, 5
    table = random_table(w, m, 99)
    ts, batch = [2, 1, 3, 1], 3
    planes = [rand_terms(n, batch, t, 60 + i) for i, t in enumerate(ts)]
    add, mul = oracle_ops(oracle, n)
    words = np_lut(n, planes, table, m)
    for e in range(batch):
        want = compose_lut([p[e].ravel() for p in planes], table, w, m, add, mul, const_term(n, 1), const_term(n, 0))
        for j in range(m):
            assert np.array_equal(words[j][e].ravel(), want[j]), (e, j)


# -- decryptions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_truth_tables_decrypt(oracle, w):
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(170 + w, 64 * d + 64))
    values = np.arange(1 << w, dtype=np.uint64)
    planes = encrypt_planes(oracle, n, key, values, w, 180 + w)
    for seed in range(4):
        m = 1 + (seed * 3 + w) % 5
        table = random_table(w, m, 1000 * w + seed)
        got = decrypt_value(oracle, n, key, np_lut(n, planes, table, m))
        assert [int(v) for v in got] == table, (w, seed)


def test_compacted_today_route_same_bits(oracle):
    """Today's route, sum over k with bit j of f(k) of equalTo(a, k), decrypts to the same bits, with many more terms."""
    n, d, w = 127, 8, 3
    key, _ = oracle.keygen(n, d, glibc_draws(33, 64 * d + 64))
    values = np.arange(1 << w, dtype=np.uint64)
    planes = encrypt_planes(oracle, n, key, values, w, 34)
    table = [(5 * x + 3) % 8 for x in range(8)]
    outs = np_lut(n, planes, table, 3)
    for j in range(3):
        ks = [k for k in range(8) if (table[k] >> j) & 1]
        today = np_plain(n, EQ, planes, ks[0])
        for k in ks[1:]:
            today = np_add(today, np_plain(n, EQ, planes, k))
        assert np.array_equal(decrypt_bits(oracle, n, key, today), decrypt_bits(oracle, n, key, outs[j]))
        assert today.shape[1] >= outs[j].shape[1]
