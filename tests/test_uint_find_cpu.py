"""Encrypted tables looked up by encrypted key (csgn_uint_find*) on a box without a GPU: the term count P, the argument
checks and their order, the dispatch names and knob, the loud failure without a device, the term order the kernel
decodes (the mixed-radix digits and, for fresh planes, the pair of subsets, restated in tests/model_find.py), and the
DEFINITION -- the left-nested sum over rows r of equalTo(key row r, query) times value row r, a composition of the
reference's operator+ / operator* with ONE -- pinned against the compiled reference and the oracle, with decryptions
under random keys.  The device side is tests/test_uint_find_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, const_term, decrypt_bits, decrypt_value, encrypt_planes, lib, np_add, oracle_ops,
                         rand_terms, ref_ops, u64s)
from tests.model_find import (c_P, compose_find, digits, find_terms, fresh_subsets, np_find, np_find_decoded,
                              np_find_fast)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_formula(lib):
    rng = np.random.default_rng(7)
    for v in range(1, 17):
        assert c_P(lib, v, [1] * v, [1] * v) == 3 ** v, v
        for _ in range(4):
            u = [int(x) for x in rng.integers(1, 5, v)]
            s = [int(x) for x in rng.integers(1, 5, v)]
            assert c_P(lib, v, u, s) == find_terms(u, s) == int(np.prod([a + b + 1 for a, b in zip(u, s)], dtype=object))
    assert c_P(lib, 3, [2, 2, 2], [1, 3, 1]) == 4 * 6 * 4


def test_terms_invalid(lib):
    one = [1] * 17
    assert c_P(lib, 0, one, one) == 0                                 # key width outside 1..16
    assert c_P(lib, 17, one, one) == 0
    assert c_P(lib, 16, one, one) == 3 ** 16
    assert c_P(lib, 4, None, one) == 0                                # null pointers
    assert c_P(lib, 4, one, None) == 0
    assert c_P(lib, 3, [1, 0, 1], one) == 0                           # a plane of no terms
    assert c_P(lib, 3, one, [1, 1, 0]) == 0
    # 2^62 or more
    assert c_P(lib, 4, [1 << 16] * 4, one) == 0
    assert c_P(lib, 4, [(1 << 14) - 2] * 4, one) == (1 << 14) ** 4
    assert c_P(lib, 1, [LIMIT - 2], [1]) == 0
    assert c_P(lib, 1, [LIMIT - 3], [1]) == LIMIT - 1
    assert c_P(lib, 1, [1], [LIMIT]) == 0
    assert c_P(lib, 2, [1 << 61, 1], [1, 1]) == 0


def test_dispatch_names(lib, knobs):
    from csgn_amd import capi
    assert "uint_find_form" in capi.tuning_names()
    knobs.unset("uint_find_form")
    assert capi.get_tuning("uint_find_form") == -1

    def name(n, v, u, s, rows, w, t, member=0):
        return lib.csgn_uint_find_kernel(n, 256, v, u64s(u), u64s(s), rows, w, u64s(t), member).decode()

    one = [1] * 16
    bench = [(4, 16, 8), (8, 16, 8), (8, 256, 1), (2, 1024, 8)]       # the measured shapes: fused
    for v, rows, w in bench:
        assert name(1247, v, one, one, rows, w, [1] * w) == "k_uint_find"
    assert name(1247, 1, [2], [1], 1, 1, [3]) == "k_uint_find"
    assert name(1247, 2, one, one, 5, 0, [], 1) == "k_uint_find"      # member alone
    assert name(0, 4, one, one, 16, 8, [1] * 8) == ""                 # n_bits 0
    assert name(1247, 0, one, one, 16, 8, [1] * 8) == ""              # bad key width
    assert name(1247, 17, [1] * 17, [1] * 17, 16, 8, [1] * 8) == ""
    assert name(1247, 4, one, one, 0, 8, [1] * 8) == ""               # no rows
    assert name(1247, 4, one, one, 16, 65, [1] * 65) == ""            # value width past 64
    assert name(1247, 4, one, one, 16, 0, []) == ""                   # nothing to compute
    assert name(1247, 4, [1, 0, 1, 1], one, 16, 2, [1, 1]) == ""      # a plane of no terms
    assert name(1247, 4, one, [1, 1, 1, 0], 16, 2, [1, 1]) == ""
    assert name(1247, 4, one, one, 16, 2, [1, 0]) == ""
    assert lib.csgn_uint_find_kernel(1247, 1, 4, None, u64s(one), 16, 1, u64s(one), 0) == b""
    assert lib.csgn_uint_find_kernel(1247, 1, 4, u64s(one), u64s(one), 16, 1, None, 0) == b""
    knobs.set("uint_find_form", 0)
    assert capi.get_tuning("uint_find_form") == 0
    for v, rows, w in bench:
        assert name(1247, v, one, one, rows, w, [1] * w) == "composed"
    assert name(1247, 4, one, one, 0, 8, [1] * 8) == ""
    knobs.set("uint_find_form", 1)
    for v, rows, w in bench:
        assert name(1247, v, one, one, rows, w, [1] * w) == "k_uint_find"
    assert name(1247, 3, [2, 1, 1], [1, 1, 3], 7, 2, [1, 2], 1) == "k_uint_find"


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits, the widths, rows, host pointers, term counts (INVALID),
    2^31 words per element and 2^60 per batch (UNSUPPORTED), and only then the device (NO_DEVICE on a box without one;
    with one, the calls that pass every check are not made: their pointers are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 64)(*([p] * 64))
    one = u64s([1] * 64)
    zero_first = u64s([0] + [1] * 63)
    huge = u64s([1 << 61] * 64)

    def find(n=1247, batch=4, v=8, x=ptrs, s=one, rows=16, y=ptrs, u=one, w=8, d=ptrs, t=one, out=ptrs, member=None):
        return lib.csgn_uint_find(n, batch, v, x, s, rows, y, u, w, d, t, out, member, None)

    # each failing check wins over every later one
    assert find(n=0, v=0, rows=0, x=None) == -1                       # n_bits
    assert find(n=131073) == -2
    assert find(v=0, rows=0) == -1 and find(v=17, x=None) == -1       # key width
    assert find(w=65, rows=0) == -1                                   # value width
    assert find(w=0, rows=0) == -1                                    # width 0 without member
    assert find(rows=0, x=None) == -1                                 # rows
    assert b"rows" in lib.csgn_last_error()
    for arg in ("x", "s", "y", "u", "d", "t", "out"):                 # host pointers, before the term counts
        assert find(**{arg: None, "u": None if arg == "u" else zero_first}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    assert find(u=zero_first) == -1 and find(s=zero_first) == -1      # term counts
    assert find(t=zero_first) == -1
    assert find(u=huge, rows=1 << 40) == -1                           # P >= 2^62 is INVALID, not UNSUPPORTED
    assert find(w=0, member=p, d=None, t=None, out=None, u=zero_first) == -1
    # sizes: 3^16 * 20 words = 8.6e8 < 2^31; a third row, three value terms or 2-term planes pass it
    assert find(v=16, rows=3, w=1) == -2
    assert find(v=16, rows=1, w=1, t=u64s([3])) == -2
    assert find(v=16, rows=1, w=1, u=u64s([2] * 16)) == -2
    assert find(v=16, rows=1, w=0, member=p, u=u64s([2] * 16)) == -2  # member alone is sized too
    assert find(v=2, rows=1 << 62, w=1) == -2                         # rows * P wraps
    assert find(batch=1 << 44) == -2                                  # per batch
    assert find(v=1, rows=1, w=1, batch=1 << 59, n=64) == -2
    assert b"batch" in lib.csgn_last_error()
    if gpu:
        return
    # no device: every call that passes the checks above, the empty batch and null device pointers included
    assert find() == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert find(v=16, rows=1, w=1) == -3 and find(v=16, rows=1, w=1, t=u64s([2])) == -3
    assert find(w=0, member=p, d=None, t=None, out=None) == -3
    assert find(batch=0) == -3
    nullp = (C.c_void_p * 64)(*([p] * 3 + [None] + [p] * 60))
    assert find(x=nullp) == -3


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
CASES = [  # (v, rows, key terms u, query terms s, value terms t)
    (1, 1, [1], [1], [1]),
    (1, 2, [2], [1], [3]),
    (2, 3, [1, 1], [1, 1], [1, 2]),
    (3, 5, [1, 2, 1], [2, 1, 1], [2, 1]),
    (4, 4, [1] * 4, [1] * 4, [1, 1]),
    (3, 2, [2, 2, 2], [1, 3, 1], [1]),
]


@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("member", [False, True], ids=["plain", "member"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_definition_matches_reference(oracle, ref, n, d, case, member):
    v, rows, u, s, t = CASES[case]
    seed = 2000 * case + n
    keys = [rand_terms(n, rows, uk, seed + k) for k, uk in enumerate(u)]
    query = [rand_terms(n, 1, sk, seed + 20 + k) for k, sk in enumerate(s)]
    values = [rand_terms(n, rows, tj, seed + 50 + j) for j, tj in enumerate(t)]
    key_rows = [[keys[k][r].ravel() for k in range(v)] for r in range(rows)]
    value_rows = [[values[j][r].ravel() for j in range(len(t))] for r in range(rows)]
    flat_query = [x[0].ravel() for x in query]
    one = const_term(n, 1)
    add, mul = ref_ops(ref, n, d)
    want, want_m = compose_find(key_rows, flat_query, value_rows, add, mul, one, member)
    add, mul = oracle_ops(oracle, n)
    got, got_m = compose_find(key_rows, flat_query, value_rows, add, mul, one, member)
    words, words_m = np_find(n, keys, query, values, member)
    dl = (n + 63) // 64
    P = find_terms(u, s)
    for j in range(len(t)):
        assert np.array_equal(got[j], want[j]), j
        assert got[j].size == rows * P * t[j] * dl
        assert np.array_equal(words[j].ravel(), got[j]), j
    if member:
        assert np.array_equal(got_m, want_m) and got_m.size == rows * P * dl
        assert np.array_equal(words_m.ravel(), got_m)
    else:
        assert want_m is None and got_m is None and words_m is None


@pytest.mark.parametrize("case", range(len(CASES)))
def test_decode_gives_the_definition(case):
    """The digits csgn_uint_find.hip decodes reproduce the definition's words term for term, and so does the
    vectorised numpy form the device tests compare with."""
    v, rows, u, s, t = CASES[case]
    n, batch = 129, 2
    keys = [rand_terms(n, rows, uk, 80 + k) for k, uk in enumerate(u)]
    query = [rand_terms(n, batch, sk, 90 + k) for k, sk in enumerate(s)]
    values = [rand_terms(n, rows, tj, 100 + j) for j, tj in enumerate(t)]
    want, want_m = np_find(n, keys, query, values, True)
    for form in (np_find_decoded, np_find_fast):
        got, got_m = form(n, keys, query, values, True)
        for j in range(len(t)):
            assert np.array_equal(got[j], want[j]), (form.__name__, j)
        assert np.array_equal(got_m, want_m), form.__name__
        assert form(n, keys, query, values)[1] is None
    only_m = np_find_fast(n, keys, query, [], True)
    assert only_m[0] == [] and np.array_equal(only_m[1], want_m)


def test_decode_fresh_subsets():
    """Fresh planes: entry q is Pk[Sk] & Pq[Sq] with Sk the digits 0 and Sq the digits 1, disjoint; every ordered pair
    of disjoint subsets appears exactly once, and k = 0 is the slowest digit."""
    v = 4
    seen = [fresh_subsets(q, v) for q in range(3 ** v)]
    assert all(sk & sq == 0 for sk, sq in seen)
    assert len(set(seen)) == 3 ** v
    assert set(seen) == {(a, b) for a in range(1 << v) for b in range(1 << v) if a & b == 0}
    assert seen[0] == (15, 0) and seen[1] == (7, 8) and seen[2] == (7, 0) and seen[-1] == (0, 0)
    assert digits(27 + 2 * 9 + 3 + 0, [1] * 4, [1] * 4) == [1, 2, 1, 0]
    assert digits(2 * 4 + 3, [2, 1], [1, 2]) == [2, 3]                # radices 4 and 4: ONE is digit u + s


# -- decryptions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2, 3, 4])
def test_truth_tables_decrypt(oracle, v):
    """Every query against distinct keys: a full table, partial tables (the absent keys give 0 and member 0)."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(370 + v, 64 * d + 64))
    xs = np.arange(1 << v, dtype=np.uint64)
    query = encrypt_planes(oracle, n, key, xs, v, 380 + v)
    rng = np.random.default_rng(40 + v)
    for rows in sorted({1, (1 << v) - 1, 1 << v, int(rng.integers(1, (1 << v) + 1))}):
        w = 1 + (rows + v) % 4
        ks = rng.permutation(1 << v)[:rows].astype(np.uint64)
        vals = rng.integers(0, 1 << w, rows).astype(np.uint64)
        keys = [x.reshape(rows, 1, -1) for x in encrypt_planes(oracle, n, key, ks, v, 390 + 10 * v + rows)]
        values = [x.reshape(rows, 1, -1) for x in encrypt_planes(oracle, n, key, vals, w, 395 + 10 * v + rows)]
        outs, mem = np_find(n, keys, query, values, True)
        table = {int(k): int(x) for k, x in zip(ks, vals)}
        assert [int(g) for g in decrypt_value(oracle, n, key, outs)] == [table.get(int(x), 0) for x in xs], (v, rows)
        assert [int(b) for b in decrypt_bits(oracle, n, key, mem)] == [int(int(x) in table) for x in xs], (v, rows)


def test_duplicate_keys_xor_and_multi_term_planes(oracle):
    """A duplicated key gives the XOR of its two values and member 0 (the parity of two matches); planes that are sums
    (x + ZERO + ZERO: more terms, the same bit) read the same values."""
    n, d, v, w = 127, 8, 3, 4
    key, _ = oracle.keygen(n, d, glibc_draws(401, 64 * d + 64))
    ks = np.array([5, 2, 5, 7], dtype=np.uint64)
    vals = np.array([9, 3, 12, 6], dtype=np.uint64)
    xs = np.array([5, 2, 0], dtype=np.uint64)                         # twice, once, never
    rows = len(ks)
    keys = [x.reshape(rows, 1, -1) for x in encrypt_planes(oracle, n, key, ks, v, 402)]
    values = [x.reshape(rows, 1, -1) for x in encrypt_planes(oracle, n, key, vals, w, 403)]
    query = encrypt_planes(oracle, n, key, xs, v, 404)
    want = [9 ^ 12, 3, 0]
    for multi in (False, True):
        if multi:
            zq = encrypt_planes(oracle, n, key, np.zeros(len(xs), dtype=np.uint64), 1, 405)[0]
            zr = encrypt_planes(oracle, n, key, np.zeros(rows, dtype=np.uint64), 1, 406)[0].reshape(rows, 1, -1)
            query = [query[0], np_add(query[1], zq), np_add(np_add(query[2], zq), zq)]
            keys = [np_add(keys[0], zr), keys[1], np_add(np_add(keys[2], zr), zr)]
            values[1] = np_add(values[1], zr)
        outs, mem = np_find(n, keys, query, values, True)
        if multi:
            assert mem.shape[1] == rows * find_terms([2, 1, 3], [1, 2, 3]) and outs[1].shape[1] == 2 * mem.shape[1]
        assert [int(g) for g in decrypt_value(oracle, n, key, outs)] == want, multi
        assert [int(b) for b in decrypt_bits(oracle, n, key, mem)] == [0, 1, 0], multi
