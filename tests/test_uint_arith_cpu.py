"""a + b, a - b, a == b and a != b of encrypted integers in one launch (csgn_uint_arith*) on a box without a GPU: the
definition by position (tests/model_arith.py) against the per-bit chains of tests/model.py term for term, the term
counts, the argument checks and their order, the dispatch names and knob, and decryptions of sums, differences, both
carries and the equality through the oracle.  The device side is tests/test_uint_arith_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (ADD_FULL, ADD_HALF, LIMIT, const_term, decrypt_bits, decrypt_value, encrypt_planes, lib,  # noqa: F401
                         np_not, np_step, np_uint_add, np_uint_eq, np_uint_sub, rand_terms, u64s)
from tests.model_arith import (ADD, EQ, NE, OPS, SUB, arith_counts, arith_entry, arith_terms, c_terms, np_arith,
                               np_arith_chain, term_modes)


def planes_of(n, batch, ta, tb, seed):
    a = [rand_terms(n, batch, t, seed + k) for k, t in enumerate(ta)]
    b = [rand_terms(n, batch, t, seed + 40 + k) for k, t in enumerate(tb)]
    return a, b


# -- the definition by position against the chains --------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["1", "2", "mixed"])
@pytest.mark.parametrize("w", range(1, 7))
def test_decode_gives_the_chains(w, mode):
    n, batch = 65, 2
    ta, tb = term_modes(w, mode)
    a, b = planes_of(n, batch, ta, tb, 100 * w)
    decoded = {(op, carry): np_arith(n, op, a, b, carry) for op, carry in ((ADD, True), (SUB, True), (EQ, False), (NE, False))}
    outs, carry = decoded[ADD, True]
    want = np_uint_add(n, a, b)
    assert len(outs) == w and all(np.array_equal(o, x) for o, x in zip(outs, want))
    _, c = np_step(n, ADD_HALF, None, a[0], b[0])
    for j in range(1, w):
        _, c = np_step(n, ADD_FULL, c, a[j], b[j])
    assert np.array_equal(carry, c)
    outs, carry = decoded[SUB, True]
    want = np_uint_sub(n, a, b)
    assert len(outs) == w and all(np.array_equal(o, x) for o, x in zip(outs, want))
    c = np.broadcast_to(const_term(n, 1), (batch, 1, a[0].shape[2]))
    for j in range(w):
        _, c = np_step(n, ADD_FULL, c, a[j], np_not(n, b[j]))
    assert np.array_equal(carry, c)
    assert outs[0].shape[1] == ta[0] + tb[0] + 2                      # both ONEs of plane 0 are written
    eq = np_uint_eq(n, a, b)
    assert np.array_equal(decoded[EQ, False][0][0], eq) and decoded[EQ, False][1] is None
    assert np.array_equal(decoded[NE, False][0][0], np_not(n, eq))
    for op in (ADD, SUB):                                             # without the carry: the same planes, no carry
        planes, none = np_arith(n, op, a, b)
        assert none is None and len(planes) == w
        assert all(np.array_equal(x, y) for x, y in zip(planes, decoded[op, True][0]))
    for (op, carry), (ref, rc) in decoded.items():                    # the chain model the device tests compare with
        got, gc = np_arith_chain(n, op, a, b, carry)
        assert len(got) == len(ref) and all(np.array_equal(x, y) for x, y in zip(got, ref))
        assert (gc is None and rc is None) or np.array_equal(gc, rc)
        if carry:
            assert np_arith_chain(n, op, a, b, False)[1] is None


def test_entries_by_hand():
    """Fresh planes: plane j of a sum has 2^j + 1 terms, its carry 2^(j+1) - 1, EQ 3^w; a few entries spelt out."""
    one = [1] * 4
    T, Cs = arith_counts(ADD, one, one)
    assert T == [2, 3, 5, 9, 15] and Cs == [1, 3, 7, 15]
    T, Cs = arith_counts(SUB, one, one)
    assert T == [4, 8, 20, 56, 161] and Cs == [5, 17, 53, 161]
    assert arith_counts(EQ, one, one)[0] == [81] and arith_counts(NE, one, one)[0] == [82]
    assert [arith_entry(ADD, one, one, 1, i) for i in range(3)] == [[("a", 1, 0)], [("b", 1, 0)], [("a", 0, 0), ("b", 0, 0)]]
    # c_1 = a_1 b_1 | a_1 c_0 | b_1 c_0
    assert [arith_entry(ADD, one, one, 2, i) for i in range(2, 5)] == [
        [("a", 1, 0), ("b", 1, 0)], [("a", 1, 0), ("a", 0, 0), ("b", 0, 0)], [("b", 1, 0), ("a", 0, 0), ("b", 0, 0)]]
    # SUB: plane 0 = a_0 | b_0 | ONE | ONE; c_0 = a_0 b_0 | a_0 ONE | a_0 c_-1 | b_0 c_-1 | ONE c_-1
    assert [arith_entry(SUB, one, one, 0, i) for i in range(4)] == [[("a", 0, 0)], [("b", 0, 0)], [], []]
    assert [arith_entry(SUB, one, one, 1, i) for i in range(3, 8)] == [
        [("a", 0, 0), ("b", 0, 0)], [("a", 0, 0)], [("a", 0, 0)], [("b", 0, 0)], []]
    # EQ of two planes: digit of plane 1 fastest; 0 = a, 1 = b, 2 = ONE
    assert [arith_entry(EQ, one[:2], one[:2], 0, i) for i in (0, 1, 2, 5, 8)] == [
        [("a", 0, 0), ("a", 1, 0)], [("a", 0, 0), ("b", 1, 0)], [("a", 0, 0)], [("b", 0, 0)], []]
    assert arith_entry(NE, one[:2], one[:2], 0, 9) == []
    assert arith_entry(ADD, [2, 1], [3, 2], 2, 7) == [("a", 1, 0), ("a", 0, 1), ("b", 0, 2)]


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_sweep(lib):
    rng = np.random.default_rng(23)
    for w in range(1, 17):
        one = [1] * w
        for j in range(w):
            assert c_terms(lib, ADD, w, one, one, j) == 2 ** j + 1
        assert c_terms(lib, ADD, w, one, one, w) == 2 ** w - 1
        assert c_terms(lib, EQ, w, one, one, 0) == 3 ** w and c_terms(lib, NE, w, one, one, 0) == 3 ** w + 1
        for _ in range(4):
            ta = [int(x) for x in rng.integers(1, 5, w)]
            tb = [int(x) for x in rng.integers(1, 5, w)]
            for op in OPS.values():
                for o in range(w + 2):
                    assert c_terms(lib, op, w, ta, tb, o) == arith_terms(op, ta, tb, o), (op, ta, tb, o)
    # invalid: the op, the width, null pointers, a plane of no terms, an output the op does not have
    one = [1] * 17
    for op in OPS.values():
        assert c_terms(lib, op, 0, one, one, 0) == 0 and c_terms(lib, op, 17, one, one, 0) == 0
        assert c_terms(lib, op, 4, None, one, 0) == 0 and c_terms(lib, op, 4, one, None, 0) == 0
        assert c_terms(lib, op, 3, [1, 0, 1], one, 0) == 0 and c_terms(lib, op, 3, one, [1, 1, 0], 2) == 0
        assert c_terms(lib, op, 3, [1, 1, 0], one, 0) == 0            # even where the output does not read the plane
        assert c_terms(lib, op, 2, [LIMIT, 1], one, 0) == 0 and c_terms(lib, op, 2, one, [1, LIMIT], 0) == 0
    assert c_terms(lib, 0, 4, one, one, 0) == 0 and c_terms(lib, 5, 4, one, one, 0) == 0
    assert c_terms(lib, ADD, 4, one, one, 5) == 0 and c_terms(lib, EQ, 4, one, one, 1) == 0
    # counts near 2^62
    big = LIMIT - 1
    assert c_terms(lib, ADD, 1, [big - 1], [1], 0) == big and c_terms(lib, ADD, 1, [big], [1], 0) == 0
    assert c_terms(lib, ADD, 1, [big], [1], 1) == big                 # the carry of one plane: ta * tb
    assert c_terms(lib, ADD, 1, [1 << 31], [1 << 31], 1) == 0 and c_terms(lib, ADD, 1, [1 << 31], [(1 << 31) - 1], 1) != 0
    assert c_terms(lib, SUB, 1, [big - 3], [1], 0) == big and c_terms(lib, SUB, 1, [big - 2], [1], 0) == 0
    assert c_terms(lib, EQ, 1, [big - 2], [1], 0) == big and c_terms(lib, EQ, 1, [big - 1], [1], 0) == 0
    assert c_terms(lib, NE, 1, [big - 3], [1], 0) == big and c_terms(lib, NE, 1, [big - 2], [1], 0) == 0
    for ta, tb in (([1 << 30, 1 << 30], [1, 1]), ([1, 1 << 61], [1, 1]), ([(1 << 61) - 1, 1], [1, 3]), ([1 << 20] * 4, [1 << 11] * 4)):
        for op in OPS.values():
            for o in range(len(ta) + 1):
                assert c_terms(lib, op, len(ta), ta, tb, o) == arith_terms(op, ta, tb, o), (op, ta, tb, o)
    assert arith_terms(ADD, [1, 1 << 61], [1, 1], 1) == (1 << 61) + 2 and arith_terms(ADD, [1, 1 << 61], [1, 1], 2) == 0


def test_dispatch_names(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert "uint_arith_form" in names and names.index("uint_arith_form") == len(names) - 2
    knobs.unset("uint_arith_form")
    assert capi.get_tuning("uint_arith_form") == -1

    def name(n, op, w, ta, tb, carry=0):
        return lib.csgn_uint_arith_kernel(n, op, 256, w, u64s(ta), u64s(tb), carry).decode()

    one = [1] * 17
    for form, want in ((1, "k_uint_arith"), (0, "composed")):
        knobs.set("uint_arith_form", form)
        for op in OPS.values():
            for w in (1, 4, 8, 12, 16):
                assert name(1247, op, w, one, one) == want
            assert name(1247, op, 3, [2, 1, 3], [1, 2, 1]) == want
            assert name(0, op, 4, one, one) == ""                     # n_bits 0
            assert name(1247, op, 0, one, one) == "" and name(1247, op, 17, one, one) == ""
            assert name(1247, op, 4, [1, 0, 1, 1], one) == "" and name(1247, op, 4, one, [1, 1, 1, 0]) == ""
            assert lib.csgn_uint_arith_kernel(1247, op, 1, 4, None, u64s(one), 0) == b""
            assert lib.csgn_uint_arith_kernel(1247, op, 1, 4, u64s(one), None, 0) == b""
        assert name(1247, ADD, 8, one, one, 1) == want and name(1247, SUB, 8, one, one, 1) == want
        assert name(1247, EQ, 8, one, one, 1) == "" and name(1247, NE, 8, one, one, 1) == ""   # no carry to ask for
        assert name(1247, 0, 4, one, one) == "" and name(1247, 5, 4, one, one) == ""
        # a carry past 2^62 is a bad shape only where it is asked for
        assert name(1247, ADD, 1, [1 << 31], [1 << 31], 0) == want and name(1247, ADD, 1, [1 << 31], [1 << 31], 1) == ""
    knobs.unset("uint_arith_form")
    for op in OPS.values():
        for w in (4, 8, 12):                                          # the measured shapes
            assert name(1247, op, w, one, one, int(op == SUB)) in ("k_uint_arith", "composed")


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits, the op, the width, host pointers, term counts
    (INVALID), 2^31 words per element and 2^60 per batch (UNSUPPORTED), null device pointers (INVALID), and only then
    the device (NO_DEVICE on a box without one; with one, the calls that pass every check are not made: their pointers
    are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 17)(*([p] * 17))
    nullp = (C.c_void_p * 17)(*([p] * 3 + [None] + [p] * 13))
    null0 = (C.c_void_p * 17)(*([None] + [p] * 16))
    one = u64s([1] * 17)
    zero_first = u64s([0] + [1] * 16)
    huge = u64s([1 << 61] * 17)

    def arith(n=1247, op=ADD, batch=4, w=8, a=ptrs, ta=one, b=ptrs, tb=one, out=ptrs, carry=None):
        return lib.csgn_uint_arith(n, op, batch, w, a, ta, b, tb, out, carry, None)

    # each failing check wins over every later one
    assert arith(n=0, op=0, w=0, a=None) == -1                        # n_bits
    assert arith(n=131073, op=0) == -2
    assert arith(op=0, w=0) == -1 and arith(op=5, a=None) == -1       # the op
    assert b"operation" in lib.csgn_last_error()
    assert arith(w=0, a=None) == -1 and arith(w=17, ta=zero_first) == -1          # the width
    assert b"width" in lib.csgn_last_error()
    for arg in ("a", "ta", "b", "tb", "out"):                         # host pointers, before the term counts
        assert arith(**{arg: None, "tb": None if arg == "tb" else zero_first}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    for op in (EQ, NE):                                               # a comparison has no carry
        assert arith(op=op, carry=p, ta=zero_first) == -1 and b"carry" in lib.csgn_last_error()
    for op in OPS.values():                                           # term counts
        assert arith(op=op, ta=zero_first) == -1 and arith(op=op, tb=zero_first, batch=1 << 50) == -1
        assert arith(op=op, ta=huge, batch=1 << 50) == -1             # 2^62 or more is INVALID, not UNSUPPORTED
    assert arith(w=1, ta=u64s([1 << 31]), tb=u64s([1 << 31]), carry=p) == -1      # the carry's count, where asked for
    assert arith(w=1, ta=u64s([1 << 31]), tb=u64s([1 << 31])) == -2
    # sizes: 3^16 terms of 20 words = 8.6e8 < 2^31; planes of two terms pass it
    assert arith(op=EQ, w=16, a=nullp) == -1 and b"null device pointer" in lib.csgn_last_error()
    assert arith(op=EQ, w=16, ta=u64s([2] * 16), a=nullp) == -2
    assert arith(op=NE, w=16, tb=u64s([2] * 16)) == -2
    assert arith(op=ADD, w=16, ta=u64s([2] * 16), tb=u64s([2] * 16)) == -2
    # the carry is sized only where it is asked for: 2^w - 1 terms fit, but with 2^12 terms a plane it does not
    t12 = u64s([1 << 12] * 17)
    assert arith(op=ADD, w=2, ta=t12, tb=t12, carry=p, a=nullp) == -2
    assert b"carry" in lib.csgn_last_error()
    assert arith(op=ADD, w=1, ta=u64s([1 << 14]), tb=u64s([1 << 14]), carry=p) == -2
    assert arith(batch=1 << 52, a=nullp) == -2                        # per batch
    assert arith(w=1, batch=1 << 59, n=64) == -2
    assert b"batch" in lib.csgn_last_error()
    for arg in ("a", "b", "out"):                                     # a null device pointer inside each host array
        assert arith(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert arith(op=EQ, out=null0) == -1 and arith(batch=0, b=nullp) == -1
    if gpu:
        return
    # no device: every call that passes the checks above, the empty batch included
    assert arith() == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    for op in OPS.values():
        assert arith(op=op) == -3 and arith(op=op, w=16) == -3 and arith(op=op, batch=0) == -3
    assert arith(carry=p) == -3 and arith(op=SUB, carry=p, w=16) == -3
    assert arith(op=EQ, out=nullp) == -3 and arith(w=3, a=nullp, b=nullp, out=nullp) == -3   # only the entries it reads
    assert arith(op=ADD, w=1, ta=u64s([1 << 14]), tb=u64s([1 << 14])) == -3      # the carry is not sized unasked


def test_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        return                                                        # the device tests make the calls
    buf = np.zeros(64, dtype=np.uint64)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    one = u64s([1, 1])
    assert lib.csgn_uint_arith(1247, ADD, 1, 2, ptrs, one, ptrs, one, ptrs, None, None) == -3
    assert b"no CPU fallback" in lib.csgn_last_error()


# -- decryptions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 3, 8])
def test_decrypts(oracle, w):
    """a + b and a - b mod 2^w, carry = (a + b >= 2^w), sub's carry = (a >= b), and a == b with planted ties: every
    pair for w <= 3, 24 drawn pairs and 8 ties for w = 8."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(610 + w, 64 * d + 64))
    rng = np.random.default_rng(60 + w)
    if w <= 3:
        av, bv = (g.ravel().astype(np.uint64) for g in np.meshgrid(np.arange(1 << w), np.arange(1 << w)))
    else:
        ties = rng.integers(0, 1 << w, 8)
        av = np.concatenate([rng.integers(0, 1 << w, 24), ties, [0, 255, 255]]).astype(np.uint64)
        bv = np.concatenate([rng.integers(0, 1 << w, 24), ties, [255, 0, 1]]).astype(np.uint64)
    assert (av == bv).any() and (av < bv).any() and (av > bv).any()
    a = encrypt_planes(oracle, n, key, av, w, 620 + w)
    b = encrypt_planes(oracle, n, key, bv, w, 630 + w)
    mask = np.uint64((1 << w) - 1)
    outs, carry = np_arith_chain(n, ADD, a, b, True) if w == 8 else np_arith(n, ADD, a, b, True)
    assert np.array_equal(decrypt_value(oracle, n, key, outs), (av + bv) & mask)
    assert np.array_equal(decrypt_bits(oracle, n, key, carry), (av + bv) >> np.uint64(w) != 0)
    outs, carry = np_arith_chain(n, SUB, a, b, True) if w == 8 else np_arith(n, SUB, a, b, True)
    assert np.array_equal(decrypt_value(oracle, n, key, outs), (av - bv) & mask)
    assert np.array_equal(decrypt_bits(oracle, n, key, carry), av >= bv)
    if w == 8:                                                        # 3^8 terms an element: the first twelve elements
        a, b, av, bv = [p[20:32] for p in a], [p[20:32] for p in b], av[20:32], bv[20:32]
        assert (av == bv).any() and (av != bv).any()
    eq = np_arith(n, EQ, a, b)[0][0]
    assert np.array_equal(decrypt_bits(oracle, n, key, eq), av == bv)
    assert np.array_equal(decrypt_bits(oracle, n, key, np_arith(n, NE, a, b)[0][0]), av != bv)
