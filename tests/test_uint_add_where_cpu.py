"""a + (s ? k : 0), a public constant added where an encrypted flag is set (csgn_uint_add_where*), on a box without a
GPU: the definition's table over the oracle's and, where built, the reference's own add and multiply against its numpy
form; the decode by position against the table term for term; the term counts; the argument checks and their order;
the clear-bit recurrence; decryptions through the oracle; the knob.  The device side is
tests/test_uint_add_where_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.binding import glibc_draws, load_ref
from tests.model import (LIMIT, const_term, decrypt_bits, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms,  # noqa: F401
                         ref_ops, u64s)
from tests.model_add_where import (add_where_counts, add_where_entry, add_where_terms, c_terms, clear_add_where,
                                   compose_add_where, np_add_where, np_add_where_compose)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def term_modes(w, mode):
    """(ta, ts): fresh, or mixed 1..3."""
    if mode == "fresh":
        return [1] * w, 1
    return [1 + (j + 1) % 3 for j in range(w)], 2 + w % 2         # a: 2, 3, 1, ...; s: 2 or 3


def planes_of(n, batch, ta, ts, seed):
    return [rand_terms(n, batch, t, seed + k) for k, t in enumerate(ta)], rand_terms(n, batch, ts, seed + 90)


# -- the definition against the genuine reference and the oracle -------------------------------------------------------
@pytest.mark.parametrize("n,d", [(65, 4), (1247, 16)])
@pytest.mark.parametrize("mode", ["fresh", "mixed"])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5])
def test_definition_matches_reference_and_oracle(oracle, n, d, w, mode):
    """The table through the oracle's operators and, where the reference is built, through its own, for every k:
    the words of the numpy composition, of the sizes of the closed form."""
    ref = load_ref()
    ta, ts = term_modes(w, mode)
    dl = (n + 63) // 64
    a, s = planes_of(n, 1, ta, ts, 40 * w)
    flat, sflat = [p[0].ravel() for p in a], s[0].ravel()
    zero = const_term(n, 0)
    for k in range(1 << w):
        want, want_c = np_add_where_compose(n, a, s, k)
        counts, _ = add_where_counts(ta, ts, k)
        routes = [oracle_ops(oracle, n)] + ([ref_ops(ref, n, d)] if ref is not None else [])
        for ops in routes:
            got, got_c = compose_add_where(flat, sflat, k, *ops, zero)
            for j in range(w):
                assert np.array_equal(got[j], want[j].ravel()), (k, j)
                assert got[j].size == counts[j] * dl
            assert np.array_equal(got_c, want_c.ravel()) and got_c.size == counts[w] * dl, k


# -- the decode by position against the table --------------------------------------------------------------------------
def symbolic(ta, ts, k):
    """The table over lists of factor lists."""
    add = lambda x, y: x + y                                          # noqa: E731
    mul = lambda x, y: [p + q for p in x for q in y]                  # noqa: E731
    planes = [[[("a", j, x)] for x in range(t)] for j, t in enumerate(ta)]
    s = [[("s", 0, x)] for x in range(ts)]
    outs, c = compose_add_where(planes, s, k, add, mul, None)
    return outs + [c]


@pytest.mark.parametrize("mode", ["fresh", "mixed"])
@pytest.mark.parametrize("w", range(1, 6))
def test_decode_gives_the_table(w, mode):
    ta, ts = term_modes(w, mode)
    for k in range(1 << w):
        want = symbolic(ta, ts, k)
        T, _ = add_where_counts(ta, ts, k)
        for o in range(w + 1):
            if want[o] is None:                                       # the ZERO carry of k = 0
                assert T[o] == 1 and add_where_entry(ta, ts, k, o, 0) is None
                continue
            assert T[o] == len(want[o]), (k, o)
            for i in range(T[o]):
                assert sorted(add_where_entry(ta, ts, k, o, i)) == sorted(want[o][i]), (k, o, i)


@pytest.mark.parametrize("mode", ["fresh", "mixed"])
def test_decoded_words_are_the_composed_words(mode):
    n, w = 65, 4
    ta, ts = term_modes(w, mode)
    a, s = planes_of(n, 2, ta, ts, 7)
    for k in range(1 << w):
        outs, carry = np_add_where(n, a, s, k, True)
        want, want_c = np_add_where_compose(n, a, s, k)
        assert all(np.array_equal(x, y) for x, y in zip(outs, want)) and np.array_equal(carry, want_c), k
        planes, none = np_add_where(n, a, s, k)
        assert none is None and all(np.array_equal(x, y) for x, y in zip(planes, want))


def test_entries_by_hand():
    one = [1] * 4
    # a + (s ? 1 : 0): plane j = a_j | a_{j-1} ... a_0 s
    assert add_where_entry(one, 1, 1, 0, 1) == [("s", 0, 0)]
    assert add_where_entry(one, 1, 1, 3, 1) == [("a", 2, 0), ("a", 1, 0), ("a", 0, 0), ("s", 0, 0)]
    assert add_where_entry(one, 1, 1, 4, 0) == [("a", 3, 0), ("a", 2, 0), ("a", 1, 0), ("a", 0, 0), ("s", 0, 0)]
    # k = 0b0110: plane 0 a copy; c_1 = a_1 s; c_2 = a_2 s | a_2 c_1 | s c_1: an entry with two terms of s
    assert add_where_counts(one, 1, 6) == ([1, 2, 3, 4, 3], [0, 1, 3, 3])
    assert [add_where_entry(one, 1, 6, 3, i) for i in range(4)] == [
        [("a", 3, 0)], [("a", 2, 0), ("s", 0, 0)], [("a", 2, 0), ("a", 1, 0), ("s", 0, 0)],
        [("s", 0, 0), ("a", 1, 0), ("s", 0, 0)]]
    assert add_where_entry([2, 1], 3, 3, 2, 8) == [("a", 1, 0), ("a", 0, 1), ("s", 0, 2)]


# -- the C ABI, host side ----------------------------------------------------------------------------------------------
def test_terms(lib):
    rng = np.random.default_rng(31)
    for w in range(1, 9):
        for k in range(1 << w):
            for ta, ts in ([1] * w, 1), ([1] * w, 2), ([int(x) for x in rng.integers(1, 4, w)], int(rng.integers(1, 4))):
                assert c_terms(lib, w, k, ts, ta) == add_where_terms(ta, ts, k), (w, k, ta, ts)
    # the sizes of the issue's table, fresh a and s
    assert c_terms(lib, 8, 1, 1, [1] * 8) == [2] * 8 + [1]
    assert c_terms(lib, 8, 0x64, 1, [1] * 8) == [1, 1, 2, 2, 2, 3, 5, 8, 7]
    assert c_terms(lib, 8, 0xFF, 1, [1] * 8) == [2, 3, 5, 9, 17, 33, 65, 129, 255]
    assert sum(c_terms(lib, 16, 1, 1, [1] * 16)) == 33 and sum(c_terms(lib, 32, 1, 1, [1] * 32)) == 65
    assert c_terms(lib, 8, 0, 1, [1] * 8) == [1] * 9                  # k = 0: copies and the ZERO carry
    for w in (17, 31, 32):
        for k in (1, 1 << (w - 1), (1 << (w - 1)) | 1, 0xFF << (w - 8), (1 << w) - 1):
            for ts in (1, 2):
                assert c_terms(lib, w, k, ts, [1] * w) == add_where_terms([1] * w, ts, k), (w, k, ts)
    # invalid: the width, k, null pointers, zero counts, 2^62
    one = [1] * 33
    assert c_terms(lib, 0, 0, 1, one) is None and c_terms(lib, 33, 1, 1, one) is None
    assert c_terms(lib, 4, 16, 1, one) is None and c_terms(lib, 32, 1 << 32, 1, one) is None
    assert c_terms(lib, 4, 1, 1, None) is None
    assert lib.csgn_uint_add_where_terms(4, 1, 1, u64s(one), None) == 0
    assert c_terms(lib, 4, 1, 0, one) is None and c_terms(lib, 4, 0, 0, one) is None
    assert c_terms(lib, 3, 1, 1, [1, 0, 1]) is None and c_terms(lib, 3, 4, 1, [0, 1, 1]) is None
    assert c_terms(lib, 2, 1, LIMIT, one) is None and c_terms(lib, 2, 1, 1, [1, LIMIT]) is None
    big = LIMIT - 1
    assert c_terms(lib, 1, 1, 1, [big - 1]) == [big, big - 1] and c_terms(lib, 1, 1, 1, [big]) is None
    assert c_terms(lib, 1, 0, 1, [big]) == [big, 1]
    assert c_terms(lib, 1, 1, 1 << 31, [1 << 31]) is None and c_terms(lib, 1, 1, (1 << 31) - 1, [1 << 31]) is not None
    # the table is not written where the call fails
    out = (C.c_uint64 * 5)(*[7] * 5)
    assert lib.csgn_uint_add_where_terms(4, 1, 0, u64s([1] * 4), out) == 0 and list(out) == [7] * 5


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits, the width and k, host pointers, term counts (INVALID),
    2^31 words per element and 2^60 per batch (UNSUPPORTED), null device pointers (INVALID), and only then the device
    (NO_DEVICE on a box without one; with one, the calls that pass every check are not made: their pointers are not
    device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 33)(*([p] * 33))
    nullp = (C.c_void_p * 33)(*([p] * 3 + [None] + [p] * 29))
    one = u64s([1] * 33)
    zero_first = u64s([0] + [1] * 32)
    huge = u64s([1 << 61] * 33)

    def call(n=1247, batch=4, w=8, k=0xA5, sel=p, ts=1, a=ptrs, ta=one, out=ptrs, carry=None):
        return lib.csgn_uint_add_where(n, batch, w, k, sel, ts, a, ta, out, carry, None)

    assert call(n=0, w=0, a=None) == -1                               # n_bits
    assert call(n=131073, w=0) == -2
    assert call(w=0, a=None) == -1 and call(w=33, ta=zero_first) == -1            # the width
    assert b"width" in lib.csgn_last_error()
    assert call(k=256, a=None) == -1 and call(w=32, k=1 << 32, ta=None) == -1     # k
    assert b"does not fit" in lib.csgn_last_error()
    for arg in ("a", "ta", "out"):                                    # host pointers, before the term counts
        assert call(**{arg: None, "ts": 0}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    assert call(ta=zero_first, batch=1 << 50) == -1 and call(ts=0, batch=1 << 50) == -1   # term counts
    assert call(ta=huge, batch=1 << 50) == -1 and call(ts=1 << 62, sel=None) == -1
    assert call(k=0, ts=0) == -1                                      # also where k reads no flag
    assert call(w=1, k=1, ts=1 << 31, ta=u64s([1 << 31]), carry=p) == -1          # the carry's count, where asked for
    assert call(w=1, k=1, ts=1 << 31, ta=u64s([1 << 31])) == -2
    # sizes: fresh (8, 0xFF) fits; with 2^12 terms a plane it does not; the carry only where asked for
    t12 = u64s([1 << 12] * 33)
    assert call(w=3, k=7, ta=t12, ts=1 << 12, a=nullp) == -2
    assert call(w=1, k=1, ta=u64s([1 << 14]), ts=1 << 14, carry=p, a=nullp) == -2
    assert b"carry" in lib.csgn_last_error()
    assert call(w=32, k=(1 << 32) - 1, sel=None) == -2                # 2^32 - 1 entries a plane
    assert call(batch=1 << 56, a=nullp) == -2                         # per batch
    assert b"batch" in lib.csgn_last_error()
    for arg in ("a", "out"):                                          # a null device pointer inside each host array
        assert call(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert call(sel=None) == -1 and b"null device pointer" in lib.csgn_last_error()
    assert call(batch=0, a=nullp) == -1
    if gpu:
        return
    # no device: every call that passes the checks above, the empty batch included
    assert call() == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert call(batch=0) == -3 and call(carry=p) == -3 and call(w=32, k=1) == -3 and call(w=32, k=0x80000001, carry=p) == -3
    assert call(k=0, sel=None) == -3                                  # k = 0 reads no flag
    assert call(w=3, k=5, a=nullp, out=nullp) == -3                   # only the entries it reads
    assert call(w=1, k=1, ta=u64s([1 << 14]), ts=1 << 14) == -3       # the carry is not sized unasked


# -- clear bits ---------------------------------------------------------------------------------------------------------
def test_clear_bit_recurrence():
    """Every w <= 8, k, x and s: out_j = a_j ^ (k_j & s) ^ c with c' = maj(a_j, s, c) where k_j = 1 and a_j & c where
    k_j = 0 gives (x + (s ? k : 0)) mod 2^w and the bit that left."""
    for w in range(1, 9):
        x = np.arange(1 << w, dtype=np.int64)
        for k in range(1 << w):
            for s in (0, 1):
                c, v = np.zeros_like(x), np.zeros_like(x)
                for j in range(w):
                    aj, kj = (x >> j) & 1, (k >> j) & 1
                    v |= (aj ^ (kj & s) ^ c) << j
                    c = (aj & s) | (aj & c) | (s & c) if kj else aj & c
                want = x + (k if s else 0)
                assert np.array_equal(v, want & ((1 << w) - 1)) and np.array_equal(c, want >> w), (w, k, s)


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_decrypts(oracle, w):
    """Through the oracle's encrypt and decrypt at N = 127: planes and carry decrypt to (x + (s ? k : 0)) mod 2^w and
    the bit that left -- every k for w <= 4, six of them above; every x, both flags."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(910 + w, 64 * d + 64))
    xs = np.tile(np.arange(1 << w, dtype=np.uint64), 2)
    ss = np.repeat(np.array([0, 1], dtype=np.uint64), 1 << w)
    a = encrypt_planes(oracle, n, key, xs, w, 920 + w)
    s = encrypt_planes(oracle, n, key, ss, 1, 930 + w)[0]
    ks = range(1 << w) if w <= 4 else [0, 1, (1 << w) - 1, 1 << (w - 1), 0x14 % (1 << w), 0x2B % (1 << w)]
    for k in ks:
        outs, carry = np_add_where_compose(n, a, s, k)
        want = [clear_add_where(int(x), int(f), k, w) for x, f in zip(xs, ss)]
        assert np.array_equal(decrypt_value(oracle, n, key, outs), np.array([v for v, _ in want], dtype=np.uint64)), k
        assert np.array_equal(decrypt_bits(oracle, n, key, carry), np.array([c for _, c in want]) != 0), k


# -- the knob -----------------------------------------------------------------------------------------------------------
def test_knob_spelling(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert "uint_add_where_form" in names and names.index("uint_add_where_form") < names.index("launch_blocks")
    assert names[-1] == "launch_blocks"
    knobs.unset("uint_add_where_form")
    assert capi.get_tuning("uint_add_where_form") == -1
    for v in (0, 1, -1):
        knobs.set("uint_add_where_form", v)
        assert capi.get_tuning("uint_add_where_form") == v
    with open(os.path.join(ROOT, "csgn_amd", "csrc", "csgn_tuning.cpp")) as f:
        assert '{"uint_add_where_form", -1}' in f.read()
    with open(os.path.join(ROOT, "csgn_amd", "csrc", "csgn_tuning.h")) as f:
        header = f.read()
    assert header.index("TUNE_UINT_ADD_WHERE_FORM,") < header.index("TUNE_LAUNCH_BLOCKS,")
    # the environment spelling a child process forces the route with (tests/test_uint_add_where_cpp.py)
    knobs.unset("CSGN_UINT_ADD_WHERE_FORM")
