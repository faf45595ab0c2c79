"""Selection by an encrypted comparison (csgn_uint_lt_select*) on a box without a GPU: the term count L, the argument
checks and their order, the dispatch names and knob, the loud failure without a device, the term order the kernel decodes
(restated in tests/model_lt_select.py), and the DEFINITION -- logicMux(lessThan(a, b), X_i, Y_i), a composition of the
reference's operator+ / operator* with ONE -- pinned against the compiled reference and the oracle, with decryptions of
min, max and both payloads of a compare-exchange under random keys.  The device side is
tests/test_uint_lt_select_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, const_term, decrypt_bits, decrypt_value, encrypt_planes, lib, np_add, np_uint_lt,
                         np_uint_select, oracle_ops, rand_terms, ref_ops, u64s)
from tests.model_lt_select import (c_L, compose_lt_select, decode, fresh_subsets, lt_counts, lt_terms, minmax_requests,
                                   np_lt_decoded, np_lt_select, np_lt_select_decoded, np_lt_select_fast, out_terms)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_formula(lib):
    rng = np.random.default_rng(11)
    for w in range(1, 17):
        assert c_L(lib, w, [1] * w, [1] * w) == 3 ** w - 1, w
        for _ in range(4):
            ta = [int(x) for x in rng.integers(1, 5, w)]
            tb = [int(x) for x in rng.integers(1, 5, w)]
            Ls = lt_counts(ta, tb)
            assert Ls[0] == (ta[0] + 1) * tb[0]
            for j in range(1, w):
                assert Ls[j] == (ta[j] + tb[j]) * (tb[j] + Ls[j - 1]) + Ls[j - 1]
            assert c_L(lib, w, ta, tb) == lt_terms(ta, tb) == Ls[-1]
    assert c_L(lib, 3, [2, 1, 3], [1, 2, 1]) == (3 + 1) * (1 + ((1 + 2) * (2 + 3) + 3)) + 18 == 94


def test_terms_invalid(lib):
    one = [1] * 17
    assert c_L(lib, 0, one, one) == 0                                 # width outside 1..16
    assert c_L(lib, 17, one, one) == 0
    assert c_L(lib, 16, one, one) == 3 ** 16 - 1
    assert c_L(lib, 4, None, one) == 0                                # null pointers
    assert c_L(lib, 4, one, None) == 0
    assert c_L(lib, 3, [1, 0, 1], one) == 0                           # a plane of no terms
    assert c_L(lib, 3, one, [1, 1, 0]) == 0
    # 2^62 or more
    assert c_L(lib, 1, [LIMIT - 2], [1]) == LIMIT - 1
    assert c_L(lib, 1, [LIMIT - 1], [1]) == 0
    assert c_L(lib, 1, [1], [LIMIT]) == 0 and c_L(lib, 1, [LIMIT], [1]) == 0
    assert c_L(lib, 1, [1], [(LIMIT >> 1) - 1]) == LIMIT - 2
    assert c_L(lib, 1, [1], [LIMIT >> 1]) == 0
    assert c_L(lib, 2, [1, 1 << 61], [1, 1]) == 0                     # the step's product
    assert c_L(lib, 2, [1, 1 << 60], [1, 1]) == ((1 << 60) + 1) * 3 + 2
    assert c_L(lib, 2, [(1 << 60) - 1, 1], [1, 1]) == 2 * (1 + (1 << 60)) + (1 << 60)
    assert c_L(lib, 2, [(LIMIT // 3), 1], [1, 1]) == 0                # the step's sum: 3 * L_0 + 2 reaches 2^62
    assert c_L(lib, 4, [1 << 16] * 4, one) == 0


def test_dispatch_names(lib, knobs):
    from csgn_amd import capi
    assert "uint_lt_select_form" in capi.tuning_names()
    knobs.unset("uint_lt_select_form")
    assert capi.get_tuning("uint_lt_select_form") == -1

    def name(n, w, ta, tb, m, tx, ty, less=0):
        return lib.csgn_uint_lt_select_kernel(n, 256, w, u64s(ta), u64s(tb), m, u64s(tx), u64s(ty), less).decode()

    one = [1] * 64
    bench = [(2, 4), (4, 8), (8, 16), (8, 32), (8, 8)]                # the measured shapes: w, requests
    for form, want in ((1, "k_uint_lt_select"), (0, "composed")):
        knobs.set("uint_lt_select_form", form)
        assert capi.get_tuning("uint_lt_select_form") == form
        for w, m in bench:
            assert name(1247, w, one, one, m, one, one) == want
        assert name(1247, 3, [2, 1, 3], [1, 2, 1], 2, [1, 2], [3, 1], 1) == want
        assert name(1247, 2, one, one, 0, [], [], 1) == want          # the comparison alone
        assert name(0, 4, one, one, 8, one, one) == ""                # n_bits 0
        assert name(1247, 0, one, one, 8, one, one) == ""             # bad width
        assert name(1247, 17, one, one, 8, one, one) == ""
        assert name(1247, 4, one, one, 65, [1] * 65, [1] * 65) == ""  # more than 64 requests
        assert name(1247, 4, one, one, 0, [], []) == ""               # nothing to compute
        assert name(1247, 4, [1, 0, 1, 1], one, 2, one, one) == ""    # a plane of no terms
        assert name(1247, 4, one, [1, 1, 1, 0], 2, one, one) == ""
        assert name(1247, 4, one, one, 2, [1, 0], one) == "" and name(1247, 4, one, one, 2, one, [0, 1]) == ""
        assert lib.csgn_uint_lt_select_kernel(1247, 1, 4, None, u64s(one), 1, u64s(one), u64s(one), 0) == b""
        assert lib.csgn_uint_lt_select_kernel(1247, 1, 4, u64s(one), u64s(one), 1, None, u64s(one), 0) == b""
    knobs.unset("uint_lt_select_form")
    for w, m in bench:
        assert name(1247, w, one, one, m, one, one) in ("k_uint_lt_select", "composed")


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits, the width, the requests, host pointers, term counts
    (INVALID), 2^31 words per element and 2^60 per batch (UNSUPPORTED), null device pointers (INVALID), and only then
    the device (NO_DEVICE on a box without one; with one, the calls that pass every check are not made: their pointers
    are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 64)(*([p] * 64))
    nullp = (C.c_void_p * 64)(*([p] * 3 + [None] + [p] * 60))
    one = u64s([1] * 64)
    zero_first = u64s([0] + [1] * 63)
    huge = u64s([1 << 61] * 64)

    def sel(n=1247, batch=4, w=8, a=ptrs, ta=one, b=ptrs, tb=one, m=8, x=ptrs, tx=one, y=ptrs, ty=one, out=ptrs,
            less=None):
        return lib.csgn_uint_lt_select(n, batch, w, a, ta, b, tb, m, x, tx, y, ty, out, less, None)

    # each failing check wins over every later one
    assert sel(n=0, w=0, m=65, a=None) == -1                          # n_bits
    assert sel(n=131073) == -2
    assert sel(w=0, m=65) == -1 and sel(w=17, a=None) == -1           # width
    assert b"width" in lib.csgn_last_error()
    assert sel(m=65, a=None) == -1                                    # requests
    assert sel(m=0, a=None) == -1                                     # none, and no comparison
    for arg in ("a", "ta", "b", "tb", "x", "tx", "y", "ty", "out"):   # host pointers, before the term counts
        assert sel(**{arg: None, "tb": None if arg == "tb" else zero_first}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    assert sel(ta=zero_first) == -1 and sel(tb=zero_first) == -1      # term counts
    assert sel(tx=zero_first) == -1 and sel(ty=zero_first) == -1
    assert sel(ta=huge, batch=1 << 50) == -1                          # L >= 2^62 is INVALID, not UNSUPPORTED
    assert sel(tx=u64s([1 << 62] * 8), batch=1 << 50) == -1
    assert sel(m=0, less=p, x=None, tx=None, y=None, ty=None, out=None, ta=zero_first) == -1
    # sizes: (3^16 - 1) * 2 + 1 terms of 20 words = 1.7e9 < 2^31; a third term passes it
    assert sel(w=16, m=1, tx=u64s([3]), a=nullp) == -2
    assert sel(w=16, m=1, ty=u64s([2])) == -2
    assert sel(w=16, m=1, ta=u64s([2] * 16)) == -2
    assert sel(w=16, m=0, less=p, tb=u64s([2] * 16)) == -2            # the comparison alone is sized too
    assert sel(w=2, m=1, tx=u64s([1 << 61])) == -2                    # L * (tx + ty) past 2^62
    assert sel(batch=1 << 44, a=nullp) == -2                          # per batch
    assert sel(w=1, m=1, batch=1 << 59, n=64) == -2
    assert b"batch" in lib.csgn_last_error()
    for arg in ("a", "b", "x", "y", "out"):                           # a null device pointer inside each host array
        assert sel(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert sel(batch=0, x=nullp) == -1
    if gpu:
        return
    # no device: every call that passes the checks above, the empty batch included
    assert sel() == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert sel(w=16, m=1) == -3 and sel(w=16, m=0, less=p) == -3
    assert sel(m=0, less=p, x=None, tx=None, y=None, ty=None, out=None) == -3
    assert sel(less=p) == -3 and sel(batch=0) == -3
    assert sel(m=3, x=nullp, y=nullp, out=nullp) == -3                # only the first n_out entries are read


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
CASES = [  # (terms of a's planes, of b's planes, tx, ty)
    ([1], [1], 1, 1),
    ([2], [3], 1, 2),
    ([1, 1], [1, 1], 1, 1),
    ([2, 1, 3], [1, 2, 1], 2, 1),
    ([1] * 4, [1] * 4, 1, 1),
    ([1, 2], [3, 1], 3, 2),
]


def case_planes(n, batch, case, seed):
    ta, tb, tx, ty = CASES[case]
    a = [rand_terms(n, batch, t, seed + k) for k, t in enumerate(ta)]
    b = [rand_terms(n, batch, t, seed + 20 + k) for k, t in enumerate(tb)]
    return a, b, [rand_terms(n, batch, tx, seed + 50)], [rand_terms(n, batch, ty, seed + 51)]


@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("less", [False, True], ids=["plain", "less"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_definition_matches_reference(oracle, ref, n, d, case, less):
    ta, tb, tx, ty = CASES[case]
    a, b, xs, ys = case_planes(n, 1, case, 3000 * case + n)
    flat = lambda planes: [p[0].ravel() for p in planes]              # noqa: E731
    one = const_term(n, 1)
    add, mul = ref_ops(ref, n, d)
    want, want_l = compose_lt_select(flat(a), flat(b), flat(xs), flat(ys), add, mul, one, less)
    add, mul = oracle_ops(oracle, n)
    got, got_l = compose_lt_select(flat(a), flat(b), flat(xs), flat(ys), add, mul, one, less)
    words, words_l = np_lt_select(n, a, b, xs, ys, less)
    dl = (n + 63) // 64
    L = lt_terms(ta, tb)
    assert np.array_equal(got[0], want[0])
    assert got[0].size == out_terms(L, tx, ty) * dl
    assert np.array_equal(words[0].ravel(), got[0])
    if less:
        assert np.array_equal(got_l, want_l) and got_l.size == L * dl
        assert np.array_equal(words_l.ravel(), got_l)
    else:
        assert want_l is None and got_l is None and words_l is None


@pytest.mark.parametrize("case", range(len(CASES)))
def test_decode_gives_the_definition(case):
    """The factors csgn_uint_lt_select.hip decodes reproduce the definition's words term for term, and so does the
    numpy form the device tests compare with."""
    n, batch = 129, 2
    a, b, xs, ys = case_planes(n, batch, case, 90 + case)
    xs, ys = xs + [a[0], b[-1]], ys + [b[0], b[-1]]                    # requests that alias the operands
    want, want_l = np_lt_select(n, a, b, xs, ys, True)
    for form in (np_lt_select_decoded, np_lt_select_fast):
        got, got_l = form(n, a, b, xs, ys, True)
        for i in range(len(xs)):
            assert np.array_equal(got[i], want[i]), (form.__name__, i)
        assert np.array_equal(got_l, want_l), form.__name__
        assert form(n, a, b, xs, ys)[1] is None
    only_l = np_lt_select_fast(n, a, b, [], [], True)
    assert only_l[0] == [] and np.array_equal(only_l[1], want_l)
    assert np.array_equal(np_uint_select(n, want_l, xs, ys)[0], want[0])


def test_decode_fresh_subsets():
    """Fresh planes: term q is Pa[Sa] & Pb[Sb].  The eight terms of w = 2 in order; for w = 4 the 80 entries are
    distinct as words."""
    assert [fresh_subsets(q, 2) for q in range(8)] == [(2, 2), (3, 1), (2, 1), (0, 2), (1, 3), (0, 3), (1, 1), (0, 1)]
    assert [fresh_subsets(q, 1) for q in range(2)] == [(1, 1), (0, 1)]
    assert decode(3, [2], [3]) == [("a", 0, 1), ("b", 0, 0)] and decode(8, [2], [3]) == [("b", 0, 2)]
    n, w = 129, 4
    a = [rand_terms(n, 1, 1, 170 + k) for k in range(w)]
    b = [rand_terms(n, 1, 1, 180 + k) for k in range(w)]
    lt = np_lt_decoded(n, a, b)
    assert lt.shape[1] == 80 and np.array_equal(lt, np_uint_lt(n, a, b))
    assert len({lt[0, q].tobytes() for q in range(80)}) == 80
    seen = [fresh_subsets(q, w) for q in range(80)]
    assert all(sb for _, sb in seen) and len(set(seen)) == 80         # every term has a factor of b


# -- decryptions -------------------------------------------------------------------------------------------------------
def exchange(n, a, b, pa, pb):
    """min, max and both payloads of a compare-exchange as one set of requests: (lo, hi, plo, phi) after np_lt_select."""
    w, pw = len(a), len(pa)
    xs, ys = minmax_requests(a, b)
    pxs, pys = minmax_requests(pa, pb)
    outs, _ = np_lt_select(n, a, b, xs + pxs, ys + pys)
    return outs[:w], outs[w:2 * w], outs[2 * w:2 * w + pw], outs[2 * w + pw:]


def check_exchange(oracle, n, key, got, av, bv, pav, pbv):
    lo, hi, plo, phi = (decrypt_value(oracle, n, key, o) for o in got)
    less = av < bv
    assert np.array_equal(lo, np.minimum(av, bv)) and np.array_equal(hi, np.maximum(av, bv))
    assert np.array_equal(plo, np.where(less, pav, pbv)) and np.array_equal(phi, np.where(less, pbv, pav))


@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_compare_exchange_decrypts(oracle, w):
    """Every pair (a, b) for w <= 3; for w = 4, 64 drawn pairs and every tie.  A tie takes Y: the payloads stay put."""
    n, d, pw = 127, 8, 2
    key, _ = oracle.keygen(n, d, glibc_draws(470 + w, 64 * d + 64))
    rng = np.random.default_rng(50 + w)
    if w <= 3:
        av, bv = (g.ravel().astype(np.uint64) for g in np.meshgrid(np.arange(1 << w), np.arange(1 << w)))
    else:
        ties = np.arange(1 << w)
        av = np.concatenate([rng.integers(0, 1 << w, 64), ties]).astype(np.uint64)
        bv = np.concatenate([rng.integers(0, 1 << w, 64), ties]).astype(np.uint64)
    pav = rng.integers(0, 1 << pw, len(av)).astype(np.uint64)
    pbv = (pav ^ np.uint64(1 + len(av) % 3)) & np.uint64((1 << pw) - 1)        # differs from pa in every element
    a = encrypt_planes(oracle, n, key, av, w, 480 + w)
    b = encrypt_planes(oracle, n, key, bv, w, 485 + w)
    pa = encrypt_planes(oracle, n, key, pav, pw, 490 + w)
    pb = encrypt_planes(oracle, n, key, pbv, pw, 495 + w)
    assert (av == bv).any() and (av < bv).any() and (av > bv).any()
    check_exchange(oracle, n, key, exchange(n, a, b, pa, pb), av, bv, pav, pbv)
    _, lt = np_lt_select(n, a, b, [], [], True)
    assert np.array_equal(decrypt_bits(oracle, n, key, lt), av < bv)


def test_multi_term_planes_decrypt_the_same(oracle):
    """Planes that are sums (x + ZERO + ZERO: more terms, the same bit) select the same values."""
    n, d, w, pw = 127, 8, 3, 2
    key, _ = oracle.keygen(n, d, glibc_draws(501, 64 * d + 64))
    av = np.array([5, 2, 7, 3, 0, 6], dtype=np.uint64)
    bv = np.array([2, 5, 7, 4, 0, 1], dtype=np.uint64)
    pav = np.array([1, 2, 3, 0, 1, 2], dtype=np.uint64)
    pbv = np.array([3, 0, 1, 2, 2, 1], dtype=np.uint64)
    a = encrypt_planes(oracle, n, key, av, w, 502)
    b = encrypt_planes(oracle, n, key, bv, w, 503)
    pa = encrypt_planes(oracle, n, key, pav, pw, 504)
    pb = encrypt_planes(oracle, n, key, pbv, pw, 505)
    z = encrypt_planes(oracle, n, key, np.zeros(len(av), dtype=np.uint64), 1, 506)[0]
    a = [np_add(a[0], z), a[1], np_add(np_add(a[2], z), z)]
    b = [b[0], np_add(b[1], z), b[2]]
    pa = [pa[0], np_add(pa[1], z)]
    got = exchange(n, a, b, pa, pb)
    L = lt_terms([2, 1, 3], [1, 2, 1])
    assert got[0][0].shape[1] == out_terms(L, 2, 1) and got[3][1].shape[1] == out_terms(L, 1, 2)
    check_exchange(oracle, n, key, got, av, bv, pav, pbv)
