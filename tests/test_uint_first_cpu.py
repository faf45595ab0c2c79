"""The first row whose encrypted mask bit is set (csgn_uint_first*) on a box without a GPU: the term counts P_r, Q and
T_lab against their closed forms, the argument checks and their order, the loud failure without a device, the term
order the kernel decodes (restated in tests/model_first.py), and the DEFINITION -- F_r = n_0 * ... * n_{r-1} * m_r, the
left-nested sums of F_r * d_{r,j}, of F_r and of the F_r a label bit keeps, a composition of the reference's operator+ /
operator* with ONE -- pinned against the compiled reference and the oracle, with decryptions under random keys.  The
device side is tests/test_uint_first_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, const_term, decrypt_bits, decrypt_value, encrypt_planes, lib, np_add, oracle_ops,
                         rand_terms, ref_ops, u64s)
from tests.model_first import (c_label_terms, c_terms, compose_first, entry_digits, first_terms, fresh_subset,
                               label_terms, np_first, np_first_decoded, np_first_fast)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_formula(lib):
    rng = np.random.default_rng(11)
    for g in range(1, 62):                                            # fresh: P_r = 2^r, Q = 2^g - 1
        one = [1] * g
        assert c_terms(lib, g, one, g) == (1 << g) - 1 == first_terms(one, g), g
        for r in range(g):
            assert c_terms(lib, g, one, r) == 1 << r, (g, r)
    for g in range(1, 17):                                            # mixed: the telescoping product
        for _ in range(4):
            s = [int(x) for x in rng.integers(1, 5, g)]
            Q = int(np.prod([x + 1 for x in s], dtype=object)) - 1
            P = [c_terms(lib, g, s, r) for r in range(g)]
            assert c_terms(lib, g, s, g) == Q == sum(P) == first_terms(s, g), s
            assert P == [first_terms(s, r) for r in range(g)]
            assert P == [s[r] * int(np.prod([x + 1 for x in s[:r]], dtype=object)) for r in range(g)]
    assert [c_terms(lib, 3, [2, 3, 1], r) for r in range(4)] == [2, 9, 12, 23]


def test_label_terms(lib):
    s = [2, 1, 3, 1, 2]
    P = [first_terms(s, r) for r in range(5)]
    index = list(range(5))
    for bit in range(3):
        assert c_label_terms(lib, 5, s, index, bit) == sum(P[r] for r in range(5) if (r >> bit) & 1) \
            == label_terms(s, index, bit)
    assert c_label_terms(lib, 5, s, index, 3) == 0                    # no label has the bit: no such plane
    onehot = [1 << r for r in range(5)]
    assert [c_label_terms(lib, 5, s, onehot, b) for b in range(6)] == P + [0]
    assert c_label_terms(lib, 5, s, [(1 << 64) - 1] * 5, 63) == sum(P)
    assert c_label_terms(lib, 5, s, onehot, 64) == 0                  # bit > 63
    assert c_label_terms(lib, 5, None, onehot, 0) == 0 and c_label_terms(lib, 5, s, None, 0) == 0
    assert c_label_terms(lib, 0, s, onehot, 0) == 0 and c_label_terms(lib, 65, [1] * 65, [1] * 65, 0) == 0
    assert c_label_terms(lib, 5, [2, 1, 0, 1, 2], onehot, 0) == 0     # a row of no terms, even a skipped one
    # a plane of low rows alone exists though Q is past 2^62; one that keeps a row past it does not
    wide = [1] * 64
    assert c_terms(lib, 64, wide, 64) == 0
    assert c_label_terms(lib, 64, wide, [1 << r for r in range(64)], 5) == 32
    assert c_label_terms(lib, 64, wide, [1 << r for r in range(64)], 61) == 1 << 61
    assert c_label_terms(lib, 64, wide, [1 << r for r in range(64)], 62) == 0
    assert c_label_terms(lib, 64, wide, [1] * 64, 0) == 0             # the sum reaches 2^62


def test_terms_invalid(lib):
    one = [1] * 65
    assert c_terms(lib, 0, one, 0) == 0                               # group outside 1..64
    assert c_terms(lib, 65, one, 3) == 0
    assert c_terms(lib, 64, one, 3) == 8
    assert c_terms(lib, 4, None, 4) == 0                              # null pointer
    assert c_terms(lib, 3, [1, 0, 1], 3) == 0                         # a row of no terms, whichever row is asked for
    assert c_terms(lib, 3, [1, 1, 0], 0) == 0
    assert c_terms(lib, 3, one, 4) == 0                               # row > group
    assert c_terms(lib, 3, one, 3) == 7
    # 2^62 or more
    assert c_terms(lib, 63, one, 63) == 0 and c_terms(lib, 62, one, 62) == LIMIT - 1    # Q itself, not Q + 1
    assert c_terms(lib, 64, one, 61) == 1 << 61 and c_terms(lib, 64, one, 62) == 0
    assert c_terms(lib, 1, [LIMIT - 1], 0) == LIMIT - 1 and c_terms(lib, 1, [LIMIT], 0) == 0
    assert c_terms(lib, 1, [LIMIT - 1], 1) == LIMIT - 1 and c_terms(lib, 2, [LIMIT - 1, 1], 2) == 0
    assert c_terms(lib, 2, [(1 << 31) - 1, 1 << 30], 1) == 1 << 61
    assert c_terms(lib, 2, [(1 << 31) - 1, 1 << 31], 1) == 0
    assert c_terms(lib, 2, [(1 << 31) - 1, (1 << 31) - 1], 2) == LIMIT - 1
    assert c_terms(lib, 2, [(1 << 31) - 1, 1 << 31], 2) == 0
    assert c_terms(lib, 2, [(1 << 31) - 1, 1 << 31], 0) == (1 << 31) - 1


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits; group, n_mask, width, n_labels, nothing asked for; host
    pointers; term counts, label bits and the grouped layout's counts (INVALID); 2^31 words per element and 2^60 per
    batch (UNSUPPORTED); null device pointers (INVALID); and only then the device (NO_DEVICE on a box without one; with
    one, the calls that pass every check are not made: their pointers are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 64)(*([p] * 64))
    nullp = (C.c_void_p * 64)(*([p] * 3 + [None] + [p] * 60))
    one = u64s([1] * 64)
    zero_row = u64s([1, 0] + [1] * 62)
    index = u64s(range(64))
    bits3 = u64s([0, 1, 2])

    def first(n=1247, batch=4, g=8, m=ptrs, nm=1, s=one, w=8, d=ptrs, t=one, out=ptrs, any_=None, nl=0, L=None, lb=None,
              lo=None):
        return lib.csgn_uint_first(n, batch, g, m, nm, s, w, d, t, out, any_, nl, L, lb, lo, None)

    # each failing check wins over every later one
    assert first(n=0, g=0, m=None) == -1                              # n_bits
    assert first(n=131073, g=0) == -2
    assert first(g=0, m=None) == -1 and first(g=65, m=None) == -1     # group
    assert b"group" in lib.csgn_last_error()
    assert first(nm=0, m=None) == -1 and first(nm=7, m=None) == -1    # n_mask: 1 or the group
    assert first(w=65, m=None) == -1 and first(nl=65, m=None) == -1   # width, n_labels
    assert first(w=0, m=None) == -1                                   # nothing asked for
    assert b"no value planes" in lib.csgn_last_error()
    for arg in ("m", "s", "d", "t", "out"):                           # host pointers, before the term counts
        assert first(**{arg: None, "s": None if arg == "s" else zero_row}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    for arg in ("L", "lb", "lo"):
        kw = {"nl": 3, "L": index, "lb": bits3, "lo": ptrs, "s": zero_row}
        kw[arg] = None
        assert first(**kw) == -1 and b"null host pointer" in lib.csgn_last_error(), arg
    assert first(w=0, any_=p, d=None, t=None, out=None, s=zero_row) == -1     # not read at width 0 ...
    assert b"null host pointer" not in lib.csgn_last_error()                  # ... so the term count fails
    assert first(s=zero_row) == -1                                    # term counts
    assert first(t=u64s([1, 1, 0] + [1] * 5)) == -1
    assert first(g=64, nm=64) == -1                                   # Q >= 2^62 is INVALID, not UNSUPPORTED
    assert first(g=8, nm=8, s=u64s([1 << 61] * 8), batch=1 << 50) == -1
    lab = dict(nl=3, L=index, lb=bits3, lo=ptrs)
    assert first(**dict(lab, lb=u64s([0, 2, 1]))) == -1               # label bits: strictly ascending ...
    assert first(**dict(lab, lb=u64s([0, 1, 1]))) == -1
    assert first(**dict(lab, lb=u64s([0, 1, 64]))) == -1              # ... below 64 ...
    assert first(**dict(lab, lb=u64s([0, 1, 3]))) == -1               # ... of planes that exist (8 rows: bits 0..2)
    assert b"no label has bit 3" in lib.csgn_last_error()
    assert first(g=2, nm=1, s=u64s([1, 2])) == -1                     # the grouped layout takes one count
    assert b"grouped" in lib.csgn_last_error()
    assert first(g=2, nm=1, s=u64s([1, 2]), batch=1 << 59) == -1      # ... before the sizes
    # sizes: (2^24 - 1) * 20 words = 3.4e8 < 2^31, (2^27 - 1) * 20 is past it
    assert first(g=27, w=1) == -2 and first(g=24, w=1, t=u64s([7])) == -2
    assert first(g=27, w=0, any_=p) == -2                             # any alone is sized too
    assert first(g=24, w=1, nl=1, L=u64s([1 << 63] * 24), lb=u64s([63]), lo=ptrs, t=u64s([7])) == -2
    assert first(g=40, nm=40, w=0, nl=1, L=u64s([1 << r for r in range(40)]), lb=u64s([39]), lo=ptrs) == -2
    assert b"label plane 39" in lib.csgn_last_error()
    assert first(batch=1 << 50) == -2                                 # per batch
    assert first(g=1, w=1, batch=1 << 60, n=64) == -2
    assert b"batch" in lib.csgn_last_error()
    assert first(g=27, w=1, m=nullp) == -2                            # sizes before null device pointers
    # null device pointers, inside each host array, before the device
    assert first(g=8, nm=8, m=nullp) == -1 and b"null device pointer" in lib.csgn_last_error()
    assert first(d=nullp) == -1 and first(out=nullp) == -1
    assert first(nl=4, L=u64s([15] * 8), lb=u64s([0, 1, 2, 3]), lo=nullp) == -1
    assert b"label output 3" in lib.csgn_last_error()
    if gpu:
        return
    # no device: every call that passes the checks above, the empty batch and its null device pointers included
    assert first() == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert first(g=8, nm=8, s=u64s([1, 2, 3, 1, 2, 3, 1, 2]), any_=p, **lab) == -3
    assert first(g=24, w=1) == -3 and first(w=0, any_=p, d=None, t=None, out=None) == -3
    assert first(w=0, **lab) == -3
    # label planes of the low rows alone, though Q is past 2^62
    assert first(g=64, nm=64, w=0, nl=2, L=u64s([1 << r for r in range(64)]), lb=u64s([0, 5]), lo=ptrs) == -3
    assert first(batch=0) == -3 and first(batch=0, m=nullp, d=nullp, out=nullp) == -3


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
CASES = [  # (mask terms s per row, value terms t, labels)
    ([1], [1], [1]),
    ([1, 1], [1, 2], [0, 1]),
    ([2, 1], [3], [1, 2]),
    ([1, 1, 1], [1, 1], [0, 1, 2]),
    ([2, 1, 3], [2, 1], [1, 2, 4]),
    ([1] * 5, [1, 2], list(range(5))),
    ([1, 2, 1, 3, 1], [1], [5, 3, 6, 1 << 63, 9]),
]


def case_rows(n, batch, s, t, seed):
    mask_rows = [rand_terms(n, batch, sr, seed + r) for r, sr in enumerate(s)]
    value_rows = [[rand_terms(n, batch, tj, seed + 100 + 10 * r + j) for j, tj in enumerate(t)] for r in range(len(s))]
    return mask_rows, value_rows


@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_definition_matches_reference(oracle, ref, n, d, case):
    s, t, labels = CASES[case]
    g = len(s)
    mask_rows, value_rows = case_rows(n, 1, s, t, 3000 * case + n)
    flat_m = [m[0].ravel() for m in mask_rows]
    flat_v = [[x[0].ravel() for x in row] for row in value_rows]
    one = const_term(n, 1)
    add, mul = ref_ops(ref, n, d)
    want, want_any, want_lab = compose_first(flat_m, flat_v, labels, add, mul, one)
    add, mul = oracle_ops(oracle, n)
    got, got_any, got_lab = compose_first(flat_m, flat_v, labels, add, mul, one)
    words, words_any, words_lab = np_first(n, mask_rows, value_rows, labels)
    dl = (n + 63) // 64
    Q = first_terms(s, g)
    for j in range(len(t)):
        assert np.array_equal(got[j], want[j]), j
        assert got[j].size == Q * t[j] * dl
        assert np.array_equal(words[j].ravel(), got[j]), j
    assert np.array_equal(got_any, want_any) and got_any.size == Q * dl
    assert np.array_equal(words_any.ravel(), got_any)
    assert sorted(got_lab) == sorted(want_lab) == sorted(words_lab) == [i for i in range(64) if label_terms(s, labels, i)]
    for i in got_lab:
        assert np.array_equal(got_lab[i], want_lab[i]) and got_lab[i].size == label_terms(s, labels, i) * dl, i
        assert np.array_equal(words_lab[i].ravel(), got_lab[i]), i


@pytest.mark.parametrize("case", range(len(CASES)))
def test_decode_gives_the_definition(case):
    """The digits csgn_uint_first.hip decodes reproduce the definition's words term for term, and so does the
    vectorised numpy form the device tests compare with."""
    s, t, labels = CASES[case]
    n, batch = 129, 2
    mask_rows, value_rows = case_rows(n, batch, s, t, 70 + case)
    want, want_any, want_lab = np_first(n, mask_rows, value_rows, labels)
    for form in (np_first_decoded, np_first_fast):
        got, got_any, got_lab = form(n, mask_rows, value_rows, labels)
        for j in range(len(t)):
            assert np.array_equal(got[j], want[j]), (form.__name__, j)
        assert np.array_equal(got_any, want_any), form.__name__
        assert sorted(got_lab) == sorted(want_lab)
        for i in want_lab:
            assert np.array_equal(got_lab[i], want_lab[i]), (form.__name__, i)
        assert form(n, mask_rows, value_rows)[2] == {}


def test_decode_fresh_subsets():
    """Fresh rows: entry q of row r = the top bit of q + 1 is m_r AND a subset of the rows below; every subset appears
    exactly once, n_0 is the slowest digit and digit 0 takes the row."""
    g = 5
    seen = [fresh_subset(q) for q in range((1 << g) - 1)]
    assert [r for r, _ in seen] == [r for r in range(g) for _ in range(1 << r)]
    assert all(S >> r == 1 for r, S in seen)
    assert len({S for _, S in seen}) == (1 << g) - 1
    assert seen[0] == (0, 1) and seen[1] == (1, 3) and seen[2] == (1, 2)
    assert seen[3:7] == [(2, 7), (2, 5), (2, 6), (2, 4)]              # digits (n_0, n_1) = 00, 01, 10, 11
    assert entry_digits(2, 1 * 8 + 3 * 2 + 1, [2, 3, 2]) == (1, [1, 3])       # radices 3, 4, 2: ONE is digit s_x
    assert entry_digits(2, 2 * 8 + 0 * 2 + 0, [2, 3, 2]) == (0, [2, 0])


# -- decryptions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [False, True], ids=["fresh", "multi"])
def test_every_mask_pattern_decrypts(oracle, multi):
    """Every mask of g = 4, the zero mask included: the value of the first set row, any = OR, the index of the first
    set row and its one-hot word; 0 everywhere when no bit is set.  multi: rows that are sums (m + ZERO ...: more
    terms, the same bit)."""
    n, d, g, w = 127, 8, 4, 5
    key, _ = oracle.keygen(n, d, glibc_draws(510 + multi, 64 * d + 64))
    masks = np.arange(1 << g, dtype=np.uint64)
    mask_rows = encrypt_planes(oracle, n, key, masks, g, 520)         # plane r = row r of the 16 elements
    vals = np.random.default_rng(53).integers(0, 1 << w, (len(masks), g)).astype(np.uint64)
    value_rows = [encrypt_planes(oracle, n, key, vals[:, r].copy(), w, 530 + r) for r in range(g)]
    if multi:
        z = encrypt_planes(oracle, n, key, np.zeros(len(masks), dtype=np.uint64), 1, 540)[0]
        mask_rows = [np_add(mask_rows[0], z), mask_rows[1], np_add(np_add(mask_rows[2], z), z), mask_rows[3]]
        value_rows = [[np_add(x, z) if j == 0 else x for j, x in enumerate(row)] for row in value_rows]
    first = [next((r for r in range(g) if (int(m) >> r) & 1), None) for m in masks]
    for labels, want in ((list(range(g)), [0 if r is None else r for r in first]),
                         ([1 << r for r in range(g)], [0 if r is None else 1 << r for r in first]),
                         ([9, 6, 9, 1 << 63], [0 if r is None else [9, 6, 9, 1 << 63][r] for r in first])):
        outs, any_, lab = np_first(n, mask_rows, value_rows, labels)
        if multi:
            assert any_.shape[1] == first_terms([2, 1, 3, 1], g) and outs[0].shape[1] == 2 * any_.shape[1]
        assert [int(x) for x in decrypt_value(oracle, n, key, outs)] == \
            [0 if r is None else int(vals[e, r]) for e, r in enumerate(first)]
        assert [int(b) for b in decrypt_bits(oracle, n, key, any_)] == [int(m != 0) for m in masks]
        got = np.zeros(len(masks), dtype=object)
        for i, words in lab.items():
            got += decrypt_bits(oracle, n, key, words).astype(object) * (1 << i)
        assert [int(x) for x in got] == want, labels
