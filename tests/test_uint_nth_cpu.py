"""The (slot + 1)-th row whose encrypted mask bit is set (csgn_uint_nth*) on a box without a GPU: the term counts
P_{r,s}, Q_s and T_lab against Python integers, the argument checks and their order, the loud failure without a device,
the term order the kernel decodes (restated in tests/model_nth.py), and the DEFINITION -- G_{r,s} the sum over the
degrees d with C(d, s) odd and the d-subsets of the rows above r of their product with m_r, the left-nested sums of
G_{r,s} * d_{r,j}, of G_{r,s} and of the G_{r,s} a label bit keeps -- pinned against the compiled reference and the
oracle, with decryptions of every mask under a random key.  The device side is tests/test_uint_nth_gpu.py."""
import ctypes as C
from math import comb

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, decrypt_bits, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms, ref_ops,  # noqa: F401
                         u64s)
from tests.model_first import np_first_fast
from tests.model_nth import (c_label_terms, c_terms, compose_nth, entries, kept_degrees, label_terms, np_nth,
                             np_nth_decoded, np_nth_fast, nth_terms)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_against_the_model(lib):
    for g in range(1, 11):
        for t in (1, 2, 3):
            for slot in range(g):
                P = [c_terms(lib, g, t, slot, r) for r in range(g)]
                assert P == [nth_terms(g, t, slot, r) for r in range(g)], (g, t, slot)
                assert all(p == 0 for p in P[:slot]) and all(p > 0 for p in P[slot:])
                assert c_terms(lib, g, t, slot, g) == sum(P) == nth_terms(g, t, slot, g), (g, t, slot)
                if g <= 6:
                    assert sum(P) == len(entries(g, t, slot)), (g, t, slot)
                for labels in (list(range(g)), [1 << r for r in range(g)], [5, 3, 6, 1 << 63, 9, 0, 7, 2, 1, 4][:g]):
                    for bit in (0, 1, 2, 3, g - 1, 63):
                        assert c_label_terms(lib, g, t, slot, labels, bit) == label_terms(g, t, slot, labels, bit)


def test_terms_figures(lib):
    """The figures of the issue, brute-forced there over every mask up to g = 8."""
    assert [c_terms(lib, 8, 1, s, 8) for s in range(8)] == [255, 127, 135, 71, 93, 29, 9, 1]
    assert c_terms(lib, 16, 1, 7, 16) == 12871 and c_terms(lib, 12, 1, 2, 12) == 2015
    assert c_terms(lib, 64, 1, 62, 64) == 65 and c_terms(lib, 64, 1, 61, 64) == 2017
    assert c_terms(lib, 64, 1, 60, 64) == 43745
    for g in range(1, 62):
        assert c_terms(lib, g, 1, 0, g) == (1 << g) - 1               # slot 0: csgn_uint_first's count
        assert c_terms(lib, g, 1, g - 1, g) == 1                      # the last slot: the AND of every row
    for g in range(1, 12):
        assert c_terms(lib, g, 2, 0, g) == 3 ** g - 1                 # sum of C(g, d+1) 2^(d+1)
    # the parity of C(d, s) is Lucas' submask rule
    assert all(kept_degrees(s, 40) == [d for d in range(s, 41) if s & ~d == 0] for s in range(41))


def test_terms_invalid_and_saturation(lib):
    assert c_terms(lib, 64, 1, 0, 64) == 0                            # 2^64 - 1: saturates, never wraps
    assert c_terms(lib, 63, 1, 0, 63) == 0 and c_terms(lib, 62, 1, 0, 62) == LIMIT - 1
    assert c_terms(lib, 64, 1, 0, 61) == 1 << 61 and c_terms(lib, 64, 1, 0, 62) == 0
    assert c_terms(lib, 64, 1, 1, 64) == 0                            # sum of the odd d of C(64, d + 1) = 2^63 - 1
    assert c_terms(lib, 64, 1, 32, 64) == 0                           # about 2^63
    assert c_terms(lib, 64, 1, 48, 64) == sum(comb(64, d + 1) for d in kept_degrees(48, 63)) == 224723513577529
    assert c_terms(lib, 64, 3, 63, 64) == 0                           # 3^64
    assert c_terms(lib, 0, 1, 0, 0) == 0 and c_terms(lib, 65, 1, 0, 3) == 0        # group outside 1..64
    assert c_terms(lib, 64, 1, 3, 3) == 1
    assert c_terms(lib, 4, 1, 4, 4) == 0 and c_terms(lib, 4, 1, 5, 2) == 0         # slot >= group
    assert c_terms(lib, 4, 0, 1, 4) == 0                              # t of 0
    assert c_terms(lib, 1, LIMIT - 1, 0, 0) == LIMIT - 1 and c_terms(lib, 1, LIMIT, 0, 0) == 0
    assert c_terms(lib, 1, LIMIT - 1, 0, 1) == LIMIT - 1
    assert c_terms(lib, 2, 1 << 31, 1, 2) == 0 and c_terms(lib, 2, (1 << 31) - 1, 1, 2) == ((1 << 31) - 1) ** 2
    assert c_terms(lib, 3, 1, 0, 4) == 0 and c_terms(lib, 3, 1, 0, 3) == 7         # row > group
    # label planes
    onehot = [1 << r for r in range(64)]
    assert c_label_terms(lib, 5, 2, 1, None, 0) == 0                  # null pointer
    assert c_label_terms(lib, 5, 2, 1, onehot, 64) == 0               # bit > 63
    assert c_label_terms(lib, 5, 2, 1, onehot, 0) == 0                # only row 0 has bit 0: below the slot
    assert c_label_terms(lib, 5, 2, 1, onehot, 1) == nth_terms(5, 2, 1, 1) == 4
    assert c_label_terms(lib, 5, 2, 1, list(range(5)), 3) == 0        # no label has the bit
    assert c_label_terms(lib, 0, 1, 0, onehot, 0) == 0 and c_label_terms(lib, 5, 1, 5, onehot, 0) == 0
    assert c_label_terms(lib, 5, 0, 1, onehot, 1) == 0
    assert c_label_terms(lib, 64, 1, 0, onehot, 5) == 32 and c_label_terms(lib, 64, 1, 0, onehot, 62) == 0
    assert c_label_terms(lib, 64, 1, 0, [1] * 64, 0) == 0             # the sum reaches 2^62


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits; group, slot, n_mask, width, n_labels, nothing asked
    for; host pointers; term counts and label bits (INVALID); 2^31 words per element and 2^60 per batch (UNSUPPORTED);
    null device pointers (INVALID); and only then the device (NO_DEVICE on a box without one; with one, the calls that
    pass every check are not made: their pointers are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 64)(*([p] * 64))
    nullp = (C.c_void_p * 64)(*([p] * 3 + [None] + [p] * 60))
    one = u64s([1] * 64)
    index = u64s(range(64))
    bits3 = u64s([0, 1, 2])

    def nth(n=1247, batch=4, g=8, slot=1, m=ptrs, nm=1, tm=1, w=8, d=ptrs, t=one, out=ptrs, valid=None, nl=0, L=None,
            lb=None, lo=None):
        return lib.csgn_uint_nth(n, batch, g, slot, m, nm, tm, w, d, t, out, valid, nl, L, lb, lo, None)

    # each failing check wins over every later one
    assert nth(n=0, g=0, m=None) == -1                                # n_bits
    assert nth(n=131073, g=0) == -2
    assert nth(g=0, m=None) == -1 and nth(g=65, m=None) == -1         # group
    assert b"group" in lib.csgn_last_error()
    assert nth(slot=8, m=None) == -1 and b"slot" in lib.csgn_last_error()     # slot
    assert nth(g=1, slot=1, m=None) == -1
    assert nth(nm=0, m=None) == -1 and nth(nm=7, m=None) == -1        # n_mask: 1 or the group
    assert nth(w=65, m=None) == -1 and nth(nl=65, m=None) == -1       # width, n_labels
    assert nth(w=0, m=None) == -1                                     # nothing asked for
    assert b"no value planes" in lib.csgn_last_error()
    for arg in ("m", "d", "t", "out"):                                # host pointers, before the term counts
        assert nth(**{arg: None, "tm": 0}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    for arg in ("L", "lb", "lo"):
        kw = {"nl": 3, "L": index, "lb": bits3, "lo": ptrs, "tm": 0}
        kw[arg] = None
        assert nth(**kw) == -1 and b"null host pointer" in lib.csgn_last_error(), arg
    assert nth(w=0, valid=p, d=None, t=None, out=None, tm=0) == -1    # not read at width 0 ...
    assert b"null host pointer" not in lib.csgn_last_error()          # ... so the term count fails
    assert nth(tm=0) == -1 and nth(tm=1 << 62) == -1                  # term counts
    assert nth(t=u64s([1, 1, 0] + [1] * 5)) == -1
    assert nth(g=64, nm=64, slot=0) == -1                             # Q >= 2^62 is INVALID, not UNSUPPORTED
    assert b"overflows" in lib.csgn_last_error()
    assert nth(g=8, nm=8, tm=1 << 61, batch=1 << 50) == -1
    lab = dict(nl=3, L=index, lb=bits3, lo=ptrs)
    assert nth(**dict(lab, lb=u64s([0, 2, 1]))) == -1                 # label bits: strictly ascending ...
    assert nth(**dict(lab, lb=u64s([0, 1, 1]))) == -1
    assert nth(**dict(lab, lb=u64s([0, 1, 64]))) == -1                # ... below 64 ...
    assert nth(**dict(lab, lb=u64s([0, 1, 3]))) == -1                 # ... of planes that exist (8 rows: bits 0..2)
    assert b"label bit 3" in lib.csgn_last_error()
    assert nth(slot=7, **dict(lab, nl=1, lb=u64s([3]))) == -1         # ... from the slot on: row 7 = 0b111 alone
    assert nth(slot=7, w=0, nl=1, L=u64s([1 << r for r in range(8)]), lb=u64s([6]), lo=ptrs) == -1
    assert nth(**dict(lab, lb=u64s([0, 1, 3]), batch=1 << 59)) == -1  # ... before the sizes
    # sizes: Q(27, 0) = 2^27 - 1, times 20 words is past 2^31; Q(24, 0) * 20 is below it, times 7 terms past it
    assert nth(g=27, slot=0, w=1) == -2 and nth(g=24, slot=0, w=1, t=u64s([7])) == -2
    assert nth(g=27, slot=0, w=0, valid=p) == -2                      # valid alone is sized too
    assert nth(g=27, slot=0, w=0, nl=1, L=u64s([1] + [0] * 26), lb=u64s([0]), lo=ptrs) == -2    # and the stream itself
    assert b"selector stream" in lib.csgn_last_error()
    assert nth(g=24, slot=0, w=1, nl=1, L=u64s([1 << 63] * 24), lb=u64s([63]), lo=ptrs, t=u64s([7])) == -2
    assert nth(g=14, slot=0, nm=14, tm=2, w=1, t=u64s([40])) == -2    # (3^14 - 1) * 40 * 20 words
    assert b"output 0" in lib.csgn_last_error()
    assert nth(batch=1 << 50) == -2                                   # per batch
    assert nth(g=1, slot=0, w=1, batch=1 << 60, n=64) == -2
    assert b"batch" in lib.csgn_last_error()
    assert nth(g=27, slot=0, w=1, m=nullp) == -2                      # sizes before null device pointers
    # null device pointers, inside each host array, before the device
    assert nth(g=8, nm=8, m=nullp) == -1 and b"null device pointer" in lib.csgn_last_error()
    assert nth(d=nullp) == -1 and nth(out=nullp) == -1
    assert nth(slot=0, nl=4, L=u64s([15] * 8), lb=u64s([0, 1, 2, 3]), lo=nullp) == -1
    assert b"label output 3" in lib.csgn_last_error()
    if gpu:
        return
    # no device: every call that passes the checks above, the empty batch and its null device pointers included
    assert nth() == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert nth(g=8, nm=8, tm=3, valid=p, **lab) == -3
    assert nth(g=24, slot=0, w=1) == -3 and nth(w=0, valid=p, d=None, t=None, out=None) == -3
    assert nth(w=0, **lab) == -3
    # the high slots of a 64-bit word, in the plane layout
    assert nth(g=64, nm=64, slot=61, w=0, valid=p, nl=2, L=index, lb=u64s([0, 5]), lo=ptrs) == -3
    assert nth(g=64, nm=64, slot=63, w=0, valid=p) == -3
    assert nth(batch=0) == -3 and nth(batch=0, m=nullp, d=nullp, out=nullp) == -3


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
def case_rows(n, batch, g, t, tv, seed):
    mask_rows = [rand_terms(n, batch, t, seed + r) for r in range(g)]
    value_rows = [[rand_terms(n, batch, tj, seed + 100 + 10 * r + j) for j, tj in enumerate(tv)] for r in range(g)]
    return mask_rows, value_rows


LABELS = [5, 3, 6, 1 << 63, 9]


@pytest.mark.parametrize("n,d", [(63, 4), (1247, 16)])
@pytest.mark.parametrize("g,t", [(g, t) for g in range(1, 6) for t in (1, 2)])
def test_decode_matches_reference_and_oracle(oracle, ref, n, d, g, t):
    """The literal nested-loop composition through the compiled reference's operators and through the oracle's, against
    the words decoded from the term order, word for word, for every slot."""
    tv = [2, 1]
    mask_rows, value_rows = case_rows(n, 1, g, t, tv, 3000 * g + 17 * t + n)
    flat_m = [m[0].ravel() for m in mask_rows]
    flat_v = [[x[0].ravel() for x in row] for row in value_rows]
    labels = LABELS[:g]
    dl = (n + 63) // 64
    for slot in range(g):
        want, want_valid, want_lab = compose_nth(flat_m, flat_v, labels, slot, *ref_ops(ref, n, d))
        got, got_valid, got_lab = compose_nth(flat_m, flat_v, labels, slot, *oracle_ops(oracle, n))
        words, words_valid, words_lab = np_nth_decoded(mask_rows, value_rows, slot, labels)
        Q = nth_terms(g, t, slot, g)
        for j in range(len(tv)):
            assert np.array_equal(got[j], want[j]), (slot, j)
            assert got[j].size == Q * tv[j] * dl
            assert np.array_equal(words[j].ravel(), got[j]), (slot, j)
        assert np.array_equal(got_valid, want_valid) and got_valid.size == Q * dl
        assert np.array_equal(words_valid.ravel(), got_valid), slot
        bits = [i for i in range(64) if label_terms(g, t, slot, labels, i)]
        assert sorted(got_lab) == sorted(want_lab) == sorted(words_lab) == bits
        for i in bits:
            assert np.array_equal(got_lab[i], want_lab[i]) and got_lab[i].size == label_terms(g, t, slot, labels, i) * dl
            assert np.array_equal(words_lab[i].ravel(), got_lab[i]), (slot, i)


@pytest.mark.parametrize("g,t", [(1, 1), (2, 3), (4, 2), (5, 1), (6, 1), (3, 3)])
def test_numpy_forms_agree(g, t):
    """The vectorised numpy form the device tests compare with gives the definition's and the decode's words."""
    n, batch, tv = 129, 2, [1, 2]
    mask_rows, value_rows = case_rows(n, batch, g, t, tv, 70 + g)
    labels = list(range(1, g + 1))
    for slot in range(g):
        want, want_valid, want_lab = np_nth(mask_rows, value_rows, slot, labels)
        for form in (np_nth_decoded, np_nth_fast):
            got, got_valid, got_lab = form(mask_rows, value_rows, slot, labels)
            for j in range(len(tv)):
                assert np.array_equal(got[j], want[j]), (form.__name__, slot, j)
            assert np.array_equal(got_valid, want_valid), (form.__name__, slot)
            assert sorted(got_lab) == sorted(want_lab)
            for i in want_lab:
                assert np.array_equal(got_lab[i], want_lab[i]), (form.__name__, slot, i)
            assert form(mask_rows, value_rows, slot)[2] == {}


def test_term_order_restated():
    """Blocks ascending in r, segments in d, subsets lexicographic, i_1's digit the slowest and m_r's the fastest."""
    assert entries(3, 1, 0) == [(0, [(0, 0)]), (1, [(1, 0)]), (1, [(0, 0), (1, 0)]), (2, [(2, 0)]),
                                (2, [(0, 0), (2, 0)]), (2, [(1, 0), (2, 0)]), (2, [(0, 0), (1, 0), (2, 0)])]
    assert [r for r, _ in entries(4, 1, 2)] == [2, 3, 3, 3, 3]        # d = 2 at r = 2; d = 2 and 3 at r = 3
    assert entries(4, 1, 2)[1:] == [(3, [(0, 0), (1, 0), (3, 0)]), (3, [(0, 0), (2, 0), (3, 0)]),
                                    (3, [(1, 0), (2, 0), (3, 0)]), (3, [(0, 0), (1, 0), (2, 0), (3, 0)])]
    assert [r for r, _ in entries(5, 1, 1)] == [1] + [2] * 2 + [3] * 4 + [4] * 8      # d = 2 is never kept: C(2, 1) even
    assert entries(2, 2, 1) == [(1, [(0, a), (1, b)]) for a in range(2) for b in range(2)]
    assert kept_degrees(2, 7) == [2, 3, 6, 7] and kept_degrees(0, 3) == [0, 1, 2, 3] and kept_degrees(1, 6) == [1, 3, 5]


def test_slot_0_has_the_terms_of_first():
    """Q(g, 0) = 2^g - 1: slot 0's valid stream is csgn_uint_first's any stream as a multiset of terms, in another
    order (over F2, ~m_0 * ... * ~m_{r-1} * m_r expands to the subsets of the rows above r, times m_r)."""
    n, batch = 129, 2
    for g, t in ((1, 2), (3, 1), (4, 2), (6, 1)):
        mask_rows, value_rows = case_rows(n, batch, g, t, [], 900 + g)
        _, valid, _ = np_nth_fast(mask_rows, value_rows, 0)
        _, first, _ = np_first_fast(n, mask_rows, value_rows)
        # csgn_uint_first's ONE digits leave a row out: its terms, ONE apart, are the products of the same subsets
        assert first.shape == valid.shape == (batch, nth_terms(g, t, 0, g), valid.shape[2])
        for e in range(batch):
            assert sorted(map(bytes, valid[e])) == sorted(map(bytes, first[e])), (g, t, e)


# -- decryptions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(1, 7))
def test_every_mask_and_slot_decrypts(oracle, g):
    """Every mask of g rows, the zero mask included, and every slot: the value, the label and the index of the
    (slot + 1)-th set row, valid = "more than slot bits are set"; 0 everywhere when at most slot bits are set."""
    n, d, w = 127, 8, 3
    key, _ = oracle.keygen(n, d, glibc_draws(610 + g, 64 * d + 64))
    masks = np.arange(1 << g, dtype=np.uint64)
    mask_rows = encrypt_planes(oracle, n, key, masks, g, 620)         # plane r = row r of the 2^g elements
    vals = np.random.default_rng(63).integers(0, 1 << w, (len(masks), g)).astype(np.uint64)
    value_rows = [encrypt_planes(oracle, n, key, vals[:, r].copy(), w, 630 + r) for r in range(g)]
    labels = [9, 6, 9, 1 << 63, 3, 12][:g]
    for slot in range(g):
        set_rows = [[r for r in range(g) if (int(m) >> r) & 1] for m in masks]
        nth = [rows[slot] if len(rows) > slot else None for rows in set_rows]
        outs, valid, lab = np_nth_fast(mask_rows, value_rows, slot, labels)
        assert valid.shape[1] == nth_terms(g, 1, slot, g)
        assert [int(x) for x in decrypt_value(oracle, n, key, outs)] == \
            [0 if r is None else int(vals[e, r]) for e, r in enumerate(nth)], slot
        assert [int(b) for b in decrypt_bits(oracle, n, key, valid)] == [int(len(rows) > slot) for rows in set_rows], slot
        got = np.zeros(len(masks), dtype=object)
        for i, words in lab.items():
            got += decrypt_bits(oracle, n, key, words).astype(object) * (1 << i)
        assert [int(x) for x in got] == [0 if r is None else labels[r] for r in nth], slot
