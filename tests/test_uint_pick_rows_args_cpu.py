"""csgn_uint_pick_rows on a box without a GPU: what the launching call decides BEFORE it launches, asked of the host-only
csgn_uint_pick_rows_check; the walk of the kernel's lanes -- the search of the rows' output offsets and the division by
the row's T, the very inline function the device code calls -- through csgn_uint_pick_rows_decode against the model's
decode for every position; the form csgn_uint_pick_rows_kernel names and its knob.

The rule of this file, and of tests/test_uint_pick_rows_gpu.py: whether a size is refused is asked of
csgn_uint_pick_rows_check.  The launching entry is called with a refused argument only here, with pointers that are
never dereferenced, and only after an assertion that the check refuses the identical arguments (refused_by_both)."""
import bisect
import ctypes as C

import pytest

from tests.model import LIMIT, lib, read_terms, u64s  # noqa: F401
from tests.model_pick import decode
from tests.model_pick_rows import rows_offsets, write_shaped
from tests.model_write import row_terms
from tests.test_uint_pick_rows_cpu import INDEX_TERMS, row_counts, row_tables

OK, INVALID, UNSUPPORTED = 0, -1, -2
FAKE = 0x1000                           # a device pointer that is never dereferenced: the size checks come first


def flat(T):
    return [t for plane in T for t in plane]


def args(n_bits, batch, s, n, T):
    """(n_bits, batch, v, s, rows, width, row terms) of the check, the name function and the launching entry"""
    return (n_bits, batch, len(s), u64s(s), n, len(T), u64s(flat(T)))


def check(lib, n_bits, batch, s, n, T):
    return lib.csgn_uint_pick_rows_check(*args(n_bits, batch, s, n, T))


def kernel(lib, n_bits, batch, s, n, T):
    return lib.csgn_uint_pick_rows_kernel(*args(n_bits, batch, s, n, T)).decode()


def launch(lib, n_bits, batch, s, n, T):
    """The launching entry over host arrays of never-dereferenced device pointers."""
    a = args(n_bits, batch, s, n, T)
    x = (C.c_void_p * 16)(*([FAKE] * 16))
    p = (C.c_void_p * 64)(*([FAKE] * 64))
    return lib.csgn_uint_pick_rows(a[0], a[1], a[2], x, a[3], a[4], a[5], p, a[6], p, None)


def refused_by_both(lib, status, n_bits, batch, s, n, T):
    """The check refuses these arguments -- asserted first --, and so, with the same status, does the launching entry."""
    assert check(lib, n_bits, batch, s, n, T) == status, (n_bits, batch, s, n)
    assert launch(lib, n_bits, batch, s, n, T) == status, (n_bits, batch, s, n)


# -- the decode -------------------------------------------------------------------------------------------------------
def model_decode(s, T, out, qstart, p):
    """np_pick_rows_decoded's decode of position p (tests/model_pick_rows.py): the last row whose block begins at or
    before p, then p - out(r) = in * T[r] + c; the entry qstart(r) + in of the E stream must decode to row r."""
    n = len(T)
    r = bisect.bisect_right(out, p, 0, n) - 1
    i, c = divmod(p - out[r], T[r])
    return r, i, c


class Decoder:
    """csgn_uint_pick_rows_decode of one table, its arguments converted once"""

    def __init__(self, lib, s, T):
        self.lib, self.v, self.n = lib, len(s), len(T)
        self.s, self.T, self.out = u64s(s), u64s(T), (C.c_uint64 * 3)()

    def __call__(self, p):
        rc = self.lib.csgn_uint_pick_rows_decode(self.v, self.s, self.n, self.T, p, self.out)
        return rc, tuple(int(x) for x in self.out)


@pytest.mark.parametrize("s", INDEX_TERMS, ids=str)
def test_decode_every_position(lib, s):
    v = len(s)
    for n in row_counts(v):
        qstart = [read_terms(s, r) if r else 0 for r in range(n)]
        for T in row_tables(s, n, 10 * v + n):
            _, out = rows_offsets(s, T)
            dec = Decoder(lib, s, T)
            for p in range(out[-1]):
                want = model_decode(s, T, out, qstart, p)
                assert dec(p) == (OK, want), (n, T, p)
                row, _ = decode(qstart[want[0]] + want[1], s, n)        # the E-stream entry lies in that row
                assert row == want[0] and want[1] < row_terms(s, want[0])
            assert dec(out[-1])[0] == INVALID                           # the position past the output


def ends_of_every_block(lib, s, T):
    _, out = rows_offsets(s, T)
    dec = Decoder(lib, s, T)
    for r in range(len(T)):
        assert dec(out[r]) == (OK, (r, 0, 0)), r
        assert dec(out[r + 1] - 1) == (OK, (r, row_terms(s, r) - 1, T[r] - 1)), r
    return out[-1]


def test_decode_block_ends_of_a_written_table(lib):
    """v = 8, n = 256, written from one-term planes: the first and last position of every row's block."""
    s = [1] * 8
    assert ends_of_every_block(lib, s, write_shaped(s, 256)) == 2 * 5 ** 8 + 3 ** 8


def test_decode_block_ends_with_rows_of_2_to_the_30(lib):
    """v = 16, n = 65536 with T = 1 << 30: rows 65534 (P = 2) and 65535 (P = 1) have 2^30 terms, the others one, which
    keeps A and Tout below 2^32, where the kernel's 32-bit records end: Tout = 3^16 - 3 + 3 * 2^30 = 3 264 272 190.  The
    division by 2^30 and the search over 65536 rows, at the first and last position of every row's block."""
    s = [1] * 16
    T = [1] * 65534 + [1 << 30] * 2
    assert ends_of_every_block(lib, s, T) == 3 ** 16 - 3 + 3 * (1 << 30) < 1 << 32
    # every row of 2^30 terms: the offsets exist (csgn_uint_pick_rows_offsets), the 32-bit records do not
    dec = Decoder(lib, s, [1 << 30] * 65536)
    assert dec(0)[0] == UNSUPPORTED and dec(3 ** 16 << 30)[0] == INVALID


def test_decode_invalid(lib):
    out = (C.c_uint64 * 3)()
    one = u64s([1] * 8)
    assert lib.csgn_uint_pick_rows_decode(3, one, 8, one, 26, out) == OK and tuple(out) == (7, 0, 0)
    assert lib.csgn_uint_pick_rows_decode(3, one, 8, one, 27, out) == INVALID
    assert lib.csgn_uint_pick_rows_decode(0, one, 1, one, 0, out) == INVALID
    assert lib.csgn_uint_pick_rows_decode(3, one, 9, one, 0, out) == INVALID
    assert lib.csgn_uint_pick_rows_decode(3, None, 8, one, 0, out) == INVALID
    assert lib.csgn_uint_pick_rows_decode(3, one, 8, None, 0, out) == INVALID
    assert lib.csgn_uint_pick_rows_decode(3, one, 8, one, 0, None) == INVALID
    assert lib.csgn_uint_pick_rows_decode(3, one, 8, u64s([1, 0, 1, 1, 1, 1, 1, 1]), 0, out) == INVALID


# -- the boundaries of the check ---------------------------------------------------------------------------------------
def limits(n_bits, s, T):
    """From the model's offsets, in Python integers: (the largest words of one element, the largest accepted batch).
    A batch is accepted while batch * A_j * dL < 2^60 and batch * Tout_j * dL < 2^60 for every plane."""
    dl = (n_bits + 63) // 64
    sizes = [rows_offsets(s, t) for t in T]
    per_element = max(max(src[-1], out[-1]) for src, out in sizes) * dl
    return max(out[-1] for _, out in sizes) * dl, ((1 << 60) - 1) // per_element


BATCH_CASES = [
    # DESIGN §4.30's fault: v = 3, n = 8, rows of one term, N = 1247 (dL = 20).  Tout = E = 27 terms = 540 words an
    # element; 2^50 * 540 = 2^59.08 < 2^60: ACCEPTED -- the call that expected a refusal was valid and was launched --,
    # 2^56 * 540 = 2^65.08: refused.  The largest accepted batch is (2^60 - 1) // 540 = 2 135 039 823 346 012.
    ("the fault of 4.30", 1247, [1] * 3, [[1] * 8], 1 << 50, 1 << 56),
    # the same index over the table csgn_uint_write leaves (T = 17, 9, 9, 5, 9, 5, 5, 3): Tout = 277 terms = 5540 words;
    # 2^47 * 5540 = 2^59.44 accepted, 2^48 * 5540 = 2^60.44 refused (so 2^50 is refused at THIS table)
    ("written v = 3", 1247, [1] * 3, [write_shaped([1] * 3, 8)], 1 << 47, 1 << 48),
    # v = 8, n = 256 written: Tout = 2 * 5^8 + 3^8 = 787 811 terms = 15 756 220 words (2^23.9);
    # 2^36 * that = 2^59.91 accepted, 2^37 * that = 2^60.91 refused
    ("written v = 8", 1247, [1] * 8, [write_shaped([1] * 8, 256)], 1 << 36, 1 << 37),
    # planes with different tables at N = 65 (dL = 2): the largest plane decides.  [1, 40, 1] under s = (2, 1):
    # P = 6, 4, 3, Tout = 6 + 160 + 3 = 169 terms = 338 words; 2^51 * 338 = 2^59.40 accepted, 2^52 * 338 refused
    ("per-plane tables", 65, [2, 1], [[1, 1, 1], [1, 40, 1], [3, 3, 3]], 1 << 51, 1 << 52),
]


@pytest.mark.parametrize("what,n_bits,s,T,accepted,refused", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batch_boundary(lib, what, n_bits, s, T, accepted, refused):
    n = len(T[0])
    element, largest = limits(n_bits, s, T)
    assert element < 1 << 31 and accepted <= largest < refused
    assert largest * element < 1 << 60 <= (largest + 1) * element
    for batch in (0, 1, accepted, largest):
        assert check(lib, n_bits, batch, s, n, T) == OK, batch
        assert kernel(lib, n_bits, batch, s, n, T) == "k_uint_pick_rows"
    for batch in (largest + 1, refused, (1 << 64) - 1):
        assert kernel(lib, n_bits, batch, s, n, T) == ""
        refused_by_both(lib, UNSUPPORTED, n_bits, batch, s, n, T)


def test_the_fault_of_4_30_was_a_valid_call(lib):
    """The arithmetic that settles it: 2^50 elements of 27 terms of 20 words are 2^50 * 540 = 607 985 949 695 016 960
    words, below 2^60 = 1 152 921 504 606 846 976, so the check accepts them and the launching call, as documented, went
    on to launch -- over buffers of 32 KB.  What that test meant to ask is refused from 2 135 039 823 346 013 on."""
    assert (1 << 50) * 27 * 20 == 607985949695016960 < 1 << 60
    assert limits(1247, [1] * 3, [[1] * 8]) == (540, 2135039823346012)
    assert check(lib, 1247, 1 << 50, [1] * 3, 8, [[1] * 8] * 8) == OK
    assert check(lib, 1247, 2135039823346012, [1] * 3, 8, [[1] * 8] * 8) == OK
    assert check(lib, 1247, 2135039823346013, [1] * 3, 8, [[1] * 8] * 8) == UNSUPPORTED
    assert check(lib, 1247, 1 << 56, [1] * 3, 8, [[1] * 8] * 8) == UNSUPPORTED


def test_element_boundary(lib):
    """Tout_j * dL below 2^31 words per element.  v = 1, n = 2, fresh: P = 2, 1, so T = (t, 1) gives Tout = 2 t + 1;
    at N = 1247 (dL = 20) the largest accepted t has (2 t + 1) * 20 < 2^31: t = 53 687 090 (Tout * 20 = 2 147 483 620),
    and t + 1 gives 2 147 483 660 >= 2^31 = 2 147 483 648.  At N = 64 (dL = 1): t = 2^30 - 1, Tout = 2^31 - 1."""
    for n_bits, dl in ((1247, 20), (64, 1)):
        t = (((1 << 31) - 1) // dl - 1) // 2
        assert (2 * t + 1) * dl < 1 << 31 <= (2 * (t + 1) + 1) * dl
        assert check(lib, n_bits, 1, [1], 2, [[t, 1]]) == OK
        assert check(lib, n_bits, 1, [1], 2, [[1, 1], [t, 1]]) == OK
        refused_by_both(lib, UNSUPPORTED, n_bits, 1, [1], 2, [[t + 1, 1]])
        refused_by_both(lib, UNSUPPORTED, n_bits, 1, [1], 2, [[1, 1], [t + 1, 1]])      # any plane
    assert (1 << 31) - 1 == 2 * ((1 << 30) - 1) + 1


def test_invalid_arguments(lib):
    s, T = [1] * 3, [[1] * 8] * 2
    assert check(lib, 1247, 3, s, 8, T) == OK
    refused_by_both(lib, INVALID, 0, 3, s, 8, T)                                # n_bits
    refused_by_both(lib, INVALID, 1247, 3, [1] * 17, 8, T)                      # index width outside 1..16
    refused_by_both(lib, INVALID, 1247, 3, s, 9, [[1] * 9])                     # rows outside 1..2^v
    refused_by_both(lib, INVALID, 1247, 3, s, 8, [[1] * 8] * 65)                # width outside 1..64
    refused_by_both(lib, INVALID, 1247, 3, [1, 0, 1], 8, T)                     # a plane of no terms
    refused_by_both(lib, INVALID, 1247, 3, s, 8, [[1] * 8, [1, 1, 0, 1, 1, 1, 1, 1]])   # a row of no terms
    refused_by_both(lib, INVALID, 1247, 3, s, 8, [[1] * 7 + [LIMIT]])           # what the offsets refuse: 2^62
    refused_by_both(lib, INVALID, 1247, 3, [LIMIT, 1, 1], 8, T)
    one = u64s([1] * 64)
    assert lib.csgn_uint_pick_rows_check(1247, 3, 0, one, 1, 1, one) == INVALID
    assert lib.csgn_uint_pick_rows_check(1247, 3, 3, one, 0, 1, one) == INVALID
    assert lib.csgn_uint_pick_rows_check(1247, 3, 3, one, 8, 0, one) == INVALID
    assert lib.csgn_uint_pick_rows_check(1247, 3, 3, None, 8, 1, one) == INVALID       # null pointers
    assert lib.csgn_uint_pick_rows_check(1247, 3, 3, one, 8, 1, None) == INVALID
    assert lib.csgn_uint_pick_rows_kernel(1247, 3, 3, None, 8, 1, one) == b""
    # n_bits past the library's term size: every entry point's own limit, UNSUPPORTED
    refused_by_both(lib, UNSUPPORTED, 16384 * 8 + 1, 3, s, 8, T)
    # the launching entry's own checks come after: null host arrays
    a = args(1247, 3, s, 8, T)
    p = (C.c_void_p * 64)(*([FAKE] * 64))
    assert lib.csgn_uint_pick_rows(a[0], a[1], a[2], None, a[3], a[4], a[5], p, a[6], p, None) == INVALID
    assert lib.csgn_uint_pick_rows(a[0], a[1], a[2], p, a[3], a[4], a[5], None, a[6], p, None) == INVALID
    assert lib.csgn_uint_pick_rows(a[0], a[1], a[2], p, a[3], a[4], a[5], p, a[6], None, None) == INVALID


# -- the form and its knob ---------------------------------------------------------------------------------------------
def test_check_and_name_agree(lib, knobs):
    """'' exactly where the check refuses, whatever the knob says; the knob forces the name elsewhere."""
    written = write_shaped([1] * 3, 8)
    cases = [(1247, 3, [1] * 3, 8, [written] * 2), (63, 1, [2, 1, 3], 5, [[1, 2, 3, 4, 5]]), (1247, 0, [1], 1, [[7]]),
             (0, 3, [1] * 3, 8, [written]), (1247, 3, [1] * 3, 9, [[1] * 9]), (1247, 1 << 56, [1] * 3, 8, [[1] * 8]),
             (1247, 1 << 50, [1] * 3, 8, [[1] * 8]), (1247, 1 << 50, [1] * 3, 8, [written]),
             (1247, 1, [1], 2, [[1 << 27, 1]]), (1247, 3, [1, 0], 2, [[1, 1]]), (64, 1, [1], 2, [[(1 << 30) - 1, 1]])]
    for form, fused in ((-1, "k_uint_pick_rows"), (0, "composed"), (1, "k_uint_pick_rows")):
        if form < 0:
            knobs.unset("uint_pick_rows_form")
        else:
            knobs.set("uint_pick_rows_form", form)
        seen = set()
        for c in cases:
            ok = check(lib, *c) == OK
            seen.add(ok)
            assert kernel(lib, *c) == (fused if ok else ""), (form, c[:4])
        assert seen == {True, False}


def test_the_knob(lib, knobs):
    import os

    from csgn_amd import capi
    names = capi.tuning_names()
    assert names.index("uint_write_fused") < names.index("uint_pick_rows_form") == names.index("uint_decrypt_form") - 1
    assert names[-2:] == ["uint_arith_form", "launch_blocks"]
    assert not "uint_pick_rows_form".endswith("_fused")
    knobs.unset("uint_pick_rows_form")
    assert capi.get_tuning("uint_pick_rows_form") == -1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    assert '{"uint_pick_rows_form", -1}' in source
