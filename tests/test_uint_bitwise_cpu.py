"""a & b, a | b, a ^ b, ~a, select and keepWhere of encrypted integers in one launch (csgn_uint_bitwise*) on a box
without a GPU: the terms table, the six definitions (tests/model_bitwise.py) against the compiled reference and the
oracle, their decryptions, the argument checks and their order, the knob and the form names.  The device side is
tests/test_uint_bitwise_gpu.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import LIMIT, MUX, NOT as GATE_NOT, OR as GATE_OR, lib, oracle_ops, rand_terms, ref_ops, u64s  # noqa: F401
from tests.model_bitwise import (AND, KEEP, NOT, OPS, OR, READS_B, READS_SEL, SELECT, XOR, bitwise_clear, bitwise_terms,
                                 compose_bitwise, np_bitwise, np_bitwise_plane)


# -- the terms table --------------------------------------------------------------------------------------------------
def test_terms_table(lib):
    rng = np.random.default_rng(31)
    counts = [(1, 1, 1), (1, 2, 3), (3, 5, 2), (64, 64, 64), (7, 1, 9), (6560, 1, 1)]
    counts += [tuple(int(x) for x in rng.integers(1, 1000, 3)) for _ in range(40)]
    for ts, ta, tb in counts:
        want = {AND: ta * tb, OR: ta + tb + ta * tb, XOR: ta + tb, NOT: ta + 1, SELECT: ts * (ta + tb) + tb, KEEP: ts * ta}
        for op in OPS.values():
            assert lib.csgn_uint_bitwise_terms(op, ts, ta, tb) == bitwise_terms(op, ts, ta, tb) == want[op], (op, ts, ta, tb)
        # the gates the class operators issued
        assert lib.csgn_uint_bitwise_terms(OR, 0, ta, tb) == lib.csgn_gate_terms(GATE_OR, 0, ta, tb)
        assert lib.csgn_uint_bitwise_terms(NOT, 0, ta, 0) == lib.csgn_gate_terms(GATE_NOT, 0, ta, 0)
        assert lib.csgn_uint_bitwise_terms(SELECT, ts, ta, tb) == lib.csgn_gate_terms(MUX, ts, ta, tb)
    for bad in (0, 7, -1, 100):
        assert lib.csgn_uint_bitwise_terms(bad, 1, 1, 1) == 0 and bitwise_terms(bad, 1, 1, 1) == 0


def test_terms_zero_and_overflow(lib):
    terms = lambda op, ts, ta, tb: int(lib.csgn_uint_bitwise_terms(op, ts, ta, tb))   # noqa: E731
    big = LIMIT - 1
    for op in OPS.values():
        assert terms(op, 1, 0, 1) == 0                                # a is read by every op
        assert (terms(op, 1, 1, 0) == 0) == (op in READS_B)           # a zero count counts only where it is read
        assert (terms(op, 0, 1, 1) == 0) == (op in READS_SEL)
        assert terms(op, 1, LIMIT, 1) == 0
        assert (terms(op, 1, 1, LIMIT) == 0) == (op in READS_B)       # so does a count past the limit
        assert (terms(op, LIMIT, 1, 1) == 0) == (op in READS_SEL)
        for ts, ta, tb in itertools.product((0, 1, 2, 3, 1 << 31, 1 << 61, big, LIMIT, (1 << 64) - 1), repeat=3):
            assert terms(op, ts, ta, tb) == bitwise_terms(op, ts, ta, tb), (op, ts, ta, tb)
    # the last count that fits and the first that does not
    assert terms(AND, 0, 1 << 31, (1 << 31) - 1) == (1 << 62) - (1 << 31) and terms(AND, 0, 1 << 31, 1 << 31) == 0
    assert terms(XOR, 0, big - 1, 1) == big and terms(XOR, 0, big, 1) == 0
    assert terms(NOT, 0, big - 1, 0) == big and terms(NOT, 0, big, 0) == 0
    assert terms(OR, 0, 1 << 30, (1 << 31) - 1) != 0 and terms(OR, 0, (1 << 31) - 1, (1 << 31) + 1) == 0
    assert terms(SELECT, 1, big - 2, 1) == big and terms(SELECT, 1, big - 1, 1) == 0
    assert terms(SELECT, 2, (1 << 60) - 1, 1 << 60) == 0 and terms(KEEP, 2, 1 << 61, 0) == 0
    assert terms(KEEP, 2, (1 << 61) - 1, 0) == (1 << 62) - 2


# -- the definition against the reference and the oracle -------------------------------------------------------------
COUNTS = [(1, 1, 1), (2, 1, 3), (1, 3, 2), (3, 2, 2), (3, 3, 3)]


@pytest.mark.parametrize("n,d", [(64, 4), (127, 8), (1247, 16)])
@pytest.mark.parametrize("op", sorted(OPS.values()))
def test_definition_matches_reference_and_oracle(oracle, ref, n, d, op):
    dl = (n + 63) // 64
    for ts, ta, tb in COUNTS:
        a, b, s = rand_terms(n, 2, ta, 1), rand_terms(n, 2, tb, 2), rand_terms(n, 2, ts, 3)
        words = np_bitwise_plane(n, op, a, b, s)
        assert words.shape[1] == bitwise_terms(op, ts, ta, tb)
        for e in range(2):
            flat = (a[e].ravel(), b[e].ravel(), s[e].ravel())
            want = compose_bitwise(ref_ops(ref, n, d), n, op, *flat)
            got = compose_bitwise(oracle_ops(oracle, n), n, op, *flat)
            assert np.array_equal(got, want), (op, ts, ta, tb)
            assert got.size == bitwise_terms(op, ts, ta, tb) * dl
            assert np.array_equal(words[e].ravel(), got), (op, ts, ta, tb)


def test_integer_model_is_the_plane_model():
    n, batch = 127, 3
    a = [rand_terms(n, batch, t, 10 + t) for t in (1, 2, 3)]
    b = [rand_terms(n, batch, t, 20 + t) for t in (2, 1, 4)]
    s = rand_terms(n, batch, 2, 30)
    for op in OPS.values():
        outs = np_bitwise(n, op, a, b, s)
        assert len(outs) == 3
        for j in range(3):
            assert np.array_equal(outs[j], np_bitwise_plane(n, op, a[j], b[j], s))
            assert outs[j].shape[1] == bitwise_terms(op, 2, a[j].shape[1], b[j].shape[1])


@pytest.mark.parametrize("n,d", [(64, 4), (127, 8), (1247, 16)])
def test_every_input_combination_decrypts(oracle, n, d):
    """Under random keys every op's composition decrypts to the clear &, |, ^, ~, s ? a : b and s ? a : 0."""
    dl = (n + 63) // 64
    ops = oracle_ops(oracle, n)
    for k in range(4):
        key, _ = oracle.keygen(n, d, glibc_draws(300 + k, 64 * d + 64))
        bits = [0, 1] * 3
        cts, _ = oracle.encrypt_seq(n, key, bits, glibc_draws(400 + k, len(bits) * (n + 2)))
        ct = [cts[i * dl:(i + 1) * dl] for i in range(len(bits))]
        for op in OPS.values():
            for s, x, y in itertools.product((0, 1), repeat=3):
                w = compose_bitwise(ops, n, op, ct[x], ct[2 + y], ct[4 + s])
                assert oracle.decrypt_canonical(n, key, w) == bitwise_clear(op, x, y, s), (op, s, x, y)


# -- the argument checks ---------------------------------------------------------------------------------------------
def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits, the op, the width, the host arrays and the device
    pointers in them, the term counts (INVALID), 2^31 words per element and 2^60 per batch (UNSUPPORTED), and only then
    the device (NO_DEVICE on a box without one; with one, the calls that pass every check are not made: their pointers
    are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 65)(*([p] * 65))
    nullp = (C.c_void_p * 65)(*([p] * 3 + [None] + [p] * 61))
    one = u64s([1] * 65)
    zero_first = u64s([0] + [1] * 64)
    huge = u64s([1 << 62] * 65)
    t14 = u64s([1 << 14] * 65)

    def bitwise(n=1247, op=AND, batch=4, w=8, sel=p, ts=1, a=ptrs, ta=one, b=ptrs, tb=one, out=ptrs):
        return lib.csgn_uint_bitwise(n, op, batch, w, sel, ts, a, ta, b, tb, out, None)

    # each failing check wins over every later one
    assert bitwise(n=0, op=0, w=0, a=None) == -1                      # n_bits
    assert bitwise(n=131073, op=0) == -2
    assert bitwise(op=0, w=0) == -1 and bitwise(op=7, a=None) == -1   # the op
    assert b"operation" in lib.csgn_last_error()
    assert bitwise(w=0, a=None) == -1 and bitwise(w=65, ta=zero_first) == -1      # the width
    assert b"width" in lib.csgn_last_error()
    for op in OPS.values():
        read = ["a", "ta", "out"] + (["b", "tb"] if op in READS_B else [])
        for arg in ("a", "ta", "b", "tb", "out"):                     # host arrays, before the term counts
            got = bitwise(op=op, **{arg: None, **({} if arg == "ta" else {"ta": zero_first})})
            if arg in read:
                assert got == -1 and b"null host pointer" in lib.csgn_last_error(), (op, arg)
            else:
                assert got == -1 and b"no terms" in lib.csgn_last_error(), (op, arg)   # not looked at: the counts fail next
        for arg in ("a", "b", "out"):                                 # a null device pointer inside each host array
            got = bitwise(op=op, ta=zero_first, **{arg: nullp})
            assert got == -1, (op, arg)
            assert (b"null device pointer" in lib.csgn_last_error()) == (arg in read), (op, arg)
        got = bitwise(op=op, sel=None, ta=zero_first)                 # the selector, where it is read
        assert got == -1 and (b"selector" in lib.csgn_last_error()) == (op in READS_SEL), op
        assert bitwise(op=op, w=3, a=nullp, b=nullp, out=nullp, ta=zero_first) == -1   # past the width: not read
        assert b"no terms" in lib.csgn_last_error()
        # term counts: INVALID, before the sizes
        assert bitwise(op=op, ta=zero_first, batch=1 << 59) == -1
        assert bitwise(op=op, ta=huge, tb=huge, ts=1 << 61, batch=1 << 59) == -1   # 2^62 or more is INVALID, not UNSUPPORTED
        if op in READS_B:
            assert bitwise(op=op, tb=zero_first) == -1
        if op in READS_SEL:
            assert bitwise(op=op, ts=0) == -1 and bitwise(op=op, ts=1 << 62) == -1
    # sizes: 2^28 terms of 20 words pass 2^31 words an element; 2^14 + 2^14 do not
    assert bitwise(op=AND, ta=t14, tb=t14) == -2 and b"2^31" in lib.csgn_last_error()
    assert bitwise(op=OR, ta=t14, tb=t14) == -2 and bitwise(op=KEEP, ts=1 << 14, ta=t14) == -2
    assert bitwise(op=SELECT, ts=1 << 14, ta=t14, tb=t14) == -2
    assert bitwise(op=AND, w=64, ta=u64s([1] * 63 + [1 << 14]), tb=t14) == -2     # the last plane alone
    assert bitwise(batch=1 << 56) == -2 and b"batch" in lib.csgn_last_error()     # per batch
    assert bitwise(op=NOT, w=1, batch=1 << 59, n=64) == -2
    if gpu:
        return
    # no device: every call that passes the checks above, the empty batch included
    assert bitwise() == -3
    assert b"no CPU fallback" in lib.csgn_last_error()
    for op in OPS.values():
        assert bitwise(op=op) == -3 and bitwise(op=op, w=64) == -3 and bitwise(op=op, w=1, batch=0) == -3
    assert bitwise(op=XOR, ta=t14, tb=t14) == -3 and bitwise(op=NOT, ta=t14) == -3
    # operands the op does not read: neither their pointers nor their counts are looked at
    assert bitwise(op=NOT, sel=None, ts=0, b=None, tb=None) == -3 and bitwise(op=NOT, b=nullp, tb=zero_first) == -3
    assert bitwise(op=KEEP, b=None, tb=None) == -3 and bitwise(op=KEEP, b=nullp, tb=huge) == -3
    for op in (AND, OR, XOR):
        assert bitwise(op=op, sel=None, ts=0) == -3 and bitwise(op=op, sel=None, ts=1 << 63) == -3


def test_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        return                                                        # the device tests make the calls
    buf = np.zeros(64, dtype=np.uint64)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    one = u64s([1, 1])
    for op in OPS.values():
        assert lib.csgn_uint_bitwise(1247, op, 1, 2, buf.ctypes.data, 1, ptrs, one, ptrs, one, ptrs, None) == -3
        assert b"no CPU fallback" in lib.csgn_last_error()


# -- the knob and the form names ---------------------------------------------------------------------------------------
def test_the_knob(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert "uint_bitwise_form" in names and not "uint_bitwise_form".endswith("_fused")
    assert names[-2:] == ["uint_arith_form", "launch_blocks"]
    assert names.index("uint_bitwise_form") == names.index("uint_decrypt_chunk") + 1 == names.index("uint_arith_form") - 1
    knobs.unset("uint_bitwise_form")
    assert capi.get_tuning("uint_bitwise_form") == -1 and capi.get_tuning("CSGN_UINT_BITWISE_FORM") == -1
    capi.reset_tuning()
    assert capi.get_tuning("uint_bitwise_form") == -1                 # the default
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.h")).read()
    assert "TUNE_UINT_BITWISE_FORM," in header
    assert header.index("TUNE_UINT_DECRYPT_CHUNK,") < header.index("TUNE_UINT_BITWISE_FORM,") < header.index("TUNE_UINT_ARITH_FORM,")


def test_form_names(lib, knobs):
    def name(n, op, w, ta, tb, ts=1, batch=256):
        return lib.csgn_uint_bitwise_kernel(n, op, batch, w, ts, u64s(ta), u64s(tb)).decode()

    one = [1] * 65
    shapes = [(1247, 1, one, one, 1), (1247, 8, one, one, 1), (1300, 64, one, one, 2), (64, 3, [1, 2, 3], [2, 1, 4], 3),
              (1247, 4, [2, 3, 5, 9], [2, 3, 4, 6], 6560)]
    knobs.unset("gate_fused")
    for form, want in ((1, "k_uint_bitwise"), (0, "planes")):
        knobs.set("uint_bitwise_form", form)
        for op in OPS.values():
            for n, w, ta, tb, ts in shapes:
                assert name(n, op, w, ta, tb, ts) == want, (form, op, n, w)
                assert name(n, op, w, ta, tb, ts, batch=1 << 20) == want
        for gates in (0, 1):                                          # the bitwise knob, forced, wins over a forced gate form
            knobs.set("gate_fused", gates)
            assert name(1247, OR, 8, one, one) == want
        knobs.unset("gate_fused")
    # one element of all planes past one launch's lanes: the planes, whatever the knob says
    knobs.set("uint_bitwise_form", 1)
    t = [1 << 25] * 64                                                # N = 64: one word a term
    assert name(64, XOR, 64, t, t) == "planes" and name(64, XOR, 2, t, t) == "k_uint_bitwise"
    assert name(64, NOT, 64, [1 << 26] * 64, t) == "planes" and name(64, NOT, 64, t, t) == "k_uint_bitwise"
    # left at -1: by shape, and a forced gate form gives the planes
    knobs.unset("uint_bitwise_form")
    assert knobs.capi.get_tuning("uint_bitwise_form") == -1
    for op in OPS.values():
        for n, w, ta, tb, ts in shapes:
            assert name(n, op, w, ta, tb, ts) in ("k_uint_bitwise", "planes")
            for gates in (0, 1):
                knobs.set("gate_fused", gates)
                assert name(n, op, w, ta, tb, ts) == "planes", (op, n, w, gates)
                assert name(n, op, w, ta, tb, ts, batch=1) == "planes"
            knobs.unset("gate_fused")


def test_invalid_shapes_have_no_form(lib, knobs):
    one = u64s([1] * 65)
    zero_mid = u64s([1, 1, 0, 1])
    for form in (-1, 0, 1):
        knobs.set("uint_bitwise_form", form)
        for op in OPS.values():
            kernel = lambda n=1247, op=op, batch=256, w=4, ts=1, ta=one, tb=one: lib.csgn_uint_bitwise_kernel(  # noqa: E731
                n, op, batch, w, ts, ta, tb)
            assert kernel() in (b"k_uint_bitwise", b"planes")
            assert kernel(n=0) == b""                                 # n_bits 0
            assert kernel(w=0) == b"" and kernel(w=65) == b""         # the width
            assert kernel(ta=None) == b"" and kernel(ta=zero_mid) == b""
            assert (kernel(tb=None) == b"") == (op in READS_B) and (kernel(tb=zero_mid) == b"") == (op in READS_B)
            assert (kernel(ts=0) == b"") == (op in READS_SEL) and (kernel(ts=1 << 62) == b"") == (op in READS_SEL)
            assert kernel(ta=u64s([1 << 62] * 4)) == b""
            assert kernel(w=3, ta=zero_mid) == b"" and kernel(w=2, ta=zero_mid) != b""   # only the planes of the width
        assert lib.csgn_uint_bitwise_kernel(1247, 0, 256, 4, 1, one, one) == b""
        assert lib.csgn_uint_bitwise_kernel(1247, 7, 256, 4, 1, one, one) == b""
        # an overflowing plane is a bad shape
        assert lib.csgn_uint_bitwise_kernel(1247, AND, 1, 1, 1, u64s([1 << 31]), u64s([1 << 31])) == b""
        assert lib.csgn_uint_bitwise_kernel(1247, XOR, 1, 1, 1, u64s([1 << 31]), u64s([1 << 31])) != b""
