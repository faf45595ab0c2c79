"""Products of encrypted bit matrices over F2 (csgn_matmul*) on a box without a GPU: the term count, the dispatch names
and knob, the argument checks and their order, the loud failure without a device, and the DEFINITION -- C[i,k] the
left-nested sum over e of A[i,e] * B[e,k], a composition of the reference's operator* / operator+ -- pinned against the
compiled reference and the oracle, with decryptions under random keys.  The device side is tests/test_matmul_gpu.py."""
import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (INVALID, LIMIT, NO_DEVICE, UNSUPPORTED, decrypt_bits, lib, np_add, oracle_ops,  # noqa: F401
                         rand_terms, ref_ops)
from tests.model_matmul import compose_matmul, matmul_terms, np_matmul, sum_groups_offsets


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_formula(lib):
    rng = np.random.default_rng(11)
    for _ in range(50):
        inner, ta, tb = (int(x) for x in rng.integers(1, 1000, 3))
        assert lib.csgn_matmul_terms(inner, ta, tb) == inner * ta * tb == matmul_terms(inner, ta, tb)
    assert lib.csgn_matmul_terms(1, 1, 1) == 1
    assert lib.csgn_matmul_terms(1 << 20, 1, 1) == 1 << 20


def test_terms_invalid(lib):
    for args in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)]:
        assert lib.csgn_matmul_terms(*args) == 0 == matmul_terms(*args), args
    # the 2^62 edge, on both sides, in every argument
    for args in [(LIMIT - 1, 1, 1), (1, LIMIT - 1, 1), (1, 1, LIMIT - 1), (1 << 31, 1 << 30, 1), ((1 << 31) - 1, 1 << 30, 2)]:
        want = args[0] * args[1] * args[2]
        assert want < LIMIT and lib.csgn_matmul_terms(*args) == want == matmul_terms(*args), args
    for args in [(LIMIT, 1, 1), (1, LIMIT, 1), (1, 1, LIMIT), (1 << 31, 1 << 31, 1), (1 << 31, 1 << 30, 2),
                 (1 << 21, 1 << 21, 1 << 21), (1 << 32, 1 << 32, 1), (1 << 63, 2, 1), ((1 << 64) - 1, (1 << 64) - 1, 3)]:
        assert lib.csgn_matmul_terms(*args) == 0 == matmul_terms(*args), args


def test_dispatch_names(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert "matmul_form" in names and "matmul_epart" in names
    knobs.unset("matmul_form")
    assert capi.get_tuning("matmul_form") == -1 and capi.get_tuning("matmul_epart") == 0

    def name(n=1247, rows=4, inner=5, cols=6, ta=1, tb=1, tr=0):
        return lib.csgn_matmul_kernel(n, rows, inner, cols, ta, tb, tr).decode()

    bench = [dict(rows=256, inner=256, cols=256), dict(rows=4096, inner=4096, cols=1),
             dict(rows=1024, inner=64, cols=1024, tr=1), dict(rows=64, inner=64, cols=64, ta=2, tb=2),
             dict(rows=1, inner=1 << 20, cols=1)]
    for value, want in [(-1, "k_matmul"), (0, "composed"), (1, "k_matmul")]:      # per shape: fused
        knobs.set("matmul_form", value)
        assert capi.get_tuning("matmul_form") == value
        for shape in bench:
            assert name(**shape) == want, (value, shape)
        assert name() == want and name(tr=1) == want and name(ta=3, tb=2) == want
        # every invalid argument, whatever the knob says
        for bad in [dict(n=0), dict(rows=0), dict(inner=0), dict(cols=0), dict(ta=0), dict(tb=0), dict(ta=LIMIT),
                    dict(tb=LIMIT), dict(inner=1 << 31, ta=1 << 31), dict(inner=1 << 21, ta=1 << 21, tb=1 << 21)]:
            assert name(**bad) == "", (value, bad)
    # an operand past the gather launcher's 2^32 elements is fused whatever the knob says
    knobs.set("matmul_form", 0)
    assert name(rows=1 << 16, inner=1 << 16, cols=1) == "k_matmul"
    assert name(rows=1, inner=1 << 16, cols=1 << 16) == "k_matmul"
    assert name(rows=1 << 15, inner=1 << 16, cols=1 << 15) == "composed"


def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits; the dimensions; the term counts (INVALID); 2^31 words
    per element and 2^60 per call (UNSUPPORTED, computed without wrap-around); null device pointers (INVALID); and only
    then the device (NO_DEVICE on a box without one; with one, the calls that pass every check are not made: their
    pointers are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data

    def mm(n=1247, rows=2, inner=3, cols=2, a=p, ta=1, b=p, tb=1, tr=0, out=p):
        return lib.csgn_matmul(n, rows, inner, cols, a, ta, b, tb, tr, out, None)

    # each failing check wins over every later one
    assert mm(n=0, rows=0, ta=0, a=None) == INVALID                   # n_bits
    assert b"n_bits" in lib.csgn_last_error()
    assert mm(n=131073, rows=0) == UNSUPPORTED
    for dim in ("rows", "inner", "cols"):                             # dimensions, before the term counts
        assert mm(**{dim: 0, "ta": 0, "a": None}) == INVALID, dim
        assert b"dimension" in lib.csgn_last_error(), dim
    for t in ("ta", "tb"):                                            # term counts, before the sizes and the pointers
        assert mm(**{t: 0, "inner": 1 << 40, "a": None}) == INVALID, t
        assert b"terms" in lib.csgn_last_error(), t
        assert mm(**{t: LIMIT, "out": None}) == INVALID, t
        assert mm(**{t: (1 << 64) - 1}) == INVALID, t
        assert mm(**{t: LIMIT - 1, "out": None}) == UNSUPPORTED, t    # a valid count, but past the sizes
    # sizes, before the pointers: 2^31 words per element ...
    dl = 20
    edge = (1 << 31) // dl                                            # inner * dL >= 2^31 from here on
    assert mm(inner=edge + 1, a=None) == UNSUPPORTED
    assert b"per element" in lib.csgn_last_error()
    assert mm(inner=1 << 31, n=64, out=None) == UNSUPPORTED
    assert mm(inner=1 << 16, ta=1 << 8, tb=1 << 7, n=64, b=None) == UNSUPPORTED
    # ... without wrap-around: 2^63 terms at dL = 1, and products that wrap to small numbers
    assert mm(inner=1 << 21, ta=1 << 21, tb=1 << 21, n=64, a=None) == UNSUPPORTED
    assert mm(inner=1 << 32, ta=1 << 32, tb=1, n=64, a=None) == UNSUPPORTED
    assert mm(inner=1 << 62, ta=4, tb=1, n=64, a=None) == UNSUPPORTED
    assert mm(inner=1 << 60, ta=1, tb=1, n=1024, a=None) == UNSUPPORTED          # T * dL wraps to 0
    # ... and 2^60 words per call
    assert mm(rows=1 << 59, inner=1, cols=1, n=128, a=None) == UNSUPPORTED
    assert b"size overflows" in lib.csgn_last_error()
    assert mm(rows=1 << 59, inner=32, cols=1, n=64, a=None) == UNSUPPORTED       # rows * T wraps to 0
    assert mm(rows=1 << 32, inner=1, cols=1 << 32, n=64, a=None) == UNSUPPORTED  # rows * cols wraps to 0
    assert mm(rows=1 << 30, inner=1, cols=1 << 30, n=64, a=None) == UNSUPPORTED  # 2^60 exactly
    for arg in ("a", "b", "out"):                                     # null device pointers, before the device
        assert mm(**{arg: None}) == INVALID, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert mm(rows=1 << 59, inner=1, cols=1, n=64, a=None) == INVALID            # 2^59 words pass the size check
    assert mm(inner=edge, a=None) == INVALID                                     # as does the last size below 2^31
    if gpu:
        return
    # no device: every call that passes the checks above
    assert mm() == NO_DEVICE
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert mm(tr=1, ta=2, tb=3) == NO_DEVICE
    assert mm(inner=edge) == NO_DEVICE and mm(rows=1 << 59, inner=1, cols=1, n=64) == NO_DEVICE


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
SHAPES = [(1, 1, 1), (1, 5, 1), (2, 3, 2), (3, 2, 4)]
TERMS = [(1, 1), (2, 1), (1, 3), (2, 3)]


@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("terms", TERMS, ids=lambda t: "t%d_%d" % t)
@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
def test_definition_matches_reference(oracle, ref, n, d, shape, terms, transposed):
    rows, inner, cols = shape
    ta, tb = terms
    seed = 1000 * n + 100 * rows + 10 * inner + cols + 7 * ta + 3 * tb
    a = rand_terms(n, rows * inner, ta, seed)
    b = rand_terms(n, inner * cols, tb, seed + 1)
    flat_a = [x.ravel() for x in a]
    flat_b = [x.ravel() for x in b]
    want = compose_matmul(ref_ops(ref, n, d), flat_a, flat_b, rows, inner, cols, transposed)
    got = compose_matmul(oracle_ops(oracle, n), flat_a, flat_b, rows, inner, cols, transposed)
    words = np_matmul(a, b, rows, inner, cols, transposed)
    dl = (n + 63) // 64
    assert words.shape == (rows * cols, inner * ta * tb, dl)
    for x in range(rows * cols):
        assert np.array_equal(got[x], want[x]), x
        assert got[x].size == inner * ta * tb * dl
        assert np.array_equal(words[x].ravel(), got[x]), x


def test_layouts_agree():
    """The transposed layout of the same matrix gives the same words."""
    n, rows, inner, cols = 129, 3, 4, 5
    a, b = rand_terms(n, rows * inner, 2, 1), rand_terms(n, inner * cols, 3, 2)
    bt = b.reshape(inner, cols, 3, -1).transpose(1, 0, 2, 3).reshape(cols * inner, 3, -1)
    assert np.array_equal(np_matmul(a, b, rows, inner, cols), np_matmul(a, np.ascontiguousarray(bt), rows, inner, cols, True))


# -- decryptions -------------------------------------------------------------------------------------------------------
def encrypt_matrix(oracle, n, key, bits, seed):
    flat = np.asarray(bits, dtype=np.uint8).ravel()
    dl = (n + 63) // 64
    return oracle.encrypt_seq(n, key, flat, glibc_draws(seed, flat.size * (n + 2)))[0].reshape(flat.size, 1, dl)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 9, 1), (2, 2, 2), (3, 4, 1), (4, 9, 5)], ids=lambda s: "x".join(map(str, s)))
def test_product_decrypts(oracle, shape):
    rows, inner, cols = shape
    n, d = 127, 8
    rng = np.random.default_rng(rows * 100 + inner * 10 + cols)
    key, _ = oracle.keygen(n, d, glibc_draws(900 + inner, 64 * d + 64))
    A = rng.integers(0, 2, (rows, inner)).astype(np.uint8)
    B = rng.integers(0, 2, (inner, cols)).astype(np.uint8)
    if inner >= 2:                                                    # an output with an even number of products equal to 1
        A[0, :2] = 1
        B[:2, 0] = 1
        A[0, 2:] = 0
    want = (A.astype(np.int64) @ B.astype(np.int64)) % 2
    if inner >= 2:
        assert int((A[0] & B[:, 0]).sum()) == 2 and want[0, 0] == 0
    ea = encrypt_matrix(oracle, n, key, A, 910 + inner)
    eb = encrypt_matrix(oracle, n, key, B, 920 + inner)
    ebt = encrypt_matrix(oracle, n, key, B.T, 930 + inner)
    for c in (np_matmul(ea, eb, rows, inner, cols), np_matmul(ea, ebt, rows, inner, cols, True)):
        assert np.array_equal(decrypt_bits(oracle, n, key, c).reshape(rows, cols).astype(np.int64), want)
    # multi-term operands: x + ZERO decrypts as x
    zero_a = encrypt_matrix(oracle, n, key, np.zeros_like(A), 940)
    zero_b = encrypt_matrix(oracle, n, key, np.zeros_like(B), 941)
    c = np_matmul(np_add(ea, zero_a), np_add(np_add(eb, zero_b), zero_b), rows, inner, cols)
    assert c.shape[1] == inner * 6
    assert np.array_equal(decrypt_bits(oracle, n, key, c).reshape(rows, cols).astype(np.int64), want)


# -- sumGroups ---------------------------------------------------------------------------------------------------------
def test_sum_groups_offsets_arithmetic():
    """CiphertextBatch::sumGroups on a ragged batch keeps every g-th offset: element q then holds exactly the terms of
    elements q*g .. q*g + g - 1, in order, which is their left-nested sum; on a uniform batch that is count/g elements
    of g * terms terms."""
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 5, 24).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    words = np.arange(int(off[-1]), dtype=np.uint64)                  # one word a term
    for g in (1, 2, 3, 4, 6, 8, 12, 24):
        o = sum_groups_offsets(off, g)
        assert len(o) == 24 // g + 1 and o[0] == 0 and o[-1] == off[-1]
        for q in range(24 // g):
            want = np.concatenate([words[int(off[i]):int(off[i + 1])] for i in range(q * g, q * g + g)])
            assert np.array_equal(words[int(o[q]):int(o[q + 1])], want), (g, q)
            assert int(o[q + 1] - o[q]) == int(counts[q * g:q * g + g].sum())
    uniform = np.arange(25, dtype=np.uint64) * np.uint64(3)           # 24 elements of 3 terms
    for g in (1, 2, 4, 24):
        assert np.array_equal(sum_groups_offsets(uniform, g), np.arange(24 // g + 1, dtype=np.uint64) * np.uint64(3 * g))
    for g in (0, 5, 25):
        with pytest.raises(AssertionError):
            sum_groups_offsets(off, g)
