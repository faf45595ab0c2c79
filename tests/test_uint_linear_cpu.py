"""A public matrix over F2 applied to an encrypted integer (csgn_uint_linear*), on a box without a GPU: the model
(tests/model_linear.py) against the oracle's and, where built, the reference's own operator+; csgn_uint_linear_terms and
csgn_uint_linear_decode against the model term for term; csgn_uint_linear_plan's figures replayed on the host for every
shape of tests/test_uint_linear_gpu.py; the argument checks and their order; the size guards; decryptions through the
oracle; F2Matrix's builders restated.  The device side is tests/test_uint_linear_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws, load_ref
from tests.model import (LIMIT, const_term, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms, ref_ops,  # noqa: F401
                         u64s)
from tests.model_linear import (DENSE, NS, ONE, ZERO, clear_linear, clmul, compose_linear, compose_rows, crc32_step8,
                                gpu_shapes, linear_decode, linear_terms, low, m_clmul, m_gf_mul, m_gray_decode,
                                m_gray_encode, m_identity, mix_columns, np_linear, random_rows, replay_grid, sigma0_256,
                                symbolic_linear)

TILE_UNITS = 262144                     # csgn_uint_linear.hip's kTileUnits, as csgn_uint_linear_plan reports it


def c_terms(lib, ta, row, cbit, w=None):
    return int(lib.csgn_uint_linear_terms(len(ta) if w is None else w, u64s(ta), row, cbit))


def c_decode(lib, ta, row, cbit, q):
    plane, term = C.c_uint64(77), C.c_uint64(77)
    if not lib.csgn_uint_linear_decode(len(ta), u64s(ta), row, cbit, q, C.byref(plane), C.byref(term)):
        assert plane.value == 77 and term.value == 77
        return None
    p = plane.value
    return (ONE if p == len(ta) else ZERO if p == len(ta) + 1 else p), term.value


def c_plan(lib, n, batch, ta, rows, constant):
    plan = (C.c_uint64 * 8)()
    rc = lib.csgn_uint_linear_plan(n, batch, len(ta), u64s(ta), len(rows), u64s(rows), constant, plan)
    assert rc == 0, lib.csgn_last_error()
    return [int(x) for x in plan]


# -- the definition against the genuine reference and the oracle -------------------------------------------------------
@pytest.mark.parametrize("n,d", [(65, 4), (1247, 16)])
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_definition_matches_reference_and_oracle(oracle, n, d, w):
    """Every row mask at in_width <= 4 with term counts (1, 2, 3, 1), with and without the constant, through the
    oracle's operator+ and, where the reference is built, through its own: the words of the numpy composition."""
    ref = load_ref()
    ta = [1, 2, 3, 1][:w]
    planes = [rand_terms(n, 1, t, 30 * w + i) for i, t in enumerate(ta)]
    flat = [p[0].ravel() for p in planes]
    rows = list(range(1 << w))
    dl = (n + 63) // 64
    routes = [oracle_ops(oracle, n)] + ([ref_ops(ref, n, d)] if ref is not None else [])
    for constant in (0, low(len(rows))):
        want = np_linear(n, planes, rows, constant)
        for add, _ in routes:
            got = compose_linear(flat, rows, constant, add, const_term(n, 1), const_term(n, 0))
            for j, row in enumerate(rows):
                assert np.array_equal(got[j], want[j].ravel()), (row, constant)
                assert got[j].size == linear_terms(ta, row, (constant >> j) & 1) * dl


# -- the C ABI, host side ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta", [[1], [1, 2, 3, 1], [1] * 5, [3, 70, 1, 5, 2], [2] * 7])
def test_terms_and_decode_give_the_table(lib, ta):
    w = len(ta)
    rows = list(range(1 << w)) if w <= 5 else random_rows(w, 40, 5) + [0, low(w)]
    for cbit in (0, 1):
        table = symbolic_linear(ta, rows, low(len(rows)) if cbit else 0) if len(rows) <= 64 else None
        for j, row in enumerate(rows):
            T = linear_terms(ta, row, cbit)
            assert c_terms(lib, ta, row, cbit) == T > 0, (row, cbit)
            want = table[j] if table else symbolic_linear(ta, [row], cbit)[0]
            assert len(want) == T
            for q in range(T):
                assert c_decode(lib, ta, row, cbit, q) == want[q] == linear_decode(ta, row, cbit, q), (row, cbit, q)
            assert c_decode(lib, ta, row, cbit, T) is None


def test_terms_by_hand_and_refusals(lib):
    assert c_terms(lib, [1] * 32, sigma0_256()[0], 0) == 3 and c_terms(lib, [1] * 32, sigma0_256()[31], 0) == 2
    assert c_terms(lib, [4, 5, 6], 0b101, 1) == 11 and c_terms(lib, [4, 5, 6], 0, 0) == 1 and c_terms(lib, [4, 5, 6], 0, 1) == 1
    assert c_decode(lib, [4, 5, 6], 0, 0, 0) == (ZERO, 0) and c_decode(lib, [4, 5, 6], 0, 1, 0) == (ONE, 0)
    assert c_decode(lib, [4, 5, 6], 0b101, 1, 4) == (2, 0) and c_decode(lib, [4, 5, 6], 0b101, 1, 10) == (ONE, 0)
    assert c_terms(lib, [1] * 64, (1 << 64) - 1, 1) == 65 and c_decode(lib, [1] * 64, (1 << 64) - 1, 1, 63) == (63, 0)
    # refused: the width, a null pointer, a zero count (named by the row or not), a row bit past the planes, the constant
    assert c_terms(lib, [1] * 65, 1, 0, w=65) == 0 and c_terms(lib, [1], 0, 0, w=0) == 0
    assert int(lib.csgn_uint_linear_terms(3, None, 1, 0)) == 0
    assert c_terms(lib, [1, 0, 1], 1, 0) == 0 and c_terms(lib, [1, 1, 1], 8, 0) == 0 and c_terms(lib, [1, 1], 1, 2) == 0
    # 2^62, without wrap-around
    big = LIMIT - 1
    assert c_terms(lib, [big], 1, 0) == big and c_terms(lib, [big], 1, 1) == 0 and c_terms(lib, [LIMIT], 1, 0) == 0
    assert c_terms(lib, [big, big, big, big, 8], 0b11111, 0) == 0 and c_terms(lib, [1 << 61] * 4, 0b1111, 0) == 0
    assert c_terms(lib, [1 << 61] * 4, 0b0011, 0) == 0 and c_terms(lib, [1 << 60] * 4, 0b0111, 0) == 3 << 60
    assert c_terms(lib, [1 << 60] * 4, 0b0111, 1) == (3 << 60) + 1 and c_terms(lib, [1 << 60] * 4, 0b1111, 0) == 0
    assert lib.csgn_uint_linear_decode(2, u64s([1, 1]), 3, 0, 0, None, None) == 0


# -- the plan, replayed ------------------------------------------------------------------------------------------------
def units_of(n, wide):
    dl = (n + 63) // 64
    return dl // 2 if wide and dl % 2 == 0 else dl


def check_plan(lib, knobs, n, ta, rows, constant, batch, cap=0):
    """The plan's figures against their definition, then every lane of every launch placed as the kernel places it:
    every unit of every output plane exactly once, every source in range."""
    knobs.set("launch_blocks", cap)
    plan = c_plan(lib, n, batch, ta, rows, constant)
    dl = (n + 63) // 64
    assert plan[0] == (16 if dl % 2 == 0 else 8) and plan[6] == TILE_UNITS and plan[7] == 1
    U = units_of(n, True)
    T = [linear_terms(ta, r, (constant >> j) & 1) for j, r in enumerate(rows)]
    assert plan[1] == sum(T) * U
    G = plan[2]
    assert G == min(max(1, TILE_UNITS // plan[1]), batch) and plan[3] == -(-batch // G)
    count, launches, per = replay_grid(ta, rows, constant, batch, U, G, cap if cap else (1 << 32) // 256)
    assert (plan[4], plan[5]) == (per, launches)
    for j, c in enumerate(count):
        assert c.size == batch * T[j] * U and (c == 1).all(), (n, ta, rows[j], batch, cap, j)
    if plan[0] == 16:                                                # the same shape with a pointer off alignment
        U8 = units_of(n, False)
        G8 = min(max(1, TILE_UNITS // (sum(T) * U8)), batch)
        for c in replay_grid(ta, rows, constant, batch, U8, G8, (1 << 32) // 256)[0]:
            assert (c == 1).all()
    return plan


@pytest.mark.parametrize("n", NS)
def test_plan_covers_every_unit_once(lib, knobs, n):
    for name, ta, rows, constant, batches in gpu_shapes():
        for batch in batches:
            check_plan(lib, knobs, n, ta, rows, constant, batch)


def test_plan_of_the_dense_shapes_and_the_splits(lib, knobs):
    name, ta, rows, constant, batches = DENSE
    for batch in batches:
        plan = check_plan(lib, knobs, 1247, ta, rows, constant, batch)
        assert plan[3] > 1 or batch == 2
    # two full tiles and a partial one at n = 64, then launches cut between tiles
    for name, ta, rows, constant, _ in gpu_shapes()[5:9]:
        G = c_plan(lib, 64, 1 << 30, ta, rows, constant)[2]
        assert G > 1
        plan = check_plan(lib, knobs, 64, ta, rows, constant, 2 * G + 5)
        assert plan[2:4] == [G, 3] and plan[5] == 1
        per = plan[4]
        for cap, launches in ((per, 3), (2 * per + 1, 2), (per - 1, 3), (3 * per, 1)):
            assert check_plan(lib, knobs, 64, ta, rows, constant, 2 * G + 5, cap)[5] == launches, (name, cap)
    assert c_plan(lib, 1247, 0, [1], [1], 0)[5] == 0


# -- the argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails: n_bits, the widths and the constant, host arrays, row bits and
    term counts (INVALID), 2^31 words per element and 2^60 per batch (UNSUPPORTED), null device pointers (INVALID), and
    only then the device (NO_DEVICE on a box without one; with one, the calls that pass every check are not made: their
    pointers are not device memory)."""
    import torch
    gpu = torch.cuda.is_available()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 64)(*([p] * 64))
    nullp = (C.c_void_p * 64)(*([p] * 3 + [None] + [p] * 60))
    one = u64s([1] * 64)
    rows8 = u64s([0xFF, 1, 0, 0x80, 3, 5, 9, 17])

    def call(n=1247, batch=4, w=8, a=ptrs, ta=one, m=8, rows=rows8, constant=0x21, out=ptrs):
        return lib.csgn_uint_linear(n, batch, w, a, ta, m, rows, constant, out, None)

    assert call(n=0, w=0, a=None) == -1 and call(n=131073, w=0) == -2               # n_bits
    assert call(w=0, a=None) == -1 and call(w=65, ta=None) == -1                   # the widths
    assert b"in_width" in lib.csgn_last_error()
    assert call(m=0, rows=None) == -1 and call(m=65, out=None) == -1
    assert call(constant=0x100, rows=None) == -1 and b"does not fit" in lib.csgn_last_error()
    for arg in ("a", "ta", "rows", "out"):                                         # host arrays, before rows and counts
        assert call(**{arg: None, "w": 7, "batch": 1 << 58}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    assert call(w=7, batch=1 << 58) == -1 and b"at or above in_width" in lib.csgn_last_error()   # row bits: 0xFF at 7 planes
    assert call(ta=u64s([1, 0] + [1] * 6), batch=1 << 58) == -1                    # a plane of no terms
    assert call(ta=u64s([1 << 62] * 8), a=nullp) == -1
    assert call(ta=u64s([1 << 61] * 8), a=nullp) == -1                             # row 0 sums to 2^64: no wrap-around
    assert b"overflows" in lib.csgn_last_error()
    # sizes: 2^31 words per element of an input or an output plane, 2^60 per batch
    t27 = u64s([1 << 27] * 8)                                                      # 2^27 * 20 words: past 2^31 alone
    assert call(ta=t27, a=nullp) == -2 and b"input plane" in lib.csgn_last_error()
    t24 = u64s([1 << 24] * 8)                                                      # fits alone; the 8-bit row does not
    assert call(ta=t24, a=nullp) == -2 and b"output 0" in lib.csgn_last_error()
    assert call(ta=t24, rows=u64s([1, 2, 0, 4, 3, 5, 9, 17]), a=nullp) == -1       # then it is the null pointer
    assert call(batch=1 << 56, a=nullp) == -2 and b"batch" in lib.csgn_last_error()
    assert call(batch=(1 << 60) // 20, out=nullp) == -2
    for arg in ("a", "out"):                                                       # a null device pointer in each array
        assert call(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert call(batch=0, out=nullp) == -1
    # the plan makes the same refusals up to the sizes, and needs no device
    plan = (C.c_uint64 * 8)()
    assert lib.csgn_uint_linear_plan(1247, 4, 8, one, 8, rows8, 0x21, plan) == 0 and plan[3] == 1
    assert lib.csgn_uint_linear_plan(1247, 4, 7, one, 8, rows8, 0x21, plan) == -1
    assert lib.csgn_uint_linear_plan(1247, 4, 8, t24, 8, rows8, 0x21, plan) == -2
    assert lib.csgn_uint_linear_plan(1247, 4, 8, one, 8, rows8, 0x21, None) == -1
    if gpu:
        return
    assert call() == -3 and b"no CPU fallback" in lib.csgn_last_error()
    assert call(batch=0) == -3 and call(w=64, m=64, rows=u64s([(1 << 64) - 1] * 64), constant=(1 << 64) - 1) == -3
    assert call(w=3, m=2, rows=u64s([7, 0]), constant=2, a=nullp, out=nullp) == -3   # only the entries it reads


# -- clear values and decryptions --------------------------------------------------------------------------------------
def test_builders_restated():
    rotr = lambda a, r: ((a >> r) | (a << (32 - r))) & 0xFFFFFFFF                  # noqa: E731
    for x in (0, 1, 0x80000000, 0x12345678, 0xFFFFFFFF, 0xDEADBEEF):
        assert clear_linear(sigma0_256(), 0, x) == rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3)
        crc = x
        for _ in range(8):
            crc = (crc >> 1) ^ (0xEDB88320 if crc & 1 else 0)
        assert clear_linear(crc32_step8(), 0, x) == crc
    for x in range(256):
        assert clear_linear(m_gf_mul(8, 2, 0x11B), 0, x) == ((x << 1) ^ (0x1B if x & 0x80 else 0)) & 0xFF
        assert clear_linear(m_gf_mul(8, 2, 0x1B), 0, x) == clear_linear(m_gf_mul(8, 2, 0x11B), 0, x)
        assert clear_linear(m_clmul(8, 0x1D), 0, x) == clmul(x, 0x1D) & 0xFF
        assert clear_linear(m_gray_encode(8), 0, x) == x ^ (x >> 1)
    for w in (1, 2, 7, 32, 64):
        assert compose_rows(m_gray_decode(w), m_gray_encode(w)) == m_identity(w)   # public duplicates cancel
    # MixColumns: the column (db 13 53 45) -> (8e 4d a1 bc) of the AES specification's example
    assert clear_linear(mix_columns(), 0, 0x455313DB) == 0xBCA14D8E
    assert sum(bin(r).count("1") for r in crc32_step8()) > 32 * 4                  # a dense matrix


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_decrypts(oracle, w):
    """Through the oracle's encrypt and decrypt at N = 127: the model's planes decrypt to matrix times bit vector XOR
    constant, for all 2^w inputs; every row mask for w <= 4, random matrices and the builders above."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(1210 + w, 64 * d + 64))
    xs = np.arange(1 << w, dtype=np.uint64)
    a = encrypt_planes(oracle, n, key, xs, w, 1220 + w)
    maps = [(list(range(1 << w))[:64], 0x5A5A5A5A5A5A5A5A & low(min(1 << w, 64)))] if w <= 4 else []
    maps += [(random_rows(w, m, 9 * w + m), int(np.random.default_rng(m).integers(0, 1 << m))) for m in (1, w, 9)]
    maps += [(m_gray_encode(w), 0), (m_gray_decode(w), low(w)), (m_clmul(w, low(w) & 0x2B), 1)]
    for rows, constant in maps:
        outs = np_linear(n, a, rows, constant)
        want = np.array([clear_linear(rows, constant, int(x)) for x in xs], dtype=np.uint64)
        assert np.array_equal(decrypt_value(oracle, n, key, outs), want), (rows, constant)
