"""Encrypted integers summed into encrypted integers (csgn_wsum*) on a box without a GPU: the term count and its edges,
the argument checks and their order, the loud failure without a device, and the DEFINITION -- plane j the left-nested
sum, over the count vectors and their selections, of the left-nested products of the selected inputs -- pinned against
the oracle and the compiled reference, with decryptions under random keys.  The device side is
tests/test_wsum_gpu.py."""
import ctypes as C
from itertools import product
from math import comb, prod

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (INVALID, LIMIT, NO_DEVICE, OK, UNSUPPORTED, decrypt_value, encrypt_planes, lib, np_mul,  # noqa: F401
                         oracle_ops, rand_terms, ref_ops)
from tests.model_count import np_count
from tests.model_wsum import compose_wsum, count_vectors, np_wsum, product_classes, wsum_terms


def u64s(xs):
    return (C.c_uint64 * max(len(xs), 1))(*[int(x) for x in xs])


def c_terms(lib, ns, t, j):
    return lib.csgn_wsum_terms(len(ns), u64s(ns), t, j)


# the issue's table: term counts of fresh planes 0, 1, 2, ...
SUM_4x3 = ([4, 4, 4], [4, 10, 35, 161, 315])
SUM_8x4 = ([8, 8, 8, 8], [8, 36, 330, 6435, 245149])
MUL_4x4 = ([1, 2, 3, 4, 3, 2, 1], [1, 2, 4, 10, 34, 129, 383, 511])
MUL_8x8_LOW = ([1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 4, 10, 36, 202, 1828, 27338])


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_against_the_model(lib):
    for C_ in range(1, 5):
        for ns in product(range(5), repeat=C_):
            for t in (1, 2, 3):
                for j in range(7):
                    assert c_terms(lib, ns, t, j) == wsum_terms(ns, t, j), (ns, t, j)
    for ns, row in (SUM_4x3, SUM_8x4, MUL_4x4, MUL_8x8_LOW):
        assert [c_terms(lib, ns, 1, j) for j in range(len(row))] == row == [wsum_terms(ns, 1, j) for j in range(len(row))]


def test_terms_are_the_count_vectors(lib):
    """T_j by the definition's own sum over the count vectors, and with one class csgn_count's count."""
    for ns, t in [([2, 1, 1], 2), ([3, 3], 2), ([2, 0, 3], 3), (MUL_4x4[0], 1), ([4, 4, 4], 2)]:
        for j in range(8):
            T = sum(prod(comb(n, k) * t ** k for n, k in zip(list(ns) + [0] * 8, m)) for m in count_vectors(ns, j))
            assert c_terms(lib, ns, t, j) == T == wsum_terms(ns, t, j), (ns, t, j)
    for g in (1, 5, 8, 64, 65):
        for t in (1, 3):
            for j in range(7):
                assert c_terms(lib, [g], t, j) == lib.csgn_count_terms(g, t, j), (g, t, j)


def test_terms_saturate_and_refuse(lib):
    """A plane of 2^62 terms or more gives 0, as does an empty plane and every bad argument; nothing wraps."""
    assert comb(65, 32) < LIMIT <= comb(66, 32)
    assert c_terms(lib, [65], 1, 5) == comb(65, 32) == wsum_terms([65], 1, 5)
    assert c_terms(lib, [66], 1, 5) == 0 == wsum_terms([66], 1, 5)
    assert c_terms(lib, [65], 2, 5) == 0 == wsum_terms([65], 2, 5)
    assert c_terms(lib, [200, 200], 1, 6) == 0 == wsum_terms([200, 200], 1, 6)
    assert c_terms(lib, [2], (1 << 31) - 1, 1) == ((1 << 31) - 1) ** 2 and c_terms(lib, [2], 1 << 31, 1) == 0
    assert c_terms(lib, [0, 0, 1], LIMIT - 1, 2) == LIMIT - 1 and c_terms(lib, [0, 0, 1], LIMIT, 2) == 0
    # saturated on the way but not at the end: C(65536, m) passes 2^62 in the middle, plane 16 is the one subset of all
    assert c_terms(lib, [65536], 1, 16) == 1
    assert c_terms(lib, [65536], 1, 1) == comb(65536, 2)
    # empty planes: nothing weighs 2^j
    assert c_terms(lib, [3], 1, 2) == 0 == wsum_terms([3], 1, 2)
    assert c_terms(lib, [2, 0, 3], 1, 4) == 0 == wsum_terms([2, 0, 3], 1, 4)           # 2 + 12 < 16
    assert c_terms(lib, [0, 1], 1, 0) == 0 == wsum_terms([0, 1], 1, 0)
    assert c_terms(lib, [1], 1, 62) == 0 and c_terms(lib, [0] * 62 + [1], 1, 62) == 1
    # bad arguments
    assert lib.csgn_wsum_terms(1, None, 1, 0) == 0 and lib.csgn_wsum_terms(0, u64s([1]), 1, 0) == 0
    assert c_terms(lib, [1] * 65, 1, 0) == 0 == wsum_terms([1] * 65, 1, 0)
    assert c_terms(lib, [0, 0], 1, 0) == 0 and c_terms(lib, [65537], 1, 0) == 0 and c_terms(lib, [65536, 1], 1, 0) == 0
    assert c_terms(lib, [1 << 63, 1 << 63, 1], 1, 0) == 0                               # the sum of the n_c does not wrap
    assert c_terms(lib, [4], 0, 0) == 0 and c_terms(lib, [4], 1, 63) == 0


def test_argument_checks_in_order(lib):
    """csgn_wsum_create: the status is that of the first check that fails: the plan pointer, the classes, t, the planes
    (strictly ascending, within 0..62, none of them empty) (INVALID); a plane of 2^31 terms or more (UNSUPPORTED); and
    only then the device (NO_DEVICE on a box without one).  csgn_wsum: n_bits, then the plan, the count and the host
    pointers (INVALID); the sizes (UNSUPPORTED, computed without wrap-around); null device pointers (INVALID)."""
    import torch
    gpu = torch.cuda.is_available()

    def create(ns=(3, 3), t=1, js=(0, 1, 2, 3), plan=0, h_n=0, h_js=0, n_classes=None):
        handle = C.c_void_p()
        rc = lib.csgn_wsum_create(len(ns) if n_classes is None else n_classes, u64s(ns) if h_n == 0 else h_n, t, len(js),
                                  u64s(js) if h_js == 0 else h_js, C.byref(handle) if plan == 0 else plan)
        assert (handle.value is not None) == (rc == OK)
        return rc, handle

    assert create(plan=None, ns=())[0] == INVALID
    for bad in [dict(ns=()), dict(ns=(0, 0)), dict(ns=(1,) * 65), dict(ns=(65537,)), dict(ns=(65536, 1)), dict(h_n=None),
                dict(t=0), dict(t=LIMIT), dict(js=()), dict(js=tuple(range(64))), dict(h_js=None), dict(js=(1, 0)),
                dict(js=(1, 1)), dict(js=(63,)), dict(js=(0, 4)), dict(ns=(2, 0, 3), js=(0, 1, 2, 3, 4))]:
        assert create(**bad)[0] == INVALID, bad
    # ... over the sizes: C(64, 8) is past 2^31, C(200, 64) past 2^62
    assert create(ns=(64,), js=(3, 2))[0] == INVALID                      # unsorted
    assert create(ns=(64,), js=(3, 7))[0] == INVALID                      # plane 7 of 64 bits is empty
    assert b"no count vector" in lib.csgn_last_error()
    assert create(ns=(64,), js=(1, 3))[0] == UNSUPPORTED
    assert b"2^31" in lib.csgn_last_error()
    assert create(ns=(200,), js=(6,))[0] == UNSUPPORTED
    assert create(ns=(2,), t=1 << 16, js=(1,))[0] == UNSUPPORTED          # t^2 = 2^32
    assert lib.csgn_wsum_plan_terms(None, 0) == 0
    lib.csgn_wsum_destroy(None)
    buf = np.zeros(8, dtype=np.uint64)
    p = buf.ctypes.data
    two = (C.c_void_p * 2)(p, p)
    four = (C.c_void_p * 4)(p, p, p, p)
    assert lib.csgn_wsum(None, 0, 1, two, four, None) == INVALID          # n_bits
    assert b"n_bits" in lib.csgn_last_error()
    assert lib.csgn_wsum(None, 131073, 1, two, four, None) == UNSUPPORTED
    assert lib.csgn_wsum(None, 1247, 1, two, four, None) == INVALID       # the plan
    rc, plan = create()
    if not gpu:
        assert rc == NO_DEVICE
        assert b"no CPU" in lib.csgn_last_error()
        assert create(ns=(2, 0, 3), js=(0, 1, 3))[0] == NO_DEVICE and create(ns=MUL_8x8_LOW[0], js=range(8))[0] == NO_DEVICE
        return
    # with a device: a plan exists, and the calls that pass every check are not made (their pointers are not device memory)
    assert rc == OK
    try:
        assert [lib.csgn_wsum_plan_terms(plan, x) for x in range(5)] == [3, 6, 12, 3, 0]
        assert lib.csgn_wsum(plan, 0, 0, None, None, None) == INVALID
        assert lib.csgn_wsum(plan, 1247, 0, two, four, None) == INVALID
        assert lib.csgn_wsum(plan, 1247, 1, None, four, None) == INVALID and lib.csgn_wsum(plan, 1247, 1, two, None, None) == INVALID
        null_in, null_out = (C.c_void_p * 2)(p, None), (C.c_void_p * 4)(p, p, None, p)
        assert lib.csgn_wsum(plan, 1247, 1 << 56, null_in, four, None) == UNSUPPORTED      # 2^56 * 3 * 20 words
        assert b"size overflows" in lib.csgn_last_error()
        assert lib.csgn_wsum(plan, 64, 1 << 63, two, null_out, None) == UNSUPPORTED        # count * T wraps
        assert lib.csgn_wsum(plan, 1247, 1, null_in, four, None) == INVALID
        assert b"null device pointer" in lib.csgn_last_error()
        assert lib.csgn_wsum(plan, 1247, 1, two, null_out, None) == INVALID
    finally:
        lib.csgn_wsum_destroy(plan)


def test_knob(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert names.index("count_cpart") < names.index("wsum_cpart") < names.index("launch_blocks")
    knobs.unset("wsum_cpart")
    assert capi.get_tuning("wsum_cpart") == 0


# -- the definition against the oracle and the genuine reference -----------------------------------------------------
SHAPES = [([2, 1, 1], 1), ([2, 1, 1], 2), ([3, 3], 1), ([3, 3], 2), ([2, 0, 3], 2), (MUL_4x4[0], 1)]
SHAPE_IDS = ["n%s_t%d" % ("".join(map(str, ns)), t) for ns, t in SHAPES]


def all_planes(ns):
    return [j for j in range(10) if count_vectors(ns, j)]


def class_inputs(n, ns, t, count, seed):
    return [rand_terms(n, count * k, t, seed + c) if k else None for c, k in enumerate(ns)]


def check_definition(ops, n, ns, t):
    count = 2
    xs = class_inputs(n, ns, t, count, 1000 * n + 10 * sum(ns) + t)
    js = all_planes(ns)
    dl = (n + 63) // 64
    for j, w in zip(js, np_wsum(xs, ns, js)):
        assert w.shape == (count, wsum_terms(ns, t, j), dl), j
        for q in range(count):
            classes = [[xs[c][q * k + i].ravel() for i in range(k)] for c, k in enumerate(ns)]
            got = compose_wsum(ops, classes, j)
            assert got.size == w[q].size and np.array_equal(w[q].ravel(), got), (j, q)


@pytest.mark.parametrize("n", [63, 129])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_decode_is_the_composition_by_the_oracle(oracle, n, shape):
    check_definition(oracle_ops(oracle, n), n, *shape)


@pytest.mark.parametrize("n,d", [(63, 4), (129, 8)])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_decode_is_the_composition_by_the_reference(ref, n, d, shape):
    check_definition(ref_ops(ref, n, d), n, *shape)


def test_the_planes_skip_what_is_empty():
    assert all_planes([2, 0, 3]) == [0, 1, 2, 3] and all_planes([0, 0, 3]) == [2, 3] and all_planes([2, 1, 1]) == [0, 1, 2, 3]
    assert count_vectors([3, 3], 2) == [[2, 1, 0], [0, 2, 0]]           # m_1 = 1 before m_1 = 2: ascending, m_j first
    assert count_vectors([4, 4, 4], 2) == [[4, 0, 0], [2, 1, 0], [0, 2, 0], [0, 0, 1]]


@pytest.mark.parametrize("g,t,js", [(5, 2, [0, 1, 2]), (8, 1, [0, 1, 2, 3]), (6, 3, [1, 2])])
def test_one_class_is_the_count(g, t, js):
    x = rand_terms(129, 3 * g, t, 40 + g)
    for a, b in zip(np_wsum([x], [g], js), np_count(x, g, js)):
        assert np.array_equal(a, b)


# -- decryptions -------------------------------------------------------------------------------------------------------
def test_sums_decrypt_for_every_pattern(oracle):
    """n = [3, 3]: all 64 patterns of three bits of weight 1 and three of weight 2; the planes decrypt to the sum."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(801, 64 * d + 64))
    pats = np.arange(64, dtype=np.uint64)
    bits = ((pats[:, None] >> np.arange(6, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)    # [64, 6]
    dl = (n + 63) // 64
    xs = []
    for c in range(2):
        flat = np.ascontiguousarray(bits[:, 3 * c:3 * c + 3]).ravel()
        xs.append(oracle.encrypt_seq(n, key, flat, glibc_draws(810 + c, flat.size * (n + 2)))[0].reshape(flat.size, 1, dl))
    want = bits[:, :3].sum(axis=1).astype(np.uint64) + 2 * bits[:, 3:].sum(axis=1).astype(np.uint64)
    assert want.max() == 9
    assert np.array_equal(decrypt_value(oracle, n, key, np_wsum(xs, [3, 3], [0, 1, 2, 3])), want)


def test_products_decrypt_for_every_pair(oracle):
    """All 256 pairs of 4-bit integers: the eight planes of the partial products' sum decrypt to a * b."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(802, 64 * d + 64))
    a, b = np.divmod(np.arange(256, dtype=np.uint64), np.uint64(16))
    xs, ns = product_classes(encrypt_planes(oracle, n, key, a, 4, 82), encrypt_planes(oracle, n, key, b, 4, 83), np_mul)
    assert ns == MUL_4x4[0]
    outs = np_wsum(xs, ns, list(range(8)))
    assert [o.shape[1] for o in outs] == MUL_4x4[1]
    assert np.array_equal(decrypt_value(oracle, n, key, outs), a * b)
