"""Shifts, rotates and per-element reads by encrypted amounts (csgn_uint_pick*) on a box without a GPU: the term counts
E_j, the argument checks, the dispatch names and knob, the loud failure without a device, the per-output decode the
kernel performs (restated in tests/model_pick.py), and the DEFINITION -- output j is the left-nested sum over
r < rows_j of csgn_uint_plain's EQ(index, r) times the source the row names -- pinned against the compiled reference
and the oracle, with decryptions under random keys of EVERY distance against plain integer arithmetic.  The device side
is tests/test_uint_pick_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (LIMIT, const_term, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms, ref_ops,  # noqa: F401
                         u64s)
from tests.model_pick import (EACH, OPS, ROTL, ROTR, SHIFTS, SHL, SHR, c_pick_terms, clear_pick, compose_pick, np_pick,
                              np_pick_decoded, np_pick_fast, pick_terms, rows_of)

WIDTHS = (1, 2, 3, 5, 8)                # w < 2^v, w = 2^v, w > 2^v, and no power of two for the rotates


def each_rows(v):
    return sorted({1, (1 << v) - 1, 1 << v} - {0})


def shapes(op, v):
    """(w, n) of every case of the issue at index width v."""
    if op == EACH:
        return [(w, n) for w in WIDTHS for n in each_rows(v)]
    return [(w, 0) for w in WIDTHS]


def index_terms(v, mixed):
    return [1 + (k + 1) % 3 for k in range(v)] if mixed else [1] * v


def operands(n_bits, op, s, w, n, t, batch, seed):
    index = [rand_terms(n_bits, batch, sk, seed + k) for k, sk in enumerate(s)]
    a = [rand_terms(n_bits, batch * (n if op == EACH else 1), t, seed + 40 + j) for j in range(w)]
    return index, a


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_terms_agree_with_the_model(lib):
    for op in OPS.values():
        for v in (1, 2, 3):
            for mixed in (False, True):
                s = index_terms(v, mixed)
                for w, n in shapes(op, v):
                    for j in range(w):
                        assert c_pick_terms(lib, op, v, s, w, n, j) == pick_terms(op, s, w, n, j), (op, v, s, w, n, j)
    # the figures of include/csgn_hip.h
    assert c_pick_terms(lib, SHL, 3, [1] * 3, 8, 0, 7) == 27
    assert c_pick_terms(lib, SHL, 3, [1] * 3, 8, 0, 0) == 8
    assert c_pick_terms(lib, SHR, 3, [1] * 3, 8, 0, 7) == 8
    assert all(c_pick_terms(lib, ROTL, 5, [1] * 5, 32, 0, j) == 243 for j in range(32))


def test_terms_invalid(lib):
    one = [1] * 17
    assert c_pick_terms(lib, SHL, 3, one, 8, 0, 7) == 27
    assert c_pick_terms(lib, 0, 3, one, 8, 0, 7) == 0                   # unknown op
    assert c_pick_terms(lib, 6, 3, one, 8, 0, 7) == 0
    assert c_pick_terms(lib, -1, 3, one, 8, 0, 7) == 0
    assert c_pick_terms(lib, SHL, 0, one, 8, 0, 7) == 0                 # index width outside 1..16
    assert c_pick_terms(lib, SHL, 17, one, 8, 0, 7) == 0
    assert c_pick_terms(lib, SHL, 3, one, 0, 0, 0) == 0                 # width outside 1..64
    assert c_pick_terms(lib, SHL, 3, one, 65, 0, 0) == 0
    assert c_pick_terms(lib, SHL, 3, one, 8, 0, 8) == 0                 # j past the width
    for op in SHIFTS:
        assert c_pick_terms(lib, op, 3, one, 8, 1, 0) == 0              # rows given to a shift or rotate
    assert c_pick_terms(lib, EACH, 3, one, 8, 0, 0) == 0                # rows outside 1..2^v
    assert c_pick_terms(lib, EACH, 3, one, 8, 9, 0) == 0
    assert c_pick_terms(lib, EACH, 3, one, 8, 8, 0) == 27
    assert c_pick_terms(lib, SHL, 3, None, 8, 0, 7) == 0                # null pointer
    assert c_pick_terms(lib, SHL, 3, [1, 0, 1], 8, 0, 7) == 0           # a plane of no terms
    assert c_pick_terms(lib, ROTL, 4, [1 << 16] * 4, 8, 0, 0) == 0      # 2^62 or more
    assert c_pick_terms(lib, ROTL, 1, [LIMIT], 1, 0, 0) == 0


def test_dispatch_names(lib, knobs):
    from csgn_amd import capi
    names = capi.tuning_names()
    assert "uint_pick_fused" in names and names.index("uint_pick_fused") < names.index("launch_blocks")
    assert "uint_pick_stage" in names and capi.get_tuning("uint_pick_stage") in (-1, 0, 1)
    knobs.unset("uint_pick_fused")
    assert capi.get_tuning("uint_pick_fused") == -1

    def name(n, op, v, s, w, rows, t, batch=256):
        return lib.csgn_uint_pick_kernel(n, op, batch, v, u64s(s), w, rows, t).decode()

    for op, rows in ((SHL, 0), (SHR, 0), (ROTL, 0), (ROTR, 0), (EACH, 5)):
        assert name(1247, op, 3, [1] * 3, 8, rows, 1) == "k_uint_pick"         # per shape: fused for every shape
        assert name(1247, op, 3, [2, 1, 3], 64, rows, 2, batch=1) == "k_uint_pick"
    assert name(0, SHL, 3, [1] * 3, 8, 0, 1) == ""                      # n_bits 0
    assert name(1247, 0, 3, [1] * 3, 8, 0, 1) == ""                     # unknown op
    assert name(1247, 6, 3, [1] * 3, 8, 0, 1) == ""
    assert name(1247, SHL, 17, [1] * 17, 8, 0, 1) == ""                 # bad index width
    assert name(1247, SHL, 3, [1] * 3, 0, 0, 1) == ""                   # bad width
    assert name(1247, SHL, 3, [1] * 3, 65, 0, 1) == ""
    assert name(1247, ROTL, 3, [1] * 3, 8, 8, 1) == ""                  # rows given to a rotate
    assert name(1247, EACH, 3, [1] * 3, 8, 0, 1) == ""                  # rows outside 1..2^v
    assert name(1247, EACH, 3, [1] * 3, 8, 9, 1) == ""
    assert name(1247, SHL, 3, [1, 0, 1], 8, 0, 1) == ""                 # a plane of no terms
    assert name(1247, SHL, 3, [1] * 3, 8, 0, 0) == ""
    knobs.set("uint_pick_fused", 0)
    assert capi.get_tuning("uint_pick_fused") == 0
    assert name(1247, SHL, 3, [1] * 3, 8, 0, 1) == "composed"
    assert name(1247, EACH, 3, [1] * 3, 8, 8, 1) == "composed"
    assert name(1247, EACH, 3, [1] * 3, 8, 8, 1, batch=1 << 29) == "k_uint_pick"   # past the gather's counts
    assert name(1247, EACH, 3, [1] * 3, 8, 8, 1, batch=(1 << 29) - 1) == "composed"
    assert name(1247, EACH, 3, [1] * 3, 8, 8, 1, batch=1 << 61) == "k_uint_pick"   # batch * n wraps to 0 in 64 bits
    knobs.set("uint_pick_fused", 1)
    assert name(1247, ROTR, 3, [1] * 3, 8, 0, 1) == "k_uint_pick"


def test_the_knob_is_spelt_as_the_library_stores_it():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = open(os.path.join(root, "csgn_amd", "csrc", "csgn_tuning.cpp")).read()
    assert '{"uint_pick_fused", -1}' in source


def test_plan_figures(lib):
    """csgn_uint_pick_plan: the tile of the fused form; the parts of QP entries cover the longest output's stream."""
    plan = (C.c_uint64 * 4)()
    assert lib.csgn_uint_pick_plan(4096, SHL, 2, 3, u64s([1] * 3), 8, 0, 4, 1, plan) == 0
    G, KC, QP, parts = (int(x) for x in plan)
    assert G >= 1 and KC == 32 and (parts - 1) * QP < 27 <= parts * QP
    assert lib.csgn_uint_pick_plan(4096, SHL, 0, 3, u64s([1] * 3), 8, 0, 4, 1, plan) == -1    # empty batch
    assert lib.csgn_uint_pick_plan(4096, 9, 2, 3, u64s([1] * 3), 8, 0, 4, 1, plan) == -1
    assert lib.csgn_uint_pick_plan(4096, SHL, 2, 3, u64s([1] * 3), 8, 0, 4, 1, None) == -1


def test_fails_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_uint_pick_gpu.py covers the device")
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    ptrs = (C.c_void_p * 64)(*([p] * 64))
    one = u64s([1] * 64)
    rc = lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, None)
    assert rc == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert lib.csgn_uint_pick(1247, EACH, 4, 3, ptrs, one, 8, 5, ptrs, 1, ptrs, None) == -3
    # argument errors are reported before the device is looked for
    assert lib.csgn_uint_pick(0, SHL, 4, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, None) == -1        # n_bits
    assert lib.csgn_uint_pick(1247, 0, 4, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, None) == -1       # op
    assert lib.csgn_uint_pick(1247, 6, 4, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 0, ptrs, one, 8, 0, ptrs, 1, ptrs, None) == -1     # index width
    assert lib.csgn_uint_pick(1247, SHL, 4, 17, ptrs, one, 8, 0, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, one, 0, 0, ptrs, 1, ptrs, None) == -1     # width
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, one, 65, 0, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, ROTR, 4, 3, ptrs, one, 8, 8, ptrs, 1, ptrs, None) == -1    # rows
    assert lib.csgn_uint_pick(1247, EACH, 4, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, EACH, 4, 3, ptrs, one, 8, 9, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, one, 8, 0, ptrs, 0, ptrs, None) == -1     # terms
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, one, 8, 0, ptrs, LIMIT, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, u64s([1, 0, 1]), 8, 0, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, u64s([1, LIMIT, 1]), 8, 0, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, None, one, 8, 0, ptrs, 1, ptrs, None) == -1     # host arrays
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, None, 8, 0, ptrs, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, one, 8, 0, None, 1, ptrs, None) == -1
    assert lib.csgn_uint_pick(1247, SHL, 4, 3, ptrs, one, 8, 0, ptrs, 1, None, None) == -1
    # too large: 3^16 terms * 20 words = 8.6e8 < 2^31, but 3 source terms pass it
    assert lib.csgn_uint_pick(1247, ROTL, 4, 16, ptrs, one, 1, 0, ptrs, 3, ptrs, None) == -2
    assert lib.csgn_uint_pick(1247, ROTL, 4, 16, ptrs, one, 1, 0, ptrs, 2, ptrs, None) == -3
    assert lib.csgn_uint_pick(1247, EACH, 4, 16, ptrs, u64s([2] * 16), 1, 1 << 16, ptrs, 1, ptrs, None) == -2
    assert lib.csgn_uint_pick(1247, ROTL, 1 << 44, 8, ptrs, one, 8, 0, ptrs, 1, ptrs, None) == -2   # batch


# -- the definition against the genuine reference and the oracle -----------------------------------------------------
def element_value(op, a, n, e=0):
    """value(p, r) of ONE element as flat words (compose_pick's argument)."""
    if op == EACH:
        return lambda p, r: a[p][e * n + r].ravel()
    return lambda p, r: a[p][e].ravel()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("v", [1, 2, 3])
@pytest.mark.parametrize("op", sorted(OPS))
def test_definition_matches_reference(oracle, ref, op, v, t, mixed):
    n_bits, d = 65, 4
    op = OPS[op]
    s = index_terms(v, mixed)
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    dl = (n_bits + 63) // 64
    for w, n in shapes(op, v):
        index, a = operands(n_bits, op, s, w, n, t, 1, 1000 * v + 10 * w + n)
        planes = [x[0].ravel() for x in index]
        add, mul = ref_ops(ref, n_bits, d)
        want = compose_pick(op, planes, element_value(op, a, n), w, n, add, mul, one, zero)
        add, mul = oracle_ops(oracle, n_bits)
        got = compose_pick(op, planes, element_value(op, a, n), w, n, add, mul, one, zero)
        words = np_pick(n_bits, op, index, a, n)
        for j in range(w):
            assert np.array_equal(got[j], want[j]), (w, n, j)
            assert got[j].size == t * pick_terms(op, s, w, n, j) * dl, (w, n, j)
            assert np.array_equal(words[j].ravel(), got[j]), (w, n, j)


@pytest.mark.parametrize("n_bits,d", [(63, 4), (129, 8), (1247, 16)])
def test_definition_matches_reference_at_other_sizes(oracle, ref, n_bits, d):
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    for op, w, n in ((SHL, 3, 0), (SHR, 5, 0), (ROTL, 3, 0), (ROTR, 5, 0), (EACH, 2, 3)):
        s = [2, 1]
        index, a = operands(n_bits, op, s, w, n, 2, 1, 77 + op)
        planes = [x[0].ravel() for x in index]
        add, mul = ref_ops(ref, n_bits, d)
        want = compose_pick(op, planes, element_value(op, a, n), w, n, add, mul, one, zero)
        words = np_pick(n_bits, op, index, a, n)
        for j in range(w):
            assert np.array_equal(words[j].ravel(), want[j]), (op, j)


@pytest.mark.parametrize("n_bits", [64, 63, 1247])
def test_definition_matches_oracle_batched(oracle, n_bits):
    """Element e with element e: every element of a batch against the oracle's operators on its own words."""
    s, t, batch = [2, 1, 3], 2, 3
    one, zero = const_term(n_bits, 1), const_term(n_bits, 0)
    add, mul = oracle_ops(oracle, n_bits)
    for op, w, n in ((SHL, 5, 0), (SHR, 3, 0), (ROTL, 5, 0), (ROTR, 3, 0), (EACH, 2, 6)):
        index, a = operands(n_bits, op, s, w, n, t, batch, 60 + op)
        words = np_pick(n_bits, op, index, a, n)
        for e in range(batch):
            want = compose_pick(op, [x[e].ravel() for x in index], element_value(op, a, n, e), w, n, add, mul, one, zero)
            for j in range(w):
                assert np.array_equal(words[j][e].ravel(), want[j]), (op, e, j)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("v", [1, 2, 3])
@pytest.mark.parametrize("op", sorted(OPS))
def test_decode_gives_the_definition(op, v, mixed):
    """One decode of every entry against rows_max, cut per output at E_j, reproduces the definition's words term for
    term; so does the concatenated numpy form the device tests compare against."""
    n_bits, batch = 129, 2
    op = OPS[op]
    s = index_terms(v, mixed)
    for w, n in shapes(op, v):
        for t in (1, 2):
            index, a = operands(n_bits, op, s, w, n, t, batch, 80 + w + n)
            want = np_pick(n_bits, op, index, a, n)
            got = np_pick_decoded(n_bits, op, index, a, n)
            fast = np_pick_fast(n_bits, op, index, a, n)
            for j in range(w):
                assert np.array_equal(got[j], want[j]), (w, n, t, j)
                assert np.array_equal(fast[j], want[j]), (w, n, t, j)


def test_shorter_outputs_are_prefixes_of_the_selector_stream():
    """With a source of ONE words the outputs ARE the E streams: output j's is the first E_j entries of the longest."""
    n_bits, v, w = 65, 3, 8
    index = [rand_terms(n_bits, 2, sk, 90 + k) for k, sk in enumerate([1, 2, 1])]
    ones = [np.broadcast_to(const_term(n_bits, 1), (2, 1, 2)).copy() for _ in range(w)]
    for op in (SHL, SHR):
        outs = np_pick(n_bits, op, index, ones)
        longest = max(outs, key=lambda o: o.shape[1])
        assert sorted({rows_of(op, v, w, 0, j) for j in range(w)}) == list(range(1, 9))
        for o in outs:
            assert np.array_equal(o, longest[:, :o.shape[1]])


# -- decryptions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2, 3])
@pytest.mark.parametrize("op", ["shl", "shr", "rotl", "rotr"])
def test_every_distance_decrypts(oracle, op, v):
    n_bits, d = 127, 8
    op = OPS[op]
    key, _ = oracle.keygen(n_bits, d, glibc_draws(270 + v, 64 * d + 64))
    rng = np.random.default_rng(v + 10 * op)
    for w in WIDTHS:
        ds = np.tile(np.arange(1 << v, dtype=np.uint64), 3)            # every distance, three integers each
        xs = rng.integers(0, 1 << w, len(ds)).astype(np.uint64)
        xs[:1 << v] = (1 << w) - 1                                      # every bit set: nothing shifted in is hidden
        index = encrypt_planes(oracle, n_bits, key, ds, v, 280 + v)
        a = encrypt_planes(oracle, n_bits, key, xs, w, 290 + w)
        got = decrypt_value(oracle, n_bits, key, np_pick(n_bits, op, index, a))
        want = [clear_pick(op, w, 0, int(x), int(dd)) for x, dd in zip(xs, ds)]
        assert [int(g) for g in got] == want, (op, v, w)


@pytest.mark.parametrize("v", [1, 2, 3])
def test_every_index_of_an_own_array_decrypts(oracle, v):
    n_bits, d = 127, 8
    key, _ = oracle.keygen(n_bits, d, glibc_draws(370 + v, 64 * d + 64))
    rng = np.random.default_rng(v)
    for n in each_rows(v):
        for w in (1, 3, 8):
            ds = np.arange(1 << v, dtype=np.uint64)                     # every index, past n too
            arrays = rng.integers(0, 1 << w, (len(ds), n)).astype(np.uint64)   # a different array per element
            index = encrypt_planes(oracle, n_bits, key, ds, v, 380 + v)
            a = encrypt_planes(oracle, n_bits, key, arrays.ravel(), w, 390 + w + n)
            got = decrypt_value(oracle, n_bits, key, np_pick(n_bits, EACH, index, a, n))
            want = [clear_pick(EACH, w, n, arrays[e], int(dd)) for e, dd in enumerate(ds)]
            assert [int(g) for g in got] == want, (v, n, w)


def test_multi_term_planes_decrypt(oracle):
    """Distance planes that are sums (x + ZERO ...: more terms, the same bit) shift by the same distances."""
    from tests.model import np_add
    n_bits, d, v, w = 127, 8, 3, 5
    key, _ = oracle.keygen(n_bits, d, glibc_draws(401, 64 * d + 64))
    ds = np.arange(1 << v, dtype=np.uint64)
    xs = np.full(len(ds), 0b10111, dtype=np.uint64)
    index = encrypt_planes(oracle, n_bits, key, ds, v, 402)
    zero = encrypt_planes(oracle, n_bits, key, np.zeros(len(ds), dtype=np.uint64), 1, 403)[0]
    index = [index[0], np_add(index[1], zero), np_add(np_add(index[2], zero), zero)]
    a = [np_add(p, zero) for p in encrypt_planes(oracle, n_bits, key, xs, w, 404)]
    for op in SHIFTS:
        outs = np_pick(n_bits, op, index, a)
        assert outs[w - 1].shape[1] == 2 * pick_terms(op, [1, 2, 3], w, 0, w - 1)
        got = decrypt_value(oracle, n_bits, key, outs)
        assert [int(g) for g in got] == [clear_pick(op, w, 0, int(x), int(dd)) for x, dd in zip(xs, ds)], op
