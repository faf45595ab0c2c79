"""Bit-sliced encrypted integers (csgn_uint_*) on a box without a GPU: the term-count table, the dispatch names, the
loud failure without a device, the DEFINITION of every per-bit step -- the composition of the reference's operator+ /
operator* with the ONE term -- pinned against the compiled reference and the oracle, and the whole operations (add,
subtract, the six comparisons, select) composed from those steps and decrypted under random keys.  The device side is
tests/test_uint_gpu.py."""

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (ADD_FULL, ADD_HALF, EQ_STEP, LT_FIRST, LT_STEP, MASK64, STEPS, compose_step, lib, np_mul,
                         np_not, np_step, np_uint_add, np_uint_eq, np_uint_lt, np_uint_select, np_uint_sub, oracle_ops,
                         rand_terms, ref_ops, step_terms)


# -- the C ABI, host side ---------------------------------------------------------------------------------------------
def test_uint_step_terms_table(lib):
    for step in STEPS.values():
        for tx, ta, tb in [(1, 1, 1), (3, 1, 1), (2, 3, 5), (26, 1, 1), (64, 64, 64), (7, 1, 9)]:
            want = step_terms(step, tx, ta, tb)
            for output in range(2):
                got = lib.csgn_uint_step_terms(step, output, tx, ta, tb)
                assert got == (want[output] if output < len(want) else 0), (step, output, tx, ta, tb)
    for bad in (0, 6, -1, 100):
        assert lib.csgn_uint_step_terms(bad, 0, 1, 1, 1) == 0
    for step in (EQ_STEP, LT_FIRST, LT_STEP):
        assert lib.csgn_uint_step_terms(step, 1, 1, 1, 1) == 0       # only the ADD steps have a carry
    assert lib.csgn_uint_step_terms(ADD_HALF, 2, 1, 1, 1) == 0
    assert lib.csgn_uint_step_terms(ADD_HALF, -1, 1, 1, 1) == 0
    # an operand the step reads has no terms; the ones it does not read may be 0
    assert lib.csgn_uint_step_terms(ADD_HALF, 0, 0, 2, 3) == 5
    assert lib.csgn_uint_step_terms(LT_FIRST, 0, 0, 2, 3) == 9
    assert lib.csgn_uint_step_terms(ADD_FULL, 0, 0, 1, 1) == 0
    assert lib.csgn_uint_step_terms(EQ_STEP, 0, 0, 1, 1) == 0
    assert lib.csgn_uint_step_terms(LT_STEP, 0, 0, 1, 1) == 0
    assert lib.csgn_uint_step_terms(ADD_HALF, 0, 1, 0, 1) == 0
    assert lib.csgn_uint_step_terms(LT_STEP, 0, 1, 1, 0) == 0
    # overflow
    assert lib.csgn_uint_step_terms(ADD_HALF, 1, 0, 1 << 32, 1 << 32) == 0
    assert lib.csgn_uint_step_terms(ADD_HALF, 0, 0, 1 << 32, 1 << 32) == 1 << 33     # the sum alone does not
    assert lib.csgn_uint_step_terms(ADD_FULL, 1, 1 << 40, 1 << 30, 1) == 0
    assert lib.csgn_uint_step_terms(EQ_STEP, 0, 1 << 40, 1 << 30, 1) == 0
    assert lib.csgn_uint_step_terms(LT_STEP, 0, MASK64, 1, 1) == 0
    assert lib.csgn_uint_step_terms(LT_FIRST, 0, 0, MASK64, 1) == 0


def test_uint_dispatch_names(lib, knobs):
    knobs.unset("uint_fused")
    name = lambda st, tx, ta, tb, n=1247: lib.csgn_uint_step_kernel(n, st, 1 << 20, tx, ta, tb).decode()
    for st in STEPS.values():
        assert name(st, 1, 1, 1) == "k_uint_step", st               # fresh operands: one kernel
        assert name(st, 3, 1, 1) == "k_uint_step", st               # short carries and accumulators too
    # past the cut (64 product terms per element, 162 for LT_STEP): the tuned launchers into the outputs' slices
    assert name(ADD_HALF, 0, 8, 8) == "k_uint_step" and name(ADD_HALF, 0, 9, 8) == "pitched"
    assert name(ADD_FULL, 63, 1, 1) == "pitched"                    # carry: 1 + 2 * 63 product terms
    assert name(ADD_FULL, 31, 1, 1) == "k_uint_step"                # 63
    assert name(LT_FIRST, 0, 64, 1) == "pitched"
    assert name(LT_STEP, 80, 1, 1) == "k_uint_step"                 # 2 * (1 + 80): LT_STEP's cut is 162
    assert name(LT_STEP, 81, 1, 1) == "pitched"                     # rows [a x b|l], [b x b|l] as slices
    assert name(EQ_STEP, 1, 40, 40) == "pitched"
    # rows that interleave (a concatenated right operand under a left operand of more than one term): always fused
    assert name(EQ_STEP, 3, 1, 1) == "k_uint_step"
    assert name(EQ_STEP, 2187, 1, 1) == "k_uint_step"
    assert name(LT_STEP, 80, 2, 1) == "k_uint_step"
    assert name(LT_STEP, 80, 1, 2) == "k_uint_step"
    assert name(0, 1, 1, 1) == "" and name(ADD_FULL, 0, 1, 1) == ""
    knobs.set("uint_fused", 1)
    assert name(ADD_FULL, 63, 1, 1) == "k_uint_step"
    assert name(LT_STEP, 200, 1, 1) == "k_uint_step"
    knobs.set("uint_fused", 0)
    for st in STEPS.values():
        assert name(st, 1, 1, 1) == "pitched", st
    assert name(EQ_STEP, 3, 1, 1) == "k_uint_step"                  # no pitched form
    assert name(LT_STEP, 1, 2, 1) == "k_uint_step"


def test_uint_step_fails_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_uint_gpu.py covers the device")
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    rc = lib.csgn_uint_step(1247, ADD_FULL, 4, p, 1, p, 1, p, 1, p, p, None)
    assert rc == -3, lib.csgn_last_error()
    assert b"no CPU fallback" in lib.csgn_last_error()
    assert lib.csgn_uint_step(1247, ADD_HALF, 4, None, 0, p, 1, p, 1, p, None, None) == -3
    assert lib.csgn_uint_step(1247, LT_STEP, 4, p, 2, p, 1, p, 1, p, None, None) == -3
    # argument errors are reported before the device is looked for
    assert lib.csgn_uint_step(1247, 42, 4, p, 1, p, 1, p, 1, p, p, None) == -1
    assert lib.csgn_uint_step(0, ADD_FULL, 4, p, 1, p, 1, p, 1, p, p, None) == -1
    assert lib.csgn_uint_step(1247, ADD_FULL, 4, p, 0, p, 1, p, 1, p, p, None) == -1      # a carry of no terms
    assert lib.csgn_uint_step(1247, EQ_STEP, 4, p, 1, p, 0, p, 1, p, None, None) == -1
    # too large: 3^17 terms * 20 words per element exceed 2^31 words
    assert lib.csgn_uint_step(1247, EQ_STEP, 4, p, 3 ** 16, p, 1, p, 1, p, None, None) == -2
    assert lib.csgn_uint_step(1247, ADD_FULL, 4, p, 1 << 26, p, 1, p, 1, p, p, None) == -2   # the carry's 2^27 + 1
    assert lib.csgn_uint_step(1247, ADD_FULL, 4, p, 1 << 26, p, 1, p, 1, p, None, None) == -3  # ... not computed
    assert lib.csgn_uint_step(1247, ADD_FULL, 4, p, 1 << 25, p, 1, p, 1, p, p, None) == -3   # 2^26 + 1 terms fit
    assert lib.csgn_uint_step(1247, ADD_FULL, 1 << 56, p, 1, p, 1, p, 1, p, p, None) == -2  # batch


# -- every step's definition against the genuine reference and the oracle -------------------------------------------------
# N % 64 != 0 only for the reference (tests/test_gates_cpu.py: it writes past its bitlen array at N % 64 == 0)
@pytest.mark.parametrize("n,d", [(63, 4), (65, 4), (129, 8), (1247, 16)])
@pytest.mark.parametrize("step", sorted(STEPS.values()))
@pytest.mark.parametrize("tx,ta,tb", [(1, 1, 1), (3, 1, 1), (2, 3, 2), (4, 2, 1)])
def test_step_definition_matches_reference(oracle, ref, n, d, step, tx, ta, tb):
    x, a, b = (rand_terms(n, 1, t, seed)[0].ravel() for t, seed in ((tx, 11), (ta, 12), (tb, 13)))
    want = compose_step(ref_ops(ref, n, d), n, step, x, a, b)
    got = compose_step(oracle_ops(oracle, n), n, step, x, a, b)
    words = np_step(n, step, x.reshape(1, tx, -1), a.reshape(1, ta, -1), b.reshape(1, tb, -1))
    dl = (n + 63) // 64
    for o in range(len(want)):
        assert np.array_equal(got[o], want[o]), (step, o)
        assert got[o].size == step_terms(step, tx, ta, tb)[o] * dl
        assert np.array_equal(words[o].ravel(), got[o]), (step, o)


@pytest.mark.parametrize("n", [64, 4096, 63, 1247])
@pytest.mark.parametrize("step", sorted(STEPS.values()))
def test_step_definition_matches_oracle(oracle, n, step):
    tx, ta, tb, batch = 3, 2, 2, 4
    x, a, b = rand_terms(n, batch, tx, 21), rand_terms(n, batch, ta, 22), rand_terms(n, batch, tb, 23)
    words = np_step(n, step, x, a, b)
    for e in range(batch):
        want = compose_step(oracle_ops(oracle, n), n, step, x[e].ravel(), a[e].ravel(), b[e].ravel())
        for o in range(len(want)):
            assert np.array_equal(words[o][e].ravel(), want[o]), (e, o)


def test_step_layout_examples():
    """The carry of ADD_FULL is [a x b rows][a x c rows][b x c rows]; LT_STEP's product rows are a_i x [b | l], then
    b_i x [b | l]."""
    n = 129
    x, a, b = rand_terms(n, 1, 2, 31), rand_terms(n, 1, 2, 32), rand_terms(n, 1, 3, 33)
    _, carry = np_step(n, ADD_FULL, x, a, b)
    assert np.array_equal(carry, np.concatenate([np_mul(a, b), np_mul(a, x), np_mul(b, x)], axis=1))
    (lt,) = np_step(n, LT_STEP, x, a, b)
    rows = [a[:, i:i + 1] & np.concatenate([b, x], axis=1) for i in range(2)] + \
           [b[:, i:i + 1] & np.concatenate([b, x], axis=1) for i in range(3)]
    assert np.array_equal(lt, np.concatenate(rows + [x], axis=1))


# -- whole operations: decryptions equal clear unsigned arithmetic ----------------------------------------------------------
def run_whole_ops(oracle, n, d, w, va, vb, vs, seed):
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(seed, 64 * d + 64))
    count = len(va)

    def enc(values, bit, s):
        bits = ((np.asarray(values) >> bit) & 1).astype(np.uint8)
        return oracle.encrypt_seq(n, key, bits, glibc_draws(s, count * (n + 2)))[0].reshape(count, 1, dl)

    a = [enc(va, j, seed * 100 + j) for j in range(w)]
    b = [enc(vb, j, seed * 100 + 50 + j) for j in range(w)]
    s = enc(vs, 0, seed * 100 + 99)

    def dec(x):
        return np.array([oracle.decrypt_canonical(n, key, x[e].ravel()) for e in range(count)], dtype=np.uint64)

    def dec_int(planes):
        return sum(dec(p) << np.uint64(j) for j, p in enumerate(planes))

    va, vb, vs = (np.asarray(v, dtype=np.uint64) for v in (va, vb, vs))
    mod = np.uint64((1 << w) - 1)
    assert np.array_equal(dec_int(np_uint_add(n, a, b)), (va + vb) & mod)
    assert np.array_equal(dec_int(np_uint_sub(n, a, b)), (va - vb) & mod)
    eq, lt, gt = np_uint_eq(n, a, b), np_uint_lt(n, a, b), np_uint_lt(n, b, a)
    assert np.array_equal(dec(eq), va == vb)
    assert np.array_equal(dec(np_not(n, eq)), va != vb)
    assert np.array_equal(dec(lt), va < vb)
    assert np.array_equal(dec(gt), va > vb)
    assert np.array_equal(dec(np_not(n, gt)), va <= vb)
    assert np.array_equal(dec(np_not(n, lt)), va >= vb)
    assert np.array_equal(dec_int(np_uint_select(n, s, a, b)), np.where(vs & np.uint64(1), va, vb))
    # the sizes the issue states for fresh planes
    assert np_uint_add(n, a, b)[-1].shape[1] == 2 ** (w - 1) + 1 if w > 1 else 2
    assert eq.shape[1] == 3 ** w and lt.shape[1] == 3 ** w - 1


def test_whole_ops_all_3bit_pairs(oracle):
    va, vb = np.meshgrid(np.arange(8), np.arange(8))
    va, vb = va.ravel(), vb.ravel()
    vs = np.arange(64) % 2
    run_whole_ops(oracle, 127, 8, 3, va, vb, vs, 41)


def test_whole_ops_random_8bit_pairs(oracle):
    rng = np.random.default_rng(8)
    va, vb = rng.integers(0, 256, 500), rng.integers(0, 256, 500)
    vb[::7] = va[::7]                                               # some equal pairs
    run_whole_ops(oracle, 127, 8, 8, va, vb, rng.integers(0, 2, 500), 42)
