"""Bit-sliced integer steps on the device (csgn_uint_step), word for word against the definition of include/csgn_hip.h
(pinned against the reference and the oracle in tests/test_uint_cpu.py), in every form the knob uint_fused selects.
Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (ADD_FULL, ADD_HALF, EQ_STEP, GuardedOutputs, LT_FIRST, LT_STEP, STEPS, hip, np_step, np_uint_add, np_uint_eq,
                         np_uint_lt, np_uint_sub, rand_terms, step_terms)

pytestmark = pytest.mark.gpu

NS = [63, 64, 65, 129, 1247, 4096]
# (t_x, t_a, t_b, batch): fresh operands, carries and accumulators up to past the fused / pitched cut, multi-term
# left operands (rows that interleave)
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 1000), (3, 1, 1, 7), (8, 1, 1, 3), (31, 1, 1, 3), (63, 1, 1, 3), (90, 1, 1, 2),
          (3, 2, 3, 3), (1, 9, 8, 2), (2, 1, 40, 2)]


def reads_x(step):
    return step not in (ADD_HALF, LT_FIRST)


def run_step(hip, n, step, x, a, b, carry=True, alias=False, want=None):
    """The outputs, downloaded.  With `want` (the definition's words, one array per output) they are caller tensors of
    exactly those sizes between guard words, checked word for word and for writes outside them (tests/model.py,
    GuardedOutputs)."""
    up = hip.upload
    da = up(a.ravel())
    db = da if alias else up(b.ravel())
    dx = up(x.ravel()) if reads_x(step) else None
    guarded = GuardedOutputs(hip, [w.size for w in want]) if want is not None else None
    out = hip.uint_step(n, step, a.shape[0], da, a.shape[1], db, b.shape[1], dx, x.shape[1] if reads_x(step) else 0,
                        carry=carry, outs=guarded.outs if guarded else None)
    if guarded:
        return tuple(guarded.check(want, step))
    return tuple(hip.download(o) for o in out) if isinstance(out, tuple) else (hip.download(out),)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("step", sorted(STEPS.values()))
@pytest.mark.parametrize("shape", SHAPES)
def test_step_words(hip, knobs, n, step, shape):
    tx, ta, tb, batch = shape
    x, a, b = rand_terms(n, batch, tx, 7 * step + tx), rand_terms(n, batch, ta, 100 + ta), rand_terms(n, batch, tb, 200 + tb)
    want = [w.ravel() for w in np_step(n, step, x, a, b)]
    dl = (n + 63) // 64
    for o, w in enumerate(want):
        assert w.size == batch * step_terms(step, tx, ta, tb)[o] * dl
    for fused in (-1, 0, 1):
        knobs.set("uint_fused", fused)
        kernel = hip.lib.csgn_uint_step_kernel(n, step, batch, tx, ta, tb).decode()
        got = run_step(hip, n, step, x, a, b, want=want)
        assert len(got) == len(want)
        for o in range(len(want)):
            assert np.array_equal(got[o], want[o]), (fused, kernel, o)


@pytest.mark.parametrize("n", [65, 1247, 4096])
@pytest.mark.parametrize("step", sorted(STEPS.values()))
def test_step_aliased_operands_and_no_carry(hip, knobs, n, step):
    """d_a == d_b, and d_out1 = NULL (the carry neither computed nor written)."""
    tx, ta, batch = 3, 2, 33
    x, a = rand_terms(n, batch, tx, 5), rand_terms(n, batch, ta, 6)
    want = [w.ravel() for w in np_step(n, step, x, a, a)]
    for fused in (0, 1):
        knobs.set("uint_fused", fused)
        got = run_step(hip, n, step, x, a, a, alias=True, want=want)
        for o in range(len(want)):
            assert np.array_equal(got[o], want[o]), (fused, o)
        got = run_step(hip, n, step, x, a, rand_terms(n, batch, ta, 9), carry=False)
        assert len(got) == 1
        assert np.array_equal(got[0], np_step(n, step, x, a, rand_terms(n, batch, ta, 9))[0].ravel()), fused


@pytest.mark.parametrize("n", [65, 1247])
@pytest.mark.parametrize("step", sorted(STEPS.values()))
def test_step_words_large_batch(hip, knobs, n, step):
    """65 537 fresh elements (carry of 3 terms): many workgroups, odd element count."""
    x, a, b = rand_terms(n, 65537, 3, 1), rand_terms(n, 65537, 1, 2), rand_terms(n, 65537, 1, 3)
    want = [w.ravel() for w in np_step(n, step, x, a, b)]
    for fused in (0, 1):
        knobs.set("uint_fused", fused)
        got = run_step(hip, n, step, x, a, b, want=want)
        for o in range(len(want)):
            assert np.array_equal(got[o], want[o]), (fused, o)


def test_whole_ops_on_device_decrypt(hip, oracle):
    """5-bit add, subtract, equality and less-than chained step by step on the device (fresh planes from the oracle),
    words equal to the numpy composition, decryptions equal to clear arithmetic."""
    n, d, w, count = 127, 8, 5, 300
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(77, 64 * d + 64))
    mask = hip.upload(oracle.key_mask(n, key))
    rng = np.random.default_rng(5)
    va, vb = rng.integers(0, 1 << w, count), rng.integers(0, 1 << w, count)
    vb[::5] = va[::5]

    def enc(v, j, s):
        bits = ((v >> j) & 1).astype(np.uint8)
        return oracle.encrypt_seq(n, key, bits, glibc_draws(s, count * (n + 2)))[0].reshape(count, 1, dl)

    a = [enc(va, j, 1000 + j) for j in range(w)]
    b = [enc(vb, j, 2000 + j) for j in range(w)]
    up = hip.upload

    def dec(words, terms):
        return hip.download(hip.decrypt_uniform(n, count, terms, up(words.ravel()), mask)).astype(np.uint64)

    # add on the device, plane by plane (the carry stays on the device)
    s, c = hip.uint_step(n, ADD_HALF, count, up(a[0].ravel()), 1, up(b[0].ravel()), 1)
    sums, tc = [(s, 2)], 1
    for j in range(1, w):
        s, c2 = hip.uint_step(n, ADD_FULL, count, up(a[j].ravel()), 1, up(b[j].ravel()), 1, c, tc)
        sums.append((s, 2 + tc))
        c, tc = c2, 1 + 2 * tc
    want = np_uint_add(n, a, b)
    total = np.zeros(count, dtype=np.uint64)
    for j, (s, t) in enumerate(sums):
        assert np.array_equal(hip.download(s), want[j].ravel()), j
        total |= dec(want[j], t) << np.uint64(j)
    assert np.array_equal(total, (va + vb).astype(np.uint64) & np.uint64((1 << w) - 1))
    # equality / less-than accumulators on the device
    e = np_uint_eq(n, a[:1], b[:1])
    de, te = up(e.ravel()), e.shape[1]
    dlt, tl = hip.uint_step(n, LT_FIRST, count, up(a[0].ravel()), 1, up(b[0].ravel()), 1), 2
    for j in range(1, w):
        de, te = hip.uint_step(n, EQ_STEP, count, up(a[j].ravel()), 1, up(b[j].ravel()), 1, de, te), te * 3
        dlt, tl = hip.uint_step(n, LT_STEP, count, up(a[j].ravel()), 1, up(b[j].ravel()), 1, dlt, tl), 2 * (1 + tl) + tl
    eq, lt = np_uint_eq(n, a, b), np_uint_lt(n, a, b)
    assert np.array_equal(hip.download(de), eq.ravel()) and np.array_equal(hip.download(dlt), lt.ravel())
    assert np.array_equal(dec(eq, te), (va == vb).astype(np.uint64))
    assert np.array_equal(dec(lt, tl), (va < vb).astype(np.uint64))
    sub = np_uint_sub(n, a, b)
    diff = sum(dec(p, p.shape[1]) << np.uint64(j) for j, p in enumerate(sub))
    assert np.array_equal(diff, (va - vb).astype(np.uint64) & np.uint64((1 << w) - 1))


def test_uint_step_argument_errors(hip):
    L = hip.lib
    x = hip.empty_words(64)
    p = x.data_ptr()
    assert L.csgn_uint_step(1247, 99, 1, p, 1, p, 1, p, 1, p, p, 0) == -1
    assert L.csgn_uint_step(1247, ADD_FULL, 1, None, 1, p, 1, p, 1, p, p, 0) == -1      # ADD_FULL reads x
    assert L.csgn_uint_step(1247, LT_STEP, 1, p, 1, None, 1, p, 1, p, None, 0) == -1
    assert L.csgn_uint_step(1247, ADD_HALF, 1, None, 0, p, 1, p, 1, None, p, 0) == -1   # no out0
    assert L.csgn_uint_step(1247, ADD_HALF, 0, None, 0, p, 1, p, 1, None, None, 0) == 0  # empty batch
    assert L.csgn_uint_step(1247, EQ_STEP, 1, p, 3 ** 16, p, 1, p, 1, p, None, 0) == -2
