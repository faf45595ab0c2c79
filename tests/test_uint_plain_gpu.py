"""Comparisons against a public constant on the device (csgn_uint_plain), word for word against the definition of
include/csgn_hip.h (pinned against the reference and the oracle in tests/test_uint_plain_cpu.py), in both forms the knob
uint_plain_fused selects.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import glibc_draws
from tests.model import (CLEAR, CMPS, EQ, GE, GT, LE, LT, NE, GuardedOutputs, decrypt_bits, encrypt_planes, full_width_cases, hip,
                         np_plain, plain_terms, rand_terms, u64s)

pytestmark = pytest.mark.gpu


def edge_ks(w):
    top = (1 << w) - 1
    ks = {0, 1, top, 1 << (w - 1), top ^ 1, 0x5555 & top, 0xAAAA & top, (0x2D1B * w) & top}
    return sorted(ks)


def run(hip, n, cmp, planes, k, want=None):
    """The output, downloaded.  With `want` (the definition's words) the output is a caller tensor of exactly that size
    between guard words, checked word for word and for writes outside it (tests/model.py, GuardedOutputs)."""
    dev = [hip.upload(p.ravel()) for p in planes]
    if want is None:
        return hip.download(hip.uint_plain(n, cmp, planes[0].shape[0], dev, [p.shape[1] for p in planes], k))
    guarded = GuardedOutputs(hip, [want.size])
    hip.uint_plain(n, cmp, planes[0].shape[0], dev, [p.shape[1] for p in planes], k, out=guarded.outs[0])
    return guarded.check([want], (cmp, k))[0]


def check_forms(hip, knobs, n, cmp, planes, k):
    want = np_plain(n, cmp, planes, k).ravel()
    for fused in (-1, 0, 1):
        knobs.set("uint_plain_fused", fused)
        got = run(hip, n, cmp, planes, k, want)
        assert np.array_equal(got, want), (fused, cmp, k, [p.shape[1] for p in planes])


# 63 and 129: odd dL, the 8-byte-unit kernel
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("tmode", ["1", "2", "3", "mixed"])
def test_plain_words(hip, knobs, n, w, tmode):
    rng = np.random.default_rng(w * 10 + len(tmode))
    ts = [int(x) for x in rng.integers(1, 4, w)] if tmode == "mixed" else [int(tmode)] * w
    if w == 8 and tmode != "1":
        ts = ts[:6] + [1, 1]                                        # at most 4^6 * 2 * 2 = 16384 terms (EQ, k = 0)
    batch = 3
    planes = [rand_terms(n, batch, t, 300 + 7 * j + t) for j, t in enumerate(ts)]
    for k in edge_ks(w):
        for cmp in CMPS.values():
            check_forms(hip, knobs, n, cmp, planes, k)


@pytest.mark.parametrize("w", [12, 16])
def test_plain_words_wide(hip, knobs, w):
    n, batch = 1247, 2
    planes = [rand_terms(n, batch, 1, 500 + j) for j in range(w)]
    top = (1 << w) - 1
    for k in (top, top ^ 0x0F0, 0xA5A5 & top, 1 << (w - 1), 4711 & top):
        for cmp in (EQ, NE, LT, LE, GT, GE):
            if plain_terms(cmp, w, k, [1] * w) <= 4096:
                check_forms(hip, knobs, n, cmp, planes, k)


@pytest.mark.parametrize("n", [65, 1247])
@pytest.mark.parametrize("w", [17, 31, 32, 33, 63, 64])
def test_plain_words_full_width(hip, knobs, n, w):
    """Levels at and above bit 16, 32 and 63: the kernel's 64-bit level masks and 64-entry tables, every (cmp, k) of at
    most 4096 terms over fresh planes."""
    batch = 3
    planes = [rand_terms(n, batch, 1, 4000 + 67 * w + j) for j in range(w)]
    for cmp, k in full_width_cases(w):
        check_forms(hip, knobs, n, cmp, planes, k)


def test_plain_64bit_by_decryption(hip, knobs, oracle):
    """w = 64 against clear uint64 comparisons, values and constants at and around 0, 2^63 and 2^64 - 1."""
    n, d, w = 1247, 16, 64
    key, _ = oracle.keygen(n, d, glibc_draws(164, 64 * d + 64))
    rng = np.random.default_rng(64)
    values = np.concatenate([np.array([0, 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, (1 << 64) - 1, (1 << 64) - 2],
                                      dtype=np.uint64), rng.integers(0, 2**64 - 1, 9, dtype=np.uint64, endpoint=True)])
    planes = encrypt_planes(oracle, n, key, values, w, 190)
    knobs.unset("uint_plain_fused")
    ks = [0, 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, (1 << 64) - 1, (1 << 64) - 2, int(values[-1]) | 0xFFFFFFFFFFFF0000]
    for k in ks:
        for cmp, f in CLEAR.items():
            if not 0 < plain_terms(cmp, w, k, [1] * w) <= 4096:
                continue
            got = run(hip, n, cmp, planes, k).reshape(len(values), -1, (n + 63) // 64)
            assert np.array_equal(got.reshape(-1), np_plain(n, cmp, planes, k).ravel()), (cmp, k)
            assert np.array_equal(decrypt_bits(oracle, n, key, got), f(values, np.uint64(k))), (cmp, k)


@pytest.mark.parametrize("batch", [1, 2, 255, 257, 4099, (1 << 16) + 3])
def test_plain_batches(hip, knobs, batch):
    n, w = 65, 4
    ts = [1, 2, 1, 1]
    planes = [rand_terms(n, batch, t, 700 + j) for j, t in enumerate(ts)]
    for k, cmp in ((5, EQ), (9, LT), (6, GE), (0, LT), (15, LE)):
        check_forms(hip, knobs, n, cmp, planes, k)


def test_plain_16bit_spans_many_workgroups(hip, knobs):
    """2^16 terms (10.5 MB) per element at N=1247: every element is written by many workgroups."""
    n, w, batch = 1247, 16, 3
    planes = [rand_terms(n, batch, 1, 900 + j) for j in range(w)]
    for cmp, k in ((EQ, 0), (LT, 1), (GE, 1), (GT, 1)):
        want = np_plain(n, cmp, planes, k).ravel()
        assert want.size >= batch * ((1 << 15) - 1) * 20
        for fused in (1, 0):
            knobs.set("uint_plain_fused", fused)
            assert np.array_equal(run(hip, n, cmp, planes, k, want), want), (cmp, fused)


@pytest.mark.parametrize("w", [1, 2, 3, 4, 8])
def test_plain_truth_tables_by_decryption(hip, knobs, oracle, w):
    n, d = 1247, 16
    key, _ = oracle.keygen(n, d, glibc_draws(170 + w, 64 * d + 64))
    values = np.arange(1 << w, dtype=np.uint64) if w <= 4 else np.random.default_rng(w).integers(0, 1 << w, 64).astype(np.uint64)
    planes = encrypt_planes(oracle, n, key, values, w, 180 + w)
    ks = range(1 << w) if w <= 4 else [0, 1, 77, 128, 254, 255, int(values[3])]
    knobs.unset("uint_plain_fused")
    for k in ks:
        for cmp, f in CLEAR.items():
            got = run(hip, n, cmp, planes, k).reshape(len(values), -1, (n + 63) // 64)
            assert np.array_equal(decrypt_bits(oracle, n, key, got), f(values, np.uint64(k))), (cmp, k)


def test_plain_argument_errors(hip):
    lib = hip.lib
    t = hip.upload(np.zeros(64 * 20, dtype=np.uint64))
    planes = (C.c_void_p * 64)(*([t.data_ptr()] * 64))
    one = u64s([1] * 64)
    out = t.data_ptr()
    assert lib.csgn_uint_plain(1247, 0, 1, 4, 3, planes, one, out, hip.stream) == -1
    assert lib.csgn_uint_plain(1247, EQ, 1, 4, 16, planes, one, out, hip.stream) == -1
    assert lib.csgn_uint_plain(1247, EQ, 1, 0, 0, planes, one, out, hip.stream) == -1
    assert lib.csgn_uint_plain(1247, EQ, 1, 4, 3, planes, u64s([1, 1, 0, 1]), out, hip.stream) == -1
    assert lib.csgn_uint_plain(1247, EQ, 1, 4, 3, planes, one, None, hip.stream) == -1
    nullp = (C.c_void_p * 4)(t.data_ptr(), None, t.data_ptr(), t.data_ptr())
    assert lib.csgn_uint_plain(1247, EQ, 1, 4, 3, nullp, one, out, hip.stream) == -1
    assert lib.csgn_uint_plain(1247, EQ, 1, 27, 0, planes, one, out, hip.stream) == -2
    assert lib.csgn_uint_plain(1247, EQ, 0, 4, 3, planes, one, None, hip.stream) == 0      # empty batch
    for cmp in (NE, LE, GT, GE, LT):
        assert lib.csgn_uint_plain(1247, cmp, 0, 4, 3, planes, one, out, hip.stream) == 0
