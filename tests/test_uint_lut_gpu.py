"""Public lookup tables on the device (csgn_uint_lut_apply), word for word against the definition of include/csgn_hip.h
(pinned against the reference and the oracle in tests/test_uint_lut_cpu.py), in both forms the knob uint_lut_fused
selects.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (EQ, GuardedOutputs, aes_sbox, c_terms, decrypt_bits, decrypt_value, encrypt_planes, hip, mul4x4,
                         np_add, np_lut, np_plain, rand_terms, random_table, u64s)

pytestmark = pytest.mark.gpu


def run(hip, n, planes, table, m, want=None):
    """The outputs, downloaded.  With `want` (the definition's words, one array per output) they are caller tensors of
    exactly those sizes between guard words, checked word for word and for writes outside them (tests/model.py,
    GuardedOutputs)."""
    dev = [hip.upload(p.ravel()) for p in planes]
    guarded = GuardedOutputs(hip, [x.size for x in want]) if want is not None else None
    outs = hip.uint_lut(n, planes[0].shape[0], dev, [p.shape[1] for p in planes], table, m,
                        outs=guarded.outs if guarded else None)
    return guarded.check(want, m) if guarded else [hip.download(o) for o in outs]


def check_forms(hip, knobs, n, planes, table, m, forms=(-1, 0, 1)):
    want = [x.ravel() for x in np_lut(n, planes, table, m)]
    for fused in forms:
        knobs.set("uint_lut_fused", fused)
        got = run(hip, n, planes, table, m, want)
        for j in range(m):
            assert np.array_equal(got[j], want[j]), (fused, j, [p.shape[1] for p in planes])


def tables_for(w, m, seed):
    top = (1 << m) - 1 if m < 64 else (1 << 64) - 1
    return [random_table(w, m, seed), [(3 * x + 1) & top for x in range(1 << w)], [0] * (1 << w), [top] * (1 << w),
            [x & top for x in range(1 << w)]]


# 63 and 129: odd dL, the 8-byte-unit kernel
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("tmode", ["1", "2", "3", "mixed"])
def test_lut_words(hip, knobs, n, w, tmode):
    rng = np.random.default_rng(w * 10 + len(tmode))
    ts = [int(x) for x in rng.integers(1, 4, w)] if tmode == "mixed" else [int(tmode)] * w
    if w == 8 and tmode != "1":
        ts = ts[:3] + [1] * 5                                       # at most 27 * 2^5 terms a monomial
    batch = 3
    planes = [rand_terms(n, batch, t, 300 + 7 * i + t) for i, t in enumerate(ts)]
    for m in (1, 8, 64):
        if w == 8 and m == 64 and tmode != "1":
            continue
        forms = (-1, 0, 1) if (w < 8 or m == 1) else (-1, 1)      # the composed form: one launch per factor
        for table in tables_for(w, m, w * 1000 + m + n)[: 2 if m == 64 else 5]:
            check_forms(hip, knobs, n, planes, table, m, forms)


@pytest.mark.parametrize("batch", [1, 257, 4099, (1 << 16) + 3])
@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_lut_batches(hip, knobs, batch, tmode):
    n, w = 65, 4
    ts = [1] * w if tmode == "1" else [1, 2, 1, 3]
    planes = [rand_terms(n, batch, t, 700 + i) for i, t in enumerate(ts)]
    check_forms(hip, knobs, n, planes, [(3 * x) % 16 for x in range(16)], 4)
    check_forms(hip, knobs, n, planes, [bin(x).count("1") for x in range(16)], 3, (-1, 1))


@pytest.mark.parametrize("w,m", [(12, 1), (12, 3), (16, 1)])
@pytest.mark.parametrize("n", [1247, 4096])
def test_lut_wide_inputs_span_many_workgroups(hip, knobs, w, m, n):
    """Three subset tables; at N=4096 they pass the LDS budget at whole terms and are built over slices of units."""
    batch = 2
    planes = [rand_terms(n, batch, 1, 900 + i) for i in range(w)]
    table = random_table(w, m, w * 7 + m)
    want = [x.ravel() for x in np_lut(n, planes, table, m)]
    assert want[0].size >= batch * (1 << (w - 2)) * ((n + 63) // 64)
    knobs.set("uint_lut_fused", 1)
    got = run(hip, n, planes, table, m)
    for j in range(m):
        assert np.array_equal(got[j], want[j]), j


def test_lut_sbox_all_inputs_by_decryption(hip, knobs, oracle):
    n, d = 1247, 16
    key, _ = oracle.keygen(n, d, glibc_draws(201, 64 * d + 64))
    values = np.arange(256, dtype=np.uint64)
    planes = encrypt_planes(oracle, n, key, values, 8, 202)
    sbox = aes_sbox()
    knobs.unset("uint_lut_fused")
    outs = run(hip, n, planes, sbox, 8)
    want = np_lut(n, planes, sbox, 8)
    for j in range(8):
        assert np.array_equal(outs[j], want[j].ravel()), j
    got = decrypt_value(oracle, n, key, [o.reshape(256, -1, (n + 63) // 64) for o in outs])
    assert [int(v) for v in got] == sbox


def test_lut_two_input_multiply_by_decryption(hip, knobs, oracle):
    """4x4-bit multiply as one 8-bit index a + (b << 4): the planes of a, then those of b."""
    n, d = 1247, 16
    key, _ = oracle.keygen(n, d, glibc_draws(211, 64 * d + 64))
    rng = np.random.default_rng(3)
    a = rng.integers(0, 16, 200).astype(np.uint64)
    b = rng.integers(0, 16, 200).astype(np.uint64)
    planes = encrypt_planes(oracle, n, key, a, 4, 212) + encrypt_planes(oracle, n, key, b, 4, 213)
    knobs.unset("uint_lut_fused")
    outs = run(hip, n, planes, mul4x4(), 8)
    got = decrypt_value(oracle, n, key, [o.reshape(200, -1, (n + 63) // 64) for o in outs])
    assert np.array_equal(got, a * b)


def test_lut_compact_keeps_count_and_today_route_compacts_to_it(hip, knobs, oracle):
    """The ANF is already reduced: compacting it drops nothing.  Today's route, sum over k of equalTo(a, k), compacts to
    the same term count and decrypts to the same bits."""
    n, d, w = 1247, 16, 4
    key, _ = oracle.keygen(n, d, glibc_draws(221, 64 * d + 64))
    values = np.arange(16, dtype=np.uint64)
    planes = encrypt_planes(oracle, n, key, values, w, 222)
    table = [(3 * x) % 16 for x in range(16)]
    knobs.unset("uint_lut_fused")
    outs = run(hip, n, planes, table, 4)
    dl = (n + 63) // 64
    for j in range(4):
        mine = outs[j].reshape(16, -1, dl)
        ks = [k for k in range(16) if (table[k] >> j) & 1]
        today = np_plain(n, EQ, planes, ks[0])
        for k in ks[1:]:
            today = np_add(today, np_plain(n, EQ, planes, k))
        for e in range(16):
            c_mine = oracle.compact(n, mine[e].ravel())
            c_today = oracle.compact(n, today[e].ravel())
            assert c_mine.size == mine[e].size, (j, e)
            assert c_today.size == c_mine.size, (j, e)
        assert np.array_equal(decrypt_bits(oracle, n, key, mine), decrypt_bits(oracle, n, key, today))


def test_lut_graph_capture_and_replay(hip, knobs):
    n, w, m, batch = 1247, 8, 8, 37
    sbox = aes_sbox()
    planes = [rand_terms(n, batch, 1, 800 + i) for i in range(w)]
    want = [x.ravel() for x in np_lut(n, planes, sbox, m)]
    knobs.set("uint_lut_fused", 1)
    dev = [hip.upload(p.ravel()) for p in planes]
    rc, T = c_terms(hip.lib, sbox, w, m, [1] * w)
    assert rc == 0
    dl = (n + 63) // 64
    outs = [hip.empty_words(batch * t * dl) for t in T]
    handle = hip.uint_lut_create(sbox, w, m, [1] * w)
    try:
        assert hip.lib.csgn_uint_lut_kernel(n, handle, batch) == b"k_uint_lut"
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            hip.uint_lut_apply(handle, n, batch, dev, T, outs)          # warm-up outside the capture
        s.synchronize()
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            hip.uint_lut_apply(handle, n, batch, dev, T, outs)
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for j in range(m):
            assert np.array_equal(hip.download(outs[j]), want[j]), j
    finally:
        torch.cuda.synchronize()
        hip.lib.csgn_uint_lut_destroy(handle)


def test_lut_dispatch_names(hip, knobs):
    handle = hip.uint_lut_create(list(range(16)), 4, 4, [1] * 4)
    try:
        knobs.unset("uint_lut_fused")
        assert hip.lib.csgn_uint_lut_kernel(1247, handle, 1 << 16) == b"k_uint_lut"
        knobs.set("uint_lut_fused", 0)
        assert hip.lib.csgn_uint_lut_kernel(1247, handle, 1 << 16) == b"composed"
        knobs.set("uint_lut_fused", 1)
        assert hip.lib.csgn_uint_lut_kernel(1247, handle, 1) == b"k_uint_lut"
        assert hip.lib.csgn_uint_lut_kernel(0, handle, 1) == b""
        assert hip.lib.csgn_uint_lut_kernel(1247, None, 1) == b""
    finally:
        hip.lib.csgn_uint_lut_destroy(handle)


def test_lut_argument_errors(hip):
    lib = hip.lib
    handle = C.c_void_p()
    assert lib.csgn_uint_lut_create(4, 3, u64s(list(range(16))), u64s([1] * 4), C.byref(handle)) == -1
    assert lib.csgn_uint_lut_create(17, 1, u64s([0] * (1 << 17)), u64s([1] * 17), C.byref(handle)) == -1
    assert lib.csgn_uint_lut_create(4, 1, u64s([0] * 15 + [1]), u64s([216] * 4), C.byref(handle)) == -2
    h = hip.uint_lut_create([1] + [0] * 65535, 16, 1, [1] * 16)    # 2^16 terms of one output
    t = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([t.data_ptr()] * 64))
    try:
        assert lib.csgn_uint_lut_apply(h, 0, 1, ptrs, ptrs, hip.stream) == -1
        assert lib.csgn_uint_lut_apply(None, 1247, 1, ptrs, ptrs, hip.stream) == -1
        assert lib.csgn_uint_lut_apply(h, 1247, 1, None, ptrs, hip.stream) == -1
        nullp = (C.c_void_p * 16)(*([t.data_ptr()] * 3 + [None] + [t.data_ptr()] * 12))
        assert lib.csgn_uint_lut_apply(h, 1247, 1, nullp, ptrs, hip.stream) == -1
        assert lib.csgn_uint_lut_apply(h, 1247, 1, ptrs, (C.c_void_p * 1)(None), hip.stream) == -1
        # 41^4 terms (every monomial over planes of 40 terms) * 2048 words per element pass 2^31 words
        big = hip.uint_lut_create([1] + [0] * 15, 4, 1, [40] * 4)
        try:
            assert lib.csgn_uint_lut_apply(big, 131072, 1, ptrs, ptrs, hip.stream) == -2
        finally:
            lib.csgn_uint_lut_destroy(big)
        assert lib.csgn_uint_lut_apply(h, 1247, 1 << 44, ptrs, ptrs, hip.stream) == -2
        assert lib.csgn_uint_lut_apply(h, 1247, 0, ptrs, ptrs, hip.stream) == 0       # empty batch
    finally:
        lib.csgn_uint_lut_destroy(h)
