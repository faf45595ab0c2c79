"""Encrypted tables read at encrypted indices on the device (csgn_uint_read), word for word against the definition of
include/csgn_hip.h (pinned against the reference and the oracle in tests/test_uint_read_cpu.py), in both forms the knob
uint_read_fused selects; decryptions; cross-checks against lookup tables and gathers.  Run with `pytest -m gpu` on an
MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (GuardedOutputs, const_term, decrypt_value, encrypt_planes, hip, np_read_fast, rand_terms,
                         read_terms, u64s)

pytestmark = pytest.mark.gpu


def run(hip, n, index, table, want=None):
    """index[k]: words[batch, s_k, dL], table[j]: words[rows, t_j, dL] (host arrays).  The outputs, downloaded.  With
    `want` (the definition's words, one array per output) they are caller tensors of exactly those sizes between guard
    words, checked word for word and for writes outside them (tests/model.py, GuardedOutputs)."""
    dx = [hip.upload(p.ravel()) for p in index]
    dt = [hip.upload(p.ravel()) for p in table]
    guarded = GuardedOutputs(hip, [x.size for x in want]) if want is not None else None
    outs = hip.uint_read(n, index[0].shape[0], dx, [p.shape[1] for p in index], table[0].shape[0], dt,
                         [p.shape[1] for p in table], outs=guarded.outs if guarded else None)
    torch.cuda.synchronize()
    return guarded.check(want, table[0].shape[0]) if guarded else [hip.download(o) for o in outs]


def check_forms(hip, knobs, n, index, table, forms=(-1, 0, 1)):
    want = [x.ravel() for x in np_read_fast(n, index, table)]
    for fused in forms:
        knobs.set("uint_read_fused", fused)
        got = run(hip, n, index, table, want)
        for j in range(len(table)):
            assert np.array_equal(got[j], want[j]), (fused, j, [p.shape[1] for p in index], table[0].shape[0])


def term_counts(tmode, count, rng):
    if tmode == "mixed":
        return [int(x) for x in rng.integers(1, 4, count)]
    return [int(tmode)] * count


# 63 and 129: odd dL, the 8-byte-unit kernel
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("v", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("tmode", ["1", "2", "3", "mixed"])
def test_read_words(hip, knobs, n, v, tmode):
    rng = np.random.default_rng(v * 100 + n + len(tmode))
    s = term_counts(tmode, v, rng)
    if v == 8 and tmode != "1":
        s = s[:2] + [1] * 6                                           # at most 49 * 3^6 entries
    batch, dl = 2, (n + 63) // 64
    index = [rand_terms(n, batch, sk, 400 + 7 * k + sk) for k, sk in enumerate(s)]
    partial = int(rng.integers(1, (1 << v) + 1))
    for rows in sorted({1, (1 << v) - 1, 1 << v, partial} - {0}):
        E = read_terms(s, rows)
        for w in (1, 8, 64):
            t = term_counts(tmode, w, rng)
            if batch * sum(t) * E * dl * 8 > (48 << 20):
                continue                                              # the numpy side, not the device, is the limit
            table = [rand_terms(n, rows, tj, 500 + 11 * j + rows) for j, tj in enumerate(t)]
            forms = (-1, 0, 1) if rows * (w + 2) <= 4096 else (-1, 1)
            check_forms(hip, knobs, n, index, table, forms)


@pytest.mark.parametrize("batch", [1, 257, 4099, (1 << 16) + 3])
@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_read_batches(hip, knobs, batch, tmode):
    n, v, rows = 65, 4, 13
    s = [1] * v if tmode == "1" else [1, 2, 1, 3]
    t = [1, 1, 1] if tmode == "1" else [2, 1, 3]
    index = [rand_terms(n, batch, sk, 700 + k) for k, sk in enumerate(s)]
    table = [rand_terms(n, rows, tj, 710 + j) for j, tj in enumerate(t)]
    check_forms(hip, knobs, n, index, table, (-1, 1) if batch > 5000 else (-1, 0, 1))


@pytest.mark.parametrize("v,rows,w,batch", [(10, 1024, 1, 3), (12, 4096, 1, 1), (12, 3000, 2, 1)])
@pytest.mark.parametrize("n", [1247, 4096])
def test_read_wide_indices_span_many_workgroups(hip, knobs, v, rows, w, batch, n):
    """Two (v = 10) and three (v = 12) subset tables, one slice of units at either N: at N=4096 (32 units of 16 bytes a
    term) the tables of one element at whole terms take 64 x 16 x 32 = 32 768 B and 48 x 16 x 32 = 24 576 B, neither
    past the kernel's 32 768-byte budget."""
    index = [rand_terms(n, batch, 1, 900 + k) for k in range(v)]
    table = [rand_terms(n, rows, 1, 950 + j) for j in range(w)]
    check_forms(hip, knobs, n, index, table, (1,))


@pytest.mark.parametrize("n", [8320, 8256])
def test_read_short_last_unit_slice(hip, knobs, n):
    """v = 5: one subset table of 32 entries.  N = 8320 is 65 units of 16 bytes a term: 32 x 16 x 65 = 33 280 B pass the
    kernel's 32 768-byte budget, so subset_plan cuts the terms into two slices of 33 units, the last one 32 units long.
    N = 8256 (129 words, odd) is 129 units of 8 bytes: 32 x 8 x 129 = 33 024 B, slices of 65 and 64 units.  All 32 rows
    and a partial last row; table planes of 1 and 2 terms."""
    v, batch = 5, 2
    index = [rand_terms(n, batch, 1, 1100 + k) for k in range(v)]
    for rows in (32, 19):
        table = [rand_terms(n, rows, tj, 1150 + j + rows) for j, tj in enumerate((1, 2))]
        check_forms(hip, knobs, n, index, table, (-1, 1))


def test_read_decrypts(hip, knobs, oracle):
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(601, 64 * d + 64))
    rng = np.random.default_rng(602)
    knobs.unset("uint_read_fused")
    for v, rows, w, batch in [(1, 2, 3, 5), (3, 6, 4, 100), (4, 16, 8, 333), (5, 20, 2, 1000), (8, 256, 8, 64)]:
        xs = np.concatenate([np.arange(min(1 << v, batch)), rng.integers(0, 1 << v, max(0, batch - (1 << v)))])
        xs = xs.astype(np.uint64)
        values = rng.integers(0, 1 << w, rows).astype(np.uint64)
        index = encrypt_planes(oracle, n, key, xs, v, 610 + v)
        table = [p.reshape(rows, 1, -1) for p in encrypt_planes(oracle, n, key, values, w, 620 + v)]
        outs = run(hip, n, index, table)
        dl = (n + 63) // 64
        got = decrypt_value(oracle, n, key, [o.reshape(batch, -1, dl) for o in outs])
        want = [int(values[x]) if x < rows else 0 for x in xs]
        assert [int(g) for g in got] == want, (v, rows, w, batch)


def test_constant_table_matches_lookup(hip, knobs, oracle):
    """A trivially encrypted table (UIntBatch::constant: one ONE / ZERO term per bit) read at encrypted x decrypts to
    what lookup(x, f) of the same table does."""
    n, d, v, w, batch = 1247, 16, 8, 8, 300
    key, _ = oracle.keygen(n, d, glibc_draws(631, 64 * d + 64))
    rng = np.random.default_rng(632)
    xs = np.concatenate([np.arange(256), rng.integers(0, 256, batch - 256)]).astype(np.uint64)
    index = encrypt_planes(oracle, n, key, xs, v, 633)
    f = [int(x) for x in rng.integers(0, 256, 256)]
    table = [np.stack([const_term(n, (f[r] >> j) & 1) for r in range(256)]).reshape(256, 1, -1) for j in range(w)]
    knobs.unset("uint_read_fused")
    knobs.unset("uint_lut_fused")
    outs = run(hip, n, index, table)
    dx = [hip.upload(p.ravel()) for p in index]
    louts = [hip.download(o) for o in hip.uint_lut(n, batch, dx, [1] * v, f, w)]
    dl = (n + 63) // 64
    got = decrypt_value(oracle, n, key, [o.reshape(batch, -1, dl) for o in outs])
    via_lut = decrypt_value(oracle, n, key, [o.reshape(batch, -1, dl) for o in louts])
    assert np.array_equal(got, via_lut)
    assert [int(g) for g in got] == [f[int(x)] for x in xs]


def test_trivial_index_matches_gather(hip, knobs, oracle):
    """An encrypted table read at trivially encrypted indices decrypts to what a gather of those indices does."""
    n, d, v, w, rows, batch = 1247, 16, 6, 5, 50, 200
    key, _ = oracle.keygen(n, d, glibc_draws(641, 64 * d + 64))
    rng = np.random.default_rng(642)
    idx = rng.integers(0, rows, batch).astype(np.uint64)
    index = [np.stack([const_term(n, (int(x) >> k) & 1) for x in idx]).reshape(batch, 1, -1) for k in range(v)]
    values = rng.integers(0, 1 << w, rows).astype(np.uint64)
    table = [p.reshape(rows, 1, -1) for p in encrypt_planes(oracle, n, key, values, w, 643)]
    knobs.unset("uint_read_fused")
    outs = run(hip, n, index, table)
    dt = [hip.upload(p.ravel()) for p in table]
    gouts = hip.gather_planes(n, dt, [1] * w, rows, batch, hip.upload(idx))
    torch.cuda.synchronize()
    dl = (n + 63) // 64
    got = decrypt_value(oracle, n, key, [o.reshape(batch, -1, dl) for o in outs])
    via_gather = decrypt_value(oracle, n, key, [hip.download(o).reshape(batch, -1, dl) for o in gouts])
    assert np.array_equal(got, via_gather)
    assert np.array_equal(got, values[idx])


def test_read_output_past_4_gib(hip, knobs):
    """One call of about 4.3 GB in ONE output plane (8-bit index, 256 rows, 4096 elements at N=1247): offsets pass 2^32
    bytes.  Elements at both ends and inside are compared with the definition."""
    n, v, rows, batch = 1247, 8, 256, 4096
    dl = (n + 63) // 64
    E = 3 ** v
    assert batch * E * dl * 8 > 1 << 32
    index = [rand_terms(n, batch, 1, 1100 + k) for k in range(v)]
    table = [rand_terms(n, rows, 1, 1200)]
    knobs.set("uint_read_fused", 1)
    dx = [hip.upload(p.ravel()) for p in index]
    dt = [hip.upload(p.ravel()) for p in table]
    out = hip.uint_read(n, batch, dx, [1] * v, rows, dt, [1])[0]
    torch.cuda.synchronize()
    per = E * dl
    for e in (0, 1, 1000, 2047, 3333, batch - 2, batch - 1):
        want = np_read_fast(n, [p[e:e + 1] for p in index], table)[0].ravel()
        got = hip.download(out[e * per:(e + 1) * per])
        assert np.array_equal(got, want), e
    del out
    torch.cuda.empty_cache()


def test_read_graph_capture_and_replay(hip, knobs):
    n, v, rows, w, batch = 1247, 8, 200, 8, 37
    index = [rand_terms(n, batch, 1, 1300 + k) for k in range(v)]
    table = [rand_terms(n, rows, 1 + j % 2, 1400 + j) for j in range(w)]
    t = [p.shape[1] for p in table]
    want = [x.ravel() for x in np_read_fast(n, index, table)]
    knobs.set("uint_read_fused", 1)
    dx = [hip.upload(p.ravel()) for p in index]
    dt = [hip.upload(p.ravel()) for p in table]
    E = read_terms([1] * v, rows)
    dl = (n + 63) // 64
    outs = [hip.empty_words(batch * tj * E * dl) for tj in t]
    assert hip.lib.csgn_uint_read_kernel(n, batch, v, u64s([1] * v), rows, w, u64s(t)) == b"k_uint_read"
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hip.uint_read(n, batch, dx, [1] * v, rows, dt, t, outs)           # warm-up outside the capture
    s.synchronize()
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        hip.uint_read(n, batch, dx, [1] * v, rows, dt, t, outs)
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for j in range(w):
        assert np.array_equal(hip.download(outs[j]), want[j]), j


def test_read_dispatch_names(hip, knobs):
    lib = hip.lib

    def name(batch, v, s, rows, w, t):
        return lib.csgn_uint_read_kernel(1247, batch, v, u64s(s), rows, w, u64s(t))

    knobs.unset("uint_read_fused")
    assert name(1 << 16, 8, [1] * 8, 256, 8, [1] * 8) == b"k_uint_read"
    assert name(1, 2, [3, 1], 3, 64, [2] * 64) == b"k_uint_read"
    knobs.set("uint_read_fused", 0)
    assert name(1 << 16, 8, [1] * 8, 256, 8, [1] * 8) == b"composed"
    knobs.set("uint_read_fused", 1)
    assert name(1, 1, [1], 1, 1, [1]) == b"k_uint_read"
    assert name(1, 1, [1], 3, 1, [1]) == b""
    assert lib.csgn_uint_read_kernel(0, 1, 1, u64s([1]), 1, 1, u64s([1])) == b""


def test_read_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([buf.data_ptr()] * 64))
    one = u64s([1] * 64)
    st = hip.stream
    assert lib.csgn_uint_read(0, 1, 4, ptrs, one, 16, 1, ptrs, one, ptrs, st) == -1           # n_bits
    assert lib.csgn_uint_read(1247, 1, 0, ptrs, one, 1, 1, ptrs, one, ptrs, st) == -1         # index width
    assert lib.csgn_uint_read(1247, 1, 17, ptrs, one, 1, 1, ptrs, one, ptrs, st) == -1
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 0, 1, ptrs, one, ptrs, st) == -1         # rows
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 17, 1, ptrs, one, ptrs, st) == -1
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 16, 0, ptrs, one, ptrs, st) == -1        # table width
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 16, 65, ptrs, one, ptrs, st) == -1
    assert lib.csgn_uint_read(1247, 1, 4, None, one, 16, 1, ptrs, one, ptrs, st) == -1        # host pointers
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, None, 16, 1, ptrs, one, ptrs, st) == -1
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 16, 1, None, one, ptrs, st) == -1
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 16, 1, ptrs, None, ptrs, st) == -1
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 16, 1, ptrs, one, None, st) == -1
    assert lib.csgn_uint_read(1247, 1, 3, ptrs, u64s([1, 0, 1]), 8, 1, ptrs, one, ptrs, st) == -1   # 0 terms
    assert lib.csgn_uint_read(1247, 1, 3, ptrs, one, 8, 2, ptrs, u64s([1, 0]), ptrs, st) == -1
    nullp = (C.c_void_p * 64)(*([buf.data_ptr()] * 3 + [None] + [buf.data_ptr()] * 60))
    assert lib.csgn_uint_read(1247, 1, 4, nullp, one, 16, 1, ptrs, one, ptrs, st) == -1       # device pointers
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 16, 4, nullp, one, ptrs, st) == -1
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, one, 16, 4, ptrs, one, nullp, st) == -1
    assert lib.csgn_uint_read(1247, 1, 16, ptrs, one, 1 << 16, 1, ptrs, u64s([3]), ptrs, st) == -2   # 2^31 words
    assert lib.csgn_uint_read(1247, 1, 16, ptrs, u64s([2] * 16), 1 << 16, 1, ptrs, one, ptrs, st) == -2
    assert lib.csgn_uint_read(1247, 1, 4, ptrs, u64s([1 << 16] * 4), 16, 1, ptrs, one, ptrs, st) == -1  # 2^62
    assert lib.csgn_uint_read(1247, 1 << 44, 8, ptrs, one, 256, 8, ptrs, one, ptrs, st) == -2  # batch
    assert lib.csgn_uint_read(1247, 0, 4, ptrs, one, 16, 1, ptrs, one, ptrs, st) == 0         # empty batch
    assert lib.csgn_uint_read(1247, 0, 4, nullp, one, 16, 1, nullp, one, nullp, st) == 0
