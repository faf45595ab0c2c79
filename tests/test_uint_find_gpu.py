"""Encrypted tables looked up by encrypted key on the device (csgn_uint_find), word for word against the definition of
include/csgn_hip.h (pinned against the reference and the oracle in tests/test_uint_find_cpu.py), in both forms the knob
uint_find_form selects; decryptions; cross-checks against positional reads and gathers.  Run with `pytest -m gpu` on an
MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (GuardedOutputs, const_term, decrypt_bits, decrypt_value, encrypt_planes, hip, rand_terms, u64s)
from tests.model_find import find_terms, np_find_fast

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs: the numpy side, not the device, is the limit


def terms_of(planes):
    return [p.shape[1] for p in planes]


def run(hip, n, keys, query, values, member, want=None):
    """keys[k]: words[rows, u_k, dL], query[k]: words[batch, s_k, dL], values[j]: words[rows, t_j, dL] (host arrays).
    The outputs and member (last, when asked for), downloaded.  With `want` (the definition's words, one array per
    output) they are caller tensors of exactly those sizes between guard words, checked word for word and for writes
    outside them (tests/model.py, GuardedOutputs)."""
    dy = [hip.upload(p.ravel()) for p in keys]
    dx = [hip.upload(p.ravel()) for p in query]
    dv = [hip.upload(p.ravel()) for p in values]
    w = len(values)
    guarded = GuardedOutputs(hip, [x.size for x in want]) if want is not None else None
    outs, mem = hip.uint_find(n, query[0].shape[0], dx, terms_of(query), keys[0].shape[0], dy, terms_of(keys), dv,
                              terms_of(values), outs=guarded.outs[:w] if guarded else None,
                              member=(guarded.outs[w] if guarded else True) if member else False)
    torch.cuda.synchronize()
    if guarded:
        return guarded.check(want, (terms_of(keys), terms_of(query), keys[0].shape[0], w, member))
    return [hip.download(o) for o in outs] + ([hip.download(mem)] if member else [])


def definition(n, keys, query, values, member):
    outs, mem = np_find_fast(n, keys, query, values, member)
    return [x.ravel() for x in outs] + ([mem.ravel()] if member else [])


def check_forms(hip, knobs, n, keys, query, values, member, forms=(-1, 0, 1)):
    want = definition(n, keys, query, values, member)
    for form in forms:
        knobs.set("uint_find_form", form)
        run(hip, n, keys, query, values, member, want)          # GuardedOutputs.check asserts every word


def forms_for(rows, v, w):
    return (-1, 0, 1) if rows * (v + w + 3) <= 4096 else (-1, 1)


def term_counts(tmode, count, rng, fresh=False):
    """Terms of `count` planes: all 1 (the fresh path), all 2, or 1..3 drawn independently; "kfresh" is fresh keys
    (`fresh`) under a query that is not."""
    if tmode in ("1", "2"):
        return [int(tmode)] * count
    if tmode == "kfresh" and fresh:
        return [1] * count
    t = [int(x) for x in rng.integers(1, 4, count)]
    if tmode == "kfresh" and count:
        t[0] = max(t[0], 2)
    return t


# 63 and 129: odd dL, the 8-byte-unit kernel; 5 -> 6 planes: one -> two subset tables
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("v", [1, 2, 3, 5, 6, 8])
@pytest.mark.parametrize("tmode", ["1", "2", "mixed", "kfresh"])
def test_find_words(hip, knobs, n, v, tmode):
    rng = np.random.default_rng(v * 100 + n + len(tmode))
    batch, dl = 2, (n + 63) // 64
    u, s = term_counts(tmode, v, rng, fresh=True), term_counts(tmode, v, rng)
    P = find_terms(u, s)
    query = [rand_terms(n, batch, sk, 400 + 7 * k + sk) for k, sk in enumerate(s)]
    ran = 0
    for rows in (1, 2, 7, 33):
        keys = [rand_terms(n, rows, uk, 450 + 5 * k + rows) for k, uk in enumerate(u)]
        for w in (0, 1, 8, 64):
            t = term_counts("mixed" if tmode == "kfresh" else tmode, w, rng)
            values = [rand_terms(n, rows, tj, 500 + 11 * j + rows) for j, tj in enumerate(t)]
            for member in (True, False) if w else (True,):
                if batch * rows * P * (sum(t) + member) * dl * 8 > MAX_BYTES:
                    continue
                check_forms(hip, knobs, n, keys, query, values, member, forms_for(rows, v, w))
                ran += 1
    # the smallest call, one row and member alone, is the only thing the 48 MB rule may leave nothing of
    assert ran or batch * P * dl * 8 > MAX_BYTES


@pytest.mark.parametrize("batch", [1, 257, 4099, (1 << 16) + 3])
def test_find_batches(hip, knobs, batch):
    """Partial last element groups and many groups a launch, in every form (every batch here is ONE launch of the fused
    kernel; the launches launch_groups cuts a batch into run in tests/test_launch_split_gpu.py).  The largest batch
    writes one value plane (1.1 GB at 13 * 81 terms an element) without member; the others two planes and member."""
    n, v, rows = 65, 4, 13
    keys = [rand_terms(n, rows, 1, 700 + k) for k in range(v)]
    query = [rand_terms(n, batch, 1, 720 + k) for k in range(v)]
    values = [rand_terms(n, rows, 1 + j, 740 + j) for j in range(1 if batch > 5000 else 2)]
    check_forms(hip, knobs, n, keys, query, values, batch <= 5000)


@pytest.mark.parametrize("n", [1247, 4096])
def test_find_three_subset_tables_and_unit_slices(hip, knobs, n):
    """11 planes: three subset tables a set, one slice of units at either N: at N=4096 (32 units of 16 bytes a term) a
    set's tables of one element at whole terms take 40 x 16 x 32 = 20 480 B, not past the kernel's 20 480-byte budget."""
    v, rows, batch = 11, 2, 1
    keys = [rand_terms(n, rows, 1, 900 + k) for k in range(v)]
    query = [rand_terms(n, batch, 1, 930 + k) for k in range(v)]
    values = [rand_terms(n, rows, 1, 960)]
    check_forms(hip, knobs, n, keys, query, values, False, (1,))


@pytest.mark.parametrize("n", [5248, 5184])
def test_find_short_last_unit_slice(hip, knobs, n):
    """v = 5: one subset table of 32 entries a set.  N = 5248 is 41 units of 16 bytes a term: 32 x 16 x 41 = 20 992 B
    pass the kernel's 20 480-byte budget, so subset_plan cuts the terms into two slices of 21 units, the last one 20
    units long.  N = 5184 (81 words, odd) is 81 units of 8 bytes: 32 x 8 x 81 = 20 736 B, slices of 41 and 40 units.
    Value planes of 1 and 2 terms, and member."""
    v, rows, batch = 5, 3, 2
    keys = [rand_terms(n, rows, 1, 1100 + k) for k in range(v)]
    query = [rand_terms(n, batch, 1, 1130 + k) for k in range(v)]
    values = [rand_terms(n, rows, tj, 1160 + j) for j, tj in enumerate((1, 2))]
    check_forms(hip, knobs, n, keys, query, values, True, (-1, 1))


def test_find_many_rows(hip, knobs):
    """The row range is split over many workgroups."""
    n, v, rows, w, batch = 1247, 2, 5000, 2, 3
    keys = [rand_terms(n, rows, 1, 1000 + k) for k in range(v)]
    query = [rand_terms(n, batch, 1, 1010 + k) for k in range(v)]
    values = [rand_terms(n, rows, 1, 1020 + j) for j in range(w)]
    check_forms(hip, knobs, n, keys, query, values, True, (-1, 1))


@pytest.mark.parametrize("n", [63, 1247])
@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_find_rows_split_over_launches(hip, knobs, n, tmode):
    """A table with more row parts than one launch takes is cut into row ranges on the host, each launch with its own
    key, value and output offsets.  No shape that fits memory gets there by itself (16 M workgroups a query group), so
    knob uint_find_rparts lowers the limit: 1, 2 and 5 row parts a launch, a last launch that is not full, both unit
    sizes, the fresh and the multi-term path, with member."""
    rng = np.random.default_rng(n + len(tmode))
    v, rows, batch = 2, 37, 3
    u, s, t = term_counts(tmode, v, rng), term_counts(tmode, v, rng), term_counts(tmode, 3, rng)
    keys = [rand_terms(n, rows, uk, 1100 + k) for k, uk in enumerate(u)]
    query = [rand_terms(n, batch, sk, 1110 + k) for k, sk in enumerate(s)]
    values = [rand_terms(n, rows, tj, 1120 + j) for j, tj in enumerate(t)]
    for rparts in (1, 2, 5):
        knobs.set("uint_find_rparts", rparts)
        check_forms(hip, knobs, n, keys, query, values, True, (1,))


def encrypted_table(oracle, n, key, ks, vals, v, w, seed):
    rows = len(ks)
    keys = [p.reshape(rows, 1, -1) for p in encrypt_planes(oracle, n, key, ks, v, seed)]
    values = [p.reshape(rows, 1, -1) for p in encrypt_planes(oracle, n, key, vals, w, seed + 1)]
    return keys, values


def decrypted(oracle, n, key, outs, batch):
    dl = (n + 63) // 64
    return [o.reshape(batch, -1, dl) for o in outs]


def test_find_decrypts(hip, knobs, oracle):
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(601, 64 * d + 64))
    rng = np.random.default_rng(602)
    knobs.unset("uint_find_form")
    for v, rows, w, batch in [(1, 2, 3, 5), (3, 6, 4, 100), (4, 11, 8, 333), (8, 40, 8, 16)]:
        ks = rng.permutation(1 << v)[:rows].astype(np.uint64)                   # distinct
        vals = rng.integers(0, 1 << w, rows).astype(np.uint64)
        xs = np.concatenate([np.arange(min(1 << v, batch)), rng.integers(0, 1 << v, max(0, batch - (1 << v)))])
        xs = xs.astype(np.uint64)
        if v == 8:
            xs[::2] = ks[rng.integers(0, rows, len(xs[::2]))]                   # half of them present
        keys, values = encrypted_table(oracle, n, key, ks, vals, v, w, 610 + 2 * v)
        query = encrypt_planes(oracle, n, key, xs, v, 630 + v)
        outs = decrypted(oracle, n, key, run(hip, n, keys, query, values, True), batch)
        table = {int(k): int(x) for k, x in zip(ks, vals)}
        assert [int(g) for g in decrypt_value(oracle, n, key, outs[:w])] == [table.get(int(x), 0) for x in xs], (v, rows)
        assert [int(b) for b in decrypt_bits(oracle, n, key, outs[w])] == [int(int(x) in table) for x in xs], (v, rows)
        assert any(int(x) not in table for x in xs) or rows == 1 << v


def test_trivial_keys_match_positional_read(hip, knobs, oracle):
    """Trivially encrypted keys 0..rows-1 (one ONE / ZERO term per bit) give what uint_read gives on the same table
    and index."""
    n, d, v, w, rows, batch = 1247, 16, 5, 4, 20, 64
    key, _ = oracle.keygen(n, d, glibc_draws(641, 64 * d + 64))
    rng = np.random.default_rng(642)
    xs = np.concatenate([np.arange(32), rng.integers(0, 32, batch - 32)]).astype(np.uint64)
    vals = rng.integers(0, 1 << w, rows).astype(np.uint64)
    keys = [np.stack([const_term(n, (r >> k) & 1) for r in range(rows)]).reshape(rows, 1, -1) for k in range(v)]
    values = [p.reshape(rows, 1, -1) for p in encrypt_planes(oracle, n, key, vals, w, 643)]
    query = encrypt_planes(oracle, n, key, xs, v, 644)
    knobs.unset("uint_find_form")
    knobs.unset("uint_read_fused")
    got = decrypt_value(oracle, n, key, decrypted(oracle, n, key, run(hip, n, keys, query, values, False), batch))
    dx = [hip.upload(p.ravel()) for p in query]
    dv = [hip.upload(p.ravel()) for p in values]
    routs = hip.uint_read(n, batch, dx, [1] * v, rows, dv, [1] * w)
    torch.cuda.synchronize()
    via_read = decrypt_value(oracle, n, key, decrypted(oracle, n, key, [hip.download(o) for o in routs], batch))
    assert np.array_equal(got, via_read)
    assert [int(g) for g in got] == [int(vals[x]) if x < rows else 0 for x in xs]


def test_trivial_queries_match_gather(hip, knobs, oracle):
    """Trivially encrypted queries give what a gather of the matching rows gives."""
    n, d, v, w, rows, batch = 1247, 16, 5, 5, 24, 100
    key, _ = oracle.keygen(n, d, glibc_draws(651, 64 * d + 64))
    rng = np.random.default_rng(652)
    ks = rng.permutation(1 << v)[:rows].astype(np.uint64)
    vals = rng.integers(0, 1 << w, rows).astype(np.uint64)
    idx = rng.integers(0, rows, batch).astype(np.uint64)              # the row every query matches
    keys, values = encrypted_table(oracle, n, key, ks, vals, v, w, 653)
    query = [np.stack([const_term(n, (int(ks[i]) >> k) & 1) for i in idx]).reshape(batch, 1, -1) for k in range(v)]
    knobs.unset("uint_find_form")
    got = decrypt_value(oracle, n, key, decrypted(oracle, n, key, run(hip, n, keys, query, values, False), batch))
    dv = [hip.upload(p.ravel()) for p in values]
    gouts = hip.gather_planes(n, dv, [1] * w, rows, batch, hip.upload(idx))
    torch.cuda.synchronize()
    via_gather = decrypt_value(oracle, n, key, decrypted(oracle, n, key, [hip.download(o) for o in gouts], batch))
    assert np.array_equal(got, via_gather)
    assert np.array_equal(got, vals[idx])


def test_find_graph_capture_and_replay(hip, knobs):
    n, v, rows, w, batch = 1247, 6, 20, 4, 37
    keys = [rand_terms(n, rows, 1, 1300 + k) for k in range(v)]
    query = [rand_terms(n, batch, 1, 1320 + k) for k in range(v)]
    values = [rand_terms(n, rows, 1 + j % 2, 1400 + j) for j in range(w)]
    t = terms_of(values)
    want = definition(n, keys, query, values, True)
    knobs.set("uint_find_form", 1)
    dy = [hip.upload(p.ravel()) for p in keys]
    dx = [hip.upload(p.ravel()) for p in query]
    dv = [hip.upload(p.ravel()) for p in values]
    outs = [hip.empty_words(x.size) for x in want]
    one = u64s([1] * v)
    assert hip.lib.csgn_uint_find_kernel(n, batch, v, one, one, rows, w, u64s(t), 1) == b"k_uint_find"
    call = lambda: hip.uint_find(n, batch, dx, [1] * v, rows, dy, [1] * v, dv, t, outs=outs[:w], member=outs[w])  # noqa: E731
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()                                                        # warm-up outside the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for j in range(w + 1):
        assert np.array_equal(hip.download(outs[j]), want[j]), j


def test_find_dispatch_names(hip, knobs):
    lib = hip.lib
    one = u64s([1] * 16)

    def name(v, rows, w, member=0):
        return lib.csgn_uint_find_kernel(1247, 64, v, one, one, rows, w, one, member)

    knobs.unset("uint_find_form")
    for v, rows, w in [(4, 16, 8), (8, 16, 8), (8, 256, 1), (2, 1024, 8)]:
        assert name(v, rows, w) == b"k_uint_find"
    knobs.set("uint_find_form", 0)
    assert name(4, 16, 8) == b"composed" and name(2, 5, 0, 1) == b"composed"
    knobs.set("uint_find_form", 1)
    assert name(4, 16, 8) == b"k_uint_find" and name(4, 16, 0) == b"" and name(4, 0, 1) == b""


def test_find_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    mem = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([buf.data_ptr()] * 64))
    nullp = (C.c_void_p * 64)(*([buf.data_ptr()] * 3 + [None] + [buf.data_ptr()] * 60))
    one = u64s([1] * 64)
    st = hip.stream

    def find(n=1247, batch=1, v=4, x=ptrs, s=one, rows=16, y=ptrs, u=one, w=4, d=ptrs, t=one, out=ptrs, member=None):
        return lib.csgn_uint_find(n, batch, v, x, s, rows, y, u, w, d, t, out, member, st)

    assert find(n=0) == -1                                            # n_bits
    assert find(v=0) == -1 and find(v=17) == -1                       # key width
    assert find(w=65) == -1 and find(w=0) == -1                       # value width; width 0 without member
    assert find(rows=0) == -1                                         # rows
    for arg in ("x", "s", "y", "u", "d", "t", "out"):                 # host pointers
        assert find(**{arg: None}) == -1, arg
    assert find(u=u64s([1, 0, 1, 1])) == -1 and find(s=u64s([1, 1, 1, 0])) == -1   # 0 terms
    assert find(t=u64s([1, 0, 1, 1])) == -1
    assert find(u=u64s([1 << 16] * 4), s=u64s([1 << 16] * 4)) == -1   # 2^62
    for arg in ("x", "y", "d", "out"):                                # a null device pointer inside each host array
        assert find(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert find(v=16, rows=3, w=1) == -2                              # 2^31 words
    assert find(v=16, rows=1, w=1, t=u64s([3])) == -2
    assert find(v=16, rows=1, w=0, member=mem.data_ptr(), u=u64s([2] * 16)) == -2
    assert find(v=8, batch=1 << 44) == -2                             # batch
    assert find(batch=0) == 0                                         # empty batch
    assert find(batch=0, x=nullp, y=nullp, d=nullp, out=nullp) == 0
    assert find(batch=0, w=0, d=None, t=None, out=None, member=mem.data_ptr()) == 0
