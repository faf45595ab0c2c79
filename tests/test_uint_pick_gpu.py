"""Shifts, rotates and per-element reads by encrypted amounts on the device (csgn_uint_pick), word for word against the
definition of include/csgn_hip.h (tests/model_pick.py, pinned against the reference and the oracle in
tests/test_uint_pick_cpu.py), in both forms the knob uint_pick_fused selects; decryptions of every distance;
cross-checks against public lookup tables, shared-table reads and the public-distance semantics; graph capture.  Run
with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (GuardedOutputs, const_term, decrypt_value, encrypt_planes, hip, np_read_fast, rand_terms,  # noqa: F401
                         u64s)
from tests.model_pick import (EACH, OPS, ROTL, ROTR, SHIFTS, SHL, SHR, clear_pick, np_pick_fast, pick_terms, rows_max)

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs: the numpy side, not the device, is the limit


def run(hip, n_bits, op, index, a, n=0, want=None):
    """index[k]: words[batch, s_k, dL], a[j]: words[batch (* n), t, dL] (host arrays).  The outputs, downloaded.  With
    `want` (the definition's words, one array per output) they are caller tensors of exactly those sizes between guard
    words, checked word for word and for writes outside them (tests/model.py, GuardedOutputs)."""
    dx = [hip.upload(p.ravel()) for p in index]
    da = [hip.upload(p.ravel()) for p in a]
    guarded = GuardedOutputs(hip, [x.size for x in want]) if want is not None else None
    outs = hip.uint_pick(n_bits, op, index[0].shape[0], dx, [p.shape[1] for p in index], da, a[0].shape[1], n,
                         outs=guarded.outs if guarded else None)
    torch.cuda.synchronize()
    what = (op, [p.shape[1] for p in index], len(a), n, a[0].shape[1])
    return guarded.check(want, what) if guarded else [hip.download(o) for o in outs]


def check_forms(hip, knobs, n_bits, op, index, a, n=0, forms=(-1, 0, 1)):
    want = [x.ravel() for x in np_pick_fast(n_bits, op, index, a, n)]
    for fused in forms:
        knobs.set("uint_pick_fused", fused)
        for stage in ((-1,) if fused == 0 else (0, 1)):                # the fused kernel with and without its LDS value slice
            knobs.set("uint_pick_stage", stage)
            run(hip, n_bits, op, index, a, n, want)                    # GuardedOutputs.check asserts every word
    return want


def out_bytes(n_bits, op, s, w, n, t, batch):
    dl = (n_bits + 63) // 64
    return batch * t * sum(pick_terms(op, s, w, n, j) for j in range(w)) * dl * 8


def operands(n_bits, op, s, w, n, t, batch, seed):
    index = [rand_terms(n_bits, batch, sk, seed + 7 * k + sk) for k, sk in enumerate(s)]
    a = [rand_terms(n_bits, batch * (n if op == EACH else 1), t, seed + 100 + 11 * j) for j in range(w)]
    return index, a


def mixed_terms(v, rng):
    return [int(x) for x in rng.integers(1, 4, v)]


# 63 and 129: odd dL, the 8-byte-unit kernel
@pytest.mark.parametrize("n_bits", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("v,w", [(1, 1), (1, 3), (2, 3), (2, 4), (3, 5), (3, 8), (3, 13), (4, 16), (6, 64)])
@pytest.mark.parametrize("op", sorted(OPS))
def test_pick_words(hip, knobs, n_bits, v, w, op):
    """Source planes of 1 and 3 terms under fresh and mixed (1..3 terms) distance planes; (6, 64) with fresh planes
    only.  A call whose outputs pass 48 MB is skipped: the numpy side, not the device, is the limit."""
    op = OPS[op]
    rng = np.random.default_rng(100 * v + w + n_bits)
    n = int(rng.integers(1, (1 << v) + 1)) if op == EACH else 0
    ran = 0
    for t in (1, 3):
        for s in ([1] * v, mixed_terms(v, rng)):
            if (v, w) == (6, 64) and (t != 1 or s != [1] * v):
                continue
            if out_bytes(n_bits, op, s, w, n, t, 2) > MAX_BYTES:
                continue
            index, a = operands(n_bits, op, s, w, n, t, 2, 300 + t)
            check_forms(hip, knobs, n_bits, op, index, a, n)
            ran += 1
    assert ran, "nothing ran"


EACH_BATCH = 3


def each_cases(v, w):
    """(n_bits, n, t, s) of test_pick_each_rows at (v, w): arrays of 1, 2^v - 1, 2^v and a random number of rows, fresh
    one-term planes and planes of 2 terms under a mixed index, at N = 1247 and 65, less the calls past 48 MB."""
    partial = int(np.random.default_rng(v).integers(1, (1 << v) + 1))
    return [(n_bits, n, t, s) for n in sorted({1, (1 << v) - 1, 1 << v, partial} - {0}) for n_bits in (1247, 65)
            for t, s in ((1, [1] * v), (2, ([2, 3] + [1] * v)[:v]))
            if out_bytes(n_bits, EACH, s, w, n, t, EACH_BATCH) <= MAX_BYTES]


@pytest.mark.parametrize("v", [1, 3, 4, 8])
@pytest.mark.parametrize("w", [1, 8, 64])
def test_pick_each_rows(hip, knobs, v, w):
    cases = each_cases(v, w)
    for n in {1, (1 << v) - 1, 1 << v} - {0}:
        assert any(c[1] == n for c in cases), ("no case ran with this many rows", n)
    for n_bits, n, t, s in cases:
        index, a = operands(n_bits, EACH, s, w, n, t, EACH_BATCH, 500 + n)
        check_forms(hip, knobs, n_bits, EACH, index, a, n)


def test_pick_each_rows_cover_one_part_and_several(hip):
    """What the (v, n) pairs of test_pick_each_rows are chosen for, from the fused form's own tile
    (csgn_uint_pick_plan): an element's stream of E entries is cut into parts of QP entries, one workgroup's decoded range
    each.  The cases hold a stream that is one part, a stream that spans several parts with the last one short -- the
    element's array ends inside that workgroup's range -- and workgroups that own several elements."""
    plan = (C.c_uint64 * 4)()
    seen = set()
    for v in (1, 3, 4, 8):
        for w in (1, 8, 64):
            for n_bits, n, t, s in each_cases(v, w):
                assert hip.lib.csgn_uint_pick_plan(n_bits, EACH, EACH_BATCH, v, u64s(s), w, n, t, 1, plan) == 0
                QP, parts = int(plan[2]), int(plan[3])
                E = pick_terms(EACH, s, w, n, 0)
                assert (parts - 1) * QP < E <= parts * QP
                seen.add("one" if parts == 1 else "short last" if E % QP else "even")
                if int(plan[0]) > 1:
                    seen.add("several elements")
    assert {"one", "short last", "several elements"} <= seen, seen


@pytest.mark.parametrize("batch", [1, 257, 4099, (1 << 16) + 3])
@pytest.mark.parametrize("tmode", ["1", "mixed"])
@pytest.mark.parametrize("op", ["shl", "each"])
def test_pick_batches(hip, knobs, batch, tmode, op):
    n_bits, v, w = 65, 2, 3
    op = OPS[op]
    s, t = ([1, 1], 1) if tmode == "1" else ([1, 2], 2)
    n = 3 if op == EACH else 0
    index, a = operands(n_bits, op, s, w, n, t, batch, 700)
    check_forms(hip, knobs, n_bits, op, index, a, n)


@pytest.mark.parametrize("n_bits,tmode", [(63, "1"), (1247, "1"), (1247, "mixed")])
@pytest.mark.parametrize("op", ["rotl", "each"])
def test_pick_batch_split_over_launches(hip, knobs, n_bits, tmode, op):
    """Knob launch_blocks lowers the workgroups of one launch, so launch_groups cuts the batch into several launches,
    each with its own index, source and output offsets (EACH: the sources advance by e0 * n elements); a last launch
    that is not full."""
    op = OPS[op]
    v, w, batch = 3, 5, 37
    s, t = ([1] * v, 1) if tmode == "1" else ([2, 1, 3], 2)
    n = 6 if op == EACH else 0
    index, a = operands(n_bits, op, s, w, n, t, batch, 800)
    want = [x.ravel() for x in np_pick_fast(n_bits, op, index, a, n)]
    knobs.set("uint_pick_fused", 1)
    for blocks in (1, 3, 7):
        knobs.set("launch_blocks", blocks)
        for stage in (0, 1):
            knobs.set("uint_pick_stage", stage)
            run(hip, n_bits, op, index, a, n, want)


@pytest.mark.parametrize("v,n,batch", [(10, 1024, 3), (12, 1500, 1)])
@pytest.mark.parametrize("n_bits", [1247, 4096])
def test_pick_wide_indices_span_many_workgroups(hip, knobs, v, n, batch, n_bits):
    """Two (v = 10) and three (v = 12) subset tables, one slice of units at either N (the tables of one element at whole
    terms stay within the kernel's 32 768-byte budget, as in k_uint_read)."""
    index, a = operands(n_bits, EACH, [1] * v, 1, n, 1, batch, 900)
    check_forms(hip, knobs, n_bits, EACH, index, a, n)


@pytest.mark.parametrize("n_bits", [8320, 8256])
def test_pick_short_last_unit_slice(hip, knobs, n_bits):
    """v = 5: one subset table of 32 entries.  N = 8320 is 65 units of 16 bytes a term: 32 x 16 x 65 = 33 280 B pass the
    kernel's 32 768-byte budget, so the terms are cut into two slices of 33 units, the last one 32 units long.  N = 8256
    (129 words, odd) is 129 units of 8 bytes: slices of 65 and 64 units."""
    v = 5
    plan = (C.c_uint64 * 4)()
    assert hip.lib.csgn_uint_pick_plan(n_bits, ROTL, 2, v, u64s([1] * v), 3, 0, 1, 1, plan) == 0
    units = (n_bits + 63) // 64 // (2 if n_bits == 8320 else 1)
    assert int(plan[1]) < units < 2 * int(plan[1]), "the unit slices do not end short"
    for op, w, n, t in ((ROTL, 3, 0, 1), (SHR, 3, 0, 2), (EACH, 2, 19, 2)):
        index, a = operands(n_bits, op, [1] * v, w, n, t, 2, 1100)
        check_forms(hip, knobs, n_bits, op, index, a, n)


@pytest.mark.parametrize("op", ["shl", "shr"])
def test_pick_prefix_edges(hip, knobs, op):
    """(v, w) = (3, 8), fresh: E_j = 8, 12, 16, 18, 22, 24, 26, 27 over 1..8 rows.  The shape (N = 4096, 4 source terms)
    makes the fused form cut the stream of 27 entries into parts, asserted from csgn_uint_pick_plan: the one-row plane
    ends inside the first part, and a plane ends strictly inside a LATER part's decoded range."""
    op = OPS[op]
    n_bits, v, w, t, batch = 4096, 3, 8, 4, 2
    s = [1] * v
    E = [pick_terms(op, s, w, 0, j) for j in range(w)]
    assert sorted(E) == [8, 12, 16, 18, 22, 24, 26, 27]
    plan = (C.c_uint64 * 4)()
    assert hip.lib.csgn_uint_pick_plan(n_bits, op, batch, v, u64s(s), w, 0, t, 1, plan) == 0
    QP, parts = int(plan[2]), int(plan[3])
    assert parts >= 2 and (parts - 1) * QP < 27 <= parts * QP
    one_row = 0 if op == SHL else w - 1
    assert E[one_row] == 8 and 0 < E[one_row] < QP                      # ends in the middle of part 0
    inside = [j for j in range(w) if E[j] // QP >= 1 and E[j] % QP and E[j] < 27]
    assert inside, "no plane ends strictly inside a later part"
    index, a = operands(n_bits, op, s, w, 0, t, batch, 1200)
    want = check_forms(hip, knobs, n_bits, op, index, a, 0)
    dl = (n_bits + 63) // 64
    knobs.set("uint_pick_fused", 1)
    got = run(hip, n_bits, op, index, a)
    for j in [one_row] + inside:
        assert got[j].size == batch * t * E[j] * dl
        assert np.array_equal(got[j], want[j]), j


def test_pick_decrypts(hip, knobs, oracle):
    n_bits, d = 127, 8
    key, _ = oracle.keygen(n_bits, d, glibc_draws(601, 64 * d + 64))
    rng = np.random.default_rng(602)
    dl = (n_bits + 63) // 64
    knobs.unset("uint_pick_fused")
    for v, w in [(1, 3), (3, 8), (3, 5), (4, 16), (5, 8)]:
        ds = np.tile(np.arange(1 << v, dtype=np.uint64), 3)            # every distance
        batch = len(ds)
        xs = rng.integers(0, 1 << w, batch).astype(np.uint64)
        xs[:1 << v] = (1 << w) - 1
        index = encrypt_planes(oracle, n_bits, key, ds, v, 610 + v)
        a = encrypt_planes(oracle, n_bits, key, xs, w, 620 + w)
        for op in SHIFTS:
            outs = run(hip, n_bits, op, index, a)
            got = decrypt_value(oracle, n_bits, key, [o.reshape(batch, -1, dl) for o in outs])
            assert [int(g) for g in got] == [clear_pick(op, w, 0, int(x), int(dd)) for x, dd in zip(xs, ds)], (op, v, w)
        n = max(1, (1 << v) - 1)
        arrays = rng.integers(0, 1 << w, (batch, n)).astype(np.uint64)
        rows = encrypt_planes(oracle, n_bits, key, arrays.ravel(), w, 630 + w)
        outs = run(hip, n_bits, EACH, index, rows, n)
        got = decrypt_value(oracle, n_bits, key, [o.reshape(batch, -1, dl) for o in outs])
        assert [int(g) for g in got] == [clear_pick(EACH, w, n, arrays[e], int(dd)) for e, dd in enumerate(ds)], (v, w)


def test_trivial_distances_match_public_shifts(hip, knobs, oracle):
    """Trivially encrypted distances (one ONE / ZERO term per bit): the outputs decrypt to what shiftLeft(s) /
    shiftRight(s) / rotateLeft(s) / rotateRight(s) of certfhe/UInt.h give for the public s -- the planes moved by s."""
    n_bits, d, v, w = 1247, 16, 3, 8
    key, _ = oracle.keygen(n_bits, d, glibc_draws(641, 64 * d + 64))
    rng = np.random.default_rng(642)
    ds = np.tile(np.arange(1 << v), 4)
    batch = len(ds)
    xs = rng.integers(0, 1 << w, batch).astype(np.uint64)
    index = [np.stack([const_term(n_bits, (int(x) >> k) & 1) for x in ds]).reshape(batch, 1, -1) for k in range(v)]
    a = encrypt_planes(oracle, n_bits, key, xs, w, 643)
    bits = [decrypt_value(oracle, n_bits, key, [p]) for p in a]        # bit j of every element, by decryption
    dl = (n_bits + 63) // 64
    knobs.unset("uint_pick_fused")

    def moved(op, j, s):                                                # the plane the public-distance method puts at j
        p = {SHL: j - s, SHR: j + s, ROTL: (j - s) % w, ROTR: (j + s) % w}[op]
        return p if 0 <= p < w else None

    for op in SHIFTS:
        outs = run(hip, n_bits, op, index, a)
        got = decrypt_value(oracle, n_bits, key, [o.reshape(batch, -1, dl) for o in outs])
        for e in range(batch):
            want = 0
            for j in range(w):
                p = moved(op, j, int(ds[e]))
                want |= (int(bits[p][e]) if p is not None else 0) << j
            assert int(got[e]) == want == clear_pick(op, w, 0, int(xs[e]), int(ds[e])), (op, e)


def test_shift_matches_barrel_shifter_lookup(hip, knobs, oracle):
    """w = 8, v = 3: the 11-input lookup table of the barrel shifter (csgn_uint_lut) decrypts to the same integers."""
    n_bits, d, v, w, batch = 1247, 16, 3, 8, 64
    key, _ = oracle.keygen(n_bits, d, glibc_draws(651, 64 * d + 64))
    rng = np.random.default_rng(652)
    ds = np.arange(batch, dtype=np.uint64) % np.uint64(1 << v)
    xs = rng.integers(0, 1 << w, batch).astype(np.uint64)
    index = encrypt_planes(oracle, n_bits, key, ds, v, 653)
    a = encrypt_planes(oracle, n_bits, key, xs, w, 654)
    knobs.unset("uint_pick_fused")
    knobs.unset("uint_lut_fused")
    dl = (n_bits + 63) // 64
    planes = [hip.upload(p.ravel()) for p in a + index]                # table index: a + (d << 8)
    for op in (SHL, ROTR):
        f = [clear_pick(op, w, 0, x & 255, x >> 8) for x in range(1 << (w + v))]
        louts = [hip.download(o) for o in hip.uint_lut(n_bits, batch, planes, [1] * (w + v), f, w)]
        outs = run(hip, n_bits, op, index, a)
        got = decrypt_value(oracle, n_bits, key, [o.reshape(batch, -1, dl) for o in outs])
        via_lut = decrypt_value(oracle, n_bits, key, [o.reshape(batch, -1, dl) for o in louts])
        assert np.array_equal(got, via_lut), op
        assert [int(g) for g in got] == [clear_pick(op, w, 0, int(x), int(dd)) for x, dd in zip(xs, ds)], op


@pytest.mark.parametrize("s", [[1, 1, 1, 1], [1, 2, 1, 1]], ids=["fresh", "mixed"])
@pytest.mark.parametrize("n_bits", [129, 1247])
def test_each_of_equal_arrays_is_the_shared_read(hip, knobs, n_bits, s):
    """Every element's array the same table: csgn_uint_read of that one table has IDENTICAL words, in every form of
    either operation, with fresh index planes (the tables and the decoded list) and mixed ones (the walk and the
    digits per unit)."""
    v, n, w, batch = 4, 11, 3, 9
    index = [rand_terms(n_bits, batch, sk, 1300 + k) for k, sk in enumerate(s)]
    table = [rand_terms(n_bits, n, 2, 1310 + j) for j in range(w)]
    a = [np.tile(p, (batch, 1, 1)) for p in table]
    dx = [hip.upload(p.ravel()) for p in index]
    dt = [hip.upload(p.ravel()) for p in table]
    want = [x.ravel() for x in np_read_fast(n_bits, index, table)]
    reads = {}
    for fused in (-1, 0, 1):
        knobs.set("uint_read_fused", fused)
        reads[fused] = [hip.download(o) for o in hip.uint_read(n_bits, batch, dx, s, n, dt, [2] * w)]
        for j in range(w):
            assert np.array_equal(reads[fused][j], want[j]), ("read", fused, j)
    for fused, stage in ((-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)):
        knobs.set("uint_pick_fused", fused)
        knobs.set("uint_pick_stage", stage)
        got = run(hip, n_bits, EACH, index, a, n)
        for j in range(w):
            for rf, read in reads.items():
                assert np.array_equal(got[j], read[j]), (fused, stage, rf, j)
            assert np.array_equal(got[j], want[j]), (fused, stage, j)


def test_pick_graph_capture_and_replay(hip, knobs):
    n_bits, v, w, t, batch = 1247, 5, 32, 2, 5
    s = [1] * v
    index, a = operands(n_bits, ROTL, s, w, 0, t, batch, 1400)
    want = [x.ravel() for x in np_pick_fast(n_bits, ROTL, index, a)]
    knobs.set("uint_pick_fused", 1)
    dx = [hip.upload(p.ravel()) for p in index]
    da = [hip.upload(p.ravel()) for p in a]
    dl = (n_bits + 63) // 64
    outs = [hip.empty_words(batch * t * 243 * dl) for _ in range(w)]
    assert hip.lib.csgn_uint_pick_kernel(n_bits, ROTL, batch, v, u64s(s), w, 0, t) == b"k_uint_pick"
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        hip.uint_pick(n_bits, ROTL, batch, dx, s, da, t, 0, outs)         # warm-up outside the capture
    st.synchronize()
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        hip.uint_pick(n_bits, ROTL, batch, dx, s, da, t, 0, outs)
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for j in range(w):
        assert np.array_equal(hip.download(outs[j]), want[j]), j


def test_pick_dispatch_names(hip, knobs):
    lib = hip.lib

    def name(op, batch, v, s, w, rows, t):
        return lib.csgn_uint_pick_kernel(1247, op, batch, v, u64s(s), w, rows, t)

    knobs.unset("uint_pick_fused")
    assert name(SHL, 1 << 16, 3, [1] * 3, 8, 0, 1) == b"k_uint_pick"
    assert name(EACH, 1, 2, [3, 1], 64, 3, 2) == b"k_uint_pick"
    knobs.set("uint_pick_fused", 0)
    assert name(ROTL, 4096, 5, [1] * 5, 32, 0, 1) == b"composed"
    knobs.set("uint_pick_fused", 1)
    assert name(ROTR, 1, 1, [1], 1, 0, 1) == b"k_uint_pick"
    assert name(ROTR, 1, 1, [1], 1, 1, 1) == b""
    assert name(EACH, 1, 1, [1], 1, 3, 1) == b""


def test_pick_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([buf.data_ptr()] * 64))
    one = u64s([1] * 64)
    st = hip.stream
    assert lib.csgn_uint_pick(0, SHL, 1, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == -1          # n_bits
    assert lib.csgn_uint_pick(1247, 0, 1, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == -1         # op
    assert lib.csgn_uint_pick(1247, 6, 1, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 0, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == -1       # index width
    assert lib.csgn_uint_pick(1247, SHL, 1, 17, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 0, 0, ptrs, 1, ptrs, st) == -1       # width
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 65, 0, ptrs, 1, ptrs, st) == -1
    for op in SHIFTS:
        assert lib.csgn_uint_pick(1247, op, 1, 3, ptrs, one, 8, 1, ptrs, 1, ptrs, st) == -1    # rows
    assert lib.csgn_uint_pick(1247, EACH, 1, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, EACH, 1, 3, ptrs, one, 8, 9, ptrs, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 8, 0, ptrs, 0, ptrs, st) == -1       # terms
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 8, 0, ptrs, 1 << 62, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, u64s([1, 0, 1]), 8, 0, ptrs, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, u64s([1, 1 << 62, 1]), 8, 0, ptrs, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, None, one, 8, 0, ptrs, 1, ptrs, st) == -1       # host arrays
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, None, 8, 0, ptrs, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 8, 0, None, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 8, 0, ptrs, 1, None, st) == -1
    nullp = (C.c_void_p * 64)(*([buf.data_ptr()] * 2 + [None] + [buf.data_ptr()] * 61))
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, nullp, one, 8, 0, ptrs, 1, ptrs, st) == -1      # device pointers
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 8, 0, nullp, 1, ptrs, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 3, ptrs, one, 8, 0, ptrs, 1, nullp, st) == -1
    assert lib.csgn_uint_pick(1247, SHL, 1, 2, nullp, one, 2, 0, nullp, 1, nullp, st) == 0     # ... past the first v / w
    assert lib.csgn_uint_pick(1247, ROTL, 1, 16, ptrs, one, 1, 0, ptrs, 3, ptrs, st) == -2     # 2^31 words
    assert lib.csgn_uint_pick(1247, EACH, 1, 16, ptrs, u64s([2] * 16), 1, 1 << 16, ptrs, 1, ptrs, st) == -2
    assert lib.csgn_uint_pick(1247, ROTL, 1 << 44, 8, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == -2   # batch
    assert lib.csgn_uint_pick(1247, EACH, 1 << 40, 1, ptrs, one, 1, 1, ptrs, 1 << 20, ptrs, st) == -2
    assert lib.csgn_uint_pick(1247, SHL, 0, 3, ptrs, one, 8, 0, ptrs, 1, ptrs, st) == 0        # empty batch
    assert lib.csgn_uint_pick(1247, EACH, 0, 3, nullp, one, 8, 5, nullp, 1, nullp, st) == 0
    torch.cuda.synchronize()
