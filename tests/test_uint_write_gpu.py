"""Encrypted arrays written at encrypted indices on the device (csgn_uint_write), word for word against the definition
of include/csgn_hip.h (tests/model_write.py, pinned against the reference and the oracle in
tests/test_uint_write_cpu.py), in both forms the knob uint_write_fused selects, every run into caller outputs between
guard words; the host's split into launches; what the fused form's tile makes of the cases; decryptions of every index;
graph capture.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import GuardedOutputs, decrypt_value, encrypt_planes, hip, rand_terms, read_terms, u64s  # noqa: F401
from tests.model_write import array_terms, clear_write, np_write_fast, row_terms, write_offset

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs: the numpy side, not the device, is the limit

N_BITS = [63, 65, 129, 1247, 4096]      # 63 and 129: odd dL, the 8-byte-unit kernel
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 3, 3), (2, 4, 4), (3, 5, 8), (3, 8, 13), (4, 16, 64), (8, 200, 2), (8, 256, 2)]
VALUE_ARRAY_TERMS = ((1, 1), (2, 3), (3, 1))


def out_bytes(n_bits, s, n, tv, td, batch):
    """of one call: tv / td are the lists over the planes"""
    dl = (n_bits + 63) // 64
    return batch * sum(array_terms(s, n, a, b) for a, b in zip(tv, td)) * dl * 8


def operands(n_bits, s, n, tv, td, batch, seed):
    index = [rand_terms(n_bits, batch, sk, seed + 7 * k + sk) for k, sk in enumerate(s)]
    value = [rand_terms(n_bits, batch, t, seed + 100 + 11 * j) for j, t in enumerate(tv)]
    arrays = [rand_terms(n_bits, batch * n, t, seed + 500 + 13 * j) for j, t in enumerate(td)]
    return index, value, arrays


def run(hip, n_bits, index, value, arrays, n, want):
    """index[k]: words[batch, s_k, dL], value[j]: words[batch, tv_j, dL], arrays[j]: words[batch * n, td_j, dL] (host
    arrays).  The outputs are caller tensors of exactly the documented sizes between guard words, checked word for word
    against `want` and for writes outside them (tests/model.py, GuardedOutputs)."""
    dx = [hip.upload(p.ravel()) for p in index]
    dv = [hip.upload(p.ravel()) for p in value]
    da = [hip.upload(p.ravel()) for p in arrays]
    guarded = GuardedOutputs(hip, [x.size for x in want])
    hip.uint_write(n_bits, index[0].shape[0], dx, [p.shape[1] for p in index], n, dv, [p.shape[1] for p in value], da,
                   [p.shape[1] for p in arrays], outs=guarded.outs)
    torch.cuda.synchronize()
    what = ([p.shape[1] for p in index], n, [p.shape[1] for p in value], [p.shape[1] for p in arrays])
    return guarded.check(want, what)


def check_forms(hip, knobs, n_bits, index, value, arrays, n, forms=(0, 1), limit=MAX_BYTES):
    """Both forms against one computation of the definition's words."""
    want = [x.ravel() for x in np_write_fast(n_bits, index, value, arrays, n)]
    assert sum(x.nbytes for x in want) <= limit
    s, tv, td = ([p.shape[1] for p in x] for x in (index, value, arrays))
    for fused in forms:
        knobs.set("uint_write_fused", fused)
        name = hip.lib.csgn_uint_write_kernel(n_bits, index[0].shape[0], len(s), u64s(s), n, len(tv), u64s(tv), u64s(td))
        assert name == (b"k_uint_write" if fused else b"composed")
        run(hip, n_bits, index, value, arrays, n, want)                 # GuardedOutputs.check asserts every word
    return want


def mixed_terms(v, seed):
    """index planes of 1..3 terms, not all fresh"""
    s = [int(x) for x in np.random.default_rng(seed).integers(1, 4, v)]
    if s == [1] * v:
        s[0] = 2
    return s


def word_cases(n_bits, v, n, w):
    """(s, tv, td, batch) of test_write_words at one shape: fresh index planes and mixed ones of 1..3 terms (v = 8 and
    w = 64: fresh only), every plane with the same (tv, td) of the three and, with several planes, the three dealt over
    the planes.  The batch is 3 arrays, or fewer where three would pass 48 MB: every case stays below it."""
    cases = []
    for s in ([1] * v, mixed_terms(v, 100 * v + w + n_bits)):
        if s != [1] * v and (v == 8 or w == 64):
            continue
        kinds = [([a] * w, [b] * w) for a, b in VALUE_ARRAY_TERMS]
        if w > 1:
            kinds.append(([VALUE_ARRAY_TERMS[j % 3][0] for j in range(w)], [VALUE_ARRAY_TERMS[j % 3][1] for j in range(w)]))
        for tv, td in kinds:
            batch = min(3, MAX_BYTES // out_bytes(n_bits, s, n, tv, td, 1))
            assert batch >= 1, ("one array passes 48 MB", n_bits, s, n, tv, td)
            cases.append((s, tv, td, batch))
    return cases


@pytest.mark.parametrize("n_bits", N_BITS)
@pytest.mark.parametrize("v,n,w", SHAPES)
def test_write_words(hip, knobs, n_bits, v, n, w):
    for i, (s, tv, td, batch) in enumerate(word_cases(n_bits, v, n, w)):
        assert out_bytes(n_bits, s, n, tv, td, batch) <= MAX_BYTES
        index, value, arrays = operands(n_bits, s, n, tv, td, batch, 300 + i)
        check_forms(hip, knobs, n_bits, index, value, arrays, n)


def test_write_cases_cover_the_tile(hip):
    """What the shapes of test_write_words are chosen for, from the fused form's own tile (csgn_uint_write_plan): an
    array's stream of E entries is cut into parts of QP entries, one workgroup's decoded range each, and a row's raw
    copy is written by the workgroup that owns the row's last entry.  The cases hold a stream that is one part, a
    stream of several parts with a short last one, a part boundary that falls exactly behind a row's last entry, one
    that falls inside a row, and workgroups that own several arrays."""
    plan = (C.c_uint64 * 4)()
    seen = set()
    for n_bits in N_BITS:
        for v, n, w in SHAPES:
            for s, tv, td, batch in word_cases(n_bits, v, n, w):
                assert hip.lib.csgn_uint_write_plan(n_bits, batch, v, u64s(s), n, w, u64s(tv), u64s(td), 1, plan) == 0
                G, QP, parts = int(plan[0]), int(plan[2]), int(plan[3])
                E = read_terms(s, n)
                assert (parts - 1) * QP < E <= parts * QP
                seen.add("one part" if parts == 1 else "short last part" if E % QP else "even parts")
                row_ends = set(np.cumsum([row_terms(s, r) for r in range(n)]).tolist())
                for p in range(1, parts):
                    seen.add("boundary behind a row's last entry" if p * QP in row_ends else "boundary inside a row")
                if G > 1:
                    seen.add("several arrays")
    assert {"one part", "short last part", "boundary behind a row's last entry", "boundary inside a row",
            "several arrays"} <= seen, seen


@pytest.mark.parametrize("batch", [1, 257, 4099, (1 << 16) + 3])
def test_write_batches(hip, knobs, batch):
    """(v, n, w) = (2, 3, 3) at N = 65.  Fresh planes with one-term values and rows at every batch; mixed index planes
    with (tv, td) = (2, 3) up to 4099.  The largest batch writes 65 539 x 3 x 19 terms x 16 bytes = 59.8 MB at its
    smallest term counts: the one call of this file past 48 MB, held to exactly that size."""
    n_bits, n, w = 65, 3, 3
    index, value, arrays = operands(n_bits, [1, 1], n, [1] * w, [1] * w, batch, 700)
    limit = MAX_BYTES if batch < 1 << 16 else 65539 * 3 * 19 * 16
    assert out_bytes(n_bits, [1, 1], n, [1] * w, [1] * w, batch) <= limit
    check_forms(hip, knobs, n_bits, index, value, arrays, n, limit=limit)
    if batch < 1 << 16:
        assert out_bytes(n_bits, [1, 2], n, [2] * w, [3] * w, batch) <= MAX_BYTES
        index, value, arrays = operands(n_bits, [1, 2], n, [2] * w, [3] * w, batch, 710)
        check_forms(hip, knobs, n_bits, index, value, arrays, n)


@pytest.mark.parametrize("n_bits,tmode", [(63, "1"), (1247, "1"), (1247, "mixed")])
def test_write_batch_split_over_launches(hip, knobs, n_bits, tmode):
    """Knob launch_blocks lowers the workgroups of one launch, so launch_groups cuts the batch into several launches,
    each with its own index, value, array and output offsets (the arrays advance by e0 * n elements, the outputs by
    e0 * A_j terms); a last launch that is not full."""
    v, n, w, batch = 3, 6, 5, 37
    s = [1] * v if tmode == "1" else [2, 1, 3]
    tv, td = ([1] * w, [1] * w) if tmode == "1" else ([2, 1, 3, 2, 1], [3, 1, 1, 3, 2])
    assert out_bytes(n_bits, s, n, tv, td, batch) <= MAX_BYTES
    index, value, arrays = operands(n_bits, s, n, tv, td, batch, 800)
    want = [x.ravel() for x in np_write_fast(n_bits, index, value, arrays, n)]
    knobs.set("uint_write_fused", 1)
    for blocks in (1, 3, 7):
        knobs.set("launch_blocks", blocks)
        run(hip, n_bits, index, value, arrays, n, want)


def test_write_decrypts(hip, knobs, oracle):
    """v = 3, w = 4, n = 5 and 8: every index 0..7 in one batch decrypts to the array with that row replaced, and to the
    array untouched where the index is >= n."""
    n_bits, d, v, w = 127, 8, 3, 4
    key, _ = oracle.keygen(n_bits, d, glibc_draws(901, 64 * d + 64))
    rng = np.random.default_rng(902)
    dl = (n_bits + 63) // 64
    for n in (5, 8):
        ds = np.tile(np.arange(1 << v, dtype=np.uint64), 2)
        batch = len(ds)
        table = rng.integers(0, 1 << w, (batch, n)).astype(np.uint64)
        vals = rng.integers(0, 1 << w, batch).astype(np.uint64)
        vals[:1 << v] = table[:1 << v, 0] ^ np.uint64((1 << w) - 1)     # every bit of the written row changes
        index = encrypt_planes(oracle, n_bits, key, ds, v, 910 + n)
        value = encrypt_planes(oracle, n_bits, key, vals, w, 920 + n)
        arrays = encrypt_planes(oracle, n_bits, key, table.ravel(), w, 930 + n)
        A = array_terms([1] * v, n, 1, 1)
        for fused in (0, 1):
            knobs.set("uint_write_fused", fused)
            want = [x.ravel() for x in np_write_fast(n_bits, index, value, arrays, n)]
            outs = [o.reshape(batch, A, dl) for o in run(hip, n_bits, index, value, arrays, n, want)]
            for r in range(n):
                lo, hi = write_offset([1] * v, r, 1, 1), write_offset([1] * v, r + 1, 1, 1)
                got = decrypt_value(oracle, n_bits, key, [o[:, lo:hi, :] for o in outs])
                for e in range(batch):
                    assert int(got[e]) == clear_write(n, table[e], int(ds[e]), vals[e])[r], (fused, n, e, r)


def test_write_graph_capture_and_replay(hip, knobs):
    n_bits, v, n, w, batch = 1247, 5, 32, 8, 5
    s, tv, td = [1] * v, [2] * w, [1] * w
    index, value, arrays = operands(n_bits, s, n, tv, td, batch, 1400)
    want = [x.ravel() for x in np_write_fast(n_bits, index, value, arrays, n)]
    assert sum(x.nbytes for x in want) <= MAX_BYTES
    knobs.set("uint_write_fused", 1)
    dx = [hip.upload(p.ravel()) for p in index]
    dv = [hip.upload(p.ravel()) for p in value]
    da = [hip.upload(p.ravel()) for p in arrays]
    assert hip.lib.csgn_uint_write_kernel(n_bits, batch, v, u64s(s), n, w, u64s(tv), u64s(td)) == b"k_uint_write"
    st = torch.cuda.Stream()
    warm = [hip.empty_words(x.size) for x in want]
    with torch.cuda.stream(st):
        hip.uint_write(n_bits, batch, dx, s, n, dv, tv, da, td, warm)          # warm-up outside the capture
    st.synchronize()
    guarded = GuardedOutputs(hip, [x.size for x in want])                      # fresh outputs for the replay
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        hip.uint_write(n_bits, batch, dx, s, n, dv, tv, da, td, guarded.outs)
    torch.cuda.synchronize()
    fresh = GuardedOutputs(hip, [x.size for x in want])
    for whole, again in zip(guarded.whole, fresh.whole):
        whole.copy_(again)                                                     # every word back to the fill
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    guarded.check(want, "replay")


def test_write_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([buf.data_ptr()] * 64))
    nullp = (C.c_void_p * 64)(*([buf.data_ptr()] * 2 + [None] + [buf.data_ptr()] * 61))
    one = u64s([1] * 64)
    st = hip.stream
    assert lib.csgn_uint_write(0, 1, 3, ptrs, one, 8, 8, ptrs, one, ptrs, one, ptrs, st) == -1          # n_bits
    assert lib.csgn_uint_write(1247, 1, 17, ptrs, one, 8, 8, ptrs, one, ptrs, one, ptrs, st) == -1      # index width
    assert lib.csgn_uint_write(1247, 1, 3, ptrs, one, 8, 65, ptrs, one, ptrs, one, ptrs, st) == -1      # width
    assert lib.csgn_uint_write(1247, 1, 3, ptrs, one, 9, 8, ptrs, one, ptrs, one, ptrs, st) == -1       # rows
    assert lib.csgn_uint_write(1247, 1, 3, nullp, one, 8, 8, ptrs, one, ptrs, one, ptrs, st) == -1      # device pointers
    assert lib.csgn_uint_write(1247, 1, 3, ptrs, one, 8, 8, nullp, one, ptrs, one, ptrs, st) == -1
    assert lib.csgn_uint_write(1247, 1, 3, ptrs, one, 8, 8, ptrs, one, nullp, one, ptrs, st) == -1
    assert lib.csgn_uint_write(1247, 1, 3, ptrs, one, 8, 8, ptrs, one, ptrs, one, nullp, st) == -1
    assert lib.csgn_uint_write(1247, 1, 16, ptrs, one, 1 << 16, 1, ptrs, u64s([2]), ptrs, one, ptrs, st) == -2   # 2^31 words
    assert lib.csgn_uint_write(1247, 1 << 50, 3, ptrs, one, 8, 8, ptrs, one, ptrs, one, ptrs, st) == -2  # batch
    assert lib.csgn_uint_write(1247, 0, 3, nullp, one, 8, 8, nullp, one, nullp, one, nullp, st) == 0     # empty batch
    torch.cuda.synchronize()
