"""Sums of comparisons of an encrypted integer against public constants (csgn_uint_plain_sum*), on a box without a GPU:
csgn_uint_plain_sum_terms against the model (tests/model_plain_sum.py) over a sweep; every term of every plane of the
shapes of tests/test_uint_plain_sum_gpu.py rebuilt from csgn_uint_plain_sum_decode's factors and compared word for word
with the numpy composition; the composition against the oracle's and, where built, the reference's own operators; the
decryptions of ranges, sets, step functions and sparse tables through the oracle; the argument checks and their order;
csgn_uint_plain_sum_launches against a host replay of the grid.  The device side is tests/test_uint_plain_sum_gpu.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle.binding import glibc_draws, load_ref
from tests.model import (EQ, GE, GT, INVALID, LE, LIMIT, LT, NE, NO_DEVICE, OK, UNSUPPORTED, const_term, decrypt_value,  # noqa: F401
                         encrypt_planes, lib, oracle_ops, rand_terms, ref_ops, u64s)
from tests.model_plain_sum import (NS, ONE, ZERO, clear_plain_sum, clear_range, clear_sparse, clear_step,
                                   compose_plain_sum, decode, gpu_shapes, np_plain_sum, plane_runs, range_entries,
                                   ranges_entries, rebuild, replay_grid, set_entries, sparse_entries, step_entries,
                                   sum_terms, symbolic_plain_sum)

CMPS = (EQ, NE, LT, LE, GT, GE)


def ints(xs):
    xs = list(xs)
    return (C.c_int * max(len(xs), 1))(*xs)


def arrays(entries):
    return ints(c for c, _ in entries), u64s([k for _, k in entries] or [0])


def c_terms(lib, ta, entries, cbit):
    cmp, k = arrays(entries)
    return int(lib.csgn_uint_plain_sum_terms(len(ta), u64s(ta), len(entries), cmp, k, cbit))


def c_decode(lib, ta, entries, cbit, q):
    """The factors of term q as sorted (plane, term) labels, or None where the C ABI refuses."""
    cmp, k = arrays(entries)
    plane, term, n = (C.c_uint64 * 65)(*([77] * 65)), (C.c_uint64 * 65)(*([77] * 65)), C.c_uint64(77)
    if not lib.csgn_uint_plain_sum_decode(len(ta), u64s(ta), len(entries), cmp, k, cbit, q, plane, term, C.byref(n)):
        assert n.value == 77 and plane[0] == 77 and term[0] == 77
        return None
    assert 1 <= n.value <= 64
    w = len(ta)
    out = [((ONE if plane[f] == w else ZERO if plane[f] == w + 1 else int(plane[f])), int(term[f])) for f in range(n.value)]
    return sorted(out, key=str)


def shape_arrays(ta, planes_entries):
    flat = [e for entries in planes_entries for e in entries]
    first = list(itertools.accumulate([0] + [len(e) for e in planes_entries]))
    cmp, k = arrays(flat)
    return u64s(ta), u64s(first), cmp, k


def c_launches(lib, n, batch, ta, planes_entries, constant):
    t, first, cmp, k = shape_arrays(ta, planes_entries)
    plan = (C.c_uint64 * 6)()
    rc = lib.csgn_uint_plain_sum_launches(n, batch, len(ta), t, len(planes_entries), first, cmp, k, constant, plan)
    assert rc == 0, lib.csgn_last_error()
    return [int(x) for x in plan]


# -- the term counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 8, 33, 64])
def test_terms_equal_the_model(lib, w):
    """Widths 1, 2, 3, 8, 33 and 64; term vectors of 1, 2 and 3 terms; all six comparisons at k = 0, 1, the top, the
    top - 1 and the middle (the ZERO cases among them); single entries, all of them in one plane, the empty plane; both
    constant bits.  Counts past 2^62 are 0 on both sides."""
    top = (1 << w) - 1
    ks = sorted({0, 1 & top, top, max(top - 1, 0), 1 << (w - 1), top ^ (1 << (w - 1))})
    for ta in ([1] * w, [2] * w, [3] * w, [1 + j % 3 for j in range(w)]):
        entries = [(c, k) for k in ks for c in CMPS]
        for cbit in (0, 1):
            assert c_terms(lib, ta, [], cbit) == sum_terms(ta, [], cbit) == 1
            fits = []
            for e in entries:
                want = sum_terms(ta, [e], cbit)
                assert c_terms(lib, ta, [e], cbit) == want, (ta, e, cbit)
                if 0 < want < 1 << 40:
                    fits.append(e)
            assert fits
            assert c_terms(lib, ta, fits, cbit) == sum_terms(ta, fits, cbit) == sum(sum_terms(ta, [e], 0) for e in fits) + cbit
            assert c_terms(lib, ta, entries, cbit) == sum_terms(ta, entries, cbit)


def test_terms_by_hand_and_refusals(lib):
    one3 = [1, 1, 1]
    assert c_terms(lib, one3, [(LT, 6), (LT, 2)], 0) == 4 + 4 and c_terms(lib, one3, [(EQ, 7)] * 5, 1) == 6
    assert c_terms(lib, one3, [(LT, 0)], 0) == 1 and c_terms(lib, one3, [(GE, 0)], 1) == 3 and c_terms(lib, one3, [(GT, 7)], 0) == 1
    # refused: the width, null arrays, a zero count, a comparison, a constant that does not fit, the constant bit
    assert int(lib.csgn_uint_plain_sum_terms(0, u64s([1]), 0, None, None, 0)) == 0
    assert int(lib.csgn_uint_plain_sum_terms(65, u64s([1] * 65), 0, None, None, 0)) == 0
    assert int(lib.csgn_uint_plain_sum_terms(3, None, 0, None, None, 0)) == 0
    assert int(lib.csgn_uint_plain_sum_terms(3, u64s(one3), 1, None, u64s([1]), 0)) == 0
    assert int(lib.csgn_uint_plain_sum_terms(3, u64s(one3), 1, ints([EQ]), None, 0)) == 0
    assert int(lib.csgn_uint_plain_sum_terms(3, u64s(one3), 0, None, None, 0)) == 1
    assert c_terms(lib, [1, 0, 1], [(EQ, 1)], 0) == 0 and c_terms(lib, one3, [(0, 1)], 0) == 0 and c_terms(lib, one3, [(7, 1)], 0) == 0
    assert c_terms(lib, one3, [(EQ, 8)], 0) == 0 and c_terms(lib, one3, [(EQ, 1)], 2) == 0
    # 2^62, without wrap-around
    big = LIMIT - 1
    assert c_terms(lib, [big], [(EQ, 1)], 0) == big and c_terms(lib, [big], [(EQ, 1)], 1) == 0
    assert c_terms(lib, [big], [(EQ, 1), (EQ, 1)], 0) == 0 and c_terms(lib, [1 << 60], [(EQ, 1)] * 3, 1) == (3 << 60) + 1
    assert c_terms(lib, [1 << 60], [(EQ, 1)] * 4, 0) == 0 and c_terms(lib, [1 << 61] * 2, [(EQ, 3)], 0) == 0
    assert lib.csgn_uint_plain_sum_decode(3, u64s(one3), 0, None, None, 0, 0, None, None, None) == 0


# -- the decode by position --------------------------------------------------------------------------------------------
SHAPES = gpu_shapes()


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_decode_rebuilds_every_term(lib, shape):
    """Every term q of every plane of the GPU shapes: the AND of csgn_uint_plain_sum_decode's factors over random planes
    equals the numpy composition word for word; where the symbolic composition is small it equals the factors too."""
    name, ta, planes_entries, constant, _ = shape
    n, batch = 1247, 2
    planes = [rand_terms(n, batch, t, 900 + 7 * j + t) for j, t in enumerate(ta)]
    want = np_plain_sum(n, planes, planes_entries, constant)
    small = sum(o.shape[1] for o in want) <= 3000
    table = symbolic_plain_sum(ta, planes_entries, constant) if small else None
    for x, entries in enumerate(planes_entries):
        cbit = (constant >> x) & 1
        T = want[x].shape[1]
        assert c_terms(lib, ta, entries, cbit) == T == sum_terms(ta, entries, cbit)
        for q in range(T):
            factors = c_decode(lib, ta, entries, cbit, q)
            assert factors is not None, (name, x, q)
            assert np.array_equal(rebuild(n, planes, factors), want[x][:, q, :]), (name, x, q, factors)
            if table is not None:
                assert factors == sorted(table[x][q], key=str), (name, x, q)
        assert c_decode(lib, ta, entries, cbit, T) is None


def test_decode_by_hand(lib):
    one3 = [1, 1, 1]
    assert c_decode(lib, one3, [], 0, 0) == [(ZERO, 0)] and c_decode(lib, one3, [], 1, 0) == [(ONE, 0)]
    assert c_decode(lib, one3, [(EQ, 7)], 1, 0) == [(0, 0), (1, 0), (2, 0)] and c_decode(lib, one3, [(EQ, 7)], 1, 1) == [(ONE, 0)]
    assert c_decode(lib, one3, [(LT, 0), (NE, 7)], 0, 0) == [(ZERO, 0)] and c_decode(lib, one3, [(LT, 0), (NE, 7)], 0, 2) == [(ONE, 0)]
    assert c_decode(lib, [2, 3], [(EQ, 3), (EQ, 3)], 0, 6 + 4) == decode([2, 3], [(EQ, 3), (EQ, 3)], 0, 10) == [(0, 1), (1, 1)]


# -- the definition against the genuine reference and the oracle -------------------------------------------------------
@pytest.mark.parametrize("n,d", [(65, 4), (1247, 16)])
def test_definition_matches_reference_and_oracle(oracle, n, d):
    """A few shapes through the oracle's operator+ / operator* and, where the reference is built, through its own: the
    words of the numpy composition."""
    ref = load_ref()
    routes = [oracle_ops(oracle, n)] + ([ref_ops(ref, n, d)] if ref is not None else [])
    dl = (n + 63) // 64
    for name, ta, planes_entries, constant, _ in [s for s in SHAPES if s[0] in ("range-w3", "mixed", "runs", "t23", "w1")]:
        planes = [rand_terms(n, 1, t, 40 + j) for j, t in enumerate(ta)]
        flat = [p[0].ravel() for p in planes]
        want = np_plain_sum(n, planes, planes_entries, constant)
        for add, mul in routes:
            got = compose_plain_sum(flat, planes_entries, constant, add, mul, const_term(n, 1), const_term(n, 0))
            for x, entries in enumerate(planes_entries):
                assert np.array_equal(got[x], want[x].ravel()), (name, x)
                assert got[x].size == sum_terms(ta, entries, (constant >> x) & 1) * dl


# -- semantics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_decrypts(oracle, w):
    """Through the oracle's encrypt and decrypt at N = 127, for every a below 2^w: ranges (every pair for w <= 3), a
    union of ranges, sets, step functions, bucketOf and sparse tables decrypt to their clear values."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(2210 + w, 64 * d + 64))
    xs = np.arange(1 << w, dtype=np.uint64)
    a = encrypt_planes(oracle, n, key, xs, w, 2220 + w)
    top = (1 << w) - 1
    rng = np.random.default_rng(w)

    def check(planes_entries, constant, clear, what):
        outs = np_plain_sum(n, a, planes_entries, constant)
        want = np.array([clear(int(x)) for x in xs], dtype=np.uint64)
        assert np.array_equal(decrypt_value(oracle, n, key, outs), want), what
        assert [clear_plain_sum(planes_entries, constant, int(x)) for x in xs] == list(want), what

    pairs = [(lo, hi) for lo in range(top + 1) for hi in range(lo, top + 1)]
    if w > 3:
        pairs = [(0, top), (0, top // 2), (top // 3, top), (1, top - 1), (top // 2, top // 2), (3, 9), (top - 1, top - 1)]
    for lo, hi in pairs:
        entries, cbit = range_entries(w, lo, hi)
        check([entries, entries], cbit | ((cbit ^ 1) << 1), lambda x: clear_range(lo, hi, x) | ((1 - clear_range(lo, hi, x)) << 1),
              ("range", lo, hi))
    if w >= 3:
        intervals = [(0, 1), (3, 3), (top - 1, top)] if w == 3 else [(1, 2), (5, 9), (11, 11), (top - 2, top)]
        entries, cbit = ranges_entries(w, intervals)
        check([entries], cbit, lambda x: int(any(lo <= x <= hi for lo, hi in intervals)), ("ranges", intervals))
    for size in (1, 2, min(5, top + 1)):
        keys = [int(k) for k in rng.choice(top + 1, size=size, replace=False)] + [int(rng.integers(0, top + 1))]
        entries, cbit = set_entries(keys)
        check([entries, entries], 0b10, lambda x: int(x in keys) | (int(x not in keys) << 1), ("set", keys))
    if w >= 2:
        m = min(3, top)
        thresholds = sorted(int(t) for t in rng.choice(np.arange(1, top + 1), size=m, replace=False))
        values = [int(v) for v in rng.integers(0, 16, m + 1)]
        planes_entries, constant = step_entries(thresholds, values, 4)
        check(planes_entries, constant, lambda x: clear_step(thresholds, values, x), ("step", thresholds, values))
        planes_entries, constant = step_entries(thresholds, list(range(m + 1)), 2)
        check(planes_entries, constant, lambda x: sum(1 for t in thresholds if x >= t), ("bucket", thresholds))
    keys = [int(k) for k in rng.choice(top + 1, size=min(4, top + 1), replace=False)]
    values = [int(v) for v in rng.integers(0, 32, len(keys))]
    for otherwise in (0, 0b10110):
        planes_entries, constant = sparse_entries(keys, values, 5, otherwise)
        check(planes_entries, constant, lambda x: clear_sparse(keys, values, otherwise, x), ("sparse", keys, values, otherwise))


# -- the argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_order(lib):
    """csgn_uint_plain_sum_create: the status is that of the first check that fails, in the documented order, the
    device last (NO_DEVICE on a box without one, never a CPU fallback).  csgn_uint_plain_sum: n_bits, the host arrays,
    then the plan -- without a device there is no plan, and the call says NO_DEVICE."""
    import torch
    gpu = torch.cuda.is_available()
    one8 = u64s([1] * 8)
    first2 = u64s([0, 2, 3])
    cmp3, k3 = ints([LT, LT, EQ]), u64s([200, 17, 255])

    def create(w=8, ta=one8, m=2, first=first2, cmp=cmp3, k=k3, constant=0b10, handle=True):
        h = C.c_void_p(77)
        rc = lib.csgn_uint_plain_sum_create(w, ta, m, first, cmp, k, constant, C.byref(h) if handle else None)
        if rc != OK and handle:
            assert h.value is None                                   # nothing is handed out on failure
        if rc == OK:
            lib.csgn_uint_plain_sum_destroy(h)
        return rc

    assert create(handle=False) == INVALID and b"plan is null" in lib.csgn_last_error()
    assert create(w=0, ta=None) == INVALID and create(w=65, first=None) == INVALID          # the width
    assert b"width" in lib.csgn_last_error()
    assert create(m=0, ta=None) == INVALID and create(m=65, ta=None) == INVALID              # n_out
    assert create(constant=0b100, ta=None) == INVALID and b"does not fit" in lib.csgn_last_error()
    assert create(ta=None, first=u64s([1, 2, 3])) == INVALID and b"null host pointer" in lib.csgn_last_error()
    assert create(first=None, cmp=None) == INVALID and b"null host pointer" in lib.csgn_last_error()
    assert create(first=u64s([1, 2, 3]), cmp=None) == INVALID and b"h_first[0]" in lib.csgn_last_error()
    assert create(first=u64s([0, 3, 2]), cmp=None) == INVALID and b"descends" in lib.csgn_last_error()
    assert create(cmp=None, ta=u64s([0] * 8)) == INVALID and b"null host pointer" in lib.csgn_last_error()
    assert create(k=None, ta=u64s([0] * 8)) == INVALID and b"null host pointer" in lib.csgn_last_error()
    # more than 65536 entries, before any entry or count is looked at
    many = 65537
    assert create(first=u64s([0, many, many]), cmp=ints([0] * many), k=u64s([0] * many), ta=u64s([0] * 8)) == UNSUPPORTED
    assert b"65536" in lib.csgn_last_error()
    assert create(ta=u64s([1, 0] + [1] * 6), cmp=ints([9, LT, EQ])) == INVALID and b"no terms" in lib.csgn_last_error()
    assert create(cmp=ints([LT, 9, EQ]), k=u64s([200, 17, 256])) == INVALID and b"unknown comparison" in lib.csgn_last_error()
    assert create(k=u64s([200, 256, 255])) == INVALID and b"does not fit" in lib.csgn_last_error()
    # a result of 2^62 terms or more (INVALID) before a plane of 2^31 (UNSUPPORTED)
    assert create(ta=u64s([1 << 8] * 8), cmp=ints([EQ, LT, EQ])) == INVALID and b"overflows" in lib.csgn_last_error()
    assert create(ta=u64s([1 << 4] * 8), cmp=ints([LT, LT, EQ]), k=u64s([200, 17, 0])) == UNSUPPORTED  # 16 * 17^7 terms in LT 17
    assert b"2^31" in lib.csgn_last_error()
    assert create(ta=u64s([1 << 4] * 8), cmp=ints([EQ, LT, EQ]), k=u64s([255, 17, 255])) == UNSUPPORTED   # 2^32 in plane 0
    # the launch query makes the same refusals, then the sizes, and needs no device
    plan = (C.c_uint64 * 6)()

    def launches(n=1247, batch=4, w=8, ta=one8, m=2, first=first2, cmp=cmp3, k=k3, constant=0b10, out=plan):
        return lib.csgn_uint_plain_sum_launches(n, batch, w, ta, m, first, cmp, k, constant, out)

    assert launches() == OK and plan[0] == 16 and plan[2] == 1 and plan[3] == 1 and plan[4] == 4
    assert launches(batch=0) == OK and list(plan)[3:] == [0, 0, 0]
    assert launches(n=0, w=0) == INVALID and launches(n=131073, w=0) == UNSUPPORTED
    assert launches(w=0) == INVALID and launches(constant=4) == INVALID and launches(out=None) == INVALID
    assert launches(k=u64s([200, 256, 255]), out=None) == INVALID and b"does not fit" in lib.csgn_last_error()
    assert launches(ta=u64s([1 << 27] * 8), cmp=ints([LT, LT, LT]), k=u64s([128, 128, 128])) == UNSUPPORTED   # inputs: 2^27 * 20 words
    assert b"input plane" in lib.csgn_last_error()
    assert launches(batch=1 << 56) == UNSUPPORTED and b"batch" in lib.csgn_last_error()
    # the launching call: n_bits, the host arrays, the plan
    buf = np.zeros(64, dtype=np.uint64)
    ptrs = (C.c_void_p * 64)(*([buf.ctypes.data] * 64))
    assert lib.csgn_uint_plain_sum(None, 0, 1, ptrs, ptrs, None) == INVALID
    assert lib.csgn_uint_plain_sum(None, 1247, 1, None, ptrs, None) == INVALID and b"null host pointer" in lib.csgn_last_error()
    assert lib.csgn_uint_plain_sum(None, 1247, 1, ptrs, None, None) == INVALID
    assert int(lib.csgn_uint_plain_sum_plan_terms(None, 0)) == 0
    lib.csgn_uint_plain_sum_destroy(None)
    if gpu:
        assert lib.csgn_uint_plain_sum(None, 1247, 1, ptrs, ptrs, None) == INVALID and b"plan is null" in lib.csgn_last_error()
        return
    assert create() == NO_DEVICE and b"no CPU" in lib.csgn_last_error()
    assert create(m=1, first=u64s([0, 0]), cmp=None, k=None, constant=1) == NO_DEVICE         # an empty plane is a plan too
    for batch in (0, 1):
        assert lib.csgn_uint_plain_sum(None, 1247, batch, ptrs, ptrs, None) == NO_DEVICE
        assert b"no CPU" in lib.csgn_last_error()
    assert (buf == 0).all()                                             # and nothing was computed on the host


# -- the launch query, replayed ----------------------------------------------------------------------------------------
def units_of(n, wide):
    dl = (n + 63) // 64
    return dl // 2 if wide and dl % 2 == 0 else dl


def check_launches(lib, knobs, n, ta, planes_entries, constant, batch, cap=0):
    """The query's figures against their definition, then every lane of every launch placed as the kernel places it:
    every item of every output plane exactly once."""
    knobs.set("launch_blocks", cap)
    plan = c_launches(lib, n, batch, ta, planes_entries, constant)
    dl = (n + 63) // 64
    U = units_of(n, True)
    runs = [plane_runs(ta, e, (constant >> x) & 1)[2] for x, e in enumerate(planes_entries)]
    assert plan[0] == (16 if dl % 2 == 0 else 8) and plan[1] == sum(runs) * U and plan[2] == 1
    count, launches, first = replay_grid(ta, planes_entries, constant, batch, U, cap if cap else ((1 << 32) - 1) // 256)
    assert (plan[3], plan[4], plan[5]) == (launches, first[0], first[1]), (n, batch, cap)
    for x, c in enumerate(count):
        assert c.size == batch * runs[x] * U and (c == 1).all(), (n, ta, x, batch, cap)
    if plan[0] == 16:                                                # the same shape with a pointer off alignment
        for c in replay_grid(ta, planes_entries, constant, batch, units_of(n, False), ((1 << 32) - 1) // 256)[0]:
            assert (c == 1).all()
    return plan


@pytest.mark.parametrize("n", NS)
def test_launches_cover_every_item_once(lib, knobs, n):
    for name, ta, planes_entries, constant, batches in SHAPES:
        if name in ("wg-edge", "eq300") and n != 64:
            batches = batches[:1]                                    # thousands of workgroups: one batch is the replay
        for batch in batches:
            check_launches(lib, knobs, n, ta, planes_entries, constant, batch)


def test_launches_under_caps(lib, knobs):
    """launch_blocks caps that cut a call into 2 and 3 launches, one that leaves it whole, one below an element's
    workgroups (an element still goes whole), one at the number of planes."""
    for name in ("mixed", "t23", "planes64", "runs"):
        _, ta, planes_entries, constant, _ = next(s for s in SHAPES if s[0] == name)
        whole = check_launches(lib, knobs, 1247, ta, planes_entries, constant, 40)
        assert whole[3] == 1 and whole[4] == 40
        np_, items = len(planes_entries), whole[1]
        for want in (2, 3):
            per = -(-40 // want)                                       # elements a launch
            cap = -(-per * items // 256) + np_
            assert check_launches(lib, knobs, 1247, ta, planes_entries, constant, 40, cap)[3] == want, (name, want)
        assert check_launches(lib, knobs, 1247, ta, planes_entries, constant, 40, whole[5] + np_)[3] == 1
        assert check_launches(lib, knobs, 1247, ta, planes_entries, constant, 5, 1)[3] == 5
        assert check_launches(lib, knobs, 1247, ta, planes_entries, constant, 5, np_)[3] == 5
