"""Selection by an encrypted comparison on the device (csgn_uint_lt_select), word for word against the definition of
include/csgn_hip.h (pinned against the reference and the oracle in tests/test_uint_lt_select_cpu.py), in both forms the
knob uint_lt_select_form selects; the cross-check against the chained csgn_uint_step / csgn_gate_uniform calls a user
issues today; decryptions of compare-exchanges; graph capture.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (LT_FIRST, LT_STEP, MUX, GuardedOutputs, decrypt_bits, decrypt_value, encrypt_planes, hip,
                         np_uint_lt, rand_terms, u64s)
from tests.model_lt_select import lt_counts, lt_terms, minmax_requests, out_terms, place

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs: the numpy side, not the device, is the limit
MAX_COMPOSED_LAUNCHES = 256


def terms_of(planes):
    return [p.shape[1] for p in planes]


class Operands:
    """a, b and a pool of request planes on the host and, uploaded once, on the device; planes are named by index into
    `host`, so that requests which alias a or b hand over the very same device pointers."""

    def __init__(self, hip, n, a, b, extra=()):
        self.hip, self.n, self.w = hip, n, len(a)
        self.host = list(a) + list(b) + list(extra)
        self.dev = [hip.upload(p.ravel()) for p in self.host]
        self.batch = a[0].shape[0]
        self.lt = np_uint_lt(n, a, b)                                  # the reference, computed once

    def a(self, j):
        return j

    def b(self, j):
        return self.w + j

    def extra(self, j):
        return 2 * self.w + j

    def want(self, xs, ys, less):
        outs = place(self.lt, [self.host[i] for i in xs], [self.host[i] for i in ys])
        return [o.ravel() for o in outs] + ([self.lt.ravel()] if less else [])

    def out_bytes(self, xs, ys, less):
        L, dl = self.lt.shape[1], self.lt.shape[2]
        terms = sum(out_terms(L, self.host[x].shape[1], self.host[y].shape[1]) for x, y in zip(xs, ys)) + (L if less else 0)
        return self.batch * terms * dl * 8

    def call(self, xs, ys, outs, less):
        w = self.w
        return self.hip.uint_lt_select(self.n, self.batch, self.dev[:w], terms_of(self.host[:w]), self.dev[w:2 * w],
                                       terms_of(self.host[w:2 * w]), [self.dev[i] for i in xs],
                                       [self.host[i].shape[1] for i in xs], [self.dev[i] for i in ys],
                                       [self.host[i].shape[1] for i in ys], outs=outs, less=less)

    def run(self, xs, ys, less, want=None, shift=0):
        """The outputs and the comparison (last, when asked for), downloaded.  With `want` they are caller tensors of
        exactly those sizes between guard words, checked word for word and for writes outside them (GuardedOutputs)."""
        m = len(xs)
        guarded = GuardedOutputs(self.hip, [x.size for x in want], shift) if want is not None else None
        outs, lt = self.call(xs, ys, guarded.outs[:m] if guarded else None,
                             (guarded.outs[m] if guarded else True) if less else False)
        torch.cuda.synchronize()
        if guarded:
            return guarded.check(want, (terms_of(self.host[:2 * self.w]), xs, ys, less))
        return [self.hip.download(o) for o in outs] + ([self.hip.download(lt)] if less else [])

    def check_forms(self, knobs, xs, ys, less, forms=(-1, 0, 1)):
        want = self.want(xs, ys, less)
        for form in forms:
            if form == 0 and self.w * (len(xs) + 1) > MAX_COMPOSED_LAUNCHES:
                continue
            knobs.set("uint_lt_select_form", form)
            self.run(xs, ys, less, want)                               # GuardedOutputs.check asserts every word


def term_counts(tmode, count, rng, fresh=False):
    """Terms of `count` planes: all 1 (the fresh path), all 2, or 1..3 drawn independently; "afresh" is a fresh a
    (`fresh`) under a b that is not."""
    if tmode in ("1", "2"):
        return [int(tmode)] * count
    if tmode == "afresh" and fresh:
        return [1] * count
    t = [int(x) for x in rng.integers(1, 4, count)]
    if tmode == "afresh" and count:
        t[0] = max(t[0], 2)
    return t


def operands(hip, n, batch, ta, tb, extra_terms=(), seed=0):
    a = [rand_terms(n, batch, t, seed + 400 + 7 * k + t) for k, t in enumerate(ta)]
    b = [rand_terms(n, batch, t, seed + 450 + 5 * k + t) for k, t in enumerate(tb)]
    extra = [rand_terms(n, batch, t, seed + 500 + 11 * k) for k, t in enumerate(extra_terms)]
    return Operands(hip, n, a, b, extra)


# 63 and 129: odd dL, the 8-byte-unit kernel; 65 and 1247 / 4096: 16-byte units; 5 -> 6 planes: one -> two subset tables
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("w", [1, 2, 3, 5, 6, 8])
def test_lt_select_words(hip, knobs, n, w):
    """Every term mode at one (N, width): the comparison alone, one request, min and max (requests that alias a and b)
    and 64 requests that mix the operands with payload planes of 1 to 3 terms.  A call whose outputs pass 48 MB is
    skipped; a mode of which nothing ran is one whose smallest call, the comparison alone, is already past it."""
    batch, dl = 2, (n + 63) // 64
    ran = {}
    for tmode in ("1", "2", "mixed", "afresh"):
        rng = np.random.default_rng(w * 100 + n + len(tmode))
        ta, tb = term_counts(tmode, w, rng, fresh=True), term_counts(tmode, w, rng)
        L = lt_terms(ta, tb)
        ran[tmode] = 0
        if batch * L * dl * 8 > MAX_BYTES:
            continue
        ops = operands(hip, n, batch, ta, tb, extra_terms=(1, 2, 3, 1), seed=w)
        pool = [ops.a(j) for j in range(w)] + [ops.b(j) for j in range(w)] + [ops.extra(j) for j in range(4)]
        mn, mx = minmax_requests([ops.a(j) for j in range(w)], [ops.b(j) for j in range(w)])
        picks = rng.integers(0, len(pool), (2, 64))
        requests = [([], [], True),
                    ([ops.extra(int(rng.integers(0, 4)))], [ops.extra(int(rng.integers(0, 4)))], False),
                    (mn, mx, True), (mn, mx, False),
                    ([pool[i] for i in picks[0]], [pool[i] for i in picks[1]], True)]
        for xs, ys, less in requests:
            if ops.out_bytes(xs, ys, less) > MAX_BYTES:
                continue
            ops.check_forms(knobs, xs, ys, less)
            ran[tmode] += 1
    assert ran["1"] >= 2, ran                                         # fresh planes: at least the comparison and one request
    assert sum(ran.values()) >= 1


@pytest.mark.parametrize("batch", [1, 257, 4099, (1 << 16) + 3])
def test_lt_select_batches(hip, knobs, batch):
    """Partial last element groups and many groups a launch, in every form.  The largest batch writes one request (55 MB
    at 53 terms an element); the others min, max and the comparison."""
    n, w = 65, 3
    ops = operands(hip, n, batch, [1] * w, [1] * w, seed=batch % 1000)
    if batch > 5000:
        ops.check_forms(knobs, [ops.a(1)], [ops.b(2)], False)
    else:
        mn, mx = minmax_requests([ops.a(j) for j in range(w)], [ops.b(j) for j in range(w)])
        ops.check_forms(knobs, mn, mx, True)


@pytest.mark.parametrize("n,tmode", [(63, "1"), (1247, "1"), (1247, "mixed")])
def test_lt_select_batch_split_over_launches(hip, knobs, n, tmode):
    """Knob launch_blocks lowers the workgroups of one launch, so launch_groups cuts the batch into several launches,
    each with its own operand, request and output offsets; a last launch that is not full."""
    rng = np.random.default_rng(n)
    w, batch = 3, 37
    ops = operands(hip, n, batch, term_counts(tmode, w, rng), term_counts(tmode, w, rng), extra_terms=(2, 3), seed=5)
    xs, ys = [ops.a(0), ops.extra(0), ops.b(1)], [ops.b(0), ops.extra(1), ops.b(1)]
    for blocks in (1, 3, 7):
        knobs.set("launch_blocks", blocks)
        ops.check_forms(knobs, xs, ys, True, (1,))


def test_lt_select_three_subset_tables(hip, knobs):
    """11 planes: three subset tables a side (4 + 4 + 3 planes)."""
    n, w = 129, 11
    ops = operands(hip, n, 1, [1] * w, [1] * w, seed=11)
    ops.check_forms(knobs, [ops.a(10)], [ops.b(0)], False, (-1, 1))


def test_lt_select_unit_slices(hip, knobs):
    """N = 4096 (32 units of 16 bytes a term), w = 9: the smallest width whose subset tables (32 + 16 entries a unit, 24
    KB a set at whole terms) pass the 20 KB a set of the kernel's LDS budget, so subset_plan cuts the terms into two
    slices of 16 units and a workgroup builds its tables for one slice.  (w = 8: 16 + 16 entries, 16 KB, one slice.)"""
    n, w = 4096, 9
    ops = operands(hip, n, 1, [1] * w, [1] * w, seed=9)
    ops.check_forms(knobs, [ops.b(3)], [ops.a(8)], False, (1,))


@pytest.mark.parametrize("n", [5248, 5184])
def test_lt_select_short_last_unit_slice(hip, knobs, n):
    """w = 5: one subset table of 32 entries a set.  N = 5248 is 41 units of 16 bytes a term: 32 x 16 x 41 = 20 992 B
    pass the kernel's 20 480-byte budget, so subset_plan cuts the terms into two slices of 21 units, the last one 20
    units long.  N = 5184 (81 words, odd) is 81 units of 8 bytes: 32 x 8 x 81 = 20 736 B, slices of 41 and 40 units.
    Min and max (requests that alias a and b), whose tail copies walk the same slices, and the comparison."""
    w = 5
    ops = operands(hip, n, 2, [1] * w, [1] * w, seed=n % 100)
    mn, mx = minmax_requests([ops.a(j) for j in range(w)], [ops.b(j) for j in range(w)])
    ops.check_forms(knobs, mn, mx, True, (-1, 1))


@pytest.mark.parametrize("ty", [1, 3])
@pytest.mark.parametrize("same", [True, False], ids=["y_is_b", "y_distinct"])
def test_lt_select_tail_terms(hip, knobs, ty, same):
    """The last ty terms of an output are Y's, copied: Y a plane of b itself (b_1 has ty terms) or a plane apart."""
    n, w, batch = 1247, 3, 5
    ops = operands(hip, n, batch, [1, 2, 1], [1, ty, 2], extra_terms=(2, ty), seed=20 + ty)
    y = ops.b(1) if same else ops.extra(1)
    ops.check_forms(knobs, [ops.extra(0), ops.a(1)], [y, y], False)
    ops.run([ops.extra(0)], [y], True, ops.want([ops.extra(0)], [y], True), shift=1)     # outputs 8 bytes off: 8-byte units


@pytest.mark.parametrize("n,w,tmode", [(1247, 4, "1"), (129, 3, "mixed"), (65, 6, "1")])
def test_chained_steps_and_mux_give_the_same_words(hip, knobs, n, w, tmode):
    """The cross-check nobody can argue with: the LT steps chained through csgn_uint_step and one csgn_gate_uniform MUX
    per request -- the calls select(lessThan(a, b), x, y) issues -- against the fused kernel's outputs, word for word."""
    rng = np.random.default_rng(n + w)
    batch = 7
    ta, tb = term_counts(tmode, w, rng), term_counts(tmode, w, rng)
    ops = operands(hip, n, batch, ta, tb, extra_terms=(1, 3), seed=30)
    Ls = lt_counts(ta, tb)
    lt = hip.uint_step(n, LT_FIRST, batch, ops.dev[0], ta[0], ops.dev[w], tb[0])
    for j in range(1, w):
        lt = hip.uint_step(n, LT_STEP, batch, ops.dev[j], ta[j], ops.dev[w + j], tb[j], x=lt, t_x=Ls[j - 1])
    xs = [ops.a(j) for j in range(w)] + [ops.extra(0), ops.extra(1)]
    ys = [ops.b(j) for j in range(w)] + [ops.extra(1), ops.extra(0)]
    chained = [hip.gate_uniform(n, MUX, batch, ops.dev[x], ops.host[x].shape[1], ops.dev[y], ops.host[y].shape[1],
                                sel=lt, t_sel=Ls[-1]) for x, y in zip(xs, ys)]
    torch.cuda.synchronize()
    knobs.set("uint_lt_select_form", 1)
    assert hip.lib.csgn_uint_lt_select_kernel(n, batch, w, u64s(ta), u64s(tb), 1, u64s([1]), u64s([1]), 1) == b"k_uint_lt_select"
    fused = ops.run(xs, ys, True)
    for i, c in enumerate(chained):
        assert np.array_equal(hip.download(c), fused[i]), i
    assert np.array_equal(hip.download(lt), fused[-1])


def test_lt_select_decrypts(hip, knobs, oracle):
    """min, max and both payloads of a compare-exchange, against integers; a tie takes Y (lo = b, plo = pb)."""
    n, d, pw = 127, 8, 3
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(701, 64 * d + 64))
    rng = np.random.default_rng(702)
    knobs.unset("uint_lt_select_form")
    for w, batch in [(1, 5), (3, 100), (4, 333), (8, 16)]:
        av = rng.integers(0, 1 << w, batch).astype(np.uint64)
        bv = rng.integers(0, 1 << w, batch).astype(np.uint64)
        bv[::4] = av[::4]                                             # ties
        pav = rng.integers(0, 1 << pw, batch).astype(np.uint64)
        pbv = pav ^ np.uint64(5)
        a, b = encrypt_planes(oracle, n, key, av, w, 710 + w), encrypt_planes(oracle, n, key, bv, w, 720 + w)
        pa, pb = encrypt_planes(oracle, n, key, pav, pw, 730 + w), encrypt_planes(oracle, n, key, pbv, pw, 740 + w)
        ops = Operands(hip, n, a, b, pa + pb)
        mn, mx = minmax_requests([ops.a(j) for j in range(w)], [ops.b(j) for j in range(w)])
        pl, ph = minmax_requests([ops.extra(j) for j in range(pw)], [ops.extra(pw + j) for j in range(pw)])
        got = [o.reshape(batch, -1, dl) for o in ops.run(mn + pl, mx + ph, True)]
        lo, hi = got[:w], got[w:2 * w]
        plo, phi = got[2 * w:2 * w + pw], got[2 * w + pw:2 * w + 2 * pw]
        less = av < bv
        assert np.array_equal(decrypt_value(oracle, n, key, lo), np.minimum(av, bv)), w
        assert np.array_equal(decrypt_value(oracle, n, key, hi), np.maximum(av, bv)), w
        assert np.array_equal(decrypt_value(oracle, n, key, plo), np.where(less, pav, pbv)), w
        assert np.array_equal(decrypt_value(oracle, n, key, phi), np.where(less, pbv, pav)), w
        assert np.array_equal(decrypt_bits(oracle, n, key, got[-1]), less), w


def test_lt_select_graph_capture_and_replay(hip, knobs):
    n, w, batch = 1247, 6, 37
    ops = operands(hip, n, batch, [1] * w, [1] * w, extra_terms=(1, 2), seed=40)
    xs, ys = [ops.a(0), ops.b(5), ops.extra(0), ops.extra(1)], [ops.b(0), ops.a(5), ops.extra(1), ops.a(2)]
    want = ops.want(xs, ys, True)
    knobs.set("uint_lt_select_form", 1)
    outs = [hip.empty_words(x.size) for x in want]
    call = lambda: ops.call(xs, ys, outs[:4], outs[4])                # noqa: E731
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
    for j in range(5):
        assert np.array_equal(hip.download(outs[j]), want[j]), j


def test_lt_select_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    cmp_out = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 64)(*([buf.data_ptr()] * 64))
    nullp = (C.c_void_p * 64)(*([buf.data_ptr()] * 3 + [None] + [buf.data_ptr()] * 60))
    one = u64s([1] * 64)
    st = hip.stream

    def sel(n=1247, batch=1, w=4, a=ptrs, ta=one, b=ptrs, tb=one, m=4, x=ptrs, tx=one, y=ptrs, ty=one, out=ptrs,
            less=None):
        return lib.csgn_uint_lt_select(n, batch, w, a, ta, b, tb, m, x, tx, y, ty, out, less, st)

    assert sel(n=0) == -1                                             # n_bits
    assert sel(w=0) == -1 and sel(w=17) == -1                         # width
    assert sel(m=65) == -1 and sel(m=0) == -1                         # requests; none without the comparison
    for arg in ("a", "ta", "b", "tb", "x", "tx", "y", "ty", "out"):   # host pointers
        assert sel(**{arg: None}) == -1, arg
    assert sel(ta=u64s([1, 0, 1, 1])) == -1 and sel(tb=u64s([1, 1, 1, 0])) == -1   # 0 terms
    assert sel(tx=u64s([1, 0, 1, 1])) == -1 and sel(ty=u64s([0, 1, 1, 1])) == -1
    assert sel(ta=u64s([1 << 61] * 4)) == -1                          # 2^62
    for arg in ("a", "b", "x", "y", "out"):                           # a null device pointer inside each host array
        assert sel(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert sel(m=3, x=nullp, y=nullp, out=nullp, batch=0) == 0        # past the requests: not read
    assert sel(w=16, m=1, tx=u64s([3])) == -2                         # 2^31 words
    assert sel(w=16, m=0, less=cmp_out.data_ptr(), ta=u64s([2] * 16)) == -2
    assert sel(w=8, batch=1 << 44) == -2                              # batch
    assert sel(batch=0) == 0                                          # empty batch
    assert sel(batch=0, m=0, x=None, tx=None, y=None, ty=None, out=None, less=cmp_out.data_ptr()) == 0
