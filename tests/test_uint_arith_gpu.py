"""a + b, a - b, a == b and a != b of encrypted integers on the device (csgn_uint_arith), word for word against the
per-bit chains of tests/model.py (shown equal to the definition by position in tests/test_uint_arith_cpu.py), in both
forms the knob uint_arith_form selects; the cross-check against the chained csgn_uint_step / csgn_gate_uniform calls a
user issues today; decryptions; graph capture.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import (ADD_FULL, ADD_HALF, EQ_STEP, NOT, XNOR, GuardedOutputs, decrypt_bits, decrypt_value,
                         encrypt_planes, hip, rand_terms, u64s)  # noqa: F401
from tests.model_arith import ADD, EQ, NE, OPS, SUB, arith_counts, np_arith_chain

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs: the numpy side, not the device, is the limit


def terms_of(planes):
    return [p.shape[1] for p in planes]


class Operands:
    """a and b on the host and, uploaded once, on the device; b may BE a (the same device pointers)."""

    def __init__(self, hip, n, a, b=None):
        self.hip, self.n, self.w, self.batch = hip, n, len(a), a[0].shape[0]
        self.a, self.b = a, a if b is None else b
        self.da = [hip.upload(p.ravel()) for p in a]
        self.db = self.da if b is None else [hip.upload(p.ravel()) for p in b]
        self.ta, self.tb = terms_of(self.a), terms_of(self.b)
        self.wants = {}

    def want(self, op, carry):
        """The reference, computed once for (op, carry) and left unchanged."""
        if (op, carry) not in self.wants and (op, True) in self.wants:
            self.wants[op, carry] = self.wants[op, True][:-1]          # the planes do not depend on the carry
        if (op, carry) not in self.wants:
            outs, c = np_arith_chain(self.n, op, self.a, self.b, carry)
            self.wants[op, carry] = [o.ravel() for o in outs] + ([c.ravel()] if carry else [])
        return self.wants[op, carry]

    def out_bytes(self, op, carry):
        T, _ = arith_counts(op, self.ta, self.tb)
        terms = sum(T) if carry or op in (EQ, NE) else sum(T[:-1])
        return self.batch * terms * ((self.n + 63) // 64) * 8

    def call(self, op, outs, carry):
        return self.hip.uint_arith(self.n, op, self.batch, self.da, self.ta, self.db, self.tb, outs=outs, carry=carry)

    def run(self, op, carry, want=None, shift=0):
        """The outputs and the carry (last, when asked for), downloaded.  With `want` they are caller tensors of exactly
        those sizes between guard words, checked word for word and for writes outside them (GuardedOutputs)."""
        m = self.w if op in (ADD, SUB) else 1
        guarded = GuardedOutputs(self.hip, [x.size for x in want], shift) if want is not None else None
        outs, c = self.call(op, guarded.outs[:m] if guarded else None, (guarded.outs[m] if guarded else True) if carry else False)
        torch.cuda.synchronize()
        if guarded:
            return guarded.check(want, (op, self.ta, self.tb, carry))
        return [self.hip.download(o) for o in outs] + ([self.hip.download(c)] if carry else [])

    def check_forms(self, knobs, op, carry, forms=(-1, 0, 1), shift=0):
        want = self.want(op, carry)
        for form in forms:
            knobs.set("uint_arith_form", form)
            self.run(op, carry, want, shift)                           # GuardedOutputs.check asserts every word

    def check_all(self, knobs, forms=(-1, 0, 1), ops=tuple(OPS.values())):
        """Every op, the sums with and without the carry."""
        for op in ops:
            for carry in ((True, False) if op in (ADD, SUB) else (False,)):
                self.check_forms(knobs, op, carry, forms)


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


def operands(hip, n, batch, ta, tb=None, seed=0):
    a = [rand_terms(n, batch, t, seed + 400 + 7 * k + t) for k, t in enumerate(ta)]
    b = None if tb is None else [rand_terms(n, batch, t, seed + 450 + 5 * k + t) for k, t in enumerate(tb)]
    return Operands(hip, n, a, b)


# 63 and 129: odd dL, the 8-byte-unit kernel; 65 and 1247 / 4096: 16-byte units; 5 -> 6 planes: one -> two subset tables
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("w", [1, 2, 3, 5, 6, 8])
def test_arith_words(hip, knobs, n, w):
    """Every term mode at one (N, width), every op, the sums with and without the carry, in every form.  A call whose
    outputs pass 48 MB is skipped; fresh planes run all four ops at every (N, width)."""
    batch = 2
    ran = {}
    for tmode in ("1", "2", "mixed", "afresh"):
        rng = np.random.default_rng(w * 100 + n + len(tmode))
        ta, tb = term_counts(tmode, w, rng, fresh=True), term_counts(tmode, w, rng)
        ops = operands(hip, n, batch, ta, tb, seed=w)
        ran[tmode] = set()
        for op in OPS.values():
            for carry in ((True, False) if op in (ADD, SUB) else (False,)):
                if ops.out_bytes(op, carry) > MAX_BYTES:
                    continue
                ops.check_forms(knobs, op, carry)
                ran[tmode].add((op, carry))
    assert len(ran["1"]) == 6, ran                                    # fresh planes: everything ran


@pytest.mark.parametrize("batch", [1, 257, 4099, (1 << 16) + 3])
def test_arith_batches(hip, knobs, batch):
    """Partial last element groups and many groups a launch, in every form: 27 (EQ) to 32 (SUB with its carry) terms an
    element."""
    ops = operands(hip, 65, batch, [1] * 3, [1] * 3, seed=batch % 1000)
    ops.check_all(knobs)


@pytest.mark.parametrize("n,tmode", [(63, "1"), (1247, "1"), (1247, "mixed")])
def test_arith_batch_split_over_launches(hip, knobs, n, tmode):
    """Knob launch_blocks lowers the workgroups of one launch, so launch_groups cuts the batch into several launches,
    each with its own operand and output offsets; a last launch that is not full."""
    rng = np.random.default_rng(n)
    w, batch = 3, 37
    ops = operands(hip, n, batch, term_counts(tmode, w, rng), term_counts(tmode, w, rng), seed=5)
    for blocks in (1, 3, 7):
        knobs.set("launch_blocks", blocks)
        ops.check_all(knobs, (1,))


def test_arith_three_subset_tables(hip, knobs):
    """11 planes: three subset tables a side (4 + 4 + 3 planes); the stream of a sum crosses outputs inside a part."""
    ops = operands(hip, 129, 1, [1] * 11, [1] * 11, seed=11)
    ops.check_all(knobs, (-1, 1))


def test_arith_unit_slices(hip, knobs):
    """N = 4096 (32 units of 16 bytes a term), w = 9: the smallest width whose subset tables (32 + 16 entries a unit, 24
    KB a set at whole terms) pass the 20 KB a set of the kernel's LDS budget, so subset_plan cuts the terms into two
    slices of 16 units and a workgroup builds its tables for one slice."""
    ops = operands(hip, 4096, 1, [1] * 9, [1] * 9, seed=9)
    ops.check_all(knobs, (1,))


@pytest.mark.parametrize("n", [5248, 5184])
def test_arith_short_last_unit_slice(hip, knobs, n):
    """w = 5: one subset table of 32 entries a set.  N = 5248 is 41 units of 16 bytes a term: two slices of 21 units,
    the last one 20 units long.  N = 5184 (81 words, odd) is 81 units of 8 bytes: slices of 41 and 40 units."""
    ops = operands(hip, n, 2, [1] * 5, [1] * 5, seed=n % 100)
    ops.check_all(knobs, (-1, 1))


@pytest.mark.parametrize("tmode", ["1", "mixed"])
def test_arith_b_is_a(hip, knobs, tmode):
    """a + a, a - a, equalTo(a, a): both operands the very same device planes."""
    rng = np.random.default_rng(77)
    ops = operands(hip, 1247, 5, term_counts(tmode, 4, rng), None, seed=70)
    ops.check_all(knobs)


@pytest.mark.parametrize("n", [1247, 129])
def test_arith_outputs_8_bytes_off(hip, knobs, n):
    """Outputs that start 8 bytes off a 16-byte boundary: the 8-byte units, also where dL is even."""
    ops = operands(hip, n, 5, [1, 2, 1], [1, 1, 2], seed=20)
    fresh = operands(hip, n, 5, [1] * 3, [1] * 3, seed=21)
    for o in (ops, fresh):
        for op in OPS.values():
            o.check_forms(knobs, op, op in (ADD, SUB), shift=1)


@pytest.mark.parametrize("n,w,tmode", [(1247, 4, "1"), (129, 3, "mixed"), (65, 6, "1")])
def test_chained_steps_give_the_same_words(hip, knobs, n, w, tmode):
    """The cross-check nobody can argue with: the steps chained through csgn_uint_step and csgn_gate_uniform -- the
    calls operator+, operator-, equalTo and notEqualTo issued -- against the one launch, word for word."""
    rng = np.random.default_rng(n + w)
    batch = 7
    ta, tb = term_counts(tmode, w, rng), term_counts(tmode, w, rng)
    ops = operands(hip, n, batch, ta, tb, seed=30)
    _, Ca = arith_counts(ADD, ta, tb)
    _, Cs = arith_counts(SUB, ta, tb)
    s, c = hip.uint_step(n, ADD_HALF, batch, ops.da[0], ta[0], ops.db[0], tb[0])
    add = [s]
    for j in range(1, w):
        s, c = hip.uint_step(n, ADD_FULL, batch, ops.da[j], ta[j], ops.db[j], tb[j], x=c, t_x=Ca[j - 1])
        add.append(s)
    add.append(c)
    c, sub = hip.const_fill(n, batch), []
    for j in range(w):
        nb = hip.gate_uniform(n, NOT, batch, ops.db[j], tb[j])
        s, c = hip.uint_step(n, ADD_FULL, batch, ops.da[j], ta[j], nb, tb[j] + 1, x=c, t_x=Cs[j - 1] if j else 1)
        sub.append(s)
    sub.append(c)
    e, te = hip.gate_uniform(n, XNOR, batch, ops.da[0], ta[0], ops.db[0], tb[0]), ta[0] + tb[0] + 1
    for j in range(1, w):
        e = hip.uint_step(n, EQ_STEP, batch, ops.da[j], ta[j], ops.db[j], tb[j], x=e, t_x=te)
        te *= ta[j] + tb[j] + 1
    ne = hip.gate_uniform(n, NOT, batch, e, te)
    torch.cuda.synchronize()
    knobs.set("uint_arith_form", 1)
    for op, chained in ((ADD, add), (SUB, sub), (EQ, [e]), (NE, [ne])):
        carry = op in (ADD, SUB)
        assert hip.lib.csgn_uint_arith_kernel(n, op, batch, w, u64s(ta), u64s(tb), int(carry)) == b"k_uint_arith"
        fused = ops.run(op, carry)
        assert len(fused) == len(chained)
        for i, x in enumerate(chained):
            assert np.array_equal(hip.download(x), fused[i]), (op, i)


def test_arith_decrypts(hip, knobs, oracle):
    """a + b and a - b mod 2^w with both carries, and a == b / a != b with planted ties, against integers."""
    n, d = 127, 8
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(801, 64 * d + 64))
    rng = np.random.default_rng(802)
    knobs.unset("uint_arith_form")
    for w, batch in [(1, 5), (3, 100), (4, 333), (8, 16)]:
        av = rng.integers(0, 1 << w, batch).astype(np.uint64)
        bv = rng.integers(0, 1 << w, batch).astype(np.uint64)
        bv[::4] = av[::4]                                             # ties
        a, b = encrypt_planes(oracle, n, key, av, w, 810 + w), encrypt_planes(oracle, n, key, bv, w, 820 + w)
        ops = Operands(hip, n, a, b)
        mask = np.uint64((1 << w) - 1)
        got = [o.reshape(batch, -1, dl) for o in ops.run(ADD, True)]
        assert np.array_equal(decrypt_value(oracle, n, key, got[:w]), (av + bv) & mask), w
        assert np.array_equal(decrypt_bits(oracle, n, key, got[w]), (av + bv) >> np.uint64(w) != 0), w
        got = [o.reshape(batch, -1, dl) for o in ops.run(SUB, True)]
        assert np.array_equal(decrypt_value(oracle, n, key, got[:w]), (av - bv) & mask), w
        assert np.array_equal(decrypt_bits(oracle, n, key, got[w]), av >= bv), w
        assert np.array_equal(decrypt_bits(oracle, n, key, ops.run(EQ, False)[0].reshape(batch, -1, dl)), av == bv), w
        assert np.array_equal(decrypt_bits(oracle, n, key, ops.run(NE, False)[0].reshape(batch, -1, dl)), av != bv), w


@pytest.mark.parametrize("op", list(OPS.values()), ids=list(OPS))
def test_arith_graph_capture_and_replay(hip, knobs, op):
    n, w, batch = 1247, 6, 37
    ops = operands(hip, n, batch, [1] * w, [1] * w, seed=40)
    carry = op in (ADD, SUB)
    want = ops.want(op, carry)
    knobs.set("uint_arith_form", 1)
    outs = [hip.empty_words(x.size) for x in want]
    m = len(outs) - int(carry)
    call = lambda: ops.call(op, outs[:m], outs[m] if carry else False)   # noqa: E731
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
    for j in range(len(outs)):
        assert np.array_equal(hip.download(outs[j]), want[j]), j


def test_arith_argument_errors(hip):
    lib = hip.lib
    buf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    cbuf = hip.upload(np.zeros(64 * 64, dtype=np.uint64))
    ptrs = (C.c_void_p * 17)(*([buf.data_ptr()] * 17))
    nullp = (C.c_void_p * 17)(*([buf.data_ptr()] * 3 + [None] + [buf.data_ptr()] * 13))
    one = u64s([1] * 17)
    st = hip.stream

    def arith(n=1247, op=ADD, batch=1, w=4, a=ptrs, ta=one, b=ptrs, tb=one, out=ptrs, carry=None):
        return lib.csgn_uint_arith(n, op, batch, w, a, ta, b, tb, out, carry, st)

    assert arith(n=0) == -1                                           # n_bits
    assert arith(op=0) == -1 and arith(op=5) == -1                    # the op
    assert arith(w=0) == -1 and arith(w=17) == -1                     # width
    for arg in ("a", "ta", "b", "tb", "out"):                         # host pointers
        assert arith(**{arg: None}) == -1, arg
    assert arith(op=EQ, carry=cbuf.data_ptr()) == -1 and arith(op=NE, carry=cbuf.data_ptr()) == -1
    assert arith(ta=u64s([1, 0, 1, 1])) == -1 and arith(tb=u64s([1, 1, 1, 0])) == -1   # 0 terms
    assert arith(ta=u64s([1 << 61] * 4)) == -1                        # 2^62
    for arg in ("a", "b", "out"):                                     # a null device pointer inside each host array
        assert arith(**{arg: nullp}) == -1, arg
        assert b"null device pointer" in lib.csgn_last_error(), arg
    assert arith(w=3, a=nullp, b=nullp, out=nullp, batch=0) == 0      # past the planes: not read
    assert arith(op=EQ, out=nullp, batch=0) == 0                      # a comparison reads one output pointer
    assert arith(op=EQ, w=16, ta=u64s([2] * 16)) == -2                # 2^31 words
    assert arith(op=ADD, w=1, ta=u64s([1 << 14]), tb=u64s([1 << 14]), carry=cbuf.data_ptr()) == -2
    assert arith(w=8, batch=1 << 52) == -2                            # batch
    assert arith(batch=0) == 0 and arith(op=SUB, batch=0, carry=cbuf.data_ptr()) == 0   # empty batch
