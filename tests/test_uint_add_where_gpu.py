"""a + (s ? k : 0) on the device (csgn_uint_add_where): every call writes into GuardedOutputs of exactly the documented
sizes and is checked word for word against the numpy composition of include/csgn_hip.h's table (shown equal to the
decode by position, the oracle and the reference in tests/test_uint_add_where_cpu.py); batches, aliased and misaligned
operands, the host's split, the chain of csgn_add_uniform / csgn_mul_uniform calls a user issues today, decryptions,
graph capture.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.binding import glibc_draws
from tests.model import GuardedOutputs, decrypt_bits, decrypt_value, encrypt_planes, hip, rand_terms, u64s  # noqa: F401
from tests.model_add_where import add_where_counts, clear_add_where, np_add_where_compose

pytestmark = pytest.mark.gpu

MAX_BYTES = 48 << 20                    # of one call's outputs: the numpy side, not the device, is the limit


def term_counts(mode, w, rng):
    """(ta, ts): fresh; ts = 2 over a fresh a; all drawn from 1..3; all 2; fresh except plane 3 of 2 terms."""
    if mode == "fresh":
        return [1] * w, 1
    if mode == "ts2":
        return [1] * w, 2
    if mode == "all2":
        return [2] * w, 2
    if mode == "plane3":
        return [2 if j == 3 else 1 for j in range(w)], 1
    return [int(x) for x in rng.integers(1, 4, w)], int(rng.integers(1, 4))


def moved(hip, a, shift):
    """Device copy of the words; with shift = 1 it starts 8 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a).ravel()
    t = hip.upload(np.concatenate([np.zeros(shift, np.uint64), a]))[shift:]
    assert t.data_ptr() % 16 == 8 * shift
    return t


class Case:
    """An integer a and a flag s on the host and, uploaded once, on the device.  alias: s IS plane 0 of a (the same
    device pointer) and plane 2 IS plane 1."""

    def __init__(self, hip, n, batch, ta, ts, k, seed=0, shift=0, alias=False):
        self.hip, self.n, self.batch, self.w, self.k = hip, n, batch, len(ta), k
        self.a = [rand_terms(n, batch, t, seed + 500 + 7 * j + t) for j, t in enumerate(ta)]
        self.s = rand_terms(n, batch, ts, seed + 499)
        self.da = [moved(hip, p, shift) for p in self.a]
        self.ds = moved(hip, self.s, shift)
        if alias:
            assert self.w >= 3 and ta[1] == ta[2]
            self.s, self.ds = self.a[0], self.da[0]
            self.a[2], self.da[2] = self.a[1], self.da[1]
        self.ta, self.ts = ta, self.s.shape[1]
        self.T, _ = add_where_counts(self.ta, self.ts, k)
        self.dl = (n + 63) // 64
        self.wants = None

    def out_bytes(self, carry):
        return self.batch * sum(self.T if carry else self.T[:-1]) * self.dl * 8

    def want(self, carry):
        """The reference, computed once and left unchanged."""
        if self.wants is None:
            outs, c = np_add_where_compose(self.n, self.a, self.s, self.k)
            self.wants = [o.ravel() for o in outs] + [np.ascontiguousarray(c).ravel()]
            assert [x.size for x in self.wants] == [self.batch * t * self.dl for t in self.T]
        return self.wants if carry else self.wants[:-1]

    def call(self, outs, carry):
        return self.hip.uint_add_where(self.n, self.batch, self.da, self.ta, self.ds, self.ts, self.k, outs=outs, carry=carry)

    def check(self, carry, shift=0):
        """One call into guarded outputs of exactly the documented sizes, every word asserted."""
        assert self.out_bytes(carry) < MAX_BYTES, (self.w, self.k, self.ta, self.ts, self.out_bytes(carry))
        want = self.want(carry)
        g = GuardedOutputs(self.hip, [x.size for x in want], shift)
        self.call(g.outs[:self.w], g.outs[self.w] if carry else False)
        torch.cuda.synchronize()
        return g.check(want, (self.n, self.w, hex(self.k), self.ta, self.ts, carry))


SMALL = [(1, 0), (1, 1), (2, 2), (3, 5), (5, 0x1F), (5, 0x14)]
WIDE = [(17, 1), (17, 0x10001), (32, 1), (32, 0x80000001), (32, 0xFF000000)]
SHAPES = ([(w, k, ("fresh", "ts2", "mixed")) for w, k in SMALL] +
          [(8, 1, ("fresh", "ts2", "mixed")), (8, 0x80, ("fresh", "ts2", "mixed", "all2")),
           (8, 0xA5, ("fresh", "ts2", "all2")), (8, 0xFF, ("fresh", "ts2"))] +
          [(w, k, ("fresh", "ts2", "plane3")) for w, k in WIDE])


# 63 and 129: odd dL, the 8-byte units; 65 and 1247 / 4096: 16-byte units, dL = 2, the workload's N, 32 units a term
@pytest.mark.parametrize("n", [63, 65, 129, 1247, 4096])
@pytest.mark.parametrize("w,k,modes", SHAPES, ids=["%d-%x" % (w, k) for w, k, _ in SHAPES])
def test_add_where_words(hip, n, w, k, modes):
    """Every term mode of the shape, with and without the carry: the copies below the lowest set bit, a k_j = 0 level
    between two set bits, entries with several terms of s, ranges that cross outputs, widths on both sides of 16, the
    staged form (fresh a) and the walk (planes of several terms).  No case is skipped: every call's output bytes are
    asserted below 48 MB."""
    for mode in modes:
        rng = np.random.default_rng(1000 * w + k % 997 + n)
        ta, ts = term_counts(mode, w, rng)
        case = Case(hip, n, 2, ta, ts, k, seed=w)
        for carry in (True, False):
            case.check(carry)


@pytest.mark.parametrize("mode", ["fresh", "ts2"])
@pytest.mark.parametrize("batch", [1, 257, 4099, 65539])
def test_add_where_batches(hip, batch, mode):
    """Partial last element groups and many groups a launch: (5, 0x13) at N = 65, planes of 18 (fresh) or 37 (ts = 2)
    terms an element and a carry of 7 or 26.  Every call stays under the 48 MB cap but one: with ts = 2 the planes AND
    the carry of 65 539 elements are 63 terms of 16 bytes each, 66 MB, so that batch checks the carry with fresh operands
    (26 MB) and the planes alone with ts = 2 (39 MB)."""
    ta, ts = term_counts(mode, 5, None)
    case = Case(hip, 65, batch, ta, ts, 0x13, seed=batch % 1000)
    if case.out_bytes(True) < MAX_BYTES:
        case.check(True)
    else:
        assert (batch, mode) == (65539, "ts2")
    case.check(False)


@pytest.mark.parametrize("n", [1247, 129])
@pytest.mark.parametrize("mode", ["fresh", "all2"])
def test_add_where_aliased_operands(hip, n, mode):
    """d_sel is the same device pointer as a_0, and planes 1 and 2 of a are one pointer: the words of the definition
    with equal operands."""
    ta, ts = term_counts(mode, 4, None)
    for k in (0xB, 0x6):
        Case(hip, n, 5, ta, ts, k, seed=60, alias=True).check(True)


def test_add_where_8_bytes_off(hip):
    """Operands and outputs begin 8 bytes past a 16-byte boundary with even dL: the 8-byte units."""
    case = Case(hip, 1247, 3, [1] * 8, 1, 0xA5, seed=20, shift=1)
    case.check(True, shift=1)
    case.check(False, shift=1)


def test_add_where_split_over_launches(hip, knobs):
    """Knob launch_blocks lowers the workgroups of one launch, so launch_groups cuts the batch into several launches,
    each with its own operand and output offsets; a last launch that is not full.  The words must be the same."""
    case = Case(hip, 65, 64, [1] * 8, 1, 0xFF, seed=5)
    for blocks in (1, 3, 7):
        knobs.set("launch_blocks", blocks)
        case.check(True)
    walk = Case(hip, 65, 37, [1, 2, 1], 2, 0x5, seed=6)
    for blocks in (1, 3):
        knobs.set("launch_blocks", blocks)
        walk.check(True)


@pytest.mark.parametrize("w,k", [(8, 0xA5), (16, 1)])
@pytest.mark.parametrize("mode", ["fresh", "ts2"])
def test_chained_library_calls_give_the_same_words(hip, w, k, mode):
    """The chain of csgn_add_uniform / csgn_mul_uniform calls the class-level loop issues, entry points of the parent
    commit, against the one launch, word for word."""
    n, batch = 1247, 7
    ta, ts = term_counts(mode, w, None)
    case = Case(hip, n, batch, ta, ts, k, seed=30)
    add = lambda x, tx, y, ty: (hip.add_uniform(n, batch, tx, ty, x, y), tx + ty)        # noqa: E731
    mul = lambda x, tx, y, ty: (hip.mul_uniform(n, batch, tx, ty, x, y), tx * ty)        # noqa: E731
    m = (k & -k).bit_length() - 1
    chained, c = [], None
    for j in range(w):
        aj, s = (case.da[j], ta[j]), (case.ds, ts)
        if j < m:
            chained.append(aj)
        elif j == m:
            chained.append(add(*aj, *s))
            c = mul(*aj, *s)
        elif (k >> j) & 1:
            ab = add(*aj, *s)
            chained.append(add(*ab, *c))
            c = add(*mul(*aj, *s), *mul(*ab, *c))
        else:
            chained.append(add(*aj, *c))
            c = mul(*aj, *c)
    chained.append(c)
    torch.cuda.synchronize()
    assert [t for _, t in chained] == case.T
    got = case.check(True)
    for o, (x, t) in enumerate(chained):
        assert np.array_equal(hip.download(x)[: batch * t * case.dl], got[o]), o


def test_add_where_decrypts(hip, oracle):
    """N = 1247, d = 16, 64 elements with random values and flags: planes and carry decrypt to clear arithmetic, and
    so does a second increment applied to the first one's result, whose planes are no longer fresh (w = 8: at w = 32
    the carries of two-term planes double a plane, 2^32 terms at the top, and the call refuses the shape)."""
    n, d, count = 1247, 16, 64
    dl = (n + 63) // 64
    key, _ = oracle.keygen(n, d, glibc_draws(901, 64 * d + 64))
    rng = np.random.default_rng(902)
    for w, ks in ((8, (1, 0x80, 0xA5)), (32, (1, 0x80, 0x80000001))):
        xs = rng.integers(0, 1 << w, count).astype(np.uint64)
        xs[:4] = [(1 << w) - 1, (1 << w) - 1, 0, (1 << w) - 2]       # the carry leaves, and does not
        fs = rng.integers(0, 2, count).astype(np.uint64)
        fs[:4] = [1, 0, 1, 1]
        a = encrypt_planes(oracle, n, key, xs, w, 910 + w)
        s = encrypt_planes(oracle, n, key, fs, 1, 940 + w)[0]
        da, ds = [hip.upload(p.ravel()) for p in a], hip.upload(s.ravel())
        for k in ks:
            outs, carry = hip.uint_add_where(n, count, da, [1] * w, ds, 1, k, carry=True)
            torch.cuda.synchronize()
            T, _ = add_where_counts([1] * w, 1, k)
            got = [hip.download(o).reshape(count, t, dl) for o, t in zip(outs + [carry], T)]
            want = [clear_add_where(int(x), int(f), k, w) for x, f in zip(xs, fs)]
            assert np.array_equal(decrypt_value(oracle, n, key, got[:w]), np.array([v for v, _ in want], dtype=np.uint64)), (w, k)
            assert np.array_equal(decrypt_bits(oracle, n, key, got[w]), np.array([c for _, c in want]) != 0), (w, k)
            if k != 1:
                continue
            if w == 32:
                p = (C.c_void_p * w)(*[o.data_ptr() for o in outs])
                assert hip.lib.csgn_uint_add_where(n, count, w, 1, ds.data_ptr(), 1, p, u64s(T[:w]), p, None, hip.stream) == -2
                continue
            outs2, carry2 = hip.uint_add_where(n, count, outs, T[:w], ds, 1, 1, carry=True)
            torch.cuda.synchronize()
            T2, _ = add_where_counts(T[:w], 1, 1)
            got2 = [hip.download(o).reshape(count, t, dl) for o, t in zip(outs2 + [carry2], T2)]
            twice = [clear_add_where(v, int(f), 1, w) for (v, _), f in zip(want, fs)]
            assert np.array_equal(decrypt_value(oracle, n, key, got2[:w]), np.array([v for v, _ in twice], dtype=np.uint64))
            assert np.array_equal(decrypt_bits(oracle, n, key, got2[w]), np.array([c for _, c in twice]) != 0)


@pytest.mark.parametrize("w,k,mode", [(32, 1, "fresh"), (8, 0xA5, "all2")])
def test_add_where_graph_capture_and_replay(hip, w, k, mode):
    """One call captured, replayed once and compared; the runtime's defaults."""
    n, batch = 1247, 37
    ta, ts = term_counts(mode, w, None)
    case = Case(hip, n, batch, ta, ts, k, seed=40)
    want = case.want(True)
    outs = [hip.empty_words(x.size) for x in want]
    call = lambda: case.call(outs[:w], outs[w])                       # noqa: E731
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
