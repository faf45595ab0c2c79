"""Sums of comparisons of an encrypted integer against public constants on the device (csgn_uint_plain_sum): every call
writes into GuardedOutputs of exactly the documented sizes and is checked word for word against the numpy composition
of include/csgn_hip.h's definition (shown equal to the decode by position, the oracle and the reference in
tests/test_uint_plain_sum_cpu.py, which also replays these shapes' grids on the host); aliased and misaligned operands,
the host's split, the XCD order, graph capture, one plan for two batches.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests.model import EQ, GE, GT, LE, LT, NE, GuardedOutputs, hip, rand_terms  # noqa: F401
from tests.model_plain_sum import NS, gpu_shapes, np_plain_sum, sum_terms

pytestmark = pytest.mark.gpu


def moved(hip, a, shift):
    """Device copy of the words; with shift = 1 it starts 8 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a).ravel()
    t = hip.upload(np.concatenate([np.zeros(shift, np.uint64), a]))[shift:]
    assert t.data_ptr() % 16 == 8 * shift
    return t


class Case:
    """Input planes on the host and, uploaded once, on the device; the reference computed once and left unchanged.
    alias: plane 1 IS plane 0 (the same device pointer)."""

    def __init__(self, hip, n, batch, ta, planes_entries, constant, seed=0, shift=0, alias=False):
        self.hip, self.n, self.batch, self.ta, self.entries, self.constant = hip, n, batch, list(ta), planes_entries, constant
        self.a = [rand_terms(n, batch, t, seed + 700 + 13 * j + t) for j, t in enumerate(ta)]
        self.da = [moved(hip, p, shift) for p in self.a]
        if alias:
            assert len(ta) >= 2 and ta[0] == ta[1]
            self.a[1], self.da[1] = self.a[0], self.da[0]
        self.want = [o.ravel() for o in np_plain_sum(n, self.a, planes_entries, constant)]
        dl = (n + 63) // 64
        T = [sum_terms(self.ta, e, (constant >> x) & 1) for x, e in enumerate(planes_entries)]
        assert [x.size for x in self.want] == [batch * t * dl for t in T]

    def check(self, shift=0):
        """One call into guarded outputs of exactly the documented sizes, every word asserted."""
        g = GuardedOutputs(self.hip, [x.size for x in self.want], shift)
        self.hip.uint_plain_sum(self.n, self.batch, self.da, self.ta, self.entries, self.constant, outs=g.outs)
        torch.cuda.synchronize()
        return g.check(self.want, (self.n, self.batch, self.ta, self.entries, hex(self.constant), shift))


SHAPES = gpu_shapes()


def shape(name):
    return next(s for s in SHAPES if s[0] == name)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_plain_sum_words(hip, n, shape):
    """Ranges at w = 3 and 8; all six comparisons in one plane; ZERO entries; empty planes and the constant alone; a
    single entry; 1-term entries; entries of 15, 16 and 17 terms; an entry ending at a workgroup's last item; planes of
    2 and 3 terms; w = 1, 33 and 64; 300 entries in a plane; 64 planes.  Batches 1, 3 and 257."""
    name, ta, planes_entries, constant, batches = shape
    for batch in batches:
        Case(hip, n, batch, ta, planes_entries, constant, seed=len(ta)).check()


@pytest.mark.parametrize("n", [1247, 1300])
def test_plain_sum_misaligned(hip, n):
    """Inputs, outputs, or both one word off 16-byte alignment: 8-byte units at an even word count too."""
    for name in ("mixed", "runs", "t23", "ones"):
        _, ta, planes_entries, constant, batches = shape(name)
        for in_shift, out_shift in ((1, 0), (0, 1), (1, 1)):
            Case(hip, n, batches[1], ta, planes_entries, constant, seed=3, shift=in_shift).check(out_shift)


def test_plain_sum_aliased_inputs(hip):
    """Two input planes that are the same pointer."""
    for n in NS:
        for name in ("mixed", "t23"):
            _, ta, planes_entries, constant, _ = shape(name)
            ta = [ta[0]] + ta[:1] + ta[2:]
            Case(hip, n, 5, ta, planes_entries, constant, alias=True).check()


def test_plain_sum_launch_caps(hip, knobs):
    """launch_blocks caps that cut the call into 2 and 3 launches (cut at elements), the count asserted from the host
    query, and a cap below one element's workgroups (an element still goes whole)."""
    for name in ("mixed", "t23", "planes64"):
        _, ta, planes_entries, constant, _ = shape(name)
        case = Case(hip, 1247, 40, ta, planes_entries, constant, seed=17)
        knobs.set("launch_blocks", 0)
        whole = hip.uint_plain_sum_launches(1247, 40, ta, planes_entries, constant)
        assert whole[3] == 1
        case.check()
        for want in (2, 3):
            per = -(-40 // want)
            knobs.set("launch_blocks", -(-per * whole[1] // 256) + len(planes_entries))
            assert hip.uint_plain_sum_launches(1247, 40, ta, planes_entries, constant)[3] == want
            case.check()
        knobs.set("launch_blocks", 1)
        assert hip.uint_plain_sum_launches(1247, 40, ta, planes_entries, constant)[3] == 40
        case.check()


def test_plain_sum_xcd_order_at_small_grids(hip, knobs):
    """stream_xcd = 1 forced at grids below one round of the 8 XCDs and just above, and at a few hundred workgroups."""
    knobs.set("stream_xcd", 1)
    seen = set()
    for name, n, batch in (("range-w3", 64, 1), ("range-w3", 1247, 3), ("runs", 1247, 3), ("runs", 1247, 22), ("mixed", 1300, 3),
                           ("t23", 1247, 3), ("eq300", 1247, 1), ("mixed", 1247, 257)):
        _, ta, planes_entries, constant, _ = shape(name)
        seen.add(hip.uint_plain_sum_launches(n, batch, ta, planes_entries, constant)[5])
        Case(hip, n, batch, ta, planes_entries, constant, seed=5).check()
    assert any(g < 8 for g in seen) and any(8 < g <= 12 for g in seen) and any(g > 100 for g in seen), sorted(seen)


def test_plain_sum_graph_replay(hip):
    """One call captured into a graph and replayed into re-poisoned outputs."""
    _, ta, planes_entries, constant, _ = shape("mixed")
    case = Case(hip, 1247, 9, ta, planes_entries, constant, seed=9)
    g = GuardedOutputs(hip, [x.size for x in case.want])
    handle = hip.uint_plain_sum_create(ta, planes_entries, constant)
    try:
        call = lambda: hip.uint_plain_sum_apply(handle, case.n, case.batch, case.da, len(planes_entries), outs=g.outs)  # noqa: E731
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            call()                                                   # warm-up outside the capture
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call()
        for o in g.outs:
            o.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        g.check(case.want, "graph replay")
    finally:
        hip.lib.csgn_uint_plain_sum_destroy(handle)


def test_plain_sum_one_plan_two_batches(hip):
    """One plan launched for two batches of different size and different n_bits."""
    _, ta, planes_entries, constant, _ = shape("t23")
    handle = hip.uint_plain_sum_create(ta, planes_entries, constant)
    try:
        for n, batch in ((1247, 3), (1300, 61), (64, 257), (1247, 1)):
            case = Case(hip, n, batch, ta, planes_entries, constant, seed=batch)
            g = GuardedOutputs(hip, [x.size for x in case.want])
            hip.uint_plain_sum_apply(handle, n, batch, case.da, len(planes_entries), outs=g.outs)
            torch.cuda.synchronize()
            g.check(case.want, (n, batch))
    finally:
        hip.lib.csgn_uint_plain_sum_destroy(handle)
