"""A public matrix over F2 applied to an encrypted integer on the device (csgn_uint_linear): every call writes into
GuardedOutputs of exactly the documented sizes and is checked word for word against the numpy composition of
include/csgn_hip.h's definition (shown equal to the decode by position, the oracle and the reference in
tests/test_uint_linear_cpu.py, which also replays these shapes' grids on the host); batches across tiles, aliased and
misaligned operands, the host's split, the XCD order, graph capture.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests.model import GuardedOutputs, hip, rand_terms  # noqa: F401
from tests.model_linear import DENSE, NS, gpu_shapes, linear_terms, np_linear

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

    def __init__(self, hip, n, batch, ta, rows, constant, seed=0, shift=0, alias=False):
        self.hip, self.n, self.batch, self.ta, self.rows, self.constant = hip, n, batch, list(ta), list(rows), constant
        self.a = [rand_terms(n, batch, t, seed + 800 + 11 * i + t) for i, t in enumerate(ta)]
        self.da = [moved(hip, p, shift) for p in self.a]
        if alias:
            assert len(ta) >= 2 and ta[0] == ta[1]
            self.a[1], self.da[1] = self.a[0], self.da[0]
        self.want = [o.ravel() for o in np_linear(n, self.a, self.rows, constant)]
        dl = (n + 63) // 64
        T = [linear_terms(self.ta, r, (constant >> j) & 1) for j, r in enumerate(self.rows)]
        assert [x.size for x in self.want] == [batch * t * dl for t in T]

    def check(self, shift=0):
        """One call into guarded outputs of exactly the documented sizes, every word asserted."""
        g = GuardedOutputs(self.hip, [x.size for x in self.want], shift)
        self.hip.uint_linear(self.n, self.batch, self.da, self.ta, self.rows, self.constant, outs=g.outs)
        torch.cuda.synchronize()
        return g.check(self.want, (self.n, self.batch, self.ta, [hex(r) for r in self.rows], hex(self.constant), shift))


SHAPES = gpu_shapes()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_linear_words(hip, n, shape):
    """in_width 1, 2, 3 and 5 with one-term planes (the fast division) and planes of 1, 2, 3, ... terms (the LDS
    table): single-bit, full, zero, constant and repeated rows, with and without the constant; batch 1, 3 and 257;
    segment ends inside a wave and inside a workgroup."""
    name, ta, rows, constant, batches = shape
    for batch in batches:
        Case(hip, n, batch, ta, rows, constant, seed=len(ta)).check()


@pytest.mark.parametrize("n", [1247, 1300])
def test_linear_misaligned(hip, n):
    """Inputs, outputs, or both one word off 16-byte alignment: 8-byte units at an even word count too."""
    for name, ta, rows, constant, batches in SHAPES[4:]:
        for in_shift, out_shift in ((1, 0), (0, 1), (1, 1)):
            Case(hip, n, batches[1], ta, rows, constant, seed=3, shift=in_shift).check(out_shift)


@pytest.mark.parametrize("batch", DENSE[4])
def test_linear_dense_64_by_64(hip, batch):
    """in_width = out_width = 64 under a random dense matrix: every argument array full, several tiles at batch 33."""
    name, ta, rows, constant, _ = DENSE
    case = Case(hip, 1247, batch, ta, rows, constant)
    case.check()
    if batch == 2:
        case.check(1)                                                # the same planes into misaligned outputs
        Case(hip, 64, batch, [2] * 64, rows, constant).check()


def test_linear_aliased_inputs(hip):
    """Two input planes that are the same pointer, read by one row and by different rows."""
    for n in NS:
        Case(hip, n, 5, [2, 2, 1], [0b011, 0b101, 0b110, 0b111], 0b1000, alias=True).check()


def test_linear_tiles_and_launches(hip, knobs):
    """2 G + 5 elements at n = 64, G read from the plan: two full tiles and a partial one in one launch, then under
    launch_blocks caps that cut between tiles, and one below a tile's workgroups (a tile still goes whole)."""
    for name, ta, rows, constant, _ in SHAPES[5:9]:
        knobs.set("launch_blocks", 0)
        G = hip.uint_linear_plan(64, 1 << 30, ta, rows, constant)[2]
        batch = 2 * G + 5
        case = Case(hip, 64, batch, ta, rows, constant, seed=17)
        plan = hip.uint_linear_plan(64, batch, ta, rows, constant)
        assert plan[2:4] == [G, 3] and plan[5] == 1
        case.check()
        per = plan[4]
        for cap, launches in ((per, 3), (2 * per + 1, 2), (per - 1, 3)):
            knobs.set("launch_blocks", cap)
            assert hip.uint_linear_plan(64, batch, ta, rows, constant)[5] == launches
            case.check()


def test_linear_xcd_order_at_small_grids(hip, knobs):
    """stream_xcd = 1 forced at grids of a few workgroups (below one round of the 8 XCDs, and just above) and at
    several tiles, whole and split."""
    knobs.set("stream_xcd", 1)
    for name, ta, rows, constant, batches in SHAPES[4:]:
        for batch in batches:
            Case(hip, 1247, batch, ta, rows, constant, seed=5).check()
    name, ta, rows, constant, _ = DENSE
    case = Case(hip, 1247, 29, ta, rows, constant, seed=6)
    case.check()
    knobs.set("launch_blocks", 2 * hip.uint_linear_plan(1247, 29, ta, rows, constant)[4])
    case.check()


def test_linear_graph_replay(hip):
    """One call captured into a graph and replayed into re-poisoned outputs."""
    name, ta, rows, constant, _ = SHAPES[7]
    case = Case(hip, 1247, 9, ta, rows, constant, seed=9)
    g = GuardedOutputs(hip, [x.size for x in case.want])
    call = lambda: hip.uint_linear(case.n, case.batch, case.da, case.ta, case.rows, case.constant, outs=g.outs)  # noqa: E731
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()                                                       # warm-up outside the capture
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
