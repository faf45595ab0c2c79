"""A public bilinear form over F2 of two encrypted integers on the device (csgn_uint_bilinear): every call writes into
GuardedOutputs of exactly the documented sizes and is checked word for word against the numpy composition of
include/csgn_hip.h's definition (shown equal to the decode by position, the oracle and the reference in
tests/test_uint_bilinear_cpu.py, which also replays these shapes' grids on the host); batches across tiles, staged and
unstaged shapes, aliased and misaligned operands, the host's split, the XCD order, graph capture.  Run with
`pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests.model import GuardedOutputs, hip, rand_terms  # noqa: F401
from tests.model_bilinear import (ALIASED, ALIASED_BATCH, BOUNDARIES, DENSE, NS, PAST_EDGE, STAGED_EDGE, TILE_SHAPES, UNSTAGED,
                                  XCD_DENSE, bilinear_terms, gpu_shapes, np_bilinear)

pytestmark = pytest.mark.gpu


def moved(hip, a, shift):
    """Device copy of the words; with shift = 1 it starts 8 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a).ravel()
    t = hip.upload(np.concatenate([np.zeros(shift, np.uint64), a]))[shift:]
    assert t.data_ptr() % 16 == 8 * shift
    return t


class Case:
    """Input planes on the host and, uploaded once, on the device; the reference computed once and left unchanged.
    square: b IS a (the same device pointers); alias: plane 1 of a IS plane 0 (the same device pointer)."""

    def __init__(self, hip, n, batch, ta, tb, form, constant, seed=0, shift=0, square=False, alias=False):
        self.hip, self.n, self.batch, self.ta, self.tb = hip, n, batch, list(ta), list(tb)
        self.form, self.constant = [list(p) for p in form], constant
        self.a = [rand_terms(n, batch, t, seed + 900 + 11 * i + t) for i, t in enumerate(ta)]
        self.da = [moved(hip, p, shift) for p in self.a]
        if alias:
            assert len(ta) >= 2 and ta[0] == ta[1]
            self.a[1], self.da[1] = self.a[0], self.da[0]
        if square:
            assert self.ta == self.tb
            self.b, self.db = self.a, self.da
        else:
            self.b = [rand_terms(n, batch, t, seed + 1900 + 13 * l + t) for l, t in enumerate(tb)]
            self.db = [moved(hip, p, shift) for p in self.b]
        self.want = [o.ravel() for o in np_bilinear(n, self.a, self.b, self.form, constant)]
        dl = (n + 63) // 64
        T = [bilinear_terms(self.ta, self.tb, p, (constant >> x) & 1) for x, p in enumerate(self.form)]
        assert [x.size for x in self.want] == [batch * t * dl for t in T]

    def launches(self):
        return self.hip.uint_bilinear_launches(self.n, self.batch, self.ta, self.tb, self.form, self.constant)

    def check(self, shift=0):
        """One call into guarded outputs of exactly the documented sizes, every word asserted."""
        g = GuardedOutputs(self.hip, [x.size for x in self.want], shift)
        self.hip.uint_bilinear(self.n, self.batch, self.da, self.ta, self.db, self.tb, self.form, self.constant, outs=g.outs)
        torch.cuda.synchronize()
        return g.check(self.want, (self.n, self.batch, self.ta, self.tb, self.form, hex(self.constant), shift))


SHAPES = gpu_shapes()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_bilinear_words(hip, n, shape):
    """wa, wb in 1, 2, 3 and 5 with one-term planes (the divisions) and planes of 1, 2, 3, ... terms on either side (the
    table): one pair, all pairs, empty, constant, repeated and unsorted rows, with and without the constant; batch 1, 3
    and 257."""
    name, ta, tb, form, constant, batches = shape
    for batch in batches:
        Case(hip, n, batch, ta, tb, form, constant, seed=len(ta)).check()


@pytest.mark.parametrize("n", NS)
def test_bilinear_entry_boundaries(hip, n):
    """ta = [3, 70], tb = [1, 5, 2]: entry ends inside a wave and past a wave."""
    name, ta, tb, form, constant, batches = BOUNDARIES
    for batch in batches:
        Case(hip, n, batch, ta, tb, form, constant, seed=2).check()


@pytest.mark.parametrize("shape", DENSE, ids=["%s-n%d" % (s[0], s[1]) for s in DENSE])
def test_bilinear_dense(hip, shape):
    """clmulWide(32) (63 planes, 1024 pairs) and random forms with wa = wb = 64 and 64 planes of 32 pairs: every
    argument array full, 2048 entries (the table through the vector cache), several workgroups a tile; 128 operand
    terms of 160 bytes pass the LDS budget, of 8 bytes they are staged."""
    name, n, ta, tb, form, constant, batches = shape
    for batch in batches:
        case = Case(hip, n, batch, ta, tb, form, constant)
        assert case.launches()[8] == (0 if name == "random64" and n == 1247 else 1)
        case.check()
        if name == "random64" and n == 1247:
            case.check(1)                                            # the same planes into misaligned outputs


def test_bilinear_unstaged_and_the_budget(hip):
    """Operand planes past the LDS budget (215 terms of 160 bytes) read from memory; 102 terms are staged, 103 not."""
    for (name, ta, tb, form, constant, batches), staged in ((UNSTAGED, 0), (STAGED_EDGE, 1), (PAST_EDGE, 0)):
        case = Case(hip, 1247, batches[0], ta, tb, form, constant, seed=4)
        assert case.launches()[8] == staged, name
        case.check()


def test_bilinear_aliased_inputs(hip):
    """a and b the same pointers (squares); two planes of a the same pointer."""
    for n in NS:
        for (ta, tb, form, constant), (square, alias) in zip(ALIASED, ((True, False), (False, True), (True, True))):
            Case(hip, n, ALIASED_BATCH, ta, tb, form, constant, square=square, alias=alias).check()


@pytest.mark.parametrize("n", [1247, 1300])
def test_bilinear_misaligned(hip, n):
    """Inputs, outputs, or both one word off 16-byte alignment: 8-byte units at an even word count too."""
    for name, ta, tb, form, constant, batches in SHAPES[13:19] + [BOUNDARIES]:
        for in_shift, out_shift in ((1, 0), (0, 1), (1, 1)):
            Case(hip, n, batches[1], ta, tb, form, constant, seed=3, shift=in_shift).check(out_shift)


def test_bilinear_tiles_and_launches(hip, knobs):
    """2 G + 5 elements, G read from the launches: two full tiles and a partial one in one launch, then under
    launch_blocks caps that cut between tiles, and one below a tile's workgroups (a tile still goes whole)."""
    for n, (name, ta, tb, form, constant, _) in ((n, SHAPES[i]) for n, i in TILE_SHAPES):
        knobs.set("launch_blocks", 0)
        G = hip.uint_bilinear_launches(n, 1 << 30, ta, tb, form, constant)[2]
        case = Case(hip, n, 2 * G + 5, ta, tb, form, constant, seed=17)
        plan = case.launches()
        assert plan[2:4] == [G, 3] and plan[5] == 1
        case.check()
        per = plan[4]
        assert per > 1                                               # so that per - 1 is a cap below a tile's workgroups
        for cap, launches in ((per, 3), (2 * per, 2), (per - 1, 3)):
            knobs.set("launch_blocks", cap)
            assert case.launches()[5] == launches
            case.check()


def test_bilinear_xcd_order(hip, knobs):
    """stream_xcd = 1 forced at grids of a few workgroups (below one round of the 8 XCDs, and just above) and at
    several tiles, whole and split."""
    knobs.set("stream_xcd", 1)
    for name, ta, tb, form, constant, batches in SHAPES[16:20] + [BOUNDARIES]:
        for batch in batches:
            Case(hip, 1247, batch, ta, tb, form, constant, seed=5).check()
    for shape, batch in XCD_DENSE:                                   # staged, one element a tile; unstaged, twelve
        name, n, ta, tb, form, constant, _ = shape
        knobs.set("launch_blocks", 0)
        case = Case(hip, n, batch, ta, tb, form, constant, seed=6)
        assert case.launches()[3] > 2
        case.check()
        knobs.set("launch_blocks", 2 * case.launches()[4])
        assert case.launches()[5] > 1
        case.check()


def test_bilinear_graph_replay(hip):
    """One call captured into a graph and replayed into re-poisoned outputs."""
    name, ta, tb, form, constant, _ = SHAPES[18]
    case = Case(hip, 1247, 9, ta, tb, form, constant, seed=9)
    g = GuardedOutputs(hip, [x.size for x in case.want])
    handle = hip.uint_bilinear_create(ta, tb, form, constant)
    try:
        call = lambda: hip.uint_bilinear_apply(handle, case.n, case.batch, case.da, case.db, len(form), outs=g.outs)  # noqa: E731
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
        hip.lib.csgn_uint_bilinear_destroy(handle)
