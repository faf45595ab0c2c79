"""A public polynomial over F2 of encrypted planes on the device (csgn_uint_poly): every call writes into
GuardedOutputs of exactly the documented sizes and is checked word for word against the numpy composition of
include/csgn_hip.h's definition (shown equal to the decode by position, the oracle and the reference in
tests/test_uint_poly_cpu.py, which also replays these shapes' grids on the host); batches across tiles, staged and
unstaged shapes, aliased and misaligned inputs, the host's split, the XCD order, graph capture, and the words of
csgn_uint_linear and csgn_uint_bilinear on forms they can express.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests.model import GuardedOutputs, hip, rand_terms  # noqa: F401
from tests.model_poly import (ALIASED, ALIASED_BATCH, BOUNDARIES, FULL, NS, PAST_EDGE, STAGED_EDGE, TILE_SHAPES, UNSTAGED,
                              XCD_FULL, f_linear, gpu_shapes, np_poly, poly_terms)

pytestmark = pytest.mark.gpu


def moved(hip, a, shift):
    """Device copy of the words; with shift = 1 it starts 8 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a).ravel()
    t = hip.upload(np.concatenate([np.zeros(shift, np.uint64), a]))[shift:]
    assert t.data_ptr() % 16 == 8 * shift
    return t


class Case:
    """Input planes on the host and, uploaded once, on the device; the reference computed once and left unchanged.
    same[i] (optional): input plane i IS plane same[i], the same device pointer."""

    def __init__(self, hip, n, batch, terms, form, constant, seed=0, shift=0, same=None):
        self.hip, self.n, self.batch, self.terms = hip, n, batch, list(terms)
        self.form, self.constant = [list(p) for p in form], constant
        self.planes = [rand_terms(n, batch, t, seed + 900 + 11 * i + t) for i, t in enumerate(terms)]
        self.dev = [moved(hip, p, shift) for p in self.planes]
        for i, j in enumerate(same or []):
            assert terms[i] == terms[j]
            self.planes[i], self.dev[i] = self.planes[j], self.dev[j]
        self.want = [o.ravel() for o in np_poly(n, self.planes, self.form, constant)]
        dl = (n + 63) // 64
        T = [poly_terms(self.terms, p, (constant >> x) & 1) for x, p in enumerate(self.form)]
        assert [x.size for x in self.want] == [batch * t * dl for t in T]

    def launches(self):
        return self.hip.uint_poly_launches(self.n, self.batch, self.terms, self.form, self.constant)

    def check(self, shift=0):
        """One call into guarded outputs of exactly the documented sizes, every word asserted."""
        g = GuardedOutputs(self.hip, [x.size for x in self.want], shift)
        self.hip.uint_poly(self.n, self.batch, self.dev, self.terms, self.form, self.constant, outs=g.outs)
        torch.cuda.synchronize()
        return g.check(self.want, (self.n, self.batch, self.terms, self.form, hex(self.constant), shift))


SHAPES = gpu_shapes()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_poly_words(hip, n, shape):
    """n_in in 1, 2, 3 and 5 with one-term planes (nothing divided) and planes of 1, 2, 3, ... terms (the planes'
    divisors): one monomial of each degree 1..4 and of degree 8, every monomial of degree <= 3, empty, constant,
    repeated monomials and factors, unsorted rows, with and without the constant; then one count and one degree (the
    one division); batch 1, 3 and 257."""
    name, terms, form, constant, batches = shape
    for batch in batches:
        Case(hip, n, batch, terms, form, constant, seed=len(terms)).check()


@pytest.mark.parametrize("n", NS)
def test_poly_monomial_boundaries(hip, n):
    """t = [3, 70, 1, 5, 2]: monomial ends inside a wave and past a wave."""
    name, terms, form, constant, batches = BOUNDARIES
    for batch in batches:
        Case(hip, n, batch, terms, form, constant, seed=2).check()


@pytest.mark.parametrize("shape", FULL, ids=["%s-n%d" % (s[0], s[1]) for s in FULL])
def test_poly_full_arrays(hip, shape):
    """256 one-term planes into 64 planes of random monomials of degree <= 3, 576 in all (the records through the
    vector cache); ch and maj at w = 32 (96 planes), chi at w = 64 (192 planes); a degree-8 monomial of 2-term planes."""
    name, n, terms, form, constant, batches = shape
    for batch in batches:
        case = Case(hip, n, batch, terms, form, constant)
        case.check()
        if name == "random256" and n == 1247:
            case.check(1)                                            # the same planes into misaligned outputs


def test_poly_unstaged_and_the_budget(hip):
    """Operand planes far past the LDS budget read from memory; as many terms as fit are staged, one more is not."""
    for (name, terms, form, constant, batches), staged in ((UNSTAGED, 0), (STAGED_EDGE, 1), (PAST_EDGE, 0)):
        case = Case(hip, 1247, batches[0], terms, form, constant, seed=4)
        assert case.launches()[8] == staged, name
        case.check()


def test_poly_aliased_inputs(hip):
    """Several planes the same pointer; every operand the same integer."""
    for n in NS:
        for terms, same, form, constant in ALIASED:
            Case(hip, n, ALIASED_BATCH, terms, form, constant, same=same).check()


@pytest.mark.parametrize("n", [1247, 1300])
def test_poly_misaligned(hip, n):
    """Inputs, outputs, or both one word off 16-byte alignment: 8-byte units at an even word count too."""
    for name, terms, form, constant, batches in SHAPES[3:5] + SHAPES[7:9] + [BOUNDARIES]:
        for in_shift, out_shift in ((1, 0), (0, 1), (1, 1)):
            Case(hip, n, batches[1], terms, form, constant, seed=3, shift=in_shift).check(out_shift)


def test_poly_tiles_and_launches(hip, knobs):
    """2 G + 5 elements, G read from the launches: two full tiles and a partial one in one launch, then under
    launch_blocks caps that cut between tiles, and one below a tile's workgroups (a tile still goes whole)."""
    for n, (name, terms, form, constant, _) in ((n, SHAPES[i]) for n, i in TILE_SHAPES):
        knobs.set("launch_blocks", 0)
        G = hip.uint_poly_launches(n, 1 << 30, terms, form, constant)[2]
        case = Case(hip, n, 2 * G + 5, terms, form, constant, seed=17)
        plan = case.launches()
        assert plan[2:4] == [G, 3] and plan[5] == 1
        case.check()
        per = plan[4]
        assert per > 1                                               # so that per - 1 is a cap below a tile's workgroups
        for cap, launches in ((per, 3), (2 * per, 2), (per - 1, 3)):
            knobs.set("launch_blocks", cap)
            assert case.launches()[5] == launches
            case.check()


def test_poly_xcd_order(hip, knobs):
    """stream_xcd = 1 forced at grids of a few workgroups and at several tiles, whole and split."""
    knobs.set("stream_xcd", 1)
    for name, terms, form, constant, batches in SHAPES[4:7] + [BOUNDARIES]:
        for batch in batches:
            Case(hip, 1247, batch, terms, form, constant, seed=5).check()
    for shape, batch in XCD_FULL:                                    # staged, six elements a tile; unstaged, 45
        name, n, terms, form, constant, _ = shape
        knobs.set("launch_blocks", 0)
        case = Case(hip, n, batch, terms, form, constant, seed=6)
        assert case.launches()[3] > 2
        case.check()
        knobs.set("launch_blocks", 2 * case.launches()[4])
        assert case.launches()[5] > 1
        case.check()


def test_poly_graph_replay(hip):
    """One call captured into a graph and replayed into re-poisoned outputs."""
    name, terms, form, constant, _ = SHAPES[4]
    case = Case(hip, 1247, 9, terms, form, constant, seed=9)
    g = GuardedOutputs(hip, [x.size for x in case.want])
    handle = hip.uint_poly_create(terms, form, constant)
    try:
        call = lambda: hip.uint_poly_apply(handle, case.n, case.batch, case.dev, len(form), outs=g.outs)  # noqa: E731
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
        hip.lib.csgn_uint_poly_destroy(handle)


@pytest.mark.parametrize("n", NS)
def test_poly_agrees_with_the_shipped_kernels(hip, n):
    """On a linear form the words of csgn_uint_poly are csgn_uint_linear's, on a bilinear form csgn_uint_bilinear's, on
    the same operands."""
    batch, ta, tb = 7, [1, 2, 3], [2, 1]
    rows, lconst = [0b101, 0b010, 0, 0b111], 0b1000
    case = Case(hip, n, batch, ta, f_linear(rows), lconst, seed=21)
    got = case.check()
    g = GuardedOutputs(hip, [x.size for x in case.want])
    hip.uint_linear(n, batch, case.dev, ta, rows, lconst, outs=g.outs)
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(got, g.check(case.want, "csgn_uint_linear")))
    pairs, bconst = [[(0, 0), (2, 1)], [], [(1, 1), (1, 0), (0, 1)]], 0b101
    case = Case(hip, n, batch, ta + tb, [[(i, 3 + l) for i, l in p] for p in pairs], bconst, seed=22)
    got = case.check()
    g = GuardedOutputs(hip, [x.size for x in case.want])
    hip.uint_bilinear(n, batch, case.dev[:3], ta, case.dev[3:], tb, pairs, bconst, outs=g.outs)
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(got, g.check(case.want, "csgn_uint_bilinear")))
