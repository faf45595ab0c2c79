"""Encrypted integers summed into encrypted integers on the device (csgn_wsum), word for word against the definition of
include/csgn_hip.h (pinned against the oracle and the reference in tests/test_wsum_cpu.py), through caller outputs of
exactly the documented size between guard words: every plane kind, empty classes and skipped planes, the split of the
selection ranks over workgroups, several elements a workgroup, the LDS budget, the 8-byte path, the host's split into
launches, a captured graph.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests.model import GuardedOutputs, hip, rand_terms  # noqa: F401
from tests.model_count import np_count
from tests.model_wsum import np_wsum

pytestmark = pytest.mark.gpu

MUL_4x4 = [1, 2, 3, 4, 3, 2, 1]


def offset_upload(hip, words, shift):
    """`words` on the device, `shift` words past a fresh tensor's start."""
    whole = hip.upload(np.concatenate([np.zeros(shift, dtype=np.uint64), words.ravel()]))
    return whole[shift:]


def class_inputs(n, ns, t, count, seed):
    return [rand_terms(n, count * k, t, seed + c) if k else None for c, k in enumerate(ns)]


def run(hip, n, count, ns, t, js, xs, wants, shift=0, shift_class=None):
    """One csgn_wsum into outputs of exactly the documented sizes between guard words (tests/model.py, GuardedOutputs),
    checked word for word and for writes outside them.  shift: words every operand lies past a 16-byte boundary;
    shift_class: only that class's input does."""
    ins = [None if x is None else offset_upload(hip, x, shift if shift_class in (None, c) else 0) for c, x in enumerate(xs)]
    guarded = GuardedOutputs(hip, [w.size for w in wants], shift=shift if shift_class is None else 0)
    hip.wsum(n, count, ns, t, ins, js, outs=guarded.outs)
    torch.cuda.synchronize()
    guarded.check(wants, (n, count, ns, t, js, shift, shift_class))


def check(hip, n, count, ns, t, js, seed, **how):
    """The reference once, then the call; returns (xs, wants) for a caller that runs more knobs."""
    xs = class_inputs(n, ns, t, count, seed)
    wants = np_wsum(xs, ns, js)
    run(hip, n, count, ns, t, js, xs, wants, **how)
    return xs, wants


WORDS = [([2, 1, 1], 1, [0, 1, 2, 3]), ([2, 1, 1], 2, [0, 1, 2, 3]), ([3, 3], 2, [0, 1, 2, 3]),
         ([2, 0, 3], 2, [0, 1, 2, 3]), ([1, 0, 3], 2, [0, 2, 3]), ([4, 4, 4], 1, [0, 1, 2, 3, 4]),
         (MUL_4x4, 1, list(range(8)))]


# 63: dL = 1; 65 and 1247: even dL, 16-byte units; 129: odd dL, the 8-byte kernel
@pytest.mark.parametrize("n", [63, 65, 129, 1247])
@pytest.mark.parametrize("shape", WORDS, ids=lambda s: "n%s_t%d_%s" % ("".join(map(str, s[0])), s[1], "".join(map(str, s[2]))))
def test_wsum_words(hip, n, shape):
    """Every plane of small shapes, five elements: [2,1,1] has 4 / 6 / 10 / 16 terms at t = 2 and [3,3] 6 / 18 / 84 / 96;
    [2,0,3] has an empty class (a null pointer), and plane 1 of [1,0,3] is empty: its plane list skips it; the top
    planes of [4,4,4] and of the 4 x 4 product have 7 and 29 count vectors."""
    ns, t, js = shape
    xs, wants = check(hip, n, 5, ns, t, js, 100 + n + sum(ns))
    if ns == [2, 1, 1] and t == 2:
        assert [w.shape[1] for w in wants] == [4, 6, 10, 16]
    if ns == [3, 3]:
        assert [w.shape[1] for w in wants] == [6, 18, 84, 96]


@pytest.mark.parametrize("t", [1, 3])
def test_wsum_of_one_class_is_the_count(hip, t):
    """One class of 8 inputs, planes 1 and 2: the words csgn_count writes."""
    n, count, g, js = 1247, 3, 8, [1, 2]
    x = rand_terms(n, count * g, t, 150 + t)
    wants = np_count(x, g, js)
    run(hip, n, count, [g], t, js, [x], wants)
    counted = hip.count(n, count, g, t, [hip.upload(x.ravel())], js)
    summed = hip.wsum(n, count, [g], t, [hip.upload(x.ravel())], js)
    torch.cuda.synchronize()
    for a, b in zip(counted, summed):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", [63, 1247])
def test_wsum_rank_split(hip, knobs, n):
    """Knob wsum_cpart forces the selection ranks of a part.  [5,4] at t = 2, plane 2: vectors (m_1, m_0) = (0, 4) of 5
    selections, (1, 2) of 4 * 10 = 40 -- a row of S_1 is the 10 subsets of class 0 -- and (2, 0) of 6.  Parts of 1: every
    selection its own part, a vector's last among them; 7: parts begin inside a row (40 = 5 * 7 + 5); 10: at a row's
    end; 39: the second part of the middle vector is its last selection alone.  One class of 20 at plane 1 (190 pairs,
    the row i_1 = 0 holds 19): parts of 7, 19 and 20 begin inside a row, at a row's end and one past it."""
    xs, wants = check(hip, n, 3, [5, 4], 2, [1, 2], 200 + n)
    ys, wanty = check(hip, n, 3, [20], 1, [0, 1], 210 + n)
    for cpart in (1, 7, 10, 19, 20, 39):
        knobs.set("wsum_cpart", cpart)
        run(hip, n, 3, [5, 4], 2, [1, 2], xs, wants)
        run(hip, n, 3, [20], 1, [0, 1], ys, wanty)


@pytest.mark.parametrize("n,t", [(63, 1), (63, 2), (1247, 1)])
def test_wsum_element_groups(hip, n, t):
    """[2,1], planes 0 and 1, 2729 elements: an element is three parts (plane 0, and the vectors (0, 2) and (1, 0) of
    plane 1) of whole staged terms, at most 4 terms each.  A workgroup takes EG elements, doubled while the largest part
    of 2 EG elements is at most 16 384 units, their inputs fit the LDS budget and 3 * ceil(count / (2 EG)) workgroups are
    at least 2048: 3 * 1365 and 3 * 683 are, 3 * 342 is not, so EG = 4 and 2729 = 4 * 682 + 1 leaves a last group of ONE
    element."""
    check(hip, n, 2729, [2, 1], t, [0, 1], 250 + n + t)


# What wsum_fused (csgn_wsum.hip) plans for each case, by its own arithmetic.  ub = bytes a unit, U = units a term,
# nt = inputs of the classes that take part * t.  The inputs are staged whole when nt U ub <= 57344; otherwise fit =
# 57344 / (nt ub) units; fit >= 16: chunks = ceil(U / fit) slices of KC = ceil(U / chunks) units, the last of
# U - (chunks - 1) KC; fit < 16: nothing is staged and every factor is read from memory.
#   (n, ns, t, js)                   U  ub   nt   bytes    fit  slices
#   (4096, [64,64], 1, [1])          32 16   128  65536    28   16 + 16
#   (5000, [64,64], 1, [1])          79  8   128  80896    56   40 + 39 (a short last slice: kc < KC)
#   (1247, [200,200], 1, [1])        10 16   400  64000     8   unstaged
#   (1247, [100,100], 2, [1])        10 16   400  64000     8   unstaged, with digits
#   (1247, [0,200,200], 1, [2])      10 16   400  64000     8   unstaged, an empty class below the others
BUDGET = [(4096, [64, 64], 1, [1]), (5000, [64, 64], 1, [1]), (1247, [200, 200], 1, [1]), (1247, [100, 100], 2, [1]),
          (1247, [0, 200, 200], 1, [2])]


@pytest.mark.parametrize("case", BUDGET, ids=lambda c: "n%d_%s_t%d" % (c[0], "_".join(map(str, c[1])), c[2]))
def test_wsum_unit_slices_and_unstaged_inputs(hip, case):
    """Inputs past the LDS budget: slices of units (chunk, k0, and kc < KC on a short last slice), and factors read from
    memory once a slice would be under 16 units."""
    n, ns, t, js = case
    check(hip, n, 1, ns, t, js, 300 + sum(ns))


@pytest.mark.parametrize("n", [65, 1247])
def test_wsum_misaligned_operands_take_the_8_byte_path(hip, n):
    """Even dL, and every operand -- or the input of ONE class alone -- one word off a 16-byte boundary: the same words,
    by 8-byte units."""
    xs, wants = check(hip, n, 3, [3, 3], 2, [0, 1, 2, 3], 400 + n, shift=1)
    run(hip, n, 3, [3, 3], 2, [0, 1, 2, 3], xs, wants, shift=1, shift_class=1)
    check(hip, n, 1, [200, 200], 1, [1], 410 + n, shift=1, shift_class=0)       # unstaged


@pytest.mark.parametrize("cap", [4, 15])
def test_wsum_launches(hip, knobs, cap):
    """The host cuts the call's workgroups, in order, into launches of launch_blocks (knob) each.  [3,3] at t = 2, planes
    0 .. 3, is 1 + 2 + 2 + 1 = 6 workgroups an element, 42 for 7 elements: launches of 4 and of 15 end inside an
    element.  With parts of one selection it is 3 + 6 + 12 + 3 = 24 an element."""
    knobs.set("launch_blocks", cap)
    xs, wants = check(hip, 63, 7, [3, 3], 2, [0, 1, 2, 3], 500)
    knobs.set("wsum_cpart", 1)
    run(hip, 63, 7, [3, 3], 2, [0, 1, 2, 3], xs, wants)


def test_wsum_graph_capture(hip):
    """The launch is capturable: one replay of a captured call writes the planes again."""
    n, count, ns, t, js = 1247, 5, [3, 3], 2, [0, 1, 2, 3]
    xs = class_inputs(n, ns, t, count, 600)
    wants = np_wsum(xs, ns, js)
    ins = [hip.upload(x.ravel()) for x in xs]
    outs = [hip.empty_words(w.size) for w in wants]
    handle = hip.wsum_create(ns, t, js)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            hip.wsum_apply(handle, n, count, ins, len(js), outs)            # warm-up outside the capture
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            hip.wsum_apply(handle, n, count, ins, len(js), outs)
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for j, w in enumerate(wants):
            assert np.array_equal(hip.download(outs[j]), w.ravel()), j
    finally:
        hip.lib.csgn_wsum_destroy(handle)
