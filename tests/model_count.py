"""What the csgn_count tests share: include/csgn_hip.h's definition of the bits of the number of ones among g encrypted
bits, by its decode in numpy on uniform batches and as the literal nested-loop composition over any (add, mul) pair of
tests/model.py (ref_ops, oracle_ops)."""
from itertools import combinations
from math import comb

import numpy as np

from tests.model import LIMIT


def count_terms(g, t, j):
    """C(g, 2^j) * t^(2^j) by the definition itself (Python integers: no overflow); 0 for a zero argument, j > 6,
    2^j > g, t >= 2^62 or a count of 2^62 or more."""
    if not (g and t) or t >= LIMIT or j > 6 or (1 << j) > g:
        return 0
    m = 1 << j
    c = comb(g, m)
    if c >= LIMIT:
        return 0
    T = c
    for _ in range(m):                      # t^m one factor at a time: the early exit keeps huge t cheap
        T *= t
        if T >= LIMIT:
            return 0
    return T


def np_count(x, g, js, layout="grouped"):
    """Words of the planes js by the decode.  grouped: x = words[count * g, t, dL], input i of element q is element
    q * g + i; planes: x = a list of g arrays words[count, t, dL].  Term p = c * t^m + (d_1 ... d_m in base t, d_1
    slowest) of plane j is the AND over k of term d_k of input i_k, (i_1 ... i_m) the m-subset of lexicographic rank c.
    Returns one array words[count, T_j, dL] per plane."""
    if layout == "planes":
        assert len(x) == g
        X = np.stack(x, axis=1)                                         # [count, g, t, dL]
    else:
        X = x.reshape(-1, g, x.shape[1], x.shape[2])
    count, _, t, dl = X.shape
    outs = []
    for j in js:
        m = 1 << j
        subsets = np.array(list(combinations(range(g), m)), dtype=np.int64)       # lexicographic by construction
        assert subsets.shape == (comb(g, m), m)
        acc = X[:, subsets[:, 0]]                                       # [count, C, t, dL]
        for k in range(1, m):
            f = X[:, subsets[:, k]]
            acc = (acc[:, :, :, None, :] & f[:, :, None, :, :]).reshape(count, len(subsets), -1, dl)
        outs.append(acc.reshape(count, len(subsets) * t ** m, dl))
    return outs


def compose_count(ops, xs, j):
    """The definition, literally, for ONE element: the left-nested sum over i_1 < i_2 < ... < i_m (the nested loops, in
    their own order) of ((x_{i_1} * x_{i_2}) * ...) * x_{i_m}, through ops = (add, mul) on flat word arrays.  xs: the g
    inputs, one flat array each."""
    add, mul = ops
    g, m = len(xs), 1 << j
    acc = None

    def loops(start, depth, prod):
        nonlocal acc
        if depth == m:
            acc = prod if acc is None else add(acc, prod)
            return
        for i in range(start, g - (m - depth) + 1):
            loops(i + 1, depth + 1, xs[i] if prod is None else mul(prod, xs[i]))

    loops(0, 0, None)
    return acc


def popcount_planes(values, planes):
    """Bit j of every value's count of ones, j < planes."""
    pc = np.array([bin(int(v)).count("1") for v in values], dtype=np.uint64)
    return pc & np.uint64((1 << planes) - 1)
