"""What the csgn_uint_arith tests share: include/csgn_hip.h's definition of a + b, a - b, a == b and a != b over uniform
planes BY POSITION -- the term counts, the factors of every entry as csgn_uint_arith.hip decodes them, and the words
placed from that decode -- beside the same words composed from the per-bit steps of tests/model.py (the chain the
classes began with), which tests/test_uint_arith_cpu.py shows to be equal term for term."""
import numpy as np

from tests.model import (ADD_FULL, ADD_HALF, LIMIT, const_term, np_not, np_step, np_uint_add, np_uint_eq, np_uint_sub,
                         u64s)

ADD, SUB, EQ, NE = 1, 2, 3, 4
OPS = {"add": ADD, "sub": SUB, "eq": EQ, "ne": NE}
MAX_WIDTH = 16


def arith_counts(op, ta, tb):
    """(T, C): the terms of every output (planes 0..w-1 and the carry-out for ADD / SUB, the one result for EQ / NE) and
    of every carry c_0..c_{w-1}, as Python integers (no overflow)."""
    w = len(ta)
    if op in (EQ, NE):
        e = 1
        for j in range(w):
            e *= ta[j] + tb[j] + 1
        return [e + (op == NE)], []
    one = 1 if op == SUB else 0
    T, Cs, c = [], [], one
    for j in range(w):
        tn = tb[j] + one
        T.append(ta[j] + tn + c)
        c = ta[j] * tn + (ta[j] + tn) * c
        Cs.append(c)
    return T + [c], Cs


def arith_terms(op, ta, tb, output):
    """csgn_uint_arith_terms: 0 for anything invalid or a count of 2^62 or more."""
    w = len(ta)
    if op not in (ADD, SUB, EQ, NE) or not 1 <= w <= MAX_WIDTH or len(tb) != w:
        return 0
    if any(not 0 < t < LIMIT for t in list(ta) + list(tb)):
        return 0
    T, _ = arith_counts(op, ta, tb)
    if output >= len(T):
        return 0
    return T[output] if T[output] < LIMIT else 0


def arith_entry(op, ta, tb, o, i):
    """The factors of entry i of output o: a list of ("a" | "b", plane, term); ONE contributes nothing."""
    w = len(ta)
    if op in (EQ, NE):
        e = arith_counts(EQ, ta, tb)[0][0]
        if i >= e:
            return []                                                 # NE's closing ONE
        f = []
        for j in reversed(range(w)):                                  # the fastest digit belongs to plane w - 1
            i, d = divmod(i, ta[j] + tb[j] + 1)
            if d < ta[j]:
                f.append(("a", j, d))
            elif d < ta[j] + tb[j]:
                f.append(("b", j, d - ta[j]))
        return f[::-1]
    one = 1 if op == SUB else 0
    _, Cs = arith_counts(op, ta, tb)
    cin = lambda j: Cs[j - 1] if j else one                           # noqa: E731  C_{j-1}

    def nb(j, x):                                                     # term x of b_j (+ ONE, which comes last)
        return [("b", j, x)] if x < tb[j] else []

    f = []
    if o < w:
        if i < ta[o]:
            return [("a", o, i)]
        if i < ta[o] + tb[o] + one:
            return nb(o, i - ta[o])
        q, j = i - ta[o] - tb[o] - one, o - 1
    else:
        q, j = i, w - 1
    while j >= 0:
        tn = tb[j] + one
        if q < ta[j] * tn:
            return f + [("a", j, q // tn)] + nb(j, q % tn)
        q -= ta[j] * tn
        p, q = divmod(q, cin(j))
        f += [("a", j, p)] if p < ta[j] else nb(j, p - ta[j])
        j -= 1
    return f                                                          # c_{-1} of SUB: ONE


def np_arith(n, op, a, b, carry=False):
    """(outputs, carry or None) over uniform planes words[batch, t_j, dL], every term placed from arith_entry."""
    ta, tb = [p.shape[1] for p in a], [p.shape[1] for p in b]
    batch, _, dl = a[0].shape
    T, _ = arith_counts(op, ta, tb)
    if op in (ADD, SUB) and not carry:
        T = T[:-1]
    one = const_term(n, 1)
    src = {"a": a, "b": b}
    outs = []
    for o, t in enumerate(T):
        out = np.empty((batch, t, dl), dtype=np.uint64)
        for i in range(t):
            v = np.broadcast_to(one, (batch, dl)).copy()
            for side, j, x in arith_entry(op, ta, tb, o, i):
                v &= src[side][j][:, x, :]
            out[:, i, :] = v
        outs.append(out)
    if op in (ADD, SUB) and carry:
        return outs[:-1], outs[-1]
    return outs, None


def np_arith_chain(n, op, a, b, carry=False):
    """The same through the per-bit steps, as tests/model.py composes the class operators: np_uint_add / np_uint_sub /
    np_uint_eq (np_not of it for NE), the carry-out from the chained ADD_FULL's output 1."""
    if op == EQ:
        return [np_uint_eq(n, a, b)], None
    if op == NE:
        return [np_not(n, np_uint_eq(n, a, b))], None
    outs = np_uint_add(n, a, b) if op == ADD else np_uint_sub(n, a, b)
    if not carry:
        return outs, None
    if op == ADD:
        _, c = np_step(n, ADD_HALF, None, a[0], b[0])
        for j in range(1, len(a)):
            _, c = np_step(n, ADD_FULL, c, a[j], b[j])
    else:
        c = np.broadcast_to(const_term(n, 1), (a[0].shape[0], 1, a[0].shape[2]))
        for j in range(len(a)):
            _, c = np_step(n, ADD_FULL, c, a[j], np_not(n, b[j]))
    return outs, c


def c_terms(lib, op, w, ta, tb, output):
    return int(lib.csgn_uint_arith_terms(op, w, None if ta is None else u64s(ta), None if tb is None else u64s(tb), output))


def term_modes(w, mode):
    """The term counts of a's and b's planes: all 1, all 2, or mixed 1..3."""
    if mode == "1":
        return [1] * w, [1] * w
    if mode == "2":
        return [2] * w, [2] * w
    return [1 + (j + 1) % 3 for j in range(w)], [1 + (2 * j) % 3 for j in range(w)]      # a: 2, 3, 1, ...; b: 1, 3, 2, ...
