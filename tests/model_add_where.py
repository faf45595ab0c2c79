"""What the csgn_uint_add_where tests share: include/csgn_hip.h's definition of a + (s ? k : 0) -- the table composed
in its order over any add / multiply (the reference's, the oracle's, numpy's), the term counts as Python integers, the
factors of every entry BY POSITION as csgn_uint_add_where.hip decodes them (tests/model_arith.arith_entry with b_j := s
where k_j = 1 and b_j absent elsewhere), and the words placed from that decode."""
import ctypes as C

import numpy as np

from tests.model import LIMIT, const_term, np_add, np_mul, u64s
from tests.model_arith import ADD, arith_entry

MAX_WIDTH = 32


def compose_add_where(planes, s, k, add, mul, zero):
    """(outputs, carry-out): the table of include/csgn_hip.h, operand order included."""
    w = len(planes)
    if k == 0:
        return list(planes), zero
    m = (k & -k).bit_length() - 1
    outs, c = [], None
    for j, a in enumerate(planes):
        if j < m:
            outs.append(a)
        elif j == m:
            outs.append(add(a, s))
            c = mul(a, s)
        elif (k >> j) & 1:
            ab = add(a, s)
            outs.append(add(ab, c))
            c = add(mul(a, s), mul(ab, c))
        else:
            outs.append(add(a, c))
            c = mul(a, c)
    assert len(outs) == w
    return outs, c


def np_add_where_compose(n, a, s, k):
    """The composition over uniform planes words[batch, t_j, dL] and s = words[batch, ts, dL]."""
    batch, _, dl = a[0].shape
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    return compose_add_where(a, s, k, np_add, np_mul, zero)


def add_where_counts(ta, ts, k):
    """(T, C): the terms of every output (planes 0..w-1 and the carry-out) and of every carry c_0..c_{w-1}."""
    T, Cs, c = [], [], 0
    for j, t in enumerate(ta):
        tn = ts if (k >> j) & 1 else 0
        T.append(t + tn + c)
        c = t * tn + (t + tn) * c
        Cs.append(c)
    return T + [c if k else 1], Cs


def add_where_terms(ta, ts, k):
    """csgn_uint_add_where_terms: None for anything invalid or a count of 2^62 or more."""
    w = len(ta)
    if not 1 <= w <= MAX_WIDTH or k >> w or not 0 < ts < LIMIT or any(not 0 < t < LIMIT for t in ta):
        return None
    T, _ = add_where_counts(ta, ts, k)
    return T if all(t < LIMIT for t in T) else None


def add_where_entry(ta, ts, k, o, i):
    """The factors of entry i of output o: a list of ("a", plane, term) and ("s", 0, term).  It is arith_entry of ADD
    with tb_j = ts where k_j = 1 and tb_j = 0 elsewhere; ("b", j, x) there is term x of s.  The carry-out of k = 0 is
    ZERO: None."""
    w = len(ta)
    if k == 0 and o == w:
        return None
    tn = [ts if (k >> j) & 1 else 0 for j in range(w)]
    return [("s", 0, x) if side == "b" else (side, j, x) for side, j, x in arith_entry(ADD, ta, tn, o, i)]


def np_add_where(n, a, s, k, carry=False):
    """(outputs, carry or None) over uniform planes, every term placed from add_where_entry."""
    ta, ts = [p.shape[1] for p in a], s.shape[1]
    batch, _, dl = a[0].shape
    T, _ = add_where_counts(ta, ts, k)
    one = const_term(n, 1)
    outs = []
    for o, t in enumerate(T if carry else T[:-1]):
        out = np.empty((batch, t, dl), dtype=np.uint64)
        for i in range(t):
            f = add_where_entry(ta, ts, k, o, i)
            v = np.broadcast_to(one if f is not None else const_term(n, 0), (batch, dl)).copy()
            for side, j, x in f or []:
                v &= a[j][:, x, :] if side == "a" else s[:, x, :]
            out[:, i, :] = v
        outs.append(out)
    return (outs[:-1], outs[-1]) if carry else (outs, None)


def c_terms(lib, w, k, ts, ta):
    out = (C.c_uint64 * (MAX_WIDTH + 2))()
    ok = lib.csgn_uint_add_where_terms(w, k, ts, None if ta is None else u64s(ta), out)
    return list(out)[:w + 1] if ok else None


def clear_add_where(x, s, k, w):
    """(value, carry) of x + (s ? k : 0) in clear integers."""
    v = x + (k if s else 0)
    return v & ((1 << w) - 1), v >> w
