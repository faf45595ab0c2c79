"""The plane-by-plane operators of encrypted integers (csgn_uint_bitwise, include/csgn_hip.h): the six definitions per
plane composed from tests/model.py's np_add, np_mul and const_term in the order of the header's table, and the terms
table.  Shared by tests/test_uint_bitwise_cpu.py, tests/test_uint_bitwise_gpu.py and tools/bench_uint_bitwise.py."""
import numpy as np

from tests.model import LIMIT, const_term, np_add, np_mul

AND, OR, XOR, NOT, SELECT, KEEP = 1, 2, 3, 4, 5, 6
OPS = {"and": AND, "or": OR, "xor": XOR, "not": NOT, "select": SELECT, "keep": KEEP}
READS_B = (AND, OR, XOR, SELECT)
READS_SEL = (SELECT, KEEP)


def np_bitwise_plane(n, op, a, b=None, sel=None):
    """Words [batch, terms, dL] of one output plane."""
    if op == AND:
        return np_mul(a, b)
    if op == OR:
        return np_add(np_add(a, b), np_mul(a, b))
    if op == XOR:
        return np_add(a, b)
    if op == NOT:
        return np_add(a, np.broadcast_to(const_term(n, 1), (a.shape[0], 1, a.shape[2])))
    if op == SELECT:
        return np_add(np_mul(sel, np_add(a, b)), b)
    if op == KEEP:
        return np_mul(sel, a)                                         # the selector is the LEFT operand
    raise ValueError(op)


def np_bitwise(n, op, a, b=None, sel=None):
    """Every output plane of the integers a and b (lists of planes) under the one selector batch."""
    return [np_bitwise_plane(n, op, a[j], b[j] if op in READS_B else None, sel if op in READS_SEL else None)
            for j in range(len(a))]


def compose_bitwise(ops, n, op, a, b=None, sel=None):
    """The same definition for ONE element of one plane through `ops` = (add, mul) on flat word arrays: the compiled
    reference's operators or the oracle's (tests/model.py: ref_ops, oracle_ops)."""
    add, mul = ops
    if op == AND:
        return mul(a, b)
    if op == OR:
        return add(add(a, b), mul(a, b))
    if op == XOR:
        return add(a, b)
    if op == NOT:
        return add(a, const_term(n, 1))
    if op == SELECT:
        return add(mul(sel, add(a, b)), b)
    if op == KEEP:
        return mul(sel, a)
    raise ValueError(op)


def bitwise_terms(op, ts, ta, tb):
    """csgn_uint_bitwise_terms: 0 for an unknown op, a zero or too large count of an operand the op reads, or a result of
    2^62 or more; the counts of operands the op does not read are ignored."""
    if op not in OPS.values() or not 0 < ta < LIMIT:
        return 0
    if op in READS_B and not 0 < tb < LIMIT:
        return 0
    if op in READS_SEL and not 0 < ts < LIMIT:
        return 0
    t = {AND: ta * tb, OR: ta + tb + ta * tb, XOR: ta + tb, NOT: ta + 1, SELECT: ts * (ta + tb) + tb, KEEP: ts * ta}[op]
    parts = {AND: ta * tb, OR: ta * tb, SELECT: ts * (ta + tb), KEEP: ts * ta}.get(op, 0)
    return t if t < LIMIT and parts < LIMIT else 0


def bitwise_clear(op, a, b=0, s=0):
    """The clear value of one bit."""
    return {AND: a & b, OR: a | b, XOR: a ^ b, NOT: 1 - a, SELECT: a if s else b, KEEP: a if s else 0}[op]
