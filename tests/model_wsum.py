"""What the csgn_wsum tests share: include/csgn_hip.h's definition of the bits of a sum of encrypted bits of public
weights 2^c -- plane j the sum, over the count vectors (m_j .. m_0) with sum m_c 2^c = 2^j and over their selections, of
the product of the selected inputs --, by its decode in numpy on uniform batches and as the literal nested-loop
composition over any (add, mul) pair of tests/model.py (ref_ops, oracle_ops)."""
from itertools import combinations, product
from math import comb

import numpy as np

from tests.model import LIMIT

MAX_CLASSES, MAX_INPUTS, MAX_PLANE = 64, 65536, 62


def wsum_terms(ns, t, j):
    """T_j: the coefficient of z^(2^j) in prod_c (1 + t z^(2^c))^(n_c), in Python integers (no overflow).  0 for a bad
    argument, a plane with no count vector or a count of 2^62 or more."""
    if not (1 <= len(ns) <= MAX_CLASSES and 1 <= sum(ns) <= MAX_INPUTS and 0 < t < LIMIT and 0 <= j <= MAX_PLANE):
        return 0
    target = 1 << j
    poly = {0: 1}
    for c, n in enumerate(ns):
        w = 1 << c
        if w > target:
            break
        nxt = {}
        for deg, coef in poly.items():
            for m in range(min(n, (target - deg) // w) + 1):
                d = deg + m * w
                nxt[d] = nxt.get(d, 0) + coef * comb(n, m) * t ** m
        poly = nxt
    T = poly.get(target, 0)
    return T if T < LIMIT else 0


def count_vectors(ns, j):
    """The count vectors of plane j as lists m[c], c = 0 .. j, in the definition's order: the nested loops
    `for m_j = 0...: for m_{j-1} = 0...:`, m_0 the remainder, skipped when it exceeds n_0 (n_c = 0 for c >= C)."""
    n = list(ns) + [0] * (j + 1 - len(ns))
    out = []

    def loops(c, rest, m):
        if c == 0:
            if rest <= n[0]:
                out.append([rest] + m)
            return
        for k in range(min(n[c], rest >> c) + 1):
            loops(c - 1, rest - (k << c), [k] + m)

    loops(j, 1 << j, [])
    return out


def selections(ns, m):
    """The selections of a count vector in the definition's order, each as the monomial's factors [(class, index), ...]:
    S_j slowest, S_0 fastest, every class lexicographic; factors by class descending, index ascending."""
    classes = [c for c in range(len(m) - 1, -1, -1) if m[c]]
    for pick in product(*[combinations(range(ns[c]), m[c]) for c in classes]):
        yield [(c, i) for c, s in zip(classes, pick) for i in s]


def np_wsum(xs, ns, js):
    """Words of the planes js by the decode.  xs[c] = words[count * n_c, t, dL] (None or empty where n_c = 0), input i
    of element q at q * n_c + i.  Returns one array words[count, T_j, dL] per plane."""
    first = next(x for x, n in zip(xs, ns) if n)
    count, t, dl = first.shape[0] // next(n for n in ns if n), first.shape[1], first.shape[2]
    X = [None if not n else x.reshape(count, n, t, dl) for x, n in zip(xs, ns)]
    outs = []
    for j in js:
        parts = []
        for m in count_vectors(ns, j):
            sel = list(selections(ns, m))
            deg = len(sel[0])
            acc = None
            for k in range(deg):
                c = sel[0][k][0]
                f = X[c][:, np.array([s[k][1] for s in sel], dtype=np.int64)]            # [count, nsel, t, dL]
                acc = f if acc is None else (acc[:, :, :, None, :] & f[:, :, None, :, :]).reshape(count, len(sel), -1, dl)
            parts.append(acc.reshape(count, -1, dl))
        assert parts, "plane %d has no count vector" % j
        outs.append(np.concatenate(parts, axis=1))
    return outs


def compose_wsum(ops, classes, j):
    """The definition, literally, for ONE element: the left-nested sum over the count vectors and their selections (the
    nested loops, in their own order) of the left-nested product of the selection's members, through ops = (add, mul)
    on flat word arrays.  classes[c]: the inputs of class c, one flat array each."""
    add, mul = ops
    ns = [len(k) for k in classes]
    acc = None
    for m in count_vectors(ns, j):
        for factors in selections(ns, m):
            prod = None
            for c, i in factors:
                prod = classes[c][i] if prod is None else mul(prod, classes[c][i])
            acc = prod if acc is None else add(acc, prod)
    return acc


def product_classes(a_planes, b_planes, mul):
    """The classes of a * b: class c holds a_i * b_{c-i}, i ascending, a on the left.  Planes are words[count, t, dL];
    returns (xs, ns) for np_wsum."""
    wa, wb = len(a_planes), len(b_planes)
    xs, ns = [], []
    for c in range(wa + wb - 1):
        prods = [mul(a_planes[i], b_planes[c - i]) for i in range(wa) if 0 <= c - i < wb]
        ns.append(len(prods))
        xs.append(np.stack(prods, axis=1).reshape(-1, prods[0].shape[1], prods[0].shape[2]))
    return xs, ns
