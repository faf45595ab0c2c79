"""What the csgn_uint_find tests share: include/csgn_hip.h's definition of the keyed lookup over any (add, mul, one),
its numpy forms on uniform planes, its term counts and the term order the kernel decodes, restated."""
import numpy as np

from tests.model import LIMIT, const_term, np_add, np_mul, u64s


def compose_eq(y, x, add, mul, one):
    """equalTo(a = key row, b = query) of certfhe/UInt.h: logicXnor on plane 0, then the EQ_STEP chain."""
    e = add(add(y[0], x[0]), one)
    for k in range(1, len(y)):
        e = mul(e, add(add(y[k], x[k]), one))
    return e


def compose_find(key_rows, query, value_rows, add, mul, one, member=False):
    """include/csgn_hip.h's definition, in exactly its order.  key_rows[r][k]: plane k of key row r (broadcast to the
    query's elements), query[k], value_rows[r][j]: plane j of value row r.  Returns (one value per value plane, member or
    None)."""
    out, mem = None, None
    for r in range(len(key_rows)):
        eq = compose_eq(key_rows[r], query, add, mul, one)
        prods = [mul(eq, d) for d in value_rows[r]]
        out = prods if out is None else [add(o, p) for o, p in zip(out, prods)]
        if member:
            mem = eq if mem is None else add(mem, eq)
    return out, mem


def tile_rows(planes, batch):
    """rows[r][k]: row r of every plane (words[rows, t, dL]) broadcast to `batch` elements."""
    return [[np.broadcast_to(p[r:r + 1], (batch,) + p.shape[1:]) for p in planes] for r in range(planes[0].shape[0])]


def np_find(n, keys, query, values, member=False):
    """Words of every output (and member) over uniform planes: keys[k] = words[rows, u_k, dL], query[k] =
    words[batch, s_k, dL], values[j] = words[rows, t_j, dL]."""
    batch, _, dl = query[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    rows = keys[0].shape[0]
    value_rows = tile_rows(values, batch) if values else [[] for _ in range(rows)]
    return compose_find(tile_rows(keys, batch), query, value_rows, np_add, np_mul, one, member)


def np_find_fast(n, keys, query, values, member=False):
    """np_find's words with every row at once (a left-nested sum of concatenations is one concatenation): the EQ of
    every (element, row) as one array, then one AND per output."""
    batch, _, dl = query[0].shape
    rows = keys[0].shape[0]
    one = np.broadcast_to(const_term(n, 1), (batch, rows, 1, dl))
    eq = None
    for y, x in zip(keys, query):
        g = np.concatenate([np.broadcast_to(y[None], (batch,) + y.shape),
                            np.broadcast_to(x[:, None], (batch, rows) + x.shape[1:]), one], axis=2)
        eq = g if eq is None else (eq[:, :, :, None, :] & g[:, :, None, :, :]).reshape(batch, rows, -1, dl)
    outs = [(eq[:, :, :, None, :] & d[None, :, None, :, :]).reshape(batch, -1, dl) for d in values]
    return outs, (eq.reshape(batch, -1, dl) if member else None)


def find_terms(u, s):
    """P by the definition itself; 0 past 2^62."""
    P = 1
    for uk, sk in zip(u, s):
        P *= uk + sk + 1
    return P if P < LIMIT else 0


def c_P(lib, v, u, s):
    return int(lib.csgn_uint_find_terms(v, u64s(u) if u is not None else None, u64s(s) if s is not None else None))


# -- the term order the kernel decodes (csgn_uint_find.hip) -----------------------------------------------------------
def digits(q, u, s):
    """Entry q of a row's block: the mixed-radix digits d_k < u_k + s_k + 1, k = 0 slowest."""
    d = [0] * len(u)
    for k in reversed(range(len(u))):
        R = u[k] + s[k] + 1
        d[k] = q % R
        q //= R
    assert q == 0
    return d


def fresh_subsets(q, v):
    """Fresh planes: (Sk, Sq), the key planes (digit 0) and the query planes (digit 1) entry q ANDs; digit 2 is ONE."""
    d = digits(q, [1] * v, [1] * v)
    return (sum(1 << k for k in range(v) if d[k] == 0), sum(1 << k for k in range(v) if d[k] == 1))


def np_find_decoded(n, keys, query, values, member=False):
    """The same words term by term from the decode: term (r * P + q) * t_j + c = AND over k of the term digit d_k
    selects (of y_{r,k}, of x_k, or ONE) AND term c of d_{r,j}."""
    batch, _, dl = query[0].shape
    u, s = [p.shape[1] for p in keys], [p.shape[1] for p in query]
    rows, P = keys[0].shape[0], find_terms(u, s)
    one = const_term(n, 1)
    eq = np.empty((batch, rows * P, dl), dtype=np.uint64)
    for r in range(rows):
        for q in range(P):
            v = np.broadcast_to(one, (batch, dl)).copy()
            for k, dg in enumerate(digits(q, u, s)):
                if dg < u[k]:
                    v &= keys[k][r, dg, :]
                elif dg < u[k] + s[k]:
                    v &= query[k][:, dg - u[k], :]
            eq[:, r * P + q, :] = v
    outs = []
    for d in values:
        t = d.shape[1]
        o = np.empty((batch, rows * P * t, dl), dtype=np.uint64)
        for r in range(rows):
            for c in range(t):
                o[:, r * P * t + c:(r + 1) * P * t:t, :] = eq[:, r * P:(r + 1) * P, :] & d[r, c, :]
        outs.append(o)
    return outs, (eq if member else None)
