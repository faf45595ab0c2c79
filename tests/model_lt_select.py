"""What the csgn_uint_lt_select tests share: include/csgn_hip.h's definition of selection by an encrypted comparison over
any (add, mul, one), its numpy forms on uniform planes, its term counts and the term order the kernel decodes,
restated."""
import numpy as np

from tests.model import LIMIT, MUX, const_term, np_gate, np_uint_lt, u64s


def lt_counts(ta, tb):
    """L_j of every plane by the definition itself (Python integers: no overflow)."""
    Ls = [(ta[0] + 1) * tb[0]]
    for j in range(1, len(ta)):
        Ls.append((ta[j] + tb[j]) * (tb[j] + Ls[-1]) + Ls[-1])
    return Ls


def lt_terms(ta, tb):
    """L; 0 past 2^62 (the products and sums of the recurrence only grow, so the last decides)."""
    L = lt_counts(ta, tb)[-1]
    return L if L < LIMIT else 0


def out_terms(L, tx, ty):
    return L * (tx + ty) + ty


def c_L(lib, w, ta, tb):
    return int(lib.csgn_uint_lt_terms(w, u64s(ta) if ta is not None else None, u64s(tb) if tb is not None else None))


# -- the definition over any (add, mul, one) ---------------------------------------------------------------------------
def compose_lt(a, b, add, mul, one):
    """lessThan(a, b) of certfhe/UInt.h: LT_FIRST on plane 0, then the LT_STEP chain."""
    lt = mul(add(a[0], one), b[0])
    for j in range(1, len(a)):
        lt = add(mul(add(a[j], b[j]), add(b[j], lt)), lt)
    return lt


def compose_lt_select(a, b, xs, ys, add, mul, one, less=False):
    """include/csgn_hip.h's definition, in exactly its order.  Returns (one value per request, L or None)."""
    lt = compose_lt(a, b, add, mul, one)
    return [add(mul(lt, add(x, y)), y) for x, y in zip(xs, ys)], (lt if less else None)


def np_lt_select(n, a, b, xs, ys, less=False):
    """Words of every output (and L) over uniform planes (words[batch, terms, dL]): tests/model.py's np_uint_lt and the
    MUX row of np_gate."""
    lt = np_uint_lt(n, a, b)
    return [np_gate(n, MUX, a=x, b=y, sel=lt) for x, y in zip(xs, ys)], (lt if less else None)


# -- the term order the kernel decodes (csgn_uint_lt_select.hip) ------------------------------------------------------
def decode(q, ta, tb):
    """Term q of L as its factors: a list of ("a" | "b", plane, term); ONE contributes nothing."""
    Ls = lt_counts(ta, tb)
    assert 0 <= q < Ls[-1]
    f = []
    for j in range(len(ta) - 1, 0, -1):
        inner = tb[j] + Ls[j - 1]
        M = (ta[j] + tb[j]) * inner
        if q >= M:                                  # the tail copy of l_{j-1}
            q -= M
            continue
        p, c = divmod(q, inner)
        f.append(("a", j, p) if p < ta[j] else ("b", j, p - ta[j]))
        if c < tb[j]:
            f.append(("b", j, c))
            return f
        q = c - tb[j]
    p, c = divmod(q, tb[0])
    if p < ta[0]:
        f.append(("a", 0, p))
    f.append(("b", 0, c))
    return f


def fresh_subsets(q, w):
    """Fresh planes: (Sa, Sb), the planes of a and of b term q ANDs."""
    f = decode(q, [1] * w, [1] * w)
    return (sum({1 << j for s, j, _ in f if s == "a"}), sum({1 << j for s, j, _ in f if s == "b"}))


def np_lt_decoded(n, a, b):
    batch, _, dl = a[0].shape
    ta, tb = [p.shape[1] for p in a], [p.shape[1] for p in b]
    L = lt_terms(ta, tb)
    lt = np.empty((batch, L, dl), dtype=np.uint64)
    for q in range(L):
        v = np.broadcast_to(const_term(n, 1), (batch, dl)).copy()
        for s, j, t in decode(q, ta, tb):
            v &= (a if s == "a" else b)[j][:, t, :]
        lt[:, q, :] = v
    return lt


def place(lt, xs, ys):
    """The outputs from L's words by the term order alone: term q * (tx + ty) + c is L_q & (X | Y)_c, then Y's tail."""
    batch, L, dl = lt.shape
    outs = []
    for x, y in zip(xs, ys):
        tx, ty = x.shape[1], y.shape[1]
        o = np.empty((batch, out_terms(L, tx, ty), dl), dtype=np.uint64)
        body = o[:, :L * (tx + ty)].reshape(batch, L, tx + ty, dl)
        np.bitwise_and(lt[:, :, None, :], x[:, None, :, :], out=body[:, :, :tx])
        np.bitwise_and(lt[:, :, None, :], y[:, None, :, :], out=body[:, :, tx:])
        o[:, L * (tx + ty):] = y
        outs.append(o)
    return outs


def np_lt_select_decoded(n, a, b, xs, ys, less=False):
    """The same words term by term from the decode."""
    lt = np_lt_decoded(n, a, b)
    return place(lt, xs, ys), (lt if less else None)


def np_lt_select_fast(n, a, b, xs, ys, less=False):
    """np_lt_select's words with L computed once and every output written in place (no concatenations of the outputs):
    linear in the output, for the large shapes of the device tests."""
    lt = np_uint_lt(n, a, b)
    return place(lt, xs, ys), (lt if less else None)


def minmax_requests(a, b):
    """The requests of min (a_j, b_j) then max (b_j, a_j)."""
    return list(a) + list(b), list(b) + list(a)
