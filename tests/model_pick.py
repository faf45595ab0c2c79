"""include/csgn_hip.h's definition of csgn_uint_pick in numpy, beside tests/model.py: an encrypted integer shifted or
rotated by an encrypted distance, or an element's own array read at its encrypted index.  Output j is the left-nested
sum, ascending in r < rows_j, of EQ(index, r) * a_{src(j, r)} -- EQ the LEFT operand, csgn_uint_plain's EQ row with
k = r -- composed here over any (add, mul, one, zero) from tests/model.py's pieces, and restated term by term as the
kernel decodes it: entry q of the E stream of the LONGEST output gives (r, digits), and output j drops the entries
q >= E_j (rows are concatenated ascending, so a shorter output's stream is a prefix)."""
import numpy as np

from tests.model import EQ, compose_plain, const_term, np_add, np_mul, np_plain, read_terms, u64s

SHL, SHR, ROTL, ROTR, EACH = range(1, 6)
OPS = {"shl": SHL, "shr": SHR, "rotl": ROTL, "rotr": ROTR, "each": EACH}
SHIFTS = (SHL, SHR, ROTL, ROTR)


def rows_of(op, v, w, n, j):
    """rows_j: the rows output j sums over (n: EACH's row count, ignored by the others)."""
    return {SHL: min(j + 1, 1 << v), SHR: min(w - j, 1 << v), ROTL: 1 << v, ROTR: 1 << v, EACH: n}[op]


def rows_max(op, v, w, n):
    return max(rows_of(op, v, w, n, j) for j in range(w))


def src_of(op, w, j, r):
    """The source plane of row r of output j (EACH: plane j, of the element's row r)."""
    return {SHL: j - r, SHR: j + r, ROTL: (j - r) % w, ROTR: (j + r) % w, EACH: j}[op]


def pick_terms(op, s, w, n, j):
    """E_j by the definition itself: the EQ terms of output j's rows."""
    return read_terms(s, rows_of(op, len(s), w, n, j))


def c_pick_terms(lib, op, v, s, w, n, j):
    return int(lib.csgn_uint_pick_terms(op, v, u64s(s) if s is not None else None, w, n, j))


def clear_pick(op, w, n, a, d):
    """What the outputs decrypt to: a = the integer (EACH: the element's array, a list), d = the distance / index."""
    mask = (1 << w) - 1
    if op == SHL:
        return (a << d) & mask if d < w else 0
    if op == SHR:
        return a >> d if d < w else 0
    if op == ROTL:
        d %= w
        return ((a << d) | (a >> (w - d))) & mask
    if op == ROTR:
        d %= w
        return ((a >> d) | (a << (w - d))) & mask
    return int(a[d]) if d < n else 0


def compose_pick(op, index, value, w, n, add, mul, one, zero):
    """The definition in exactly its order, over any operators.  index: the v index planes; value(p, r): source plane p
    (of the element's row r, for EACH).  One value per output plane."""
    v = len(index)
    eqs = {}
    outs = []
    for j in range(w):
        out = None
        for r in range(rows_of(op, v, w, n, j)):
            if r not in eqs:
                eqs[r] = compose_plain(EQ, index, r, add, mul, one, zero)
            p = mul(eqs[r], value(src_of(op, w, j, r), r))
            out = p if out is None else add(out, p)
        outs.append(out)
    return outs


def np_value(op, a, n):
    """value(p, r) over uniform planes a[p] = words[batch (* n), t, dL]."""
    return (lambda p, r: a[p][r::n]) if op == EACH else (lambda p, r: a[p])


def np_pick(n_bits, op, index, a, n=0):
    """Words of every output over uniform planes: index[k] = words[batch, s_k, dL], a[p] = words[batch, t, dL], or, for
    EACH, words[batch * n, t, dL] with element e's array the elements e * n .. e * n + n - 1."""
    batch, _, dl = index[0].shape
    one = np.broadcast_to(const_term(n_bits, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n_bits, 0), (batch, 1, dl))
    return compose_pick(op, index, np_value(op, a, n), len(a), n, np_add, np_mul, one, zero)


def np_pick_fast(n_bits, op, index, a, n=0):
    """np_pick's words with every output concatenated once (a left-nested sum of concatenations is one concatenation):
    linear in the output, for the large shapes of the device tests."""
    v, w = len(index), len(a)
    value = np_value(op, a, n)
    eqs = [np_plain(n_bits, EQ, index, r) for r in range(rows_max(op, v, w, n))]
    return [np.concatenate([np_mul(eqs[r], value(src_of(op, w, j, r), r)) for r in range(rows_of(op, v, w, n, j))],
                           axis=1) for j in range(w)]


# -- the decode: what k_uint_pick does with a position ------------------------------------------------------------------
def decode(q, s, rows):
    """Entry q of the E stream of `rows` rows: (r, digits d_k), csgn_uint_read's term order, by the walk from the top
    index bit down and the mixed-radix digits inside row r's block."""
    v = len(s)
    F = [1] * v
    for k in range(1, v):
        F[k] = F[k - 1] * (2 * s[k - 1] + 1)
    last, r, H, tight = rows - 1, 0, 1, True
    for k in reversed(range(v)):
        if tight and not (last >> k) & 1:
            H *= s[k] + 1
            continue
        c0 = H * (s[k] + 1) * F[k]
        if q < c0:
            H *= s[k] + 1
            tight = False
        else:
            q -= c0
            r |= 1 << k
            H *= s[k]
    assert q < H
    digits = [0] * v
    for k in reversed(range(v)):
        R = s[k] if (r >> k) & 1 else s[k] + 1
        digits[k] = q % R
        q //= R
    return r, digits


def np_pick_decoded(n_bits, op, index, a, n=0):
    """The same words term by term, the kernel's way: every entry q below E_max is decoded ONCE against rows_max; output
    j takes it when q < E_j, as term q * t + c = AND over k of (digit < s_k ? x_k[digit] : ONE) AND term c of the
    source the row names."""
    batch, _, dl = index[0].shape
    s = [p.shape[1] for p in index]
    v, w, t = len(s), len(a), a[0].shape[1]
    value = np_value(op, a, n)
    E = [pick_terms(op, s, w, n, j) for j in range(w)]
    outs = [np.empty((batch, E[j] * t, dl), dtype=np.uint64) for j in range(w)]
    one = const_term(n_bits, 1)
    for q in range(max(E)):
        r, digits = decode(q, s, rows_max(op, v, w, n))
        sel = np.broadcast_to(one, (batch, dl)).copy()
        for k, dg in enumerate(digits):
            if dg < s[k]:
                sel &= index[k][:, dg, :]
        for j in range(w):
            if q >= E[j]:
                continue                                             # past output j's prefix
            assert r < rows_of(op, v, w, n, j)
            outs[j][:, q * t:(q + 1) * t, :] = sel[:, None, :] & value(src_of(op, w, j, r), r)
    return outs
