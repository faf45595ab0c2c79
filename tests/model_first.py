"""What the csgn_uint_first tests share: include/csgn_hip.h's definition of the first set row over any (add, mul, one),
its numpy forms on uniform planes, its term counts and the term order the kernel decodes, restated."""
import numpy as np

from tests.model import LIMIT, const_term, np_add, np_mul, u64s


def compose_first(mask_rows, value_rows, labels, add, mul, one):
    """include/csgn_hip.h's definition, in exactly its order.  mask_rows[r]: m_r; value_rows[r][j]: plane j of value
    row r; labels: the rows' public constants, or None.  Returns (one value per value plane, any, {bit: label plane})
    with only the label planes some label reaches."""
    g = len(mask_rows)
    out, any_, lab, run = None, None, {}, None
    for r in range(g):
        F = mask_rows[r] if r == 0 else mul(run, mask_rows[r])
        if r + 1 < g:
            n_r = add(mask_rows[r], one)
            run = n_r if r == 0 else mul(run, n_r)
        prods = [mul(F, d) for d in value_rows[r]]
        out = prods if out is None else [add(o, p) for o, p in zip(out, prods)]
        any_ = F if any_ is None else add(any_, F)
        for i in range(64):
            if labels is not None and (int(labels[r]) >> i) & 1:
                lab[i] = add(lab[i], F) if i in lab else F
    return out, any_, lab


def np_first(n, mask_rows, value_rows, labels=None):
    """Words of every output over uniform rows: mask_rows[r] = words[batch, s_r, dL], value_rows[r][j] = words[batch,
    t_j, dL]."""
    batch, _, dl = mask_rows[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    return compose_first(mask_rows, value_rows, labels, np_add, np_mul, one)


def np_first_fast(n, mask_rows, value_rows, labels=None):
    """np_first's words with every sum concatenated once (a left-nested sum of concatenations is one concatenation)
    and the running product carried along, not rebuilt."""
    batch, _, dl = mask_rows[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    F, run = [], None
    for r, m in enumerate(mask_rows):
        F.append(m if r == 0 else np_mul(run, m))
        if r + 1 < len(mask_rows):
            n_r = np_add(m, one)
            run = n_r if r == 0 else np_mul(run, n_r)
    w = len(value_rows[0])
    outs = [np.concatenate([np_mul(F[r], value_rows[r][j]) for r in range(len(F))], axis=1) for j in range(w)]
    lab = {}
    for i in range(64):
        rows = [r for r in range(len(F)) if labels is not None and (int(labels[r]) >> i) & 1]
        if rows:
            lab[i] = np.concatenate([F[r] for r in rows], axis=1)
    return outs, np.concatenate(F, axis=1), lab


def first_terms(s, row):
    """P_row (row < g) or Q (row == g) by the definition itself; 0 past 2^62."""
    P = [int(s[r]) * int(np.prod([x + 1 for x in s[:r]], dtype=object)) for r in range(len(s))]
    T = sum(P) if row == len(s) else P[row]
    return T if T < LIMIT else 0


def label_terms(s, labels, bit):
    T = sum(first_terms(s, r) for r in range(len(s)) if (int(labels[r]) >> bit) & 1)
    return T if T < LIMIT else 0


def c_terms(lib, g, s, row):
    return int(lib.csgn_uint_first_terms(g, u64s(s) if s is not None else None, row))


def c_label_terms(lib, g, s, labels, bit):
    return int(lib.csgn_uint_first_label_terms(g, u64s(s) if s is not None else None,
                                               u64s(labels) if labels is not None else None, bit))


# -- the term order the kernel decodes (csgn_uint_first.hip) ----------------------------------------------------------
def entry_digits(r, i, s):
    """Entry i of row r's block: (digit of m_r, [digits of n_0 .. n_{r-1}]); m_r's is the fastest, n_0's the slowest."""
    dm = i % s[r]
    i //= s[r]
    dn = [0] * r
    for x in reversed(range(r)):
        dn[x] = i % (s[x] + 1)
        i //= s[x] + 1
    assert i == 0
    return dm, dn


def fresh_subset(q):
    """Fresh rows: (r, S), the row of entry q (the top bit of q + 1) and the rows entry q ANDs: m_r and the m_x, x < r,
    whose binary digit is 0 (1 is ONE)."""
    r = (q + 1).bit_length() - 1
    dm, dn = entry_digits(r, q + 1 - (1 << r), [1] * (r + 1))
    return r, (1 << r) | sum(1 << x for x in range(r) if dn[x] == 0)


def np_first_decoded(n, mask_rows, value_rows, labels=None):
    """The same words term by term from the decode: the F stream entry by entry, then term q * t_j + c of out_j =
    (entry q) & (term c of d_{r(q),j}), any the bare stream, label plane i the blocks of the rows that have bit i."""
    batch, _, dl = mask_rows[0].shape
    g, s = len(mask_rows), [m.shape[1] for m in mask_rows]
    one = const_term(n, 1)
    P = [first_terms(s, r) for r in range(g)]
    stream, row = np.empty((batch, sum(P), dl), dtype=np.uint64), []
    q = 0
    for r in range(g):
        for i in range(P[r]):
            dm, dn = entry_digits(r, i, s)
            v = mask_rows[r][:, dm, :].copy()
            for x, dg in enumerate(dn):
                v &= mask_rows[x][:, dg, :] if dg < s[x] else one
            stream[:, q, :] = v
            row.append(r)
            q += 1
    row = np.array(row)
    outs = []
    for j in range(len(value_rows[0])):
        t = value_rows[0][j].shape[1]
        o = np.empty((batch, len(row) * t, dl), dtype=np.uint64)
        for q, r in enumerate(row):
            for c in range(t):
                o[:, q * t + c, :] = stream[:, q, :] & value_rows[r][j][:, c, :]
        outs.append(o)
    lab = {}
    for i in range(64):
        keep = [(int(labels[r]) >> i) & 1 == 1 for r in range(g)] if labels is not None else []
        if any(keep):
            lab[i] = stream[:, [q for q, r in enumerate(row) if keep[r]], :]
    return outs, stream, lab
