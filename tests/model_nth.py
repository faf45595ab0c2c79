"""What the csgn_uint_nth tests share: include/csgn_hip.h's definition of the (slot + 1)-th set row over any (add, mul),
its numpy forms on uniform planes, its term counts in Python integers and the term order the kernel decodes, restated."""
from itertools import combinations
from math import comb

import numpy as np

from tests.model import LIMIT, np_add, np_mul


def kept_degrees(slot, top):
    """The d in slot..top with C(d, slot) odd, ascending."""
    return [d for d in range(slot, top + 1) if comb(d, slot) % 2 == 1]


def compose_nth(mask_rows, value_rows, labels, slot, add, mul):
    """include/csgn_hip.h's definition, in exactly its loop order.  mask_rows[r]: m_r; value_rows[r][j]: plane j of
    value row r; labels: the rows' public constants, or None.  Returns (one value per value plane, valid, {bit: label
    plane}) with only the label planes some row from the slot on reaches."""
    g = len(mask_rows)
    out, valid, lab = None, None, {}
    for r in range(slot, g):
        G = None
        for d in kept_degrees(slot, r):
            for sub in combinations(range(r), d):                     # lexicographic
                p = None
                for i in sub + (r,):
                    p = mask_rows[i] if p is None else mul(p, mask_rows[i])
                G = p if G is None else add(G, p)
        prods = [mul(G, d) for d in value_rows[r]]
        out = prods if out is None else [add(o, p) for o, p in zip(out, prods)]
        valid = G if valid is None else add(valid, G)
        for i in range(64):
            if labels is not None and (int(labels[r]) >> i) & 1:
                lab[i] = add(lab[i], G) if i in lab else G
    return out, valid, lab


def np_nth(mask_rows, value_rows, slot, labels=None):
    """Words of every output over uniform rows: mask_rows[r] = words[batch, t, dL], value_rows[r][j] = words[batch, t_j,
    dL]."""
    return compose_nth(mask_rows, value_rows, labels, slot, np_add, np_mul)


def nth_terms(g, t, slot, row):
    """P_{row,slot} (row < g) or Q_slot (row == g) by the definition itself; 0 past 2^62."""
    if row == g:
        T = sum(comb(g, d + 1) * t ** (d + 1) for d in kept_degrees(slot, g - 1))
    else:
        T = sum(comb(row, d) * t ** (d + 1) for d in kept_degrees(slot, row))
    return T if T < LIMIT else 0


def label_terms(g, t, slot, labels, bit):
    P = [nth_terms(g, t, slot, r) for r in range(slot, g) if (int(labels[r]) >> bit) & 1]
    T = sum(P)
    return T if T < LIMIT and all(P) else 0


def c_terms(lib, g, t, slot, row):
    return int(lib.csgn_uint_nth_terms(g, t, slot, row))


def c_label_terms(lib, g, t, slot, labels, bit):
    from tests.model import u64s
    return int(lib.csgn_uint_nth_label_terms(g, t, slot, u64s(labels) if labels is not None else None, bit))


# -- the term order the kernel decodes (csgn_uint_nth.hip) -------------------------------------------------------------
def entries(g, t, slot):
    """The stream entry by entry: (r, [(row, digit), ...]) with the factors in the order i_1 .. i_d, r.  Blocks
    ascending in r, segments ascending in d, subsets by lexicographic rank, the digits in base t with i_1's slowest."""
    out = []
    for r in range(slot, g):
        for d in kept_degrees(slot, r):
            for sub in combinations(range(r), d):
                rows = sub + (r,)
                for x in range(t ** (d + 1)):
                    digits = [(x // t ** (d - k)) % t for k in range(d + 1)]
                    out.append((r, list(zip(rows, digits))))
    return out


def np_nth_decoded(mask_rows, value_rows, slot, labels=None):
    """The same words term by term from the decode: the G stream entry by entry, then term q * t_j + c of out_j =
    (entry q) & (term c of d_{r(q),j}), valid the bare stream, label plane i the blocks of the rows that have bit i."""
    batch, t, dl = mask_rows[0].shape
    g = len(mask_rows)
    ent = entries(g, t, slot)
    stream = np.empty((batch, len(ent), dl), dtype=np.uint64)
    for q, (r, factors) in enumerate(ent):
        v = None
        for row, dg in factors:
            v = mask_rows[row][:, dg, :].copy() if v is None else v & mask_rows[row][:, dg, :]
        stream[:, q, :] = v
    row = np.array([r for r, _ in ent])
    outs = []
    for j in range(len(value_rows[0])):
        tj = value_rows[0][j].shape[1]
        o = np.empty((batch, len(row) * tj, dl), dtype=np.uint64)
        for q, r in enumerate(row):
            o[:, q * tj:(q + 1) * tj, :] = stream[:, q, None, :] & value_rows[r][j]
        outs.append(o)
    lab = {}
    for i in range(64):
        keep = [labels is not None and r >= slot and (int(labels[r]) >> i) & 1 == 1 for r in range(g)]
        if any(keep):
            lab[i] = stream[:, [q for q, r in enumerate(row) if keep[r]], :]
    return outs, stream, lab


def np_nth_fast(mask_rows, value_rows, slot, labels=None):
    """np_nth's words with every sum concatenated once (a left-nested sum of concatenations is one concatenation) and a
    subset's product built from its prefix's."""
    g = len(mask_rows)
    G = {}
    for r in range(slot, g):
        parts = []
        for d in kept_degrees(slot, r):
            memo = {(): None}
            for sub in combinations(range(r), d):
                for k in range(1, d + 1):                             # the prefixes, left-nested
                    if sub[:k] not in memo:
                        p = memo[sub[:k - 1]]
                        memo[sub[:k]] = mask_rows[sub[k - 1]] if p is None else np_mul(p, mask_rows[sub[k - 1]])
                p = memo[sub]
                parts.append(mask_rows[r] if p is None else np_mul(p, mask_rows[r]))
        G[r] = np.concatenate(parts, axis=1)
    rows = list(range(slot, g))
    w = len(value_rows[0])
    outs = [np.concatenate([np_mul(G[r], value_rows[r][j]) for r in rows], axis=1) for j in range(w)]
    lab = {}
    for i in range(64):
        kept = [r for r in rows if labels is not None and (int(labels[r]) >> i) & 1]
        if kept:
            lab[i] = np.concatenate([G[r] for r in kept], axis=1)
    return outs, np.concatenate([G[r] for r in rows], axis=1), lab
