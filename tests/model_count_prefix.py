"""What the csgn_count_prefix tests share: include/csgn_hip.h's definition of the running counts of encrypted bits, row
r of a group the count (tests/model_count.py, np_count) of the group's first r + 1 - exclusive inputs, or the one zero
term where 2^j passes them; the rows of a plane one after the other, their offsets by summation."""
import numpy as np

from tests.model import LIMIT
from tests.model_count import count_terms, np_count


def row_inputs(r, exclusive):
    """n_r: the inputs row r counts."""
    return r + 1 - (1 if exclusive else 0)


def row_terms(g, t, j, exclusive, r):
    """T_{r,j}: the count's terms of n_r inputs, or 1, the zero term, where 2^j > n_r.  None where the count's own term
    count reaches 2^62."""
    n = row_inputs(r, exclusive)
    if (1 << j) > n:
        return 1
    T = count_terms(n, t, j)
    return T if T else None


def prefix_offset(g, t, j, exclusive, r):
    """off_j(r), the sum of T_{r',j} over r' < r (r = g: A_j), one row at a time; 0 for an invalid shape -- a zero
    argument, j > 6, 2^j > g - exclusive, t >= 2^62, r > g -- or a sum of 2^62 or more."""
    if exclusive not in (0, 1):
        return 0
    ex = int(exclusive)
    if not (g and t) or g >= LIMIT or t >= LIMIT or j > 6 or (1 << j) > g - ex or r > g:
        return 0
    total = 0
    for rr in range(r):
        T = row_terms(g, t, j, exclusive, rr)
        if T is None:
            return 0
        total += T
        if total >= LIMIT:
            return 0
    return total


def np_count_prefix(x, g, js, exclusive=False, layout="grouped"):
    """Words of the plane blocks js.  x as in np_count (grouped: words[count * g, t, dL]; planes: g arrays
    words[count, t, dL]).  Returns per plane the list of its g rows, row r an array words[count, T_{r,j}, dL]: np_count
    over the first n_r inputs, or zeros where 2^j > n_r."""
    if layout == "planes":
        assert len(x) == g
        X = np.stack(x, axis=1)                                         # [count, g, t, dL]
    else:
        X = x.reshape(-1, g, x.shape[1], x.shape[2])
    count, _, t, dl = X.shape
    outs = []
    for j in js:
        rows = []
        for r in range(g):
            n = row_inputs(r, exclusive)
            if (1 << j) > n:
                rows.append(np.zeros((count, 1, dl), dtype=np.uint64))
            else:
                prefix = np.ascontiguousarray(X[:, :n]).reshape(count * n, t, dl)
                rows.append(np_count(prefix, n, [j])[0])
        outs.append(rows)
    return outs


def block_words(rows):
    """A plane's block as the C ABI lays it out: the rows one after the other, each `count` elements."""
    return np.concatenate([r.ravel() for r in rows])


def split_block(block, g, t, j, exclusive, count, dl):
    """The rows of a downloaded block, by the summed offsets: a list of arrays words[count, T_{r,j}, dL]."""
    rows = []
    for r in range(g):
        a, b = prefix_offset(g, t, j, exclusive, r), prefix_offset(g, t, j, exclusive, r + 1)
        rows.append(block[count * a * dl: count * b * dl].reshape(count, b - a, dl))
    return rows
