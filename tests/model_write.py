"""include/csgn_hip.h's definition of csgn_uint_write in numpy, beside tests/model.py and tests/model_pick.py: element
e's own array of n rows written with the element's value at its encrypted index.  Row r of plane j becomes
logicMux(EQ(index, r), value_j, d_{r,j}) = (EQ(index, r) * (value_j + d_{r,j})) + d_{r,j} -- EQ the LEFT operand,
csgn_uint_plain's EQ row with k = r, the sum inside a concatenation with the value's terms first -- composed here over
any (add, mul, one, zero) from tests/model.py's pieces, restated as one concatenation placed by the closed-form offsets,
and restated term by term as the kernel decodes it: entry q of the E stream of n rows gives (r, digits), term c of the
entry lies at q * (tv + td) + r * td + c, and the row's raw copy follows the row's last entry."""
import numpy as np

from tests.model import EQ, compose_plain, const_term, np_add, np_mul, np_plain, read_terms, u64s
from tests.model_pick import decode


def row_terms(s, r):
    """P_r = prod_k R_k(r), R_k = r_k ? s_k : s_k + 1: the terms of EQ(index, r)."""
    p = 1
    for k, sk in enumerate(s):
        p *= sk if (r >> k) & 1 else sk + 1
    return p


def write_row_terms(s, r, tv, td):
    """The terms of row r of an output plane, by the definition itself: P_r * (tv + td) + td."""
    return row_terms(s, r) * (tv + td) + td


def write_offset_by_rows(s, r, tv, td):
    """The first term of row r inside its array: the rows below it, added up."""
    return sum(write_row_terms(s, x, tv, td) for x in range(r))


def write_offset(s, r, tv, td):
    """The same in closed form: qstart(r) * (tv + td) + r * td with qstart(r) the E stream's entries below row r."""
    return (read_terms(s, r) if r else 0) * (tv + td) + r * td


def array_terms(s, n, tv, td):
    """A = E * (tv + td) + n * td."""
    return read_terms(s, n) * (tv + td) + n * td


def c_write_offset(lib, v, s, n, r, tv, td):
    return int(lib.csgn_uint_write_offset(v, u64s(s) if s is not None else None, n, r, tv, td))


def clear_write(n, array, index, value):
    """What the outputs decrypt to: the array with row `index` replaced by `value`, untouched where index >= n."""
    out = [int(x) for x in array]
    if index < n:
        out[index] = int(value)
    return out


def compose_write(index, value, rows, add, mul, one, zero):
    """The definition in exactly its order, over any operators.  index: the v index planes; value[j]: plane j of the
    value; rows[r][j]: plane j of row r of the element's array.  out[r][j]: row r of output plane j."""
    out = []
    for r in range(len(rows)):
        eq = compose_plain(EQ, index, r, add, mul, one, zero)
        out.append([add(mul(eq, add(value[j], rows[r][j])), rows[r][j]) for j in range(len(value))])
    return out


def np_rows(arrays, n):
    """rows[r][j] over uniform planes arrays[j] = words[batch * n, td_j, dL]."""
    return [[a[r::n] for a in arrays] for r in range(n)]


def np_write(n_bits, index, value, arrays, n):
    """Words of every output plane over uniform planes: index[k] = words[batch, s_k, dL], value[j] = words[batch, tv_j,
    dL], arrays[j] = words[batch * n, td_j, dL] with element e's array the elements e * n .. e * n + n - 1.  Output j:
    words[batch, A_j, dL], the rows of an array one after the other."""
    batch, _, dl = index[0].shape
    one = np.broadcast_to(const_term(n_bits, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n_bits, 0), (batch, 1, dl))
    out = compose_write(index, value, np_rows(arrays, n), np_add, np_mul, one, zero)
    return [np.concatenate([out[r][j] for r in range(n)], axis=1) for j in range(len(value))]


def np_write_fast(n_bits, index, value, arrays, n):
    """np_write's words with every piece written once into its place by the closed-form offsets: linear in the output,
    for the large shapes of the device tests."""
    batch, _, dl = index[0].shape
    s = [p.shape[1] for p in index]
    outs = [np.empty((batch, array_terms(s, n, v.shape[1], a.shape[1]), dl), dtype=np.uint64)
            for v, a in zip(value, arrays)]
    for r in range(n):
        eq = np_plain(n_bits, EQ, index, r)
        assert eq.shape[1] == row_terms(s, r)
        for j, (v, a) in enumerate(zip(value, arrays)):
            tv, td = v.shape[1], a.shape[1]
            row = a[r::n]
            at = write_offset(s, r, tv, td)
            mid = at + eq.shape[1] * (tv + td)
            o = outs[j][:, at:mid, :].reshape(batch, eq.shape[1], tv + td, dl)
            np.bitwise_and(eq[:, :, None, :], v[:, None, :, :], out=o[:, :, :tv, :])
            np.bitwise_and(eq[:, :, None, :], row[:, None, :, :], out=o[:, :, tv:, :])
            outs[j][:, mid:mid + td, :] = row
            assert mid + td == write_offset(s, r + 1, tv, td)
    return outs


def is_last_entry(s, r, digits):
    """Whether an entry of row r is the row's last: every digit maximal -- s_k - 1 for a one-bit of r, s_k (ONE) for a
    zero-bit."""
    return all(dg == (sk - 1 if (r >> k) & 1 else sk) for k, (sk, dg) in enumerate(zip(s, digits)))


def np_write_decoded(n_bits, index, value, arrays, n):
    """The same words term by term, the kernel's way: every entry q of the E stream of n rows is decoded once into (r,
    digits); term c < tv + td of it lies at q * (tv + td) + r * td + c and is the entry ANDed with value term c or row
    term c - tv; the lane that writes a product term from a row term of the row's LAST entry writes that term's raw copy
    td terms further on."""
    batch, _, dl = index[0].shape
    s = [p.shape[1] for p in index]
    outs = [np.full((batch, array_terms(s, n, v.shape[1], a.shape[1]), dl), np.uint64(0x5A5A5A5A5A5A5A5A))
            for v, a in zip(value, arrays)]
    written = [np.zeros(o.shape[1], dtype=np.int64) for o in outs]
    one = const_term(n_bits, 1)
    for q in range(read_terms(s, n)):
        r, digits = decode(q, s, n)
        sel = np.broadcast_to(one, (batch, dl)).copy()
        for k, dg in enumerate(digits):
            if dg < s[k]:
                sel &= index[k][:, dg, :]
        last = is_last_entry(s, r, digits)
        for j, (v, a) in enumerate(zip(value, arrays)):
            tv, td = v.shape[1], a.shape[1]
            row = a[r::n]
            for c in range(tv + td):
                at = q * (tv + td) + r * td + c
                operand = v[:, c, :] if c < tv else row[:, c - tv, :]
                outs[j][:, at, :] = sel & operand
                written[j][at] += 1
                if last and c >= tv:
                    outs[j][:, at + td, :] = operand
                    written[j][at + td] += 1
    for x in written:
        assert (x == 1).all(), "a term written twice or never"
    return outs
