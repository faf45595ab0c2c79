"""The read that follows csgn_uint_write in numpy (include/csgn_hip.h, csgn_uint_pick_rows_offsets), beside
tests/model_pick.py and tests/model_write.py: an element's own array read at its encrypted index where the ROWS of an
array differ in size -- row r of plane j has T[j][r] terms in every array, which is what csgn_uint_write leaves.
Output j is the left-nested sum, ascending in r < n, of EQ(index, r) * (row r of the array, plane j) -- EQ the LEFT
operand, csgn_uint_plain's EQ row with k = r -- composed here over any (add, mul, one, zero) from tests/model.py's
pieces, restated as one concatenation placed by the offsets, and restated term by term from a POSITION of the output,
the way one launch would have to decode it: the position finds its row by a search of the rows' output offsets, then
(in, c) by a division by the row's T, and the entry qstart(r) + in of the E stream gives the digits."""
import bisect
import ctypes as C

import numpy as np

from tests.model import EQ, compose_plain, const_term, np_add, np_mul, np_plain, read_terms, u64s
from tests.model_pick import decode
from tests.model_write import row_terms, write_row_terms


def write_shaped(s, n, tv=1, td=1):
    """The rows csgn_uint_write leaves from value planes of tv and array planes of td terms."""
    return [write_row_terms(s, r, tv, td) for r in range(n)]


def rows_offsets(s, T):
    """(src_off, out_off), n + 1 entries each: row r's first term inside an array, and the first term of its block of
    P_r * T[r] terms inside an output element; the last entries are A and Tout."""
    src, out = [0], [0]
    for r, t in enumerate(T):
        src.append(src[-1] + t)
        out.append(out[-1] + row_terms(s, r) * t)
    return src, out


def out_terms(s, T):
    return rows_offsets(s, T)[1][-1]


def c_offsets(lib, v, s, n, T):
    """csgn_uint_pick_rows_offsets: (status, src_off, out_off)"""
    src, out = (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))()
    rc = lib.csgn_uint_pick_rows_offsets(v, u64s(s) if s is not None else None, n, u64s(T) if T is not None else None,
                                         src, out)
    return rc, [int(x) for x in src], [int(x) for x in out]


def clear_pick_rows(n, array, index):
    """What the outputs decrypt to."""
    return int(array[index]) if index < n else 0


def compose_pick_rows(index, rows, add, mul, one, zero):
    """The definition in exactly its order, over any operators.  index: the v index planes; rows[r][j]: plane j of row r
    of the element's array.  One value per output plane."""
    outs = []
    eqs = [compose_plain(EQ, index, r, add, mul, one, zero) for r in range(len(rows))]
    for j in range(len(rows[0])):
        out = None
        for r in range(len(rows)):
            p = mul(eqs[r], rows[r][j])
            out = p if out is None else add(out, p)
        outs.append(out)
    return outs


def np_rows(arrays, T):
    """rows[r][j] over planes arrays[j] = words[batch, A_j, dL] with the rows of T[j] inside an array."""
    offs = [rows_offsets([], t)[0] for t in T]
    return [[a[:, o[r]:o[r + 1], :] for a, o in zip(arrays, offs)] for r in range(len(T[0]))]


def np_pick_rows(n_bits, index, arrays, T):
    """Words of every output: index[k] = words[batch, s_k, dL], arrays[j] = words[batch, A_j, dL]."""
    batch, _, dl = index[0].shape
    one = np.broadcast_to(const_term(n_bits, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n_bits, 0), (batch, 1, dl))
    return compose_pick_rows(index, np_rows(arrays, T), np_add, np_mul, one, zero)


def np_pick_rows_fast(n_bits, index, arrays, T):
    """np_pick_rows' words with every block written once into its place by the offsets: linear in the output, for the
    large shapes of the device tests."""
    batch, _, dl = index[0].shape
    s = [p.shape[1] for p in index]
    n = len(T[0])
    offs = [rows_offsets(s, t) for t in T]
    outs = [np.empty((batch, o[1][-1], dl), dtype=np.uint64) for o in offs]
    for r in range(n):
        eq = np_plain(n_bits, EQ, index, r)
        assert eq.shape[1] == row_terms(s, r)
        for j, (a, (src, out)) in enumerate(zip(arrays, offs)):
            t = T[j][r]
            o = outs[j][:, out[r]:out[r + 1], :].reshape(batch, eq.shape[1], t, dl)
            np.bitwise_and(eq[:, :, None, :], a[:, None, src[r]:src[r + 1], :], out=o)
    return outs


def np_pick_rows_decoded(n_bits, index, arrays, T):
    """The same words term by term, from the position: every POSITION p of output j finds the last row whose block begins
    at or before it, p - out(r) = in * T[r] + c, entry qstart(r) + in of the E stream of n rows decodes to (r, digits),
    and the term is the AND over k of (digit < s_k ? x_k[digit] : ONE) AND term c of row r."""
    batch, _, dl = index[0].shape
    s = [p.shape[1] for p in index]
    n = len(T[0])
    one = const_term(n_bits, 1)
    qstart = [read_terms(s, r) if r else 0 for r in range(n)]
    outs = []
    for a, t in zip(arrays, T):
        src, out = rows_offsets(s, t)
        o = np.empty((batch, out[-1], dl), dtype=np.uint64)
        for p in range(out[-1]):
            r = bisect.bisect_right(out, p, 0, n) - 1
            i, c = divmod(p - out[r], t[r])
            row, digits = decode(qstart[r] + i, s, n)
            assert row == r and i < row_terms(s, r)
            sel = np.broadcast_to(one, (batch, dl)).copy()
            for k, dg in enumerate(digits):
                if dg < s[k]:
                    sel &= index[k][:, dg, :]
            o[:, p, :] = sel & a[:, src[r] + c, :]
        outs.append(o)
    return outs
