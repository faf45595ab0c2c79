"""What the csgn_matmul tests share: include/csgn_hip.h's definition of the product of encrypted bit matrices, by its
decode in numpy on uniform batches and as the literal left-nested composition over any (add, mul) pair of tests/model.py
(ref_ops, oracle_ops)."""
import numpy as np

from tests.model import LIMIT


def matmul_terms(inner, ta, tb):
    """inner * t_a * t_b by the definition itself (Python integers: no overflow); 0 for a zero argument or past 2^62."""
    if not (inner and ta and tb) or ta >= LIMIT or tb >= LIMIT:
        return 0
    T = inner * ta * tb
    return T if T < LIMIT else 0


def np_matmul(a, b, rows, inner, cols, transposed=False):
    """Words of C by the decode: a = words[rows * inner, t_a, dL], b = words[inner * cols, t_b, dL] (transposed:
    element k * inner + e).  Term q = (e * t_a + a) * t_b + b of element i * cols + k is A[i,e][a] & B[e,k][b].  Returns
    words[rows * cols, inner * t_a * t_b, dL]."""
    ta, dl = a.shape[1], a.shape[2]
    tb = b.shape[1]
    assert a.shape[0] == rows * inner and b.shape[0] == inner * cols
    A = a.reshape(rows, inner, ta, dl)
    B = b.reshape(cols, inner, tb, dl) if transposed else b.reshape(inner, cols, tb, dl).transpose(1, 0, 2, 3)
    C = A[:, None, :, :, None, :] & B[None, :, :, None, :, :]          # [i, k, e, a, b, word]
    return C.reshape(rows * cols, inner * ta * tb, dl)


def compose_matmul(ops, a, b, rows, inner, cols, transposed=False):
    """The definition, literally: C[i,k] = ((A[i,0] * B[0,k]) + (A[i,1] * B[1,k])) + ... through ops = (add, mul) on flat
    word arrays.  a[i * inner + e], b[e * cols + k] (transposed: b[k * inner + e]): one flat array per element.  Returns
    one flat array per output element, row-major."""
    add, mul = ops
    out = []
    for i in range(rows):
        for k in range(cols):
            acc = None
            for e in range(inner):
                p = mul(a[i * inner + e], b[k * inner + e] if transposed else b[e * cols + k])
                acc = p if acc is None else add(acc, p)
            out.append(acc)
    return out


def sum_groups_offsets(offsets, group):
    """CiphertextBatch::sumGroups on a ragged batch: every group-th offset."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    count = len(offsets) - 1
    assert group >= 1 and count % group == 0
    return offsets[::group]
