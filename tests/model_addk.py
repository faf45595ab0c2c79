"""What the csgn_uint_addk tests share: include/csgn_hip.h's definition of a + k over any (add, mul, one, zero), its
numpy form on uniform planes, its term counts, and the shapes the device tests run."""
import numpy as np

from tests.model import LIMIT, const_term, np_add, np_mul


def compose_addk(planes, k, add, mul, one, zero=None):
    """The table of include/csgn_hip.h, in exactly its order.  Returns (out planes, carry-out)."""
    w = len(planes)
    if k == 0:
        return list(planes), zero
    m = next(j for j in range(w) if (k >> j) & 1)
    out = list(planes[:m]) + [add(planes[m], one)]
    c = planes[m]
    for j in range(m + 1, w):
        a = planes[j]
        if (k >> j) & 1:
            out.append(add(add(a, c), one))
            c = add(mul(c, add(a, one)), a)
        else:
            out.append(add(a, c))
            c = mul(c, a)
    return out, c


def np_addk(n, planes, k, negate=False):
    """Words of every output plane and of the carry-out over uniform planes (words[batch, t_j, dL], bit 0 first);
    negate appends ONE to every output plane, never to the carry-out."""
    batch, _, dl = planes[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    outs, carry = compose_addk(planes, k, np_add, np_mul, one, zero)
    if negate:
        outs = [np_add(o, one) for o in outs]
    return outs, carry


def addk_terms(w, k, t):
    """The same composition over term counts (Python integers: no overflow): w + 1 counts, or None past 2^62."""
    outs, carry = compose_addk(list(t), k, lambda x, y: x + y, lambda x, y: x * y, 1, 1)
    counts = outs + [carry]
    return counts if all(c < LIMIT for c in counts) else None


def mask(w):
    return (1 << w) - 1


# derived operations: the constant and negate flag csgn_uint_addk is called with
def sub_k(w, k):
    return (-k) & mask(w), False            # a - k


def rsub_k(w, k):
    return ~k & mask(w), True               # k - a


def neg_k(w):
    return mask(w), True                    # -a


def term_modes(w, mode, rng):
    return [int(x) for x in rng.integers(1, 4, w)] if mode == "mixed" else [int(mode)] * w


def full_width_ks(w):
    """The issue's list at widths past 16: 0, 1, the top bit, eight set bits at the top, and bits {0, 16, 31, 32, w-1}
    below w."""
    scattered = sum(1 << b for b in {0, 16, 31, 32, w - 1} if b < w)
    return [0, 1, 1 << (w - 1), (1 << w) - (1 << (w - 8)), scattered]
