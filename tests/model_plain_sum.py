"""The model of csgn_uint_plain_sum (include/csgn_hip.h): sums over F2 of comparisons of one bit-sliced encrypted
integer against public constants.  The definition from tests/model.py's np_plain, np_add and const_term; the same
definition over any (add, mul); the term counts from plain_terms; the decode by position; the clear range, set, step
function and sparse table with certfhe/UInt.h's entry lists restated; the kernel's grid (plane, element, run, unit)
replayed on the host; and the shapes of tests/test_uint_plain_sum_gpu.py."""
import numpy as np

from tests.model import EQ, GE, GT, LE, LIMIT, LT, NE, compose_plain, const_term, full_width_cases, np_add, np_mul, plain_terms

ONE, ZERO = "one", "zero"               # the decode's constant planes (width and width + 1 in the C ABI)
RUN = 16                                # terms per lane item (csgn_uint_plain_sum.hip's kRun)


# -- the definition ----------------------------------------------------------------------------------------------------
def compose_plain_sum(planes, planes_entries, constant, add, mul, one, zero):
    """include/csgn_hip.h's definition in exactly its order, over any (add, mul): one value per output plane."""
    outs = []
    for x, entries in enumerate(planes_entries):
        r = None
        for cmp, k in entries:
            v = compose_plain(cmp, planes, k, add, mul, one, zero)
            r = v if r is None else add(r, v)
        if (constant >> x) & 1:
            r = one if r is None else add(r, one)
        outs.append(zero if r is None else r)
    return outs


def np_plain_sum(n, planes, planes_entries, constant=0):
    """Words of every output plane over uniform planes (words[batch, t_j, dL], bit 0 first)."""
    batch, _, dl = planes[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    return [np.ascontiguousarray(o) for o in compose_plain_sum(planes, planes_entries, constant, np_add, np_mul, one, zero)]


# -- the term counts and the decode by position ------------------------------------------------------------------------
def entry_terms(ta, cmp, k):
    w = len(ta)
    if not 1 <= w <= 64 or cmp not in (EQ, NE, LT, LE, GT, GE) or k >> w or any(t == 0 or t >= LIMIT for t in ta):
        return 0
    return plain_terms(cmp, w, k, ta)


def sum_terms(ta, entries, cbit):
    """T of one plane; 0 where the C ABI refuses (an entry csgn_uint_plain_terms refuses, 2^62 or more)."""
    if cbit not in (0, 1) or not 1 <= len(ta) <= 64 or any(t == 0 or t >= LIMIT for t in ta):
        return 0
    total = 0
    for cmp, k in entries:
        t = entry_terms(ta, cmp, k)
        if t == 0:
            return 0
        total += t
    total += cbit if entries else 1
    return total if total < LIMIT else 0


def symbolic_plain_sum(ta, planes_entries, constant):
    """The definition over lists of terms, a term being the tuple of its factors' (plane, term) labels: what the decode
    must give, term for term (as a multiset of factors: AND commutes)."""
    planes = [[((j, i),) for i in range(t)] for j, t in enumerate(ta)]
    return compose_plain_sum(planes, planes_entries, constant, lambda x, y: x + y,
                             lambda x, y: [a + b for a in x for b in y], [((ONE, 0),)], [((ZERO, 0),)])


def decode(ta, entries, cbit, q):
    """The factors of term q of one plane, sorted."""
    return sorted(symbolic_plain_sum(ta, [entries], cbit)[0][q], key=str)


def rebuild(n, planes, factors):
    """words[batch, dL] of the AND of the factors over uniform planes."""
    batch, _, dl = planes[0].shape
    v = np.broadcast_to(const_term(n, 1), (batch, dl)).copy()
    for plane, term in factors:
        if plane == ZERO:
            v[:] = 0
        elif plane != ONE:
            v &= planes[plane][:, term, :]
    return v


# -- the clear functions and certfhe/UInt.h's entry lists, restated -------------------------------------------------------
def clear_plain(cmp, a, k):
    return int({EQ: a == k, NE: a != k, LT: a < k, LE: a <= k, GT: a > k, GE: a >= k}[cmp])


def clear_plain_sum(planes_entries, constant, a):
    y = 0
    for x, entries in enumerate(planes_entries):
        y |= (sum(clear_plain(c, a, k) for c, k in entries) & 1) << x
    return y ^ constant


def range_entries(w, lo, hi):
    """(entries, constant bit) of lo <= a <= hi."""
    top = (1 << w) - 1
    assert 0 <= lo <= hi <= top
    if lo == 0 and hi == top:
        return [], 1
    if lo == 0:
        return [(LE, hi)], 0
    if hi == top:
        return [(GE, lo)], 0
    return [(LT, hi + 1), (LT, lo)], 0


def ranges_entries(w, intervals):
    entries, cbit = [], 0
    for lo, hi in intervals:
        e, c = range_entries(w, lo, hi)
        entries += e
        cbit ^= c
    return entries, cbit


def set_entries(keys):
    return [(EQ, k) for k in sorted(set(keys))], 0


def step_entries(thresholds, values, out_width):
    """(planes_entries, constant): plane j sums LT(a, t_i) where bit j of v_{i-1} ^ v_i is set, plus bit j of v_m."""
    assert len(values) == len(thresholds) + 1
    planes = [[(LT, t) for i, t in enumerate(thresholds) if ((values[i] ^ values[i + 1]) >> j) & 1] for j in range(out_width)]
    return planes, values[-1] & ((1 << out_width) - 1)


def sparse_entries(keys, values, out_width, otherwise=0):
    table = {}
    for k, v in zip(keys, values):
        table.setdefault(k, v)
    planes = [[(EQ, k) for k in sorted(table) if ((table[k] ^ otherwise) >> j) & 1] for j in range(out_width)]
    return planes, otherwise & ((1 << out_width) - 1)


def clear_range(lo, hi, a):
    return int(lo <= a <= hi)


def clear_step(thresholds, values, a):
    return values[sum(1 for t in thresholds if a >= t)]


def clear_sparse(keys, values, otherwise, a):
    for k, v in zip(keys, values):
        if k == a:
            return v
    return otherwise


# -- the kernel's grid, replayed ---------------------------------------------------------------------------------------
def plane_runs(ta, entries, cbit):
    """(first run of every entry, runs of the entries, runs of the plane with its constant's)."""
    starts, runs = [], 0
    for cmp, k in entries:
        starts.append(runs)
        t = entry_terms(ta, cmp, k)
        runs += -(-t // min(t, RUN))
    return starts, runs, runs + (1 if cbit or not entries else 0)


def replay_grid(ta, planes_entries, constant, batch, U, launch_blocks):
    """Every lane of every launch of k_uint_plain_sum at U units a term, placed as csgn_uint_plain_sum.hip places it.
    Returns (count[x]: per-item visit counts of plane x, launches, elements and workgroups of the first launch) and
    asserts that a workgroup the kernel takes for one entry's (the uniform path) holds lanes of that entry only."""
    info = [plane_runs(ta, e, (constant >> x) & 1) for x, e in enumerate(planes_entries)]
    ipe = [r[2] * U for r in info]
    np_ = len(planes_entries)
    assert sum(-(-i // 256) for i in ipe) <= (1 << 32) // 256, "more than one plane group: not replayed here"
    epl = max(1, (launch_blocks - np_) * 256 // sum(ipe)) if launch_blocks > np_ else 1
    count = [np.zeros(batch * i, dtype=np.int64) for i in ipe]
    launches, first = 0, (0, 0)
    for e0 in range(0, batch, epl):
        ne = min(epl, batch - e0)
        blocks = [-(-ne * i // 256) for i in ipe]
        bfirst = np.concatenate([[0], np.cumsum(blocks)])
        if launches == 0:
            first = (ne, int(bfirst[-1]))
        launches += 1
        for bid in range(int(bfirst[-1])):
            p = int(np.searchsorted(bfirst, bid, side="right")) - 1
            starts, eruns, runs = info[p]
            nent = len(starts)
            total = ne * ipe[p]
            g0 = (bid - int(bfirst[p])) * 256
            assert g0 < total
            g = g0 + np.arange(256)
            g = g[g < total]
            e, rem = g // ipe[p], g % ipe[p]
            run = rem // U
            ent = np.where(run >= eruns, nent, np.searchsorted(np.asarray(starts + [eruns]), run, side="right") - 1)
            single = nent + (runs - eruns) == 1                       # the kernel's rule, from its first and last item
            if e[0] == e[-1]:
                single = ent[0] == ent[-1]
            if single:
                assert (ent == ent[0]).all(), (p, bid)
            assert (e0 + e).max() < batch
            np.add.at(count[p], (e0 + e) * ipe[p] + rem, 1)
    return count, launches, first


# -- the shapes of tests/test_uint_plain_sum_gpu.py, which tests/test_uint_plain_sum_cpu.py decodes and replays ----------
NS = (64, 1247, 1300)                   # one 8-byte unit a term; 16-byte units (10 a term); 8-byte units (21 a term)


def wide_plane(w, limit=300):
    """Every (cmp, k) of full_width_cases(w) of at most `limit` terms over fresh planes: k at both ends and in the
    middle, the ZERO constants among them."""
    return [(c, k) for c, k in full_width_cases(w) if plain_terms(c, w, k, [1] * w) <= limit]


def gpu_shapes():
    """(name, ta, planes_entries, constant, batches)."""
    shapes = []
    # a range: LT + LT
    shapes.append(("range-w3", [1] * 3, [range_entries(3, 2, 5)[0]], 0, (1, 3, 257)))
    shapes.append(("range-w8", [1] * 8, [range_entries(8, 17, 200)[0], range_entries(8, 1, 254)[0]], 0b10, (1, 3, 257)))
    # all six comparisons in one plane (an appended ONE in the middle, entries behind it); ZERO entries; empty planes
    # with and without the constant; a single entry with and without the constant
    shapes.append(("mixed", [1] * 4,
                   [[(EQ, 5), (NE, 9), (LT, 6), (LE, 3), (GT, 7), (GE, 12), (EQ, 0)],
                    [(LT, 0), (GT, 15), (GE, 0), (LE, 15), (EQ, 3)],
                    [], [], [(GT, 3)], [(LE, 9)], [(LT, 0)], [(GT, 15)]], 0b10101000, (1, 3, 257)))
    # 1-term entries (EQ with k all ones over fresh planes): entry boundaries at every item of a wave
    shapes.append(("ones", [1] * 3, [[(EQ, 7)] * 70, [(EQ, 7)] * 3 + [(NE, 7)] * 5], 0b01, (1, 3, 257)))
    # entries of 15, 16 and 17 terms: one run, exactly one run, two runs
    ta = [3, 4]
    assert [entry_terms(ta, c, k) for c, k in ((EQ, 1), (EQ, 2), (NE, 2))] == [15, 16, 17]
    shapes.append(("runs", ta, [[(EQ, 1), (EQ, 2), (NE, 2), (EQ, 1)], [(NE, 2), (EQ, 2)]], 0b10, (1, 3, 257)))
    # an entry of 4096 terms = 256 runs: it ends exactly at a workgroup's last item at every U; entries behind it
    shapes.append(("wg-edge", [1] * 12, [[(EQ, 0), (LT, 5), (EQ, 4095)]], 0b1, (1, 3)))
    # input planes of 2 and 3 terms: radices above 1 everywhere, sum tails
    shapes.append(("t23", [2, 3, 2, 3],
                   [[(EQ, 9), (LT, 11), (GT, 4)], [(NE, 0), (LE, 6), (GE, 10), (LT, 8)], [(GT, 14), (LT, 1)]], 0b100,
                   (1, 3, 257)))
    # w = 1
    shapes.append(("w1", [1], [[(c, k) for k in (0, 1) for c in (EQ, NE, LT, LE, GT, GE)], [(EQ, 1)], []], 0b010, (1, 3, 257)))
    shapes.append(("w1-t2", [2], [[(c, k) for k in (0, 1) for c in (EQ, NE, LT, LE, GT, GE)]], 0, (1, 3, 257)))
    # w = 33 and w = 64, k near both ends
    for w in (33, 64):
        cases = wide_plane(w)
        assert len(cases) >= 8 and any(k == 0 for _, k in cases) and any(k == (1 << w) - 1 for _, k in cases)
        shapes.append(("w%d" % w, [1] * w, [cases, cases[::3]], 0b01, (1, 3)))
    # 300 EQ entries in one plane at w = 9: the per-lane search at its depth
    shapes.append(("eq300", [1] * 9, [[(EQ, k) for k in range(212, 512)]], 0, (1, 3)))
    # 64 output planes
    shapes.append(("planes64", [1] * 6, [[(EQ, x)] + ([(LT, x)] if x & 1 else []) for x in range(64)],
                   0x8421_0000_F00F_8001, (1, 3, 257)))
    return shapes
