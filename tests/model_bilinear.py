"""The model of csgn_uint_bilinear (include/csgn_hip.h): a public bilinear form over F2 of two bit-sliced encrypted
integers.  The definition from tests/model.py's np_add, np_mul and const_term; the same definition over any `add` and
`mul`; the terms table and the decode by position; a symbolic version over labels; the clear value; certfhe/UInt.h's
F2Bilinear builders restated; and the kernel's grid (tile, workgroup, position) replayed from
csgn_uint_bilinear_launches' figures.  A form is a list, per output plane, of (left, right) pairs."""
from collections import Counter

import numpy as np

from tests.model import LIMIT, const_term, np_add, np_mul
from tests.model_linear import low

ONE, ZERO = "one", "zero"               # the decode's constant entries (n_entries and n_entries + 1 in the C ABI)
MAX_ENTRIES = 262144


# -- the definition ----------------------------------------------------------------------------------------------------
def compose_bilinear(a, b, form, constant, add, mul, one, zero):
    """include/csgn_hip.h's definition in exactly its order, over any `add` and `mul`: one value per plane."""
    outs = []
    for x, pairs in enumerate(form):
        r = None
        for left, right in pairs:
            p = mul(a[left], b[right])
            r = p if r is None else add(r, p)
        if (constant >> x) & 1:
            r = one if r is None else add(r, one)
        outs.append(zero if r is None else r)
    return outs


def np_bilinear(n, a, b, form, constant=0):
    """Words of every output plane over uniform planes (words[batch, t, dL], bit 0 first)."""
    batch, _, dl = a[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    return [np.ascontiguousarray(o) for o in compose_bilinear(a, b, form, constant, np_add, np_mul, one, zero)]


# -- the terms table and the decode by position ------------------------------------------------------------------------
def bilinear_terms(ta, tb, pairs, cbit):
    """T of one plane; 0 where the C ABI refuses (a width, a zero count, an index past the planes, 2^62 or more)."""
    if not (1 <= len(ta) <= 64 and 1 <= len(tb) <= 64) or cbit not in (0, 1):
        return 0
    if any(t == 0 or t >= LIMIT for t in list(ta) + list(tb)) or any(i >= len(ta) or l >= len(tb) for i, l in pairs):
        return 0
    total = 0
    for i, l in pairs:
        if ta[i] * tb[l] >= LIMIT:
            return 0
        total += ta[i] * tb[l]
        if total >= LIMIT:
            return 0
    total += cbit if pairs else 1
    return total if total < LIMIT else 0


def bilinear_decode(ta, tb, pairs, cbit, q):
    """(entry, left term, right term) of output term q of a plane; entry ONE / ZERO for the constant."""
    for x, (i, l) in enumerate(pairs):
        if q < ta[i] * tb[l]:
            return (x,) + divmod(q, tb[l])
        q -= ta[i] * tb[l]
    assert q == 0 and (cbit or not pairs)
    return (ONE if cbit else ZERO), 0, 0


def symbolic_bilinear(ta, tb, form, constant):
    """The definition over lists of labels (left plane, left term, right plane, right term): what the decode must give
    term for term."""
    a = [[(i, x) for x in range(t)] for i, t in enumerate(ta)]
    b = [[(l, y) for y in range(t)] for l, t in enumerate(tb)]
    return compose_bilinear(a, b, form, constant, lambda x, y: x + y, lambda x, y: [u + v for u in x for v in y],
                            [(ONE,)], [(ZERO,)])


def plane_table(ta, tb, pairs, cbit):
    """Per term of a plane: arrays (left plane, left term, right plane, right term); -1 for the constant term."""
    cols = [[], [], [], []]
    for i, l in pairs:
        lt, rt = np.divmod(np.arange(ta[i] * tb[l]), tb[l])
        for c, v in zip(cols, (np.full(lt.size, i), lt, np.full(lt.size, l), rt)):
            c.append(v)
    if cbit or not pairs:
        for c in cols:
            c.append(np.array([-1]))
    return [np.concatenate(c).astype(np.int64) for c in cols]


# -- the clear value ---------------------------------------------------------------------------------------------------
def clear_bilinear(form, constant, x, y):
    z = 0
    for j, pairs in enumerate(form):
        bit = 0
        for i, l in pairs:
            bit ^= (x >> i) & (y >> l) & 1
        z |= bit << j
    return z ^ constant


# -- F2Bilinear's builders, restated -----------------------------------------------------------------------------------
def cancel(pairs):
    """Duplicates cancel over F2; what stays is sorted by (left, right)."""
    return sorted(p for p, c in Counter(pairs).items() if c % 2)


def f_clmul_wide(w):
    return [[(i, j - i) for i in range(w) if 0 <= j - i < w] for j in range(2 * w - 1)]


def f_clmul(w):
    return f_clmul_wide(w)[:w]


def reduction_rows(w, poly):
    """Rows (masks over the 2w - 1 planes of the wide product) of the reduction modulo x^w + poly's low w bits."""
    red = [1]                                                        # x^k mod poly, k < 2w - 1
    for _ in range(2 * w - 2):
        a = red[-1] << 1
        red.append((a & low(w)) ^ (poly & low(w)) if a >> w else a)
    return [sum(((r >> j) & 1) << k for k, r in enumerate(red)) for j in range(w)]


def f_gf_mul(w, poly):
    rows = reduction_rows(w, poly)
    return [[(i, l) for i in range(w) for l in range(w) if (rows[j] >> (i + l)) & 1] for j in range(w)]


def f_bitwise_and(w):
    return [[(j, j)] for j in range(w)]


def f_dot_bits(w):
    return [[(j, j) for j in range(w)]]


def f_xor(f, g):
    return [cancel(p + q) for p, q in zip(f, g)]


def f_after(rows, form):
    """The linear map `rows` (masks over the form's planes) after the form."""
    return [cancel([p for j in range(len(form)) if (row >> j) & 1 for p in form[j]]) for row in rows]


def f_compose(form, on_a, on_b):
    """The form after the linear maps on_a and on_b (rows of masks) of its arguments."""
    bits = lambda m: [i for i in range(64) if (m >> i) & 1]          # noqa: E731
    return [cancel([(i, l) for left, right in pairs for i in bits(on_a[left]) for l in bits(on_b[right])]) for pairs in form]


def random_form(wa, wb, n_out, per_plane, seed):
    rng = np.random.default_rng(seed)
    return [[(int(rng.integers(0, wa)), int(rng.integers(0, wb))) for _ in range(per_plane)] for _ in range(n_out)]


# -- the kernel's grid, replayed from the launches' figures ------------------------------------------------------------
def replay_grid(ta, tb, form, constant, batch, U, G, S, chunk, staged, stage_units, launch_blocks, order=None):
    """Every position of every workgroup of every launch of k_uint_bilinear at U units a term, G elements a tile, S
    workgroups a tile and `chunk` units a workgroup, as csgn_uint_bilinear.hip places them: returns (count[x]: per-unit
    write counts of output plane x, launches, workgroups per tile, workgroups of the first launch) and asserts every source index in range --
    of the operand planes and, staged, of the LDS copy of stage_units units.  A workgroup's lanes write the positions
    lo + lane, + 256, ... below hi: together the range [lo, hi).  Sources come from plane_table, not from the kernel's
    own search: the words are compared on the device; here it is the coverage.  order(b, nblocks), when given, is the
    launch's block order (xcd_contiguous_block): hardware block b does the work of logical block order(b, nblocks)."""
    T = [bilinear_terms(ta, tb, p, (constant >> x) & 1) for x, p in enumerate(form)]
    tables = [plane_table(ta, tb, p, (constant >> x) & 1) for x, p in enumerate(form)]
    assert chunk % 256 == 0 and all(len(t[0]) == Tx for t, Tx in zip(tables, T))
    PU = sum(T) * U
    assert S * chunk >= G * PU
    tiles = -(-batch // G)
    per_launch = max(1, launch_blocks // S)
    tin = np.array(list(ta) + list(tb))
    opre = np.concatenate([[0], np.cumsum(tin)])                     # operand terms before compact plane i
    if staged:
        assert G * int(opre[-1]) * U <= stage_units
    count = [np.zeros(batch * t * U, dtype=np.int64) for t in T]
    launches = first_blocks = 0
    for t0 in range(0, tiles, per_launch):
        nt = min(per_launch, tiles - t0)
        e_base = t0 * G
        ne = min(batch - e_base, nt * G)
        if launches == 0:
            first_blocks = nt * S
        launches += 1
        for hw in range(nt * S):
            bid = order(hw, nt * S) if order else hw
            assert 0 <= bid < nt * S
            tile, s = divmod(bid, S)
            e0 = tile * G
            assert e0 < ne
            ge = min(G, ne - e0)
            total, lo = ge * PU, s * chunk
            if lo >= total:
                continue
            pos = np.arange(lo, min(lo + chunk, total))
            tpos, k = np.divmod(pos, U)
            pre = ge * np.concatenate([[0], np.cumsum(T)])
            p = np.searchsorted(pre, tpos, side="right") - 1
            assert p.min() >= 0 and p.max() < len(form)
            for x in np.unique(p):
                m = p == x
                off = tpos[m] - pre[x]
                el, term = np.divmod(off, T[x])
                assert el.max() < ge
                L, lt, R, rt = (c[term] for c in tables[x])
                live = L >= 0
                for side, plane, t in ((0, L[live], lt[live]), (len(ta), R[live], rt[live])):
                    if plane.size == 0:
                        continue
                    terms = tin[side + plane]
                    assert (t < terms).all() and (e_base + e0 + el[live]).max() < batch
                    if staged:
                        at = ge * opre[side + plane] * U + (el[live] * terms + t) * U + k[m][live]
                        assert at.max() < ge * int(opre[-1]) * U <= stage_units
                np.add.at(count[x], ((e_base + e0) * T[x] + off) * U + k[m], 1)
    return count, launches, S, first_blocks


# -- the shapes of tests/test_uint_bilinear_gpu.py, which tests/test_uint_bilinear_cpu.py replays on the host ----------
NS = (64, 1247, 1300)                   # one 8-byte unit a term; 16-byte units (10 a term); 8-byte units (21 a term)


def term_counts(w, ramp):
    return [1 + i for i in range(w)] if ramp else [1] * w           # (1, 2, 3, ...) or one term each


def small_form(wa, wb):
    """(form, constant): one pair; all pairs; empty; empty with the constant; a pair twice; pairs out of order; a row
    with the constant."""
    every = [(i, l) for i in range(wa) for l in range(wb)]
    top = (wa - 1, wb - 1)
    form = [[top], every, [], [], [top, (0, 0), top], every[::-1][:4], every[:3]]
    return form, 0b1001000


def gpu_shapes():
    """(name, ta, tb, form, constant, batches) at every n of NS: every pair of widths with one-term planes (the
    divisions), and ramps on either side or both (the table)."""
    shapes = []
    for wa in (1, 2, 3, 5):
        for wb in (1, 2, 3, 5):
            form, constant = small_form(wa, wb)
            shapes.append(("%dx%d-ones" % (wa, wb), term_counts(wa, False), term_counts(wb, False), form, constant,
                           (1, 3, 257)))
    for wa, wb, ra, rb in ((2, 3, True, False), (3, 2, False, True), (5, 5, True, True), (1, 5, False, True),
                           (5, 1, True, False), (3, 3, True, True), (2, 2, True, True), (5, 3, True, True)):
        form, constant = small_form(wa, wb)
        name = "%dx%d-ramp%s%s" % (wa, wb, "A" if ra else "", "B" if rb else "")
        shapes.append((name, term_counts(wa, ra), term_counts(wb, rb), form, constant, (1, 3, 257)))
    return shapes


# entry ends at terms 3, 18, 158, 228, 234 and 374 of an element at n = 64 (one unit a term): inside a wave and past one
BOUNDARIES = ("boundaries", [3, 70], [1, 5, 2], [[(0, 0), (0, 1), (1, 2), (1, 0), (0, 2), (1, 2)], [(1, 1), (0, 0)], []],
              0b101, (1, 7, 40))


def alternating(w, x, y):
    return [x if i % 2 == 0 else y for i in range(w)]


# (name, n, ta, tb, form, constant, batches)
DENSE = [
    ("clmulwide32", 1247, [1] * 32, [1] * 32, f_clmul_wide(32), 0, (2,)),
    ("random64", 1247, [1] * 64, [1] * 64, random_form(64, 64, 64, 32, 64), 0x8000000000000001 | (0xF0 << 24), (2,)),
    ("random64", 64, [1] * 64, [1] * 64, random_form(64, 64, 64, 32, 64), 0x8000000000000001 | (0xF0 << 24), (33,)),
    ("random64-ragged", 64, alternating(64, 1, 2), alternating(64, 2, 1), random_form(64, 64, 64, 32, 65), 1 << 63, (33,)),
]

# 215 operand terms of 160 bytes at n = 1247 pass the 16 KiB of LDS; 102 terms are the most that fit
UNSTAGED = ("past-the-budget", [70, 40], [60, 45], [[(0, 0)], [(1, 1), (0, 1)], [(1, 0)]], 0b010, (2,))
STAGED_EDGE = ("at-the-budget", [35, 20], [30, 17], [[(0, 0)], [(1, 1), (0, 1)], [(1, 0)]], 0b010, (2,))
PAST_EDGE = ("one-term-past", [35, 20], [30, 18], [[(0, 0)], [(1, 1), (0, 1)], [(1, 0)]], 0b010, (2,))

# tests/test_uint_bilinear_gpu.py's aliased operands: (ta, tb, form, constant) at every n of NS, batch 5
SQUARE_FORM = [[(0, 0)], [(0, 1), (1, 0)], [(2, 2), (1, 1)], [(0, 2), (1, 1), (2, 0)]]
ALIASED = [([2, 2, 1], [2, 2, 1], SQUARE_FORM, 0b1000), ([2, 2, 1], [1, 3], [[(0, 0), (1, 0)], [(1, 1), (0, 1), (2, 0)]], 0b01),
           ([3, 3, 3], [3, 3, 3], SQUARE_FORM, 0)]
ALIASED_BATCH = 5
# its block-order test at several tiles: (dense shape, batch): staged with one element a tile; unstaged with twelve
XCD_DENSE = [(DENSE[0], 7), (DENSE[1], 29)]
# its tiles-and-launches test: (n, index into gpu_shapes()): more than 5 elements a tile and more than 1 workgroup a tile
TILE_SHAPES = [(64, 18), (1247, 21), (1300, 21)]
