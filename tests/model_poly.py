"""The model of csgn_uint_poly (include/csgn_hip.h): a public polynomial over F2 of bit-sliced encrypted planes.  The
definition from tests/model.py's np_add, np_mul and const_term; the same definition over any `add` and `mul`; the terms
table and the decode by position; a symbolic version over labels; the clear value; the builders of the common forms
restated; and the kernel's grid (tile, workgroup, position) replayed from csgn_uint_poly_launches' figures.  A form is a
list, per output plane, of monomials; a monomial is a tuple of input plane indices."""
import itertools
from collections import Counter

import numpy as np

from tests.model import LIMIT, const_term, np_add, np_mul

ONE, ZERO = "one", "zero"               # the decode's constant monomials (n_monomials and n_monomials + 1 in the C ABI)
MAX_MONOMIALS = 262144
MAX_DEGREE = 8


# -- the definition ----------------------------------------------------------------------------------------------------
def compose_poly(planes, form, constant, add, mul, one, zero):
    """include/csgn_hip.h's definition in exactly its order, over any `add` and `mul`: one value per plane."""
    outs = []
    for x, monomials in enumerate(form):
        r = None
        for mono in monomials:
            p = planes[mono[0]]
            for f in mono[1:]:
                p = mul(p, planes[f])
            r = p if r is None else add(r, p)
        if (constant >> x) & 1:
            r = one if r is None else add(r, one)
        outs.append(zero if r is None else r)
    return outs


def np_poly(n, planes, form, constant=0):
    """Words of every output plane over uniform planes (words[batch, t, dL])."""
    batch, _, dl = planes[0].shape
    one = np.broadcast_to(const_term(n, 1), (batch, 1, dl))
    zero = np.broadcast_to(const_term(n, 0), (batch, 1, dl))
    return [np.ascontiguousarray(o) for o in compose_poly(planes, form, constant, np_add, np_mul, one, zero)]


# -- the terms table and the decode by position ------------------------------------------------------------------------
def mono_terms(terms, mono):
    p = 1
    for f in mono:
        p *= terms[f]
    return p


def poly_terms(terms, monomials, cbit):
    """T of one plane; 0 where the C ABI refuses (n_in, a zero count, a degree, an index past the planes, 2^62 or more)."""
    if not 1 <= len(terms) <= 256 or cbit not in (0, 1) or any(t == 0 or t >= LIMIT for t in terms):
        return 0
    total = 0
    for mono in monomials:
        if not 1 <= len(mono) <= MAX_DEGREE or any(f >= len(terms) for f in mono):
            return 0
        p = 1
        for f in mono:
            p *= terms[f]
            if p >= LIMIT:
                return 0
        total += p
        if total >= LIMIT:
            return 0
    total += cbit if monomials else 1
    return total if total < LIMIT else 0


def poly_decode(terms, monomials, cbit, q):
    """(monomial, the 8 factor term indices) of output term q of a plane; monomial ONE / ZERO for the constant."""
    for x, mono in enumerate(monomials):
        p = mono_terms(terms, mono)
        if q < p:
            idx = [0] * MAX_DEGREE
            for j in range(len(mono) - 1, -1, -1):
                q, idx[j] = divmod(q, terms[mono[j]])
            return x, tuple(idx)
        q -= p
    assert q == 0 and (cbit or not monomials)
    return (ONE if cbit else ZERO), (0,) * MAX_DEGREE


def symbolic_poly(terms, form, constant):
    """The definition over lists of labels ((plane, term), (plane, term), ...): what the decode must give term for
    term."""
    planes = [[((i, x),) for x in range(t)] for i, t in enumerate(terms)]
    return compose_poly(planes, form, constant, lambda x, y: x + y, lambda x, y: [u + v for u in x for v in y],
                        [(ONE,)], [(ZERO,)])


def plane_table(terms, monomials, cbit):
    """Per term of a plane: (factor plane [T, 8], factor term [T, 8]); plane -1 past the degree and at the constant."""
    P, I = [], []
    for mono in monomials:
        count = mono_terms(terms, mono)
        idx = np.stack(np.unravel_index(np.arange(count), [terms[f] for f in mono]), axis=1)
        pl = np.full((count, MAX_DEGREE), -1, dtype=np.int64)
        it = np.zeros((count, MAX_DEGREE), dtype=np.int64)
        pl[:, :len(mono)] = mono
        it[:, :len(mono)] = idx
        P.append(pl)
        I.append(it)
    if cbit or not monomials:
        P.append(np.full((1, MAX_DEGREE), -1, dtype=np.int64))
        I.append(np.zeros((1, MAX_DEGREE), dtype=np.int64))
    return np.concatenate(P), np.concatenate(I)


# -- the clear value ---------------------------------------------------------------------------------------------------
def clear_poly(form, constant, bits):
    """bits: the clear value of every input plane, as one integer with plane i at bit i."""
    z = 0
    for j, monomials in enumerate(form):
        bit = 0
        for mono in monomials:
            bit ^= int(all((bits >> f) & 1 for f in mono))
        z |= bit << j
    return z ^ constant


def pack_operands(values, widths):
    bits, at = 0, 0
    for v, w in zip(values, widths):
        bits |= (v & ((1 << w) - 1)) << at
        at += w
    return bits


# -- the builders, restated: monomials as sorted tuples of distinct variables, rows sorted by (degree, factors) --------
def cancel(monomials):
    """x.x = x inside a monomial; duplicates cancel over F2; what stays is sorted by (degree, factors).  Returns
    (monomials, constant bit): a monomial of degree 0 is the constant."""
    c = Counter(tuple(sorted(set(m))) for m in monomials)
    kept = sorted((m for m, k in c.items() if k % 2 and m), key=lambda m: (len(m), m))
    return kept, c.get((), 0) % 2


def f_ch(w):
    """Ch(e, f, g) = ef + eg + g over operands e, f, g of w bits."""
    return [cancel([(j, w + j), (j, 2 * w + j), (2 * w + j,)])[0] for j in range(w)]


def f_maj(w):
    return [cancel([(j, w + j), (j, 2 * w + j), (w + j, 2 * w + j)])[0] for j in range(w)]


def f_chi(w):
    """x ^ (~y & z) = x + z + yz."""
    return [cancel([(j,), (2 * w + j,), (w + j, 2 * w + j)])[0] for j in range(w)]


def f_and_all(w, k):
    return [[tuple(o * w + j for o in range(k))] for j in range(w)]


def f_mux(w):
    """s ? x : y with a one-bit s (variable 0), x at 1 .. w, y at w + 1 .. 2w: s x + s y + y."""
    return [cancel([(0, 1 + j), (0, 1 + w + j), (1 + w + j,)])[0] for j in range(w)]


def f_linear(rows):
    """Rows of masks over the input planes."""
    return [[(i,) for i in range(256) if (row >> i) & 1] for row in rows]


def f_bilinear(form, wa):
    """tests/model_bilinear.py's form over a (variables 0 .. wa - 1) and b (wa ..)."""
    return [cancel([(i, wa + l) for i, l in pairs])[0] for pairs in form]


def f_xor(f, g):
    return [cancel(p + q)[0] for p, q in zip(f, g)]


def f_and(f, g, cf=0, cg=0):
    """The pointwise product of two forms with constants: (rows, constant)."""
    rows, const = [], 0
    for x, (p, q) in enumerate(zip(f, g)):
        p = list(p) + ([()] if (cf >> x) & 1 else [])
        q = list(q) + ([()] if (cg >> x) & 1 else [])
        kept, c = cancel([tuple(a) + tuple(b) for a in p for b in q])
        rows.append(kept)
        const |= c << x
    return rows, const


def f_after(rows, form):
    """The linear map `rows` (masks over the form's planes) after the form."""
    return [cancel([m for j in range(len(form)) if (row >> j) & 1 for m in form[j]])[0] for row in rows]


def f_compose(form, maps):
    """The form after linear maps of its variables: maps[v] is the list of new variables whose sum is old variable v."""
    out = []
    for monomials in form:
        expanded = []
        for mono in monomials:
            expanded += [tuple(c) for c in itertools.product(*[maps[v] for v in mono])]
        out.append(cancel(expanded)[0])
    return out


def random_form(n_in, n_out, per_plane, max_degree, seed):
    rng = np.random.default_rng(seed)
    return [[tuple(int(v) for v in rng.integers(0, n_in, int(rng.integers(1, max_degree + 1)))) for _ in range(per_plane)]
            for _ in range(n_out)]


# -- the kernel's grid, replayed from the launches' figures ------------------------------------------------------------
def replay_grid(terms, form, constant, batch, U, G, S, chunk, staged, stage_units, launch_blocks, order=None,
                lds_monomials=512):
    """Every position of every workgroup of every launch of k_uint_poly at U units a term, G elements a tile, S
    workgroups a tile and `chunk` units a workgroup, as csgn_uint_poly.hip places them: returns (count[x]: per-unit write
    counts of output plane x, launches, workgroups per tile, workgroups of the first launch) and asserts every source
    index in range -- of the operand planes, of the monomial records and, staged, of the LDS copy of stage_units units.
    Sources come from plane_table, not from the kernel's own search: the words are compared on the device; here it is
    the coverage.  order(b, nblocks), when given, is the launch's block order (xcd_contiguous_block)."""
    T = [poly_terms(terms, p, (constant >> x) & 1) for x, p in enumerate(form)]
    tables = [plane_table(terms, p, (constant >> x) & 1) for x, p in enumerate(form)]
    assert chunk % 256 == 0 and all(len(t[0]) == Tx for t, Tx in zip(tables, T))
    nmon = sum(len(p) for p in form)
    mfirst = np.concatenate([[0], np.cumsum([len(p) for p in form])])
    PU = sum(T) * U
    assert S * chunk >= G * PU
    tiles = -(-batch // G)
    per_launch = max(1, launch_blocks // S)
    tin = np.array(list(terms))
    opre = np.concatenate([[0], np.cumsum(tin)])                     # operand terms before plane i
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
                assert mfirst[x + 1] <= nmon and (nmon > lds_monomials or mfirst[x + 1] <= lds_monomials)
                P, I = (c[term] for c in tables[x])
                for j in range(MAX_DEGREE):
                    live = P[:, j] >= 0
                    if not live.any():
                        continue
                    plane, t = P[live, j], I[live, j]
                    tf = tin[plane]
                    assert plane.max() < len(terms) and (t < tf).all() and (e_base + e0 + el[live]).max() < batch
                    src = ((e_base + e0 + el[live]) * tf + t) * U + k[m][live]
                    assert (src < batch * tf * U).all()
                    if staged:
                        at = ge * opre[plane] * U + (el[live] * tf + t) * U + k[m][live]
                        assert at.max() < ge * int(opre[-1]) * U <= stage_units
                np.add.at(count[x], ((e_base + e0) * T[x] + off) * U + k[m], 1)
    return count, launches, S, first_blocks


# -- the shapes of tests/test_uint_poly_gpu.py, which tests/test_uint_poly_cpu.py replays on the host -------------------
NS = (64, 1247, 1300)                   # one 8-byte unit a term; 16-byte units (10 a term); 8-byte units (21 a term)
STAGE_BYTES = 16384                     # csgn_uint_poly.hip's kStageBytes, as csgn_uint_poly_launches reports it


def term_counts(w, ramp):
    return [1 + i for i in range(w)] if ramp else [1] * w            # (1, 2, 3, ...) or one term each


def small_form(n_in):
    """(form, constant): one monomial of each degree 1..4 and one of degree 8; every monomial of degree <= 3 over (up
    to) three planes; empty; empty with the constant; a monomial twice; a factor twice inside a monomial; unsorted
    factors and monomials; rows with the constant."""
    k = min(n_in, 3)
    top = n_in - 1
    deg = lambda d: tuple(j % n_in for j in range(d))                # noqa: E731
    eight = tuple(min(j // 3, top) for j in range(8))
    every = [m for d in (1, 2, 3) for m in itertools.product(range(k), repeat=d)]
    form = [[deg(1)], [deg(2)], [deg(3)], [deg(4)], [eight], every, [], [], [(top, 0), (0,), (top, 0)], [(top, top), (0, top, 0)],
            every[::-1][:5], [(top,), (0, top)], [(top, 0, top)]]
    return form, 0b1100010010000


def gpu_shapes():
    """(name, terms, form, constant, batches) at every n of NS: n_in in 1, 2, 3, 5 with one-term planes (nothing is
    divided) and ramps (the planes' divisors), mixed degrees (the search); then one term count and one degree (the one
    division), with one-term planes and with the shared divisor; then the shared divisor with mixed degrees."""
    shapes = []
    for n_in in (1, 2, 3, 5):
        form, constant = small_form(n_in)
        shapes.append(("%d-ones" % n_in, term_counts(n_in, False), form, constant, (1, 3, 257)))
        if n_in > 1:
            shapes.append(("%d-ramp" % n_in, term_counts(n_in, True), form, constant, (1, 3, 257)))
    pairs = [m for m in itertools.product(range(3), repeat=2)]
    shapes.append(("eq-deg2-t2", [2, 2, 2], [pairs, [(2, 1)], [], pairs[::-1][:4], [(0, 0), (0, 0)]], 0b10100, (1, 3, 257)))
    shapes.append(("eq-deg3-ones", [1] * 5, [[(0, 1, 2), (4, 3, 2)], [(4, 4, 4)], [], [(1, 2, 3)]], 0b0110, (1, 3, 257)))
    shapes.append(("eq-deg1-t3", [3, 3], [[(1,), (0,), (1,)], [(0,)]], 0b01, (1, 3, 257)))
    shapes.append(("mixed-t2", [2, 2, 2], small_form(3)[0], small_form(3)[1], (1, 3, 257)))
    return shapes


# monomial ends at terms 3, 18, 158, 228, 258 and 398 of an element at n = 64 (one unit a term): inside a wave and past one
BOUNDARIES = ("boundaries", [3, 70, 1, 5, 2], [[(0,), (0, 3), (1, 4), (1,), (0, 4, 3), (1, 2, 4)], [(3, 1), (0,)], []], 0b101,
              (1, 7, 40))

# (name, n, terms, form, constant, batches): every argument array full; 576 monomials (the records through the vector cache)
RANDOM256 = random_form(256, 64, 9, 3, 256)
FULL = [
    ("random256", 1247, [1] * 256, RANDOM256, 0x8000000000000001 | (0xF0 << 24), (2,)),
    ("random256", 64, [1] * 256, RANDOM256, 0x8000000000000001 | (0xF0 << 24), (33,)),
    ("ch32", 1247, [1] * 96, f_ch(32), 0, (2,)),
    ("ch32", 64, [1] * 96, f_ch(32), 1 << 31, (33,)),
    ("maj32", 1247, [1] * 96, f_maj(32), 0, (2,)),
    ("maj32", 64, [1] * 96, f_maj(32), 0, (33,)),
    ("chi64", 1247, [1] * 192, f_chi(64), 0, (2,)),
    ("chi64", 64, [1] * 192, f_chi(64), 1 << 63, (33,)),
    ("deg8-t2", 1247, [2] * 8, [[tuple(range(8))]], 0, (2,)),
    ("deg8-t2", 64, [2] * 8, [[tuple(range(8))], [tuple(range(7, -1, -1))]], 0b10, (33,)),
]

# at n = 1247 a term is 160 bytes: FIT operand terms are the most that the LDS budget holds
FIT = STAGE_BYTES // 160
BUDGET_FORM = [[(0, 2)], [(1, 3), (0, 3)], [(1, 2)]]
STAGED_EDGE = ("at-the-budget", [35, 20, 30, FIT - 85], BUDGET_FORM, 0b010, (2,))
PAST_EDGE = ("one-term-past", [35, 20, 30, FIT - 84], BUDGET_FORM, 0b010, (2,))
UNSTAGED = ("far-past-the-budget", [70, 40, 60, 45], BUDGET_FORM, 0b010, (2,))

# tests/test_uint_poly_gpu.py's aliased inputs: (terms, same, form, constant) at every n of NS, batch 5; input plane i is
# the device pointer of plane same[i].  Several planes the same pointer; every operand the same integer (ch, maj of x, x, x)
ALIASED = [([2, 2, 1, 2], [0, 0, 2, 0], [[(0, 1)], [(3, 2, 1), (0,)], [(1, 3, 0)], []], 0b1010),
           ([1] * 12, [i % 4 for i in range(12)], f_ch(4), 0b0001),
           ([3] * 9, [i % 3 for i in range(9)], f_maj(3), 0)]
ALIASED_BATCH = 5
# its block-order test at several tiles: (full shape, batch): staged with six elements a tile; unstaged with 45
XCD_FULL = [(FULL[8], 29), (FULL[0], 100)]
# its tiles-and-launches test: (n, index into gpu_shapes()): more than 5 elements a tile and more than 1 workgroup a tile
TILE_SHAPES = [(64, 6), (1247, 6), (1300, 6)]
