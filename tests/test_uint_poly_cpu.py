"""A public polynomial over F2 of encrypted planes (csgn_uint_poly*), on a box without a GPU: the model
(tests/model_poly.py) against the oracle's and, where built, the reference's own operator* and operator+;
csgn_uint_poly_terms and csgn_uint_poly_decode against the model term for term; csgn_uint_poly_launches' figures
replayed on the host for every shape of tests/test_uint_poly_gpu.py; the argument checks and their order; the size
guards; decryptions through the oracle; the builders restated.  The device side is tests/test_uint_poly_gpu.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle.binding import glibc_draws, load_ref
from tests.model import (LIMIT, const_term, decrypt_value, encrypt_planes, lib, np_anf, oracle_ops, rand_terms,  # noqa: F401
                         ref_ops, u64s)
from tests.model_bilinear import f_clmul, f_gf_mul, np_bilinear
from tests.model_linear import low
from tests.model_poly import (ALIASED, ALIASED_BATCH, BOUNDARIES, FIT, FULL, MAX_DEGREE, MAX_MONOMIALS, NS, ONE, PAST_EDGE,
                              STAGE_BYTES, STAGED_EDGE, TILE_SHAPES, UNSTAGED, XCD_FULL, ZERO, cancel, clear_poly, compose_poly,
                              f_after, f_and, f_and_all, f_bilinear, f_ch, f_chi, f_compose, f_linear, f_maj, f_mux, f_xor,
                              gpu_shapes, np_poly, pack_operands, poly_decode, poly_terms, random_form, replay_grid,
                              symbolic_poly)

TILE_UNITS = 262144                     # csgn_uint_poly.hip's kTileUnits
MIN_CHUNK, STAGE_RATIO, STAGE_MIN_RATIO = 2048, 4, 2
MAX_BLOCKS = ((1 << 32) - 1) // 256


def flat(form):
    """(h_first, h_mfirst, h_factor) of a form."""
    first, mfirst, factor = [0], [0], []
    for monomials in form:
        first.append(first[-1] + len(monomials))
        for mono in monomials:
            mfirst.append(mfirst[-1] + len(mono))
            factor += list(mono)
    return u64s(first), u64s(mfirst), u64s(factor or [0])


def c_terms(lib, terms, monomials, cbit, n_in=None):
    _, mfirst, factor = flat([monomials])
    return int(lib.csgn_uint_poly_terms(len(terms) if n_in is None else n_in, u64s(terms), len(monomials), mfirst, factor, cbit))


def c_decode(lib, terms, monomials, cbit, q):
    _, mfirst, factor = flat([monomials])
    mono, idx = C.c_uint64(77), (C.c_uint64 * 8)(*([77] * 8))
    if not lib.csgn_uint_poly_decode(len(terms), u64s(terms), len(monomials), mfirst, factor, cbit, q, C.byref(mono), idx):
        assert mono.value == 77 and list(idx) == [77] * 8
        return None
    m = mono.value
    return (ONE if m == len(monomials) else ZERO if m == len(monomials) + 1 else m), tuple(int(i) for i in idx)


def c_launches(lib, n, batch, terms, form, constant):
    plan = (C.c_uint64 * 14)()
    first, mfirst, factor = flat(form)
    rc = lib.csgn_uint_poly_launches(n, batch, len(terms), u64s(terms), len(form), first, mfirst, factor, constant, plan)
    assert rc == 0, lib.csgn_last_error()
    return [int(x) for x in plan]


# -- the definition against the genuine reference and the oracle -------------------------------------------------------
def monomial_lists(n_in, max_degree):
    """Every list of up to two monomials of degree <= max_degree, repeated factors and unsorted order included."""
    every = [m for d in range(1, max_degree + 1) for m in itertools.product(range(n_in), repeat=d)]
    return [list(p) for k in range(3) for p in itertools.product(every, repeat=k)]


@pytest.mark.parametrize("n,d", [(65, 4), (1247, 16)])
@pytest.mark.parametrize("n_in,max_degree", [(1, 3), (2, 3), (3, 2), (3, 3)])
def test_definition_matches_reference_and_oracle(oracle, n, d, n_in, max_degree):
    """Every list of up to two monomials of degree <= 3 over up to three planes of (1, 2, 3) terms, with and without the
    constant, and one monomial of degree 8, through the oracle's operator* and operator+ and, where the reference is
    built, through its own: the words of the numpy composition."""
    ref = load_ref()
    terms = [1, 2, 3][:n_in]
    planes = [rand_terms(n, 1, t, 40 * n_in + i) for i, t in enumerate(terms)]
    fl = [p[0].ravel() for p in planes]
    dl = (n + 63) // 64
    routes = [oracle_ops(oracle, n)] + ([ref_ops(ref, n, d)] if ref is not None else [])
    lists = monomial_lists(n_in, max_degree)[::1 if n_in < 3 else 5] + [[tuple(j % n_in for j in range(8))]]
    for g0 in range(0, len(lists), 64):
        form = lists[g0:g0 + 64]
        for constant in (0, low(len(form))):
            want = np_poly(n, planes, form, constant)
            for add, mul in routes:
                got = compose_poly(fl, form, constant, add, mul, const_term(n, 1), const_term(n, 0))
                for x, monomials in enumerate(form):
                    assert np.array_equal(got[x], want[x].ravel()), (monomials, constant)
                    assert got[x].size == poly_terms(terms, monomials, (constant >> x) & 1) * dl


# -- the C ABI, host side ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms,degrees", [([1], (1, 2, 3)), ([1, 1, 1], (1, 2, 3)), ([1, 1, 1], (3,)), ([2, 2], (2,)),
                                           ([3, 3, 3], (1, 2)), ([1, 2, 3], (1, 2, 3)), ([3, 70, 1, 5, 2], (1, 2)),
                                           ([2, 2], (8,)), ([2, 1, 3], (4, 8))])
def test_terms_and_decode_give_the_table(lib, terms, degrees):
    """One count and one degree (the one division), one-term planes (no division), equal counts with mixed degrees (the
    shared divisor under the search) and unequal counts (the planes' divisors): every term of short monomial lists
    against the symbolic composition and the model's decode."""
    n_in = len(terms)
    rng = np.random.default_rng(n_in + 7 * len(degrees))
    forms = [[]] + [[tuple(int(v) for v in rng.integers(0, n_in, int(rng.choice(degrees)))) for _ in range(k)]
                    for k in (1, 1, 2, 3, 5, 9)]
    for cbit in (0, 1):
        for monomials in forms:
            T = poly_terms(terms, monomials, cbit)
            assert c_terms(lib, terms, monomials, cbit) == T > 0, (monomials, cbit)
            if T > 20000:
                continue
            want = symbolic_poly(terms, [monomials], cbit)[0]
            assert len(want) == T
            for q in range(T):
                got = c_decode(lib, terms, monomials, cbit, q)
                assert got == poly_decode(terms, monomials, cbit, q), (monomials, cbit, q)
                label = (got[0],) if got[0] in (ONE, ZERO) else tuple((f, got[1][j]) for j, f in enumerate(monomials[got[0]]))
                assert label == want[q], (monomials, cbit, q)
            assert c_decode(lib, terms, monomials, cbit, T) is None


def test_terms_by_hand_and_refusals(lib):
    ones = [1] * 96
    assert c_terms(lib, ones, f_ch(32)[5], 0) == 3 and c_terms(lib, ones, f_maj(32)[0], 1) == 4
    assert c_terms(lib, [1] * 192, f_chi(64)[63], 0) == 3
    assert c_terms(lib, [2] * 8, [tuple(range(8))], 0) == 256                  # a degree-8 monomial of 2-term planes
    assert c_terms(lib, [4, 5, 6], [(0, 1), (2,), (0, 0), (2, 1, 0)], 1) == 20 + 6 + 16 + 120 + 1
    assert c_terms(lib, [4, 5], [], 0) == 1 and c_terms(lib, [4, 5], [], 1) == 1
    z8 = (0,) * 8
    assert c_decode(lib, [4, 5], [], 0, 0) == (ZERO, z8) and c_decode(lib, [4, 5], [], 1, 0) == (ONE, z8)
    assert c_decode(lib, [4, 5, 6], [(0, 1), (2, 1, 0)], 1, 19) == (0, (3, 4) + (0,) * 6)
    assert c_decode(lib, [4, 5, 6], [(0, 1), (2, 1, 0)], 1, 20 + 4 * 5 + 4 + 1) == (1, (1, 1, 1) + (0,) * 5)
    assert c_decode(lib, [4, 5, 6], [(0, 1), (2, 1, 0)], 1, 140) == (ONE, z8)
    assert c_decode(lib, [3, 3], [(1, 0), (0, 1), (1, 1)], 0, 9 + 9 + 7) == (2, (2, 1) + (0,) * 6)   # the division
    # refused: n_in, a null pointer, a zero count, a degree, an index at n_in, the constant bit
    assert c_terms(lib, [1] * 257, [], 0) == 0 and c_terms(lib, [1], [], 0, n_in=0) == 0
    assert c_terms(lib, [1] * 256, [(255,)], 0) == 1
    assert int(lib.csgn_uint_poly_terms(1, None, 0, None, None, 0)) == 0
    assert int(lib.csgn_uint_poly_terms(1, u64s([1]), 1, None, u64s([0]), 0)) == 0
    assert int(lib.csgn_uint_poly_terms(1, u64s([1]), 1, u64s([0, 1]), None, 0)) == 0
    assert int(lib.csgn_uint_poly_terms(1, u64s([1]), 0, None, None, 1)) == 1
    assert c_terms(lib, [1, 0], [(0,)], 0) == 0
    assert int(lib.csgn_uint_poly_terms(1, u64s([1]), 1, u64s([0, 0]), u64s([0]), 0)) == 0          # degree 0
    assert int(lib.csgn_uint_poly_terms(1, u64s([1]), 1, u64s([1, 0]), u64s([0]), 0)) == 0          # descending
    assert c_terms(lib, [1], [(0,) * 9], 0) == 0 and c_terms(lib, [1], [(0,) * 8], 0) == 1
    assert c_terms(lib, [1, 1], [(2,)], 0) == 0 and c_terms(lib, [1, 1], [(0, 2)], 0) == 0
    assert c_terms(lib, [1], [(0,)], 2) == 0
    # a plane of a plan's arrays: h_mfirst + h_first[x] with the plan's h_factor
    first, mfirst, factor = flat([[(0, 1)], [(1,), (1, 1, 0)]])
    shifted = C.cast(C.byref(mfirst, 8), C.POINTER(C.c_uint64))
    assert int(lib.csgn_uint_poly_terms(2, u64s([2, 3]), 2, shifted, factor, 0)) == 3 + 18
    # 2^62, without wrap-around
    big = LIMIT - 1
    assert c_terms(lib, [big], [(0,)], 0) == big and c_terms(lib, [big], [(0,)], 1) == 0
    assert c_terms(lib, [LIMIT], [], 0) == 0 and c_terms(lib, [1 << 31], [(0, 0)], 0) == 0
    assert c_terms(lib, [1 << 32], [(0, 0)], 0) == 0 and c_terms(lib, [1 << 8], [(0,) * 8], 0) == 0
    assert c_terms(lib, [1 << 30], [(0, 0)] * 3, 0) == 3 << 60 and c_terms(lib, [1 << 30], [(0, 0)] * 4, 0) == 0
    assert c_terms(lib, [1 << 30], [(0, 0)] * 3, 1) == (3 << 60) + 1
    assert c_terms(lib, [1 << 20], [(0, 0, 0)], 0) == 1 << 60 and c_terms(lib, [1 << 21], [(0, 0, 0)], 0) == 0
    _, mfirst, factor = flat([[(0,)]])
    assert lib.csgn_uint_poly_decode(1, u64s([1]), 1, mfirst, factor, 0, 0, None, None) == 0
    assert c_decode(lib, [1 << 16, 1 << 15], [(0, 1)], 0, 5) is None                           # a plane of 2^31 terms


# -- the launches, replayed ----------------------------------------------------------------------------------------------
def units_of(n, wide):
    dl = (n + 63) // 64
    return dl // 2 if wide and dl % 2 == 0 else dl


def cut_of(n, terms, T, batch, wide):
    """(U, units, operand units, staged, G, S, chunk) by the rules include/csgn_hip.h states."""
    U = units_of(n, wide)
    ub = 16 if wide and ((n + 63) // 64) % 2 == 0 else 8
    units, op = sum(T) * U, sum(terms) * U
    staged = op * ub <= STAGE_BYTES and units >= STAGE_MIN_RATIO * op
    G = STAGE_BYTES // (op * ub) if staged else max(1, TILE_UNITS // units)
    G = min(G, batch, max(1, (1 << 31) // units))
    least = max(MIN_CHUNK, STAGE_RATIO * G * op) if staged else MIN_CHUNK
    S = max(1, G * units // least)
    chunk = -(-(-(-G * units // S)) // 256) * 256
    return U, units, op, staged, G, S, chunk


def modes_of(terms, form):
    """(the monomial by division, the factor terms' mode) as include/csgn_hip.h states them."""
    same = len(set(terms)) == 1 and terms[0] < 1 << 31
    degrees = {len(m) for monomials in form for m in monomials}
    eq = same and len(degrees) == 1 and terms[0] ** next(iter(degrees)) < 1 << 31
    return int(eq), (0 if terms[0] == 1 else 1) if same else 2


def check_launches(lib, knobs, n, terms, form, constant, batch, cap=0, xcd=False):
    """The figures against their definition, then every position of every workgroup of every launch placed as the
    kernel places it: every unit of every output plane exactly once, every source in range."""
    knobs.set("launch_blocks", cap)
    plan = c_launches(lib, n, batch, terms, form, constant)
    T = [poly_terms(terms, p, (constant >> x) & 1) for x, p in enumerate(form)]
    dl = (n + 63) // 64
    U, units, op, staged, G, S, chunk = cut_of(n, terms, T, batch, True)
    assert plan[0] == (16 if dl % 2 == 0 else 8) and plan[7] == 1 and plan[11] == STAGE_BYTES
    assert (plan[1], plan[2], plan[3], plan[4], plan[8], plan[9], plan[10]) == (units, G, -(-batch // G), S, int(staged), chunk, op)
    assert tuple(plan[12:14]) == modes_of(terms, form)
    count, launches, per, first = replay_grid(terms, form, constant, batch, U, G, S, chunk, staged, STAGE_BYTES // plan[0],
                                              cap if cap else MAX_BLOCKS)
    assert (plan[4], plan[5], plan[6]) == (per, launches, first)
    for x, c in enumerate(count):
        assert c.size == batch * T[x] * U and (c == 1).all(), (n, terms, form[x], batch, cap, x)
    if xcd:                                                          # the same launches in the XCD-contiguous block order
        order = lambda b, nb: lib.csgn_debug_block_order(b, nb, 0)   # noqa: E731
        for c in replay_grid(terms, form, constant, batch, U, G, S, chunk, staged, STAGE_BYTES // plan[0],
                             cap if cap else MAX_BLOCKS, order)[0]:
            assert (c == 1).all()
    if plan[0] == 16:                                                # the same shape with a pointer off alignment
        U8, _, _, staged8, G8, S8, chunk8 = cut_of(n, terms, T, batch, False)
        for c in replay_grid(terms, form, constant, batch, U8, G8, S8, chunk8, staged8, STAGE_BYTES // 8, MAX_BLOCKS)[0]:
            assert (c == 1).all()
    return plan


@pytest.mark.parametrize("n", NS)
def test_launches_cover_every_unit_once(lib, knobs, n):
    for name, terms, form, constant, batches in gpu_shapes() + [BOUNDARIES]:
        for batch in batches:
            check_launches(lib, knobs, n, terms, form, constant, batch, xcd=n == 1247 and batch < 257)
    for terms, same, form, constant in ALIASED:
        check_launches(lib, knobs, n, terms, form, constant, ALIASED_BATCH)


def test_the_shapes_take_every_decode_path(lib):
    """The GPU shapes between them take the one division, the search with the records in LDS and through the cache, no
    division of the factor terms, the shared divisor and the planes' divisors."""
    seen = set()
    for name, terms, form, constant, batches in gpu_shapes() + [BOUNDARIES]:
        seen.add(tuple(c_launches(lib, 1247, batches[0], terms, form, constant)[12:14]))
    assert seen == {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)}
    assert sum(len(p) for p in FULL[0][3]) > 512 >= sum(len(p) for p in gpu_shapes()[6][2])


def test_launches_of_the_full_shapes_the_budget_and_the_splits(lib, knobs):
    several = set()
    for name, n, terms, form, constant, batches in FULL:
        for batch in batches:
            if check_launches(lib, knobs, n, terms, form, constant, batch)[4] > 1:
                several.add((name, n))
    assert ("random256", 1247) in several                            # several workgroups a tile
    # the LDS budget: FIT operand terms of 160 bytes fit, FIT + 1 do not, 215 are far past it
    for (name, terms, form, constant, batches), staged in ((UNSTAGED, 0), (STAGED_EDGE, 1), (PAST_EDGE, 0)):
        plan = check_launches(lib, knobs, 1247, terms, form, constant, batches[0])
        assert plan[8] == staged and (sum(terms) * 160 <= STAGE_BYTES) == bool(staged), name
    assert sum(STAGED_EDGE[1]) == FIT == sum(PAST_EDGE[1]) - 1 and (FIT + 1) * 160 > STAGE_BYTES >= FIT * 160
    # a form that writes less than twice what it reads is not staged: ch over fresh planes writes what it reads
    assert check_launches(lib, knobs, 1247, [1] * 24, f_ch(8), 0, 40)[8] == 0
    assert check_launches(lib, knobs, 1247, [4] * 24, f_ch(8), 0, 3)[8] == 1          # ch(8) on 4-term planes is
    for (name, n, terms, form, constant, _), batch in XCD_FULL:      # several tiles in the XCD order, whole and split
        plan = check_launches(lib, knobs, n, terms, form, constant, batch, xcd=True)
        assert plan[3] > 2
        assert check_launches(lib, knobs, n, terms, form, constant, batch, 2 * plan[4], xcd=True)[5] > 1
    for n, (name, terms, form, constant, _) in ((n, gpu_shapes()[i]) for n, i in TILE_SHAPES):
        G = c_launches(lib, n, 1 << 30, terms, form, constant)[2]
        assert G > 5
        plan = check_launches(lib, knobs, n, terms, form, constant, 2 * G + 5)
        assert plan[2:4] == [G, 3] and plan[5] == 1
        per = plan[4]
        assert per > 1                                               # so that per - 1 is a cap below a tile's workgroups
        for cap, launches in ((per, 3), (2 * per, 2), (per - 1, 3), (3 * per, 1)):
            assert check_launches(lib, knobs, n, terms, form, constant, 2 * G + 5, cap)[5] == launches, (name, cap)
    assert c_launches(lib, 1247, 0, [1], [[(0,)]], 0)[3:7] == [0, 1, 0, 0]


def test_plane_groups_of_a_tile_past_2_31_units(lib, knobs):
    """Eight planes of 2^26 terms at n = 1247 (10 units a term): one element of all planes passes 2^31 units, so G = 1
    and the planes go in runs of three, three and two, each a stream and a launch sequence of its own.  Host only."""
    terms, form = [1 << 13, 1 << 13], [[(0, 1)]] * 8
    units = (1 << 26) * 10
    S = [3 * units // MIN_CHUNK, 3 * units // MIN_CHUNK, 2 * units // MIN_CHUNK]
    assert 3 * units <= 1 << 31 < 4 * units
    for cap, batch, launches in ((0, 2, 3), (0, 40, 8), (1000, 2, 6)):       # 17, 17 and 25 tiles a launch; one under the cap
        knobs.set("launch_blocks", cap)
        plan = c_launches(lib, 1247, batch, terms, form, 0)
        assert plan[:5] == [16, 8 * units, 1, batch, sum(S)] and plan[7:9] == [3, 0], plan
        per_launch = [max(1, (cap or MAX_BLOCKS) // s) for s in S]
        assert plan[5] == launches == sum(-(-batch // t) for t in per_launch) and plan[6] == min(batch, per_launch[0]) * S[0]
        chunk = -(-(-(-3 * units // S[0])) // 256) * 256
        assert plan[9] == chunk and S[0] * chunk >= 3 * units and (S[0] - 1) * chunk < 3 * units
    # a single plane is always one group: its units stay below 2^31 by the size check
    assert c_launches(lib, 1247, 1, terms, [[(0, 1)]], 0)[7] == 1


# -- the argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails.  csgn_uint_poly_create: the plan pointer, n_in, n_out and the
    constant, the host arrays, h_first, the monomial arrays (INVALID), 262144 monomials (UNSUPPORTED), term counts,
    h_mfirst[0], degrees, factors and overflow (INVALID), a plane of 2^31 terms (UNSUPPORTED), and only then the device
    (NO_DEVICE on a box without one).  csgn_uint_poly_launches adds n_bits in front and h_plan and the sizes behind;
    csgn_uint_poly checks n_bits, the host arrays and the plan."""
    import torch
    gpu = torch.cuda.is_available()
    one = u64s([1] * 256)
    first3, mfirst3, factor3 = flat([[(0, 1), (7, 7, 2)], [], [(3,)]])
    handle = C.c_void_p(5)

    def create(n_in=8, terms=one, m=3, first=first3, mfirst=mfirst3, factor=factor3, constant=0b110, plan=C.byref(handle)):
        return lib.csgn_uint_poly_create(n_in, terms, m, first, mfirst, factor, constant, plan)

    def launches(n=1247, batch=4, n_in=8, terms=one, m=3, first=first3, mfirst=mfirst3, factor=factor3, constant=0b110,
                 plan=(C.c_uint64 * 14)()):
        return lib.csgn_uint_poly_launches(n, batch, n_in, terms, m, first, mfirst, factor, constant, plan)

    assert create(plan=None, n_in=0) == -1 and b"plan is null" in lib.csgn_last_error()
    assert create(n_in=0, m=0) == -1 and create(n_in=257, m=0) == -1 and b"n_in" in lib.csgn_last_error()
    assert create(m=0, terms=None) == -1 and create(m=65, terms=None) == -1
    assert create(constant=0b1000, terms=None) == -1 and b"does not fit" in lib.csgn_last_error()
    for arg in ("terms", "first"):                                   # host arrays, before what they hold
        assert create(**{arg: None, "factor": u64s([9] * 6)}) == -1 and b"null host pointer" in lib.csgn_last_error(), arg
    assert create(first=u64s([1, 2, 2, 3]), mfirst=None) == -1 and b"h_first[0]" in lib.csgn_last_error()
    assert create(first=u64s([0, 2, 1, 3]), mfirst=None) == -1 and b"descends" in lib.csgn_last_error()
    for arg in ("mfirst", "factor"):
        assert create(**{arg: None, "first": u64s([0, 2, 2, MAX_MONOMIALS + 1])}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    assert create(first=u64s([0, 0, 0, 0]), mfirst=None, factor=None) in (0, -3)       # no monomial: no monomial arrays
    if gpu:
        lib.csgn_uint_poly_destroy(handle)
    assert create(first=u64s([0, 2, 2, MAX_MONOMIALS + 1]), terms=u64s([0] * 8)) == -2 and b"monomials" in lib.csgn_last_error()
    assert create(terms=u64s([1, 0] + [1] * 6), mfirst=u64s([1, 2, 3, 4])) == -1 and b"input plane 1" in lib.csgn_last_error()
    assert create(terms=u64s([1 << 62] * 8), factor=u64s([9] * 6)) == -1 and b"input plane 0" in lib.csgn_last_error()
    assert create(mfirst=u64s([1, 2, 5, 6]), factor=u64s([9] * 6)) == -1 and b"h_mfirst[0]" in lib.csgn_last_error()
    assert create(mfirst=u64s([0, 2, 2, 3]), factor=u64s([0, 1, 9])) == -1 and b"monomial 1 has a degree" in lib.csgn_last_error()
    assert create(mfirst=u64s([0, 9, 10, 11]), factor=u64s([0] * 8 + [9] * 3)) == -1 and b"monomial 0 has a degree" in lib.csgn_last_error()
    assert create(mfirst=u64s([0, 8, 9, 10]), factor=u64s([0] * 10)) in (0, -3)                 # degree 8 is the most
    if gpu:
        lib.csgn_uint_poly_destroy(handle)
    assert create(factor=u64s([0, 1, 7, 8, 2, 3]), terms=u64s([1 << 61] * 8)) == -1 and b"monomial 1 names plane 8" in lib.csgn_last_error()
    assert create(n_in=7) == -1 and b"monomial 1 names plane 7" in lib.csgn_last_error()
    assert create(terms=u64s([1 << 31] * 8)) == -1 and b"overflows" in lib.csgn_last_error()   # 2^62 in monomial 0
    assert create(terms=u64s([1 << 30] * 8), first=u64s([0, 3, 3, 3])) == -1                    # 2^60 + 2^90
    assert create(terms=u64s([1 << 16] * 8)) == -2 and b"2^31" in lib.csgn_last_error()
    assert handle.value is None                                      # every refusal leaves the handle null
    # the launches: n_bits first, then create's checks, then h_plan, then the sizes
    assert launches(n=0, n_in=0) == -1 and launches(n=131073, n_in=0) == -2
    assert launches(n_in=0, plan=None) == -1 and b"n_in" in lib.csgn_last_error()
    assert launches(terms=u64s([1 << 16] * 8), plan=None) == -2
    assert launches(plan=None, batch=1 << 58) == -1 and b"null host pointer" in lib.csgn_last_error()
    assert launches(terms=u64s([1, 1, 1, 1, 1 << 27, 1, 1, 1])) == -2 and b"input plane 4" in lib.csgn_last_error()
    assert launches(terms=u64s([1 << 14] * 8), first=u64s([0, 1, 1, 1])) == -2 and b"output 0" in lib.csgn_last_error()
    assert launches(batch=1 << 56) == -2 and b"batch" in lib.csgn_last_error()
    assert launches() == 0 and launches(batch=0) == 0
    # the call: n_bits, the host arrays, the plan
    buf = np.zeros(64, dtype=np.uint64)
    ptrs = (C.c_void_p * 256)(*([buf.ctypes.data] * 256))
    assert lib.csgn_uint_poly(None, 0, 1, None, None, None) == -1
    assert lib.csgn_uint_poly(None, 131073, 1, ptrs, ptrs, None) == -2
    for a, out in ((None, ptrs), (ptrs, None)):
        assert lib.csgn_uint_poly(None, 1247, 1, a, out, None) == -1 and b"null host pointer" in lib.csgn_last_error()
    assert lib.csgn_uint_poly(None, 1247, 1, ptrs, ptrs, None) == (-1 if gpu else -3)
    assert int(lib.csgn_uint_poly_plan_terms(None, 0)) == 0
    lib.csgn_uint_poly_destroy(None)
    if gpu:
        return
    assert create() == -3 and b"no CPU fallback" in lib.csgn_last_error() and handle.value is None
    assert lib.csgn_uint_poly(None, 1247, 0, ptrs, ptrs, None) == -3


# -- clear values and decryptions --------------------------------------------------------------------------------------
def test_builders_restated():
    """ch, maj, chi, andAll and mux against their boolean definitions; linear and bilinear forms against the clear
    values of tests/model_bilinear.py's; the ANF of a 4-bit S-box; the host algebra."""
    rng = np.random.default_rng(39)
    for w in (1, 2, 3, 8, 32, 64):
        m = low(w)
        for _ in range(20):
            x, y, z = (int(v) & m for v in rng.integers(0, 2**64, 3, dtype=np.uint64))
            bits = pack_operands([x, y, z], [w] * 3)
            assert clear_poly(f_ch(w), 0, bits) == (x & y) ^ (~x & z & m)
            assert clear_poly(f_maj(w), 0, bits) == (x & y) | (x & z) | (y & z)
            assert clear_poly(f_chi(w), 0, bits) == x ^ (~y & z & m)
            assert clear_poly(f_and_all(w, 3), 0, bits) == x & y & z
            s = int(rng.integers(0, 2))
            assert clear_poly(f_mux(w), 0, pack_operands([s, x, y], [1, w, w])) == (x if s else y)
        assert all(len(p) == 3 for f in (f_ch(w), f_maj(w), f_chi(w)) for p in f)
        assert all(p == cancel(p)[0] for f in (f_ch(w), f_maj(w), f_chi(w), f_mux(w), f_and_all(w, 3)) for p in f)
    # a & b & ~c = ab + abc, by the pointwise product with a constant on one side
    w = 4
    ab = f_and_all(w, 2)
    notc = [[(2 * w + j,)] for j in range(w)]
    form, const = f_and(ab, notc, 0, low(w))
    assert const == 0 and form[1] == [(1, w + 1), (1, w + 1, 2 * w + 1)]
    for bits in range(1 << 12):
        a, b, c = bits & 15, (bits >> 4) & 15, bits >> 8
        assert clear_poly(form, const, bits) == a & b & ~c & 15
    # maj = ab ^ ac ^ bc: xor of products; xor with itself is empty
    pair = lambda o, p: [[(o * w + j, p * w + j)] for j in range(w)]  # noqa: E731
    assert f_xor(f_xor(pair(0, 1), pair(0, 2)), pair(1, 2)) == f_maj(w) and f_xor(f_maj(w), f_maj(w)) == [[]] * w
    # a bilinear form as a polynomial; the parity of ch as a linear map after it; a rotation of one operand by compose
    gf = f_gf_mul(4, 0x13)
    for bits in range(256):
        want = 0
        for j, pairs in enumerate(gf):
            want |= (sum((bits >> i) & (bits >> (4 + l)) & 1 for i, l in pairs) & 1) << j
        assert clear_poly(f_bilinear(gf, 4), 0, bits) == want
    parity = f_after([low(w)], f_ch(w))
    assert all(clear_poly(parity, 0, b) == bin(clear_poly(f_ch(w), 0, b)).count("1") & 1 for b in range(0, 1 << 12, 7))
    rot = [[(v // w) * w + (v % w + 1) % w] if v < w else [v] for v in range(3 * w)]     # e rotated by one
    rch = f_compose(f_ch(w), rot)
    for b in range(0, 1 << 12, 5):
        e = b & 15
        assert clear_poly(rch, 0, b) == clear_poly(f_ch(w), 0, (b & ~15) | ((e >> 1) | (e << 3)) & 15)
    # the ANF of a 4-bit S-box equals the table on all inputs
    table = [0xC, 5, 6, 0xB, 9, 0, 0xA, 0xD, 3, 0xE, 0xF, 8, 4, 7, 1, 2]                 # PRESENT
    anf = np_anf(table, 4)
    form = [[tuple(i for i in range(4) if (s >> i) & 1) for s in range(1, 16) if (int(anf[s]) >> j) & 1] for j in range(4)]
    const = int(anf[0])
    assert [clear_poly(form, const, x) for x in range(16)] == table


def test_linear_and_bilinear_forms_have_the_shipped_words():
    """The words of the polynomial of a linear map are csgn_uint_linear's (the concatenation of the row's planes in
    ascending order), of a bilinear form csgn_uint_bilinear's."""
    n, batch = 1247, 3
    ta, tb = [1, 2, 3], [2, 1]
    a = [rand_terms(n, batch, t, 70 + i) for i, t in enumerate(ta)]
    b = [rand_terms(n, batch, t, 80 + i) for i, t in enumerate(tb)]
    form = [[(0, 0), (2, 1)], [], [(1, 1), (1, 0), (0, 1)]]
    got = np_poly(n, a + b, [[(i, 3 + l) for i, l in pairs] for pairs in form], 0b101)
    want = np_bilinear(n, a, b, form, 0b101)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    rows = [0b101, 0b010, 0, 0b111]
    got = np_poly(n, a, f_linear(rows), 0b1000)
    one = np.broadcast_to(const_term(n, 1), (batch, 1, (n + 63) // 64))
    assert np.array_equal(got[0], np.concatenate([a[0], a[2]], axis=1)) and np.array_equal(got[1], a[1])
    assert np.array_equal(got[3], np.concatenate([a[0], a[1], a[2], one], axis=1)) and not got[2].any()


@pytest.mark.parametrize("w", [1, 2, 3])
def test_decrypts(oracle, w):
    """Through the oracle's encrypt and decrypt at N = 127: the model's planes decrypt to the form's clear value for
    every triple of w-bit values; ch, maj, chi, a 3-way AND and random forms of degree <= 4 with repeated monomials and a
    constant."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(1410 + w, 64 * d + 64))
    vals = np.arange(1 << (3 * w), dtype=np.uint64)
    planes = encrypt_planes(oracle, n, key, vals, 3 * w, 1420 + w)
    forms = [(f_ch(w), 0), (f_maj(w), low(w)), (f_chi(w), 1), (f_and_all(w, 3), 0), (f_clmul_poly(w), 0),
             (random_form(3 * w, 5, 4, 4, w), 0b10010), (random_form(3 * w, 9, 3, 4, 3 * w) + [[]], 1 << 9)]
    for form, constant in forms:
        outs = np_poly(n, planes, form, constant)
        want = np.array([clear_poly(form, constant, int(v)) for v in vals], dtype=np.uint64)
        assert np.array_equal(decrypt_value(oracle, n, key, outs), want), (form, constant)


def f_clmul_poly(w):
    return f_bilinear(f_clmul(w), w)
