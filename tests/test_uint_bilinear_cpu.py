"""A public bilinear form over F2 of two encrypted integers (csgn_uint_bilinear*), on a box without a GPU: the model
(tests/model_bilinear.py) against the oracle's and, where built, the reference's own operator* and operator+;
csgn_uint_bilinear_terms and csgn_uint_bilinear_decode against the model term for term; csgn_uint_bilinear_launches'
figures replayed on the host for every shape of tests/test_uint_bilinear_gpu.py; the argument checks and their order;
the size guards; decryptions through the oracle; F2Bilinear's builders restated.  The device side is
tests/test_uint_bilinear_gpu.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle.binding import glibc_draws, load_ref
from tests.model import (LIMIT, const_term, decrypt_value, encrypt_planes, lib, oracle_ops, rand_terms, ref_ops,  # noqa: F401
                         u64s)
from tests.model_bilinear import (ALIASED, ALIASED_BATCH, BOUNDARIES, DENSE, MAX_ENTRIES, NS, ONE, PAST_EDGE, STAGED_EDGE,
                                  TILE_SHAPES, UNSTAGED, XCD_DENSE, ZERO,
                                  bilinear_decode, bilinear_terms, cancel, clear_bilinear, compose_bilinear, f_after,
                                  f_bitwise_and, f_clmul, f_clmul_wide, f_compose, f_dot_bits, f_gf_mul, f_xor, gpu_shapes,
                                  np_bilinear, random_form, reduction_rows, replay_grid, symbolic_bilinear)
from tests.model_linear import clmul, gf_mul, low, m_gf_mul, m_identity

STAGE_BYTES = 16384                     # csgn_uint_bilinear.hip's kStageBytes, as csgn_uint_bilinear_launches reports it
TILE_UNITS = 262144                     # its kTileUnits
MIN_CHUNK, STAGE_RATIO, STAGE_MIN_RATIO = 2048, 4, 2
MAX_BLOCKS = ((1 << 32) - 1) // 256


def flat(form):
    first = [0]
    for pairs in form:
        first.append(first[-1] + len(pairs))
    every = [p for pairs in form for p in pairs]
    return u64s(first), u64s([i for i, _ in every] or [0]), u64s([l for _, l in every] or [0])


def c_terms(lib, ta, tb, pairs, cbit, wa=None, wb=None):
    return int(lib.csgn_uint_bilinear_terms(len(ta) if wa is None else wa, u64s(ta), len(tb) if wb is None else wb, u64s(tb),
                                            len(pairs), u64s([i for i, _ in pairs] or [0]), u64s([l for _, l in pairs] or [0]),
                                            cbit))


def c_decode(lib, ta, tb, pairs, cbit, q):
    entry, lt, rt = C.c_uint64(77), C.c_uint64(77), C.c_uint64(77)
    if not lib.csgn_uint_bilinear_decode(len(ta), u64s(ta), len(tb), u64s(tb), len(pairs), u64s([i for i, _ in pairs] or [0]),
                                         u64s([l for _, l in pairs] or [0]), cbit, q, C.byref(entry), C.byref(lt),
                                         C.byref(rt)):
        assert entry.value == lt.value == rt.value == 77
        return None
    e = entry.value
    return (ONE if e == len(pairs) else ZERO if e == len(pairs) + 1 else e), lt.value, rt.value


def c_launches(lib, n, batch, ta, tb, form, constant):
    plan = (C.c_uint64 * 12)()
    first, left, right = flat(form)
    rc = lib.csgn_uint_bilinear_launches(n, batch, len(ta), u64s(ta), len(tb), u64s(tb), len(form), first, left, right,
                                         constant, plan)
    assert rc == 0, lib.csgn_last_error()
    return [int(x) for x in plan]


# -- the definition against the genuine reference and the oracle -------------------------------------------------------
def pair_lists(wa, wb):
    """Every list of up to three (left, right) pairs, repetitions and unsorted order included."""
    every = [(i, l) for i in range(wa) for l in range(wb)]
    return [list(p) for k in range(4) for p in itertools.product(every, repeat=k)]


@pytest.mark.parametrize("n,d", [(65, 4), (1247, 16)])
@pytest.mark.parametrize("wa,wb", [(1, 1), (2, 1), (1, 3), (2, 2), (3, 3)])
def test_definition_matches_reference_and_oracle(oracle, n, d, wa, wb):
    """Every pair list of up to three entries at wa, wb <= 3 with term counts (1, 2, 3), with and without the constant,
    through the oracle's operator* and operator+ and, where the reference is built, through its own: the words of the
    numpy composition.  (3, 3) has 820 lists, 13 forms of up to 64 planes."""
    ref = load_ref()
    ta, tb = [1, 2, 3][:wa], [1, 2, 3][wb - 1::-1]
    a = [rand_terms(n, 1, t, 40 * wa + i) for i, t in enumerate(ta)]
    b = [rand_terms(n, 1, t, 50 * wb + l) for l, t in enumerate(tb)]
    fa, fb = [p[0].ravel() for p in a], [p[0].ravel() for p in b]
    dl = (n + 63) // 64
    routes = [oracle_ops(oracle, n)] + ([ref_ops(ref, n, d)] if ref is not None else [])
    lists = pair_lists(wa, wb)
    for g0 in range(0, len(lists), 64):
        form = lists[g0:g0 + 64]
        for constant in (0, low(len(form))):
            want = np_bilinear(n, a, b, form, constant)
            for add, mul in routes:
                got = compose_bilinear(fa, fb, form, constant, add, mul, const_term(n, 1), const_term(n, 0))
                for x, pairs in enumerate(form):
                    assert np.array_equal(got[x], want[x].ravel()), (pairs, constant)
                    assert got[x].size == bilinear_terms(ta, tb, pairs, (constant >> x) & 1) * dl


# -- the C ABI, host side ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", [([1], [1]), ([1, 1, 1], [1, 1]), ([2, 2], [3, 3, 3]), ([1, 2, 3], [3, 1]),
                                   ([3, 70], [1, 5, 2]), ([4], [1, 2, 3, 4, 5])])
def test_terms_and_decode_give_the_table(lib, ta, tb):
    """Equal counts (the divisions) and unequal ones (the search): every term of every short pair list, and of random
    longer ones, against the symbolic composition and the model's decode."""
    wa, wb = len(ta), len(tb)
    forms = pair_lists(min(wa, 2), min(wb, 2))[::1 if sum(ta) * sum(tb) < 100 else 7] + random_form(wa, wb, 6, 9, wa + 7 * wb)
    for cbit in (0, 1):
        for pairs in forms:
            T = bilinear_terms(ta, tb, pairs, cbit)
            assert c_terms(lib, ta, tb, pairs, cbit) == T > 0, (pairs, cbit)
            want = symbolic_bilinear(ta, tb, [pairs], cbit)[0]
            assert len(want) == T
            for q in range(T):
                got = c_decode(lib, ta, tb, pairs, cbit, q)
                assert got == bilinear_decode(ta, tb, pairs, cbit, q), (pairs, cbit, q)
                label = (got[0],) if got[0] in (ONE, ZERO) else (pairs[got[0]][0], got[1], pairs[got[0]][1], got[2])
                assert label == want[q], (pairs, cbit, q)
            assert c_decode(lib, ta, tb, pairs, cbit, T) is None


def test_terms_by_hand_and_refusals(lib):
    assert c_terms(lib, [1] * 32, [1] * 32, f_clmul(32)[31], 0) == 32 and c_terms(lib, [1] * 32, [1] * 32, f_clmul(32)[0], 1) == 2
    assert c_terms(lib, [4, 5], [6, 7], [(0, 0), (1, 1), (0, 0)], 1) == 24 + 35 + 24 + 1
    assert c_terms(lib, [4, 5], [6, 7], [], 0) == 1 and c_terms(lib, [4, 5], [6, 7], [], 1) == 1
    assert c_decode(lib, [4, 5], [6, 7], [], 0, 0) == (ZERO, 0, 0) and c_decode(lib, [4, 5], [6, 7], [], 1, 0) == (ONE, 0, 0)
    assert c_decode(lib, [4, 5], [6, 7], [(0, 0), (1, 1)], 1, 23) == (0, 3, 5)
    assert c_decode(lib, [4, 5], [6, 7], [(0, 0), (1, 1)], 1, 24 + 8) == (1, 1, 1)
    assert c_decode(lib, [4, 5], [6, 7], [(0, 0), (1, 1)], 1, 59) == (ONE, 0, 0)
    assert c_decode(lib, [2, 2], [3, 3], [(1, 0), (0, 1), (1, 0)], 0, 17) == (2, 1, 2)        # the divisions
    # refused: the widths, a null pointer, a zero count, an index at its width, the constant bit
    assert c_terms(lib, [1] * 65, [1], [], 0, wa=65) == 0 and c_terms(lib, [1], [1], [], 0, wb=0) == 0
    assert int(lib.csgn_uint_bilinear_terms(1, None, 1, u64s([1]), 0, None, None, 0)) == 0
    assert int(lib.csgn_uint_bilinear_terms(1, u64s([1]), 1, u64s([1]), 1, None, u64s([0]), 0)) == 0
    assert int(lib.csgn_uint_bilinear_terms(1, u64s([1]), 1, u64s([1]), 0, None, None, 1)) == 1
    assert c_terms(lib, [1, 0], [1], [(0, 0)], 0) == 0 and c_terms(lib, [1], [1, 0], [(0, 0)], 0) == 0
    assert c_terms(lib, [1, 1], [1], [(2, 0)], 0) == 0 and c_terms(lib, [1, 1], [1], [(0, 1)], 0) == 0
    assert c_terms(lib, [1], [1], [(0, 0)], 2) == 0
    # 2^62, without wrap-around
    big = LIMIT - 1
    assert c_terms(lib, [big], [1], [(0, 0)], 0) == big and c_terms(lib, [big], [1], [(0, 0)], 1) == 0
    assert c_terms(lib, [LIMIT], [1], [], 0) == 0 and c_terms(lib, [1 << 31], [1 << 31], [(0, 0)], 0) == 0
    assert c_terms(lib, [1 << 32], [1 << 32], [(0, 0)], 0) == 0 and c_terms(lib, [1 << 40], [1 << 40], [(0, 0)], 0) == 0
    assert c_terms(lib, [1 << 30], [1 << 30], [(0, 0)] * 3, 0) == 3 << 60 and c_terms(lib, [1 << 30], [1 << 30], [(0, 0)] * 4, 0) == 0
    assert c_terms(lib, [1 << 30], [1 << 30], [(0, 0)] * 3, 1) == (3 << 60) + 1
    assert c_terms(lib, [1 << 31], [1 << 30], [(0, 0)] * 8, 0) == 0                            # sums to 2^64
    assert lib.csgn_uint_bilinear_decode(1, u64s([1]), 1, u64s([1]), 1, u64s([0]), u64s([0]), 0, 0, None, None, None) == 0
    assert c_decode(lib, [1 << 16], [1 << 15], [(0, 0)], 0, 5) is None                        # a plane of 2^31 terms


# -- the launches, replayed ----------------------------------------------------------------------------------------------
def units_of(n, wide):
    dl = (n + 63) // 64
    return dl // 2 if wide and dl % 2 == 0 else dl


def cut_of(n, ta, tb, T, batch, wide):
    """(U, units, operand units, staged, G, S, chunk) by the rules include/csgn_hip.h states."""
    U = units_of(n, wide)
    ub = 16 if wide and ((n + 63) // 64) % 2 == 0 else 8
    units, op = sum(T) * U, (sum(ta) + sum(tb)) * U
    staged = op * ub <= STAGE_BYTES and units >= STAGE_MIN_RATIO * op
    G = STAGE_BYTES // (op * ub) if staged else max(1, TILE_UNITS // units)
    G = min(G, batch, max(1, (1 << 31) // units))
    least = max(MIN_CHUNK, STAGE_RATIO * G * op) if staged else MIN_CHUNK
    S = max(1, G * units // least)
    chunk = -(-(-(-G * units // S)) // 256) * 256
    return U, units, op, staged, G, S, chunk


def check_launches(lib, knobs, n, ta, tb, form, constant, batch, cap=0, xcd=False):
    """The figures against their definition, then every position of every workgroup of every launch placed as the
    kernel places it: every unit of every output plane exactly once, every source in range."""
    knobs.set("launch_blocks", cap)
    plan = c_launches(lib, n, batch, ta, tb, form, constant)
    T = [bilinear_terms(ta, tb, p, (constant >> x) & 1) for x, p in enumerate(form)]
    dl = (n + 63) // 64
    U, units, op, staged, G, S, chunk = cut_of(n, ta, tb, T, batch, True)
    assert plan[0] == (16 if dl % 2 == 0 else 8) and plan[7] == 1 and plan[11] == STAGE_BYTES
    assert (plan[1], plan[2], plan[3], plan[4], plan[8], plan[9], plan[10]) == (units, G, -(-batch // G), S, int(staged), chunk, op)
    count, launches, per, first = replay_grid(ta, tb, form, constant, batch, U, G, S, chunk, staged, STAGE_BYTES // plan[0],
                                              cap if cap else MAX_BLOCKS)
    assert (plan[4], plan[5], plan[6]) == (per, launches, first)
    for x, c in enumerate(count):
        assert c.size == batch * T[x] * U and (c == 1).all(), (n, ta, tb, form[x], batch, cap, x)
    if xcd:                                                          # the same launches in the XCD-contiguous block order
        order = lambda b, nb: lib.csgn_debug_block_order(b, nb, 0)   # noqa: E731
        for c in replay_grid(ta, tb, form, constant, batch, U, G, S, chunk, staged, STAGE_BYTES // plan[0],
                             cap if cap else MAX_BLOCKS, order)[0]:
            assert (c == 1).all()
    if plan[0] == 16:                                                # the same shape with a pointer off alignment
        U8, _, _, staged8, G8, S8, chunk8 = cut_of(n, ta, tb, T, batch, False)
        for c in replay_grid(ta, tb, form, constant, batch, U8, G8, S8, chunk8, staged8, STAGE_BYTES // 8, MAX_BLOCKS)[0]:
            assert (c == 1).all()
    return plan


@pytest.mark.parametrize("n", NS)
def test_launches_cover_every_unit_once(lib, knobs, n):
    for name, ta, tb, form, constant, batches in gpu_shapes() + [BOUNDARIES]:
        for batch in batches:
            check_launches(lib, knobs, n, ta, tb, form, constant, batch, xcd=n == 1247 and batch < 257)
    for ta, tb, form, constant in ALIASED:
        check_launches(lib, knobs, n, ta, tb, form, constant, ALIASED_BATCH)


def test_launches_of_the_dense_shapes_the_budget_and_the_splits(lib, knobs):
    for name, n, ta, tb, form, constant, batches in DENSE:
        for batch in batches:
            plan = check_launches(lib, knobs, n, ta, tb, form, constant, batch)
            assert plan[8] == (0 if name == "random64" and n == 1247 else 1) and plan[4] > 1, name   # several workgroups a tile
    # the LDS budget: 102 operand terms of 160 bytes fit, 103 do not, 215 are the issue's shape
    for (name, ta, tb, form, constant, batches), staged in ((UNSTAGED, 0), (STAGED_EDGE, 1), (PAST_EDGE, 0)):
        plan = check_launches(lib, knobs, 1247, ta, tb, form, constant, batches[0])
        assert plan[8] == staged and (sum(ta) + sum(tb)) * 160 <= STAGE_BYTES if staged else plan[8] == 0, name
    assert sum(STAGED_EDGE[1]) + sum(STAGED_EDGE[2]) + 1 == sum(PAST_EDGE[1]) + sum(PAST_EDGE[2]) == 103
    # a form that writes less than twice what it reads is not staged: dotBits
    assert check_launches(lib, knobs, 1247, [1] * 8, [1] * 8, f_dot_bits(8), 0, 40)[8] == 0
    # two full tiles and a partial one, then launches cut between tiles
    for (name, n, ta, tb, form, constant, _), batch in XCD_DENSE:    # several tiles in the XCD order, whole and split
        plan = check_launches(lib, knobs, n, ta, tb, form, constant, batch, xcd=True)
        assert plan[3] > 2
        assert check_launches(lib, knobs, n, ta, tb, form, constant, batch, 2 * plan[4], xcd=True)[5] > 1
    for n, (name, ta, tb, form, constant, _) in ((n, gpu_shapes()[i]) for n, i in TILE_SHAPES):
        G = c_launches(lib, n, 1 << 30, ta, tb, form, constant)[2]
        assert G > 5
        plan = check_launches(lib, knobs, n, ta, tb, form, constant, 2 * G + 5)
        assert plan[2:4] == [G, 3] and plan[5] == 1
        per = plan[4]
        assert per > 1                                               # so that per - 1 is a cap below a tile's workgroups
        for cap, launches in ((per, 3), (2 * per, 2), (per - 1, 3), (3 * per, 1)):
            assert check_launches(lib, knobs, n, ta, tb, form, constant, 2 * G + 5, cap)[5] == launches, (name, cap)
    assert c_launches(lib, 1247, 0, [1], [1], [[(0, 0)]], 0)[3:7] == [0, 1, 0, 0]


def test_plane_groups_of_a_tile_past_2_31_units(lib, knobs):
    """Eight planes of 2^26 terms at n = 1247 (10 units a term): one element of all planes passes 2^31 units, so G = 1
    and the planes go in runs of three, three and two, each a stream and a launch sequence of its own.  Host only."""
    ta, tb, form = [1 << 13], [1 << 13], [[(0, 0)]] * 8
    units = (1 << 26) * 10
    S = [3 * units // MIN_CHUNK, 3 * units // MIN_CHUNK, 2 * units // MIN_CHUNK]
    assert 3 * units <= 1 << 31 < 4 * units
    for cap, batch, launches in ((0, 2, 3), (0, 40, 8), (1000, 2, 6)):       # 17, 17 and 25 tiles a launch; one under the cap
        knobs.set("launch_blocks", cap)
        plan = c_launches(lib, 1247, batch, ta, tb, form, 0)
        assert plan[:5] == [16, 8 * units, 1, batch, sum(S)] and plan[7:9] == [3, 0], plan
        per_launch = [max(1, (cap or MAX_BLOCKS) // s) for s in S]
        assert plan[5] == launches == sum(-(-batch // t) for t in per_launch) and plan[6] == min(batch, per_launch[0]) * S[0]
        chunk = -(-(-(-3 * units // S[0])) // 256) * 256
        assert plan[9] == chunk and S[0] * chunk >= 3 * units and (S[0] - 1) * chunk < 3 * units
    # a single plane is always one group: its units stay below 2^31 by the size check
    assert c_launches(lib, 1247, 1, [1 << 13], [1 << 13], [[(0, 0)]], 0)[7] == 1


# -- the argument checks -----------------------------------------------------------------------------------------------
def test_argument_checks_in_order(lib):
    """The status is that of the first check that fails.  csgn_uint_bilinear_create: the plan pointer, wa, wb, n_out and
    the constant, the host arrays, h_first, the entry arrays (INVALID), 262144 entries (UNSUPPORTED), term counts,
    indices and overflow (INVALID), a plane of 2^31 terms (UNSUPPORTED), and only then the device (NO_DEVICE on a box
    without one).  csgn_uint_bilinear_launches adds n_bits in front and h_plan and the sizes behind; csgn_uint_bilinear
    checks n_bits, the host arrays and the plan."""
    import torch
    gpu = torch.cuda.is_available()
    one = u64s([1] * 64)
    first3, left3, right3 = flat([[(0, 0), (7, 7)], [], [(3, 2)]])
    handle = C.c_void_p(5)

    def create(wa=8, ta=one, wb=8, tb=one, m=3, first=first3, left=left3, right=right3, constant=0b110, plan=C.byref(handle)):
        return lib.csgn_uint_bilinear_create(wa, ta, wb, tb, m, first, left, right, constant, plan)

    def launches(n=1247, batch=4, wa=8, ta=one, wb=8, tb=one, m=3, first=first3, left=left3, right=right3, constant=0b110,
                 plan=(C.c_uint64 * 12)()):
        return lib.csgn_uint_bilinear_launches(n, batch, wa, ta, wb, tb, m, first, left, right, constant, plan)

    assert create(plan=None, wa=0) == -1 and b"plan is null" in lib.csgn_last_error()
    assert create(wa=0, ta=None) == -1 and create(wa=65, wb=0) == -1 and b"wa" in lib.csgn_last_error()
    assert create(wb=0, m=0) == -1 and create(wb=65, m=0) == -1 and b"wb" in lib.csgn_last_error()
    assert create(m=0, ta=None) == -1 and create(m=65, ta=None) == -1
    assert create(constant=0b1000, ta=None) == -1 and b"does not fit" in lib.csgn_last_error()
    for arg in ("ta", "tb", "first"):                                # host arrays, before what they hold
        assert create(**{arg: None, "left": u64s([9, 9, 9])}) == -1 and b"null host pointer" in lib.csgn_last_error(), arg
    assert create(first=u64s([1, 2, 2, 3]), left=None) == -1 and b"h_first[0]" in lib.csgn_last_error()
    assert create(first=u64s([0, 2, 1, 3]), left=None) == -1 and b"descends" in lib.csgn_last_error()
    for arg in ("left", "right"):
        assert create(**{arg: None, "first": u64s([0, 2, 2, MAX_ENTRIES + 1])}) == -1, arg
        assert b"null host pointer" in lib.csgn_last_error(), arg
    assert create(first=u64s([0, 0, 0, 0]), left=None, right=None) in (0, -3)          # no entry: no entry arrays
    if gpu:
        lib.csgn_uint_bilinear_destroy(handle)
    assert create(first=u64s([0, 2, 2, MAX_ENTRIES + 1]), ta=u64s([0] * 8)) == -2 and b"entries" in lib.csgn_last_error()
    assert create(ta=u64s([1, 0] + [1] * 6), left=u64s([9, 9, 9])) == -1 and b"plane 1 of a" in lib.csgn_last_error()
    assert create(tb=u64s([1 << 62] * 8), left=u64s([9, 9, 9])) == -1 and b"plane 0 of b" in lib.csgn_last_error()
    assert create(left=u64s([0, 8, 3]), ta=u64s([1 << 61] * 8), tb=u64s([1 << 61] * 8)) == -1
    assert b"entry 1" in lib.csgn_last_error()
    assert create(wb=2) == -1 and b"entry 1" in lib.csgn_last_error()                  # right = 7 of 2 planes
    assert create(ta=u64s([1 << 61] * 8), tb=u64s([1 << 61] * 8)) == -1 and b"overflows" in lib.csgn_last_error()
    assert create(ta=u64s([1 << 31] * 8), tb=u64s([1 << 30] * 8)) == -1                # 2^61 + 2^61 in plane 0
    assert create(ta=u64s([1 << 16] * 8), tb=u64s([1 << 15] * 8)) == -2 and b"2^31" in lib.csgn_last_error()
    assert handle.value is None                                      # every refusal leaves the handle null
    # the launches: n_bits first, then create's checks, then h_plan, then the sizes
    assert launches(n=0, wa=0) == -1 and launches(n=131073, wa=0) == -2
    assert launches(wa=0, plan=None) == -1 and b"wa" in lib.csgn_last_error()
    assert launches(ta=u64s([1 << 16] * 8), tb=u64s([1 << 15] * 8), plan=None) == -2
    assert launches(plan=None, batch=1 << 58) == -1 and b"null host pointer" in lib.csgn_last_error()
    assert launches(ta=u64s([1 << 27] * 8), tb=one, left=u64s([1, 1, 1]), right=u64s([1, 1, 1])) == -2
    assert b"plane 0 of a" in lib.csgn_last_error()
    assert launches(tb=u64s([1 << 27] * 8), first=u64s([0, 0, 0, 0])) == -2 and b"plane 0 of b" in lib.csgn_last_error()
    assert launches(ta=u64s([1 << 14] * 8), tb=u64s([1 << 13] * 8)) == -2 and b"output 0" in lib.csgn_last_error()
    assert launches(batch=1 << 56) == -2 and b"batch" in lib.csgn_last_error()
    assert launches() == 0 and launches(batch=0) == 0
    # the call: n_bits, the host arrays, the plan
    buf = np.zeros(64, dtype=np.uint64)
    ptrs = (C.c_void_p * 64)(*([buf.ctypes.data] * 64))
    assert lib.csgn_uint_bilinear(None, 0, 1, None, None, None, None) == -1
    assert lib.csgn_uint_bilinear(None, 131073, 1, ptrs, ptrs, ptrs, None) == -2
    for a, b, out in ((None, ptrs, ptrs), (ptrs, None, ptrs), (ptrs, ptrs, None)):
        assert lib.csgn_uint_bilinear(None, 1247, 1, a, b, out, None) == -1 and b"null host pointer" in lib.csgn_last_error()
    assert lib.csgn_uint_bilinear(None, 1247, 1, ptrs, ptrs, ptrs, None) == (-1 if gpu else -3)
    assert int(lib.csgn_uint_bilinear_plan_terms(None, 0)) == 0
    lib.csgn_uint_bilinear_destroy(None)
    if gpu:
        return
    assert create() == -3 and b"no CPU fallback" in lib.csgn_last_error() and handle.value is None
    assert lib.csgn_uint_bilinear(None, 1247, 0, ptrs, ptrs, ptrs, None) == -3


# -- clear values and decryptions --------------------------------------------------------------------------------------
def test_builders_restated():
    """clmul and gf_mul of tests/model_linear.py against the builders: all (x, y) at w <= 4, random at w = 8, 32, 64;
    gfMul(8, 0x11B) against the AES field; the host algebra of F2Bilinear."""
    rng = np.random.default_rng(38)
    for w in (1, 2, 3, 4, 8, 32, 64):
        poly = {1: 1, 2: 0b111, 3: 0b1011, 4: 0x13, 8: 0x11B, 32: 0x8D, 64: 0x1B}[w]
        forms = f_clmul(w), f_clmul_wide(w), f_gf_mul(w, poly), f_bitwise_and(w), f_dot_bits(w)
        assert [len(f) for f in forms] == [w, 2 * w - 1, w, w, 1]
        assert all(p == cancel(p) for f in forms for p in f)         # rows sorted by (left, right), nothing twice
        xy = [(x, y) for x in range(1 << w) for y in range(1 << w)] if w <= 4 else \
            [(int(x) & low(w), int(y) & low(w)) for x, y in rng.integers(0, 2**64, (40, 2), dtype=np.uint64)] + [(low(w), low(w)), (1, low(w))]
        for x, y in xy:
            assert clear_bilinear(forms[0], 0, x, y) == clmul(x, y) & low(w)
            assert clear_bilinear(forms[1], 0, x, y) == clmul(x, y)
            assert clear_bilinear(forms[2], 0, x, y) == gf_mul(w, x, y, poly)
            assert clear_bilinear(forms[3], 0, x, y) == x & y
            assert clear_bilinear(forms[4], 0, x, y) == bin(x & y).count("1") & 1
        if w <= 32:                                                  # gfMul is the reduction after the wide product
            assert f_after(reduction_rows(w, poly), f_clmul_wide(w)) == forms[2]
        k = (int(rng.integers(0, 2**64, dtype=np.uint64)) & low(w)) | 1            # a public factor on one side: compose
        assert f_compose(forms[2], m_gf_mul(w, k, poly), m_identity(w)) == f_compose(forms[2], m_identity(w), m_gf_mul(w, k, poly))
        assert f_xor(forms[0], forms[0]) == [[] for _ in range(w)]
    inv = {x: next(y for y in range(1, 256) if gf_mul(8, x, y, 0x11B) == 1) for x in range(1, 256)}
    aes = f_gf_mul(8, 0x11B)
    assert clear_bilinear(aes, 0, 0x57, 0x83) == 0xC1 and clear_bilinear(aes, 0, 0x53, 0xCA) == 1   # FIPS 197, 4.2
    assert all(clear_bilinear(aes, 0, x, inv[x]) == 1 for x in inv)
    assert sum(len(p) for p in aes) > 8 * 8 and sum(len(p) for p in f_gf_mul(64, 0x1B)) < MAX_ENTRIES


@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_decrypts(oracle, w):
    """Through the oracle's encrypt and decrypt at N = 127: the model's planes decrypt to the form's clear value for
    every pair (x, y) of w-bit values; the builders, random forms with repeated pairs, and a constant."""
    n, d = 127, 8
    key, _ = oracle.keygen(n, d, glibc_draws(1310 + w, 64 * d + 64))
    xs, ys = np.divmod(np.arange(1 << (2 * w), dtype=np.uint64), np.uint64(1 << w))
    a = encrypt_planes(oracle, n, key, xs, w, 1320 + w)
    b = encrypt_planes(oracle, n, key, ys, w, 1330 + w)
    poly = {1: 1, 2: 0b111, 3: 0b1011, 4: 0x13}[w]
    forms = [(f_clmul(w), 0), (f_clmul_wide(w), 1), (f_gf_mul(w, poly), low(w)), (f_dot_bits(w), 0), (f_bitwise_and(w), 0),
             (random_form(w, w, 5, 4, w), 0b10010), (random_form(w, w, 9, 2 * w, 3 * w) + [[]], 1 << 9)]
    for form, constant in forms:
        outs = np_bilinear(n, a, b, form, constant)
        want = np.array([clear_bilinear(form, constant, int(x), int(y)) for x, y in zip(xs, ys)], dtype=np.uint64)
        assert np.array_equal(decrypt_value(oracle, n, key, outs), want), (form, constant)
    sq = np_bilinear(n, a, a, f_gf_mul(w, poly), 0)                   # a and b the same planes: squares
    want = np.array([gf_mul(w, int(x), int(x), poly) for x in xs], dtype=np.uint64)
    assert np.array_equal(decrypt_value(oracle, n, key, sq), want)
