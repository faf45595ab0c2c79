"""Every kernel that reads stream_xcd (csgn_device.h), run in the XCD-contiguous block order, whole and split.

Unforced, a launcher turns the order on at 2^25 units, 512 MB a stream, which no test shape reaches; so knob stream_xcd
= 1 forces it.  xcd_contiguous_block is a bijection only on the grid it is given, and the kernels get that grid from
gridDim.x or from an nblocks argument the host refreshes for every launch of a split; a stale nblocks, or a remap
applied behind block_base, writes one slice of the output twice and leaves another untouched.  Every case therefore
runs uncapped (one launch) and under launch_blocks caps whose launches have grids below 8 (no whole round: only the
remainder term of the remap), grids of residues 0, 1, 4 and 7 mod 8 with at least one whole round, and a last launch
shorter than the others -- into outputs of exactly the documented size between guard words (tests/model.py,
GuardedOutputs), compared word for word with the model of the kernel's own GPU test, never with the unremapped run.

The grids in the docstrings follow from the host code's arithmetic (launch_groups in csgn_device.h, the tile policies
of the launchers named in each test); "k x g + r" means k launches of g workgroups and a last one of r.  The functions
below restate the three ways the host cuts a call, and every test asserts that its shape and caps cover the grids above.
Kernels whose launcher takes no cap (one launch below 2^32 units) vary the batch instead.
Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from csgn_amd.capi import check
from tests import model_placed as mp
from tests import test_count_gpu as cg
from tests import test_count_prefix_gpu as cpg
from tests import test_gates_gpu as gg
from tests import test_matmul_gpu as mm
from tests import test_placed_outputs_gpu as pog
from tests import test_uint_add_where_gpu as awg
from tests import test_uint_addk_gpu as akg
from tests import test_uint_arith_gpu as ag
from tests import test_uint_bitwise_gpu as bg
from tests import test_uint_find_gpu as fg
from tests import test_uint_first_gpu as frg
from tests import test_uint_gpu as ug
from tests import test_uint_lt_select_gpu as ltg
from tests import test_uint_lut_gpu as lg
from tests import test_uint_nth_gpu as ng
from tests import test_uint_pick_gpu as pg
from tests import test_uint_pick_rows_gpu as prg
from tests import test_uint_plain_gpu as plg
from tests import test_uint_read_gpu as rg
from tests import test_uint_write_gpu as wg
from tests import test_wsum_gpu as wsg
from tests.model import (ADD_FULL, LT, OR, GuardedOutputs, gate_terms, hip, lut_terms, np_gate,  # noqa: F401
                         np_gather_uniform, np_lut, np_plain, np_read_fast, np_step, plain_terms, rand_terms, read_terms,
                         step_terms)
from tests.model_addk import addk_terms, np_addk
from tests.model_arith import ADD
from tests.model_bitwise import SELECT, bitwise_terms
from tests.model_count import np_count
from tests.model_find import find_terms
from tests.model_matmul import np_matmul
from tests.model_pick import OPS as PICK_OPS
from tests.model_pick import np_pick_fast
from tests.model_pick_rows import np_pick_rows_fast
from tests.model_write import np_write_fast
from tests.model_wsum import np_wsum
from tests.test_launch_split_gpu import BATCH, NARROW_N, STREAM_NS, TERMS, WIDE_N, each_cap, words

pytestmark = pytest.mark.gpu

CAPS = (5, 9, 12, 15, 16)               # grids of 5 (no whole round) and of residues 1, 4, 7 and 0 mod 8


def units(n):
    """(units a term, bytes a unit) of a call whose pointers are 16-byte aligned: wide_units, csgn_device.h"""
    dl = (n + 63) // 64
    return (dl // 2, 16) if dl % 2 == 0 else (dl, 8)


def cdiv(a, b):
    return -(-a // b)


def group_grids(groups, per_group, cap):
    """launch_groups (csgn_device.h): as many groups of per_group workgroups a launch as the cap allows, one at least"""
    if not cap:
        return [groups * per_group]
    most = max(1, cap // per_group)
    return [min(most, groups - g0) * per_group for g0 in range(0, groups, most)]


def block_grids(total, cap):
    """the b0 loops (csgn_count.hip, csgn_wsum.hip, csgn_count_prefix.hip, csgn_gather.hip): cap workgroups a launch"""
    return [min(cap, total - b0) for b0 in range(0, total, cap)] if cap else [total]


def unit_grids(total_units, cap):
    """the u0 loop of the 1 x 1 multiply (csgn_mul.hip): cap * 256 units a launch, 256 a workgroup"""
    per = cap * 256 if cap else total_units
    return [cdiv(min(per, total_units - u0), 256) for u0 in range(0, total_units, per)]


def covered(splits, residues=(0, 1, 4, 7), split=True):
    """The launches of every run of a case (one list of grids per run, the uncapped run first): a grid below 8, grids of
    `residues` mod 8 with a whole round, a run whose last launch is shorter (`split`), and 17 workgroups or more
    uncapped."""
    grids = {g for run in splits for g in run}
    assert any(g < 8 for g in grids), splits
    assert set(residues) <= {g % 8 for g in grids if g >= 8}, splits
    assert not split or any(len(run) > 1 and run[-1] < run[0] for run in splits), splits
    assert len(splits[0]) == 1 and splits[0][0] >= 17, splits


def remapped(knobs, **forms):
    """stream_xcd forced on, and the kernel's form knob at the fused kernel"""
    knobs.set("stream_xcd", 1)
    for name, value in forms.items():
        knobs.set(name, value)


def batches_for(grid_of, limit=4000):
    """For a launcher without a cap: the smallest batches whose one launch (grid_of(batch) workgroups, by the launcher's
    arithmetic) has 5 to 7 workgroups, each residue 0, 1, 4, 7 with a whole round, and two rounds and a remainder."""
    kinds = [lambda g: 5 <= g < 8] + [lambda g, r=r: g >= 8 and g % 8 == r for r in (0, 1, 4, 7)] + \
            [lambda g: g >= 17 and g % 8 != 0]
    found = sorted({next(b for b in range(1, limit) if kind(grid_of(b))) for kind in kinds})
    covered([[grid_of(b)] for b in reversed(found)], split=False)
    return found


# ------------------------------------------------------------------------------ launch_groups: elements of a batch
# The shapes of tests/test_launch_split_gpu.py where it has the kernel (batch 301 at 32 and 33 units a term); elsewhere
# N = 1247 (10 units of 16 bytes) and 1300 (21 units of 8 bytes) and the batch that makes 23 groups of one workgroup:
# uncapped 23 (two rounds and 7); cap 5: 4 x 5 + 3; 9: 2 x 9 + 5; 12: 12 + 11; 15: 15 + 8; 16: 16 + 7.

def groups_of(batch, G):
    groups = cdiv(batch, G)
    covered([group_grids(groups, 1, cap) for cap in (0,) + CAPS])
    return groups


@pytest.mark.parametrize("n", [WIDE_N, NARROW_N])
def test_lut(hip, knobs, n):
    """k_uint_lut (a.nblocks): 5 fresh planes, 2 outputs of 32 terms, batch 301.  G = 2 at U = 32 (the subset tables'
    room), 3 at U = 33; one workgroup a group.  151 groups: 151; 30 x 5 + 1; 16 x 9 + 7; 12 x 12 + 7; 10 x 15 + 1;
    9 x 16 + 7.  101 groups: 101; 20 x 5 + 1; 11 x 9 + 2; 8 x 12 + 5; 6 x 15 + 11; 6 x 16 + 5."""
    ts, m = [1] * 5, 2
    table = [(1 << m) - 1] + [0] * ((1 << len(ts)) - 1)
    assert lut_terms(table, len(ts), m, ts) == [32, 32]
    assert groups_of(BATCH, 2 if n == WIDE_N else 3) == (151 if n == WIDE_N else 101)
    planes = [rand_terms(n, BATCH, t, 3000 + 7 * i + t) for i, t in enumerate(ts)]
    want = [x.ravel() for x in np_lut(n, planes, table, m)]
    remapped(knobs, uint_lut_fused=1)
    each_cap(knobs, lambda cap: lg.run(hip, n, planes, table, m, want), CAPS)


@pytest.mark.parametrize("n", [WIDE_N, NARROW_N])
def test_read(hip, knobs, n):
    """k_uint_read (sel_launch, csgn_selector.h): 3 fresh index planes, 8 rows (E = 27), table planes of 1 and 2 terms:
    81 U units an element, G = 3, one workgroup a group, 101 groups: the grids of test_lut's second list."""
    s, rows, t = [1, 1, 1], 8, [1, 2]
    assert read_terms(s, rows) == 27 and groups_of(BATCH, 3) == 101
    index = [rand_terms(n, BATCH, sk, 3100 + k) for k, sk in enumerate(s)]
    table = [rand_terms(n, rows, tj, 3110 + j) for j, tj in enumerate(t)]
    want = [x.ravel() for x in np_read_fast(n, index, table)]
    remapped(knobs, uint_read_fused=1)
    each_cap(knobs, lambda cap: rg.run(hip, n, index, table, want), CAPS)


@pytest.mark.parametrize("n", [WIDE_N, NARROW_N])
@pytest.mark.parametrize("rparts", [0, 1])
def test_find(hip, knobs, n, rparts):
    """k_uint_find: 5 rows, 2 fresh planes a side (P = 9), two 1-term value planes and member: G = 4 elements by RP = 4
    rows a workgroup, 76 groups.  uint_find_rparts unset: both row parts in one launch, 2 workgroups a group, so every
    grid is even: 152; 38 x 4; 19 x 8; 12 x 12 + 8; 10 x 14 + 12; 9 x 16 + 8.  uint_find_rparts = 1: the rows split too,
    4 rows and then 1, each over launches of one workgroup a group: 76; 15 x 5 + 1; 8 x 9 + 4; 6 x 12 + 4; 5 x 15 + 1;
    4 x 16 + 12."""
    u = s = t = [1, 1]
    rows = 5
    assert find_terms(u, s) == 9
    per_group = 1 if rparts else 2
    covered([group_grids(76, per_group, cap) for cap in (0,) + CAPS], (0, 1, 4, 7) if rparts else (0, 4))
    keys = [rand_terms(n, rows, uk, 3200 + k) for k, uk in enumerate(u)]
    query = [rand_terms(n, BATCH, sk, 3210 + k) for k, sk in enumerate(s)]
    values = [rand_terms(n, rows, tj, 3220 + j) for j, tj in enumerate(t)]
    want = fg.definition(n, keys, query, values, True)
    remapped(knobs, uint_find_form=1, uint_find_rparts=rparts)
    each_cap(knobs, lambda cap: fg.run(hip, n, keys, query, values, True, want), CAPS)


# (N, batch, elements a workgroup) of the kernels below: ReadTile::of (csgn_selector.h) gives a workgroup 8192 units to
# write, G = 8192 / (units of an element), where the fresh planes' subset tables leave room; the batch is 23 G - 1.
SMALL_NS = [1247, 1300]


def shape_of(n, wide, narrow):
    batch, G = wide if n == 1247 else narrow
    assert groups_of(batch, G) == 23 and (G == 1 or batch % G)
    return batch


@pytest.mark.parametrize("n", SMALL_NS)
@pytest.mark.parametrize("op", ["rotl", "each"])
def test_pick(hip, knobs, n, op):
    """k_uint_pick: 3 fresh distance planes, 5 value planes of one term; ROTL: E_j = 27, EACH over 6 rows: E_j = 24.
    An element writes 135 U (120 U) units: G = 6 at U = 10; G = 2 (ROTL), 3 (EACH) at U = 21.  23 groups."""
    batch = shape_of(n, (137, 6), (45, 2) if op == "rotl" else (68, 3))
    op = PICK_OPS[op]
    rows = 6 if op == pg.EACH else 0
    index, a = pg.operands(n, op, [1, 1, 1], 5, rows, 1, batch, 3300)
    want = [x.ravel() for x in np_pick_fast(n, op, index, a, rows)]
    remapped(knobs, uint_pick_fused=1)
    each_cap(knobs, lambda cap: pg.run(hip, n, op, index, a, rows, want), CAPS)


@pytest.mark.parametrize("n", SMALL_NS)
def test_pick_rows(hip, knobs, n):
    """k_uint_pick_rows: 2 fresh index planes, 3 rows, three planes (what csgn_uint_write leaves, a lone row of 40 terms,
    random sizes): E = 8, 174 terms an element: G = 4 at U = 10, 2 at U = 21.  23 groups."""
    batch = shape_of(n, (91, 4), (45, 2))
    s = [1, 1]
    kinds = prg.tables(s, 3, 9)
    T = [kinds["written"], kinds["lone"], kinds["random"]]
    assert sum(prg.out_terms(s, t) for t in T) == 174
    index, arrays = prg.operands(n, s, T, batch, 3400)
    want = [x.ravel() for x in np_pick_rows_fast(n, index, arrays, T)]
    remapped(knobs, uint_pick_rows_form=1)
    assert prg.form_name(hip, n, batch, s, T) == b"k_uint_pick_rows"
    each_cap(knobs, lambda cap: prg.run(hip, n, index, arrays, T, want), CAPS)


@pytest.mark.parametrize("n", SMALL_NS)
def test_write(hip, knobs, n):
    """k_uint_write: 3 fresh index planes, 6 rows, 5 planes of fresh values and arrays: E = 24, 270 terms an element:
    G = 3 at U = 10, 1 at U = 21.  23 groups."""
    batch = shape_of(n, (68, 3), (23, 1))
    s, rows, tv, td = [1, 1, 1], 6, [1] * 5, [1] * 5
    assert sum(wg.array_terms(s, rows, a, b) for a, b in zip(tv, td)) == 270
    index, value, arrays = wg.operands(n, s, rows, tv, td, batch, 3500)
    want = [x.ravel() for x in np_write_fast(n, index, value, arrays, rows)]
    remapped(knobs, uint_write_fused=1)
    each_cap(knobs, lambda cap: wg.run(hip, n, index, value, arrays, rows, want), CAPS)


@pytest.mark.parametrize("n", SMALL_NS)
def test_first(hip, knobs, n):
    """k_uint_first: groups of 3 fresh mask rows (Q = 7), value planes of 1 and 2 terms and any, no labels: 28 terms an
    element: G = 25 (29 by the units, 25 by the tables' room) at U = 10, 13 at U = 21.  23 groups."""
    batch = shape_of(n, (574, 25), (298, 13))
    g, s = 3, [1, 1, 1]
    mask, values, mask_rows, value_rows = frg.operands(n, batch, g, s, [1, 2], True, 3600)
    want = frg.definition(n, mask_rows, value_rows, True, None, [])
    remapped(knobs)
    each_cap(knobs, lambda cap: frg.run(hip, n, batch, g, mask, s, values, True, None, [], want), CAPS)


@pytest.mark.parametrize("n", SMALL_NS)
def test_nth(hip, knobs, n):
    """k_uint_nth: groups of 3 fresh mask rows, slot 1 (Q = 3), value planes of 1 and 2 terms and valid, no labels: 12
    terms an element: G = 25 (the tables' room) at U = 10, 24 at U = 21.  23 groups."""
    batch = shape_of(n, (574, 25), (551, 24))
    g, slot = 3, 1
    mask, values, mask_rows, value_rows = ng.operands(n, batch, g, 1, [1, 2], True, 3700)
    want = ng.definition(mask_rows, value_rows, slot, True, None, [])
    remapped(knobs)
    each_cap(knobs, lambda cap: ng.run(hip, n, batch, g, slot, mask, 1, values, True, None, [], want), CAPS)


@pytest.mark.parametrize("n", SMALL_NS)
def test_lt_select(hip, knobs, n):
    """k_uint_lt_select: 3 fresh planes a side (L = 26), three requests of 1 + 1 terms and the comparison: an element
    writes 182 U units of a part's 8192, so G doubles to 8 at U = 10 and 4 at U = 21.  23 groups."""
    batch = shape_of(n, (183, 8), (91, 4))
    ops = ltg.operands(hip, n, batch, [1] * 3, [1] * 3, extra_terms=(1, 1), seed=38)
    xs, ys = [ops.a(0), ops.extra(0), ops.b(1)], [ops.b(0), ops.extra(1), ops.b(2)]
    want = ops.want(xs, ys, True)
    remapped(knobs, uint_lt_select_form=1)
    each_cap(knobs, lambda cap: ops.run(xs, ys, True, want), CAPS)


@pytest.mark.parametrize("n", SMALL_NS)
def test_arith(hip, knobs, n):
    """k_uint_arith: a + b of 3 fresh planes with the carry, 2 + 3 + 5 + 7 = 17 terms an element.  The call is small, so
    a part is batch * 17 U / 512 units (kFillBlocks), at least 1024: 1024 at both widths; G doubles to 8 at U = 10 and
    4 at U = 21.  23 groups."""
    batch = shape_of(n, (183, 8), (91, 4))
    ops = ag.operands(hip, n, batch, [1] * 3, [1] * 3, seed=39)
    remapped(knobs)
    each_cap(knobs, lambda cap: ops.check_forms(knobs, ADD, True, (1,)), CAPS)


@pytest.mark.parametrize("n", SMALL_NS)
def test_add_where(hip, knobs, n):
    """k_uint_add_where, the staged form: a + (s ? 15 : 0) of 4 fresh planes and a fresh s with the carry, 2 + 3 + 5 + 9
    + 15 = 34 terms an element; parts of 1024 units as in k_uint_arith: G = ceil(1024 / 34 U) = 4 at U = 10, 2 at
    U = 21.  23 groups."""
    batch = shape_of(n, (91, 4), (45, 2))
    case = awg.Case(hip, n, batch, [1] * 4, 1, 0xF, seed=40)
    assert sum(case.T) == 34
    remapped(knobs)
    each_cap(knobs, lambda cap: case.check(True), CAPS)


# ------------------------------------------------------------------------------ the b0 loops: workgroups in order

def block_split_covered(total):
    covered([block_grids(total, cap) for cap in (0,) + CAPS])


@pytest.mark.parametrize("n", [65, 63])                     # one 16-byte unit a term; one 8-byte unit
def test_count(hip, knobs, n):
    """k_count (a.nblocks, a.block0): 7 elements of 33 fresh inputs, plane 1 (528 pairs), parts of 7 ranks: 76
    workgroups an element, 532: 532 (4 mod 8); 106 x 5 + 2; 59 x 9 + 1; 44 x 12 + 4; 35 x 15 + 7; 33 x 16 + 4."""
    block_split_covered(7 * cdiv(528, 7))
    x = rand_terms(n, 7 * 33, 1, 4000)
    wants = np_count(x, 33, [1])
    remapped(knobs, count_form=1, count_cpart=7)
    each_cap(knobs, lambda cap: cg.run(hip, n, 7, 33, x, [1], wants, "grouped"), CAPS)


@pytest.mark.parametrize("n", [65, 63])
def test_count_prefix(hip, knobs, n):
    """k_count_prefix: 7 elements of 9 fresh inputs, plane 1, parts of 7 ranks.  Inclusive: C(10, 3) = 120 ranks, 18
    workgroups an element, 126: 126; 25 x 5 + 1; 14 x 9; 10 x 12 + 6; 8 x 15 + 6; 7 x 16 + 14.  Exclusive: C(9, 3) = 84
    ranks, 12 an element, 84: 84; 16 x 5 + 4; 9 x 9 + 3; 7 x 12; 5 x 15 + 9; 5 x 16 + 4."""
    block_split_covered(7 * cdiv(120, 7))
    block_split_covered(7 * cdiv(84, 7))
    ref = cpg.Reference(n, 7, 9, 1, [1], 4100)
    assert [ex for ex, _, _ in ref.scans] == [False, True]
    remapped(knobs, count_cpart=7)
    each_cap(knobs, lambda cap: ref.check(hip, layouts=("grouped",)), CAPS)


@pytest.mark.parametrize("n", [65, 63])
def test_wsum(hip, knobs, n):
    """k_wsum: 7 elements of classes [3, 3] at 2 terms, planes 0 .. 3, parts of one selection: 3 + 6 + 12 + 3 = 24
    workgroups an element, 168: 168; 33 x 5 + 3; 18 x 9 + 6; 14 x 12; 11 x 15 + 3; 10 x 16 + 8."""
    block_split_covered(7 * 24)
    ns, t, js = [3, 3], 2, [0, 1, 2, 3]
    xs = wsg.class_inputs(n, ns, t, 7, 4200)
    wants = np_wsum(xs, ns, js)
    remapped(knobs, wsum_cpart=1)
    each_cap(knobs, lambda cap: wsg.run(hip, n, 7, ns, t, js, xs, wants), CAPS)


@pytest.mark.parametrize("n", STREAM_NS)
def test_gather_planes(hip, knobs, n):
    """k_gather (gridDim.x behind block_base): two planes of 1 and 3 terms, 3001 output elements, 1024 units a
    workgroup: 30 + 88 = 118 workgroups at 1247: 118; 23 x 5 + 3; 13 x 9 + 1; 9 x 12 + 10; 7 x 15 + 13; 7 x 16 + 6;
    62 + 185 = 247 at 1300: 247; 49 x 5 + 2; 27 x 9 + 4; 20 x 12 + 7; 16 x 15 + 7; 15 x 16 + 7."""
    dl, U = (n + 63) // 64, units(n)[0]
    terms, count_in, count_out = [1, 3], 97, TERMS
    total = sum(cdiv(count_out * t * U, 1024) for t in terms)
    assert total == (118 if n == 1247 else 247)
    block_split_covered(total)
    planes = [words(n + 41 * j, count_in * t * dl) for j, t in enumerate(terms)]
    dev = [hip.upload(p) for p in planes]
    idx = np.random.default_rng(n + 5).integers(0, count_in, size=count_out).astype(np.uint64)
    d_idx = hip.upload(idx)
    wants = [np_gather_uniform(planes[j], t, idx, dl) for j, t in enumerate(terms)]
    remapped(knobs)

    def call(cap):
        guarded = GuardedOutputs(hip, [x.size for x in wants])
        hip.gather_planes(n, dev, terms, count_in, count_out, d_idx, guarded.outs)
        torch.cuda.synchronize()
        guarded.check(wants, ("gather_planes", n, cap))

    each_cap(knobs, call, CAPS)


# ------------------------------------------------------------------------------ k_matmul

def matmul_runs(hip, knobs, n, a, b, rows, inner, cols):
    want = np_matmul(a, b, rows, inner, cols)
    each_cap(knobs, lambda cap: mm.run(hip, n, a, b, rows, inner, cols, False, want), CAPS)


@pytest.mark.parametrize("n", [65, 129])                    # one 16-byte unit a term; three 8-byte units
def test_matmul_rows(hip, knobs, n):
    """k_matmul (a.nblocks): 401 rows, inner = 3, 3 columns of fresh terms: an 8 x 2 tile, one part of e, two column
    tiles, so a group of 8 rows is 2 workgroups and every grid is even; 51 groups: 102; 25 x 4 + 2; 12 x 8 + 6;
    8 x 12 + 6; 7 x 14 + 4; 6 x 16 + 6."""
    covered([group_grids(51, 2, cap) for cap in (0,) + CAPS], (0, 4, 6))
    rows, inner, cols = 401, 3, 3
    a, b = rand_terms(n, rows * inner, 1, 4300), rand_terms(n, inner * cols, 1, 4310 + n)
    remapped(knobs, matmul_form=1)
    matmul_runs(hip, knobs, n, a, b, rows, inner, cols)


@pytest.mark.parametrize("n", [65, 129])
def test_matmul_parts_of_e(hip, knobs, n):
    """k_matmul at matmul_epart = 1: one row, inner = 300, 37 columns in 5 tiles of 1 x 8.  Uncapped every e is a part:
    5 x 300 = 1500 workgroups in one launch (4 mod 8).  A cap lengthens the parts to minE = ceil(300 / cap) values of
    e, which leaves ceil(300 / minE) = cap parts at every cap here, one tile a launch: 5 launches of 5, 9, 12, 15, 16."""
    inner, cols = 300, 37
    for cap in CAPS:
        assert cdiv(inner, cdiv(inner, cap)) == cap
    a, b = rand_terms(n, inner, 1, 4400 + n), rand_terms(n, inner * cols, 1, 4410)
    remapped(knobs, matmul_form=1, matmul_epart=1)
    matmul_runs(hip, knobs, n, a, b, 1, inner, cols)


# ------------------------------------------------------------------------------ the stream kernels

@pytest.mark.parametrize("n", STREAM_NS)
def test_mul_1x1_stream(hip, knobs, oracle, n):
    """k_and_stream (gridDim.x; stream_xcd is asked per launch): 3001 pairs of fresh terms, every pair from the oracle.
    30010 units at 1247: 118; 23 x 5 + 3; 13 x 9 + 1; 9 x 12 + 10; 7 x 15 + 13; 7 x 16 + 6.  63021 at 1300: 247;
    49 x 5 + 2; 27 x 9 + 4; 20 x 12 + 7; 16 x 15 + 7; 15 x 16 + 7."""
    dl, U = (n + 63) // 64, units(n)[0]
    covered([unit_grids(TERMS * U, cap) for cap in (0,) + CAPS])
    left, right = rand_terms(n, TERMS, 1, 4500 + n), rand_terms(n, TERMS, 1, 4501 + n)
    want = np.concatenate([oracle.mul(n, left[p].ravel(), right[p].ravel())[0] for p in range(TERMS)])
    assert want.size == TERMS * dl
    assert hip.lib.csgn_mul_uniform_kernel(n, TERMS, 1, 1) == b"k_and_stream"
    d_l, d_r = hip.upload(left.ravel()), hip.upload(right.ravel())
    remapped(knobs)

    def call(cap):
        guarded = GuardedOutputs(hip, [want.size])
        hip.mul_uniform(n, TERMS, 1, 1, d_l, d_r, out=guarded.outs[0])
        torch.cuda.synchronize()
        guarded.check([want], ("mul 1x1", n, cap))

    each_cap(knobs, call, CAPS)


@pytest.mark.parametrize("n", STREAM_NS)
def test_add_flat(hip, knobs, oracle, n):
    """k_add_flat, dense (gridDim.x, one launch below 2^32 units: no cap): pairs of 3 + 5 terms, 8 U units a pair and
    ceil(batch * 8 U / 256) workgroups; the batches whose grids are 5, 8, 9, 12, 15 and 17 at U = 10 and at U = 21."""
    dl, U = (n + 63) // 64, units(n)[0]
    t1, t2 = 3, 5
    batches = batches_for(lambda b: cdiv(b * (t1 + t2) * U, 256))
    assert sorted(cdiv(b * (t1 + t2) * U, 256) for b in batches) == [5, 8, 9, 12, 15, 17]
    top = batches[-1]
    left, right = rand_terms(n, top, t1, 4600 + n), rand_terms(n, top, t2, 4601 + n)
    want = np.stack([oracle.add(left[p].ravel(), right[p].ravel())[0] for p in range(top)])
    d_l, d_r = hip.upload(left.ravel()), hip.upload(right.ravel())
    remapped(knobs)
    for batch in batches:
        guarded = GuardedOutputs(hip, [batch * (t1 + t2) * dl])
        check(hip.lib.csgn_add_uniform(n, batch, t1, t2, d_l.data_ptr(), d_r.data_ptr(), guarded.outs[0].data_ptr(),
                                       hip.stream))
        torch.cuda.synchronize()
        guarded.check([want[:batch].ravel()], ("add", n, batch))


@pytest.mark.parametrize("n", STREAM_NS)
def test_add_flat_with_an_output_pitch(hip, knobs, n):
    """k_add_flat<PITCH> through a circuit that places (a + b) and copies c beside it (tests/model_placed.py,
    sum_in_sum: the sum with two operands and the strided copy with one), every word of the outer sum against numpy.
    a + b and c have 8 terms each, so both launches move batch * 8 U units: the batches of test_add_flat."""
    U = units(n)[0]
    remapped(knobs)
    for batch in batches_for(lambda b: cdiv(b * 8 * U, 256)):
        pog._run(hip, "sum_in_sum", n, batch, mp.sum_terms("sum_in_sum", 8), mp.PLACE, {"stream_xcd": 1})


# ------------------------------------------------------------------------------ one launch, the grid by the batch

@pytest.mark.parametrize("n", STREAM_NS)
def test_gate(hip, knobs, n):
    """k_gate_fused (gridDim.x): OR of 2 x 2 terms, 8 U units an element, ceil(batch * 8 U / 256) workgroups."""
    U = units(n)[0]
    ta = tb = 2
    assert gate_terms(OR, 1, ta, tb) == 8
    batches = batches_for(lambda b: cdiv(b * 8 * U, 256))
    a, b, s, plain = gg.operands(n, 1, ta, tb, batches[-1], 4700)
    want = np_gate(n, OR, a, b, s, plain)
    remapped(knobs, gate_fused=1)
    for batch in batches:
        gg.run_gate(hip, n, OR, a[:batch], b[:batch], s[:batch], plain[:batch], want[:batch].ravel())


@pytest.mark.parametrize("n", STREAM_NS)
def test_uint_step(hip, knobs, n):
    """k_uint_step (gridDim.x): ADD_FULL of fresh terms, 3 + 3 terms of sum and carry: 6 U units an element."""
    U = units(n)[0]
    assert step_terms(ADD_FULL, 1, 1, 1) == (3, 3)
    batches = batches_for(lambda b: cdiv(b * 6 * U, 256))
    top = batches[-1]
    x, a, b = rand_terms(n, top, 1, 4800), rand_terms(n, top, 1, 4801), rand_terms(n, top, 1, 4802)
    want = np_step(n, ADD_FULL, x, a, b)
    remapped(knobs, uint_fused=1)
    for batch in batches:
        ug.run_step(hip, n, ADD_FULL, x[:batch], a[:batch], b[:batch], want=[w[:batch].ravel() for w in want])


@pytest.mark.parametrize("n", STREAM_NS)
def test_uint_plain(hip, knobs, n):
    """k_uint_plain (gridDim.x): x < 5 over 3 fresh planes; a lane takes a run of up to 16 terms of one unit, so an
    element of T <= 16 terms is U lane items and the grid ceil(batch * U / 256)."""
    U = units(n)[0]
    w, k = 3, 5
    assert 0 < plain_terms(LT, w, k, [1] * w) <= 16
    batches = batches_for(lambda b: cdiv(b * U, 256))
    planes = [rand_terms(n, batches[-1], 1, 4900 + j) for j in range(w)]
    want = np_plain(n, LT, planes, k)
    remapped(knobs, uint_plain_fused=1)
    for batch in batches:
        plg.run(hip, n, LT, [p[:batch] for p in planes], k, want[:batch].ravel())


@pytest.mark.parametrize("n", STREAM_NS)
def test_uint_addk(hip, knobs, n):
    """k_uint_addk (gridDim.x): a + 5 over 3 planes of 1, 2 and 1 terms with the carry-out; every output plane's lanes
    are rounded up to whole workgroups: sum over the planes of ceil(batch * T_p * U / 256)."""
    U = units(n)[0]
    ts, k = [1, 2, 1], 5
    T = addk_terms(len(ts), k, ts)

    def grid(b):
        return sum(cdiv(b * t * U, 256) for t in T)

    batches = batches_for(grid)
    planes = [rand_terms(n, batches[-1], t, 5000 + j) for j, t in enumerate(ts)]
    outs, carry = np_addk(n, planes, k, False)
    remapped(knobs, uint_addk_fused=1)
    for batch in batches:
        akg.run(hip, n, [p[:batch] for p in planes], k, False, True,
                want=[o[:batch].ravel() for o in outs] + [carry[:batch].ravel()])


@pytest.mark.parametrize("n", STREAM_NS)
def test_uint_bitwise(hip, knobs, n):
    """k_uint_bitwise (gridDim.x; the host cuts the batch by lanes): SELECT over planes of (1, 2), (2, 1), (3, 4) terms
    under a selector of 2: T = 8, 7, 18, 33 U units an element, 121 elements.  A launch takes per = (cap - 3) * 256 /
    33 U elements, one at least, and sum over the planes of ceil(per * T_p * U / 256) workgroups; the caps are the
    smallest that give grids below 8, of residues 0, 1, 4, 7 with a whole round, and a shorter last launch."""
    U = units(n)[0]
    ta, tb, ts, batch = [1, 2, 3], [2, 1, 4], 2, 121
    T = [bitwise_terms(SELECT, ts, x, y) for x, y in zip(ta, tb)]
    assert T == [8, 7, 18]

    def grids(cap):
        per = max(1, (cap - 3) * 256 // (sum(T) * U)) if cap else batch
        return [sum(cdiv(min(per, batch - e0) * t * U, 256) for t in T) for e0 in range(0, batch, per)]

    kinds = [lambda g: g < 8] + [lambda g, r=r: g >= 8 and g % 8 == r for r in (0, 1, 4, 7)]
    caps = sorted({next(c for c in range(4, 400) if kind(grids(c)[0])) for kind in kinds})
    covered([grids(cap) for cap in [0] + caps])
    ops = bg.operands(hip, n, batch, ta, tb, ts, seed=51)
    remapped(knobs, uint_bitwise_form=1)
    each_cap(knobs, lambda cap: ops.run(SELECT), caps)
