"""The flat multiply's block-uniform indexing (k_mul_flat_blk): a workgroup decomposes its first unit once
and a lane places itself from its offset.  The shapes are the smallest at which that arithmetic can go wrong -- rows of
whole workgroups, rows of exactly one, workgroups that cross rows and pairs, a partial last workgroup, pairs on both
sides of the host's PU >= 256 * units-per-lane predicate, 8-byte units -- and EVERY word of EVERY product is compared
with the oracle.  A case is a few hundred kilobytes; its operands and expected words are computed once."""
import numpy as np
import pytest

from tests.model import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BENCH_ROWS = (1247, 2, 128, 3)       # rows of 1280 units = 5 whole workgroups: the bench geometry
ONE_BLOCK_ROWS = (4096, 3, 8, 4)     # CU = 256 exactly
CROSSING = (1247, 3, 26, 5)          # CU = 260: every workgroup crosses a row; PU = 780: pairs too; 3900 units: partial end
TALL_1247 = (1247, 191, 2, 3)        # config 5's products: rows of 20 and 64 units, two units per lane by default
TALL_4096 = (4096, 95, 2, 2)
PU_256 = (4096, 4, 2, 5)             # PU = 256 and 512: either side of the predicate with one and two units per lane
PU_512 = (4096, 8, 2, 5)
PU_260 = (1247, 13, 2, 7)            # two units per lane: the per-lane path
ODD_DL = (1300, 2, 13, 3)            # dL = 21: 8-byte units, CU = 273

_cases = {}


def _case(oracle, shape):
    """Operands and every expected word of a shape, computed once."""
    if shape not in _cases:
        n, t1, t2, batch = shape
        dl = oracle.default_len(n)
        L = oracle.synth(7001 + t1, n, 0, batch * t1 * dl)
        R = oracle.synth(9001 + t2, n, 0, batch * t2 * dl)
        want = np.concatenate([oracle.mul(n, L[b * t1 * dl:(b + 1) * t1 * dl], R[b * t2 * dl:(b + 1) * t2 * dl])[0]
                               for b in range(batch)])
        _cases[shape] = (L, R, want)
    return _cases[shape]


def _check(hip, oracle, shape):
    n, t1, t2, batch = shape
    L, R, want = _case(oracle, shape)
    got = hip.download(hip.mul_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R)))
    assert np.array_equal(got, want), shape


@pytest.mark.parametrize("shape", [BENCH_ROWS, ONE_BLOCK_ROWS, CROSSING, TALL_1247, TALL_4096, PU_256, PU_512, ODD_DL])
@pytest.mark.parametrize("touch", [3, 0])
def test_one_unit_per_lane(hip, oracle, knobs, shape, touch):
    """Every shape through the flat kernel with one unit per lane, behind the touch pass and (rows of a workgroup or
    more: with the in-kernel prefetch at its default distance, far past these launches' ends) without it."""
    knobs.set("mul_flat", 1)
    knobs.set("mul_touch", touch)
    _check(hip, oracle, shape)


@pytest.mark.parametrize("shape", [TALL_1247, TALL_4096])
def test_config5_products_by_default_dispatch(hip, oracle, shape):
    n, t1, t2, batch = shape
    assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2).decode() == "k_mul_flat"
    _check(hip, oracle, shape)


@pytest.mark.parametrize("shape", [CROSSING, ODD_DL, TALL_1247, TALL_4096])
@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("flat", [1, 2, 4, 8])
def test_block_crossing_shapes_at_every_width_and_order(hip, oracle, knobs, shape, flat, xcd):
    knobs.set("mul_flat", flat)
    knobs.set("mul_xcd", xcd)
    knobs.set("mul_touch", 3)
    _check(hip, oracle, shape)


@pytest.mark.parametrize("shape", [PU_256, PU_512, PU_260])
@pytest.mark.parametrize("flat", [1, 2])
def test_both_sides_of_the_host_predicate(hip, oracle, knobs, shape, flat):
    """PU = 256, 260 and 512 units against 256 and 512 units per workgroup."""
    knobs.set("mul_flat", flat)
    _check(hip, oracle, shape)


@pytest.mark.parametrize("shape,pf_kb", [(CROSSING, 8), (BENCH_ROWS, 32)])
@pytest.mark.parametrize("flat", [1, 2])
def test_prefetch_rows_inside_the_launch_and_past_its_end(hip, oracle, knobs, shape, pf_kb, flat):
    """Touch off and a prefetch distance of two rows (8 KiB over rows of 4160 bytes, 32 KiB over rows of 20 KiB): the
    first rows prefetch rows of the launch, the last two would reach past it and must not."""
    knobs.set("mul_flat", flat)
    knobs.set("mul_touch", 0)
    knobs.set("mul_pf_kb", pf_kb)
    _check(hip, oracle, shape)


def test_arena_wrap(hip, oracle, knobs):
    """Five pairs through two slots: launches of pairs 0-1, 2-3 and 4; slot 0 ends with pair 4, slot 1 with pair 3."""
    knobs.set("mul_flat", 1)
    n, t1, t2, batch = CROSSING
    L, R, want = _case(oracle, CROSSING)
    per = want.size // batch
    got = hip.download(hip.mul_uniform(n, batch, t1, t2, hip.upload(L), hip.upload(R), out_slots=2))
    assert got.size == 2 * per
    assert np.array_equal(got[:per], want[4 * per:])
    assert np.array_equal(got[per:], want[3 * per:4 * per])


@pytest.mark.parametrize("flat", [1, 2])
def test_operands_off_16_byte_alignment(hip, oracle, knobs, flat):
    """Operands one word off: the 8-byte-unit kernel, U = 20, rows of 520 units."""
    knobs.set("mul_flat", flat)
    n, t1, t2, batch = CROSSING
    L, R, want = _case(oracle, CROSSING)
    dL = hip.upload(np.concatenate([np.zeros(1, np.uint64), L]))[1:]
    dR = hip.upload(np.concatenate([np.zeros(1, np.uint64), R]))[1:]
    assert dL.data_ptr() % 16 == 8 and dR.data_ptr() % 16 == 8
    assert np.array_equal(hip.download(hip.mul_uniform(n, batch, t1, t2, dL, dR)), want)
