"""Placed outputs without a device: for every circuit, shape and flag set of tests/test_placed_outputs_gpu.py the plan
(csgn_circuit_plan_json) places what the case is about -- parent, offset, a pitch larger than the value, placed_a /
placed_b, the placed and hoisted counts -- and, executed in numpy at its offsets and pitches, computes the circuit; the
literal table of kernel forms (tests/model_placed.py) agrees, case by case, with the launcher's predicates restated
there and with csgn_mul_uniform_kernel under the case's knobs, and covers every form the multiply has with a pitch.
So the GPU file's preconditions are known to hold before anyone has a GPU."""
import numpy as np
import pytest

from csgn_amd import capi
from tests.model import execute, lib  # noqa: F401  (fixture)
from tests import model_placed as mp


def _plan_computes_the_circuit(lib, kind, n, batch, terms, flags):
    circ = mp.Circuit(lib, kind, n, batch, terms)
    try:
        plan = circ.d.plan(flags)
        circ.check_plan(plan, flags)
        inputs, want = mp.expected(circ)
        _, _, read = execute(circ.d, plan, inputs, np.zeros(circ.d.dl, dtype=np.uint64))
        assert np.array_equal(read(circ.s), want[circ.s])
        for v in circ.ins:
            assert np.array_equal(read(v), inputs[v])
    finally:
        circ.close()


@pytest.mark.parametrize("shape", list(mp.SHAPES))
def test_product_plans_place_the_product_and_compute_the_circuit(lib, shape):
    n, _, _, batch = mp.SHAPES[shape]
    for kind, flags, tc in mp.PRODUCT_RUNS:
        _plan_computes_the_circuit(lib, kind, n, batch, mp.product_terms(kind, shape, tc), flags)


@pytest.mark.parametrize("n,batch,T", mp.SUM_SHAPES)
def test_sum_and_copy_plans(lib, n, batch, T):
    for kind in mp.SUM_KINDS:
        for flags in mp.FLAGS:
            _plan_computes_the_circuit(lib, kind, n, batch, mp.sum_terms(kind, T), flags)


@pytest.mark.parametrize("n,batch,terms", mp.HOIST_SHAPES)
def test_hoisted_sum_plans(lib, n, batch, terms):
    assert len(set(terms)) == 3                                   # three entries of different sizes
    _plan_computes_the_circuit(lib, "sum_in_sum", n, batch, terms, mp.PLACE | mp.HOIST)


def test_sum_shapes_sit_on_the_last_workgroups_edge():
    mp.check_sum_edges()
    # every unit width has a total on the edge, one below and one above
    for n in (1247, 4096, 1300):
        edges = [e for (m, _, _), e in mp.SUM_EDGES.items() if m == n]
        assert min(edges) < 0 == sorted(edges)[1] < max(edges)
    assert {e for (m, _, _), e in mp.SUM_EDGES.items() if m == 1300} == {-1, 0, 1}


@pytest.mark.parametrize("shape", list(mp.TABLE))
def test_table_entries_are_what_the_launcher_would_run(lib, knobs, shape):
    n, t1, t2, batch = mp.SHAPES[shape]
    for setting, entry in mp.TABLE[shape].items():
        assert entry == mp.instantiation(shape, setting), setting
        knobs.restore()
        for name, value in mp.knobs_of(shape, setting).items():
            knobs.set(name, value)
        assert lib.csgn_mul_uniform_kernel(n, batch, t1, t2).decode() == mp.host_kernel_name(shape, setting), setting


def test_default_knobs_are_the_ones_the_restatement_assumes(lib):
    assert [capi.get_tuning(k) for k in ("mul_flat", "mul_xcd", "mul_touch", "mul_pf_kb", "shared_gpu")] == [0, 1, -1, -1, 0]


def test_table_covers_every_kernel_form_with_a_pitch():
    got = mp.check_table_coverage()
    assert all(shape in mp.SHAPES for cases in got.values() for shape, _ in cases)
    assert set(mp.TABLE) == set(mp.SHAPES)
    assert all(mp.SHAPES[s][3] >= 3 for s in mp.SHAPES)           # workgroups cross pairs where the skip applies
    # the three grid shapes take every width in both block orders
    for shape in ("CROSSING", "ODD_DL", "TALL_1247"):
        assert {"f%d%s" % (mf, x) for mf in (1, 2, 4, 8) for x in ("", "x0")} <= set(mp.TABLE[shape])
