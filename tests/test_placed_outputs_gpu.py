"""Placed products, sums and copies on the device (CSGN_CIRCUIT_PLACE): element e's result goes to out + e * pitch, a
slice of the sum that consumes it.  Circuits of three or four nodes (tests/model_placed.py: right, left, both, nested,
sum_in_sum) put the product of every shape of tests/test_mul_flat_block_index.py, and of the shapes the table of kernel
forms needs beside them, through k_mul_flat_blk<PITCH> at every (LONG, PF, units per lane), k_mul_flat<PITCH>, the
tiled kernel with a pitch and the pitched 1 x 1, and sums and copies through k_add_flat<PITCH> (two operands and one) and
k_copy_list at totals on, just below and just above a workgroup's edge.  Before a run the plan and csgn_circuit_stats
must show the placement the case is about (a failure, not a skip); the whole region of the sum is filled with FILL, so
that a word nobody wrote shows as never written; after it EVERY word of EVERY element of the sum equals concatenation
and all-pairs AND in numpy, and every input still holds what was uploaded -- with HOIST the other operand is copied into
the sum BEFORE the product runs, so a product that writes past its slice lands in words nobody rewrites.  A case is a few
hundred kilobytes and a graph of a few nodes; its operands and expected words are computed once."""
import ctypes as C

import numpy as np
import pytest

from csgn_amd.capi import check
from tests.model import FILL, hip  # noqa: F401  (fixture)
from tests import model_placed as mp

pytestmark = pytest.mark.gpu


def _run(hip, kind, n, batch, terms, flags, settings=None):
    """`settings`: the knobs the caller has ALREADY set (the launchers run under capture at build time), for the message."""
    import torch
    lib = hip.lib
    circ = mp.Circuit(lib, kind, n, batch, terms)
    try:
        d, dl, s = circ.d, circ.d.dl, circ.s
        circ.check_plan(d.plan(flags), flags)
        check(lib.csgn_circuit_build(d.c))
        stats = (C.c_uint64 * 8)()
        check(lib.csgn_circuit_stats(d.c, stats))
        placed, hoisted, kernels = circ.expected_counts(flags)
        assert (stats[4], stats[7], stats[3], stats[6]) == (placed, hoisted, kernels, 0), list(stats)
        inputs, want = mp.expected(circ)
        words = batch * d.terms[s] * dl
        assert int(lib.csgn_circuit_value_terms(d.c, s)) == d.terms[s]
        ps = lib.csgn_circuit_value(d.c, s)
        assert ps is not None
        fill = hip.upload(np.full(words, FILL, dtype=np.uint64))
        check(lib.csgn_memcpy_d2d(ps, fill.data_ptr(), words * 8, hip.stream))
        up = {v: hip.upload(np.array(inputs[v]).reshape(-1)) for v in circ.ins}        # (the shared arrays are read-only)
        for v, t in up.items():
            assert lib.csgn_circuit_value(d.c, v) is not None
            check(lib.csgn_memcpy_d2d(lib.csgn_circuit_value(d.c, v), t.data_ptr(), t.numel() * 8, hip.stream))
        check(lib.csgn_circuit_run(d.c, hip.stream))

        def fetch(v, count):
            t = torch.empty(count, dtype=torch.int64, device=fill.device)
            check(lib.csgn_memcpy_d2d(t.data_ptr(), lib.csgn_circuit_value(d.c, v), count * 8, hip.stream))
            torch.cuda.synchronize()
            return hip.download(t)

        got = fetch(s, words)
        ref = want[s].reshape(-1)
        wrong = got != ref
        if wrong.any():
            at = int(np.flatnonzero(wrong)[0])
            per = d.terms[s] * dl
            raise AssertionError((kind, n, batch, terms, flags, settings, "%d of %d words wrong" % (int(wrong.sum()), words),
                                  "%d of them never written" % int(np.count_nonzero(wrong & (got == FILL))),
                                  "first at element %d, word %d of %d" % (at // per, at % per, per),
                                  hex(int(got[at])), hex(int(ref[at]))))
        for v in circ.ins:
            assert np.array_equal(fetch(v, inputs[v].size), inputs[v].reshape(-1)), (kind, "input", v, "was overwritten")
    finally:
        circ.close()


def _run_all(runs):
    """Every run of a case, whatever the earlier ones did; the failures together."""
    failed = []
    for what, run in runs:
        try:
            run()
        except AssertionError as e:
            failed.append((what, e.args[0] if e.args else "assertion"))
    assert not failed, "%d of %d runs failed: %r" % (len(failed), len(runs), failed[:4])


@pytest.mark.parametrize("shape,setting", mp.PRODUCT_CASES)
def test_placed_product(hip, knobs, shape, setting):
    """One (shape, knob setting) of the table -- its entry asserted against the launcher's predicates -- in every run of
    PRODUCT_RUNS: as the first slice, a later slice (tc * dL words in: 8 bytes off a 16-byte boundary at N = 1300 with an
    odd tc), one of two placed products and a product nested two sums deep, with the other operand copied by the add
    (PLACE) or by the prologue before the product runs (PLACE | HOIST)."""
    assert mp.TABLE[shape][setting] == mp.instantiation(shape, setting)
    n, t1, t2, batch = mp.SHAPES[shape]
    settings = mp.knobs_of(shape, setting)
    for name, value in settings.items():
        knobs.set(name, value)
    assert hip.lib.csgn_mul_uniform_kernel(n, batch, t1, t2).decode() == mp.host_kernel_name(shape, setting)
    _run_all([((kind, flags, tc), lambda kind=kind, flags=flags, tc=tc:
               _run(hip, kind, n, batch, mp.product_terms(kind, shape, tc), flags, settings))
              for kind, flags, tc in mp.PRODUCT_RUNS])


def test_table_covers_every_kernel_form_with_a_pitch():
    mp.check_table_coverage()


@pytest.mark.parametrize("n,batch,T", mp.SUM_SHAPES)
def test_placed_sums_and_copies_at_the_last_workgroups_edge(hip, n, batch, T):
    """PLACE alone: a + b placed with both operands, and the one-operand copies of c (and d) beside a placed value, at
    batch * units on, just below and just above a multiple of 256, at both unit widths."""
    mp.check_sum_edges()
    _run_all([(kind, lambda kind=kind: _run(hip, kind, n, batch, mp.sum_terms(kind, T), mp.PLACE)) for kind in mp.SUM_KINDS])


@pytest.mark.parametrize("n,batch,terms", mp.HOIST_SHAPES)
def test_three_hoisted_inputs_in_one_prologue_launch(hip, n, batch, terms):
    """(a + b) + c with HOIST: three entries of different sizes in one k_copy_list launch and no other kernel; entries
    on a workgroup's edge; at N = 1300 wide and narrow entries side by side."""
    _run(hip, "sum_in_sum", n, batch, terms, mp.PLACE | mp.HOIST)
