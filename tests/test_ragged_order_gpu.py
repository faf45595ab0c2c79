"""The grouped block order of the ragged kernels (xcd_grouped_block, csgn_device.h) and the output slices of the ragged
multiply, every word of every pair against the oracle.

k_add_ragged_flat, the CSR multiply k_mul_ragged_flat and the wave-cooperative k_mul_ragged_coop renumber their
workgroups in rounds of 8 * group: knobs ragged_xcd_group (default 64) and ragged_coop_xcd_group (default 0, the
contiguous eighths of xcd_contiguous_block).  At the default a round is 512 workgroups and the tail keeps its numbers, so
no small batch is ever renumbered; groups 1, 2 and 3 (rounds of 8, 16 and 24) are, and 0 is the contiguous order.  A
workgroup's range is block id * 256 * C units from the launch's unit_base, so a wrong grid in the remap writes one range
twice and leaves another holding the fill word (tests/model.py, GuardedOutputs).

N = 1247 (10 units of 16 bytes a term) and 1300 (21 units of 8 bytes).  The totals below are chosen by the workgroups
they make, ceil(units / (256 * C)) at C = ragged_c chunks a workgroup, so that at every group 1, 2, 3 and both C some
launch is below one round, some is whole rounds exactly and some is whole rounds and a tail
(test_totals_cover_every_round_class asserts it from the host's arithmetic).  The sum's launcher also cuts the call at
launch_blocks * 256 units (csgn_add.hip); the multiply's does not read that knob (its launches are the slices, csgn_mul.hip),
so its runs under a cap repeat the uncapped grid.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from csgn_amd.capi import check
from tests.model import GuardedOutputs, csr, hip, rand_terms  # noqa: F401
from tests.test_block_order_gpu import cdiv, units
from tests.test_launch_split_gpu import STREAM_NS

pytestmark = pytest.mark.gpu

GROUPS = (0, 1, 2, 3)
CHUNKS = (1, 8)
CAPS = (0, 15, 16)
# (workgroups, at C): the terms are the most that still make that many workgroups; 3001: the terms of
# tests/test_launch_split_gpu.py (118 / 15 workgroups at C = 1 / 8 at N = 1247, 247 / 31 at 1300)
TOTALS = {"5 at C1": (5, 1), "48 at C1": (48, 1), "3001 terms": None, "48 at C8": (48, 8), "53 at C8": (53, 8)}


def total_terms(n, kind):
    if TOTALS[kind] is None:
        return 3001
    blocks, c = TOTALS[kind]
    terms = blocks * 256 * c // units(n)[0]
    assert cdiv(terms * units(n)[0], 256 * c) == blocks
    return terms


def add_grids(n, terms, c, cap):
    """csgn_add.hip, add_ragged: launches of launch_blocks * 256 units, ceil(units / (256 * C)) workgroups each"""
    total = terms * units(n)[0]
    per = cap * 256 if cap else total
    return [cdiv(min(per, total - u0), 256 * c) for u0 in range(0, total, per)]


def mul_grids(n, terms, c):
    """csgn_mul.hip, flat_range without slices: one launch"""
    return [cdiv(terms * units(n)[0], 256 * c)]


def test_totals_cover_every_round_class():
    for n in STREAM_NS:
        for c in CHUNKS:
            for what in ("add", "mul"):
                grids = set()
                for kind in TOTALS:
                    terms = total_terms(n, kind)
                    for cap in CAPS:
                        grids |= set(add_grids(n, terms, c, cap) if what == "add" else mul_grids(n, terms, c))
                for group in (1, 2, 3):
                    r = 8 * group
                    assert any(g < r for g in grids), (n, c, what, group, "below one round")
                    assert any(g >= r and g % r == 0 for g in grids), (n, c, what, group, "whole rounds")
                    assert any(g > r and g % r for g in grids), (n, c, what, group, "rounds and a tail")


def small_sizes(seed, count, top=5):
    """`count` sizes of 0 to `top` terms, every seventh and the sixth empty (as ragged_sizes,
    tests/test_launch_split_gpu.py)"""
    sizes = np.random.default_rng(seed).integers(0, top + 1, size=count)
    sizes[::7] = 0
    sizes[5] = 0
    return sizes


def sum_batch(seed, total):
    """Pairs of small operands, empties among them, and one large operand a side that brings the sum to `total` terms"""
    count, top = (400, 5) if total > 2500 else (40, 5) if total > 400 else (12, 2)
    left, right = small_sizes(seed, count, top), small_sizes(seed + 1, count, top)[::-1].copy()
    left[5], right[count - 3] = 0, 0
    assert left.sum() + right.sum() + 2 <= total
    rest = total - int(left.sum() + right.sum())
    left[5], right[count - 3] = rest // 2, rest - rest // 2
    return left, right


def product_batch(seed, total):
    """Pairs of small operands, empty operands and empty pairs among them, one large pair and a 1 x r pair that bring the
    products to `total` terms"""
    count, top = (300, 5) if total > 2500 else (30, 5) if total > 400 else (8, 2)
    t1s, t2s = small_sizes(seed, count, top), small_sizes(seed + 1, count, top)[::-1].copy()
    t1s[4], t2s[4], t1s[6], t2s[6] = 0, 0, 0, 0
    rest = total - int((t1s * t2s).sum())
    assert rest > 0
    a = max(1, int(np.sqrt(rest)))
    t1s[4], t2s[4] = a, rest // a
    t1s[6], t2s[6] = (1, rest - a * (rest // a)) if rest - a * (rest // a) else (0, 3)
    assert int((t1s * t2s).sum()) == total
    return t1s, t2s


class Sum:
    """One ragged sum on the host and the device, every pair's words from the oracle's add"""

    def __init__(self, hip, oracle, n, total):
        self.hip, self.n, self.total, dl = hip, n, total, (n + 63) // 64
        t1s, t2s = sum_batch(n + total, total)
        self.off_l, self.off_r = csr(t1s), csr(t2s)
        left = rand_terms(n, 1, max(1, int(self.off_l[-1])), 5100 + n).ravel()
        right = rand_terms(n, 1, max(1, int(self.off_r[-1])), 5101 + n).ravel()
        self.want = np.concatenate([oracle.add(left[int(self.off_l[p]) * dl:int(self.off_l[p + 1]) * dl],
                                               right[int(self.off_r[p]) * dl:int(self.off_r[p + 1]) * dl])[0]
                                    for p in range(len(t1s))])
        assert self.want.size == total * dl
        self.dev = [hip.upload(x) for x in (left, self.off_l, right, self.off_r)]

    def run(self, what):
        hip, (d_l, d_ol, d_r, d_or) = self.hip, self.dev
        guarded = GuardedOutputs(hip, [self.want.size])
        off_out = hip.empty_words(len(self.off_l))
        check(hip.lib.csgn_add_ragged_bounded(self.n, len(self.off_l) - 1, 0, 0, d_l.data_ptr(), d_ol.data_ptr(),
                                              d_r.data_ptr(), d_or.data_ptr(), guarded.outs[0].data_ptr(),
                                              off_out.data_ptr(), self.total, hip.stream))
        torch.cuda.synchronize()
        assert np.array_equal(hip.download(off_out), self.off_l + self.off_r), what
        guarded.check([self.want], ("add_ragged", self.n) + what)


class Product:
    """One ragged product on the host and the device, every pair's words from the oracle's multiply"""

    def __init__(self, hip, oracle, n, t1s, t2s, seed):
        self.hip, self.n, dl = hip, n, (n + 63) // 64
        self.t1s, self.t2s = np.asarray(t1s, dtype=np.int64), np.asarray(t2s, dtype=np.int64)
        self.off_l, self.off_r = csr(self.t1s), csr(self.t2s)
        self.off_out = csr(self.t1s * self.t2s)
        self.total = int(self.off_out[-1])
        left = rand_terms(n, 1, max(1, int(self.off_l[-1])), seed).ravel()
        right = rand_terms(n, 1, max(1, int(self.off_r[-1])), seed + 1).ravel()
        parts = [oracle.mul(n, left[int(self.off_l[p]) * dl:int(self.off_l[p + 1]) * dl],
                            right[int(self.off_r[p]) * dl:int(self.off_r[p + 1]) * dl])[0]
                 for p in range(len(self.t1s)) if self.t1s[p] and self.t2s[p]]
        self.want = np.concatenate(parts)
        assert self.want.size == self.total * dl
        self.dev = [hip.upload(x) for x in (left, self.off_l, right, self.off_r)]

    def planned(self, what):
        """csgn_mul_plan_ragged and csgn_mul_planned into an output of exactly the planned size between guard words"""
        hip, (d_l, d_ol, d_r, d_or) = self.hip, self.dev
        batch = len(self.t1s)
        off_out = hip.empty_words(batch + 1)
        plan = (C.c_uint64 * 4)()
        handle = hip.mul_plan()
        try:
            check(hip.lib.csgn_mul_plan_ragged(handle, batch, d_ol.data_ptr(), d_or.data_ptr(), off_out.data_ptr(),
                                               C.byref(plan), hip.stream))
            assert int(plan[0]) == self.total, what
            guarded = GuardedOutputs(hip, [self.want.size])
            check(hip.lib.csgn_mul_planned(handle, self.n, d_l.data_ptr(), d_r.data_ptr(), guarded.outs[0].data_ptr(),
                                           hip.stream))
            torch.cuda.synchronize()
        finally:
            hip.lib.csgn_mul_plan_destroy(handle)
        assert np.array_equal(hip.download(off_out), self.off_out), what
        guarded.check([self.want], ("mul_ragged", self.n) + what)

    def unplanned(self, what):
        """csgn_mul_ragged_async with the exact total as the caller's bound"""
        hip, (d_l, d_ol, d_r, d_or) = self.hip, self.dev
        guarded = GuardedOutputs(hip, [self.want.size])
        _, off_out, plan = hip.mul_ragged_async(self.n, d_l, d_ol, d_r, d_or, self.total, out=guarded.outs[0])
        res = hip.mul_ragged_async_result(plan)
        assert res[0] == self.total and res[4] == 0, (what, res)
        assert np.array_equal(hip.download(off_out), self.off_out), what
        guarded.check([self.want], ("mul_ragged_async", self.n) + what)


def each_setting(knobs, run):
    for group in GROUPS:
        knobs.set("ragged_xcd_group", group)
        for c in CHUNKS:
            knobs.set("ragged_c", c)
            for cap in CAPS:
                knobs.set("launch_blocks", cap)
                run((group, c, cap))
    knobs.unset("launch_blocks")


@pytest.mark.parametrize("n", STREAM_NS)
@pytest.mark.parametrize("kind", list(TOTALS))
def test_add_ragged_grouped_order(hip, knobs, oracle, n, kind):
    """k_add_ragged_flat through csgn_add_ragged_bounded without bounds: groups 0, 1, 2, 3 by 1 and 8 chunks a workgroup,
    uncapped and in launches of 15 and 16 * 256 units."""
    batch = Sum(hip, oracle, n, total_terms(n, kind))
    each_setting(knobs, batch.run)


@pytest.mark.parametrize("n", STREAM_NS)
@pytest.mark.parametrize("kind", list(TOTALS))
def test_mul_ragged_grouped_order(hip, knobs, oracle, n, kind):
    """k_mul_ragged_flat through the plan and csgn_mul_planned, ragged_flat = 1 and ragged_coop = 0 as the tests of
    tests/test_gpu_parity.py force the CSR kernel: the same settings."""
    t1s, t2s = product_batch(n + 11, total_terms(n, kind))
    batch = Product(hip, oracle, n, t1s, t2s, 5200 + n)
    knobs.set("ragged_flat", 1)
    knobs.set("ragged_coop", 0)
    each_setting(knobs, batch.planned)


@pytest.mark.parametrize("n", STREAM_NS)
def test_mul_ragged_async_huge_pairs_in_front_of_a_grouped_launch(hip, knobs, oracle, n):
    """csgn_mul_ragged_async with recorded huge pairs (65 536 product terms and more): 1024 workgroups in front of the CSR
    launch multiply them, and the CSR workgroups behind renumber themselves on the grid WITHOUT those 1024
    (blockIdx.x - huge_blocks, gridDim.x - huge_blocks).  Two pairs of 256 x 256 and 257 x 256 terms between runs of
    small pairs and empties; the run in front fills the first two CSR workgroups (512 units), which would otherwise lie
    inside a recorded pair and write nothing whatever their number; groups 0 and 3."""
    small = small_sizes(n, 60)
    t1s = np.concatenate([small, [256], small[::-1], [257], small, [2]])
    t2s = np.concatenate([small[::-1], [256], small, [256], small[::-1], [3]])
    batch = Product(hip, oracle, n, t1s, t2s, 5300 + n)
    assert int((batch.t1s * batch.t2s >= 65536).sum()) == 2
    assert int(batch.off_out[60]) * units(n)[0] >= 512
    knobs.set("ragged_coop", 0)
    for group in (0, 3):
        knobs.set("ragged_xcd_group", group)
        batch.unplanned((group,))


def coop_grid(n, total, pairs, span_knob):
    """k_mul_ragged_coop over the whole output: the units and 64 of padding a pair, four waves of `span` units a
    workgroup (csgn_mul.hip; span = 64 * ragged_coop_span, or 512 at least)"""
    axis = total * units(n)[0] + 64 * pairs
    span = 64 * span_knob if span_knob else max(512, (axis // 16384) & ~63)
    return cdiv(axis, 4 * span)


@pytest.mark.parametrize("n", STREAM_NS)
def test_mul_ragged_coop_grouped_order(hip, knobs, oracle, n):
    """k_mul_ragged_coop (ragged_coop = 1): ragged_coop_xcd_group 0, 1 and 3 by stretches of one block a wave
    (ragged_coop_span = 1) and of the launcher's own choice (0: 512 units here).  3001 product terms in 300 pairs:
    30 010 + 19 200 units at N = 1247, 193 workgroups at span 1 and 25 at 512; 63 021 + 19 200 at 1300, 322 and 41: at
    both spans groups 1 and 3 have whole rounds and a tail."""
    t1s, t2s = product_batch(n + 13, 3001)
    batch = Product(hip, oracle, n, t1s, t2s, 5400 + n)
    grids = [coop_grid(n, batch.total, len(t1s), span) for span in (1, 0)]
    assert grids == ([193, 25] if n == 1247 else [322, 41])
    assert all(g > 24 and g % 8 and g % 24 for g in grids)
    knobs.set("ragged_flat", 1)
    knobs.set("ragged_coop", 1)
    for group in (0, 1, 3):
        knobs.set("ragged_coop_xcd_group", group)
        for span in (0, 1):
            knobs.set("ragged_coop_span", span)
            batch.planned(("coop", group, span))


SLICE_UNITS = (1 << 20) // 16           # ragged_slice_mb = 1: a slice is 1 MiB of 16-byte units


@pytest.mark.parametrize("kernel", ["csr", "coop"])
def test_mul_ragged_slices(hip, knobs, oracle, kernel):
    """ragged_slice_mb = 1 at N = 1247: an output of 30 000 terms, 300 000 units of 16 bytes (4.6 MiB), goes in four
    slices of 65 536 units and one of 37 856, each behind a touch of its operands: the CSR kernel in launches of 256
    and 148 workgroups from a unit_base of its own, the wave-cooperative kernel in its "slice of a large output" form
    (the unit axis, 16 blocks a wave: 16 and 10 workgroups).  Pairs of up to 12 x 12 terms and one of 60 x 50; a pair
    straddles every slice boundary.  (8-byte units are never sliced: the touch pass is the 16-byte path's.)  The block
    orders: the default and group 3."""
    n, total = 1247, 30000
    rng = np.random.default_rng(77)
    t1s, t2s = rng.integers(0, 13, size=900), rng.integers(0, 13, size=900)
    t1s[3], t2s[3] = 60, 50
    keep = int(np.searchsorted(np.cumsum(t1s * t2s), total))
    t1s, t2s = t1s[:keep], t2s[:keep]
    rest = total - int((t1s * t2s).sum())
    t1s, t2s = np.append(t1s, [1]), np.append(t2s, [rest])
    batch = Product(hip, oracle, n, t1s, t2s, 5500)
    assert batch.total == total and 200 < len(t1s) < 900
    U = units(n)[0]
    slices = cdiv(total * U, SLICE_UNITS)
    assert 4 <= slices <= 8
    for k in range(1, slices):
        p = int(np.searchsorted(batch.off_out * U, k * SLICE_UNITS, side="right")) - 1
        assert batch.off_out[p] * U < k * SLICE_UNITS < batch.off_out[p + 1] * U, (k, "no pair straddles the boundary")
    knobs.set("ragged_flat", 1)
    knobs.set("ragged_slice_mb", 1)
    knobs.set("ragged_coop", 1 if kernel == "coop" else 0)
    group_knob = "ragged_coop_xcd_group" if kernel == "coop" else "ragged_xcd_group"
    for group in (None, 3):
        if group is not None:
            knobs.set(group_knob, group)
        batch.planned((kernel, "slices", group))
