"""a & b, a | b, a ^ b, ~a, select and keepWhere of encrypted integers on the device (csgn_uint_bitwise): every word of
every plane against the definition (tests/model_bitwise.py, pinned to the reference in tests/test_uint_bitwise_cpu.py),
in caller tensors between guard words, in both forms the knob uint_bitwise_form selects and with the knob left alone.
Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from tests.model import GuardedOutputs, hip, rand_terms, u64s  # noqa: F401
from tests.model_bitwise import OPS, READS_B, READS_SEL, SELECT, np_bitwise

pytestmark = pytest.mark.gpu

FORMS = (0, 1, None)                    # the planes, the kernel, the knob left alone


def shifted(hip, words, shift):
    """The words on the device, `shift` words off a fresh tensor's alignment."""
    if not shift:
        return hip.upload(words)
    return hip.upload(np.concatenate([np.zeros(shift, dtype=np.uint64), words]))[shift:]


class Operands:
    """a, b and the selector on the host and, uploaded once, on the device.  b_from / sel_from name planes of a that b's
    planes and the selector ARE (the same device pointers)."""

    def __init__(self, hip, n, a, b=None, sel=None, b_from=None, sel_from=None, shift=0):
        self.hip, self.n, self.w, self.batch = hip, n, len(a), a[0].shape[0]
        self.a = a
        self.da = [shifted(hip, p.ravel(), shift) for p in a]
        if b_from is not None:
            self.b, self.db = [a[j] for j in b_from], [self.da[j] for j in b_from]
        else:
            self.b, self.db = b, [shifted(hip, p.ravel(), shift) for p in b]
        if sel_from is not None:
            self.sel, self.dsel = a[sel_from], self.da[sel_from]
        else:
            self.sel, self.dsel = sel, shifted(hip, sel.ravel(), shift)
        self.ta, self.tb, self.ts = [p.shape[1] for p in self.a], [p.shape[1] for p in self.b], self.sel.shape[1]
        self.wants = {}

    def want(self, op):
        """The reference, computed once per op and left unchanged."""
        if op not in self.wants:
            self.wants[op] = [o.ravel() for o in np_bitwise(self.n, op, self.a, self.b, self.sel)]
        return self.wants[op]

    def run(self, op, shift=0):
        """One call into caller tensors of exactly the documented sizes between guard words; every word and both guards
        of every plane are checked (GuardedOutputs)."""
        want = self.want(op)
        guarded = GuardedOutputs(self.hip, [x.size for x in want], shift)
        self.hip.uint_bitwise(self.n, op, self.batch, self.da, self.ta, self.db if op in READS_B else None,
                              self.tb if op in READS_B else None, self.dsel if op in READS_SEL else None,
                              self.ts if op in READS_SEL else 0, outs=guarded.outs)
        torch.cuda.synchronize()
        guarded.check(want, (op, self.n, self.batch, self.ta, self.tb, self.ts))

    def check(self, knobs, ops=tuple(OPS.values()), forms=FORMS, shift=0):
        for form in forms:
            if form is None:
                knobs.unset("uint_bitwise_form")
            else:
                knobs.set("uint_bitwise_form", form)
                name = self.hip.lib.csgn_uint_bitwise_kernel(self.n, ops[0], self.batch, self.w, self.ts, u64s(self.ta), u64s(self.tb))
                assert name == (b"k_uint_bitwise" if form else b"planes"), (name, form)
            for op in ops:
                self.run(op, shift)


def operands(hip, n, batch, ta, tb, ts, seed=0, **kw):
    a = [rand_terms(n, batch, t, seed + 500 + 7 * k + t) for k, t in enumerate(ta)]
    b = None if tb is None else [rand_terms(n, batch, t, seed + 550 + 5 * k + t) for k, t in enumerate(tb)]
    sel = None if ts is None else rand_terms(n, batch, ts, seed + 590 + ts)
    return Operands(hip, n, a, b, sel, **kw)


# 64: one 8-byte unit a term; 1247: dL 20, 16-byte units; 1300: dL 21, 8-byte units
@pytest.mark.parametrize("n", [64, 1247, 1300])
@pytest.mark.parametrize("w", [1, 2, 3])
def test_bitwise_words(hip, knobs, n, w):
    """Fresh planes, and planes of 1, 2, 3 against 2, 1, 4 terms under selectors of 1, 2 and 3 terms: every op in every
    form."""
    operands(hip, n, 3, [1] * w, [1] * w, 1, seed=w).check(knobs)
    for ts in (1, 2, 3):
        operands(hip, n, 3, [1, 2, 3][:w], [2, 1, 4][:w], ts, seed=10 * ts + w).check(knobs)


@pytest.mark.parametrize("n", [64, 1247, 1300])
def test_bitwise_width_64(hip, knobs, n):
    """64 one-term planes: the whole argument table of the kernel."""
    operands(hip, n, 3, [1] * 64, [1] * 64, 1, seed=64).check(knobs)


@pytest.mark.parametrize("n", [64, 1247, 1300])
def test_bitwise_product_rows_longer_than_a_workgroup(hip, knobs, n):
    """One plane of 6 x 6 terms under a selector of 6: at N = 1247 a product is 360 units, a row set that no workgroup
    holds."""
    operands(hip, n, 3, [6], [6], 6, seed=6).check(knobs)


@pytest.mark.parametrize("n", [64, 1247])
@pytest.mark.parametrize("batch", [1, 3, 257])
def test_bitwise_batches(hip, knobs, n, batch):
    """At 257 elements the planes' lane ranges end inside a workgroup: the rounding to whole workgroups."""
    operands(hip, n, batch, [1, 2, 3], [2, 1, 4], 2, seed=batch).check(knobs)
    operands(hip, n, batch, [1] * 3, [1] * 3, 1, seed=batch + 1).check(knobs)


@pytest.mark.parametrize("n", [1247, 1300])
def test_bitwise_aliased_operands(hip, knobs, n):
    """b = a; b_j = a_{(j+1) mod w}, what a public rotate hands on; the selector plane 0 of a."""
    w = 3
    for b_from in (list(range(w)), [(j + 1) % w for j in range(w)]):
        operands(hip, n, 5, [1, 2, 3], None, None, seed=n % 100, b_from=b_from, sel_from=0).check(knobs)
        operands(hip, n, 5, [1] * w, None, 2, seed=n % 100 + 1, b_from=b_from).check(knobs)


def test_bitwise_views_at_odd_word_offsets(hip, knobs):
    """N = 1247 (dL 20): operands and outputs that start 8 bytes off a 16-byte boundary take the 8-byte units."""
    for op_shift, out_shift in ((1, 0), (0, 1), (1, 1)):
        operands(hip, 1247, 5, [1, 2, 3], [2, 1, 4], 2, seed=20, shift=op_shift).check(knobs, shift=out_shift)
        operands(hip, 1247, 5, [1] * 3, [1] * 3, 1, seed=21, shift=op_shift).check(knobs, shift=out_shift)


@pytest.mark.parametrize("n", [4096, 2100])
def test_bitwise_batch_split_over_launches(hip, knobs, n):
    """Knob launch_blocks lowers the workgroups of one launch, so the host cuts the 301 elements into several launches,
    each with its own operand and output offsets, the last one not full.  Every run equals the model."""
    ops = operands(hip, n, 301, [1, 2, 3], [2, 1, 4], 2, seed=n % 100)
    for blocks in (15, 16, 48, None):
        if blocks is None:
            knobs.unset("launch_blocks")
        else:
            knobs.set("launch_blocks", blocks)
        ops.check(knobs, ops=(SELECT,), forms=(1,))
    knobs.set("launch_blocks", 16)
    ops.check(knobs, forms=(1,))
