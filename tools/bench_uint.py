"""Bit-sliced integer steps on the device: csgn_uint_step against the same step composed from the existing entry points
(csgn_gate_uniform / csgn_add_uniform / csgn_mul_uniform / csgn_const_fill, one intermediate buffer per step), and the
whole 4- and 8-bit operations against their Gates.h compositions.  One JSON line per case: median time of each form
from HIP events, the algorithmic bytes (operands read once + outputs written once) and the step's share of 8 TB/s.

    python tools/bench_uint.py [--n 1247] [--batch 1048576] [--reps 20] [--sweep]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from csgn_amd import capi  # noqa: E402
from csgn_amd.batch import HipPath  # noqa: E402

PEAK = 8e12
ADD_HALF, ADD_FULL, EQ_STEP, LT_FIRST, LT_STEP = (capi.CSGN_UINT_ADD_HALF, capi.CSGN_UINT_ADD_FULL,
                                                  capi.CSGN_UINT_EQ_STEP, capi.CSGN_UINT_LT_FIRST, capi.CSGN_UINT_LT_STEP)
NAMES = {ADD_HALF: "add_half", ADD_FULL: "add_full", EQ_STEP: "eq_step", LT_FIRST: "lt_first", LT_STEP: "lt_step"}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


class Composed:
    """The definitions through the existing entry points, one buffer per intermediate."""

    def __init__(self, hip, n, batch):
        self.hip, self.n, self.batch = hip, n, batch

    def add(self, x, tx, y, ty):
        return self.hip.add_uniform(self.n, self.batch, tx, ty, x, y)

    def mul(self, x, tx, y, ty):
        return self.hip.mul_uniform(self.n, self.batch, tx, ty, x, y)

    def gate(self, g, a, ta, b=None, tb=0, s=None, ts=0):
        return self.hip.gate_uniform(self.n, g, self.batch, a, ta, b, tb, s, ts)

    def step(self, st, x, tx, a, ta, b, tb, carry=True):
        if st == ADD_HALF:
            return (self.add(a, ta, b, tb), self.mul(a, ta, b, tb)) if carry else (self.add(a, ta, b, tb),)
        if st == ADD_FULL:
            ab = self.add(a, ta, b, tb)
            s = self.add(ab, ta + tb, x, tx)
            if not carry:
                return (s,)
            return s, self.add(self.mul(a, ta, b, tb), ta * tb, self.mul(ab, ta + tb, x, tx), (ta + tb) * tx)
        if st == EQ_STEP:
            return (self.mul(x, tx, self.gate(capi.CSGN_GATE_XNOR, a, ta, b, tb), ta + tb + 1),)
        if st == LT_FIRST:
            return (self.mul(self.gate(capi.CSGN_GATE_NOT, a, ta), ta + 1, b, tb),)
        return (self.add(self.mul(self.add(a, ta, b, tb), ta + tb, self.add(b, tb, x, tx), tb + tx),
                         (ta + tb) * (tb + tx), x, tx),)


def step_case(hip, n, st, batch, tx, ta, tb, reps, fused):
    dl = hip.default_len(n)
    reads_x = st not in (ADD_HALF, LT_FIRST)
    tx = tx if reads_x else 0
    words = lambda t: hip.empty_words(max(batch * t * dl, 1)).random_()
    x, a, b = words(tx), words(ta), words(tb)
    comp = Composed(hip, n, batch)
    capi.set_tuning("uint_fused", fused)
    kernel = hip.lib.csgn_uint_step_kernel(n, st, batch, tx, ta, tb).decode()
    t_step = timed(lambda: hip.uint_step(n, st, batch, a, ta, b, tb, x if reads_x else None, tx), reps)
    capi.set_tuning("uint_fused", -1)
    t_comp = timed(lambda: comp.step(st, x, tx, a, ta, b, tb), reps)
    out_terms = sum(int(hip.lib.csgn_uint_step_terms(st, o, tx, ta, tb)) for o in (0, 1))
    nbytes = batch * (tx + ta + tb + out_terms) * dl * 8
    return {"step": NAMES[st], "n": n, "batch": batch, "shape": [tx, ta, tb], "kernel": kernel, "forced": fused,
            "step_s": t_step, "composed_s": t_comp, "speedup": t_comp / t_step, "bytes": nbytes,
            "step_tbps": nbytes / t_step / 1e12, "frac_of_8tbps": nbytes / t_step / PEAK}


# -- whole operations: chains of steps (fused) or of the Gates.h compositions --------------------------------------------
def whole(hip, n, batch, w, op, fused_path):
    """Planes of fresh 1-term values; returns a closure running `op` ("add", "sub", "eq", "lt") once."""
    dl = hip.default_len(n)
    a = [hip.empty_words(batch * dl).random_() for _ in range(w)]
    b = [hip.empty_words(batch * dl).random_() for _ in range(w)]
    one = hip.const_fill(n, batch, None, 1)
    comp = Composed(hip, n, batch)
    run = (lambda st, x, tx, aa, ta, bb, tb, carry=True: hip.uint_step(n, st, batch, aa, ta, bb, tb, x, tx, carry)) \
        if fused_path else comp.step
    gate = lambda g, x, tx, y=None, ty=0: hip.gate_uniform(n, g, batch, x, tx, y, ty)
    as_tuple = lambda r: r if isinstance(r, tuple) else (r,)

    def go():
        if op in ("add", "sub"):
            c, tc = (one, 1) if op == "sub" else (None, 0)
            for j in range(w):
                bj, tbj = (gate(capi.CSGN_GATE_NOT, b[j], 1), 2) if op == "sub" else (b[j], 1)
                last = j == w - 1
                if c is None:
                    r = as_tuple(run(ADD_HALF, None, 0, a[j], 1, bj, tbj, not last))
                    c, tc = (r[1], tbj) if not last else (None, 0)
                else:
                    r = as_tuple(run(ADD_FULL, c, tc, a[j], 1, bj, tbj, not last))
                    if not last:
                        c, tc = r[1], tbj + (1 + tbj) * tc
        elif op == "eq":
            e, te = gate(capi.CSGN_GATE_XNOR, a[0], 1, b[0], 1), 3
            for j in range(1, w):
                e, te = as_tuple(run(EQ_STEP, e, te, a[j], 1, b[j], 1))[0], te * 3
        else:
            lt, tl = as_tuple(run(LT_FIRST, None, 0, a[0], 1, b[0], 1))[0], 2
            for j in range(1, w):
                lt, tl = as_tuple(run(LT_STEP, lt, tl, a[j], 1, b[j], 1))[0], 2 * (1 + tl) + tl
    return go


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="also both forms (uint_fused 0 / 1) over the carries past the cut")
    ap.add_argument("--no-whole", action="store_true", help="skip the whole 4- and 8-bit operations")
    args = ap.parse_args()
    hip = HipPath(0)
    emit = lambda r: print(json.dumps(r), flush=True)
    for st in NAMES:                                                   # fresh operands, short accumulators
        for tx in ((1, 3) if st not in (ADD_HALF, LT_FIRST) else (1,)):
            emit(step_case(hip, args.n, st, args.batch, tx, 1, 1, args.reps, -1))
    for st, tx, ta, tb, batch in ((ADD_FULL, 127, 1, 1, 16384), (LT_STEP, 127, 1, 1, 16384), (ADD_HALF, 0, 16, 16, 16384),
                                  (EQ_STEP, 1, 40, 40, 16384), (LT_FIRST, 0, 64, 1, 16384)):   # the pitched region
        emit(step_case(hip, args.n, st, batch, tx, ta, tb, args.reps, -1))
    for st, tx, batch in ((EQ_STEP, 27, 65536), (LT_STEP, 26, 65536)):  # interleaved rows: always fused
        emit(step_case(hip, args.n, st, batch, tx, 2 if st == LT_STEP else 1, 1, args.reps, -1))
    if args.sweep:
        for st, txs in ((ADD_FULL, (7, 15, 31, 63, 127)), (LT_STEP, (8, 15, 26, 31, 80))):
            for tx in txs:
                batch = max(4096, (1 << 24) // (4 * tx))
                for fused in (0, 1):
                    emit(step_case(hip, args.n, st, batch, tx, 1, 1, args.reps, fused))
    if not args.no_whole:
        for w, batch in ((4, 65536), (8, 4096)):
            for op in ("add", "sub", "eq", "lt"):
                t_f = timed(whole(hip, args.n, batch, w, op, True), args.reps)
                t_c = timed(whole(hip, args.n, batch, w, op, False), args.reps)
                emit({"whole": op, "width": w, "n": args.n, "batch": batch, "steps_s": t_f, "composed_s": t_c,
                      "speedup": t_c / t_f})
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
