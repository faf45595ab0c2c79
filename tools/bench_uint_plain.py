"""Comparisons against a public constant on the device: csgn_uint_plain's fused kernel (k_uint_plain) against the same
words composed level by level from the tuned launchers (knob uint_plain_fused = 0), and against today's route -- the
constant trivially encrypted (UIntBatch::constant) and compared with csgn_gate_uniform XNOR + csgn_uint_step.  One JSON
line per case: median microseconds of each form from HIP events, the algorithmic bytes (output written once + planes
read once) and the fused form's share of 8 TB/s.

    python tools/bench_uint_plain.py [--n 1247] [--reps 10] [--today-max-gb 4]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from csgn_amd import capi  # noqa: E402
from csgn_amd.batch import HipPath  # noqa: E402

PEAK = 8e12
NAMES = {capi.CSGN_UINT_PLAIN_EQ: "eq", capi.CSGN_UINT_PLAIN_NE: "ne", capi.CSGN_UINT_PLAIN_LT: "lt",
         capi.CSGN_UINT_PLAIN_LE: "le", capi.CSGN_UINT_PLAIN_GT: "gt", capi.CSGN_UINT_PLAIN_GE: "ge"}
# (width, k, batches)
SHAPES = [(4, 5, (1 << 16, 1 << 18, 1 << 20)), (8, 100, (1 << 16, 1 << 18, 1 << 20)), (12, 2718, (1024,)),
          (16, 4711, (1024,))]


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


def set_knob(lib, value):
    capi.check(lib.csgn_set_tuning(b"uint_plain_fused", value))


def today(hip, n, batch, w, k, planes, cmp):
    """equalTo / lessThan(a, constant(k)) as UIntBatch does it today: the constant's planes are trivial encryptions."""
    dl = hip.default_len(n)
    const = []
    for j in range(w):
        c = hip.empty_words(batch * dl)
        capi.check(hip.lib.csgn_const_fill(n, batch, None, (k >> j) & 1, c.data_ptr(), hip.stream))
        const.append(c)
    if cmp == capi.CSGN_UINT_PLAIN_EQ:
        e, te = hip.gate_uniform(n, capi.CSGN_GATE_XNOR, batch, planes[0], 1, const[0], 1), 3
        for j in range(1, w):
            e, te = hip.uint_step(n, capi.CSGN_UINT_EQ_STEP, batch, planes[j], 1, const[j], 1, e, te), te * 3
        return te
    lt, tl = hip.uint_step(n, capi.CSGN_UINT_LT_FIRST, batch, planes[0], 1, const[0], 1), 2
    for j in range(1, w):
        lt, tl = hip.uint_step(n, capi.CSGN_UINT_LT_STEP, batch, planes[j], 1, const[j], 1, lt, tl), 2 * (1 + tl) + tl
    return tl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--today-max-gb", type=float, default=4.0)
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    for w, k, batches in SHAPES:
        for batch in batches:
            planes = [hip.synth_fill(11 + j, n, 0, batch * dl) for j in range(w)]
            for cmp in (capi.CSGN_UINT_PLAIN_EQ, capi.CSGN_UINT_PLAIN_LT, capi.CSGN_UINT_PLAIN_GT,
                        capi.CSGN_UINT_PLAIN_GE):
                terms = int(lib.csgn_uint_plain_terms(cmp, w, k, (C.c_uint64 * w)(*([1] * w))))
                nbytes = batch * (terms + w) * dl * 8
                rec = {"cmp": NAMES[cmp], "w": w, "k": k, "batch": batch, "n": n, "terms": terms, "bytes": nbytes}
                out = {}
                for form, knob in (("fused", 1), ("composed", 0)):
                    set_knob(lib, knob)
                    fn = lambda: out.__setitem__(form, hip.uint_plain(n, cmp, batch, planes, [1] * w, k))  # noqa: E731
                    rec[form + "_us"] = round(timed(fn, args.reps) * 1e6, 1)
                    rec[form + "_kernel"] = lib.csgn_uint_plain_kernel(n, cmp, batch, w, k,
                                                                       (C.c_uint64 * w)(*([1] * w))).decode()
                set_knob(lib, -1)
                assert torch.equal(out["fused"], out["composed"])
                del out
                rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
                rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
                rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
                if cmp in (capi.CSGN_UINT_PLAIN_EQ, capi.CSGN_UINT_PLAIN_LT):
                    tt = 3 ** w if cmp == capi.CSGN_UINT_PLAIN_EQ else 3 ** w - 1
                    rec["today_terms"] = tt
                    if batch * tt * dl * 8 * 2 <= args.today_max_gb * 1e9:
                        rec["today_us"] = round(timed(lambda: today(hip, n, batch, w, k, planes, cmp), args.reps) * 1e6, 1)
                        rec["speedup_vs_today"] = round(rec["today_us"] / rec["fused_us"], 2)
                    else:
                        rec["today_us"] = "not measured (output too large)"
                print(json.dumps(rec), flush=True)
                torch.cuda.empty_cache()
            del planes
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
