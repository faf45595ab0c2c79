"""Shifts, rotates and per-element reads by encrypted amounts on the device: csgn_uint_pick's fused kernel (k_uint_pick)
-- as dispatched ("fused": a workgroup's value slice staged in LDS where it fits) and with plain global loads of the value
units ("plain", knob uint_pick_stage = 0) -- against the same words composed row by row from the tuned launchers (knob
uint_pick_fused = 0), and against an emulation of the loop a user writes at the class level today -- out_j = sum over r of equalTo(d, r) * source, one
csgn_uint_plain per row (and, for readAtEach, one gather), and per plane one multiply and one add (a copy of the whole
running sum) per row.  The index planes and the operands rotate over enough copies to pass the 256 MiB memory-side cache.
The words of every timed form are compared with the fused form's before anything is printed.  One JSON line per case:
median microseconds of each form from HIP events (a sample is four calls queued back to back between two events, their
argument arrays built beforehand: timed()), the algorithmic bytes (outputs written once + index and source planes read
once) and the fused form's share of 8 TB/s.

    python tools/bench_uint_pick.py [--n 1247] [--reps 10] [--only K]
    python tools/bench_uint_pick.py --ab-rounds 4                     # fused kernel only: plain and staged value units in turn
    python tools/bench_uint_pick.py --only 0 --fused-calls 20         # nothing but 20 plain and 20 staged calls (kernel trace)
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
ROTATE_BYTES = 512 << 20
SHL, SHR, ROTL, ROTR, EACH = range(1, 6)
NAMES = {SHL: "SHL", SHR: "SHR", ROTL: "ROTL", ROTR: "ROTR", EACH: "EACH"}


def shapes():
    """(op, width w, index width v, rows n of an element's array, elements m), fresh 1-term planes."""
    return [(SHL, 8, 3, 0, 1 << 16), (ROTL, 32, 5, 0, 1 << 12), (SHR, 64, 6, 0, 512), (ROTL, 8, 3, 0, 1 << 16),
            (EACH, 8, 4, 16, 1 << 14)]


def rows_of(op, v, w, n, j):
    return {SHL: min(j + 1, 1 << v), SHR: min(w - j, 1 << v), ROTL: 1 << v, ROTR: 1 << v, EACH: n}[op]


def src_of(op, w, j, r):
    return {SHL: j - r, SHR: j + r, ROTL: (j - r) % w, ROTR: (j + r) % w, EACH: j}[op]


def timed(fn, reps, inner=4):
    """Median of `reps` samples; a sample is `inner` calls queued back to back between two HIP events, divided by
    `inner`, so that the host's work for a call (the launch itself included) overlaps the call before it instead of
    being timed with an idle GPU.  fn(i) takes a running call number, which the callers turn into the operand copy."""
    for i in range(3):                                  # steady state: the first calls of a form run slower
        fn(i)
    torch.cuda.synchronize()
    ts, i = [], 3
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn(i)
            i += 1
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / inner)
    ts.sort()
    return ts[len(ts) // 2]


def prepared(hip, n_bits, op, m, v, w, n, sets, srcs, outs):
    """call(i): one csgn_uint_pick on copy i mod copies, its argument arrays built beforehand -- the timed region holds
    the C call and nothing else (HipPath.uint_pick would add w + 4 ctypes conversions per call)."""
    vp = C.c_void_p
    h_s = (C.c_uint64 * v)(*([1] * v))
    h_out = (vp * w)(*[o.data_ptr() for o in outs])
    args = [((vp * v)(*[p.data_ptr() for p in x]), (vp * w)(*[p.data_ptr() for p in a])) for x, a in zip(sets, srcs)]
    lib, stream = hip.lib, hip.stream

    def call(i):
        h_x, h_a = args[i % len(args)]
        capi.check(lib.csgn_uint_pick(n_bits, op, m, v, h_x, h_s, w, n, h_a, 1, h_out, stream))
    return call


def today(hip, n_bits, m, op, v, w, n, index, a, lists):
    """The class-level loop: the running sum of every plane, one add (a fresh copy) per row."""
    dl = hip.default_len(n_bits)
    acc, tacc = [None] * w, [0] * w
    for r in range(max(rows_of(op, v, w, n, j) for j in range(w))):
        eq = hip.uint_plain(n_bits, capi.CSGN_UINT_PLAIN_EQ, m, index, [1] * v, r)
        te = eq.numel() // (m * dl)
        row = hip.gather_planes(n_bits, a, [1] * w, m * n, m, lists[r]) if op == EACH else None
        for j in range(w):
            if r >= rows_of(op, v, w, n, j):
                continue
            p = hip.mul_uniform(n_bits, m, te, 1, eq, row[j] if op == EACH else a[src_of(op, w, j, r)])
            acc[j] = p if acc[j] is None else hip.add_uniform(n_bits, m, tacc[j], te, acc[j], p)
            tacc[j] += te
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="the one shape to run (its position in the list)")
    ap.add_argument("--ab-rounds", type=int, default=0,
                    help="time nothing but the fused kernel, plain and staged in turn, this many rounds")
    ap.add_argument("--fused-calls", type=int, default=0,
                    help="run nothing but this many plain and this many staged fused calls (for a kernel trace)")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n_bits = hip.lib, args.n
    dl = hip.default_len(n_bits)
    for k, (op, w, v, n, m) in enumerate(shapes()):
        if args.only >= 0 and k != args.only:
            continue
        s = (C.c_uint64 * v)(*([1] * v))
        E = [int(lib.csgn_uint_pick_terms(op, v, s, w, n, j)) for j in range(w)]
        per = n if op == EACH else 1
        in_bytes = (v * m + w * m * per) * dl * 8
        copies = max(1, -(-ROTATE_BYTES // in_bytes))
        sets = [[hip.synth_fill(11 + 97 * c + i, n_bits, 0, m * dl) for i in range(v)] for c in range(copies)]
        srcs = [[hip.synth_fill(7 + 89 * c + 31 * j, n_bits, 0, m * per * dl) for j in range(w)] for c in range(copies)]
        lists = [torch.arange(m, dtype=torch.int64, device="cuda") * n + r for r in range(n)] if op == EACH else None
        outs = [hip.empty_words(m * e * dl) for e in E]
        out_bytes = m * sum(E) * dl * 8
        nbytes = out_bytes + in_bytes
        rec = {"op": NAMES[op], "w": w, "v": v, "rows": n, "m": m, "n": n_bits, "E_max": max(E), "E_sum": sum(E),
               "copies": copies, "out_gb": round(out_bytes / 1e9, 3), "bytes": nbytes}
        call = prepared(hip, n_bits, op, m, v, w, n, sets, srcs, outs)
        if args.fused_calls or args.ab_rounds:
            capi.check(lib.csgn_set_tuning(b"uint_pick_fused", 1))
            for name, stage in (("plain", 0), ("staged", 1)):
                rec[name + "_us"] = []
            for _ in range(max(1, args.ab_rounds)):
                for name, stage in (("plain", 0), ("staged", 1)):
                    capi.check(lib.csgn_set_tuning(b"uint_pick_stage", stage))
                    if args.fused_calls:
                        for i in range(args.fused_calls):
                            call(i)
                        torch.cuda.synchronize()
                    else:
                        rec[name + "_us"].append(round(timed(call, args.reps) * 1e6, 1))
            if args.fused_calls:
                rec = {"op": NAMES[op], "w": w, "v": v, "m": m, "fused_calls_each": args.fused_calls}
            print(json.dumps(rec), flush=True)
            del sets, srcs, outs
            torch.cuda.empty_cache()
            continue
        words = {}
        for form, knob, stage in (("fused", 1, -1), ("plain", 1, 0), ("composed", 0, -1)):
            capi.check(lib.csgn_set_tuning(b"uint_pick_fused", knob))
            capi.check(lib.csgn_set_tuning(b"uint_pick_stage", stage))
            rec[form + "_kernel"] = lib.csgn_uint_pick_kernel(n_bits, op, m, v, s, w, n, 1).decode()
            rec[form + "_us"] = round(timed(call, args.reps) * 1e6, 1)
            call(0)
            torch.cuda.synchronize()
            words[form] = [o.clone() for o in outs] if form != "composed" else outs
        capi.check(lib.csgn_set_tuning(b"uint_pick_fused", -1))
        rec["plain_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], words.pop("plain")))
        rec["default_kernel"] = lib.csgn_uint_pick_kernel(n_bits, op, m, v, s, w, n, 1).decode()
        rec["composed_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], words["composed"]))
        rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
        rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
        rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
        del outs, call
        words.pop("composed")
        torch.cuda.empty_cache()
        got = today(hip, n_bits, m, op, v, w, n, sets[0], srcs[0], lists)
        torch.cuda.synchronize()
        rec["today_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], got))
        del got
        fn = lambda r: today(hip, n_bits, m, op, v, w, n, sets[r % copies], srcs[r % copies], lists)  # noqa: E731
        rec["today_us"] = round(timed(fn, max(3, args.reps // 3), inner=1) * 1e6, 1)
        rec["speedup_vs_today"] = round(rec["today_us"] / rec["fused_us"], 2)
        print(json.dumps(rec), flush=True)
        assert rec["composed_same_words"] and rec["plain_same_words"] and rec["today_same_words"], \
            "a timed form's words differ from the fused form's"
        del sets, srcs, words
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
