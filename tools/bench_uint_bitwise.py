"""a & b, a | b, a ^ b, ~a, select and keepWhere of encrypted integers on the device: csgn_uint_bitwise's one kernel
(k_uint_bitwise, knob uint_bitwise_form = 1) against one call per plane of the entry points the class operators issued
before -- csgn_mul_uniform (AND, KEEP), csgn_add_uniform (XOR), csgn_gate_uniform (OR, NOT, MUX) -- which this
operation does not touch.  Every op at widths 8, 32 and 64, on fresh 1-term planes and on the planes of an 8-bit a + b
(2, 3, 5, 9, 17, 33, 65 and 129 terms, repeated over the width), SELECT and KEEP also under the 6560-term selector of an
8-bit lessThan, each at one small batch (about 1 MB of outputs: the per-plane calls are launch-bound) and at one whose
outputs pass the 256 MiB memory-side cache (about 1 GB).  The operands rotate over several copies.  The two are timed
in turns in the same run (HIP events, medians); both are issued from this process on host arrays built beforehand.  One
JSON line per case: microseconds and WRITTEN bytes per second of each, whether the words agree, the form this run shows
to be no slower -- the kernel where it takes at most 1.05 times the per-plane time (an allowance of 5 % for the spread
between machines; a form within it counts as level), else the planes -- the form the per-shape default names, and
whether that default keeps the rule: the kernel only where it is no slower (the planes are always allowed).

    python tools/bench_uint_bitwise.py [--n 1247] [--reps 20] [--only I]
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

OPS = {"and": 1, "or": 2, "xor": 3, "not": 4, "select": 5, "keep": 6}
GATE_NOT, GATE_OR, GATE_MUX = 1, 4, 6
SMALL_BYTES, LARGE_BYTES = 1 << 20, 1 << 30
ROTATE = 4
MARGIN = 1.05
SUM_PLANES = (2, 3, 5, 9, 17, 33, 65, 129)          # the planes of a + b at 8 bits
LESS_THAN_8 = 6560                                   # terms of an 8-bit lessThan of fresh planes
MAX_CASE_BYTES = 6 << 30


def shapes():
    """(op name, width, plane kind, selector terms)"""
    out = []
    for name in OPS:
        for w in (8, 32, 64):
            for kind in ("fresh", "sum"):
                out.append((name, w, kind, 1))
                if name in ("select", "keep"):
                    out.append((name, w, kind, LESS_THAN_8))
    return [s + (size,) for s in out for size in ("small", "large")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    vp = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])     # noqa: E731

    for i, (name, w, kind, ts, size) in enumerate(shapes()):
        if args.only >= 0 and i != args.only:
            continue
        op = OPS[name]
        with_b, with_sel = op in (1, 2, 3, 5), op in (5, 6)
        ta = [1] * w if kind == "fresh" else [SUM_PLANES[j % 8] for j in range(w)]
        tb = ta if with_b else [0] * w
        T = [int(lib.csgn_uint_bitwise_terms(op, ts, ta[j], tb[j])) for j in range(w)]
        per_element = sum(T) * dl * 8
        m = max(1, (SMALL_BYTES if size == "small" else LARGE_BYTES) // per_element)
        out_bytes = m * per_element
        rec = {"op": name, "w": w, "planes": kind, "sel_terms": ts if with_sel else 0, "m": m, "batch": size, "n": n,
               "terms": sum(T), "written_bytes": out_bytes}
        if out_bytes > MAX_CASE_BYTES:
            rec["skipped"] = "one element of all planes passes %d GiB" % (MAX_CASE_BYTES >> 30)
            print(json.dumps(rec), flush=True)
            continue
        h_ta, h_tb = (C.c_uint64 * w)(*ta), (C.c_uint64 * w)(*tb)
        outs = [hip.empty_words(m * t * dl) for t in T]
        h_out = vp(outs)
        sets = []
        for c in range(ROTATE):
            a = [hip.synth_fill(11 + 97 * c + j, n, 0, m * ta[j] * dl) for j in range(w)]
            b = [hip.synth_fill(5011 + 97 * c + j, n, 0, m * tb[j] * dl) for j in range(w)] if with_b else []
            s = hip.synth_fill(9001 + c, n, 0, m * ts * dl) if with_sel else None
            sets.append((a, b, s, vp(a), vp(b) if with_b else None))
        st = hip.stream

        def kernel(r):
            a, b, s, h_a, h_b = sets[r % ROTATE]
            capi.check(lib.csgn_uint_bitwise(n, op, m, w, s.data_ptr() if with_sel else None, ts, h_a, h_ta, h_b,
                                             h_tb if with_b else None, h_out, st))

        def planes(r):
            a, b, s, _, _ = sets[r % ROTATE]
            for j in range(w):
                A, o = a[j].data_ptr(), outs[j].data_ptr()
                if name == "and":
                    rc = lib.csgn_mul_uniform(n, m, ta[j], tb[j], A, b[j].data_ptr(), o, 0, st)
                elif name == "xor":
                    rc = lib.csgn_add_uniform(n, m, ta[j], tb[j], A, b[j].data_ptr(), o, st)
                elif name == "or":
                    rc = lib.csgn_gate_uniform(n, GATE_OR, m, 0, ta[j], tb[j], None, A, b[j].data_ptr(), None, o, st)
                elif name == "not":
                    rc = lib.csgn_gate_uniform(n, GATE_NOT, m, 0, ta[j], 0, None, A, None, None, o, st)
                elif name == "select":
                    rc = lib.csgn_gate_uniform(n, GATE_MUX, m, ts, ta[j], tb[j], s.data_ptr(), A, b[j].data_ptr(), None, o, st)
                else:
                    rc = lib.csgn_mul_uniform(n, m, ts, ta[j], s.data_ptr(), A, o, 0, st)
                capi.check(rc)

        capi.check(lib.csgn_set_tuning(b"uint_bitwise_form", 1))
        rec["kernel_form"] = lib.csgn_uint_bitwise_kernel(n, op, m, w, ts, h_ta, h_tb).decode()
        forms = (("kernel", kernel), ("planes", planes))
        words = {}
        for form, call in forms:                      # warm-up of both, and their words on the same operands
            call(0)
            torch.cuda.synchronize()
            words[form] = [o.clone() for o in outs] if out_bytes <= (2 << 30) else None
        if words["kernel"] is not None:
            rec["same_words"] = all(torch.equal(x, y) for x, y in zip(words["kernel"], words["planes"]))
        del words
        times = {"kernel": [], "planes": []}
        for r in range(args.reps):                    # in turns, so that a drift of the machine meets both
            for form, call in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(r + 1)
                e1.record()
                e1.synchronize()
                times[form].append(e0.elapsed_time(e1) * 1e-3)
        for form, _ in forms:
            t = sorted(times[form])
            rec[form + "_us"] = round(t[len(t) // 2] * 1e6, 1)
            rec[form + "_min_us"] = round(t[0] * 1e6, 1)
            rec[form + "_written_tbps"] = round(out_bytes / t[len(t) // 2] * 1e-12, 3)
        rec["speedup"] = round(rec["planes_us"] / rec["kernel_us"], 2)
        rec["no_slower"] = "k_uint_bitwise" if rec["kernel_us"] <= MARGIN * rec["planes_us"] else "planes"
        capi.check(lib.csgn_set_tuning(b"uint_bitwise_form", -1))
        rec["default_form"] = lib.csgn_uint_bitwise_kernel(n, op, m, w, ts, h_ta, h_tb).decode()
        # the rule of DESIGN 4.31: the kernel by default only where it is no slower; the planes are always allowed
        rec["default_within_rule"] = rec["default_form"] == "planes" or rec["no_slower"] == "k_uint_bitwise"
        print(json.dumps(rec), flush=True)
        del outs, sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
