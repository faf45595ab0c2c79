"""Encrypted bits counted into encrypted integers on the device: csgn_count's fused kernel (k_count) against the same
words from the composed form (knob count_form = 0: the factors tiled by the gather launcher, uniform multiplies), and
against the mark -- csgn_mul_uniform alone writing an output of the same bytes (per plane one all-pairs multiply of
t1 x t2 = T_j terms per element, t1 the largest divisor of T_j up to its square root), all on the same run's clock.  The
inputs rotate over enough copies to pass the 256 MiB memory-side cache.  One JSON line per case: median microseconds of
each form from HIP events, the bytes written, every form's written bytes per second and the ratios.

    python tools/bench_count.py [--reps 7] [--only INDEX] [--max-gb 40]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ctypes as C  # noqa: E402

import torch  # noqa: E402

from csgn_amd import capi  # noqa: E402
from csgn_amd.batch import HipPath  # noqa: E402

ROTATE_BYTES = 512 << 20


def shapes():
    """(n, count, group, t, planes)."""
    out = [(1247, count, g, 1, js) for g in (64, 32) for js in ((1,), (1, 2)) for count in (1, 256, 4096)]
    out += [(1247, count, 8, 3, (1, 2)) for count in (256, 4096)]
    out += [(4096, count, 64, 1, (1,)) for count in (1, 256, 4096)]
    return out


def timed(fn, reps):
    fn(0)
    torch.cuda.synchronize()
    ts = []
    for r in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(r + 1)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


def split(T):
    """T = t1 * t2 with t1 the largest divisor up to the square root."""
    t1 = int(T ** 0.5)
    while T % t1:
        t1 -= 1
    return t1, T // t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    ap.add_argument("--max-gb", type=float, default=40.0, help="skip shapes whose outputs are larger")
    args = ap.parse_args()
    hip = HipPath(0)
    lib = hip.lib
    for x, (n, count, g, t, js) in enumerate(shapes()):
        if args.only >= 0 and x != args.only:
            continue
        dl = hip.default_len(n)
        T = [int(lib.csgn_count_terms(g, t, j)) for j in js]
        out_words = [count * Tj * dl for Tj in T]
        rec = {"n": n, "count": count, "group": g, "t": t, "planes": list(js), "terms": T,
               "out_gb": round(sum(out_words) * 8 / 1e9, 3)}
        if sum(out_words) * 8 > args.max_gb * 1e9:
            rec["skipped"] = "outputs past --max-gb"
            print(json.dumps(rec), flush=True)
            continue
        in_words = count * g * t * dl
        copies = max(1, min(8, -(-ROTATE_BYTES // (in_words * 8))))
        X = [hip.synth_fill(11 + 97 * c, n, 0, in_words) for c in range(copies)]
        outs = [hip.empty_words(w) for w in out_words]
        nbytes = sum(out_words) * 8
        h_js = (C.c_uint64 * len(js))(*js)
        call = lambda r: hip.count(n, count, g, t, [X[r % copies]], js, outs=outs)  # noqa: E731
        fused = None
        for form, knob in (("fused", 1), ("composed", 0)):
            capi.set_tuning("count_form", knob)
            rec[form + "_kernel"] = lib.csgn_count_kernel(n, count, g, t, 1, len(js), h_js).decode()
            rec[form + "_us"] = round(timed(call, args.reps if knob else max(3, args.reps // 2)) * 1e6, 1)
            rec[form + "_tbps"] = round(nbytes / rec[form + "_us"] * 1e6 / 1e12, 3)
            call(0)
            torch.cuda.synchronize()
            if form == "fused":
                fused = [o.clone() for o in outs]
            else:
                rec["composed_same_words"] = all(bool(torch.equal(f, o)) for f, o in zip(fused, outs))
        capi.set_tuning("count_form", -1)
        rec["default_kernel"] = lib.csgn_count_kernel(n, count, g, t, 1, len(js), h_js).decode()
        del fused
        # the mark: the uniform multiply writing the same bytes, plane by plane
        mark = 0.0
        for Tj, o in zip(T, outs):
            t1, t2 = split(Tj)
            L = [hip.synth_fill(17 + 5 * c, n, 0, count * t1 * dl) for c in range(copies)]
            R = [hip.synth_fill(19 + 7 * c, n, 0, count * t2 * dl) for c in range(copies)]
            mark += timed(lambda r: hip.mul_uniform(n, count, t1, t2, L[r % copies], R[r % copies], out=o), args.reps)
            del L, R
        rec["mark_us"] = round(mark * 1e6, 1)
        rec["mark_tbps"] = round(nbytes / rec["mark_us"] * 1e6 / 1e12, 3)
        rec["fused_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
        rec["fused_vs_mark"] = round(rec["mark_us"] / rec["fused_us"], 2)
        print(json.dumps(rec), flush=True)
        del X, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
