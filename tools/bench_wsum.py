"""Encrypted integers summed into encrypted integers on the device: csgn_wsum's kernel (k_wsum) against the mark --
csgn_mul_uniform alone writing an output of the same bytes (per plane one all-pairs multiply of t1 x t2 = T_j terms per
element, t1 the largest divisor of T_j up to its square root) -- and, on one-class shapes, against csgn_count's fused
kernel, which writes the same words; all on the same run's clock.  The inputs rotate over enough copies to pass the
256 MiB memory-side cache.  One JSON line per case: median microseconds of each from HIP events, the bytes written, the
written bytes per second and the ratios.

    python tools/bench_wsum.py [--reps 7] [--only INDEX] [--max-gb 40]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from csgn_amd import capi  # noqa: E402
from csgn_amd.batch import HipPath  # noqa: E402

ROTATE_BYTES = 512 << 20


def shapes():
    """(name, n, count, classes, t, planes)."""
    return [("sum of 8 x 4-bit", 1247, 4096, [8] * 4, 1, [0, 1, 2, 3]),
            ("sum of 4 x 3-bit", 1247, 1 << 16, [4] * 3, 1, [0, 1, 2, 3, 4]),
            ("low 8 planes of 8 x 8", 1247, 1024, list(range(1, 9)), 1, list(range(8))),
            ("one class of 64", 1247, 4096, [64], 1, [1])]


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
    for x, (name, n, count, ns, t, js) in enumerate(shapes()):
        if args.only >= 0 and x != args.only:
            continue
        dl = hip.default_len(n)
        handle = hip.wsum_create(ns, t, js)
        T = [int(lib.csgn_wsum_plan_terms(handle, k)) for k in range(len(js))]
        out_words = [count * Tj * dl for Tj in T]
        rec = {"shape": name, "n": n, "count": count, "classes": ns, "t": t, "planes": js, "terms": T,
               "out_gb": round(sum(out_words) * 8 / 1e9, 3)}
        if sum(out_words) * 8 > args.max_gb * 1e9:
            rec["skipped"] = "outputs past --max-gb"
            print(json.dumps(rec), flush=True)
            lib.csgn_wsum_destroy(handle)
            continue
        in_words = count * sum(ns) * t * dl
        copies = max(1, min(8, -(-ROTATE_BYTES // (in_words * 8))))
        X = [[hip.synth_fill(11 + 97 * c + k, n, 0, count * nk * t * dl) for k, nk in enumerate(ns)] for c in range(copies)]
        outs = [hip.empty_words(w) for w in out_words]
        nbytes = sum(out_words) * 8
        rec["wsum_us"] = round(timed(lambda r: hip.wsum_apply(handle, n, count, X[r % copies], len(js), outs), args.reps) * 1e6, 1)
        rec["wsum_tbps"] = round(nbytes / rec["wsum_us"] * 1e6 / 1e12, 3)
        lib.csgn_wsum_destroy(handle)
        if len(ns) == 1:                                         # csgn_count writes the same words
            summed = [o.clone() for o in outs]
            capi.set_tuning("count_form", 1)
            rec["count_us"] = round(timed(lambda r: hip.count(n, count, ns[0], t, [X[r % copies][0]], js, outs=outs), args.reps) * 1e6, 1)
            capi.set_tuning("count_form", -1)
            hip.count(n, count, ns[0], t, [X[0][0]], js, outs=outs)
            hip.wsum(n, count, ns, t, X[0], js, outs=summed)
            torch.cuda.synchronize()
            rec["count_same_words"] = all(bool(torch.equal(a, b)) for a, b in zip(summed, outs))
            rec["count_tbps"] = round(nbytes / rec["count_us"] * 1e6 / 1e12, 3)
            rec["wsum_vs_count"] = round(rec["count_us"] / rec["wsum_us"], 2)
            del summed
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
        rec["wsum_vs_mark"] = round(rec["mark_us"] / rec["wsum_us"], 2)
        print(json.dumps(rec), flush=True)
        del X, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
