"""Encrypted tables looked up by encrypted key on the device: csgn_uint_find's fused kernel (k_uint_find) against the same
words composed row by row from the tuned launchers (knob uint_find_form = 0), and against an emulation of today's
route, the loop a user of the classes writes without readWhere -- per row the broadcast of the key and value row,
equalTo (the XNOR gate and one EQ_STEP per further plane), and per plane one multiply and one add (a copy of the whole
running sum) -- where it fits.  The emulation issues that launcher sequence through the Python wrappers: it has none
of the classes' own overhead and no block cache, and is not the C++ loop itself.  The query planes rotate over enough
copies to pass the 256 MiB memory-side cache.  One JSON line per case: median microseconds of each form from HIP
events, P, the algorithmic bytes (outputs written once + key, query and value planes read once) and the fused form's
share of 8 TB/s.

    python tools/bench_uint_find.py [--n 1247] [--reps 10] [--today-max-gb 3000] [--composed-max-launches 20000]
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


def shapes():
    """(key width v, rows, value width w, query elements m), fresh 1-term planes."""
    return [(4, 16, 8, 1 << 16), (8, 16, 8, 256), (8, 256, 1, 64), (2, 1024, 8, 4096)]


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


def today(hip, n, m, v, rows, w, query, keys, values):
    """Today's route, emulated: the launches of the class-level loop, the running sum of every plane re-copied by one
    add per row."""
    dl = hip.default_len(n)
    acc, tacc = [None] * w, 0
    for r in range(rows):
        krow = hip.gather_planes(n, [p[r * dl:(r + 1) * dl] for p in keys], [1] * v, 1, m)
        vrow = hip.gather_planes(n, [p[r * dl:(r + 1) * dl] for p in values], [1] * w, 1, m)
        eq, te = hip.gate_uniform(n, capi.CSGN_GATE_XNOR, m, krow[0], 1, query[0], 1), 3
        for k in range(1, v):
            eq = hip.uint_step(n, capi.CSGN_UINT_EQ_STEP, m, krow[k], 1, query[k], 1, x=eq, t_x=te)
            te *= 3
        for j in range(w):
            p = hip.mul_uniform(n, m, te, 1, eq, vrow[j])
            acc[j] = p if acc[j] is None else hip.add_uniform(n, m, tacc, te, acc[j], p)
        tacc += te
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--today-max-gb", type=float, default=3000.0, help="GB of copies today's route makes, at most")
    ap.add_argument("--composed-max-launches", type=int, default=20000)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    for i, (v, rows, w, m) in enumerate(shapes()):
        if args.only >= 0 and i != args.only:
            continue
        one = (C.c_uint64 * v)(*([1] * v))
        t = (C.c_uint64 * w)(*([1] * w))
        P = int(lib.csgn_uint_find_terms(v, one, one))
        E = rows * P
        plane_bytes = v * m * dl * 8
        copies = max(1, min(8, -(-ROTATE_BYTES // plane_bytes)))
        sets = [[hip.synth_fill(11 + 97 * c + k, n, 0, m * dl) for k in range(v)] for c in range(copies)]
        keys = [hip.synth_fill(5 + 13 * k, n, 0, rows * dl) for k in range(v)]
        values = [hip.synth_fill(7 + 31 * j, n, 0, rows * dl) for j in range(w)]
        outs = [hip.empty_words(m * E * dl) for _ in range(w)]
        out_bytes = w * m * E * dl * 8
        nbytes = out_bytes + (v * m + (v + w) * rows) * dl * 8
        rec = {"v": v, "rows": rows, "w": w, "m": m, "n": n, "P": P, "out_gb": round(out_bytes / 1e9, 3),
               "bytes": nbytes}
        words = {}
        launches = rows * (v + w + 3)
        call = lambda r: hip.uint_find(n, m, sets[r % copies], [1] * v, rows, keys, [1] * v, values, [1] * w, outs)  # noqa: E731
        for form, knob in (("fused", 1), ("composed", 0)):
            if knob == 0 and launches > args.composed_max_launches:
                rec["composed_us"] = f"not measured ({launches} launches)"
                continue
            capi.check(lib.csgn_set_tuning(b"uint_find_form", knob))
            rec[form + "_kernel"] = lib.csgn_uint_find_kernel(n, m, v, one, one, rows, w, t, 0).decode()
            rec[form + "_us"] = round(timed(call, args.reps if knob else max(3, args.reps // 3)) * 1e6, 1)
            call(0)
            torch.cuda.synchronize()
            words[form] = [o.clone() for o in outs] if form == "fused" and 3 * out_bytes < torch.cuda.mem_get_info()[0] else None
            if form == "composed" and words.get("fused"):
                rec["composed_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], outs))
        capi.check(lib.csgn_set_tuning(b"uint_find_form", -1))
        rec["default_kernel"] = lib.csgn_uint_find_kernel(n, m, v, one, one, rows, w, t, 0).decode()
        rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
        rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
        if isinstance(rec.get("composed_us"), float):
            rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
        copied = out_bytes * rows / 2
        del outs
        torch.cuda.empty_cache()
        if copied <= args.today_max_gb * 1e9 and 3 * out_bytes < torch.cuda.mem_get_info()[0] and words.get("fused"):
            got = today(hip, n, m, v, rows, w, sets[0], keys, values)
            torch.cuda.synchronize()
            rec["today_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], got))
            del got
            rec["today_us"] = round(timed(lambda r: today(hip, n, m, v, rows, w, sets[r % copies], keys, values),
                                          max(3, args.reps // 3)) * 1e6, 1)
            rec["speedup_vs_today"] = round(rec["today_us"] / rec["fused_us"], 2)
        else:
            rec["today_us"] = f"not measured ({copied / 1e9:.0f} GB of copies, {3 * out_bytes / 1e9:.0f} GB live)"
        print(json.dumps(rec), flush=True)
        del sets, words
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
