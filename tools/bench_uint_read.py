"""Encrypted tables read at encrypted indices on the device: csgn_uint_read's fused kernel (k_uint_read) against the same
words composed row by row from the tuned launchers (knob uint_read_fused = 0), and against today's route at the class
level -- out_j = sum over r of equalTo(x, r) * row r broadcast, one csgn_uint_plain, one broadcast, and per plane one
multiply and one add (a copy of the whole running sum) per row -- where it fits.  The index planes rotate over enough
copies to pass the 256 MiB memory-side cache.  One JSON line per case: median microseconds of each form from HIP events,
E, the algorithmic bytes (outputs written once + index and table planes read once) and the fused form's share of
8 TB/s.

    python tools/bench_uint_read.py [--n 1247] [--reps 10] [--today-max-gb 2000] [--composed-max-launches 20000] [--only K]
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
    """(index width v, rows, table width w, elements m), fresh 1-term planes."""
    return [(4, 16, 8, 1 << 14), (8, 256, 8, 256), (8, 200, 8, 256), (10, 1024, 1, 256), (12, 4096, 4, 8)]


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


def today(hip, n, m, v, rows, w, index, table):
    """Today's route: the running sum of every plane, one add (a fresh copy) per row."""
    dl = hip.default_len(n)
    acc, tacc = [None] * w, 0
    for r in range(rows):
        eq = hip.uint_plain(n, capi.CSGN_UINT_PLAIN_EQ, m, index, [1] * v, r)
        te = eq.numel() // (m * dl)
        row = hip.gather_planes(n, [p[r * dl:(r + 1) * dl] for p in table], [1] * w, 1, m)
        for j in range(w):
            p = hip.mul_uniform(n, m, te, 1, eq, row[j])
            acc[j] = p if acc[j] is None else hip.add_uniform(n, m, tacc, te, acc[j], p)
        tacc += te
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--today-max-gb", type=float, default=2000.0, help="GB of copies today's route makes, at most")
    ap.add_argument("--composed-max-launches", type=int, default=20000)
    ap.add_argument("--only", type=int, default=-1, help="the one shape to run (its position in the list)")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    for k, (v, rows, w, m) in enumerate(shapes()):
        if args.only >= 0 and k != args.only:
            continue
        s = (C.c_uint64 * v)(*([1] * v))
        t = (C.c_uint64 * w)(*([1] * w))
        E = int(lib.csgn_uint_read_terms(v, s, rows))
        plane_bytes = v * m * dl * 8
        copies = max(1, min(8, -(-ROTATE_BYTES // plane_bytes)))
        sets = [[hip.synth_fill(11 + 97 * c + k, n, 0, m * dl) for k in range(v)] for c in range(copies)]
        table = [hip.synth_fill(7 + 31 * j, n, 0, rows * dl) for j in range(w)]
        outs = [hip.empty_words(m * E * dl) for _ in range(w)]
        out_bytes = w * m * E * dl * 8
        nbytes = out_bytes + (v * m + w * rows) * dl * 8
        rec = {"v": v, "rows": rows, "w": w, "m": m, "n": n, "E": E, "out_gb": round(out_bytes / 1e9, 3),
               "bytes": nbytes}
        words = {}
        launches = rows * (2 + w)
        for form, knob in (("fused", 1), ("composed", 0)):
            if knob == 0 and launches > args.composed_max_launches:
                rec["composed_us"] = f"not measured ({launches} launches)"
                continue
            capi.check(lib.csgn_set_tuning(b"uint_read_fused", knob))
            rec[form + "_kernel"] = lib.csgn_uint_read_kernel(n, m, v, s, rows, w, t).decode()
            fn = lambda r: hip.uint_read(n, m, sets[r % copies], [1] * v, rows, table, [1] * w, outs)  # noqa: E731
            rec[form + "_us"] = round(timed(fn, args.reps) * 1e6, 1)
            hip.uint_read(n, m, sets[0], [1] * v, rows, table, [1] * w, outs)
            torch.cuda.synchronize()
            words[form] = [o.clone() for o in outs] if form == "fused" else outs
        capi.check(lib.csgn_set_tuning(b"uint_read_fused", -1))
        if "composed" in words:
            rec["composed_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], words["composed"]))
        rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
        rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
        if isinstance(rec.get("composed_us"), float):
            rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
        copied = out_bytes * rows / 2
        if copied <= args.today_max_gb * 1e9 and 3 * out_bytes < 0.5 * torch.cuda.get_device_properties(0).total_memory:
            del outs
            torch.cuda.empty_cache()
            got = today(hip, n, m, v, rows, w, sets[0], table)
            torch.cuda.synchronize()
            rec["today_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], got))
            del got
            rec["today_us"] = round(timed(lambda r: today(hip, n, m, v, rows, w, sets[r % copies], table),
                                          max(3, args.reps // 3)) * 1e6, 1)
            rec["speedup_vs_today"] = round(rec["today_us"] / rec["fused_us"], 2)
        else:
            rec["today_us"] = f"not measured ({copied / 1e9:.0f} GB of copies)"
        print(json.dumps(rec), flush=True)
        del sets, words
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
