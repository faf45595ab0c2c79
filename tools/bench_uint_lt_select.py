"""Selection by an encrypted comparison on the device: csgn_uint_lt_select's fused kernel (k_uint_lt_select) against the
same words composed from the tuned launchers (knob uint_lt_select_form = 0), and against an emulation of the route a user
takes without it, select(lessThan(a, b), x, y): LT_FIRST and one LT_STEP per further plane, each writing the running
comparison the next reads back, then one MUX gate per output plane, each re-reading the whole comparison.  The emulation
issues that launcher sequence through the Python wrappers into preallocated tensors: it has none of the classes' own
overhead and no block cache, and is not the C++ calls themselves.  The operand planes rotate over enough copies to pass
the 256 MiB memory-side cache.  One JSON line per case: median microseconds of each form from HIP events, L, the
algorithmic bytes (outputs written once + every operand and request plane read once) and each form's share of 8 TB/s.

    python tools/bench_uint_lt_select.py [--n 1247] [--reps 10] [--only I]
    python tools/bench_uint_lt_select.py --only 2 --fused-calls 5      # nothing but five fused calls (for a kernel trace)
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csgn_amd import capi  # noqa: E402
from csgn_amd.batch import HipPath  # noqa: E402

PEAK = 8e12
ROTATE_BYTES = 512 << 20


def shapes():
    """(width w, elements m, what, payload width), fresh 1-term planes."""
    return [(2, 1 << 20, "minMax", 0), (4, 1 << 16, "minMax", 0), (8, 256, "minMax", 0),
            (8, 128, "compareExchange", 8), (8, 1024, "min", 0)]


def requests(what, w, pw):
    """(x, y) per output plane as indices into the set [a planes, b planes, pa planes, pb planes]."""
    a, b = list(range(w)), list(range(w, 2 * w))
    pa, pb = list(range(2 * w, 2 * w + pw)), list(range(2 * w + pw, 2 * w + 2 * pw))
    if what == "min":
        return a, b
    if what == "minMax":
        return a + b, b + a
    return a + b + pa + pb, b + a + pb + pa


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


def parent_route(hip, n, m, w, planes, xs, ys, tmp, outs):
    """select(lessThan(a, b), x, y) as its launches: the steps into two temporaries that take turns, one MUX an output."""
    cur = (w - 1) & 1
    hip.uint_step(n, capi.CSGN_UINT_LT_FIRST, m, planes[0], 1, planes[w], 1, outs=[tmp[cur]])
    L = 2
    for j in range(1, w):
        hip.uint_step(n, capi.CSGN_UINT_LT_STEP, m, planes[j], 1, planes[w + j], 1, x=tmp[cur], t_x=L, outs=[tmp[cur ^ 1]])
        L = 3 * L + 2
        cur ^= 1
    for x, y, o in zip(xs, ys, outs):
        hip.gate_uniform(n, capi.CSGN_GATE_MUX, m, planes[x], 1, planes[y], 1, sel=tmp[0], t_sel=L, out=o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    ap.add_argument("--fused-calls", type=int, default=0, help="run nothing but this many fused calls (operands uploaded, not generated)")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    for i, (w, m, what, pw) in enumerate(shapes()):
        if args.only >= 0 and i != args.only:
            continue
        one = (C.c_uint64 * 64)(*([1] * 64))
        L = int(lib.csgn_uint_lt_terms(w, one, one))
        xs, ys = requests(what, w, pw)
        n_out, n_planes = len(xs), 2 * w + 2 * pw
        T = 2 * L + 1
        plane_bytes = n_planes * m * dl * 8
        out_bytes = n_out * m * T * dl * 8
        nbytes = out_bytes + plane_bytes
        outs = [hip.empty_words(m * T * dl) for _ in range(n_out)]
        if args.fused_calls:
            rng = np.random.default_rng(3)
            planes = [hip.upload(rng.integers(0, 2**63, m * dl, dtype=np.uint64)) for _ in range(n_planes)]
            capi.check(lib.csgn_set_tuning(b"uint_lt_select_form", 1))
            for _ in range(args.fused_calls):
                hip.uint_lt_select(n, m, planes[:w], [1] * w, planes[w:2 * w], [1] * w, [planes[x] for x in xs],
                                   [1] * n_out, [planes[y] for y in ys], [1] * n_out, outs=outs)
            torch.cuda.synchronize()
            print(json.dumps({"w": w, "m": m, "what": what, "fused_calls": args.fused_calls}), flush=True)
            continue
        copies = max(1, min(8, -(-ROTATE_BYTES // plane_bytes)))
        sets = [[hip.synth_fill(11 + 97 * c + k, n, 0, m * dl) for k in range(n_planes)] for c in range(copies)]
        rec = {"w": w, "m": m, "what": what, "outputs": n_out, "n": n, "L": L, "out_gb": round(out_bytes / 1e9, 3),
               "bytes": nbytes}

        def call(r):
            p = sets[r % copies]
            hip.uint_lt_select(n, m, p[:w], [1] * w, p[w:2 * w], [1] * w, [p[x] for x in xs], [1] * n_out,
                               [p[y] for y in ys], [1] * n_out, outs=outs)

        words = None
        for form, knob in (("fused", 1), ("composed", 0)):
            capi.check(lib.csgn_set_tuning(b"uint_lt_select_form", knob))
            rec[form + "_kernel"] = lib.csgn_uint_lt_select_kernel(n, m, w, one, one, n_out, one, one, 0).decode()
            rec[form + "_us"] = round(timed(call, args.reps if knob else max(3, args.reps // 3)) * 1e6, 1)
            call(0)
            torch.cuda.synchronize()
            if form == "fused":
                words = [o.clone() for o in outs]
            else:
                rec["composed_same_words"] = all(torch.equal(a, b) for a, b in zip(words, outs))
        capi.check(lib.csgn_set_tuning(b"uint_lt_select_form", -1))
        rec["default_kernel"] = lib.csgn_uint_lt_select_kernel(n, m, w, one, one, n_out, one, one, 0).decode()
        tmp = [hip.empty_words(m * L * dl), hip.empty_words(m * max(L // 3, 1) * dl)]
        parent_route(hip, n, m, w, sets[0], xs, ys, tmp, outs)
        torch.cuda.synchronize()
        rec["parent_same_words"] = all(torch.equal(a, b) for a, b in zip(words, outs))
        rec["parent_us"] = round(timed(lambda r: parent_route(hip, n, m, w, sets[r % copies], xs, ys, tmp, outs),
                                       max(3, args.reps // 3)) * 1e6, 1)
        rec["parent_route"] = "emulation: the launcher sequence through the Python wrappers"
        for form in ("fused", "composed", "parent"):
            rec[form + "_tbps"] = round(nbytes / rec[form + "_us"] * 1e-6, 2)
        rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
        rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
        rec["speedup_vs_parent"] = round(rec["parent_us"] / rec["fused_us"], 2)
        print(json.dumps(rec), flush=True)
        del outs, sets, words, tmp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
