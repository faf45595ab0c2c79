"""An encrypted integer plus a public constant on the device: csgn_uint_addk's fused kernel (k_uint_addk) against the
same words composed plane by plane from the tuned launchers (knob uint_addk_fused = 0), and against today's route --
the constant trivially encrypted (UIntBatch::constant) and added with csgn_uint_step.  One JSON line per case: median
microseconds of each form from HIP events, the algorithmic bytes (outputs written once + planes read once) and the fused
form's share of 8 TB/s.  The fused and composed forms write into outputs allocated once; today's route takes its
outputs from torch's caching allocator inside the timed region (no device allocation after the warm-up call).  The inputs rotate over more than 512 MiB of distinct planes, so no call re-reads what the
memory-side cache still holds from the one before.

    python tools/bench_uint_addk.py [--n 1247] [--reps 10] [--today-max-gb 16]
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
ROTATE_BYTES = 512 << 20
# (width, batch, constants)
SHAPES = [(8, 1 << 16, (1, 100, 255)), (8, 1 << 20, (1, 100, 255)), (16, 1 << 16, (1, 0xFF00)),
          (32, 1 << 16, (1, 3, 0xFF000000))]


def timed(fn, reps):
    fn(0)
    torch.cuda.synchronize()
    ts = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i + 1)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


def today(hip, n, batch, w, k, planes):
    """a + constant(k) as UIntBatch does it today: the constant's planes are trivial encryptions."""
    dl = hip.default_len(n)
    const = []
    for j in range(w):
        c = hip.empty_words(batch * dl)
        capi.check(hip.lib.csgn_const_fill(n, batch, None, (k >> j) & 1, c.data_ptr(), hip.stream))
        const.append(c)
    s, c = hip.uint_step(n, capi.CSGN_UINT_ADD_HALF, batch, planes[0], 1, const[0], 1, carry=True)
    tc = 1
    for j in range(1, w):
        if j + 1 < w:
            s, c = hip.uint_step(n, capi.CSGN_UINT_ADD_FULL, batch, planes[j], 1, const[j], 1, c, tc, carry=True)
            tc = 1 + 2 * tc
        else:
            s = hip.uint_step(n, capi.CSGN_UINT_ADD_FULL, batch, planes[j], 1, const[j], 1, c, tc, carry=False)


def today_terms(w):
    """Terms of every plane of today's sum and of the carries it keeps between planes."""
    return [2 ** j + 1 for j in range(w)], [2 ** (j + 1) - 1 for j in range(w - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--today-max-gb", type=float, default=16.0)
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    for w, batch, ks in SHAPES:
        in_bytes = w * batch * dl * 8
        sets = ROTATE_BYTES // in_bytes + 2
        planes = [[hip.synth_fill(11 + 97 * r + j, n, 0, batch * dl) for j in range(w)] for r in range(sets)]
        for k in ks:
            T = hip.uint_addk_terms([1] * w, k)
            nbytes = batch * (sum(T[:w]) + w) * dl * 8
            rec = {"w": w, "k": k, "batch": batch, "n": n, "terms_top": T[w - 1], "terms_max": max(T[:w]),
                   "terms_sum": sum(T[:w]), "bytes": nbytes, "input_sets": sets}
            outs = [hip.empty_words(batch * t * dl) for t in T[:w]]
            kept = {}
            for form, knob in (("fused", 1), ("composed", 0)):
                capi.check(lib.csgn_set_tuning(b"uint_addk_fused", knob))
                fn = lambda i: hip.uint_addk(n, batch, planes[i % sets], [1] * w, k, outs=outs)  # noqa: E731
                rec[form + "_us"] = round(timed(fn, args.reps) * 1e6, 1)
                hip.uint_addk(n, batch, planes[0], [1] * w, k, outs=outs)
                torch.cuda.synchronize()
                kept[form] = [hip.digest(o) for o in outs]
            capi.check(lib.csgn_set_tuning(b"uint_addk_fused", -1))
            assert kept["fused"] == kept["composed"], "the two forms' words differ"
            del outs
            rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
            rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
            rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
            sums, carries = today_terms(w)
            rec["today_terms_top"], rec["today_terms_sum"] = sums[-1], sum(sums)
            if batch * (sum(sums) + sum(carries)) * dl * 8 <= args.today_max_gb * 1e9:
                fn = lambda i: today(hip, n, batch, w, k, planes[i % sets])  # noqa: E731
                rec["today_us"] = round(timed(fn, args.reps) * 1e6, 1)
                rec["speedup_vs_today"] = round(rec["today_us"] / rec["fused_us"], 2)
            else:
                rec["today_us"] = "not measured (output too large)"
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
        del planes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
