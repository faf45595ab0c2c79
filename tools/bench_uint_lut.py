"""Public lookup tables on the device: csgn_uint_lut_apply's fused kernel (k_uint_lut) against the same words composed
monomial by monomial from the tuned launchers (knob uint_lut_fused = 0), and against today's route -- output j as the sum
over the k with bit j of f(k) set of equalTo(a, k) (csgn_uint_plain, one launch per k and one copy per add) -- where its
output fits.  The input planes rotate over enough copies to pass the 256 MiB memory-side cache.  One JSON line per case:
median microseconds of each form from HIP events, the term counts, the algorithmic bytes (outputs written once + planes
read once) and the fused form's share of 8 TB/s.

    python tools/bench_uint_lut.py [--n 1247] [--reps 10] [--today-max-gb 16] [--composed-max-launches 20000]
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
from tests.test_uint_lut_cpu import aes_sbox, np_anf, random_table  # noqa: E402

PEAK = 8e12
ROTATE_BYTES = 512 << 20


def shapes():
    return [("x*3 mod 16", 4, 4, [(3 * x) % 16 for x in range(16)], (1 << 14, 1 << 20)),
            ("popcount", 4, 3, [bin(x).count("1") for x in range(16)], (1 << 14, 1 << 20)),
            ("aes sbox", 8, 8, aes_sbox(), (1 << 10, 1 << 14, 1 << 16)),
            ("random 12->1", 12, 1, random_table(12, 1, 12), (1024,)),
            ("random 16->1", 16, 1, random_table(16, 1, 16), (64,))]


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


def today(hip, n, batch, w, table, j, planes, out):
    """Output j by today's route into `out` (batch x T x dL words)."""
    dl = hip.default_len(n)
    view = out.view(batch, -1, dl)
    off = 0
    for k in range(1 << w):
        if (table[k] >> j) & 1:
            e = hip.uint_plain(n, capi.CSGN_UINT_PLAIN_EQ, batch, planes, [1] * w, k).view(batch, -1, dl)
            view[:, off:off + e.shape[1], :].copy_(e)
            off += e.shape[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--today-max-gb", type=float, default=16.0)
    ap.add_argument("--composed-max-launches", type=int, default=20000)
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    for name, w, m, table, batches in shapes():
        anf = np_anf(table, w)
        T = (C.c_uint64 * m)()
        capi.check(lib.csgn_uint_lut_terms(w, m, (C.c_uint64 * len(table))(*table), (C.c_uint64 * w)(*([1] * w)), T))
        T = [int(t) for t in T]
        launches = sum(max(1, bin(S).count("1") - 1) for S in range(1 << w) for j in range(m) if (anf[S] >> j) & 1)
        today_terms = [sum(2 ** (w - bin(k).count("1")) for k in range(1 << w) if (table[k] >> j) & 1) for j in range(m)]
        handle = hip.uint_lut_create(table, w, m, [1] * w)
        for batch in batches:
            plane_bytes = w * batch * dl * 8
            copies = max(1, min(8, -(-ROTATE_BYTES // plane_bytes)))
            sets = [[hip.synth_fill(11 + 97 * c + i, n, 0, batch * dl) for i in range(w)] for c in range(copies)]
            outs = [hip.empty_words(batch * t * dl) for t in T]
            nbytes = batch * (sum(T) + w) * dl * 8
            rec = {"table": name, "w": w, "out_width": m, "batch": batch, "n": n, "terms": T,
                   "terms_total": sum(T), "today_terms_total": sum(today_terms), "bytes": nbytes}
            words = {}
            for form, knob in (("fused", 1), ("composed", 0)):
                if knob == 0 and launches > args.composed_max_launches:
                    rec["composed_us"] = f"not measured ({launches} launches)"
                    continue
                capi.check(lib.csgn_set_tuning(b"uint_lut_fused", knob))
                rec[form + "_kernel"] = lib.csgn_uint_lut_kernel(n, handle, batch).decode()
                fn = lambda r: hip.uint_lut_apply(handle, n, batch, sets[r % copies], T, outs)  # noqa: E731
                rec[form + "_us"] = round(timed(fn, args.reps) * 1e6, 1)
                hip.uint_lut_apply(handle, n, batch, sets[0], T, outs)
                torch.cuda.synchronize()
                words[form] = [o.clone() for o in outs] if form == "fused" else outs
            capi.check(lib.csgn_set_tuning(b"uint_lut_fused", -1))
            if "composed" in words:
                assert all(torch.equal(a, b) for a, b in zip(words["fused"], words["composed"]))
            del words
            rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
            rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
            if isinstance(rec.get("composed_us"), float):
                rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
            if batch * (sum(today_terms) + max(today_terms)) * dl * 8 <= args.today_max_gb * 1e9:
                touts = [hip.empty_words(batch * t * dl) for t in today_terms]

                def route(r):
                    for j in range(m):
                        today(hip, n, batch, w, table, j, sets[r % copies], touts[j])

                rec["today_us"] = round(timed(route, max(3, args.reps // 3)) * 1e6, 1)
                rec["speedup_vs_today"] = round(rec["today_us"] / rec["fused_us"], 2)
                del touts
            else:
                rec["today_us"] = "not measured (output too large)"
            print(json.dumps(rec), flush=True)
            del sets, outs
            torch.cuda.empty_cache()
        lib.csgn_uint_lut_destroy(handle)


if __name__ == "__main__":
    main()
