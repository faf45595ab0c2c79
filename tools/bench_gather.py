"""Gather / tile / broadcast on the device: csgn_gather (k_gather, k_gather_ragged) and csgn_gather_planes against
csgn_memcpy_d2d of the same output bytes, and at 2^14 elements against the per-element route (one csgn_memcpy_d2d per
element: what `at` plus `pack` costs).  Sources rotate over enough copies to pass 512 MiB, so they come from HBM.  One JSON
line per case: median microseconds from HIP events, the algorithmic bytes (output written once + the source bytes the
gather reads once) and their rate, and the gather's time as a share of the copy's.

    python tools/bench_gather.py [--n 1247] [--reps 20]
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


def copies_for(nbytes):
    return max(1, -(-ROTATE_BYTES // max(nbytes, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    st = hip.stream
    rng = np.random.default_rng(1)

    def memcpy_us(out_bytes):
        a, b = hip.empty_words(out_bytes // 8), hip.empty_words(out_bytes // 8)
        return timed(lambda r: capi.check(lib.csgn_memcpy_d2d(a.data_ptr(), b.data_ptr(), out_bytes, st)), args.reps)

    def emit(case, us, alg_bytes, out_bytes, extra=None):
        cp = memcpy_us(out_bytes)
        line = {"case": case, "n": n, "us": round(us * 1e6, 2), "memcpy_us": round(cp * 1e6, 2),
                "alg_bytes": alg_bytes, "alg_tbps": round(alg_bytes / us / 1e12, 3),
                "pct_of_8tbps": round(100 * alg_bytes / us / PEAK, 1), "memcpy_time_over_gather": round(cp / us, 3)}
        line.update(extra or {})
        print(json.dumps(line), flush=True)

    # uniform sources
    for t, count, kinds in ((1, 1 << 14, ("perm",)), (1, 1 << 16, ("identity", "perm", "broadcast")),
                            (1, 1 << 20, ("identity", "perm", "broadcast")), (64, 1 << 14, ("identity", "perm", "broadcast"))):
        elem = t * dl
        src_bytes = count * elem * 8
        srcs = [hip.synth_fill(7 + c, n, 0, count * elem) for c in range(copies_for(src_bytes))]
        out = hip.empty_words(count * elem)
        for kind in kinds:
            if kind == "broadcast":
                idx, count_in, read = None, 1, elem * 8
            else:
                perm = np.arange(count) if kind == "identity" else rng.permutation(count)
                idx, count_in, read = hip.upload(perm.astype(np.uint64)), count, src_bytes

            def run(r, idx=idx, count_in=count_in):
                s = srcs[r % len(srcs)]
                capi.check(lib.csgn_gather(n, count_in, s.data_ptr(), None, t, count, 0 if idx is None else idx.data_ptr(),
                                           out.data_ptr(), None, 0, st))
            extra = {"t": t, "count": count, "kind": kind}
            if count == 1 << 14 and kind == "perm":
                perm_h = hip.download(idx).astype(np.int64)

                def per_element(r):
                    s = srcs[r % len(srcs)].data_ptr()
                    for e in range(count):
                        capi.check(lib.csgn_memcpy_d2d(out.data_ptr() + e * elem * 8, s + int(perm_h[e]) * elem * 8,
                                                       elem * 8, st))
                pe = timed(per_element, max(3, args.reps // 5))
                extra["per_element_us"] = round(pe * 1e6, 1)
            emit(f"uniform t={t} count={count} {kind}", timed(run, args.reps), count * elem * 8 + read, count * elem * 8,
                 extra)
        del srcs, out
        torch.cuda.empty_cache()

    # a ragged log-normal batch, gathered by a random permutation
    count = 1 << 16
    sizes = np.minimum(np.floor(rng.lognormal(1.0, 1.2, size=count)), 4096).astype(np.uint64)
    src_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(src_off[-1])
    srcs = [hip.synth_fill(40 + c, n, 0, total * dl) for c in range(copies_for(total * dl * 8))]
    d_off = hip.upload(src_off)
    perm = hip.upload(rng.permutation(count).astype(np.uint64))
    rc, tot, bad, out_off = hip.gather_plan(count, count, perm, d_off)
    capi.check(rc)
    out = hip.empty_words(tot * dl)
    plan_us = timed(lambda r: hip.gather_plan(count, count, perm, d_off, out_off), args.reps)

    def run_ragged(r):
        s = srcs[r % len(srcs)]
        capi.check(lib.csgn_gather(n, count, s.data_ptr(), d_off.data_ptr(), 0, count, perm.data_ptr(), out.data_ptr(),
                                   out_off.data_ptr(), tot, st))
    emit(f"ragged lognormal count={count} perm", timed(run_ragged, args.reps), 2 * tot * dl * 8, tot * dl * 8,
         {"count": count, "terms": tot, "max_terms": int(sizes.max()), "kind": "perm",
          "plan_us_with_sync": round(plan_us * 1e6, 1)})
    del srcs, out
    torch.cuda.empty_cache()

    # a UIntBatch of 8 one-term planes, every plane in one launch
    count, w = 1 << 20, 8
    plane_bytes = count * dl * 8
    sets = [[hip.synth_fill(60 + 8 * c + j, n, 0, count * dl) for j in range(w)]
            for c in range(copies_for(w * plane_bytes))]
    outs = [hip.empty_words(count * dl) for _ in range(w)]
    perm = hip.upload(rng.permutation(count).astype(np.uint64))
    h_dst = (C.c_void_p * w)(*[o.data_ptr() for o in outs])
    h_terms = (C.c_uint64 * w)(*([1] * w))
    h_srcs = [(C.c_void_p * w)(*[p.data_ptr() for p in s]) for s in sets]

    def run_planes(r):
        capi.check(lib.csgn_gather_planes(n, w, h_srcs[r % len(h_srcs)], h_terms, count, count, perm.data_ptr(), h_dst, st))
    emit(f"uint w={w} count={count} perm", timed(run_planes, args.reps), 2 * w * plane_bytes, w * plane_bytes,
         {"count": count, "planes": w, "kind": "perm"})


if __name__ == "__main__":
    main()
