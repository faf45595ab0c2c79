"""a + (s ? k : 0) on the device: csgn_uint_add_where's one launch (k_uint_add_where) against code of the commit before
it, never the new kernel:
  (a) "loop": the launch sequence of the class-level loop, the definition's table through csgn_add_uniform /
      csgn_mul_uniform, its temporaries allocated beforehand;
  (b) "today", at w = 8 only: what a user wrote before, a + keepWhere(s, constant(k)) as csgn_const_fill +
      csgn_uint_bitwise KEEP + csgn_uint_arith ADD.  It writes DIFFERENT AND MORE words (518 terms an element whatever
      k is), so its figure is a time, not a rate to compare.
N = 1247.  The operands rotate over copies that together pass the 256 MiB memory-side cache; every shape is warmed up;
the versions are timed in turns in one process (HIP events, medians of --reps >= 20).  One JSON line per shape:
microseconds per call and WRITTEN bytes per second of each version, and whether the loop's words equal the launch's.

    python tools/bench_uint_add_where.py [--n 1247] [--reps 20] [--only I] [--scale S]
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

# (w, k, ts, log2 batch)
SHAPES = [(32, 1, 1, 16), (32, 1, 8, 14), (16, 1, 1, 18), (8, 1, 1, 20), (8, 0xA5, 1, 18), (8, 0xFF, 1, 14)]
CACHE = 256 << 20


def u64s(xs):
    return (C.c_uint64 * len(xs))(*[int(x) for x in xs])


def vps(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    ap.add_argument("--scale", type=int, default=0, help="halve every batch this many times (a quick look)")
    args = ap.parse_args()
    assert args.reps >= 20 or args.scale
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    st = hip.stream

    for i, (w, k, ts, lg) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        m = 1 << max(lg - args.scale, 0)
        ta = [1] * w
        T = hip.uint_add_where_terms(ta, ts, k)
        out_bytes = m * sum(T) * dl * 8
        in_bytes = m * (w + ts) * dl * 8
        rotate = max(2, -(-2 * CACHE // in_bytes))
        sets = [([hip.synth_fill(11 + 97 * c + j, n, 0, m * dl) for j in range(w)],
                 hip.synth_fill(5 + 97 * c, n, 0, m * ts * dl)) for c in range(rotate)]
        outs = [hip.empty_words(m * t * dl) for t in T]
        h_sets = [(vps(a), s.data_ptr()) for a, s in sets]
        h_out, h_ta = vps(outs[:w]), u64s(ta)

        def fused(r):
            h_a, d_s = h_sets[r % rotate]
            capi.check(lib.csgn_uint_add_where(n, m, w, k, d_s, ts, h_a, h_ta, h_out, outs[w].data_ptr(), st))

        # (a) the loop: every add and multiply of the table as one C call into buffers made beforehand; the carries take
        # turns between temporaries of their own, the outputs are written in place
        lout = [hip.empty_words(m * t * dl) for t in T]
        mlow = (k & -k).bit_length() - 1
        plan = []                                     # (fn, t1, t2, left, right, out); an operand: ("a", j), "s" or a tensor

        def add(x, tx, y, ty, out):
            plan.append((lib.csgn_add_uniform, tx, ty, x, y, out))
            return out, tx + ty

        def mul(x, tx, y, ty, out=None):
            out = hip.empty_words(m * tx * ty * dl) if out is None else out
            plan.append((lib.csgn_mul_uniform, tx, ty, x, y, out))
            return out, tx * ty

        c = None
        for j in range(w):
            aj, s = (("a", j), 1), ("s", ts)
            last = j + 1 == w
            if j < mlow:
                plan.append(("copy", 1, 0, ("a", j), None, lout[j]))
            elif j == mlow:
                add(*aj, *s, lout[j])
                c = mul(*aj, *s, lout[w] if last else None)
            elif (k >> j) & 1:
                ab = add(*aj, *s, hip.empty_words(m * (1 + ts) * dl))
                add(*ab, *c, lout[j])
                p = mul(*aj, *s)
                q = mul(*ab, *c)
                c = add(*p, *q, lout[w] if last else hip.empty_words(m * (p[1] + q[1]) * dl))
            else:
                add(*aj, *c, lout[j])
                c = mul(*aj, *c, lout[w] if last else None)
        assert c[1] == T[w]

        def loop(r):
            planes, d_s = sets[r % rotate]
            ptr = lambda x: (planes[x[1]] if isinstance(x, tuple) else d_s if isinstance(x, str) else x).data_ptr()   # noqa: E731
            for fn, t1, t2, x, y, out in plan:
                if fn == "copy":
                    capi.check(lib.csgn_memcpy_d2d(out.data_ptr(), ptr(x), m * dl * 8, st))
                elif fn is lib.csgn_mul_uniform:
                    capi.check(fn(n, m, t1, t2, ptr(x), ptr(y), out.data_ptr(), 0, st))
                else:
                    capi.check(fn(n, m, t1, t2, ptr(x), ptr(y), out.data_ptr(), st))

        versions = [("fused", fused, out_bytes), ("loop", loop, out_bytes)]
        # (b) today's expression at w = 8, fresh operands: the constant's planes, KEEP, ADD
        if w == 8 and ts == 1:
            one = u64s([1] * w)
            kp = [hip.empty_words(m * dl) for _ in range(w)]
            kept = [hip.empty_words(m * dl) for _ in range(w)]
            A = [int(lib.csgn_uint_arith_terms(1, w, one, one, o)) for o in range(w + 1)]
            aout = [hip.empty_words(m * t * dl) for t in A]
            h_kp, h_kept, h_aout = vps(kp), vps(kept), vps(aout[:w])

            def today(r):
                h_a, d_s = h_sets[r % rotate]
                for j in range(w):
                    capi.check(lib.csgn_const_fill(n, m, None, (k >> j) & 1, kp[j].data_ptr(), st))
                capi.check(lib.csgn_uint_bitwise(n, 6, m, w, d_s, 1, h_kp, one, None, None, h_kept, st))
                capi.check(lib.csgn_uint_arith(n, 1, m, w, h_a, one, h_kept, one, h_aout, aout[w].data_ptr(), st))

            versions.append(("today", today, m * (sum(A) + 2 * w) * dl * 8))

        rec = {"w": w, "k": k, "ts": ts, "m": m, "n": n, "terms": sum(T), "written_bytes": out_bytes,
               "rotate": rotate, "loop_launches": len(plan)}
        for name, fn, _ in versions:                  # warm-up of every version, and the words on the same operands
            fn(0)
            torch.cuda.synchronize()
        rec["same_words"] = all(torch.equal(x, y) for x, y in zip(outs, lout))
        times = {name: [] for name, _, _ in versions}
        for r in range(args.reps):                    # in turns, so that a drift of the machine meets all of them
            for name, fn, _ in versions:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(r + 1)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e-3)
        for name, _, written in versions:
            t = sorted(times[name])
            rec[name + "_us"] = round(t[len(t) // 2] * 1e6, 1)
            rec[name + "_min_us"] = round(t[0] * 1e6, 1)
            rec[name + "_written_tbps"] = round(written / t[len(t) // 2] * 1e-12, 3)
        rec["speedup_over_loop"] = round(rec["loop_us"] / rec["fused_us"], 2)
        if "today_us" in rec:
            rec["today_written_bytes"] = versions[2][2]
            rec["speedup_over_today"] = round(rec["today_us"] / rec["fused_us"], 2)
        print(json.dumps(rec), flush=True)
        del sets, outs, lout, plan, versions, h_sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
