"""The k-th row whose encrypted mask bit is set on the device: csgn_uint_nth's one launch (k_uint_nth) against the
class-level loop composed from the existing batch operators -- per segment (row r, degree d) one gather per factor
over the (element, subset) pairs, the product chain, one sum into G_r; per row a gather of every value plane, G_r times
every value plane and one sum per output -- issued through the UNCHANGED entry points csgn_gather, csgn_gather_planes,
csgn_mul_uniform and csgn_add_uniform, which this operation does not touch.  The loop tiles the subsets of a segment
through gather, so it launches per segment and not per subset: the cheapest loop the classes can compose.  Shapes:
nthWhere with 8 value planes and valid, and atLeast alone (width 0), over g = 8, 12 and 16 fresh rows at slots 0, 1 and
g / 2, and over g = 8 rows of 2 terms; each at a batch whose outputs come to about 256 MB (one element at least).  The
operands rotate over several copies.  The two are timed in turns in the same run (HIP events, medians); both are issued
from this process on host arrays built beforehand.  One JSON line per shape: microseconds of each, WRITTEN bytes per
second of the call against the pure-fill ceiling of DESIGN section 0's table (7.3 TB/s), whether the words agree, and
which is no slower -- the call where it takes at most 1.05 times the loop's time (5 % for the spread between machines).

    python tools/bench_uint_nth.py [--n 1247] [--reps 10] [--only I]
"""
import argparse
import json
import os
import sys
from itertools import combinations
from math import comb

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csgn_amd.batch import HipPath  # noqa: E402

TARGET_BYTES = 256 << 20
ROTATE = 3
MARGIN = 1.05
FILL_TBPS = 7.3

# (group, mask terms, slot, value planes)
SHAPES = [(g, 1, s, w) for g in (8, 12, 16) for s in (0, 1, g // 2) for w in (8, 0)] + \
         [(8, 2, s, w) for s in (0, 1, 4) for w in (8, 0)]


def segments(g, slot):
    return [(r, d) for r in range(slot, g) for d in range(slot, r + 1) if slot & ~d == 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    args = ap.parse_args()
    hip = HipPath(0)
    n = args.n
    dl = hip.default_len(n)

    for i, (g, t, slot, w) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        segs = segments(g, slot)
        Q = sum(comb(r, d) * t ** (d + 1) for r, d in segs)
        assert Q == int(hip.lib.csgn_uint_nth_terms(g, t, slot, g))
        T = [Q] * (w + 1)
        per_element = sum(T) * dl * 8
        m = max(1, TARGET_BYTES // per_element)
        out_bytes = m * per_element
        name = ("nthWhere" if w else "atLeast") + " g=%d slot=%d" % (g, slot) + (", %d-term masks" % t if t > 1 else "")
        rec = {"shape": name, "group": g, "mask_terms": t, "slot": slot, "width": w, "m": m, "n": n, "segments": len(segs),
               "terms": sum(T), "written_bytes": out_bytes}
        outs = [hip.empty_words(m * Q * dl) for _ in range(w)]
        valid = hip.empty_words(m * Q * dl)
        rows = [hip.upload(np.arange(m, dtype=np.uint64) * g + r) for r in range(g)]
        # factor k of the (element, subset) pairs of segment (r, d): element q * g + subset[k], the subsets lexicographic
        tiles = {}
        for r, d in segs:
            subs = np.array(list(combinations(range(r), d)), dtype=np.uint64).reshape(comb(r, d), d)
            subs = np.concatenate([subs, np.full((len(subs), 1), r, dtype=np.uint64)], axis=1)
            q = np.arange(m, dtype=np.uint64)[:, None] * np.uint64(g)
            tiles[r, d] = [hip.upload((q + subs[None, :, k]).ravel()) for k in range(d + 1)]
        sets = []
        for c in range(ROTATE):
            mask = [hip.synth_fill(11 + 97 * c, n, 0, m * g * t * dl)]
            values = [hip.synth_fill(5011 + 97 * c + j, n, 0, m * g * dl) for j in range(w)]
            sets.append((mask, values))

        def call(k):
            mask, values = sets[k % ROTATE]
            hip.uint_nth(n, m, g, slot, mask, t, values, [1] * w, outs=outs, valid=valid)
            return outs + [valid]

        def loop(k):
            mask, values = sets[k % ROTATE]
            acc = [None] * len(T)
            for r in range(slot, g):
                G, tg = None, 0
                for d in range(slot, r + 1):
                    if slot & ~d:
                        continue
                    idx = tiles[r, d]
                    pairs = m * comb(r, d)
                    p, tp = hip.gather(n, m * g, mask[0], t, pairs, idx[0]), t
                    for x in idx[1:]:
                        p, tp = hip.mul_uniform(n, pairs, tp, t, p, hip.gather(n, m * g, mask[0], t, pairs, x)), tp * t
                    tp *= comb(r, d)                    # m elements of C(r, d) * t^(d+1) terms: the segment
                    G, tg = (p, tp) if G is None else (hip.add_uniform(n, m, tg, tp, G, p), tg + tp)
                kept = [G]
                if w:
                    dv = hip.gather_planes(n, values, [1] * w, m * g, m, rows[r])
                    kept = [hip.mul_uniform(n, m, tg, 1, G, dj) for dj in dv] + kept
                for x, p in enumerate(kept):
                    if acc[x] is None:
                        acc[x] = (p, tg)
                    else:
                        acc[x] = (hip.add_uniform(n, m, acc[x][1], tg, acc[x][0], p), acc[x][1] + tg)
            return [a[0] for a in acc]

        forms = (("call", call), ("loop", loop))
        words = {}
        for form, fn in forms:                          # warm-up of both, and their words on the same operands
            got = fn(0)
            torch.cuda.synchronize()
            words[form] = [o[: m * x * dl].clone() for o, x in zip(got, T)]
        rec["same_words"] = all(torch.equal(x, y) for x, y in zip(words["call"], words["loop"]))
        del words, got
        times = {"call": [], "loop": []}
        for k in range(args.reps):                      # in turns, so that a drift of the machine meets both
            for form, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(k + 1)
                e1.record()
                e1.synchronize()
                times[form].append(e0.elapsed_time(e1) * 1e-3)
        for form, _ in forms:
            ts = sorted(times[form])
            rec[form + "_us"] = round(ts[len(ts) // 2] * 1e6, 1)
            rec[form + "_min_us"] = round(ts[0] * 1e6, 1)
        rec["call_written_tbps"] = round(out_bytes / (rec["call_us"] * 1e-6) * 1e-12, 3)
        rec["call_of_fill_ceiling"] = round(rec["call_written_tbps"] / FILL_TBPS, 3)
        rec["speedup"] = round(rec["loop_us"] / rec["call_us"], 2)
        rec["no_slower"] = "call" if rec["call_us"] <= MARGIN * rec["loop_us"] else "loop"
        print(json.dumps(rec), flush=True)
        del outs, valid, sets, tiles, rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
