"""The first row whose encrypted mask bit is set on the device: csgn_uint_first's one launch (k_uint_first) against the
loop a user of the classes had to write before -- per row a gather of the mask row and of every value plane, logicNot,
the running product, F_r times every value plane and one sum per output -- issued through the UNCHANGED entry points
csgn_gather, csgn_gather_planes, csgn_gate_uniform, csgn_mul_uniform and csgn_add_uniform, which this operation does
not touch.  Shapes: firstWhere with 8 value planes and any over g = 4, 8, 12 and 16 fresh rows, over g = 8 rows of 2
terms, bitLength of a fresh 16-bit integer (the plane layout from the top, labels 16 - r, 5 planes) and anyOf alone at
g = 16; each at a batch whose outputs come to about 256 MB (one element at least).  The operands rotate over several
copies.  The two are timed in turns in the same run (HIP events, medians); both are issued from this process on host
arrays built beforehand.  One JSON line per shape: microseconds of each, WRITTEN bytes per second of the call against
the pure-fill ceiling of DESIGN section 0's table (7.3 TB/s), whether the words agree, and which is no slower -- the
call where it takes at most 1.05 times the loop's time (5 % for the spread between machines).

    python tools/bench_uint_first.py [--n 1247] [--reps 10] [--only I]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csgn_amd.batch import HipPath  # noqa: E402

GATE_NOT = 1
TARGET_BYTES = 256 << 20
ROTATE = 3
MARGIN = 1.05
FILL_TBPS = 7.3

# (name, group, mask terms, value planes, any, labels, planes of them, plane layout)
SHAPES = [("firstWhere g=4", 4, 1, 8, True, None, 0, False),
          ("firstWhere g=8", 8, 1, 8, True, None, 0, False),
          ("firstWhere g=12", 12, 1, 8, True, None, 0, False),
          ("firstWhere g=16", 16, 1, 8, True, None, 0, False),
          ("firstWhere g=8, 2-term masks", 8, 2, 8, True, None, 0, False),
          ("bitLength of 16 bits", 16, 1, 0, False, [16 - r for r in range(16)], 5, True),
          ("anyOf g=16", 16, 1, 0, True, None, 0, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    args = ap.parse_args()
    hip = HipPath(0)
    n = args.n
    dl = hip.default_len(n)

    for i, (name, g, s, w, any_, labels, planes, plane_layout) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        P = [s * (s + 1) ** r for r in range(g)]
        Q = sum(P)
        bits = [b for b in range(planes) if any((labels[r] >> b) & 1 for r in range(g))]
        T = [Q] * (w + any_) + [sum(P[r] for r in range(g) if (labels[r] >> b) & 1) for b in bits]
        per_element = sum(T) * dl * 8
        m = max(1, TARGET_BYTES // per_element)
        out_bytes = m * per_element
        rec = {"shape": name, "group": g, "mask_terms": s, "width": w, "any": any_, "label_planes": len(bits), "m": m, "n": n,
               "terms": sum(T), "written_bytes": out_bytes}
        outs = [hip.empty_words(m * Q * dl) for _ in range(w)]
        any_out = hip.empty_words(m * Q * dl) if any_ else False
        lab_outs = [hip.empty_words(m * t * dl) for t in T[w + any_:]]
        rows = [hip.upload(np.arange(m, dtype=np.uint64) * g + r) for r in range(g)]
        sets = []
        for c in range(ROTATE):
            if plane_layout:
                mask = [hip.synth_fill(11 + 97 * c + r, n, 0, m * s * dl) for r in range(g)]
            else:
                mask = [hip.synth_fill(11 + 97 * c, n, 0, m * g * s * dl)]
            values = [hip.synth_fill(5011 + 97 * c + j, n, 0, m * g * dl) for j in range(w)]
            sets.append((mask, values))

        def call(k):
            mask, values = sets[k % ROTATE]
            hip.uint_first(n, m, g, mask, [s] * g, values, [1] * w, outs=outs, any=any_out, labels=labels,
                           label_bits=bits, label_outs=lab_outs)
            return outs + ([any_out] if any_ else []) + lab_outs

        def loop(k):
            mask, values = sets[k % ROTATE]
            acc = [None] * len(T)
            run, tr = None, 0
            for r in range(g):
                mr = mask[r] if plane_layout else hip.gather(n, m * g, mask[0], s, m, rows[r])
                F, tf = (mr, s) if r == 0 else (hip.mul_uniform(n, m, tr, s, run, mr), tr * s)
                if r + 1 < g:
                    nr = hip.gate_uniform(n, GATE_NOT, m, mr, s)
                    run, tr = (nr, s + 1) if r == 0 else (hip.mul_uniform(n, m, tr, s + 1, run, nr), tr * (s + 1))
                kept = [F] * (any_ + 0)
                if w:
                    d = hip.gather_planes(n, values, [1] * w, m * g, m, rows[r])
                    kept = [hip.mul_uniform(n, m, tf, 1, F, dj) for dj in d] + kept
                kept += [F if (labels[r] >> b) & 1 else None for b in bits]
                for x, p in enumerate(kept):
                    if p is None:
                        continue
                    if acc[x] is None:
                        acc[x] = (p, tf)
                    else:
                        acc[x] = (hip.add_uniform(n, m, acc[x][1], tf, acc[x][0], p), acc[x][1] + tf)
            return [a[0] for a in acc]

        forms = (("call", call), ("loop", loop))
        words = {}
        for form, fn in forms:                          # warm-up of both, and their words on the same operands
            got = fn(0)
            torch.cuda.synchronize()
            words[form] = [o[: m * t * dl].clone() for o, t in zip(got, T)]
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
            t = sorted(times[form])
            rec[form + "_us"] = round(t[len(t) // 2] * 1e6, 1)
            rec[form + "_min_us"] = round(t[0] * 1e6, 1)
        rec["call_written_tbps"] = round(out_bytes / (rec["call_us"] * 1e-6) * 1e-12, 3)
        rec["call_of_fill_ceiling"] = round(rec["call_written_tbps"] / FILL_TBPS, 3)
        rec["speedup"] = round(rec["loop_us"] / rec["call_us"], 2)
        rec["no_slower"] = "call" if rec["call_us"] <= MARGIN * rec["loop_us"] else "loop"
        print(json.dumps(rec), flush=True)
        del outs, any_out, lab_outs, sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
