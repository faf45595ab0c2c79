"""Running counts of encrypted flags on the device: csgn_count_prefix's one launch (k_count_prefix) against the cheapest
loop the classes can compose -- per row one csgn_gather of the row's prefix and one csgn_count over it (the plane
layout hands csgn_count the first planes and needs no gather) --, both issued through the UNCHANGED entry points
csgn_gather and csgn_count, which this operation does not touch.  Shapes: fresh flags in groups of 8, 16, 32 and 64 with
every plane whose rows together stay within the batch's budget, groups of 8 two-term flags, and the plane layout at 32
bits; each at a batch whose outputs come to about 256 MB (one element at least).  The operands rotate over several
copies.  The two are timed in turns in the same run (HIP events, medians); both are issued from this process on host
arrays built beforehand.  One JSON line per shape: microseconds of each, WRITTEN bytes per second of the call against
the pure-fill ceiling of DESIGN section 0's table (7.3 TB/s), whether the words agree, and which is no slower -- the call
where it takes at most 1.05 times the loop's time (5 % for the spread between machines).

    python tools/bench_count_prefix.py [--n 1247] [--reps 10] [--only I] [--exclusive]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csgn_amd.batch import HipPath  # noqa: E402

TARGET_BYTES = 256 << 20
ROTATE = 3
MARGIN = 1.05
FILL_TBPS = 7.3

# (group, terms of a flag, layout)
SHAPES = [(8, 1, "grouped"), (16, 1, "grouped"), (32, 1, "grouped"), (64, 1, "grouped"), (8, 2, "grouped"),
          (32, 1, "planes")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    ap.add_argument("--exclusive", action="store_true")
    args = ap.parse_args()
    hip = HipPath(0)
    n = args.n
    dl = hip.default_len(n)
    ex = 1 if args.exclusive else 0

    def offset(g, t, j, r):
        return int(hip.lib.csgn_count_prefix_offset(g, t, j, ex, r))

    for i, (g, t, layout) in enumerate(SHAPES):
        if args.only >= 0 and i != args.only:
            continue
        # the planes that fit: the rows of one element within the budget (and the last row below 2^31 words)
        js = [j for j in range(7) if 0 < offset(g, t, j, g) * dl * 8 <= TARGET_BYTES
              and int(hip.lib.csgn_count_terms(g - ex, t, j)) * dl < (1 << 31)]
        A = [offset(g, t, j, g) for j in js]
        per_element = sum(A) * dl * 8
        m = max(1, TARGET_BYTES // per_element)
        out_bytes = m * per_element
        rec = {"shape": "g=%d%s%s%s" % (g, ", %d-term flags" % t if t > 1 else "", ", plane layout" if layout == "planes" else "",
                                        ", exclusive" if ex else ""),
               "group": g, "t": t, "layout": layout, "exclusive": ex, "planes": js, "m": m, "n": n, "terms": sum(A),
               "written_bytes": out_bytes}
        blocks = [hip.empty_words(m * a * dl) for a in A]
        rows = range(ex, g)                                   # the rows that count an input at least
        prefix_idx = {}
        if layout == "grouped":
            for r in rows:
                nr = r + 1 - ex
                q = np.arange(m, dtype=np.uint64)[:, None] * np.uint64(g)
                prefix_idx[r] = hip.upload((q + np.arange(nr, dtype=np.uint64)[None, :]).ravel())
        sets = []
        for c in range(ROTATE):
            if layout == "grouped":
                sets.append([hip.synth_fill(11 + 97 * c, n, 0, m * g * t * dl)])
            else:
                sets.append([hip.synth_fill(11 + 97 * c + 7 * b, n, 0, m * t * dl) for b in range(g)])

        # row r of plane j inside its block, for the comparison of the words (no part of the timed call)
        span = {(r, j): (x, m * offset(g, t, j, r) * dl, m * offset(g, t, j, r + 1) * dl)
                for x, j in enumerate(js) for r in rows if (1 << j) <= r + 1 - ex}

        def call(k):
            hip.count_prefix(n, m, g, t, sets[k % ROTATE], js, exclusive=bool(ex), outs=blocks)
            return span

        def loop(k):
            ins = sets[k % ROTATE]
            out = {}
            for r in rows:
                nr = r + 1 - ex
                have = [j for j in js if (1 << j) <= nr]
                if not have:
                    continue
                if layout == "grouped":
                    prefix = [hip.gather(n, m * g, ins[0], t, m * nr, prefix_idx[r])]
                else:
                    prefix = ins[:nr]
                for j, o in zip(have, hip.count(n, m, nr, t, prefix, have)):
                    out[r, j] = o
            return out

        forms = (("call", call), ("loop", loop))
        words = {}
        for form, fn in forms:                          # warm-up of both, and their words on the same operands
            got = fn(0)
            torch.cuda.synchronize()
            if form == "call":
                got = {key: blocks[x][lo:hi] for key, (x, lo, hi) in got.items()}
            words[form] = {key: o.clone() for key, o in got.items()}
        rec["same_words"] = words["call"].keys() == words["loop"].keys() and \
            all(torch.equal(words["call"][key], words["loop"][key]) for key in words["call"])
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
        del blocks, sets, prefix_idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
