"""a + b, a - b, a == b and a != b of encrypted integers on the device: csgn_uint_arith's one launch (k_uint_arith)
against the per-bit chain (knob uint_arith_form = 0: csgn_uint_step's and csgn_gate_uniform's launchers plane by plane,
the launches the class operators issued before), on fresh planes.  ADD and SUB with their carry, EQ and NE, at widths
4, 8 and 12, each at one small batch (about 1 MB of outputs: the chain is launch-bound) and at one whose outputs pass
the 256 MiB memory-side cache (about 1 GB).  The operand planes rotate over several copies.  The two forms are timed
in turns in the same run (HIP events, medians).  One JSON line per case: microseconds and WRITTEN bytes per second of
each form, whether the words agree, the form the per-shape default names and the form this run shows to be no slower:
the one launch where it takes at most 1.05 times the chain's time (an allowance of 5 % on the chain's figure, for the
spread between machines; a form within it counts as level), else the chain.

    python tools/bench_uint_arith.py [--n 1247] [--reps 20] [--only I]
    python tools/bench_uint_arith.py --only 7 --fused-calls 5       # nothing but five fused calls (for a kernel trace)
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

OPS = {"add": 1, "sub": 2, "eq": 3, "ne": 4}
SMALL_BYTES, LARGE_BYTES = 1 << 20, 1 << 30
ROTATE = 4
MARGIN = 1.05


def shapes(terms_of):
    """(op name, width, elements, "small" | "large"), fresh 1-term planes."""
    out = []
    for name in OPS:
        for w in (4, 8, 12):
            per_element = terms_of(name, w)
            for size, target in (("small", SMALL_BYTES), ("large", LARGE_BYTES)):
                out.append((name, w, max(1, -(-target // per_element)), size))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    ap.add_argument("--fused-calls", type=int, default=0, help="run nothing but this many fused calls")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    one = (C.c_uint64 * 16)(*([1] * 16))

    def terms(name, w):
        op = OPS[name]
        outs = range(w + 1) if op <= 2 else range(1)
        return [int(lib.csgn_uint_arith_terms(op, w, one, one, o)) for o in outs]

    for i, (name, w, m, size) in enumerate(shapes(lambda name, w: sum(terms(name, w)) * dl * 8)):
        if args.only >= 0 and i != args.only:
            continue
        op, T = OPS[name], terms(name, w)
        carry = op <= 2
        out_bytes = m * sum(T) * dl * 8
        outs = [hip.empty_words(m * t * dl) for t in T]
        planes_out, carry_out = (outs[:-1], outs[-1]) if carry else (outs, False)
        sets = [[hip.synth_fill(11 + 97 * c + k, n, 0, m * dl) for k in range(2 * w)] for c in range(ROTATE)]

        # the C call itself on host arrays built beforehand: at the small batches the wrapper of csgn_amd/batch.py, which
        # builds them and asks for every term count, would cost more than the launches that are being compared
        vp = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])     # noqa: E731
        h_sets = [(vp(p[:w]), vp(p[w:])) for p in sets]
        h_out, d_carry = vp(planes_out), (carry_out.data_ptr() if carry else None)

        def call(r):
            h_a, h_b = h_sets[r % ROTATE]
            capi.check(lib.csgn_uint_arith(n, op, m, w, h_a, one, h_b, one, h_out, d_carry, hip.stream))

        if args.fused_calls:
            capi.check(lib.csgn_set_tuning(b"uint_arith_form", 1))
            for r in range(args.fused_calls):
                call(r)
            torch.cuda.synchronize()
            print(json.dumps({"op": name, "w": w, "m": m, "fused_calls": args.fused_calls}), flush=True)
            continue
        rec = {"op": name, "w": w, "m": m, "batch": size, "n": n, "carry": carry, "terms": sum(T),
               "written_bytes": out_bytes}
        forms = (("fused", 1), ("chain", 0))
        words = {}
        for form, knob in forms:                      # warm-up of both forms, and their words on the same operands
            capi.check(lib.csgn_set_tuning(b"uint_arith_form", knob))
            rec[form + "_kernel"] = lib.csgn_uint_arith_kernel(n, op, m, w, one, one, int(carry)).decode()
            call(0)
            torch.cuda.synchronize()
            words[form] = [o.clone() for o in outs] if out_bytes <= (2 << 30) else None
        if words["fused"] is not None:
            rec["same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], words["chain"]))
        del words
        times = {"fused": [], "chain": []}
        for r in range(args.reps):                    # in turns, so that a drift of the machine meets both
            for form, knob in forms:
                capi.check(lib.csgn_set_tuning(b"uint_arith_form", knob))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(r + 1)
                e1.record()
                e1.synchronize()
                times[form].append(e0.elapsed_time(e1) * 1e-3)
        for form, _ in forms:
            ts = sorted(times[form])
            rec[form + "_us"] = round(ts[len(ts) // 2] * 1e6, 1)
            rec[form + "_min_us"] = round(ts[0] * 1e6, 1)
            rec[form + "_written_tbps"] = round(out_bytes / ts[len(ts) // 2] * 1e-12, 3)
        rec["speedup"] = round(rec["chain_us"] / rec["fused_us"], 2)
        rec["no_slower"] = "k_uint_arith" if rec["fused_us"] <= MARGIN * rec["chain_us"] else "composed"
        capi.check(lib.csgn_set_tuning(b"uint_arith_form", -1))
        rec["default_kernel"] = lib.csgn_uint_arith_kernel(n, op, m, w, one, one, int(carry)).decode()
        rec["default_is_no_slower"] = rec["default_kernel"] == rec["no_slower"]
        print(json.dumps(rec), flush=True)
        del outs, planes_out, carry_out, sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
