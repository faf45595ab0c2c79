"""Encrypted arrays written at encrypted indices on the device: csgn_uint_write's fused kernel (k_uint_write) against the
same words composed row by row from the tuned launchers (knob uint_write_fused = 0), against an emulation of the loop a
user writes at the class level without it -- per row one csgn_uint_plain EQ and one gather of the row, per plane one
logicMux gate, and the placement of every row in the arrays' layout by ONE strided copy (concat and the permuting
gather of the class level move every word twice: the emulation is a lower bound of that loop) -- and, in bytes written
per second, against k_uint_pick EACH (readAtEach) of the same (v, n, w, t): the same E stream and the same tables.  The
index planes and the operands rotate over enough copies to pass the 256 MiB memory-side cache.  The words of every timed
form are compared with the fused form's before anything is printed.  One JSON line per case: median microseconds of each
form from HIP events (a sample is four calls queued back to back between two events, their argument arrays built
beforehand: timed()), the bytes written and the algorithmic bytes (outputs written once + operands read once).

    python tools/bench_uint_write.py [--n 1247] [--reps 10] [--only K]
    python tools/bench_uint_write.py --ab-rounds 4          # interleaved: fused write, composed write and pick EACH in turn
    python tools/bench_uint_write.py --only 0 --fused-calls 20      # nothing but 20 fused writes and 20 picks (kernel trace)
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
PICK_EACH = 5


def shapes():
    """(width w, index width v, rows n of an array, terms t of every value and array plane, arrays m): fresh 1-term index
    planes; the batches write about half a gigabyte."""
    return [(8, 4, 16, 1, 2048), (8, 8, 256, 1, 32), (32, 5, 32, 1, 192), (8, 3, 8, 3, 2048)]


def timed(fn, reps, inner=4):
    """Median of `reps` samples; a sample is `inner` calls queued back to back between two HIP events, divided by
    `inner`, so that the host's work for a call (the launch itself included) overlaps the call before it instead of
    being timed with an idle GPU.  fn(i) takes a running call number, which the callers turn into the operand copy."""
    for i in range(3):                                  # steady state: the first calls of a form run slower
        fn(i)
    torch.cuda.synchronize()
    ts, i = [], 3
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn(i)
            i += 1
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / inner)
    ts.sort()
    return ts[len(ts) // 2]


def prepared_write(hip, n_bits, m, v, w, n, t, sets, vals, srcs, outs):
    """call(i): one csgn_uint_write on copy i mod copies, its argument arrays built beforehand -- the timed region holds
    the C call and nothing else."""
    vp = C.c_void_p
    h_s = (C.c_uint64 * v)(*([1] * v))
    h_t = (C.c_uint64 * w)(*([t] * w))
    h_out = (vp * w)(*[o.data_ptr() for o in outs])
    args = [((vp * v)(*[p.data_ptr() for p in x]), (vp * w)(*[p.data_ptr() for p in val]),
             (vp * w)(*[p.data_ptr() for p in a])) for x, val, a in zip(sets, vals, srcs)]
    lib, stream = hip.lib, hip.stream

    def call(i):
        h_x, h_v, h_a = args[i % len(args)]
        capi.check(lib.csgn_uint_write(n_bits, m, v, h_x, h_s, n, w, h_v, h_t, h_a, h_t, h_out, stream))
    return call


def prepared_pick(hip, n_bits, m, v, w, n, t, sets, srcs, outs):
    """call(i): one csgn_uint_pick EACH over the same index planes and arrays."""
    vp = C.c_void_p
    h_s = (C.c_uint64 * v)(*([1] * v))
    h_out = (vp * w)(*[o.data_ptr() for o in outs])
    args = [((vp * v)(*[p.data_ptr() for p in x]), (vp * w)(*[p.data_ptr() for p in a])) for x, a in zip(sets, srcs)]
    lib, stream = hip.lib, hip.stream

    def call(i):
        h_x, h_a = args[i % len(args)]
        capi.check(lib.csgn_uint_pick(n_bits, PICK_EACH, m, v, h_x, h_s, w, n, h_a, t, h_out, stream))
    return call


def today(hip, n_bits, m, v, w, n, t, index, value, arrays, lists, offsets, A):
    """The class-level loop without the write: per row equalTo(index, r), the gather of the row, one logicMux a plane,
    and every row copied once into its place in the arrays' layout."""
    dl = hip.default_len(n_bits)
    outs = [hip.empty_words(m * A * dl) for _ in range(w)]
    views = [o.view(m, A * dl) for o in outs]
    for r in range(n):
        eq = hip.uint_plain(n_bits, capi.CSGN_UINT_PLAIN_EQ, m, index, [1] * v, r)
        te = eq.numel() // (m * dl)
        rows = hip.gather_planes(n_bits, arrays, [t] * w, m * n, m, lists[r])
        for j in range(w):
            mux = hip.gate_uniform(n_bits, capi.CSGN_GATE_MUX, m, value[j], t, rows[j], t, eq, te)
            tr = te * 2 * t + t
            views[j][:, offsets[r] * dl:(offsets[r] + tr) * dl].copy_(mux[:m * tr * dl].view(m, tr * dl))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="the one shape to run (its position in the list)")
    ap.add_argument("--ab-rounds", type=int, default=0,
                    help="interleaved: time the fused write, the composed write and pick EACH in turn, this many rounds")
    ap.add_argument("--fused-calls", type=int, default=0,
                    help="run nothing but this many fused writes and this many picks (for a kernel trace)")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n_bits = hip.lib, args.n
    dl = hip.default_len(n_bits)
    for k, (w, v, n, t, m) in enumerate(shapes()):
        if args.only >= 0 and k != args.only:
            continue
        s = (C.c_uint64 * v)(*([1] * v))
        tt = (C.c_uint64 * w)(*([t] * w))
        E = int(lib.csgn_uint_read_terms(v, s, n))
        offsets = [int(lib.csgn_uint_write_offset(v, s, n, r, t, t)) for r in range(n + 1)]
        A = offsets[n]
        assert A == E * 2 * t + n * t
        in_bytes = (v * m + w * m * t + w * m * n * t) * dl * 8
        copies = max(1, -(-ROTATE_BYTES // in_bytes))
        sets = [[hip.synth_fill(11 + 97 * c + i, n_bits, 0, m * dl) for i in range(v)] for c in range(copies)]
        vals = [[hip.synth_fill(5 + 83 * c + 29 * j, n_bits, 0, m * t * dl) for j in range(w)] for c in range(copies)]
        srcs = [[hip.synth_fill(7 + 89 * c + 31 * j, n_bits, 0, m * n * t * dl) for j in range(w)] for c in range(copies)]
        lists = [torch.arange(m, dtype=torch.int64, device="cuda") * n + r for r in range(n)]
        outs = [hip.empty_words(m * A * dl) for _ in range(w)]
        pouts = [hip.empty_words(m * t * E * dl) for _ in range(w)]
        out_bytes = m * w * A * dl * 8
        pick_bytes = m * w * t * E * dl * 8
        nbytes = out_bytes + in_bytes
        rec = {"w": w, "v": v, "rows": n, "t": t, "m": m, "n": n_bits, "E": E, "A": A, "copies": copies,
               "out_gb": round(out_bytes / 1e9, 3), "pick_out_gb": round(pick_bytes / 1e9, 3), "bytes": nbytes}
        write = prepared_write(hip, n_bits, m, v, w, n, t, sets, vals, srcs, outs)
        pick = prepared_pick(hip, n_bits, m, v, w, n, t, sets, srcs, pouts)
        if args.fused_calls:
            capi.check(lib.csgn_set_tuning(b"uint_write_fused", 1))
            for i in range(args.fused_calls):
                write(i)
            for i in range(args.fused_calls):
                pick(i)
            torch.cuda.synchronize()
            print(json.dumps({"w": w, "v": v, "rows": n, "t": t, "m": m, "fused_calls_each": args.fused_calls}),
                  flush=True)
        elif args.ab_rounds:
            for name in ("fused", "composed", "pick"):
                rec[name + "_us"] = []
            for _ in range(args.ab_rounds):
                for name, knob, fn in (("fused", 1, write), ("composed", 0, write), ("pick", -1, pick)):
                    capi.check(lib.csgn_set_tuning(b"uint_write_fused", knob))
                    rec[name + "_us"].append(round(timed(fn, args.reps) * 1e6, 1))
            capi.check(lib.csgn_set_tuning(b"uint_write_fused", -1))
            rec["fused_written_gbps"] = [round(out_bytes / us * 1e-3, 1) for us in rec["fused_us"]]
            rec["pick_written_gbps"] = [round(pick_bytes / us * 1e-3, 1) for us in rec["pick_us"]]
            rec["fused_vs_composed"] = [round(c / f, 2) for c, f in zip(rec["composed_us"], rec["fused_us"])]
            print(json.dumps(rec), flush=True)
        else:
            words = {}
            for form, knob in (("fused", 1), ("composed", 0)):
                capi.check(lib.csgn_set_tuning(b"uint_write_fused", knob))
                rec[form + "_kernel"] = lib.csgn_uint_write_kernel(n_bits, m, v, s, n, w, tt, tt).decode()
                rec[form + "_us"] = round(timed(write, args.reps) * 1e6, 1)
                write(0)
                torch.cuda.synchronize()
                words[form] = [o.clone() for o in outs] if form == "fused" else outs
            capi.check(lib.csgn_set_tuning(b"uint_write_fused", -1))
            rec["default_kernel"] = lib.csgn_uint_write_kernel(n_bits, m, v, s, n, w, tt, tt).decode()
            rec["composed_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], words["composed"]))
            rec["pick_us"] = round(timed(pick, args.reps) * 1e6, 1)
            rec["fused_written_gbps"] = round(out_bytes / rec["fused_us"] * 1e-3, 1)
            rec["pick_written_gbps"] = round(pick_bytes / rec["pick_us"] * 1e-3, 1)
            rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
            rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
            rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
            words.pop("composed")
            del outs, pouts, write, pick
            torch.cuda.empty_cache()
            got = today(hip, n_bits, m, v, w, n, t, sets[0], vals[0], srcs[0], lists, offsets, A)
            torch.cuda.synchronize()
            rec["today_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], got))
            del got
            fn = lambda r: today(hip, n_bits, m, v, w, n, t, sets[r % copies], vals[r % copies], srcs[r % copies],  # noqa: E731
                                 lists, offsets, A)
            rec["today_us"] = round(timed(fn, max(3, args.reps // 3), inner=1) * 1e6, 1)
            rec["speedup_vs_today"] = round(rec["today_us"] / rec["fused_us"], 2)
            print(json.dumps(rec), flush=True)
            assert rec["composed_same_words"] and rec["today_same_words"], \
                "a timed form's words differ from the fused form's"
            del words
        outs = pouts = write = pick = None
        del sets, vals, srcs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
