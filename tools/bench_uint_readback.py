"""The read that follows a write on the device: csgn_uint_pick_rows' fused kernel (k_uint_pick_rows) against the same
words composed row by row from the tuned launchers (knob uint_pick_rows_form = 0) and against an emulation of the
class-level loop readAtEach took over written planes before it -- per row one csgn_uint_plain EQ, per plane the gather
of the row (one strided copy), one csgn_mul_uniform, and the product's placement in the output by ONE strided copy (the
loop's operator+ moves every earlier word again with each row, and its gather and multiply are the ragged ones: the
emulation is a lower bound of that loop).  The arrays have the rows csgn_uint_write leaves from one-term planes.  The
index planes and the arrays rotate over enough copies to pass the 256 MiB memory-side cache.  The words of every timed
form are compared with the fused form's before anything is printed.  One JSON line per case: median microseconds of each
form from HIP events (a sample is four calls queued back to back between two events, their argument arrays built
beforehand: timed()), the bytes written and the algorithmic bytes (outputs written once + operands read once).

    python tools/bench_uint_readback.py [--n 1247] [--reps 10] [--only K]
    python tools/bench_uint_readback.py --ab-rounds 4          # interleaved: fused and composed in turn
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
KNOB = b"uint_pick_rows_form"


def shapes():
    """(width w, index width v, rows n of an array, arrays m): fresh 1-term index planes over tables written once from
    one-term planes, N = 1247, w = 8, each at a small and a large batch (the large one writes about half a gigabyte)."""
    return [(8, 3, 8, 16), (8, 3, 8, 1536), (8, 8, 256, 1), (8, 8, 256, 4)]


def written_rows(v, n):
    """T[r] = 2^zeros(r) * 2 + 1: what csgn_uint_write leaves from one-term value and array planes"""
    return [(1 << sum(1 for k in range(v) if not (r >> k) & 1)) * 2 + 1 for r in range(n)]


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


def prepared_read(hip, n_bits, m, v, w, n, T, sets, srcs, outs):
    """call(i): one csgn_uint_pick_rows on copy i mod copies, its argument arrays built beforehand -- the timed region
    holds the C call and nothing else."""
    vp = C.c_void_p
    h_s = (C.c_uint64 * v)(*([1] * v))
    h_T = (C.c_uint64 * (w * n))(*(T * w))
    h_out = (vp * w)(*[o.data_ptr() for o in outs])
    args = [((vp * v)(*[p.data_ptr() for p in x]), (vp * w)(*[p.data_ptr() for p in a])) for x, a in zip(sets, srcs)]
    lib, stream = hip.lib, hip.stream

    def call(i):
        h_x, h_a = args[i % len(args)]
        capi.check(lib.csgn_uint_pick_rows(n_bits, m, v, h_x, h_s, n, w, h_a, h_T, h_out, stream))
    return call


def loop(hip, n_bits, m, v, w, n, T, src_off, out_off, index, arrays):
    """The class-level loop without the launch: per row equalTo(index, r), per plane the row gathered out of the arrays,
    one multiply, and the product copied once into its block of the output."""
    dl = hip.default_len(n_bits)
    A, Tout = src_off[n], out_off[n]
    outs = [hip.empty_words(m * Tout * dl) for _ in range(w)]
    views = [o.view(m, Tout * dl) for o in outs]
    for r in range(n):
        eq = hip.uint_plain(n_bits, capi.CSGN_UINT_PLAIN_EQ, m, index, [1] * v, r)
        te = eq.numel() // (m * dl)
        for j in range(w):
            row = arrays[j].view(m, A * dl)[:, src_off[r] * dl:src_off[r + 1] * dl].contiguous().view(-1)
            p = hip.mul_uniform(n_bits, m, te, T[r], eq, row)
            views[j][:, out_off[r] * dl:out_off[r + 1] * dl].copy_(p[:m * te * T[r] * dl].view(m, te * T[r] * dl))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="the one shape to run (its position in the list)")
    ap.add_argument("--ab-rounds", type=int, default=0,
                    help="interleaved: time the fused and the composed form in turn, this many rounds")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n_bits = hip.lib, args.n
    dl = hip.default_len(n_bits)
    for k, (w, v, n, m) in enumerate(shapes()):
        if args.only >= 0 and k != args.only:
            continue
        s = (C.c_uint64 * v)(*([1] * v))
        T = written_rows(v, n)
        h_T1 = (C.c_uint64 * n)(*T)
        h_T = (C.c_uint64 * (w * n))(*(T * w))
        so, oo = (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))()
        capi.check(lib.csgn_uint_pick_rows_offsets(v, s, n, h_T1, so, oo))
        src_off, out_off = [int(x) for x in so], [int(x) for x in oo]
        A, Tout = src_off[n], out_off[n]
        capi.check(lib.csgn_uint_pick_rows_check(n_bits, m, v, s, n, w, h_T))
        in_bytes = (v * m + w * m * A) * dl * 8
        copies = max(1, -(-ROTATE_BYTES // in_bytes))
        sets = [[hip.synth_fill(11 + 97 * c + i, n_bits, 0, m * dl) for i in range(v)] for c in range(copies)]
        srcs = [[hip.synth_fill(7 + 89 * c + 31 * j, n_bits, 0, m * A * dl) for j in range(w)] for c in range(copies)]
        outs = [hip.empty_words(m * Tout * dl) for _ in range(w)]
        out_bytes = m * w * Tout * dl * 8
        nbytes = out_bytes + in_bytes
        rec = {"w": w, "v": v, "rows": n, "m": m, "n": n_bits, "A": A, "Tout": Tout, "copies": copies,
               "out_gb": round(out_bytes / 1e9, 3), "bytes": nbytes}
        read = prepared_read(hip, n_bits, m, v, w, n, T, sets, srcs, outs)
        if args.ab_rounds:
            for name in ("fused", "composed"):
                rec[name + "_us"] = []
            for _ in range(args.ab_rounds):
                for name, knob in (("fused", 1), ("composed", 0)):
                    capi.check(lib.csgn_set_tuning(KNOB, knob))
                    rec[name + "_us"].append(round(timed(read, args.reps) * 1e6, 1))
            capi.check(lib.csgn_set_tuning(KNOB, -1))
            rec["fused_vs_composed"] = [round(c / f, 2) for c, f in zip(rec["composed_us"], rec["fused_us"])]
            print(json.dumps(rec), flush=True)
        else:
            words = {}
            for form, knob in (("fused", 1), ("composed", 0)):
                capi.check(lib.csgn_set_tuning(KNOB, knob))
                rec[form + "_kernel"] = lib.csgn_uint_pick_rows_kernel(n_bits, m, v, s, n, w, h_T).decode()
                rec[form + "_us"] = round(timed(read, args.reps) * 1e6, 1)
                read(0)
                torch.cuda.synchronize()
                words[form] = [o.clone() for o in outs] if form == "fused" else outs
            capi.check(lib.csgn_set_tuning(KNOB, -1))
            rec["default_kernel"] = lib.csgn_uint_pick_rows_kernel(n_bits, m, v, s, n, w, h_T).decode()
            rec["composed_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], words["composed"]))
            rec["fused_written_gbps"] = round(out_bytes / rec["fused_us"] * 1e-3, 1)
            rec["fused_tbps"] = round(nbytes / rec["fused_us"] * 1e-6, 2)
            rec["fused_peak_share"] = round(nbytes / rec["fused_us"] * 1e6 / PEAK, 3)
            rec["speedup_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
            words.pop("composed")
            del outs, read
            torch.cuda.empty_cache()
            got = loop(hip, n_bits, m, v, w, n, T, src_off, out_off, sets[0], srcs[0])
            torch.cuda.synchronize()
            rec["loop_same_words"] = all(torch.equal(a, b) for a, b in zip(words["fused"], got))
            del got
            fn = lambda r: loop(hip, n_bits, m, v, w, n, T, src_off, out_off, sets[r % copies], srcs[r % copies])  # noqa: E731
            rec["loop_us"] = round(timed(fn, max(3, args.reps // 3), inner=1) * 1e6, 1)
            rec["speedup_vs_loop"] = round(rec["loop_us"] / rec["fused_us"], 2)
            print(json.dumps(rec), flush=True)
            assert rec["composed_same_words"] and rec["loop_same_words"], \
                "a timed form's words differ from the fused form's"
            del words
        outs = read = None
        del sets, srcs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
