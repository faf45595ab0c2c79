"""Products of encrypted bit matrices on the device: csgn_matmul's fused kernel (k_matmul) against the same words from
the composed form (knob matmul_form = 0: both operands tiled by the gather launcher, one uniform multiply), and against
the mark -- csgn_mul_uniform alone on operands tiled beforehand, writing the same bytes.  The operands rotate over enough
copies to pass the 256 MiB memory-side cache.  One JSON line per case: median microseconds of each form from HIP events,
the algorithmic bytes (output written once + operands read once), every form's share of 8 TB/s, and "today": the
launches and copied bytes of the per-pair Ciphertext::operator* / operator+ loop, computed, not timed.

    python tools/bench_matmul.py [--n 1247] [--reps 7] [--only INDEX]
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


def shapes():
    """(name, rows, inner, cols, t_a, t_b, transposed)."""
    return [("square", 256, 256, 256, 1, 1, False), ("matrix-vector", 4096, 4096, 1, 1, 1, False),
            ("many inner products", 1024, 64, 1024, 1, 1, True), ("multi-term", 64, 64, 64, 2, 2, False),
            ("one dot", 1, 1 << 20, 1, 1, 1, False)]


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


def tile_indices(hip, rows, inner, cols, transposed):
    p = torch.arange(rows * cols * inner, dtype=torch.int64, device=hip.device)
    e, ik = p % inner, p // inner
    i, k = ik // cols, ik % cols
    return i * inner + e, (k * inner + e) if transposed else (e * cols + k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", type=int, default=-1, help="index of the one shape to run")
    args = ap.parse_args()
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    for x, (name, rows, inner, cols, ta, tb, tr) in enumerate(shapes()):
        if args.only >= 0 and x != args.only:
            continue
        T = inner * ta * tb
        a_words, b_words, out_words = rows * inner * ta * dl, inner * cols * tb * dl, rows * cols * T * dl
        copies = max(1, min(8, -(-ROTATE_BYTES // ((a_words + b_words) * 8))))
        A = [hip.synth_fill(11 + 97 * c, n, 0, a_words) for c in range(copies)]
        B = [hip.synth_fill(13 + 89 * c, n, 0, b_words) for c in range(copies)]
        out = hip.empty_words(out_words)
        nbytes = (out_words + a_words + b_words) * 8
        rec = {"shape": name, "rows": rows, "inner": inner, "cols": cols, "t_a": ta, "t_b": tb, "transposed": tr, "n": n,
               "out_gb": round(out_words * 8 / 1e9, 3), "bytes": nbytes}
        call = lambda r: hip.matmul(n, rows, inner, cols, A[r % copies], ta, B[r % copies], tb, tr, out=out)  # noqa: E731
        fused = None
        for form, knob in (("fused", 1), ("composed", 0)):
            capi.set_tuning("matmul_form", knob)
            rec[form + "_kernel"] = lib.csgn_matmul_kernel(n, rows, inner, cols, ta, tb, int(tr)).decode()
            rec[form + "_us"] = round(timed(call, args.reps if knob else max(3, args.reps // 2)) * 1e6, 1)
            rec[form + "_peak_share"] = round(nbytes / rec[form + "_us"] * 1e6 / PEAK, 3)
            call(0)
            torch.cuda.synchronize()
            if form == "fused":
                fused = out.clone()
            else:
                rec["composed_same_words"] = bool(torch.equal(fused, out))
        capi.set_tuning("matmul_form", -1)
        rec["default_kernel"] = lib.csgn_matmul_kernel(n, rows, inner, cols, ta, tb, int(tr)).decode()
        # the mark: one uniform multiply over operands tiled beforehand
        ia, ib = tile_indices(hip, rows, inner, cols, tr)
        pairs = rows * cols * inner
        tiled_a = hip.gather(n, rows * inner, A[0], ta, pairs, ia)
        tiled_b = hip.gather(n, inner * cols, B[0], tb, pairs, ib)
        del ia, ib
        rec["mark_us"] = round(timed(lambda r: hip.mul_uniform(n, pairs, ta, tb, tiled_a, tiled_b, out=out), args.reps) * 1e6, 1)
        torch.cuda.synchronize()
        rec["mark_same_words"] = bool(torch.equal(fused, out))
        rec["mark_bytes"] = (out_words + pairs * (ta + tb) * dl) * 8
        rec["fused_vs_composed"] = round(rec["composed_us"] / rec["fused_us"], 2)
        rec["fused_vs_mark"] = round(rec["mark_us"] / rec["fused_us"], 2)
        # today: per output element `inner` products and inner - 1 sums, every sum a copy of the running sum and the product
        term_bytes = ta * tb * dl * 8
        rec["today_launches"] = rows * cols * (2 * inner - 1)
        rec["today_copied_bytes"] = rows * cols * term_bytes * (inner + sum(e + 1 for e in range(1, inner)))
        print(json.dumps(rec), flush=True)
        del A, B, out, fused, tiled_a, tiled_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
