"""Gates on the device: csgn_gate_uniform against the same gate composed from the existing entry points
(csgn_add_uniform / csgn_mul_uniform / csgn_const_fill, one intermediate buffer per step).  One JSON line per case:
median time of each form from HIP events, the algorithmic bytes (operands read once + output written once) and the
fused form's share of 8 TB/s.

    python tools/bench_gates.py [--n 1247] [--batch 1048576] [--reps 20]
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
NAMES = {capi.CSGN_GATE_NOT: "not", capi.CSGN_GATE_XNOR: "xnor", capi.CSGN_GATE_NAND: "nand", capi.CSGN_GATE_OR: "or",
         capi.CSGN_GATE_NOR: "nor", capi.CSGN_GATE_MUX: "mux", capi.CSGN_GATE_ADD_PLAIN: "add_plain",
         capi.CSGN_GATE_MUL_PLAIN: "mul_plain"}
BINARY = (capi.CSGN_GATE_XNOR, capi.CSGN_GATE_NAND, capi.CSGN_GATE_OR, capi.CSGN_GATE_NOR, capi.CSGN_GATE_MUX)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


def composed(hip, n, gate, batch, ts, ta, tb, s, a, b, plain, one, pc):
    """The definition, step by step through the existing entry points (ONE / the plain constants made beforehand)."""
    add = lambda x, tx, y, ty: hip.add_uniform(n, batch, tx, ty, x, y)
    mul = lambda x, tx, y, ty: hip.mul_uniform(n, batch, tx, ty, x, y)
    if gate == capi.CSGN_GATE_NOT:
        return add(a, ta, one, 1)
    if gate == capi.CSGN_GATE_XNOR:
        return add(add(a, ta, b, tb), ta + tb, one, 1)
    if gate == capi.CSGN_GATE_NAND:
        return add(mul(a, ta, b, tb), ta * tb, one, 1)
    if gate == capi.CSGN_GATE_OR:
        return add(add(a, ta, b, tb), ta + tb, mul(a, ta, b, tb), ta * tb)
    if gate == capi.CSGN_GATE_NOR:
        return add(add(add(a, ta, b, tb), ta + tb, mul(a, ta, b, tb), ta * tb), ta + tb + ta * tb, one, 1)
    if gate == capi.CSGN_GATE_MUX:
        return add(mul(s, ts, add(a, ta, b, tb), ta + tb), ts * (ta + tb), b, tb)
    if gate == capi.CSGN_GATE_ADD_PLAIN:
        return add(a, ta, pc, 1)
    return mul(a, ta, pc, 1)


def case(hip, n, gate, batch, ts, ta, tb, reps, fused):
    dl = hip.default_len(n)
    words = lambda t: hip.empty_words(batch * t * dl).random_()
    s, a = words(ts), words(ta)
    b = words(tb) if gate in BINARY else None
    plain = torch.randint(0, 2, (batch,), dtype=torch.uint8, device=hip.device)
    one = hip.const_fill(n, batch, None, 1)
    pc = hip.const_fill(n, batch, plain)
    capi.set_tuning("gate_fused", fused)
    kernel = hip.lib.csgn_gate_uniform_kernel(n, gate, batch, ts, ta, tb).decode()
    t_gate = timed(lambda: hip.gate_uniform(n, gate, batch, a, ta, b, tb, s, ts, plain), reps)
    capi.set_tuning("gate_fused", -1)
    t_comp = timed(lambda: composed(hip, n, gate, batch, ts, ta, tb, s, a, b, plain, one, pc), reps)
    terms = int(hip.lib.csgn_gate_terms(gate, ts, ta, tb))
    read = {capi.CSGN_GATE_MUX: ts + ta + tb}.get(gate, ta + tb if gate in BINARY else ta)
    nbytes = batch * (read + terms) * dl * 8 + (batch if gate in (capi.CSGN_GATE_ADD_PLAIN, capi.CSGN_GATE_MUL_PLAIN) else 0)
    return {"gate": NAMES[gate], "n": n, "batch": batch, "shape": [ts, ta, tb], "kernel": kernel,
            "gate_s": t_gate, "composed_s": t_comp, "speedup": t_comp / t_gate, "bytes": nbytes,
            "gate_tbps": nbytes / t_gate / 1e12, "frac_of_8tbps": nbytes / t_gate / PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="also both forms (gate_fused 0 / 1) of OR over a range of shapes")
    args = ap.parse_args()
    hip = HipPath(0)
    for gate in NAMES:
        print(json.dumps(case(hip, args.n, gate, args.batch, 1, 1, 1, args.reps, -1)), flush=True)
    for gate in (capi.CSGN_GATE_OR, capi.CSGN_GATE_NAND):
        print(json.dumps(case(hip, args.n, gate, 4096, 1, 64, 64, args.reps, -1)), flush=True)
    if args.sweep:
        for ta, tb, batch in ((2, 2, 1 << 18), (4, 4, 1 << 16), (4, 5, 1 << 16), (8, 8, 1 << 14), (16, 16, 1 << 12),
                              (64, 64, 4096)):
            for fused in (0, 1):
                r = case(hip, args.n, capi.CSGN_GATE_OR, batch, 1, ta, tb, args.reps, fused)
                r["forced"] = fused
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
