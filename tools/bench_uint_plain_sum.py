"""Ranges, sets and step functions on the device: csgn_uint_plain_sum's one launch (k_uint_plain_sum) against the launch
sequence a caller writes without it -- csgn_uint_plain per entry into a temporary of its own, then the csgn_add_uniform
chain that copies the running sum once per link (and once more for a + ONE), as of the commit before, into buffers
made beforehand.  The loop writes MORE bytes; its time and its bytes are both reported.
Workloads at N = 1247 on fresh planes, each at about 1 MB and about 1 GB of outputs: an 8-bit range, a 32-bit range,
isIn with 16 keys at w = 16, an 8-threshold bucketOf at w = 16, lookupSparse with 64 keys at w = 32 into 8 planes (keys
of four zero bits: a comparison's terms double with every zero bit of an EQ key, csgn_uint_plain's cost, not this
kernel's).  Beside them, the largest single comparison of the workload through csgn_uint_plain (k_uint_plain) and
through a one-entry plan of this kernel, in the same run: their shares of the 8 TB/s peak side by side.
The operands rotate over copies that together pass the 256 MiB memory-side cache; every version is warmed up; the
versions are timed in turns in one process (HIP events, medians of --reps >= 10).  One JSON line per shape and size.

    python tools/bench_uint_plain_sum.py [--n 1247] [--reps 10] [--only I] [--small-only]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CACHE = 256 << 20
PEAK = 8e12
EQ, NE, LT, LE, GT, GE = range(1, 7)


def step_planes(thresholds, values, out_width):
    planes = [[(LT, t) for i, t in enumerate(thresholds) if ((values[i] ^ values[i + 1]) >> j) & 1] for j in range(out_width)]
    return planes, values[-1] & ((1 << out_width) - 1)


def sparse_planes(keys, values, out_width):
    return [[(EQ, k) for k, v in sorted(zip(keys, values)) if (v >> j) & 1] for j in range(out_width)], 0


def workloads():
    rng = random.Random(37)
    keys16 = sorted(rng.sample(range(1 << 16), 16))
    keys32 = sorted({0xFFFFFFFF ^ sum(1 << b for b in rng.sample(range(32), 4)) for _ in range(80)})[:64]
    values = [rng.randrange(1, 256) for _ in keys32]
    return [("range8", 8, [[(LT, 201), (LT, 17)]], 0),
            ("range32", 32, [[(LT, 0xC0000000), (LT, 0x00FF0000)]], 0),
            ("isin16", 16, [[(EQ, k) for k in keys16]], 0),
            ("bucket8", 16) + step_planes([4096 + 7000 * i for i in range(8)], list(range(9)), 4),
            ("sparse64", 32) + sparse_planes(keys32, values, 8)]


SIZES = [("1MB", 1 << 20), ("1GB", 1 << 30)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=-1, help="index of the one workload to run")
    ap.add_argument("--small-only", action="store_true", help="the 1 MB size alone (a quick look)")
    args = ap.parse_args()
    assert args.reps >= 10

    import torch
    from csgn_amd import capi
    from csgn_amd.batch import HipPath

    u64s = lambda xs: (C.c_uint64 * max(len(xs), 1))(*[int(x) for x in xs])     # noqa: E731
    vps = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])        # noqa: E731
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    st = hip.stream

    for i, (name, w, planes, constant) in enumerate(workloads()):
        if args.only >= 0 and i != args.only:
            continue
        h_ta = u64s([1] * w)
        terms = [[int(lib.csgn_uint_plain_terms(c, w, k, h_ta)) for c, k in entries] for entries in planes]
        assert all(all(t) for t in terms)
        T = [sum(t) + ((constant >> x) & 1) if t else 1 for x, t in enumerate(terms)]
        entries_all = [(c, k, t) for entries, ts in zip(planes, terms) for (c, k), t in zip(entries, ts)]
        big = max(entries_all, key=lambda e: e[2])
        for size_name, target in SIZES[:1] if args.small_only else SIZES:
            m = max(1, target // (sum(T) * dl * 8))
            out_bytes = m * sum(T) * dl * 8
            in_bytes = m * w * dl * 8
            rotate = min(256, max(2, -(-2 * CACHE // (in_bytes + out_bytes)) if out_bytes < CACHE else 2))
            sets = [[hip.synth_fill(11 + 97 * c + j, n, 0, m * dl) for j in range(w)] for c in range(rotate)]
            outs = [[hip.empty_words(m * t * dl) for t in T] for _ in range(min(rotate, 2 if out_bytes >= CACHE else rotate))]
            h_sets, h_outs = [vps(s) for s in sets], [vps(o) for o in outs]
            handle = hip.uint_plain_sum_create([1] * w, planes, constant)
            single = hip.uint_plain_sum_create([1] * w, [[big[:2]]], 0)
            single_out = hip.empty_words(m * big[2] * dl)
            h_single = vps([single_out])

            def call(r):
                capi.check(lib.csgn_uint_plain_sum(handle, n, m, h_sets[r % rotate], h_outs[r % len(outs)], st))

            def single_sum(r):
                capi.check(lib.csgn_uint_plain_sum(single, n, m, h_sets[r % rotate], h_single, st))

            def single_plain(r):
                capi.check(lib.csgn_uint_plain(n, big[0], m, w, big[1], h_sets[r % rotate], h_ta, single_out.data_ptr(), st))

            # the loop: every entry into a temporary of its own, then the chain; the last link of a plane writes `final`
            one = hip.const_fill(n, m, None, 1)
            temps = [[hip.empty_words(m * t * dl) for t in ts] for ts in terms]
            most = max(T)
            ping = [hip.empty_words(m * most * dl) for _ in range(2)]
            final = [hip.empty_words(m * t * dl) for t in T]
            loop_bytes, loop_calls = 0, 0
            for x, ts in enumerate(terms):
                if not ts:                                # a constant plane: one fill
                    loop_calls += 1
                    loop_bytes += m * dl * 8
                    continue
                links = ts[1:] + ([1] if (constant >> x) & 1 else [])
                loop_calls += len(ts) + len(links)
                loop_bytes += sum(ts) * m * dl * 8        # every comparison once
                acc = ts[0]
                for t in links:                           # every link writes the running sum again
                    acc += t
                    loop_bytes += acc * m * dl * 8

            def loop(r):
                src = h_sets[r % rotate]
                for x, (entries, ts) in enumerate(zip(planes, terms)):
                    bit = (constant >> x) & 1
                    if not ts:
                        capi.check(lib.csgn_const_fill(n, m, None, bit, final[x].data_ptr(), st))
                        continue
                    rights = [(temps[x][e], ts[e]) for e in range(1, len(ts))] + ([(one, 1)] if bit else [])
                    for e, (c, k) in enumerate(entries):
                        dst = final[x] if e == 0 and not rights else temps[x][e]
                        capi.check(lib.csgn_uint_plain(n, c, m, w, k, src, h_ta, dst.data_ptr(), st))
                    cur, acc = temps[x][0], ts[0]
                    for q, (right, t) in enumerate(rights):
                        dst = final[x] if q == len(rights) - 1 else ping[q % 2]
                        capi.check(lib.csgn_add_uniform(n, m, acc, t, cur.data_ptr(), right.data_ptr(), dst.data_ptr(), st))
                        cur, acc = dst, acc + t

            versions = [("call", call, out_bytes), ("loop", loop, loop_bytes),
                        ("single_sum", single_sum, m * big[2] * dl * 8), ("single_plain", single_plain, m * big[2] * dl * 8)]
            rec = {"workload": name, "size": size_name, "n": n, "m": m, "width": w, "planes": len(planes),
                   "entries": len(entries_all), "terms": sum(T), "written_bytes": out_bytes, "loop_written_bytes": loop_bytes,
                   "loop_launch_calls": loop_calls, "rotate": rotate, "largest_entry_terms": big[2],
                   "launches": hip.uint_plain_sum_launches(n, m, [1] * w, planes, constant)}
            for _, fn, _ in versions:                     # warm-up of every version, and the words on the same operands
                fn(0)
                torch.cuda.synchronize()
            rec["same_words"] = all(torch.equal(x, y) for x, y in zip(outs[0], final))
            times = {nm: [] for nm, _, _ in versions}
            order_rng = random.Random(1)
            for r in range(args.reps):                    # in turns, each turn in an order of its own (seeded)
                turn = list(versions)
                order_rng.shuffle(turn)
                for nm, fn, _ in turn:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(r + 1)
                    e1.record()
                    e1.synchronize()
                    times[nm].append(e0.elapsed_time(e1) * 1e-3)
            for nm, _, written in versions:
                t = sorted(times[nm])
                rec[nm + "_us"] = round(t[len(t) // 2] * 1e6, 1)
                rec[nm + "_min_us"] = round(t[0] * 1e6, 1)
                rec[nm + "_written_tbps"] = round(written / t[len(t) // 2] * 1e-12, 3)
                rec[nm + "_share_of_peak"] = round(written / t[len(t) // 2] / PEAK, 3)
            rec["speedup_over_loop"] = round(rec["loop_us"] / rec["call_us"], 2)
            print(json.dumps(rec), flush=True)
            lib.csgn_uint_plain_sum_destroy(handle)
            lib.csgn_uint_plain_sum_destroy(single)
            del sets, outs, temps, ping, final, versions, h_sets, h_outs, single_out, one
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
