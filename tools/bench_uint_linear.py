"""A public matrix over F2 on the device: csgn_uint_linear's one launch (k_uint_linear) against the launch sequence of
the XOR chain a user writes without it -- a ^ b over publicly re-indexed operands, link after link through
csgn_uint_bitwise as of the commit before, into buffers made beforehand.  The chain copies the running sum once per
link, so it writes MORE bytes; its time and its bytes are both reported.
Workloads at N = 1247 on fresh planes, each at about 1 MB and about 1 GB of outputs: SHA-256's sigma 0 (row weight 3),
AES MixColumns, the CRC-32 eight-step matrix (dense) and a random 64 x 64 matrix.  The operands rotate over copies that
together pass the 256 MiB memory-side cache; every version is warmed up; the versions are timed in turns in one
process (HIP events, medians of --reps >= 20).  One JSON line per shape and size.

The tile budget is a compile-time constant of csgn_uint_linear.hip, not a knob.  To time other budgets,
    python tools/bench_uint_linear.py --build-variants 16384,262144
compiles that one file with -DCSGN_LINEAR_TILE_UNITS=<units> and links each object with the library's other objects
into tools/bin/libcsgn_hip_tile<units>.so (no device needed); a later run times every such library it finds beside the
built one, in the same turns.

    python tools/bench_uint_linear.py [--n 1247] [--reps 20] [--only I] [--small-only]
"""
import argparse
import ctypes as C
import glob
import json
import os
import random
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "tools", "bin")
CACHE = 256 << 20


def bits_of(mask):
    return [i for i in range(64) if (mask >> i) & 1]


def from_columns(w, image):
    cols = [image(i) for i in range(w)]
    return [sum(((cols[i] >> j) & 1) << i for i in range(w)) for j in range(w)]


def sigma0():
    return [(1 << ((j + 7) % 32)) | (1 << ((j + 18) % 32)) | ((1 << (j + 3)) if j + 3 < 32 else 0) for j in range(32)]


def xtime(v):
    return ((v << 1) ^ (0x1B if v & 0x80 else 0)) & 0xFF


def mix_columns():
    def image(i):
        c, x = divmod(i, 8)
        v = 1 << x
        f = {1: v, 2: xtime(v), 3: xtime(v) ^ v}
        return sum(f[[2, 3, 1, 1][(c - r) % 4]] << (8 * r) for r in range(4))
    return from_columns(32, image)


def crc32_step8():
    def image(i):
        c = 1 << i
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
        return c
    return from_columns(32, image)


def random64():
    import numpy as np
    return [int(x) for x in np.random.default_rng(64).integers(0, 2**64, 64, dtype=np.uint64)]


WORKLOADS = [("sigma0", 32, sigma0), ("mixcolumns", 32, mix_columns), ("crc32x8", 32, crc32_step8), ("random64", 64, random64)]
SIZES = [("1MB", 1 << 20), ("1GB", 1 << 30)]


def build_variants(units):
    from csgn_amd import build
    build.build_hip()
    os.makedirs(BIN, exist_ok=True)
    src = os.path.join(build.CSRC, "csgn_uint_linear.hip")
    for u in units:
        obj = os.path.join(BIN, "csgn_uint_linear_tile%d.o" % u)
        subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed",
                               "-I" + build.INCLUDE, "-I" + build.CSRC, "-DCSGN_LINEAR_TILE_UNITS=%d" % u, "-c", "-o", obj, src])
        objs = [obj if name == "csgn_uint_linear.hip" else os.path.join(build.OBJDIR, os.path.splitext(name)[0] + ".o")
                for name in build.HIP_SOURCES]
        out = os.path.join(BIN, "libcsgn_hip_tile%d.so" % u)
        subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
        print("built", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="index of the one workload to run")
    ap.add_argument("--small-only", action="store_true", help="the 1 MB size alone (a quick look)")
    ap.add_argument("--build-variants", default="", help="comma-separated tile budgets to build libraries for, then exit")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants([int(x) for x in args.build_variants.split(",")])
    assert args.reps >= 20

    import torch
    from csgn_amd import capi
    from csgn_amd.batch import HipPath

    u64s = lambda xs: (C.c_uint64 * len(xs))(*[int(x) for x in xs])              # noqa: E731
    vps = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])        # noqa: E731
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    st = hip.stream
    libs = [("call", lib)]
    for path in sorted(glob.glob(os.path.join(BIN, "libcsgn_hip_tile*.so"))):
        v = capi.load_library(path)
        capi.check(v.csgn_init(0))
        libs.append(("call_tile%s" % re.search(r"tile(\d+)", path).group(1), v))
    plan0 = hip.uint_linear_plan(n, 1, [1], [1])
    budget = plan0[6]

    for i, (name, w, make) in enumerate(WORKLOADS):
        if args.only >= 0 and i != args.only:
            continue
        rows = make()
        weights = [len(bits_of(r)) for r in rows]
        assert min(weights) >= 1
        T = sum(weights)
        for size_name, target in SIZES[:1] if args.small_only else SIZES:
            m = max(1, target // (T * dl * 8))
            out_bytes = m * T * dl * 8
            in_bytes = m * w * dl * 8
            rotate = min(512, max(2, -(-2 * CACHE // (in_bytes + out_bytes)) if out_bytes < CACHE else 2))
            sets = [[hip.synth_fill(11 + 97 * c + j, n, 0, m * dl) for j in range(w)] for c in range(rotate)]
            outs = [[hip.empty_words(m * t * dl) for t in weights] for _ in range(min(rotate, 2 if out_bytes >= CACHE else rotate))]
            h_sets, h_outs = [vps(s) for s in sets], [vps(o) for o in outs]
            h_ta, h_rows = u64s([1] * w), u64s(rows)

            def call_with(v):
                def call(r):
                    capi.check(v.csgn_uint_linear(n, m, w, h_sets[r % rotate], h_ta, len(rows), h_rows, 0,
                                                  h_outs[r % len(outs)], st))
                return call

            # the chain: link k adds the (k + 1)-th named plane to the running sum of every row that has one, the rows
            # of fewer bits having left; two buffers a row take turns, the last link of a row writes its final buffer
            top = max(weights)
            ping = [[hip.empty_words(m * min(top - 1, wt) * dl) if wt > 2 else None for wt in weights] for _ in range(2)]
            final = [hip.empty_words(m * wt * dl) for wt in weights]
            links = []                                    # (rows still active, ta, written bytes)
            for k in range(1, top):
                active = [j for j, wt in enumerate(weights) if wt > k]
                links.append((active, k, m * (k + 1) * dl * 8 * len(active)))
            chain_bytes = sum(b for _, _, b in links) + sum(m * dl * 8 for wt in weights if wt == 1)
            one = u64s([1] * 64)

            named = [bits_of(r) for r in rows]
            chain_args = []                               # per operand set: every link's host arrays, made beforehand
            for planes in sets:
                per_set = []
                for active, k, _ in links:
                    a = [planes[named[j][0]] if k == 1 else ping[k % 2][j] for j in active]
                    b = [planes[named[j][k]] for j in active]
                    o = [final[j] if weights[j] == k + 1 else ping[(k + 1) % 2][j] for j in active]
                    per_set.append((len(active), vps(a), u64s([k] * len(active)), vps(b), vps(o)))
                chain_args.append(per_set)

            def chain(r):
                planes = sets[r % rotate]
                for j, wt in enumerate(weights):          # a row of one bit: today a shared payload; here a copy, so
                    if wt == 1:                           # that both versions write every plane
                        capi.check(lib.csgn_memcpy_d2d(final[j].data_ptr(), planes[named[j][0]].data_ptr(), m * dl * 8, st))
                for width, h_a, h_ka, h_b, h_o in chain_args[r % rotate]:
                    capi.check(lib.csgn_uint_bitwise(n, 3, m, width, None, 0, h_a, h_ka, h_b, one, h_o, st))

            def forced_xcd(value):                        # the built library under knob stream_xcd = 0 / 1
                inner = call_with(lib)

                def call(r):
                    capi.set_tuning("stream_xcd", value)
                    inner(r)
                    capi.set_tuning("stream_xcd", -1)
                return call

            versions = ([(nm, call_with(v), out_bytes) for nm, v in libs] +
                        [("call_xcd%d" % x, forced_xcd(x), out_bytes) for x in (0, 1)] + [("chain", chain, chain_bytes)])
            rec = {"workload": name, "size": size_name, "n": n, "m": m, "in_width": w, "rows": len(rows),
                   "mean_row_weight": round(T / len(rows), 2), "written_bytes": out_bytes, "chain_written_bytes": chain_bytes,
                   "chain_launch_calls": len(links), "rotate": rotate, "tile_units": budget,
                   "plan": hip.uint_linear_plan(n, m, [1] * w, rows)}
            for _, fn, _ in versions:                     # warm-up of every version, and the words on the same operands
                fn(0)
                torch.cuda.synchronize()
            rec["same_words"] = all(torch.equal(x, y) for x, y in zip(outs[0], final))
            times = {nm: [] for nm, _, _ in versions}
            order_rng = random.Random(1)
            for r in range(args.reps):                    # in turns, so that a drift of the machine meets all of them; each
                turn = list(versions)                     # turn in an order of its own (seeded), because a version pays
                order_rng.shuffle(turn)                   # for the writes the one before it left in flight
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
            rec["speedup_over_chain"] = round(rec["chain_us"] / rec["call_us"], 2)
            print(json.dumps(rec), flush=True)
            del sets, outs, ping, final, versions, h_sets, h_outs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
