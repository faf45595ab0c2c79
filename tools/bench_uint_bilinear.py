"""A public bilinear form over F2 of two encrypted integers on the device: csgn_uint_bilinear's one launch
(k_uint_bilinear) against the composed sequence a user writes without it, at the C ABI as of the commit before -- two
concatenating gathers (a's planes into one batch, b's into another), then per output plane two csgn_gather that copy
every named operand plane once per pair and one csgn_mul_uniform, into buffers made beforehand (sumGroups is free).  The
sequence writes the operand copies besides the products; its time and its bytes are both reported, and its words are
asserted equal to the launch's.
Workloads at N = 1247, each at about 1 MB and about 1 GB of outputs: clmul(32), clmulWide(32), gfMul(8, 0x11B),
gfMul(64, x^64 + x^4 + x^3 + x + 1), dotBits(64) on fresh planes, and clmul(8) on planes of 4 terms.  The operands rotate
over copies that together pass the 256 MiB memory-side cache; every version is warmed up; the versions are timed in
turns in one process (HIP events, medians of --reps >= 20).  One JSON line per shape and size.

The budgets are compile-time constants of csgn_uint_bilinear.hip, not knobs.  To time other values,
    python tools/bench_uint_bilinear.py --build-variants stage=0,stage=16384,ratio=2,ratio=8,chunk=8192,tile=65536
compiles that one file with -DCSGN_BILINEAR_STAGE_BYTES / _STAGE_RATIO / _MIN_CHUNK / _TILE_UNITS = <value> (stage=0:
nothing is staged) and links each object with the library's other objects into tools/bin/libcsgn_hip_bilinear_<name>.so
(no device needed); a later run times every such library it finds beside the built one, in the same turns.

    python tools/bench_uint_bilinear.py [--n 1247] [--reps 20] [--only I] [--small-only]
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
MACROS = {"stage": "CSGN_BILINEAR_STAGE_BYTES", "ratio": "CSGN_BILINEAR_STAGE_RATIO", "chunk": "CSGN_BILINEAR_MIN_CHUNK",
          "tile": "CSGN_BILINEAR_TILE_UNITS"}


def clmul_wide(w):
    return [[(i, j - i) for i in range(w) if 0 <= j - i < w] for j in range(2 * w - 1)]


def gf_mul(w, poly):
    low = (1 << w) - 1
    red = [1]
    for _ in range(2 * w - 2):
        a = red[-1] << 1
        red.append((a & low) ^ (poly & low) if a >> w else a)
    return [[(i, l) for i in range(w) for l in range(w) if (red[i + l] >> j) & 1] for j in range(w)]


# (name, width, terms per input plane, form)
WORKLOADS = [("clmul32", 32, 1, lambda: clmul_wide(32)[:32]), ("clmulwide32", 32, 1, lambda: clmul_wide(32)),
             ("gfmul8", 8, 1, lambda: gf_mul(8, 0x11B)), ("gfmul64", 64, 1, lambda: gf_mul(64, 0x1B)),
             ("dotbits64", 64, 1, lambda: [[(j, j) for j in range(64)]]), ("clmul8_t4", 8, 4, lambda: clmul_wide(8)[:8])]
SIZES = [("1MB", 1 << 20), ("1GB", 1 << 30)]


def build_variants(specs):
    from csgn_amd import build
    build.build_hip()
    os.makedirs(BIN, exist_ok=True)
    src = os.path.join(build.CSRC, "csgn_uint_bilinear.hip")
    for spec in specs:
        key, value = spec.split("=")
        name = "%s%d" % (key, int(value))
        obj = os.path.join(BIN, "csgn_uint_bilinear_%s.o" % name)
        subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed",
                               "-I" + build.INCLUDE, "-I" + build.CSRC, "-D%s=%d" % (MACROS[key], int(value)), "-c", "-o", obj, src])
        objs = [obj if nm == "csgn_uint_bilinear.hip" else os.path.join(build.OBJDIR, os.path.splitext(nm)[0] + ".o")
                for nm in build.HIP_SOURCES]
        out = os.path.join(BIN, "libcsgn_hip_bilinear_%s.so" % name)
        subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
        print("built", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="index of the one workload to run")
    ap.add_argument("--small-only", action="store_true", help="the 1 MB size alone (a quick look)")
    ap.add_argument("--build-variants", default="", help="comma-separated key=value budgets to build libraries for, then exit")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants(args.build_variants.split(","))
    assert args.reps >= 20

    import torch
    from csgn_amd import capi
    from csgn_amd.batch import HipPath

    u64s = lambda xs: (C.c_uint64 * max(len(xs), 1))(*[int(x) for x in xs])      # noqa: E731
    vps = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])        # noqa: E731
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    st = hip.stream
    libs = [("call", lib)]
    for path in sorted(glob.glob(os.path.join(BIN, "libcsgn_hip_bilinear_*.so"))):
        v = capi.load_library(path)
        capi.check(v.csgn_init(0))
        libs.append(("call_" + re.search(r"bilinear_(\w+)\.so", path).group(1), v))

    for i, (name, w, t, make) in enumerate(WORKLOADS):
        if args.only >= 0 and i != args.only:
            continue
        form = make()
        pairs = [len(p) for p in form]
        assert min(pairs) >= 1
        T = [k * t * t for k in pairs]
        ta = [t] * w
        flat = [p for row in form for p in row]
        first = [0]
        for k in pairs:
            first.append(first[-1] + k)
        h_ta, h_first = u64s(ta), u64s(first)
        h_left, h_right = u64s([a for a, _ in flat]), u64s([b for _, b in flat])
        plans = []
        for nm, v in libs:
            handle = C.c_void_p()
            capi.check(v.csgn_uint_bilinear_create(w, h_ta, w, h_ta, len(form), h_first, h_left, h_right, 0, C.byref(handle)))
            plans.append((nm, v, handle))
        for size_name, target in SIZES[:1] if args.small_only else SIZES:
            m = max(1, target // (sum(T) * dl * 8))
            out_bytes = m * sum(T) * dl * 8
            in_bytes = 2 * m * w * t * dl * 8
            plane_words = m * t * dl
            rotate = min(512, max(2, -(-2 * CACHE // (in_bytes + out_bytes)) if out_bytes < CACHE else 2))
            # one tensor per integer: its planes one after the other, so that the composed form's concat is one copy
            sets = [(hip.synth_fill(11 + 97 * c, n, 0, w * plane_words), hip.synth_fill(12 + 97 * c, n, 0, w * plane_words))
                    for c in range(rotate)]
            planes = [([a[j * plane_words:(j + 1) * plane_words] for j in range(w)],
                       [b[j * plane_words:(j + 1) * plane_words] for j in range(w)]) for a, b in sets]
            outs = [[hip.empty_words(m * tx * dl) for tx in T] for _ in range(min(rotate, 2 if out_bytes >= CACHE else rotate))]
            h_sets = [(vps(a), vps(b)) for a, b in planes]
            h_outs = [vps(o) for o in outs]

            def call_with(v, handle):
                def call(r):
                    h_a, h_b = h_sets[r % rotate]
                    capi.check(v.csgn_uint_bilinear(handle, n, m, h_a, h_b, h_outs[r % len(outs)], st))
                return call

            # the composed sequence: A and B are the concatenated planes (w * m elements of t terms); per plane the
            # gathered operands (m * pairs elements, element e's pairs together) and their element-wise product
            cat_a, cat_b = hip.empty_words(w * plane_words), hip.empty_words(w * plane_words)
            top = max(pairs)
            tmp_l, tmp_r = hip.empty_words(m * top * t * dl), hip.empty_words(m * top * t * dl)
            final = [hip.empty_words(m * tx * dl) for tx in T]
            e = torch.arange(m, dtype=torch.int64, device=hip.device)[:, None]
            index = []
            for row in form:
                li = (torch.tensor([a for a, _ in row], dtype=torch.int64, device=hip.device)[None, :] * m + e).reshape(-1)
                ri = (torch.tensor([b for _, b in row], dtype=torch.int64, device=hip.device)[None, :] * m + e).reshape(-1)
                index.append((li.contiguous(), ri.contiguous()))
            composed_bytes = 2 * w * plane_words * 8 + sum(2 * m * k * t * dl * 8 for k in pairs) + out_bytes

            def composed(r):
                a, b = sets[r % rotate]
                capi.check(lib.csgn_gather(n, w * m, a.data_ptr(), None, t, w * m, None, cat_a.data_ptr(), None, 0, st))
                capi.check(lib.csgn_gather(n, w * m, b.data_ptr(), None, t, w * m, None, cat_b.data_ptr(), None, 0, st))
                for x, k in enumerate(pairs):
                    li, ri = index[x]
                    capi.check(lib.csgn_gather(n, w * m, cat_a.data_ptr(), None, t, m * k, li.data_ptr(), tmp_l.data_ptr(), None, 0, st))
                    capi.check(lib.csgn_gather(n, w * m, cat_b.data_ptr(), None, t, m * k, ri.data_ptr(), tmp_r.data_ptr(), None, 0, st))
                    capi.check(lib.csgn_mul_uniform(n, m * k, t, t, tmp_l.data_ptr(), tmp_r.data_ptr(), final[x].data_ptr(), 0, st))

            def forced_xcd(value):                        # the built library under knob stream_xcd = 0 / 1
                inner = call_with(lib, plans[0][2])

                def call(r):
                    capi.set_tuning("stream_xcd", value)
                    inner(r)
                    capi.set_tuning("stream_xcd", -1)
                return call

            versions = ([(nm, call_with(v, handle), out_bytes) for nm, v, handle in plans] +
                        [("call_xcd%d" % x, forced_xcd(x), out_bytes) for x in (0, 1)] + [("composed", composed, composed_bytes)])
            rec = {"workload": name, "size": size_name, "n": n, "m": m, "width": w, "planes": len(form), "pairs": sum(pairs),
                   "terms_per_input_plane": t, "written_bytes": out_bytes, "composed_written_bytes": composed_bytes,
                   "composed_launch_calls": 2 + 3 * len(form), "rotate": rotate,
                   "launches": hip.uint_bilinear_launches(n, m, ta, ta, form)}
            for _, fn, _ in versions:                     # warm-up of every version, and the words on the same operands
                fn(0)
                torch.cuda.synchronize()
            rec["same_words"] = all(torch.equal(x, y) for x, y in zip(outs[0], final))
            assert rec["same_words"], name
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
                ts = sorted(times[nm])
                rec[nm + "_us"] = round(ts[len(ts) // 2] * 1e6, 1)
                rec[nm + "_min_us"] = round(ts[0] * 1e6, 1)
                rec[nm + "_written_tbps"] = round(written / ts[len(ts) // 2] * 1e-12, 3)
            rec["speedup_over_composed"] = round(rec["composed_us"] / rec["call_us"], 2)
            print(json.dumps(rec), flush=True)
            del sets, planes, outs, final, versions, h_sets, h_outs, cat_a, cat_b, tmp_l, tmp_r, index
            torch.cuda.empty_cache()
        for _, v, handle in plans:
            v.csgn_uint_bilinear_destroy(handle)


if __name__ == "__main__":
    main()
