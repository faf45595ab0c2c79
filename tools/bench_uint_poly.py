"""A public polynomial over F2 of encrypted planes on the device: csgn_uint_poly's one launch (k_uint_poly) against what
a user writes without it, at the C ABI as of the commit before:
  composed   one concatenating gather of all input planes, then per output plane and per degree d present (ascending) d
             csgn_gather that copy every named plane once per monomial and d - 1 csgn_mul_uniform, then csgn_add_uniform
             between the degree groups, into buffers and index lists made beforehand (sumGroups is free).  Its words are
             asserted equal to the launch's.
  bitwise    for ch, maj and chi the chain of csgn_uint_bitwise calls a user writes today ((e & f) ^ (~e & g), ...); its
             words differ, so it is only timed.
  linear / bilinear   csgn_uint_linear and csgn_uint_bilinear on forms they can express (sigma0, clmul(32),
             gfMul(8, 0x11B)); their words are asserted equal to the launch's.
Workloads at N = 1247, each at about 1 MB and about 1 GB of outputs.  The operands rotate over copies that together
pass the 256 MiB memory-side cache; every version is warmed up; the versions are timed in turns in one process, each
turn in a seeded order of its own (HIP events, medians of --reps >= 20).  One JSON line per shape and size.

The budgets are compile-time constants of csgn_uint_poly.hip, not knobs.  To time other values,
    python tools/bench_uint_poly.py --build-variants stage=0,stage=8192,ratio=2,chunk=8192,tile=65536
compiles that one file with -DCSGN_POLY_STAGE_BYTES / _STAGE_RATIO / _MIN_CHUNK / _TILE_UNITS = <value> (stage=0: nothing
is staged) and links each object with the library's other objects into tools/bin/libcsgn_hip_poly_<name>.so (no device
needed); a later run times every such library it finds beside the built one, in the same turns.

    python tools/bench_uint_poly.py [--n 1247] [--reps 20] [--only I] [--small-only]
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
MACROS = {"stage": "CSGN_POLY_STAGE_BYTES", "ratio": "CSGN_POLY_STAGE_RATIO", "chunk": "CSGN_POLY_MIN_CHUNK",
          "tile": "CSGN_POLY_TILE_UNITS"}


def canon(monomials):
    return sorted({tuple(sorted(set(m))) for m in monomials}, key=lambda m: (len(m), m))


def f_ch(w):
    return [canon([(j, w + j), (j, 2 * w + j), (2 * w + j,)]) for j in range(w)]


def f_maj(w):
    return [canon([(j, w + j), (j, 2 * w + j), (w + j, 2 * w + j)]) for j in range(w)]


def f_chi(w):
    return [canon([(j,), (2 * w + j,), (w + j, 2 * w + j)]) for j in range(w)]


def f_simon(w):
    """One Simon round on (x, y, k): y ^ (x <<< 1 & x <<< 8) ^ x <<< 2 ^ k."""
    rot = lambda j, s: (j - s) % w                                                # noqa: E731
    return [canon([(w + j,), (rot(j, 1), rot(j, 8)), (rot(j, 2),), (2 * w + j,)]) for j in range(w)]


def f_random(n_in, n_out, per, seed):
    rng = random.Random(seed)
    rows = []
    for _ in range(n_out):
        row = set()
        while len(row) < per:
            row.add(tuple(sorted(rng.sample(range(n_in), rng.randint(1, 3)))))
        rows.append(canon(row))
    return rows


def clmul_pairs(w):
    return [[(i, j - i) for i in range(j + 1)] for j in range(w)]


def gf_mul_pairs(w, poly):
    low = (1 << w) - 1
    red = [1]
    for _ in range(2 * w - 2):
        a = red[-1] << 1
        red.append((a & low) ^ (poly & low) if a >> w else a)
    return [[(i, l) for i in range(w) for l in range(w) if (red[i + l] >> j) & 1] for j in range(w)]


def sigma0_rows(w=32):
    rot = lambda j, s: (j + s) % w                                                # noqa: E731
    return [(1 << rot(j, 7)) ^ (1 << rot(j, 18)) ^ ((1 << (j + 3)) if j + 3 < w else 0) for j in range(w)]


# (name, input planes, terms per input plane, form, extra): extra = ("bitwise", kind, w) | ("linear", rows) |
# ("bilinear", pairs, wa) | None
WORKLOADS = [
    ("ch32", 96, 1, lambda: f_ch(32), ("bitwise", "ch", 32)),
    ("maj32", 96, 1, lambda: f_maj(32), ("bitwise", "maj", 32)),
    ("chi64", 192, 1, lambda: f_chi(64), ("bitwise", "chi", 64)),
    ("simon64", 96, 1, lambda: f_simon(32), None),
    ("andall32x4", 128, 1, lambda: [[tuple(o * 32 + j for o in range(4))] for j in range(32)], None),
    ("random256", 256, 1, lambda: f_random(256, 64, 32, 7), None),
    ("ch8_t4", 24, 4, lambda: f_ch(8), ("bitwise", "ch", 8)),
    ("sigma0", 32, 1, lambda: [[(i,) for i in range(32) if (r >> i) & 1] for r in sigma0_rows()], ("linear", sigma0_rows())),
    ("clmul32", 64, 1, lambda: [[(i, 32 + l) for i, l in p] for p in clmul_pairs(32)], ("bilinear", clmul_pairs(32), 32)),
    ("gfmul8", 16, 1, lambda: [[(i, 8 + l) for i, l in p] for p in gf_mul_pairs(8, 0x11B)], ("bilinear", gf_mul_pairs(8, 0x11B), 8)),
]
SIZES = [("1MB", 1 << 20), ("1GB", 1 << 30)]


def build_variants(specs):
    from csgn_amd import build
    build.build_hip()
    os.makedirs(BIN, exist_ok=True)
    src = os.path.join(build.CSRC, "csgn_uint_poly.hip")
    for spec in specs:
        key, value = spec.split("=")
        name = "%s%d" % (key, int(value))
        obj = os.path.join(BIN, "csgn_uint_poly_%s.o" % name)
        subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed",
                               "-I" + build.INCLUDE, "-I" + build.CSRC, "-D%s=%d" % (MACROS[key], int(value)), "-c", "-o", obj, src])
        objs = [obj if nm == "csgn_uint_poly.hip" else os.path.join(build.OBJDIR, os.path.splitext(nm)[0] + ".o")
                for nm in build.HIP_SOURCES]
        out = os.path.join(BIN, "libcsgn_hip_poly_%s.so" % name)
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

    vps = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])        # noqa: E731
    hip = HipPath(0)
    lib, n = hip.lib, args.n
    dl = hip.default_len(n)
    st = hip.stream
    libs = [("call", lib)]
    for path in sorted(glob.glob(os.path.join(BIN, "libcsgn_hip_poly_*.so"))):
        v = capi.load_library(path)
        capi.check(v.csgn_init(0))
        libs.append(("call_" + re.search(r"poly_(\w+)\.so", path).group(1), v))

    for i, (name, n_in, t, make, extra) in enumerate(WORKLOADS):
        if args.only >= 0 and i != args.only:
            continue
        form = make()
        assert all(row and row == canon(row) for row in form)
        terms = [t] * n_in
        T = [sum(t ** len(mo) for mo in row) for row in form]
        h_terms, h_first, h_mfirst, h_factor = hip._poly_arrays(terms, form)
        plans = []
        for nm, v in libs:
            handle = C.c_void_p()
            capi.check(v.csgn_uint_poly_create(n_in, h_terms, len(form), h_first, h_mfirst, h_factor, 0, C.byref(handle)))
            plans.append((nm, v, handle))
        for size_name, target in SIZES[:1] if args.small_only else SIZES:
            m = max(1, target // (sum(T) * dl * 8))
            out_bytes = m * sum(T) * dl * 8
            in_bytes = m * n_in * t * dl * 8
            plane_words = m * t * dl
            rotate = min(512, max(2, -(-2 * CACHE // (in_bytes + out_bytes)) if out_bytes < CACHE else 2))
            # one tensor for all planes, one after the other, so that the composed form's concat is one copy
            sets = [hip.synth_fill(11 + 97 * c, n, 0, n_in * plane_words) for c in range(rotate)]
            planes = [[a[j * plane_words:(j + 1) * plane_words] for j in range(n_in)] for a in sets]
            outs = [[hip.empty_words(m * tx * dl) for tx in T] for _ in range(min(rotate, 2 if out_bytes >= CACHE else rotate))]
            h_sets = [vps(p) for p in planes]
            h_outs = [vps(o) for o in outs]

            def call_with(v, handle):
                def call(r):
                    capi.check(v.csgn_uint_poly(handle, n, m, h_sets[r % rotate], h_outs[r % len(outs)], st))
                return call

            # the composed sequence
            cat = hip.empty_words(n_in * plane_words)
            final = [hip.empty_words(m * tx * dl) for tx in T]
            e = torch.arange(m, dtype=torch.int64, device=hip.device)[:, None]
            steps, composed_bytes, calls, most = [], n_in * plane_words * 8, 1, 0
            for x, row in enumerate(form):
                groups = []
                for d in sorted({len(mo) for mo in row}):
                    monos = [mo for mo in row if len(mo) == d]
                    idx = [(torch.tensor([mo[k] for mo in monos], dtype=torch.int64, device=hip.device)[None, :] * m + e)
                           .reshape(-1).contiguous() for k in range(d)]
                    groups.append((d, len(monos), idx))
                    most = max(most, len(monos) * t ** d)
                    composed_bytes += m * len(monos) * dl * 8 * (d * t + sum(t ** (k + 1) for k in range(1, d)))
                    calls += 2 * d - 1
                composed_bytes += sum(m * tx * dl * 8 for tx in [T[x]] * (len(groups) - 1))
                calls += len(groups) - 1
                steps.append(groups)
            tmp = [hip.empty_words(m * most * dl) for _ in range(3)]
            grp = [hip.empty_words(m * most * dl) for _ in range(max(len(g) for g in steps))]
            acc = [hip.empty_words(m * max(T) * dl) for _ in range(2)]

            def composed(r):
                capi.check(lib.csgn_gather(n, n_in * m, sets[r % rotate].data_ptr(), None, t, n_in * m, None, cat.data_ptr(), None, 0, st))
                for x, groups in enumerate(steps):
                    for gi, (d, k, idx) in enumerate(groups):
                        dest = final[x] if len(groups) == 1 else grp[gi]
                        cur, tc = (dest if d == 1 else tmp[0]), t
                        capi.check(lib.csgn_gather(n, n_in * m, cat.data_ptr(), None, t, m * k, idx[0].data_ptr(), cur.data_ptr(), None, 0, st))
                        for f in range(1, d):
                            capi.check(lib.csgn_gather(n, n_in * m, cat.data_ptr(), None, t, m * k, idx[f].data_ptr(), tmp[1].data_ptr(), None, 0, st))
                            nxt = dest if f == d - 1 else (tmp[2] if cur is tmp[0] else tmp[0])
                            capi.check(lib.csgn_mul_uniform(n, m * k, tc, t, cur.data_ptr(), tmp[1].data_ptr(), nxt.data_ptr(), 0, st))
                            cur, tc = nxt, tc * t
                    run, tr = grp[0], groups[0][1] * t ** groups[0][0]
                    for gi in range(1, len(groups)):
                        tg = groups[gi][1] * t ** groups[gi][0]
                        nxt = final[x] if gi == len(groups) - 1 else acc[gi % 2]
                        capi.check(lib.csgn_add_uniform(n, m, tr, tg, run.data_ptr(), grp[gi].data_ptr(), nxt.data_ptr(), st))
                        run, tr = nxt, tr + tg

            versions = [(nm, call_with(v, handle), out_bytes) for nm, v, handle in plans] + [("composed", composed, composed_bytes)]
            same = [("composed", final)]
            if extra and extra[0] == "bitwise":
                _, kind, w = extra
                ops = lambda p: [p[o * w:(o + 1) * w] for o in range(3)]            # noqa: E731
                tt = [t] * w
                b1 = [hip.empty_words(m * t * t * dl) for _ in range(w)]
                b2 = [hip.empty_words(m * max(t * t, t + 1) * dl) for _ in range(w)]
                b3 = [hip.empty_words(m * (t + 1) * t * dl) for _ in range(w)]
                b4 = [hip.empty_words(m * (3 * t * t + t) * dl) for _ in range(w)]
                b5 = [hip.empty_words(m * 3 * t * t * dl) for _ in range(w)]

                def bitwise(r):
                    a, b, c = ops(planes[r % rotate])
                    if kind == "ch":                      # (e & f) ^ (~e & g)
                        hip.uint_bitwise(n, 1, m, a, tt, b, tt, outs=b1)
                        hip.uint_bitwise(n, 4, m, a, tt, outs=b2)
                        hip.uint_bitwise(n, 1, m, b2, [t + 1] * w, c, tt, outs=b3)
                        hip.uint_bitwise(n, 3, m, b1, [t * t] * w, b3, [(t + 1) * t] * w, outs=b4)
                    elif kind == "maj":                   # (a & b) ^ (a & c) ^ (b & c)
                        hip.uint_bitwise(n, 1, m, a, tt, b, tt, outs=b1)
                        hip.uint_bitwise(n, 1, m, a, tt, c, tt, outs=b2)
                        hip.uint_bitwise(n, 1, m, b, tt, c, tt, outs=b3)
                        hip.uint_bitwise(n, 3, m, b1, [t * t] * w, b2, [t * t] * w, outs=b4)
                        hip.uint_bitwise(n, 3, m, b4, [2 * t * t] * w, b3, [t * t] * w, outs=b5)
                    else:                                 # a ^ (~b & c)
                        hip.uint_bitwise(n, 4, m, b, tt, outs=b2)
                        hip.uint_bitwise(n, 1, m, b2, [t + 1] * w, c, tt, outs=b3)
                        hip.uint_bitwise(n, 3, m, a, tt, b3, [(t + 1) * t] * w, outs=b4)

                versions.append(("bitwise", bitwise, 0))
            elif extra and extra[0] == "linear":
                lin = [hip.empty_words(m * tx * dl) for tx in T]
                versions.append(("linear", lambda r: hip.uint_linear(n, m, planes[r % rotate], terms, extra[1], 0, outs=lin), out_bytes))
                same.append(("linear", lin))
            elif extra and extra[0] == "bilinear":
                bil = [hip.empty_words(m * tx * dl) for tx in T]
                wa = extra[2]
                handle_b = hip.uint_bilinear_create(terms[:wa], terms[wa:], extra[1], 0)
                versions.append(("bilinear", lambda r: hip.uint_bilinear_apply(handle_b, n, m, planes[r % rotate][:wa],
                                                                               planes[r % rotate][wa:], len(form), outs=bil), out_bytes))
                same.append(("bilinear", bil))
            rec = {"workload": name, "size": size_name, "n": n, "m": m, "inputs": n_in, "planes": len(form),
                   "monomials": sum(len(row) for row in form), "terms_per_input_plane": t, "written_bytes": out_bytes,
                   "read_bytes": in_bytes, "composed_written_bytes": composed_bytes, "composed_launch_calls": calls, "rotate": rotate,
                   "launches": hip.uint_poly_launches(n, m, terms, form)}
            for _, fn, _ in versions:                     # warm-up of every version, and the words on the same operands
                fn(0)
                torch.cuda.synchronize()
            for nm, got in same:
                rec["same_words_" + nm] = all(torch.equal(x, y) for x, y in zip(outs[0], got))
                assert rec["same_words_" + nm], (name, nm)
            times = {nm: [] for nm, _, _ in versions}
            order_rng = random.Random(1)
            for r in range(args.reps):                    # in turns, each in a seeded order of its own
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
                ts = sorted(times[nm])
                rec[nm + "_us"] = round(ts[len(ts) // 2] * 1e6, 1)
                rec[nm + "_min_us"] = round(ts[0] * 1e6, 1)
                if written:
                    rec[nm + "_written_tbps"] = round(written / ts[len(ts) // 2] * 1e-12, 3)
            rec["speedup_over_composed"] = round(rec["composed_us"] / rec["call_us"], 2)
            print(json.dumps(rec), flush=True)
            if extra and extra[0] == "bilinear":
                lib.csgn_uint_bilinear_destroy(handle_b)
            del sets, planes, outs, final, versions, h_sets, h_outs, cat, tmp, grp, acc, steps, same
            torch.cuda.empty_cache()
        for _, v, handle in plans:
            v.csgn_uint_poly_destroy(handle)


if __name__ == "__main__":
    main()
