"""The two ends of an encrypted-integer pipeline on the device, end to end (kernels, the copy to or from the host and the
synchronisation, timed by the host clock around work that ends in a synchronise):

  decrypt  UIntBatch::decrypt-equivalent work: csgn_uint_decrypt's one pass (one call, one copy of 8 bytes an element,
           one synchronisation) against the per-plane calls the classes issued before (per plane: csgn_decrypt_uniform,
           a synchronisation, a copy of one byte an element, the host's OR), on fresh planes of width 8, 16 and 64 at
           256, 65 536 and 2^20 elements, on the planes of an 8-bit sum at 4096 and 65 536 elements, and on a 16-bit
           sum at 16 elements (its long planes are cut into chunks: the atomic form).  Half of the terms cover the
           key mask, so the hit path runs.  The planes rotate over several copies; the two routes are timed in turns.
  encrypt  UIntBatch::encrypt's two routes at width 8 and 32, 256 and 2^20 elements: per plane (bit extraction, upload
           and csgn_encrypt_keyed at stream position j * count) against one block (one host pass, one upload, one
           csgn_encrypt_keyed over width * count ciphertexts).

One JSON line per case: the medians and minima of both routes in microseconds, the READ (decrypt) or WRITTEN (encrypt)
bytes per second, whether the results agree, the spread of each route over the rounds and the route this run shows to
be no slower: the one pass where its median is at most the per-plane median plus that route's own spread.

    python tools/bench_uint_decrypt.py [--n 1247] [--reps 15] [--only decrypt|encrypt] [--max-gb 12]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csgn_amd import capi  # noqa: E402
from csgn_amd.batch import HipPath  # noqa: E402

SUM8 = [1, 2, 3, 5, 9, 17, 33, 65, 129]
SUM16 = [2 ** j + 1 for j in range(16)]


def decrypt_shapes():
    out = [("fresh", [1] * w, m) for w in (8, 16, 64) for m in (256, 65536, 1 << 20)]
    out += [("sum8", SUM8, m) for m in (4096, 65536)]
    out.append(("sum16", SUM16, 16))
    return out


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1] - ts[0]


def timed(fn, reps_of):
    t0 = time.perf_counter()
    r = fn(reps_of)
    return r, time.perf_counter() - t0


def bench_decrypt(hip, n, reps, max_bytes):
    lib, dl = hip.lib, hip.default_len(n)
    d = 16 if n >= 1024 else 4
    key = np.random.default_rng(5).permutation(n)[:d].astype(np.uint64)
    dmask = hip.upload(hip.key_mask(n, key))
    for name, T, m in decrypt_shapes():
        w = len(T)
        nbytes = m * sum(T) * dl * 8
        rotate = int(max(1, min(4, max_bytes // nbytes)))
        if nbytes > max_bytes:
            print(json.dumps({"case": "decrypt", "planes": name, "width": w, "elements": m, "skipped": "past --max-gb"}), flush=True)
            continue
        sets = []
        for c in range(rotate):
            planes = []
            for j, t in enumerate(T):
                p = hip.synth_fill(31 + 131 * c + j, n, 0, m * t * dl)
                p.view(-1, dl)[(c + j) % 2::2] |= dmask              # every second term covers the key mask
                planes.append(p)
            sets.append(planes)
        h_terms = (C.c_uint64 * w)(*T)
        h_sets = [(C.c_void_p * w)(*[p.data_ptr() for p in planes]) for planes in sets]
        d_values = hip.empty_words(m)
        h_values = torch.empty(m, dtype=torch.int64, pin_memory=True)
        d_bits = torch.empty(m, dtype=torch.uint8, device=hip.device)
        h_bits = torch.empty(m, dtype=torch.uint8, pin_memory=True)
        scratch = torch.empty(int(lib.csgn_decrypt_scratch_bytes(m, m * max(T))), dtype=torch.uint8, device=hip.device)

        def packed(r):
            capi.check(lib.csgn_uint_decrypt(n, m, w, h_sets[r % rotate], h_terms, None, None, None, dmask.data_ptr(),
                                             d_values.data_ptr(), hip.stream))
            h_values.copy_(d_values, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return h_values.numpy().view(np.uint64)

        def per_plane(r):
            values = np.zeros(m, dtype=np.uint64)
            for j, t in enumerate(T):
                capi.check(lib.csgn_decrypt_uniform(n, m, t, sets[r % rotate][j].data_ptr(), dmask.data_ptr(),
                                                    d_bits.data_ptr(), scratch.data_ptr(), hip.stream))
                h_bits.copy_(d_bits, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                values |= h_bits.numpy().astype(np.uint64) << np.uint64(j)
            return values

        routes = (("one_pass", packed), ("per_plane", per_plane))
        rec = {"case": "decrypt", "planes": name, "width": w, "elements": m, "n": n, "terms": sum(T), "read_bytes": nbytes,
               "rotate": rotate, "kernel": lib.csgn_uint_decrypt_kernel(n, m, w, h_terms).decode()}
        got = {k: f(0).copy() for k, f in routes}                        # warm-up of both, and their values
        rec["same_values"] = bool(np.array_equal(got["one_pass"], got["per_plane"]))
        rec["ones"] = round(float(np.unpackbits(got["one_pass"].view(np.uint8)).sum()) / (m * w), 3)
        times = {k: [] for k, _ in routes}
        for r in range(reps):                                            # in turns, so that a drift meets both
            for k, f in routes:
                times[k].append(timed(f, r + 1)[1])
        for k, _ in routes:
            med, low, spread = stats(times[k])
            rec[k + "_us"], rec[k + "_min_us"], rec[k + "_spread_us"] = round(med * 1e6, 1), round(low * 1e6, 1), round(spread * 1e6, 1)
            rec[k + "_read_tbps"] = round(nbytes / med * 1e-12, 3)
        rec["speedup"] = round(rec["per_plane_us"] / rec["one_pass_us"], 2)
        rec["no_slower"] = "one_pass" if rec["one_pass_us"] <= rec["per_plane_us"] + rec["per_plane_spread_us"] else "per_plane"
        print(json.dumps(rec), flush=True)
        del sets, h_sets, planes
        torch.cuda.empty_cache()


def bench_encrypt(hip, n, reps):
    lib, dl = hip.lib, hip.default_len(n)
    d = 16 if n >= 1024 else 4
    key = np.random.default_rng(5).permutation(n)[:d].astype(np.uint64)
    dkey, dmask = hip.upload(key), hip.upload(hip.key_mask(n, key))
    rng = hip.rng_from_seed(9)
    for w in (8, 32):
        for m in (256, 1 << 20):
            values = np.random.default_rng(w + m).integers(0, 1 << w, size=m, dtype=np.uint64)
            block = hip.empty_words(w * m * dl)
            views = [block[j * m * dl:(j + 1) * m * dl] for j in range(w)]
            other = hip.empty_words(w * m * dl)

            bits = np.empty((w, m), dtype=np.uint8)                      # both routes extract plane by plane into it

            def extract(j):
                np.bitwise_and(values >> np.uint64(j), np.uint64(1), out=bits[j], casting="unsafe")

            def per_plane(_):
                for j in range(w):
                    extract(j)
                    hip.encrypt_keyed(n, d, hip.upload(bits[j]), dkey, dmask, rng, first_ciphertext=j * m, out=views[j])
                torch.cuda.current_stream().synchronize()

            def one_block(_):
                for j in range(w):
                    extract(j)
                hip.encrypt_keyed(n, d, hip.upload(bits.reshape(-1)), dkey, dmask, rng, first_ciphertext=0, out=other)
                torch.cuda.current_stream().synchronize()

            routes = (("one_block", one_block), ("per_plane", per_plane))
            for _, f in routes:
                f(0)
            rec = {"case": "encrypt", "width": w, "elements": m, "n": n, "written_bytes": w * m * dl * 8,
                   "same_words": bool(torch.equal(block, other))}
            times = {k: [] for k, _ in routes}
            for r in range(reps):
                for k, f in routes:
                    times[k].append(timed(f, r)[1])
            for k, _ in routes:
                med, low, spread = stats(times[k])
                rec[k + "_us"], rec[k + "_min_us"], rec[k + "_spread_us"] = round(med * 1e6, 1), round(low * 1e6, 1), round(spread * 1e6, 1)
            rec["speedup"] = round(rec["per_plane_us"] / rec["one_block_us"], 2)
            # the launches alone, plaintext already on the device (HIP events): what is left is the host's share
            d_bits = hip.upload(bits.reshape(-1))
            for k, calls in (("one_block", [(0, w * m, other)]), ("per_plane", [(j * m, m, views[j]) for j in range(w)])):
                ts = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for first, count, out in calls:
                        hip.encrypt_keyed(n, d, d_bits[first:first + count], dkey, dmask, rng, first_ciphertext=first, out=out)
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e-3)
                rec[k + "_launches_us"] = round(stats(ts)[0] * 1e6, 1)
            print(json.dumps(rec), flush=True)
            del block, views, other
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1247)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=("decrypt", "encrypt"), default=None)
    ap.add_argument("--max-gb", type=float, default=12.0, help="the most bytes one copy of a case's planes may take")
    args = ap.parse_args()
    hip = HipPath(0)
    if args.only != "encrypt":
        bench_decrypt(hip, args.n, args.reps, int(args.max_gb * (1 << 30)))
    if args.only != "decrypt":
        bench_encrypt(hip, args.n, args.reps)


if __name__ == "__main__":
    main()
