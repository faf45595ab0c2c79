// csgn_gather.hip -- gather, tile and broadcast of ciphertext batches: output element e is a bit-for-bit copy of source
// element idx[e] (tile: e mod count_in), include/csgn_hip.h's definition.  Pure data movement, bound by HBM.
// Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md (section 4.16).
#include "csgn_device.h"

#include <algorithm>

namespace csgn {

namespace {

// ---------------------------------------------------------------------------------------------- uniform sources
// The grid walks the flattened output of every plane: a workgroup owns kGatherK * 256 consecutive units of ONE plane
// (16 bytes when dL is even and every pointer is 16-byte aligned, else 8: the convention of add_uniform and
// k_copy_list), lane l the units l, l + 256, ..., so every wave-level store is 1 KiB (or 512 B) of contiguous output.
// A plane's units start on a workgroup boundary: plane j owns the workgroups [first[j], first[j + 1]) of a virtual
// grid that launches slice at launch_blocks().  A lane finds its element by a FastDiv of its unit inside the workgroup's
// first element (the workgroup's first element is one 64-bit division, paid once per workgroup), so outputs past 2^32
// units need no special case.  The lanes of one element load the same index word: one request per wave and element.
constexpr u32 kGatherK = 4;                           // units per lane: four loads in flight before the first store
constexpr u32 kGatherBlockUnits = 256u * kGatherK;

struct GatherArgs {
    const void *src[kGatherMaxPlanes];
    void *dst[kGatherMaxPlanes];
    u64 first[kGatherMaxPlanes + 1];                  // virtual workgroup where plane j starts; first[n_planes]: the end
    FastDivTable<kGatherMaxPlanes> eu;                // units per element of plane j (t_j * U)
    const u64 *idx;                                   // nullptr: tile, idx[e] = e mod count_in
    u64 block_base;                                   // virtual workgroup of this launch's workgroup 0
    u32 count_in, count_out;
    FastDiv d_in;                                     // by count_in (tile)
    u32 n_planes;
    u32 xcd;                                          // XCD-contiguous workgroup order (stream_xcd)
};

template <typename Unit>
__global__ void __launch_bounds__(256) k_gather(GatherArgs a)
{
    const u32 b = a.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const u64 vb = a.block_base + b;
    // plane of this workgroup: largest j with first[j] <= vb (workgroup-uniform: scalar loads, at most 6 steps)
    u32 lo = 0, hi = a.n_planes;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (a.first[mid] <= vb)
            lo = mid;
        else
            hi = mid;
    }
    const u32 j = lo;
    const FastDiv deu = a.eu.at(j);
    const u32 eu = deu.d;
    const Unit *__restrict__ src = reinterpret_cast<const Unit *>(a.src[j]);
    Unit *__restrict__ dst = reinterpret_cast<Unit *>(a.dst[j]);
    const u64 units = (u64)a.count_out * eu;
    const u64 u0 = (vb - a.first[j]) * kGatherBlockUnits;          // this workgroup's first unit inside plane j
    const u64 e0 = u0 / eu;
    const u32 r0 = (u32)(u0 - e0 * eu);                            // < eu < 2^31
    u64 from[kGatherK];
    bool live[kGatherK];
#pragma unroll
    for (u32 m = 0; m < kGatherK; ++m) {
        const u32 r = r0 + m * 256u + threadIdx.x;
        const u32 de = csgn_fastdiv(r, deu);
        const u32 k = r - de * eu;
        const u64 e = e0 + de;
        live[m] = u0 + m * 256u + threadIdx.x < units;
        // lanes past the plane's end read the last element's index (in range) and store nothing
        const u32 ec = live[m] ? (u32)e : a.count_out - 1u;
        u64 s;
        if (a.idx)
            s = a.idx[ec];
        else
            s = ec - csgn_fastdiv(ec, a.d_in) * a.count_in;
        // an index past the source is never followed: its element is not written, its lane reads unit 0 of the
        // source (the host refuses count_in == 0 with a nonempty output, so unit 0 exists)
        live[m] = live[m] && s < a.count_in;
        from[m] = live[m] ? s * eu + k : 0ull;
    }
    Unit v[kGatherK];
#pragma unroll
    for (u32 m = 0; m < kGatherK; ++m)
        v[m] = src[from[m]];
#pragma unroll
    for (u32 m = 0; m < kGatherK; ++m)
        asm volatile("" : "+v"(v[m]));                             // every load issued before the first store
#pragma unroll
    for (u32 m = 0; m < kGatherK; ++m)
        if (live[m])
            unit_store<Unit, true>(dst + u0 + m * 256u + threadIdx.x, v[m]);
}

// ------------------------------------------------------------------------------------------------ ragged sources
// CSR source, CSR output (offsets from csgn_gather_plan).  The skeleton of k_add_ragged_flat with one operand: the grid
// covers the flattened output, a workgroup owns C consecutive chunks of 256 units, its first element comes from a 64-ary
// wave search of the output offsets.  Per chunk it bets on the element it was in (scalar loads); when that element does
// not hold the whole chunk it stages the next 256 elements in LDS -- output offset, source start and source length,
// each one coalesced (offsets, indices) or gathered (source offsets) load per thread -- and every lane finds its element
// by an LDS binary search.  Because a workgroup owns a fixed stretch of OUTPUT, one huge element among many small ones
// is cut into many workgroups' worth of work and small elements are packed 256 to a window: skew costs no idle waves
// (the split-long-lists rule of the scatter/gather guidance).
constexpr u32 kGatherWin = 256;
constexpr u64 kBadStart = ~0ull;

template <typename Unit, int C>
__global__ void __launch_bounds__(256) k_gather_ragged(const Unit *__restrict__ src, const u64 *__restrict__ src_off,
                                                       u32 count_in, const u64 *__restrict__ idx,
                                                       Unit *__restrict__ dst, const u64 *__restrict__ out_off,
                                                       u32 count_out, u64 unit_base, u64 total_units, u32 U, FastDiv dU,
                                                       FastDiv d_in)
{
    __shared__ u64 w_o[kGatherWin + 1], w_s[kGatherWin], w_n[kGatherWin];
    __shared__ u32 s_next;
    const u64 g_begin = unit_base + (u64)blockIdx.x * (256u * C);
    if (g_begin >= total_units)
        return;
    const u64 term0 = g_begin / U;
    const u32 r0blk = (u32)(g_begin - term0 * U);
    u32 pw = wave_find(out_off, 0u, count_out, term0);             // the same answer in every wave
    auto source_of = [&](u32 e, u64 &start, u64 &len) {            // source start and length of output element e
        const u64 ix = idx ? idx[e] : (u64)(e - csgn_fastdiv(e, d_in) * count_in);
        if (ix < count_in) {
            start = src_off[ix];
            len = src_off[ix + 1] - start;
        } else {
            start = kBadStart;
            len = 0;
        }
    };
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const u64 c_begin = g_begin + (u32)c * 256u;
        if (c_begin >= total_units)
            break;
        const u64 c_end = min(c_begin + 256u, total_units);
        const u64 last_term = term0 + csgn_fastdiv(r0blk + (u32)(c_end - g_begin) - 1u, dU);
        const u64 o0 = out_off[pw], o1 = out_off[pw + 1];
        const bool whole = last_term < o1;                         // workgroup-uniform
        u64 s0 = 0, n0 = 0;
        if (whole)
            source_of(pw, s0, n0);
        else {
            const u32 i = threadIdx.x;
            const u32 p = min(pw + i, count_out - 1u);
            w_o[i] = out_off[min(pw + i, count_out)];
            if (i == 0)
                w_o[kGatherWin] = out_off[min(pw + kGatherWin, count_out)];
            u64 st, ln;
            source_of(p, st, ln);
            w_s[i] = st;
            w_n[i] = ln;
            __syncthreads();
        }
        const u64 g = c_begin + threadIdx.x;
        const bool in_range = g < total_units;
        const u32 back = in_range ? 0u : (u32)(g - (total_units - 1u));   // past the end: redo the last unit, store nothing
        const u32 r = r0blk + (u32)c * 256u + threadIdx.x - back;
        const u32 dt = csgn_fastdiv(r, dU);
        const u64 term = term0 + dt;
        const u32 k = r - dt * U;
        u32 p = pw;
        u64 ostart = o0, sstart = s0, slen = n0;
        if (!whole) {
            // largest j in [0, kGatherWin] with w_o[j] <= term
            u32 lo = 0, hi = kGatherWin + 1u;
#pragma unroll
            for (int step = 0; step < 9; ++step) {
                const u32 mid = (lo + hi) >> 1;
                const bool le = w_o[mid] <= term;
                lo = le ? mid : lo;
                hi = le ? hi : mid;
            }
            if (lo == kGatherWin) {                                // beyond the window (long runs of empty elements)
                p = csr_gallop(out_off, pw + kGatherWin, count_out, term);
                ostart = out_off[p];
                source_of(p, sstart, slen);
            } else {
                p = pw + lo;
                ostart = w_o[lo];
                sstart = w_s[lo];
                slen = w_n[lo];
            }
        }
        const u64 q = term - ostart;                               // term inside the element
        const bool ok = in_range && sstart != kBadStart && q < slen;
        const Unit v = src[ok ? (sstart + q) * U + k : 0ull];
        if (ok)
            unit_store<Unit, true>(dst + g, v);
        if (!whole) {
            if (threadIdx.x == 255u)
                s_next = p;
            __syncthreads();
            pw = s_next;
        }
    }
}

// --------------------------------------------------------------------------------------------------------- plan
// Two passes, one kernel.  CHECK (scan = 0): every index is compared with count_in; the wave's count of bad ones goes
// to stat[0] by one atomic.  SCAN (scan = 1, ragged sources): the exclusive prefix sums of the gathered elements'
// term counts, written as the output offsets -- one workgroup per 4096 elements takes a ticket, scans its elements and
// gets the sum of every chunk before it by the decoupled look-back of csgn_device.h (the pattern of k_plan in
// csgn_mul.hip), so the offsets are written once and never leave the device.  The scan pass reads stat[0] first and
// writes nothing when the check found a bad index.  stat = [bad][total][ticket][one look-back granule per chunk].
constexpr u32 kGPlanThreads = 1024, kGPlanPer = 4, kGPlanChunk = kGPlanThreads * kGPlanPer;
constexpr u32 kGPlanStatus = 3;

__global__ void __launch_bounds__(kGPlanThreads) k_gather_plan(u32 scan, u32 count_in, const u64 *__restrict__ src_off,
                                                                 u32 count_out, const u64 *__restrict__ idx, FastDiv d_in,
                                                                 u64 *__restrict__ out_off, u64 *__restrict__ stat)
{
    constexpr u32 kWaves = kGPlanThreads / kWave;
    const u32 tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    if (!scan) {
        u32 bad = 0;
        for (u64 e = (u64)blockIdx.x * kGPlanThreads + tid; e < count_out; e += (u64)gridDim.x * kGPlanThreads)
            bad += idx[e] >= count_in ? 1u : 0u;
        for (u32 d = 32; d > 0; d >>= 1)
            bad += __shfl_xor(bad, d, kWave);
        if (lane == 0 && bad)
            atomicAdd(reinterpret_cast<unsigned long long *>(stat), (unsigned long long)bad);
        return;
    }
    __shared__ u64 wtot[kWaves], s_prefix;
    __shared__ u32 s_chunk, s_bad;
    if (tid == 0) {
        s_bad = __hip_atomic_load(stat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;
        s_chunk = atomicAdd(reinterpret_cast<u32 *>(stat + 2), 1u);     // chunks in the order they started
    }
    __syncthreads();
    if (s_bad)
        return;                                                    // (every workgroup: nobody waits for another)
    const u32 chunk = s_chunk;
    const u64 b0 = (u64)chunk * kGPlanChunk + (u64)tid * kGPlanPer;
    u64 t[kGPlanPer], mine = 0;
#pragma unroll
    for (u32 i = 0; i < kGPlanPer; ++i) {
        const u64 e = b0 + i;
        t[i] = 0;
        if (e < count_out) {
            const u64 ix = idx ? idx[e] : (u64)((u32)e - csgn_fastdiv((u32)e, d_in) * count_in);
            if (ix < count_in)
                t[i] = src_off[ix + 1] - src_off[ix];
        }
        mine += t[i];
    }
    u64 incl = mine;
    for (u32 d = 1; d < kWave; d <<= 1) {
        const u64 nb = (u64)__shfl_up(incl, d, kWave);
        if (lane >= d)
            incl += nb;
    }
    if (lane == kWave - 1)
        wtot[wv] = incl;
    __syncthreads();
    u64 wbase = 0, all = 0;
    for (u32 w = 0; w < kWaves; ++w) {
        wbase += w < wv ? wtot[w] : 0ull;
        all += wtot[w];
    }
    if (wv == 0) {
        const u64 excl = lookback(stat + kGPlanStatus, chunk, all);
        if (lane == 0)
            s_prefix = excl;
    }
    __syncthreads();
    u64 run = s_prefix + wbase + incl - mine;
#pragma unroll
    for (u32 i = 0; i < kGPlanPer; ++i) {
        const u64 e = b0 + i;
        if (e <= count_out)
            out_off[e] = run;                                      // e == count_out: the closing entry, the total
        if (e == count_out)
            stat[1] = run;
        run += t[i];
    }
}

} // namespace

// ------------------------------------------------------------------------------ public

const char *gather_kernel_name(u64 n_bits, u64 count_out, bool ragged, u64 n_planes)
{
    if (n_bits == 0 || n_planes == 0 || n_planes > kGatherMaxPlanes || (ragged && n_planes != 1))
        return "";
    if (count_out == 0)
        return "none";
    return ragged ? "k_gather_ragged" : "k_gather";
}

int gather_plan(u64 count_in, const u64 *src_off, u64 count_out, const u64 *idx, u64 *out_off, u64 result[2],
                hipError_t &herr, hipStream_t s)
{
    herr = hipSuccess;
    result[0] = result[1] = 0;
    const bool ragged = src_off != nullptr;
    if (!ragged && !idx)
        return 0;                                                  // a uniform tile: nothing to check or size
    const u64 nchunks = count_out / kGPlanChunk + 1;              // (the closing entry count_out belongs to a chunk)
    const u64 words = kGPlanStatus + nchunks;
    // the status words: a plain block the thread keeps (scratch_take, csgn_kernels.h); the call drains s before it
    // returns, so the next call on s finds them free
    bool owned = false;
    u64 *stat = scratch_take(SCRATCH_GATHER, words * 8, s, owned, herr);
    if (herr != hipSuccess)
        return 1;
    auto fail = [&](hipError_t e) {
        herr = scratch_done(stat, owned, e);
        return 1;
    };
    if ((herr = zero_words(stat, words, s)) != hipSuccess)
        return fail(herr);
    const FastDiv d_in = csgn_fastdiv_make(count_in ? (u32)count_in : 1u);
    if (idx && count_out) {
        const u32 blocks = (u32)std::min<u64>((count_out + kGPlanThreads - 1) / kGPlanThreads, 2048u);
        k_gather_plan<<<blocks, kGPlanThreads, 0, s>>>(0u, (u32)count_in, src_off, (u32)count_out, idx, d_in, out_off, stat);
        if ((herr = hipGetLastError()) != hipSuccess)
            return fail(herr);
    }
    if (ragged) {
        k_gather_plan<<<(u32)nchunks, kGPlanThreads, 0, s>>>(1u, (u32)count_in, src_off, (u32)count_out, idx, d_in,
                                                             out_off, stat);
        if ((herr = hipGetLastError()) != hipSuccess)
            return fail(herr);
    }
    u64 h[2] = {0, 0};
    if ((herr = hipMemcpyAsync(h, stat, 16, hipMemcpyDeviceToHost, s)) != hipSuccess)
        return fail(herr);
    if ((herr = hipStreamSynchronize(s)) != hipSuccess)
        return fail(herr);
    if ((herr = scratch_done(stat, owned, hipSuccess)) != hipSuccess)
        return 1;
    result[0] = h[0] ? 0 : h[1];
    result[1] = h[0];
    return 0;
}

hipError_t gather_planes(u64 n_bits, u64 n_planes, const u64 *const *src, const u64 *terms, u64 count_in,
                         u64 count_out, const u64 *idx, u64 *const *dst, hipStream_t s)
{
    const u64 dL = (n_bits + 63) / 64;
    if (count_out == 0 || n_planes == 0 || n_planes > kGatherMaxPlanes)
        return n_planes > kGatherMaxPlanes ? hipErrorInvalidValue : hipSuccess;
    const bool wide = wide_units(dL, ptr_array(src, n_planes), ptr_array(dst, n_planes));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    GatherArgs a;
    u32 n = 0;
    u64 blocks = 0, units = 0;
    for (u64 j = 0; j < n_planes; ++j) {
        if (terms[j] == 0)
            continue;                                              // an empty plane: nothing to write
        const u32 eu = (u32)(terms[j] * U);
        a.src[n] = src[j];
        a.dst[n] = dst[j];
        a.eu.set(n, eu);
        a.first[n] = blocks;
        blocks += (count_out * eu + kGatherBlockUnits - 1) / kGatherBlockUnits;
        units += count_out * eu;
        ++n;
    }
    if (n == 0)
        return hipSuccess;
    a.first[n] = blocks;
    a.n_planes = n;
    a.idx = idx;
    a.count_in = (u32)count_in;
    a.count_out = (u32)count_out;
    a.d_in = csgn_fastdiv_make(count_in ? (u32)count_in : 1u);
    a.xcd = stream_xcd(units);
    const u64 max_blocks = launch_blocks();
    for (u64 b0 = 0; b0 < blocks; b0 += max_blocks) {
        a.block_base = b0;
        const u32 nb = (u32)std::min<u64>(blocks - b0, max_blocks);
        if (wide)
            k_gather<unit16><<<nb, 256, 0, s>>>(a);
        else
            k_gather<unit8><<<nb, 256, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t gather_ragged(u64 n_bits, u64 count_in, const u64 *src, const u64 *src_off, u64 count_out, const u64 *idx,
                         u64 *dst, const u64 *out_off, u64 total_terms_out, hipStream_t s)
{
    const u64 dL = (n_bits + 63) / 64;
    if (count_out == 0 || total_terms_out == 0)
        return hipSuccess;
    const bool wide = wide_units(dL, src, dst);
    const u32 U = (u32)(wide ? dL / 2 : dL);
    const u64 total_units = total_terms_out * U;
    const FastDiv dU = csgn_fastdiv_make(U), d_in = csgn_fastdiv_make(count_in ? (u32)count_in : 1u);
    const int chunks = ragged_chunks(total_units);
    // units of one launch.  No multiple of 256 * C (kMaxBlocks256 is 15 mod 16): every launch is a grid of its own, whose
    // workgroup b starts at u0 + b * 256 * C and whose end u0 + nu bounds every chunk as total_units, so its last
    // workgroup stops where the next launch starts (tests/test_launch_split_gpu.py runs caps of both residues)
    const u64 per_launch = launch_blocks() * 256u;
    for (u64 u0 = 0; u0 < total_units; u0 += per_launch) {
        const u64 nu = std::min(total_units - u0, per_launch);
        const u32 blocks = ceil_div_u64(nu, 256u * (u32)chunks);
#define CSGN_GATHER_RAGGED(CH)                                                                                       \
    do {                                                                                                            \
        if (wide)                                                                                                   \
            k_gather_ragged<unit16, CH><<<blocks, 256, 0, s>>>(                                                    \
                reinterpret_cast<const unit16 *>(src), src_off, (u32)count_in, idx, reinterpret_cast<unit16 *>(dst), \
                out_off, (u32)count_out, u0, u0 + nu, U, dU, d_in);                                                 \
        else                                                                                                        \
            k_gather_ragged<unit8, CH><<<blocks, 256, 0, s>>>(src, src_off, (u32)count_in, idx, dst, out_off,      \
                                                              (u32)count_out, u0, u0 + nu, U, dU, d_in);           \
    } while (0)
        switch (chunks) {
        case 1: CSGN_GATHER_RAGGED(1); break;
        case 2: CSGN_GATHER_RAGGED(2); break;
        case 4: CSGN_GATHER_RAGGED(4); break;
        case 16: CSGN_GATHER_RAGGED(16); break;
        default: CSGN_GATHER_RAGGED(8); break;
        }
#undef CSGN_GATHER_RAGGED
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace csgn
