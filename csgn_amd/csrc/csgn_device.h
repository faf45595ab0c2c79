// csgn_device.h -- helpers shared by the kernel translation units (csgn_mul.hip, csgn_add.hip, csgn_decrypt.hip,
// csgn_encrypt.hip, csgn_permute.hip, csgn_compact.hip, csgn_harness.hip, and the uniform-batch families
// csgn_gates.hip, csgn_uint.hip, csgn_uint_plain.hip, csgn_uint_addk.hip, csgn_uint_lut.hip, csgn_uint_read.hip,
// csgn_uint_find.hip, csgn_uint_first.hip, csgn_uint_nth.hip, csgn_uint_lt_select.hip, csgn_uint_decrypt.hip, csgn_matmul.hip, csgn_count.hip, csgn_count_prefix.hip, csgn_uint_add_where.hip, csgn_uint_linear.hip, csgn_uint_plain_sum.hip, csgn_uint_bilinear.hip, csgn_uint_poly.hip, csgn_wsum.hip, csgn_gather.hip):
// 16-/8-byte unit access and the choice between them, the ONE and ZERO terms' units, FastDiv tables in kernel
// arguments, the XCD-contiguous block order, CSR pair search, the LDS subset tables of DESIGN §4.15 (csgn_selector.h
// builds the skeleton of the read, find and lt_select kernels on them), launch limits,
// the term-count limit and the knob-dependent launch choices (csgn_tuning.h).  Everything has internal linkage (one
// copy per translation unit).
//
// Common shape of the data path: lanes own consecutive 16-byte units so every wave-level
// load/store is one global_{load,store}_dwordx4 covering 1 KiB of contiguous, 128-B-aligned
// HBM.  All of it is bitwise integer work bound by HBM bandwidth: there is no MFMA anywhere.
// Design notes live in DESIGN.md; reference citations (/root/reference/...) name the scalar loop
// each kernel replaces.
#pragma once

#include "csgn_kernels.h"
#include "csgn_tuning.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kWave = 64;

template <typename Unit, bool NT>
__device__ inline void unit_store(Unit *p, Unit v)
{
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// true iff every mask bit is set in x
__device__ inline bool unit_covers(unit16 x, unit16 m)
{
    unit16 d = (x & m) ^ m;
    return (d.x | d.y | d.z | d.w) == 0u;
}
__device__ inline bool unit_covers(unit8 x, unit8 m) { return (x & m) == m; }

// the ONE term's unit k of U: every bit set except the unused low bits of the term's last word (last_mask:
// last_word_mask), which stay zero as in every canonical term.  It decrypts to 1 under every key, ZERO to 0.
__device__ inline unit16 one_unit(unit16, u32 k, u32 U, u64 last_mask)
{
    unit16 v = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (k == U - 1u) {
        v.z = (u32)last_mask;
        v.w = (u32)(last_mask >> 32);
    }
    return v;
}
__device__ inline unit8 one_unit(unit8, u32 k, u32 U, u64 last_mask) { return k == U - 1u ? last_mask : ~0ull; }
__device__ inline unit16 zero_unit(unit16) { return unit16{0u, 0u, 0u, 0u}; }
__device__ inline unit8 zero_unit(unit8) { return 0ull; }

// N divisors of a kernel's arguments as three parallel u32 arrays (d, magic, shift), the layout the scalar loads of a
// uniform index read: set on the host, at() on the device.
template <u32 N>
struct FastDivTable {
    u32 d[N], magic[N], shift[N];

    void set(u32 i, u32 divisor)
    {
        const FastDiv f = csgn_fastdiv_make(divisor);
        d[i] = f.d;
        magic[i] = f.magic;
        shift[i] = f.shift;
    }
    __device__ FastDiv at(u32 i) const { return FastDiv{d[i], magic[i], shift[i]}; }
};

inline u32 ceil_div_u64(u64 a, u64 b) { return (u32)((a + b - 1) / b); }

// HIP refuses a launch whose gridDim.x * blockDim.x reaches 2^32 (hipErrorInvalidConfiguration),
// so the number of workgroups per launch is bounded by the block size, not by 2^31.
constexpr u64 kMaxBlocks256 = ((1ull << 32) - 1) / 256;    // 256-thread workgroups
constexpr u64 kMaxBlocks512 = ((1ull << 32) - 1) / 512;    // the tiled kernel's upper block size
constexpr u64 kMaxBlocks1024 = ((1ull << 32) - 1) / 1024;

// 256-thread workgroups one launch takes where the HOST cuts a call into several launches: kMaxBlocks256, or what knob
// launch_blocks says when that is lower, which is how the tests run the second and later launches of every split (no
// shape that fits a test gets there by itself).  Host only; a host call reads it once.
inline u64 launch_blocks()
{
    const int forced = tune(TUNE_LAUNCH_BLOCKS);
    return forced > 0 ? std::min<u64>((u64)forced, kMaxBlocks256) : kMaxBlocks256;
}

// Workgroups are dealt round-robin over the 8 XCDs (block b runs on XCD b % 8; placement is
// a speed matter only, never correctness).  Remapping the block id so that XCD x owns the
// x-th contiguous eighth of the logical block range makes every XCD's L2 write back one
// sequential address stream instead of every 8th 4 KiB chunk: +5 % on a pure fill
// (tools/wbench.hip: 6.9 -> 7.3 TB/s).  Bijective for any grid size, and only on the grid of the launch itself:
// nblocks is that launch's workgroup count.  Callable from the host so that the CPU tests pin it
// (csgn_debug_block_order, tests/test_capi_symbols.py).
__host__ __device__ inline u32 xcd_contiguous_block(u32 b, u32 nblocks)
{
    const u32 q = nblocks >> 3, r = nblocks & 7u, x = b & 7u;
    return x * q + (x < r ? x : r) + (b >> 3);
}

// The same with the XCDs taking GROUPS of `group` consecutive logical blocks in turn (XCD x owns groups x, x + 8, ...)
// instead of one contiguous eighth each: every XCD still writes runs of group x 4-16 KiB, but a stretch of the output
// whose blocks are slow (the single-term pairs behind one huge pair of a skewed ragged batch: latency-bound workgroups)
// is spread over all eight XCDs instead of being the tail of ONE (round 5: 640 such workgroups, 6 % of the output,
// were 2.5 rounds of 32 CUs at the end of a launch the other 224 CUs had left).  group = 0: the contiguous eighths.
// Bijective for any grid size: the blocks past the last whole round of 8 groups keep their own index.
__host__ __device__ inline u32 xcd_grouped_block(u32 b, u32 nblocks, u32 group)
{
    if (group == 0u)
        return xcd_contiguous_block(b, nblocks);
    const u32 round = 8u * group, full = nblocks - nblocks % round;
    if (b >= full)
        return b;
    const u32 x = b & 7u, q = b >> 3;                            // XCD, index inside the XCD
    return ((q / group) * 8u + x) * group + q % group;
}

// largest p in [lo, hi) with off[p] <= term   (requires off[lo] <= term)
__device__ inline u32 csr_find(const u64 *__restrict__ off, u32 lo, u32 hi, u64 term)
{
    while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= term)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// largest p >= lo with off[p] <= term, looking near lo first (requires off[lo] <= term): the
// common answers are lo itself (one load) or a pair a few steps on
__device__ inline u32 csr_gallop(const u64 *__restrict__ off, u32 lo, u32 batch, u64 term)
{
    u32 hi = lo + 1u, step = 1u;
    while (hi < batch && off[hi] <= term) {
        lo = hi;
        step <<= 1;
        hi = (batch - lo > step) ? lo + step : batch;
    }
    return csr_find(off, lo, hi, term);
}

// The same answer as csr_find(off, lo, hi, term), computed by a whole WAVE: a 64-ary search, every
// step one load per lane (64 probes spread over the range) and one __ballot -- log64(batch) dependent
// round trips (3 for 65 536 pairs, 4 for 1 M) where the binary search makes 17 to 20.  The start-up
// search of a ragged workgroup was ~10 us of a lifetime in which it writes 16 KiB (~5 us at full
// rate): with few workgroup rounds (a 178 MB output) nothing hid it (round 2: 2.7 TB/s on one
// 1024x1024 pair among 65 535 singles).  Requires off[lo] <= term; every lane returns the result.
__device__ inline u32 wave_find(const u64 *__restrict__ off, u32 lo, u32 hi, u64 term)
{
    const u32 lane = threadIdx.x & (kWave - 1);
    while (hi - lo > 1) {
        const u32 n = hi - lo, s = (n + kWave - 1) / kWave;
        const u64 idx = (u64)lo + (u64)lane * s;
        const bool ok = idx < hi && off[idx] <= term;          // monotone in the lane number; lane 0 holds by the invariant
        const u32 c = (u32)__popcll(__ballot(ok));             // >= 1
        lo += (c - 1u) * s;
        hi = min(lo + s, hi);
    }
    return lo;
}

template <int VEC>
struct UnitWords {
    u64 w[VEC];
};
__device__ inline UnitWords<2> unit_to_words(unit16 v)
{
    UnitWords<2> r;
    r.w[0] = ((u64)v.y << 32) | v.x;
    r.w[1] = ((u64)v.w << 32) | v.z;
    return r;
}
__device__ inline UnitWords<1> unit_to_words(unit8 v)
{
    UnitWords<1> r;
    r.w[0] = v;
    return r;
}
__device__ inline void words_to_unit(const UnitWords<2> &r, unit16 &v)
{
    v.x = (u32)r.w[0];
    v.y = (u32)(r.w[0] >> 32);
    v.z = (u32)r.w[1];
    v.w = (u32)(r.w[1] >> 32);
}
__device__ inline void words_to_unit(const UnitWords<1> &r, unit8 &v) { v = r.w[0]; }

// v_writelane_b32: drop a wave-uniform 64-bit value into ONE lane of a VGPR pair (hipcc 7.2
// exposes no builtin for it).  `lane` must be a compile-time constant.  The s_nop is the
// gfx940+ "VALU writes SGPR -> VALU reads that SGPR" hazard (2 wait states): the ballot is
// produced by a v_cmp immediately before, and hipcc pads nothing inside an asm statement
// (observed: without it the low word of some lanes read a stale SGPR).
__device__ inline void write_lane64(u64 uniform_value, int lane, u32 &lo, u32 &hi)
{
    asm volatile("s_nop 1\n\tv_writelane_b32 %0, %2, %4\n\tv_writelane_b32 %1, %3, %4"
                 : "+v"(lo), "+v"(hi)
                 : "s"((u32)uniform_value), "s"((u32)(uniform_value >> 32)), "n"(lane));
}

// ---------------------------------------------------------------------- chained scan across workgroups
constexpr u64 kFlagAggregate = 1ull << 62, kFlagPrefix = 2ull << 62, kValueMask = (1ull << 62) - 1;

// Decoupled look-back (one wave): publish this group's count, add up the counts of the groups before
// it back to the nearest one whose inclusive prefix is known, publish the own inclusive prefix.  Every
// granule is ONE 8-byte agent-scope store/load carrying flag and value together, so no ordering
// between data and flag is needed.  Returns the exclusive prefix in every lane.
__device__ inline u64 lookback(u64 *status, u32 gid, u64 count)
{
    const u32 lane = threadIdx.x & (kWave - 1);
    if (lane == 0)
        __hip_atomic_store(status + gid, kFlagAggregate | count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u64 excl = 0;
    long long base = (long long)gid - 1;
    while (base >= 0) {
        const long long idx = base - (long long)lane;
        const u64 v = idx >= 0 ? __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                               : kFlagPrefix;              // before group 0: prefix 0
        const u32 flag = (u32)(v >> 62);
        const u64 pending = __ballot(flag == 0u), known = __ballot(flag == 2u);
        const u32 first = known ? (u32)__builtin_ctzll(known) : kWave;     // nearest lane holding a prefix
        const u64 need = first < kWave - 1 ? (2ull << first) - 1ull : ~0ull;
        if (pending & need) {
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        u64 mine = lane <= first ? (v & kValueMask) : 0ull;
        for (u32 d = 32; d > 0; d >>= 1)
            mine += __shfl_xor(mine, d, kWave);
        excl += mine;
        if (first < kWave)
            break;
        base -= kWave;
    }
    if (lane == 0)
        __hip_atomic_store(status + gid, kFlagPrefix | (excl + count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

// The same with one MARK bit riding along (value: 61 bits): a group may mark itself, and every group learns whether
// any group before it did.  k_plan marks chunks that hold a pair of more than one product term, so the LAST chunk
// knows from its look-back alone -- no counter of finished workgroups, no fence -- the batch total and whether every
// pair of the batch is 1 x 1.
constexpr u64 kMarkBit = 1ull << 61, kMarkedValueMask = kMarkBit - 1;
__device__ inline u64 lookback_marked(u64 *status, u32 gid, u64 count, bool mark, bool &marked_before)
{
    const u32 lane = threadIdx.x & (kWave - 1);
    const u64 own = mark ? kMarkBit : 0ull;
    if (lane == 0)
        __hip_atomic_store(status + gid, kFlagAggregate | own | (count & kMarkedValueMask), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    u64 excl = 0;
    bool before = false;
    long long base = (long long)gid - 1;
    while (base >= 0) {
        const long long idx = base - (long long)lane;
        const u64 v = idx >= 0 ? __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                               : kFlagPrefix;              // before group 0: prefix 0, no mark
        const u32 flag = (u32)(v >> 62);
        const u64 pending = __ballot(flag == 0u), known = __ballot(flag == 2u);
        const u32 first = known ? (u32)__builtin_ctzll(known) : kWave;     // nearest lane holding a prefix
        const u64 need = first < kWave - 1 ? (2ull << first) - 1ull : ~0ull;
        if (pending & need) {
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        u64 mine = lane <= first ? (v & kMarkedValueMask) : 0ull;
        before |= __ballot(lane <= first && (v & kMarkBit) != 0ull) != 0ull;
        for (u32 d = 32; d > 0; d >>= 1)
            mine += __shfl_xor(mine, d, kWave);
        excl += mine;
        if (first < kWave)
            break;
        base -= kWave;
    }
    if (lane == 0)
        __hip_atomic_store(status + gid, kFlagPrefix | ((before || mark) ? kMarkBit : 0ull) | ((excl + count) & kMarkedValueMask),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    marked_before = before;
    return excl;
}

// A workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every global load, store and
// atomic the wave has in flight (s_waitcnt vmcnt(0)); where a wave has issued a global request whose result it wants
// AFTER the barrier, this one lets it stay in flight.
__device__ inline void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Zero-fill as a KERNEL: no compute path of this library calls hipMemsetAsync, so a circuit's graph
// (csgn_circuit_*) holds kernel nodes only.  Why (profiles/r05/graph_memset_*.log): circuits whose
// zero fills were captured as memset NODES have twice returned wrong data inside the long-lived test process
// (round 4: the inputs of a circuit with a compaction node read as zeros; round 5: one wrong bit in the second
// of five runs of a long-uniform decrypt), never with kernel nodes.  The cause is NOT pinned: a minimal HIP
// program (tools/graph_memset_probe.hip: memset node against uploads, fills and atomics on every stream kind,
// under the ROCm 7.2.0 runtime and under the 7.0.2 one torch bundles) orders memset nodes correctly, and the
// failing circuit alone ran 240 times clean (tools/graph_memset_case.py).  Dev knob zero_memset = 1 brings the
// memset form back for such experiments.
__global__ void __launch_bounds__(256) k_zero_words(u64 *__restrict__ p, u64 n)
{
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u)
        p[i] = 0ull;
}
inline hipError_t zero_words(u64 *p, u64 n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    if (tune(TUNE_ZERO_MEMSET))                      // dev only (see above)
        return hipMemsetAsync(p, 0, n * 8, s);
    const u32 blocks = (u32)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    k_zero_words<<<blocks, 256, 0, s>>>(p, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------- launch helpers
// the used bits of a term's last word (MSB first; the unused low bits stay zero): ONE's last word
inline u64 last_word_mask(u64 n_bits)
{
    const u32 r = (u32)(n_bits % 64);
    return r ? ~0ull << (64 - r) : ~0ull;
}

template <typename T>
inline bool aligned16(const T *p)
{
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// the n pointers of an array, as one argument of wide_units
template <typename T>
struct PtrArray {
    T *const *p;
    u64 n;
};
template <typename T>
inline PtrArray<T> ptr_array(T *const *p, u64 n) { return PtrArray<T>{p, n}; }
template <typename T>
inline bool aligned16(PtrArray<T> a) { return std::all_of(a.p, a.p + a.n, [](T *q) { return aligned16(q); }); }

// The unit of the uniform launchers: 16 bytes when dL is even and every pointer (one by one, or ptr_array) is 16-byte
// aligned -- a null pointer counts as aligned --, else 8 bytes.
template <typename... P>
inline bool wide_units(u64 dL, P... p)
{
    return dL % 2 == 0 && (aligned16(p) && ...);
}

// Term counts per element stay below 2^62, every count the C ABI computes or accepts.
constexpr u64 kTermLimit = 1ull << 62;

// p = x * y; false when the product reaches kTermLimit
inline bool term_mul(u64 x, u64 y, u64 &p)
{
    unsigned long long q;
    if (__builtin_mul_overflow((unsigned long long)x, (unsigned long long)y, &q) || q >= kTermLimit)
        return false;
    p = q;
    return true;
}

// Block order of the one-unit-per-lane stream kernels (1x1 multiply, uniform add): XCD-contiguous
// once a launch is large (measured +3-5 % from 32 M units = 512 MB per stream up, -1-2 % at
// 10 M units).  Knob stream_xcd = 0 / 1 forces it.
inline u32 stream_xcd(u64 units)
{
    return tune_choose(TUNE_STREAM_XCD, units >= (1ull << 25)) ? 1u : 0u;
}

// The launches of a grid of per_group workgroups for every group of G elements, as many groups per launch as
// max_blocks (the caller's launch_blocks()) allows: launch(e0, elements, workgroups) issues the one from element e0 on.
template <typename Launch>
inline hipError_t launch_groups(u64 max_blocks, u64 batch, u32 G, u64 per_group, Launch launch)
{
    const u64 max_groups = std::max<u64>(1, max_blocks / per_group);
    const u64 groups = (batch + G - 1) / G;
    for (u64 g0 = 0; g0 < groups; g0 += max_groups) {
        const u64 ng = std::min(max_groups, groups - g0), e0 = g0 * G;
        launch(e0, std::min<u64>(batch - e0, ng * G), (u32)(ng * per_group));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// 4 KiB chunks per workgroup of the flat ragged kernels: as many as 8 (the workgroup's first search
// is paid once per C chunks) while the grid still has >= 8192 workgroups to fill the chip with.
// Knob ragged_c = 1, 2, 4, 8, 16 overrides.
inline int ragged_chunks(u64 total_units)
{
    const int forced = tune(TUNE_RAGGED_C);
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 16)
        return forced;
    int c = 1;
    while (c < 8 && total_units / (256u * 2u * (u64)c) >= 8192u)
        c *= 2;
    return c;
}

// ------------------------------------------------------------------------- chain decode
// The left-nested product / sum chains over the planes a_j and n_j = a_j + ONE that csgn_uint_plain.hip and
// csgn_uint_addk.hip decode.  Args is the kernel's level table, by value in its arguments: plane[j], t[j], pend[j]
// (the start of a sum level's tail, above every index for a product level), rad (the factor's length as a FastDiv),
// base (the level that ends every walk) and U (units per term).
// term i of a list that is a_j (i < t_j) or n_j (i == t_j: ONE); the load is issued unconditionally (clamped)
template <typename Unit, typename Args>
__device__ inline Unit chain_term(const Args &a, u32 j, u64 elem_units, u32 i, u32 k, Unit one)
{
    const u32 tj = a.t[j];
    const Unit *p = reinterpret_cast<const Unit *>(a.plane[j]);
    const Unit v = p[elem_units * tj + (u64)min(i, tj - 1u) * a.U + k];
    return i < tj ? v : one;
}

// levels j = hi down to lo (inclusive, lo >= base) applied to idx, factor(j, i) called for term i of level j's list
// (i == t_j: the ONE of n_j); returns true when a tail or the base ended the walk.  Host and device: the decode by
// position of csgn_uint_plain_sum_decode is this walk with a factor that records its arguments.
template <typename Args, typename Factor>
__host__ __device__ inline bool chain_walk_each(const Args &a, u32 hi, u32 lo, u32 &idx, Factor factor)
{
    for (u32 j = hi + 1u; j-- > lo;) {
        if (j == a.base) {
            factor(j, idx);
            return true;
        }
        const u32 pe = a.pend[j];
        if (idx >= pe) {                                  // a sum level's tail: a_j, or n_j
            factor(j, idx - pe);
            return true;
        }
        const FastDiv dr = a.rad.at(j);
        const u32 q = csgn_fastdiv(idx, dr), d = idx - q * dr.d;
        idx = q;
        factor(j, d);
    }
    return false;
}

// the same with the factors ANDed into v
template <typename Unit, typename Args>
__device__ inline bool chain_walk(const Args &a, u32 hi, u32 lo, u64 eu, u32 k, Unit one, u32 &idx, Unit &v)
{
    return chain_walk_each(a, hi, lo, idx, [&](u32 j, u32 i) { v &= chain_term<Unit>(a, j, eu, i, k, one); });
}

// One lane's run of a comparison: unit k of the nt consecutive terms from t0 on of the chain `a`
// describes (plane, t, pend, rad, base, U), written to o, o + U, ...  Levels [cut, top] are walked per term, loading only
// where the digit moves (radix above 1; `unit`: the radix-1 levels) or a tail ends the walk; the AND of the levels below
// the cut is kept in registers, keyed by the index that reaches the cut.  zero: the value is ZERO, no level is read;
// neg: term T - 1 is the appended ONE.
template <typename Unit, typename Args>
__device__ inline void chain_run(const Args &a, u32 top, u32 cut, u32 zero, u32 neg, u32 T, u64 unit, u64 eu, u32 k,
                                 Unit one, u32 t0, u32 nt, Unit *o)
{
    // the radix-1 factors of the fast levels: every term that passes the cut carries all of them
    Unit fast_unit = one;
    for (u32 j = top + 1u; !zero && j-- > cut;)
        if ((unit >> j) & 1u)
            fast_unit &= chain_term<Unit>(a, j, eu, 0u, k, one);
    u32 key = 0xFFFFFFFFu;                                // the index that reached the cut, and the AND below it
    Unit below = one;
    for (u32 q = 0; q < nt; ++q) {
        const u32 idx0 = t0 + q;
        Unit v = one;
        if (neg && idx0 == T - 1u) {
            // the appended ONE
        } else if (zero) {
            v = zero_unit(Unit());
        } else {
            u32 idx = idx0, stop = 0xFFFFFFFFu;
            for (u32 j = top + 1u; j-- > cut;) {
                const u32 pe = a.pend[j];
                if (idx >= pe) {                          // a sum level's tail
                    v &= chain_term<Unit>(a, j, eu, idx - pe, k, one);
                    stop = j;
                    break;
                }
                if ((unit >> j) & 1u)
                    continue;                             // d = 0, idx unchanged: f_j[0] is in fast_unit
                const FastDiv dr = a.rad.at(j);
                const u32 qq = csgn_fastdiv(idx, dr), d = idx - qq * dr.d;
                idx = qq;
                v &= chain_term<Unit>(a, j, eu, d, k, one);
            }
            if (stop != 0xFFFFFFFFu) {
                // a tail at level `stop` carries the radix-1 factors above it only (a short list: tails are a small
                // share of any large result)
                for (u32 j = top + 1u; j-- > stop + 1u;)
                    if ((unit >> j) & 1u)
                        v &= chain_term<Unit>(a, j, eu, 0u, k, one);
            } else {
                v &= fast_unit;
                if (idx != key) {
                    key = idx;
                    below = one;
                    chain_walk<Unit>(a, cut - 1u, a.base, eu, k, one, idx, below);
                }
                v &= below;
            }
        }
        unit_store<Unit, true>(o + (u64)q * a.U, v);
    }
}

// ------------------------------------------------------------------------- subset tables
// For a workgroup's elements and its slice of KC units of every term, table k holds the AND of every subset of the
// fresh (one-term) planes [hb[k], hb[k+1]), entry S of element el at units tbase[k] + ((el << h_k) | S) * KC on; the
// AND of any subset of all the planes is then one to three LDS reads (csgn_uint_lut.hip, and through csgn_selector.h
// csgn_uint_read.hip, csgn_uint_find.hip, csgn_uint_lt_select.hip and csgn_uint_arith.hip).
constexpr u32 kMaxSubsetTables = 3;

// by value in the kernel arguments
struct SubsetTables {
    u32 ntab, hb[kMaxSubsetTables + 1], tbase[kMaxSubsetTables];   // table k: planes [hb[k], hb[k+1]), at unit tbase[k]
};

// The build by a 256-thread workgroup for its elements [e0, e0 + ne) of G and units [k0, k0 + kc) of a KC-unit slice
// (dKC: KC), plane i of the elements from plane[i] on, an element's term `pitch` units after the one before (0: U, a
// plane of its own; csgn_uint_first.hip's grouped rows lie group * U apart); every table is complete at the closing
// barrier.
template <typename Unit>
__device__ inline void subset_build(Unit *tab, const SubsetTables &t, const void *const *plane, u32 G, u32 KC,
                                    const FastDiv &dKC, u32 U, u64 last_mask, u64 e0, u32 ne, u32 k0, u32 kc,
                                    u32 pitch = 0u)
{
    const u32 eu = pitch ? pitch : U;
    // entry 0 of every table is ONE; level b fills entries [2^b, 2^(b+1)) from [0, 2^b) and plane hb[k] + b
    for (u32 tb = 0; tb < t.ntab; ++tb) {
        const u32 h = t.hb[tb + 1] - t.hb[tb];
        for (u32 x = threadIdx.x; x < G * KC; x += 256u) {
            const u32 el = csgn_fastdiv(x, dKC), kk = x - el * KC;
            tab[t.tbase[tb] + ((el << h) * KC) + kk] = one_unit(Unit(), k0 + kk, U, last_mask);
        }
    }
    for (u32 b = 0; b < t.hb[1]; ++b) {              // table 0 is the widest
        __syncthreads();
        for (u32 tb = 0; tb < t.ntab; ++tb) {
            const u32 h = t.hb[tb + 1] - t.hb[tb];
            if (b >= h)
                continue;
            const Unit *p = reinterpret_cast<const Unit *>(plane[t.hb[tb] + b]);
            const u32 n = (G * KC) << b;
            for (u32 x = threadIdx.x; x < n; x += 256u) {
                const u32 row = csgn_fastdiv(x, dKC), kk = x - row * KC;
                const u32 el = row >> b, s = (1u << b) | (row & ((1u << b) - 1u));
                if (el >= ne || kk >= kc)
                    continue;
                const u32 at = t.tbase[tb] + ((el << h) | s) * KC + kk;
                tab[at] = tab[at - (1u << b) * KC] & p[(e0 + el) * eu + k0 + kk];
            }
        }
    }
    __syncthreads();
}

// the AND of the planes of subset S for element el, unit kk of the slice
template <typename Unit>
__device__ inline Unit subset_and(const Unit *tab, const SubsetTables &t, u32 el, u32 S, u32 KC, u32 kk)
{
    Unit v = tab[t.tbase[0] + ((el << t.hb[1]) | (S & ((1u << t.hb[1]) - 1u))) * KC + kk];
    for (u32 tb = 1; tb < t.ntab; ++tb) {
        const u32 h = t.hb[tb + 1] - t.hb[tb];
        v &= tab[t.tbase[tb] + ((el << h) | ((S >> t.hb[tb]) & ((1u << h) - 1u))) * KC + kk];
    }
    return v;
}

// The host plan: the table split and the unit slices of `planes` fresh planes (0: no tables) at U units of unit_bytes
// per term within `budget` bytes of LDS per workgroup; layout(G) places the tables of G elements.  min_tables asks for
// that many tables (no more than planes or kMaxSubsetTables) where the planes alone would get fewer: smaller tables and
// one more LDS read per AND, for an operation that writes few terms per element (csgn_uint_arith.hip).
struct SubsetPlan {
    SubsetTables t;
    u64 entries;              // table units per element and unit of a term
    u32 unit_bytes;
    u32 KC, chunks;           // units of a slice, slices of a term
    u64 max_G;                // elements whose tables fit the budget (no limit without tables)

    u32 layout(u32 G)         // tbase[]; returns the LDS bytes
    {
        u32 at = 0;
        for (u32 k = 0; k < t.ntab; ++k) {
            t.tbase[k] = at;
            at += (u32)((G << (t.hb[k + 1] - t.hb[k])) * KC);
        }
        return at * unit_bytes;
    }
};

inline SubsetPlan subset_plan(u32 planes, u32 U, u32 unit_bytes, u64 budget, u32 min_tables = 1)
{
    SubsetPlan p = {};
    p.unit_bytes = unit_bytes;
    // one table up to 5 planes, two up to 10, three above; the low tables take the odd planes
    if (planes) {
        p.t.ntab = std::max(planes <= 5 ? 1u : planes <= 10 ? 2u : 3u, std::min({min_tables, planes, kMaxSubsetTables}));
        for (u32 k = 0; k < p.t.ntab; ++k) {
            const u32 h = (planes - p.t.hb[k] + (p.t.ntab - k) - 1) / (p.t.ntab - k);
            p.t.hb[k + 1] = p.t.hb[k] + h;
            p.entries += 1ull << h;
        }
    }
    // unit chunks: only when one element's tables at whole terms pass the budget
    const u64 per_unit = p.entries * unit_bytes;
    const u32 chunks = per_unit * U > budget ? (u32)((per_unit * U + budget - 1) / budget) : 1u;
    p.KC = (U + chunks - 1) / chunks;
    p.chunks = (U + p.KC - 1) / p.KC;
    p.max_G = per_unit ? std::max<u64>(1, budget / (per_unit * p.KC)) : ~0ull;
    return p;
}

// ------------------------------------------------------------------------- subsets by rank
// What csgn_count.hip, csgn_wsum.hip and csgn_uint_nth.hip unrank their subsets with.
// C(n, k), exact, for the binomials of an unranking: every one counts subsets of the call's own C(g, m) < 2^31, and so
// does every value on the way (k <= n - k: they only grow).  The step c * (n - k + i) / i divides exactly and stays
// below 2^31 * 2^17, so it is done in double precision, whose correctly rounded quotient of an exact division is the
// integer itself -- a 64-bit integer division costs the device some 200 instructions, and a workgroup's threads each
// take a dozen binomials before the first store.  Pairs, the common plane, need no division at all.
__host__ __device__ inline u64 binom(u32 n, u32 k)
{
    if (k > n)
        return 0;
    if (k > n - k)
        k = n - k;
    if (k == 0)
        return 1;
    if (k == 1)
        return n;
    u64 c = ((u64)n * (n - 1u)) >> 1;
    if (k == 2)
        return c;
    // C(n - k + i, i) from C(n - k + i - 1, i - 1), starting at C(n - k + 2, 2)
    c = ((u64)(n - k + 2u) * (n - k + 1u)) >> 1;
    for (u32 i = 3; i <= k; ++i)
        c = (u64)((double)(c * (n - k + i)) / (double)i);
    return c;
}

// the m-subset of {0 .. g-1} of lexicographic rank r: position k takes the largest v for which the subsets whose
// position k is below v -- C(g - lo, m - k) - C(g - v, m - k) of them under the prefix -- are at most r
template <typename Put>
__host__ __device__ inline void unrank(u32 g, u32 m, u64 r, Put put)
{
    u32 lo = 0;
    for (u32 k = 0; k < m; ++k) {
        const u32 left = m - k;
        const u64 all = binom(g - lo, left);
        u32 a = lo, b = g - left + 1;
        while (b - a > 1) {
            const u32 mid = a + ((b - a) >> 1);
            if (all - binom(g - mid, left) <= r)
                a = mid;
            else
                b = mid;
        }
        r -= all - binom(g - a, left);
        put(k, a);
        lo = a + 1;
    }
}

} // namespace

} // namespace csgn
