// csgn_count_prefix.hip -- running counts of encrypted bits: for every row r of a group, every requested plane of the
// number of ones among the rows up to r (or before it), all rows of all elements in one launch.  Hand-written CDNA4
// (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.34.
//
// The definition (include/csgn_hip.h, csgn_count_prefix): row r counts the inputs x_0 .. x_{n_r - 1}, n_r = r + 1 -
// exclusive, and its plane j is csgn_count's plane j of those n_r inputs, word for word -- the m-subsets (m = 2^j) of
// {0 .. n_r - 1} in lexicographic order, term p = rank * t^m + digits, the AND of the factors' terms -- or the one ZERO
// term where m > n_r.  A plane's block holds the rows one after the other, row r a uniform batch of `count` elements
// from term count * off_j(r) on.
//
// k_count's method with the group size a property of the row.  Laid end to end, the rank streams of a plane's rows are
// the (m+1)-subsets of {0 .. N - 1}, N = g + 1 - exclusive, ordered by their largest member n and then
// lexicographically: C(N, m+1) ranks R, of which those of row n are [C(n, m+1), C(n+1, m+1)).  A workgroup owns one
// element -- or EG consecutive ones where an element's planes are a few units each --, one plane, a range of CP of those
// ranks wherever the rows' borders fall, and a slice of KC units of every term; so the triangle of row sizes is cut
// evenly and a single element fills the chip.  Every thread finds the row of the first rank of its run by bisection on
// C(n, m+1), unranks the subset with csgn_device.h's unrank, and steps to the successors, across row ends; it leaves
// per rank the subset and where the rank's terms begin.  The workgroup then stages the inputs below its last row in LDS
// once and walks the stream of its outputs with the unit fastest.  The first part of a plane also writes the ZERO
// terms of the rows shorter than m.  Nothing is uploaded and nothing is accumulated: one launch.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kLdsBudget = 49152;       // bytes of staged inputs per workgroup; with the rank records 64 KiB: two a CU
constexpr u32 kRankBytes = 16384;       // bytes of rank records per workgroup (kRankHead of them the last row's n)
constexpr u32 kRankHead = 16;
constexpr u32 kMinChunk = 16;           // units of a term slice at least, when terms are cut to fit the LDS
constexpr u64 kTargetUnits = 16384;     // units a workgroup writes at most by choice (256 KiB of 16-byte units)
constexpr u64 kMinUnits = 2048;         // ... and at least, when the range of ranks is cut further to fill the chip
constexpr u64 kFillBlocks = 2048;       // workgroups that fill 256 CUs (eight resident each)
constexpr u64 kMaxStream = 0xFFFFFE00ull;  // units of one workgroup's stream at most: its 32-bit index never wraps
constexpr u32 kMaxPlanes = 7;           // j = 0 .. 6
constexpr u32 kMaxIn = 64;              // input batches of the plane layout

// one requested plane.  A workgroup of an element is (plane, part of the ranks, unit chunk), the chunk fastest.
struct PrefixPlane {
    void *out;
    u64 bbase;                  // the plane's first workgroup among an element's
    u64 ranks;                  // C(N, m+1): the ranks of every row together
    u32 m, D;                   // 2^j, t^m
    u32 CP;                     // ranks a workgroup takes
    u32 zeros;                  // rows shorter than m: one ZERO term each, rows 0 .. zeros - 1
    FastDiv dD;
    FastDiv dEl;                // EG > 1: the units of one element of the stream, ranks * D * KC
};

// By value in the kernel arguments (uniform, scalar loads).
struct PrefixArgs {
    const void *in[kMaxIn];     // n_in == 1: the grouped batch; else input i's batch
    PrefixPlane p[kMaxPlanes];
    u64 block0;                 // this launch's first workgroup in the call
    u64 per_elem;               // workgroups of one element (of one group of EG elements)
    u64 count;
    u32 EG;                     // elements of a workgroup; above 1 only with whole terms and every plane in one part
    u32 g, nmax;                // inputs of an element; of the last row (g - exclusive)
    u32 t, U, KC, chunks, n_in, n_out, nblocks, xcd;
    u32 sbase;                  // byte offset of the rank records in the LDS
    FastDiv dKC, dT;
    FastDiv dIn;                // EG > 1: the staged units of one element, nmax * t * KC
};

// input i of element e: its first unit (term 0, unit 0)
template <typename Unit>
__device__ inline const Unit *prefix_input(const PrefixArgs &a, u64 e, u32 i)
{
    if (a.n_in == 1)
        return reinterpret_cast<const Unit *>(a.in[0]) + (e * a.g + i) * a.t * a.U;
    return reinterpret_cast<const Unit *>(a.in[i]) + e * a.t * a.U;
}

// C(n, m+1), the ranks below row n, from C(n, m) < 2^31: C(n, m) * (n - m) / (m + 1) divides exactly and the product
// stays below 2^31 * 2^17 (m >= 2: n <= 2^16), so double precision gives the integer (csgn_device.h, binom).  Pairs of
// a plane 0 with rows past 2^16 take the integer form.
__device__ inline u64 ranks_below(u32 n, u32 m)
{
    if (m == 1u)
        return ((u64)n * (n - 1u)) >> 1;
    return (u64)((double)(binom(n, m) * (u64)(n - m)) / (double)(m + 1u));
}

template <typename Unit, bool Staged, bool Digits>
__global__ void __launch_bounds__(256) k_count_prefix(PrefixArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Unit *xs = reinterpret_cast<Unit *>(smem_raw);                               // [(i * t + d) * KC + kk]
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, a.nblocks) : blockIdx.x;
    const u64 B = a.block0 + bid, eg = B / a.per_elem, rb = B - eg * a.per_elem, e = eg * a.EG;
    const u32 ne = (u32)min((u64)a.EG, a.count - e);              // elements e .. e + ne - 1
    u32 x = a.n_out - 1u;
    while (x > 0u && a.p[x].bbase > rb)
        --x;
    const PrefixPlane &P = a.p[x];
    const u64 pc = rb - P.bbase, part = pc / a.chunks;
    const u32 chunk = (u32)(pc - part * a.chunks);
    const u64 R0 = part * P.CP;
    const u32 nc = (u32)min((u64)P.CP, P.ranks - R0);
    const u32 k0 = chunk * a.KC, kc = min(a.KC, a.U - k0);
    const u32 m = P.m, t = a.t;
    // the rank records: the last row's n; per rank the first term of its cell for element e, the terms of its row
    // (the next element's cell lies that far on) and the subset -- 16-bit members, or for pairs the one input
    u32 *last_n = reinterpret_cast<u32 *>(smem_raw + a.sbase);
    u64 *rbase = reinterpret_cast<u64 *>(smem_raw + a.sbase + kRankHead);
    u32 *rT = reinterpret_cast<u32 *>(rbase + P.CP);
    u32 *sub1 = rT + P.CP;                                                       // m == 1: [cc]
    unsigned short *subs = reinterpret_cast<unsigned short *>(sub1);             // m > 1: [cc * m + k]

    // the ranks [R0, R0 + nc): thread th takes the run [th * run, th * run + run)
    {
        const u32 run = (nc + 255u) / 256u, first = threadIdx.x * run;
        if (first < nc) {
            const u64 R = R0 + first;
            // the row: the largest n in [m, nmax] with C(n, m+1) <= R
            u32 n = m, hi = a.nmax + 1u;
            while (hi - n > 1u) {
                const u32 mid = n + ((hi - n) >> 1);
                if (ranks_below(mid, m) <= R)
                    n = mid;
                else
                    hi = mid;
            }
            u64 below = ranks_below(n, m), rowc = binom(n, m), c = R - below;
            unsigned short *s = subs + first * m;
            if (m > 1u)
                unrank(n, m, c, [&](u32 k, u32 v) { s[k] = (unsigned short)v; });
            const u32 end = min(first + run, nc);
            for (u32 cc = first;;) {
                const u64 T = rowc * P.D;
                rbase[cc] = a.count * (P.zeros + below * P.D) + e * T + c * P.D;
                rT[cc] = (u32)T;
                if (m == 1u)
                    sub1[cc] = (u32)c;
                if (++cc == end)
                    break;
                if (++c == rowc) {                               // the row's end: the next row's first subset
                    below += rowc;
                    ++n;
                    rowc = binom(n, m);
                    c = 0;
                    if (m > 1u)
                        for (u32 i = 0; i < m; ++i)
                            s[m + i] = (unsigned short)i;
                } else if (m > 1u) {
                    u32 k = m - 1u;                              // the last position that can still move up
                    while (k > 0u && s[k] == n - m + k)
                        --k;
                    for (u32 i = 0; i < k; ++i)
                        s[m + i] = s[i];
                    const u32 v = s[k] + 1u;
                    for (u32 i = k; i < m; ++i)
                        s[m + i] = (unsigned short)(v + (i - k));
                }
                s += m;
            }
            if (end == nc)
                *last_n = n;
        }
    }
    __syncthreads();
    if (Staged) {
        // inputs 0 .. n - 1 of the last row this workgroup reaches (EG > 1: one part, every row)
        const u32 per = a.EG > 1u ? a.dIn.d : *last_n * t * a.KC, total = ne * per;
        for (u32 s = threadIdx.x; s < total; s += 256u) {
            const u32 el = a.EG > 1u ? csgn_fastdiv(s, a.dIn) : 0u, se = s - el * per;
            const u32 it = csgn_fastdiv(se, a.dKC), kk = se - it * a.KC;
            const u32 i = csgn_fastdiv(it, a.dT), d = it - i * t;
            if (kk < kc)
                xs[s] = prefix_input<Unit>(a, e + el, i)[(u64)d * a.U + k0 + kk];
        }
        __syncthreads();
    }

    Unit *__restrict__ out = reinterpret_cast<Unit *>(P.out);
    if (part == 0) {
        // the rows shorter than m: row r is `count` ZERO terms from term count * r on
        const u32 nz = ne * P.zeros * kc;
        for (u32 l = threadIdx.x; l < nz; l += 256u) {
            const u32 er = l / kc, kk = l - er * kc, el = er / P.zeros, r = er - el * P.zeros;
            unit_store<Unit, true>(out + (a.count * r + e + el) * a.U + k0 + kk, zero_unit(Unit()));
        }
    }
    const u32 len = ne * nc * P.D * a.KC;               // (element, rank, digits, unit), below 2^32 by the plan
    for (u32 l = threadIdx.x; l < len; l += 256u) {
        const u32 el = a.EG > 1u ? csgn_fastdiv(l, P.dEl) : 0u, le = l - el * P.dEl.d;
        const u32 cd = csgn_fastdiv(le, a.dKC), kk = le - cd * a.KC;
        if (kk >= kc)
            continue;
        u32 cc = cd, dd = 0;
        if (Digits) {
            cc = csgn_fastdiv(cd, P.dD);
            dd = cd - cc * P.D;
        }
        const unsigned short *s = subs + cc * m;
        Unit v = ~zero_unit(Unit());
        u32 rest = dd;
        for (u32 k = m; k-- > 0u;) {                             // the last factor's digit is the fastest
            u32 d = 0;
            if (Digits) {
                const u32 q = csgn_fastdiv(rest, a.dT);
                d = rest - q * t;
                rest = q;
            }
            const u32 i = m > 1u ? s[k] : sub1[cc];
            Unit w;
            if (Staged)
                w = xs[el * a.dIn.d + (i * t + d) * a.KC + kk];
            else
                w = prefix_input<Unit>(a, e + el, i)[(u64)d * a.U + k0 + kk];
            v &= w;
        }
        unit_store<Unit, true>(out + (rbase[cc] + (u64)el * rT[cc] + dd) * a.U + k0 + kk, v);
    }
}

// ------------------------------------------------------------------------------ host side

// C(n, k), or kTermLimit once it reaches that: the values on the way only grow (k <= n - k)
u64 sat_binom(u64 n, u64 k)
{
    if (k > n)
        return 0;
    k = std::min(k, n - k);
    unsigned __int128 c = 1;
    for (u64 i = 1; i <= k; ++i) {
        c = c * (n - k + i) / i;
        if (c >= kTermLimit)
            return kTermLimit;
    }
    return (u64)c;
}

// t^m, or kTermLimit once it reaches that
u64 sat_pow(u64 t, u32 m)
{
    u64 D = 1;
    for (u32 k = 0; k < m && t > 1; ++k)
        if (!term_mul(D, t, D))
            return kTermLimit;
    return D;
}

struct PrefixShape {
    u32 n_out;
    u32 m[kMaxPlanes], zeros[kMaxPlanes];
    u64 ranks[kMaxPlanes], D[kMaxPlanes];
};

template <typename Unit>
hipError_t prefix_launch(u64 count, u64 group, u64 t, u64 nmax, const u64 *const *in, u64 n_in, const PrefixShape &s,
                         u64 *const *out, u32 U, hipStream_t st)
{
    const u64 ub = sizeof(Unit);
    PrefixArgs a = {};
    for (u64 i = 0; i < n_in; ++i)
        a.in[i] = in[i];
    a.g = (u32)group;
    a.nmax = (u32)nmax;
    a.t = (u32)t;
    a.U = U;
    a.n_in = (u32)n_in;
    a.n_out = s.n_out;
    // the slice of units: whole terms unless the last row's inputs pass the budget; no staging below kMinChunk units
    // a slice
    u64 KC = U;
    bool staged = true;
    const u64 in_units = nmax * t;                      // below 2^31: the last row of the lowest plane holds as many terms
    if (in_units > kLdsBudget) {
        staged = false;
    } else if (in_units * U * ub > kLdsBudget) {
        const u64 fit = kLdsBudget / (in_units * ub);
        if (fit >= kMinChunk) {
            const u64 chunks = (U + fit - 1) / fit;
            KC = (U + chunks - 1) / chunks;
        } else {
            staged = false;
        }
    }
    a.KC = (u32)KC;
    a.chunks = (u32)((U + KC - 1) / KC);
    // the ranks of a workgroup, plane by plane: what the rank records hold, no more than kTargetUnits to write, parts
    // enough to fill the chip, evened out over the parts; or what knob count_cpart says, which is how the tests place
    // the split
    const int forced = tune(TUNE_COUNT_CPART);
    u64 per_elem = 0, units = 0;
    u32 rec_bytes = 0;
    bool digits = false;
    for (u32 x = 0; x < s.n_out; ++x) {
        PrefixPlane &P = a.p[x];
        const u64 m = s.m[x], ranks = s.ranks[x], cell = s.D[x] * KC;       // cell: units of one rank here
        const u64 rec = 12 + (m > 1 ? 2 * m : 4);
        const u64 capC = std::min<u64>({ranks, (kRankBytes - kRankHead) / rec, std::max<u64>(1, kMaxStream / cell)});
        u64 CP;
        if (forced > 0) {
            CP = std::min<u64>((u64)forced, capC);
        } else {
            CP = std::min<u64>(capC, std::max<u64>(1, (kTargetUnits + cell - 1) / cell));
            while (CP > 1 && count < kFillBlocks && count * a.chunks * ((ranks + CP - 1) / CP) < kFillBlocks &&
                   ((CP + 1) / 2) * cell >= kMinUnits)
                CP = (CP + 1) / 2;
            const u64 parts = (ranks + CP - 1) / CP;
            CP = (ranks + parts - 1) / parts;
        }
        P.out = out[x];
        P.m = (u32)m;
        P.D = (u32)s.D[x];
        P.ranks = ranks;
        P.CP = (u32)CP;
        P.zeros = s.zeros[x];
        P.dD = csgn_fastdiv_make(P.D);
        P.bbase = per_elem;
        per_elem += ((ranks + CP - 1) / CP) * a.chunks;
        units += (ranks * s.D[x] + s.zeros[x]) * U;
        rec_bytes = std::max<u32>(rec_bytes, (u32)(CP * rec));
        digits = digits || s.D[x] > 1;
    }
    // several elements a workgroup: where every plane of an element is one workgroup of whole staged terms that writes
    // under half of kTargetUnits, EG doubles while the inputs fit the budget, the largest plane stays within
    // kTargetUnits and the workgroups still fill the chip
    u64 EG = 1;
    if (forced <= 0 && staged && a.chunks == 1 && per_elem == s.n_out) {
        u64 largest = 0;
        for (u32 x = 0; x < s.n_out; ++x)
            largest = std::max(largest, (s.ranks[x] * s.D[x] + s.zeros[x]) * U);
        while (2 * EG * largest <= kTargetUnits && 2 * EG * in_units * U * ub <= kLdsBudget &&
               (count + 2 * EG - 1) / (2 * EG) >= kFillBlocks)
            EG *= 2;
    }
    a.EG = (u32)EG;
    a.count = count;
    a.per_elem = per_elem;
    a.dKC = csgn_fastdiv_make(a.KC);
    a.dT = csgn_fastdiv_make(a.t);
    a.dIn = csgn_fastdiv_make((u32)std::max<u64>(1, in_units * KC));
    for (u32 x = 0; x < s.n_out; ++x) {
        const u64 el_units = s.ranks[x] * s.D[x] * KC;                       // read where EG > 1: within kTargetUnits
        a.p[x].dEl = csgn_fastdiv_make(EG > 1 ? (u32)el_units : 1u);
    }
    a.sbase = staged ? (u32)((EG * in_units * KC * ub + 15u) & ~15ull) : 0u;
    const u32 lds = a.sbase + kRankHead + ((rec_bytes + 15u) & ~15u);
    a.xcd = stream_xcd(count * units);
    // the launches: the workgroups of the call in order, launch_blocks() at a time
    const u64 total = ((count + EG - 1) / EG) * per_elem, max_blocks = launch_blocks();
    for (u64 b0 = 0; b0 < total; b0 += max_blocks) {
        a.block0 = b0;
        a.nblocks = (u32)std::min(max_blocks, total - b0);
        const dim3 grid(a.nblocks);
        if (staged && digits)
            k_count_prefix<Unit, true, true><<<grid, 256, lds, st>>>(a);
        else if (staged)
            k_count_prefix<Unit, true, false><<<grid, 256, lds, st>>>(a);
        else if (digits)
            k_count_prefix<Unit, false, true><<<grid, 256, lds, st>>>(a);
        else
            k_count_prefix<Unit, false, false><<<grid, 256, lds, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 count_prefix_offset(u64 group, u64 t, u64 j, u64 exclusive, u64 r)
{
    // every row holds a term at least: a group of 2^62 rows is past the limit whatever the plane
    if (group == 0 || group >= kTermLimit || t == 0 || t >= kTermLimit || j > 6 || exclusive > 1 ||
        group - exclusive < (1ull << j) || r > group)
        return 0;
    // rows shorter than m hold one term each; the others' ranks add up to C(n_r, m+1), n_r of the row at r
    const u64 m = 1ull << j, short_rows = std::min(r, m - 1 + exclusive);
    const u64 C = sat_binom(r + 1 - exclusive, m + 1), D = sat_pow(t, (u32)m);
    u64 T;
    if (C == 0)
        return short_rows;
    if (C >= kTermLimit || D >= kTermLimit)
        return 0;
    if (!term_mul(C, D, T) || T + short_rows >= kTermLimit)
        return 0;
    return T + short_rows;
}

bool count_prefix_shape_ok(u64 count, u64 group, u64 t, u64 exclusive, u64 n_in, u64 n_out, const u64 *js)
{
    if (exclusive > 1 || group <= exclusive)
        return false;
    if (!count_shape_ok(count, group, t, n_in, n_out, js))
        return false;
    for (u64 x = 0; x < n_out; ++x)
        if ((1ull << js[x]) > group - exclusive)
            return false;
    return true;
}

hipError_t count_prefix(u64 n_bits, u64 count, u64 group, u64 t, u64 exclusive, const u64 *const *in, u64 n_in,
                        u64 n_out, const u64 *js, u64 *const *out, hipStream_t stream)
{
    const u64 nmax = group - exclusive;
    PrefixShape s = {};
    s.n_out = (u32)n_out;
    for (u32 x = 0; x < s.n_out; ++x) {
        s.m[x] = 1u << js[x];
        s.zeros[x] = (u32)(s.m[x] - 1 + exclusive);
        s.ranks[x] = sat_binom(nmax + 1, s.m[x] + 1);
        s.D[x] = sat_pow(t, s.m[x]);
    }
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(in, n_in), ptr_array(out, n_out));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? prefix_launch<unit16>(count, group, t, nmax, in, n_in, s, out, U, stream)
                : prefix_launch<unit8>(count, group, t, nmax, in, n_in, s, out, U, stream);
}

} // namespace csgn
