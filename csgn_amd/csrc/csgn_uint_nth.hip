// csgn_uint_nth.hip -- the (slot + 1)-th row of a group whose ENCRYPTED mask bit is set: its value planes, "at least
// slot + 1 bits are set" and the planes of its public label, every output in one launch.  Hand-written CDNA4 (gfx950)
// HIP; the kernel skeleton in csgn_selector.h, design notes in DESIGN.md §4.33.
//
// The definition (include/csgn_hip.h, csgn_uint_nth): for a row r >= s = slot, G_{r,s} is the sum, over d ascending in
// s..r with C(d, s) odd and over the d-subsets i_1 < ... < i_d of the rows below r in lexicographic order, of
// m_{i_1} * ... * m_{i_d} * m_r; out_j = sum over r of G_{r,s} * d_{r,j}, valid = sum of G_{r,s}, lab_i = sum of the
// G_{r,s} whose label has bit i.  C(d, s) is odd exactly when every bit of s is a bit of d (Lucas), so a SEGMENT is a pair
// (r, d) with s a submask of d <= r; it has C(r, d) * t^(d+1) entries, the segments of a row ascend in d, the rows in r,
// and the stream has Q = sum over d of C(g, d+1) * t^(d+1) entries.  Inside a segment entry = rank * t^(d+1) + digits,
// the digits in base t with i_1's slowest and m_r's fastest.  Term q * t_j + c of out_j is (entry q) & (term c of
// d_{r,j}); valid is the bare stream; lab_i is the bare stream without the blocks of the rows whose label lacks bit i.
//
// A workgroup builds the segment starts in static LDS from g, s and t -- Pascal's rows by the additive recurrence, one
// row a barrier, saturated at 2^32 - 1: a kept segment and every binomial above it are exact, because the host has
// checked Q -- and finds an entry's segment by bisection of them; nothing is read from a device table.  Fresh masks
// (t = 1) of up to 16 rows, the case this kernel is built for: an entry is the AND of a subset of the rows, the subset
// of rank (q - start) under r (unrank, csgn_device.h) with r added.  A workgroup owns G elements, a slice of KC units of
// every term and QP entries, for EVERY output: it builds the subset tables of §4.15 over its elements' rows and decodes
// its entries once into an LDS list (subset in the low 16 bits, row in the high 16); a written unit is then 1-3 LDS
// reads ANDed with one unit of the value row.  Larger groups and multi-term masks take the digits per unit straight
// from the rows (correct, not fast).
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kNthMaxFresh = 16;        // rows the subset tables and the 16-bit subsets of the LDS list hold

// By value in the kernel arguments (uniform, scalar loads).  Outputs [0, w) are the value planes, output w, where outs
// has it, is valid.  The label planes are bare outputs of their own.
struct NthArgs {
    SelTile tile;
    SelOutputs<kNthMaxPlanes + 1> outs;
    const void *mask[kNthMaxGroup];     // term 0 of row r of the launch's first element
    const void *values[kNthMaxPlanes];
    void *lab[kNthMaxLabels];
    u64 keep[kNthMaxLabels];            // label plane i keeps row r: bit r (rows >= slot only)
    u32 Q;                              // entries of the stream
    u32 g, slot, t, w, nlab;
    u32 gm;                             // an element's rows lie gm * t terms apart: g in the grouped layout, else 1
    SubsetTables tabs;
};
static_assert(sizeof(NthArgs) <= 4096, "the kernel arguments of k_uint_nth pass the 4 KiB limit");

// The static LDS of a workgroup: one struct of a multiple of 16 bytes, so that the dynamic LDS behind it (the tables'
// 16-byte units) stays aligned.  The Fresh form holds 16 rows, so 136 segments; the other 64 rows and 2080.
template <bool Fresh>
struct __align__(16) NthLds {
    static constexpr u32 kRows = Fresh ? kNthMaxFresh : kNthMaxGroup;
    static constexpr u32 kSegs = kRows * (kRows + 1u) / 2u;
    u32 start[(kSegs + 4u) & ~3u];      // segment i holds entries [start[i], start[i + 1])
    u32 bin[2][kRows + 4u];             // Pascal's row r and the one being made
    u32 sb[kRows + 4u];                 // row r's first segment; sb[g]: the number of segments
    u32 row[kRows + 4u];                // row r's first entry; row[g] = Q
    u32 skip[kRows + 4u];               // of one label plane at a time: the entries of the rows below r it leaves out
    unsigned short rd[(kSegs + 7u) & ~7u];      // segment i: r << 8 | d
};
static_assert(sizeof(NthLds<true>) % 16 == 0 && sizeof(NthLds<false>) % 16 == 0, "the dynamic LDS stays 16-byte aligned");

__device__ __forceinline__ bool nth_kept(u32 s, u32 d) { return d >= s && (s & ~d) == 0u; }

// The segment table of (g, s, t), by all 256 threads; complete at the closing barrier.
template <bool Fresh>
__device__ inline void nth_build(NthLds<Fresh> &L, u32 g, u32 s, u32 t)
{
    const u32 x = threadIdx.x;          // a column d of Pascal's triangle, and a row r of the stream
    u32 rank = 0, pw = 0;               // of column x: the kept columns below it, t^(x+1) (saturated)
    if (x <= g) {
        u32 base = 0;                   // the segments of the rows below x
        for (u32 r = s; r < x; ++r)
            for (u32 d = s; d <= r; ++d)
                base += nth_kept(s, d) ? 1u : 0u;
        L.sb[x] = base;
        for (u32 d = s; d < x; ++d)
            rank += nth_kept(s, d) ? 1u : 0u;
        u64 p = t;
        for (u32 i = 0; i < x; ++i)
            p = min(p * t, 0xFFFFFFFFull);
        pw = (u32)p;
        L.bin[0][x] = x == 0u ? 1u : 0u;
        L.row[x] = 0u;
    }
    if (x == 0)
        L.start[0] = 0u;
    __syncthreads();
    // row r of the triangle: the lengths of its segments into start[i + 1], then the row after it
    for (u32 r = 0; r < g; ++r) {
        const u32 *cur = L.bin[r & 1u];
        u32 *nxt = L.bin[(r & 1u) ^ 1u];
        if (x <= r && r >= s && nth_kept(s, x)) {
            const u32 i = L.sb[r] + rank;
            L.start[i + 1u] = (u32)min((u64)cur[x] * pw, 0xFFFFFFFFull);
            L.rd[i] = (unsigned short)((r << 8) | x);
        }
        if (x <= r + 1u && x <= g) {
            const u32 up = x <= r ? cur[x] : 0u, left = x > 0u ? cur[x - 1u] : 0u, sum = up + left;
            nxt[x] = sum < up ? 0xFFFFFFFFu : sum;
        }
        __syncthreads();
    }
    // the lengths into ends: each row's own, then the rows', then both
    if (x < g && x >= s) {
        u32 acc = 0;
        for (u32 i = L.sb[x]; i < L.sb[x + 1u]; ++i)
            acc += L.start[i + 1u];
        L.row[x + 1u] = acc;            // Q < 2^32: no sum of kept segments wraps
    }
    __syncthreads();
    if (x == 0)
        for (u32 r = 0; r < g; ++r)
            L.row[r + 1u] += L.row[r];
    __syncthreads();
    if (x < g && x >= s) {
        u32 acc = L.row[x];
        for (u32 i = L.sb[x]; i < L.sb[x + 1u]; ++i) {
            acc += L.start[i + 1u];
            L.start[i + 1u] = acc;
        }
    }
    __syncthreads();
}

// The segment of entry q < Q: start[seg] <= q < start[seg + 1]
template <bool Fresh>
__device__ __forceinline__ u32 nth_segment(const NthLds<Fresh> &L, u32 g, u32 q)
{
    u32 lo = 0, hi = L.sb[g];
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (L.start[mid] <= q)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The row of entry q = b.q0 + qi; the digit form also gives its segment.
template <typename Unit, bool Fresh>
__device__ __forceinline__ u32 nth_row(const NthArgs &a, const SelBlock<Unit> &b, const NthLds<Fresh> &L, u32 qi, u32 q,
                                       u32 &seg)
{
    if (Fresh)
        return b.code[qi] >> 16;
    seg = nth_segment(L, a.g, q);
    return L.rd[seg] >> 8;
}

// Entry q of row r (segment seg) at unit k = b.k0 + kk of element e = b.e0 + el
template <typename Unit, bool Fresh>
__device__ __forceinline__ Unit nth_entry(const NthArgs &a, const SelTile &t, const SelBlock<Unit> &b,
                                          const NthLds<Fresh> &L, u32 el, u64 e, u32 qi, u32 q, u32 r, u32 seg, u32 k,
                                          u32 kk)
{
    if (Fresh)
        return subset_and(b.tab, a.tabs, el, b.code[qi] & 0xFFFFu, t.KC, kk);
    const u32 d = L.rd[seg] & 0xFFu, tm = a.t, rest = q - L.start[seg];
    u32 pw = tm;                        // t^(d+1), at most the segment's entries
    for (u32 i = 0; i < d; ++i)
        pw *= tm;
    const u32 rank = rest / pw, dig = rest - rank * pw;
    const u64 eg = e * a.gm;
    Unit v = reinterpret_cast<const Unit *>(a.mask[r])[(eg * tm + dig % tm) * t.U + k];
    u32 div = pw;                       // i_1's digit is the slowest: position x has weight t^(d-x)
    unrank(r, d, (u64)rank, [&](u32, u32 i) {
        div /= tm;
        v &= reinterpret_cast<const Unit *>(a.mask[i])[(eg * tm + (dig / div) % tm) * t.U + k];
    });
    return v;
}

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_nth(NthArgs a)
{
    __shared__ NthLds<Fresh> L;
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit>(t, a.Q);

    nth_build(L, a.g, a.slot, a.t);
    if (Fresh) {
        // the range of q: the subset in the low 16 bits, the row in the high 16 (published by the tables' closing barrier)
        for (u32 i = threadIdx.x; i < b.nq; i += 256u) {
            const u32 q = b.q0 + i, seg = nth_segment(L, a.g, q), rd = L.rd[seg], r = rd >> 8;
            u32 sub = 1u << r;
            unrank(r, rd & 0xFFu, (u64)(q - L.start[seg]), [&](u32, u32 v) { sub |= 1u << v; });
            b.code[i] = sub | (r << 16);
        }
        subset_build(b.tab, a.tabs, a.mask, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc, a.gm * t.U);
    }

    for (u32 j = 0; j < a.outs.nout; ++j) {
        const u32 tj = a.outs.t[j];
        const u64 Tj = (u64)tj * a.Q;
        const bool has_value = j < a.w;
        const Unit *d = reinterpret_cast<const Unit *>(has_value ? a.values[j] : nullptr);
        sel_walk<Unit>(t, b, a.outs, j, b.ne, [&](u32 el, u32 qi, u32 c, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk, q = b.q0 + qi;
            const u64 e = b.e0 + el;
            u32 seg = 0;
            const u32 r = nth_row<Unit, Fresh>(a, b, L, qi, q, seg);
            v = nth_entry<Unit, Fresh>(a, t, b, L, el, e, qi, q, r, seg, k, kk);
            if (has_value)
                v &= d[((e * a.g + r) * tj + c) * t.U + k];
            at = (e * Tj + (u64)q * tj + c) * t.U + k;
            return true;
        });
    }

    // the label planes: bare outputs of one term per kept entry
    SelOutputs<1> lo;
    lo.t[0] = 1u;
    lo.tk.d[0] = t.dKC.d;
    lo.tk.magic[0] = t.dKC.magic;
    lo.tk.shift[0] = t.dKC.shift;
    lo.nout = 1u;
    for (u32 i = 0; i < a.nlab; ++i) {
        const u64 keep = a.keep[i];
        __syncthreads();                        // the plane before has read its skips
        if (threadIdx.x <= a.g) {
            u32 sk = 0;
            for (u32 x = 0; x < threadIdx.x; ++x)
                if (!((keep >> x) & 1u))
                    sk += L.row[x + 1u] - L.row[x];
            L.skip[threadIdx.x] = sk;
        }
        __syncthreads();
        const u64 Ti = a.Q - L.skip[a.g];
        lo.out[0] = a.lab[i];
        sel_walk<Unit>(t, b, lo, 0u, b.ne, [&](u32 el, u32 qi, u32, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk, q = b.q0 + qi;
            const u64 e = b.e0 + el;
            u32 seg = 0;
            const u32 r = nth_row<Unit, Fresh>(a, b, L, qi, q, seg);
            if (!((keep >> r) & 1u))
                return false;
            v = nth_entry<Unit, Fresh>(a, t, b, L, el, e, qi, q, r, seg, k, kk);
            at = (e * Ti + (q - L.skip[r])) * t.U + k;
            return true;
        });
    }
}

// ------------------------------------------------------------------------------ host side

constexpr u64 kSat = kTermLimit;        // a saturated count: 2^62 "or more"

u64 nth_sat_add(u64 x, u64 y) { return x >= kSat || y >= kSat || x + y >= kSat ? kSat : x + y; }

// C(n, k), saturated: the values on the way only grow, so the first that passes the limit settles it
u64 nth_binom(u64 n, u64 k)
{
    if (k > n)
        return 0;
    k = std::min(k, n - k);
    unsigned __int128 c = 1;
    for (u64 i = 1; i <= k; ++i) {
        c = c * (n - k + i) / i;
        if (c >= kSat)
            return kSat;
    }
    return (u64)c;
}

// sum over d in s..top with C(d, s) odd of C(n, d + up) * t^(d+1), saturated: P_{r,s} is (n = r, top = r, up = 0), Q_s
// is (n = g, top = g - 1, up = 1)
u64 nth_sum(u64 n, u64 top, u64 up, u64 s, u64 t)
{
    u64 T = 0, pw = 1;
    for (u64 d = 0; d <= top; ++d) {
        pw = sat_mul(pw, t);            // t^(d+1)
        if (d >= s && (s & ~d) == 0)
            T = nth_sat_add(T, sat_mul(nth_binom(n, d + up), pw));
    }
    return T;
}

bool nth_shape_ok(u64 g, u64 t, u64 slot)
{
    return g >= 1 && g <= kNthMaxGroup && slot < g && t != 0 && t < kTermLimit;
}

template <typename Unit>
hipError_t nth_launch(u64 n_bits, u64 batch, u64 g, u64 slot, const u64 *const *mask, u64 n_mask, u64 tm, u64 w,
                      const u64 *const *values, const u64 *tv, u64 *const *out, u64 *valid, u64 nlab, const u64 *keep,
                      const u64 *Tlab, u64 *const *label_out, u64 Q, u32 U, hipStream_t st)
{
    NthArgs a = {};
    a.g = (u32)g;
    a.slot = (u32)slot;
    a.t = (u32)tm;
    a.w = (u32)w;
    a.nlab = (u32)nlab;
    a.Q = (u32)Q;
    a.gm = n_mask == 1 ? (u32)g : 1u;
    const bool fresh = g <= kNthMaxFresh && tm == 1;
    const SubsetPlan sp = ReadTile::plan(fresh, g, U, (u32)sizeof(Unit));
    u64 sumt = a.outs.fill(w, [&](u32 j) { return tv[j]; }, valid != nullptr, sp.KC);
    u64 elem_terms = Q * sumt;                  // terms an element writes
    for (u32 i = 0; i < nlab; ++i) {
        a.keep[i] = keep[i];
        elem_terms += Tlab[i];
    }
    const u32 nout = a.outs.nout;
    if (nout == 0)                              // label planes only: the tile of one bare output
        a.outs.fill(0, [](u32) { return 0; }, true, sp.KC);
    const ReadTile rt = ReadTile::of(sp, batch, Q, elem_terms * sp.KC);
    a.tile.set(n_bits, U, sp, rt.QP, Q, a.outs, rt.G);
    a.outs.nout = nout;
    const u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.tabs) : 0u;
    a.tile.xcd = stream_xcd(batch * elem_terms * U);
    return sel_launch(k_uint_nth<Unit, true>, k_uint_nth<Unit, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        for (u32 r = 0; r < g; ++r)
            a.mask[r] = reinterpret_cast<const Unit *>(n_mask == 1 ? mask[0] : mask[r]) +
                        (e0 * a.gm + (n_mask == 1 ? r : 0u)) * tm * U;
        for (u32 j = 0; j < nout; ++j) {
            if (j < w)                          // valid, output w, has no value plane
                a.values[j] = reinterpret_cast<const Unit *>(values[j]) + e0 * g * tv[j] * U;
            a.outs.out[j] = reinterpret_cast<Unit *>(j < w ? out[j] : valid) + e0 * Q * a.outs.t[j] * U;
        }
        for (u32 i = 0; i < nlab; ++i)
            a.lab[i] = reinterpret_cast<Unit *>(label_out[i]) + e0 * Tlab[i] * U;
    });
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_nth_terms(u64 g, u64 t, u64 slot, u64 row)
{
    if (!nth_shape_ok(g, t, slot) || row > g)
        return 0;
    if (row < slot)                             // no entries: a row below the slot is never the (slot + 1)-th
        return 0;
    const u64 T = row == g ? nth_sum(g, g - 1, 1, slot, t) : nth_sum(row, row, 0, slot, t);
    return T < kTermLimit ? T : 0;
}

u64 uint_nth_label_terms(u64 g, u64 t, u64 slot, const u64 *labels, u64 bit)
{
    if (!nth_shape_ok(g, t, slot) || !labels || bit > 63)
        return 0;
    u64 T = 0;
    for (u64 r = slot; r < g; ++r) {
        if (!((labels[r] >> bit) & 1u))
            continue;
        const u64 P = uint_nth_terms(g, t, slot, r);
        if (P == 0 || (T += P) >= kTermLimit)
            return 0;
    }
    return T;
}

hipError_t uint_nth(u64 n_bits, u64 batch, u64 g, u64 slot, const u64 *const *mask, u64 n_mask, u64 tm, u64 w,
                    const u64 *const *values, const u64 *t, u64 *const *out, u64 *valid, u64 n_labels, const u64 *labels,
                    const u64 *label_bits, u64 *const *label_out, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    u64 keep[kNthMaxLabels], Tlab[kNthMaxLabels];
    for (u64 i = 0; i < n_labels; ++i) {
        keep[i] = 0;
        for (u64 r = slot; r < g; ++r)
            if ((labels[r] >> label_bits[i]) & 1u)
                keep[i] |= 1ull << r;
        Tlab[i] = uint_nth_label_terms(g, tm, slot, labels, label_bits[i]);
    }
    const u64 Q = uint_nth_terms(g, tm, slot, g);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(mask, n_mask), ptr_array(values, w), ptr_array(out, w), valid,
                                 ptr_array(label_out, n_labels));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? nth_launch<unit16>(n_bits, batch, g, slot, mask, n_mask, tm, w, values, t, out, valid, n_labels, keep,
                                     Tlab, label_out, Q, U, stream)
                : nth_launch<unit8>(n_bits, batch, g, slot, mask, n_mask, tm, w, values, t, out, valid, n_labels, keep,
                                    Tlab, label_out, Q, U, stream);
}

} // namespace csgn
