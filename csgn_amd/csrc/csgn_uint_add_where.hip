// csgn_uint_add_where.hip -- a + (s ? k : 0): a public constant added to an ENCRYPTED integer in the elements whose
// ENCRYPTED flag s is set; every plane of the result, the copies below the constant's lowest set bit included, and the
// carry out of the top plane in one launch.  Hand-written CDNA4 (gfx950) HIP; the tile and the launches are
// csgn_selector.h's, design notes in DESIGN.md §4.35.
//
// The definition (include/csgn_hip.h, csgn_uint_add_where) is csgn_uint_arith's ADD chain with b_j = s where k_j = 1
// and b_j ABSENT where k_j = 0, so terms are spent only where k has a set bit.  Every term of every output is decoded
// from its position: plane j is [a_j | s (k_j = 1) | the entries of c_{j-1}], and entry q of the carry c_j is a product
// term of a_j and s (q < ta_j * tn_j, which ends the walk) or a term of a_j | s ANDed with an entry of c_{j-1}.
//
// As in k_uint_arith the outputs differ in length by orders of magnitude, so the kernel walks their CONCATENATION as one
// stream of entries: a workgroup owns G elements, a slice of KC units of every term and one range of QP entries, which
// may cross from one output into the next.  One-term planes of a under a flag of at most 32 terms, the case this kernel
// is built for (a counter of 16 to 32 fresh planes and a small k): every entry is the AND of a subset of the element's
// planes and a subset of s's terms.  The workgroup decodes its range once into an LDS list (plane mask, s-term mask),
// stages its elements' operand units -- w planes and ts terms of s -- in LDS, and forms every written unit from the
// staged units named by the two masks.  Past 16 planes the subset tables of §4.15 would not fit, and the entries of a
// small k are few long prefixes a_m & ... & a_{j-1} & s: they are ANDed per entry.  Planes of several terms take the walk
// per unit straight from the planes (correct, not fast).
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kStageBudget = 40960;     // bytes of staged operand units per workgroup
constexpr u32 kMaxRange = 2048;         // entries one workgroup decodes (16 KB of LDS)
constexpr u64 kPartUnits = 8192;        // units a workgroup writes at least, where the shape has them
constexpr u64 kMinPartUnits = 1024;     // ... and where the call is small (four units a lane)
constexpr u64 kFillBlocks = 512;        // workgroups a small call is cut into where it has the units: two a CU
constexpr u32 kMaxTile = 64;            // elements of a workgroup at most
constexpr u32 kMaxSelTerms = 32;        // terms of s the staged form's mask holds
constexpr u32 kMaxOut = kAddWhereMaxWidth + 1;

// By value in the kernel arguments (uniform, scalar loads).  Output o < w is plane o and output w the carry-out.
// Output o owns entries [start[o], start[o + 1]) of the stream.
struct AddWhereArgs {
    SelTile tile;
    void *out[kMaxOut];
    const void *a[kAddWhereMaxWidth];
    const void *sel;
    u64 start[kMaxOut + 1];
    FastDivTable<kMaxOut> T;            // terms of output o
    u32 ta[kAddWhereMaxWidth];
    u32 P[kAddWhereMaxWidth];           // ta_j * tn_j: the product block at the head of c_j
    FastDivTable<kAddWhereMaxWidth> C;  // C_{j-1}, the entries of the carry into plane j (1 where there is none)
    FastDiv dts, dnx;                   // ts; nx = w + ts (w for k = 0), the staged operand slots of an element
    u32 ts, w, nout, m;                 // m: the lowest set bit of k, w for k = 0
    u32 k;
};
static_assert(sizeof(AddWhereArgs) <= 4096, "the kernel arguments of k_uint_add_where pass the 4 KiB limit");

// Entry i of output o: term(side, j, x) takes term x of plane j of a (side 0) or term x of s (side 1, j = 0).  The
// carry-out of k = 0, the ZERO term, takes nothing: its caller writes ZERO.
template <typename Term>
__host__ __device__ __forceinline__ void add_where_entry(const AddWhereArgs &a, u32 o, u32 i, Term term)
{
    u32 j = o, q = i;           // q: an entry of c_{j-1}
    if (o < a.w) {              // plane o: a_o, s where k_o is set, then c_{o-1}
        const u32 tao = a.ta[o], tno = ((a.k >> o) & 1u) ? a.ts : 0u;
        if (i < tao) {
            term(0u, o, i);
            return;
        }
        if (i < tao + tno) {
            term(1u, 0u, i - tao);
            return;
        }
        q = i - tao - tno;
    }
    while (j-- > a.m) {
        const u32 taj = a.ta[j];
        const bool set = (a.k >> j) & 1u;
        if (q < a.P[j]) {       // a_j * s
            const u32 p = csgn_fastdiv(q, a.dts);
            term(0u, j, p);
            term(1u, 0u, q - p * a.ts);
            return;
        }
        q -= a.P[j];            // (a_j | s) * c_{j-1}, or a_j * c_{j-1} where k_j = 0
        const FastDiv dc = FastDiv{a.C.d[j], a.C.magic[j], a.C.shift[j]};
        const u32 p = csgn_fastdiv(q, dc);
        q -= p * dc.d;
        if (p < taj)
            term(0u, j, p);
        else if (set)
            term(1u, 0u, p - taj);
    }
}

template <typename Unit, bool Staged>
__global__ void __launch_bounds__(256) k_uint_add_where(AddWhereArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const SelTile &t = a.tile;
    // sel_block's tile over a 64-bit stream position: (element group, unit chunk, part of the stream)
    const u32 bid = t.xcd ? xcd_contiguous_block(blockIdx.x, t.nblocks) : blockIdx.x;
    const u32 gc = bid / t.qparts, part = bid - gc * t.qparts;
    const u32 group = gc / t.chunks, k0 = (gc - group * t.chunks) * t.KC, kc = min(t.KC, t.U - k0);
    const u64 e0 = (u64)group * t.G, Q0 = (u64)part * t.QP;
    const u32 ne = (u32)min((u64)t.G, t.batch - e0), nq = (u32)min((u64)t.QP, a.start[a.nout] - Q0);
    Unit *stage = reinterpret_cast<Unit *>(smem_raw);
    uint2 *code = reinterpret_cast<uint2 *>(smem_raw + t.lbase);
    const u32 nx = a.dnx.d;

    u32 o = 0;                  // the output the range begins in
    while (a.start[o + 1] <= Q0)
        ++o;

    if (Staged) {
        // the range: the planes of a in .x, the terms of s in .y
        for (u32 i = threadIdx.x; i < nq; i += 256u) {
            const u64 Q = Q0 + i;
            u32 oo = o;
            while (a.start[oo + 1] <= Q)
                ++oo;
            u32 S[2] = {0u, 0u};
            add_where_entry(a, oo, (u32)(Q - a.start[oo]), [&](u32 side, u32 j, u32 x) { S[side] |= 1u << (side ? x : j); });
            code[i] = make_uint2(S[0], S[1]);
        }
        // the operand units of the tile: slot x < w is plane x of a, slot w + x term x of s; unit fastest
        const u32 len = ne * nx * t.KC;
        for (u32 l = threadIdx.x; l < len; l += 256u) {
            const u32 row = csgn_fastdiv(l, t.dKC), kk = l - row * t.KC;
            const u32 el = csgn_fastdiv(row, a.dnx), x = row - el * nx;
            if (kk >= kc)
                continue;
            const u64 e = e0 + el;
            stage[l] = x < a.w ? reinterpret_cast<const Unit *>(a.a[x])[e * t.U + k0 + kk]
                               : reinterpret_cast<const Unit *>(a.sel)[(e * a.ts + (x - a.w)) * t.U + k0 + kk];
        }
        __syncthreads();
    }

    // output by output: lanes take the unit fastest, then the entry and the element, so one store instruction writes
    // 64 consecutive units of one plane
    for (; o < a.nout && a.start[o] < Q0 + nq; ++o) {
        const u64 lo = max(a.start[o], Q0), hi = min(a.start[o + 1], Q0 + nq);
        const u32 n = (u32)(hi - lo), c0 = (u32)(lo - Q0), i0 = (u32)(lo - a.start[o]);
        // the range's share of this output: the whole output or a whole part, whose divisions the host made, or a cut
        const FastDiv dn = n == a.T.d[o] ? a.T.at(o) : n == t.QP ? t.dQP : csgn_fastdiv_make(n);
        const u64 To = a.T.d[o];
        const bool zero = a.k == 0u && o == a.w;    // the carry-out of k = 0
        Unit *out = reinterpret_cast<Unit *>(a.out[o]);
        const u32 len = ne * n * t.KC;              // below 2^32 by SelTile::set
        for (u32 l = threadIdx.x; l < len; l += 256u) {
            const u32 en = csgn_fastdiv(l, t.dKC), kk = l - en * t.KC;
            const u32 el = csgn_fastdiv(en, dn), qi = en - el * n;
            if (kk >= kc)
                continue;
            const u32 k = k0 + kk;
            const u64 e = e0 + el;
            Unit v = one_unit(Unit(), k, t.U, t.last_mask);
            if (zero) {
                v = zero_unit(Unit());
            } else if (Staged) {
                const uint2 cd = code[c0 + qi];
                const Unit *row = stage + el * nx * t.KC + kk;
                for (u32 pm = cd.x; pm; pm &= pm - 1u)
                    v &= row[(u32)__builtin_ctz(pm) * t.KC];
                row += a.w * t.KC;
                for (u32 sm = cd.y; sm; sm &= sm - 1u)
                    v &= row[(u32)__builtin_ctz(sm) * t.KC];
            } else {
                add_where_entry(a, o, i0 + qi, [&](u32 side, u32 j, u32 x) {
                    v &= side == 0u ? reinterpret_cast<const Unit *>(a.a[j])[(e * a.ta[j] + x) * t.U + k]
                                    : reinterpret_cast<const Unit *>(a.sel)[(e * a.ts + x) * t.U + k];
                });
            }
            unit_store<Unit, true>(out + (e * To + i0 + qi) * t.U + k, v);
        }
    }
}

// ------------------------------------------------------------------------------ host side

// x + y, saturated at kTermLimit (as sat_mul, csgn_selector.h)
u64 sat_add(u64 x, u64 y)
{
    return x >= kTermLimit || y >= kTermLimit || x + y >= kTermLimit ? kTermLimit : x + y;
}

// The terms of every output (T[o], o <= w) and of every carry (C[j] = C_j; 0 below the lowest set bit of k); a count of
// 2^62 or more is kTermLimit.  false for a bad width or k, a null pointer or a count of 0 or of 2^62 or more.
bool add_where_counts(u64 w, u64 k, u64 ts, const u64 *ta, u64 *T, u64 *C)
{
    if (w < 1 || w > kAddWhereMaxWidth || (k >> w) != 0 || !ta || ts == 0 || ts >= kTermLimit)
        return false;
    for (u64 j = 0; j < w; ++j)
        if (ta[j] == 0 || ta[j] >= kTermLimit)
            return false;
    u64 c = 0;
    for (u64 j = 0; j < w; ++j) {
        const u64 tn = ((k >> j) & 1) ? ts : 0, ab = sat_add(ta[j], tn);
        T[j] = sat_add(ab, c);
        c = sat_add(sat_mul(ta[j], tn), sat_mul(ab, c));
        C[j] = c;
    }
    T[w] = k ? c : 1;           // k = 0: the one ZERO term
    return true;
}

// The arguments but the tile, the pointers and the launch: the level tables of nout outputs.  Returns whether the staged
// form's masks hold the shape.
bool add_where_fill(AddWhereArgs &a, u64 w, u64 k, u64 ts, const u64 *ta, bool carry, const u64 *T, const u64 *C)
{
    a.w = (u32)w;
    a.k = (u32)k;
    a.ts = (u32)std::min<u64>(ts, 0xFFFFFFFFull);       // read only where k has a set bit: then below every T
    a.nout = (u32)w + (carry ? 1u : 0u);
    a.m = k ? (u32)__builtin_ctzll(k) : (u32)w;
    a.dts = csgn_fastdiv_make(a.ts);
    a.dnx = csgn_fastdiv_make((u32)(w + (k ? std::min<u64>(ts, kMaxSelTerms) : 0)));   // k = 0 reads no s
    bool fresh = ts <= kMaxSelTerms;
    for (u32 j = 0; j < w; ++j) {
        a.ta[j] = (u32)ta[j];
        // the walk reads P_j and C_{j-1} only on the way down from an output that is written: both are below its terms
        const bool read = j + 1 < a.nout && j >= a.m;
        a.P[j] = read && ((k >> j) & 1) ? (u32)(ta[j] * ts) : 0u;
        a.C.set(j, read && j > a.m ? (u32)C[j - 1] : 1u);
        fresh = fresh && ta[j] == 1;
    }
    u64 total = 0;
    for (u32 o = 0; o < a.nout; ++o) {
        a.T.set(o, (u32)T[o]);
        a.start[o] = total;
        total += T[o];
    }
    a.start[a.nout] = total;
    return fresh;
}

// The tile of a call whose level tables are filled (add_where_fill; `staged`: its answer): the unit slices, the range of
// entries and the elements of a workgroup.  Returns the LDS bytes of the staged form, 0 for the walk.
u32 add_where_plan(AddWhereArgs &a, u64 n_bits, u64 batch, u32 U, u32 unit_bytes, bool staged)
{
    const u64 total = a.start[a.nout];
    // The unit slices: only where one element's staged units at whole terms pass the budget.
    SubsetPlan sp = {};
    const u64 nx = a.dnx.d, per_unit = nx * unit_bytes;
    const u32 chunks = staged && per_unit * U > kStageBudget ? (u32)((per_unit * U + kStageBudget - 1) / kStageBudget) : 1u;
    sp.unit_bytes = unit_bytes;
    sp.KC = (U + chunks - 1) / chunks;
    sp.chunks = (U + sp.KC - 1) / sp.KC;
    sp.max_G = staged ? std::max<u64>(1, kStageBudget / (per_unit * sp.KC)) : ~0ull;
    // a stream too long for one launch's workgroups at kMaxRange entries each takes the walk, whose range may grow
    staged = staged && ((total + kMaxRange - 1) / kMaxRange) * sp.chunks <= kMaxBlocks256;
    // The range of entries a workgroup takes: the shortest with which one element gives it part_units to write and
    // eight times what it stages, no more than the LDS list holds -- then elements until it has as much.  A call of few
    // units is cut finer, down to kMinPartUnits a workgroup, so that it still has kFillBlocks of them.
    const u64 fill = std::min<u64>(kPartUnits, std::max<u64>(kMinPartUnits, batch * total * U / kFillBlocks));
    const u64 part_units = std::max<u64>(fill, staged ? 8 * nx * sp.KC : 0);
    u64 want_QP = std::min<u64>({(part_units + sp.KC - 1) / sp.KC, (u64)kMaxRange, total});
    if (!staged)
        want_QP = std::max<u64>(want_QP, (total * sp.chunks + kMaxBlocks256 - 1) / kMaxBlocks256);
    const u64 qparts = (total + want_QP - 1) / want_QP;
    const u64 QP = (total + qparts - 1) / qparts;
    const u64 capG = std::min<u64>({sp.max_G, batch, kMaxTile});
    const u64 G = std::max<u64>(1, std::min<u64>(capG, (part_units + QP * sp.KC - 1) / (QP * sp.KC)));
    SelOutputs<1> stream = {};                      // the tile's view: one stream of one term per entry
    stream.fill(0, [](u32) { return 0; }, true, sp.KC);
    a.tile.set(n_bits, U, sp, QP, total, stream, G);
    a.tile.xcd = stream_xcd(batch * total * U);
    if (!staged)
        return 0;
    a.tile.base2 = a.tile.lbase = (u32)((a.tile.G * nx * sp.KC * unit_bytes + 15u) & ~15ull);
    return a.tile.lbase + a.tile.QP * 8u;
}

template <typename Unit>
hipError_t add_where_launch(u64 n_bits, u64 batch, u64 w, u64 k, const u64 *sel, u64 ts, const u64 *const *pa,
                            const u64 *ta, u64 *const *out, u64 *carry, const u64 *T, const u64 *C, u32 U, hipStream_t st)
{
    AddWhereArgs a = {};
    const bool staged = add_where_fill(a, w, k, ts, ta, carry != nullptr, T, C);
    const u32 lds = add_where_plan(a, n_bits, batch, U, (u32)sizeof(Unit), staged);
    return sel_launch(k_uint_add_where<Unit, true>, k_uint_add_where<Unit, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        for (u32 j = 0; j < w; ++j)
            a.a[j] = reinterpret_cast<const Unit *>(pa[j]) + e0 * ta[j] * U;
        a.sel = sel ? reinterpret_cast<const Unit *>(sel) + e0 * ts * U : nullptr;
        for (u32 o = 0; o < a.nout; ++o)
            a.out[o] = reinterpret_cast<Unit *>(o < w ? out[o] : carry) + e0 * T[o] * U;
    });
}

} // namespace

// ------------------------------------------------------------------------------ public

bool uint_add_where_terms(u64 w, u64 k, u64 ts, const u64 *ta, u64 *T)
{
    u64 t[kMaxOut], C[kAddWhereMaxWidth];
    if (!T || !add_where_counts(w, k, ts, ta, t, C))
        return false;
    for (u64 o = 0; o <= w; ++o)
        if (t[o] >= kTermLimit)
            return false;
    std::copy(t, t + w + 1, T);
    return true;
}

u64 uint_add_where_output_terms(u64 w, u64 k, u64 ts, const u64 *ta, u64 output)
{
    u64 T[kMaxOut], C[kAddWhereMaxWidth];
    if (!add_where_counts(w, k, ts, ta, T, C) || output > w)
        return 0;
    return T[output] >= kTermLimit ? 0 : T[output];
}

hipError_t uint_add_where(u64 n_bits, u64 batch, u64 w, u64 k, const u64 *sel, u64 ts, const u64 *const *a,
                          const u64 *ta, u64 *const *out, u64 *carry, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    u64 T[kMaxOut], C[kAddWhereMaxWidth];
    if (!add_where_counts(w, k, ts, ta, T, C) || (k != 0 && !sel))
        return hipErrorInvalidValue;
    for (u64 o = 0; o < w + (carry ? 1 : 0); ++o)
        if (T[o] >= kTermLimit)
            return hipErrorInvalidValue;
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(a, w), sel, ptr_array(out, w), carry);
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? add_where_launch<unit16>(n_bits, batch, w, k, sel, ts, a, ta, out, carry, T, C, U, stream)
                : add_where_launch<unit8>(n_bits, batch, w, k, sel, ts, a, ta, out, carry, T, C, U, stream);
}

} // namespace csgn
