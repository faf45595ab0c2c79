// csgn_uint_arith.hip -- a + b, a - b, a == b and a != b of two ENCRYPTED integers: every plane of the result, and the
// carry out of the top plane, in one launch.  Hand-written CDNA4 (gfx950) HIP; the tile, the LDS layout and the launches
// are csgn_selector.h's, design notes in DESIGN.md §4.28.
//
// The definition (include/csgn_hip.h, csgn_uint_arith) is the chain of csgn_uint_step calls certfhe/UInt.h began with:
// ADD_HALF and ADD_FULL over the planes for ADD, ADD_FULL over a_j and b_j + ONE with a first carry of ONE for SUB, the
// XNOR gate and EQ_STEP for EQ, and EQ + ONE for NE.  Every term of every output is decoded from its position: plane j of
// a sum is [a_j | b_j (| ONE) | the entries of c_{j-1}], and entry q of the carry c_j is a product term of a_j and b_j
// (q < ta_j * tb_j, which ends the walk) or a term of a_j | b_j ANDed with an entry of c_{j-1}; an entry of EQ is its
// mixed-radix digits, the decode k_uint_find does for a key row (eq_digits, csgn_selector.h).
//
// The outputs of a call differ in length by orders of magnitude (a fresh 8-bit sum: 2 to 129 terms, and a carry of 255),
// so the kernel walks their CONCATENATION as one stream of entries: a workgroup owns G elements, a slice of KC units of
// every term and one range of QP entries, which may cross from one output into the next.  Fresh planes (every
// ta_j = tb_j = 1), the case this kernel is built for: every entry is Pa_e[Sa] & Pb_e[Sb], the ANDs of subsets of the
// element's a planes and b planes (ONE is the empty subset).  The workgroup decodes its range once into an LDS list
// (Sa | Sb << 16) and builds the subset tables of §4.15 (csgn_device.h) twice; a written unit is then 2-6 LDS reads.
// Multi-term planes take the walk per unit straight from the planes (correct, not fast).
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kTableBudget = 20480;     // bytes of subset tables per workgroup, each of the two sets (48 KB with the list)
constexpr u32 kMaxRange = 2048;         // entries one workgroup decodes (8 KB of LDS)
constexpr u64 kPartUnits = 8192;        // units a workgroup writes at least, where the shape has them
constexpr u64 kMinPartUnits = 1024;     // ... and where the call is small (four units a lane)
constexpr u64 kFillBlocks = 512;        // workgroups a small call is cut into where it has the units: two a CU
constexpr u32 kMaxTile = 64;            // elements of a workgroup at most
constexpr u32 kMaxOut = kArithMaxWidth + 1;

// By value in the kernel arguments (uniform, scalar loads).  Output o < w of ADD / SUB is plane o and output w the
// carry-out; EQ / NE have output 0 alone.  Output o owns entries [start[o], start[o + 1]) of the stream.
struct ArithArgs {
    SelTile tile;
    void *out[kMaxOut];
    const void *a[kArithMaxWidth];
    const void *b[kArithMaxWidth];
    u64 start[kMaxOut + 1];
    FastDivTable<kMaxOut> T;            // terms of output o
    u32 ta[kArithMaxWidth], tb[kArithMaxWidth];
    u32 P[kArithMaxWidth];              // ta_j * tn_j: the product block at the head of c_j
    FastDivTable<kArithMaxWidth> tn;    // the terms of b_j, or of b_j + ONE for SUB
    FastDivTable<kArithMaxWidth> C;     // C_{j-1}, the entries of the carry into plane j (1 where there is none)
    u32 op, w, nout, eq;                // eq: the entries of EQ (NE: one more, the closing ONE)
    SubsetTables tabs;          // the a tables of G elements; the b tables, the tile's second set, have the same layout
};
static_assert(sizeof(ArithArgs) <= 4096, "the kernel arguments of k_uint_arith pass the 4 KiB limit");

// Entry i of output o: term(side, j, x) takes term x of plane j of a (side 0) or b (side 1); ONE takes nothing.
template <bool Fresh, typename Term>
__device__ __forceinline__ void arith_entry(const ArithArgs &a, u32 o, u32 i, Term term)
{
    if (a.op >= CSGN_UINT_ARITH_EQ) {
        if (i < a.eq)
            eq_digits<Fresh>(i, a.w, a.ta, a.tb, term);
        return;
    }
    u32 j = o, q = i;           // q: an entry of c_{j-1}
    if (o < a.w) {              // plane o: a_o, b_o (and ONE), then c_{o-1}
        const u32 tao = a.ta[o], tno = a.tn.d[o];
        if (i < tao) {
            term(0u, o, i);
            return;
        }
        if (i < tao + tno) {
            if (i - tao < a.tb[o])
                term(1u, o, i - tao);
            return;
        }
        q = i - tao - tno;
    }
    while (j-- > 0u) {
        const FastDiv dn = a.tn.at(j);
        if (q < a.P[j]) {       // a_j * nb_j
            const u32 p = csgn_fastdiv(q, dn), c = q - p * dn.d;
            term(0u, j, p);
            if (c < a.tb[j])
                term(1u, j, c);
            return;
        }
        q -= a.P[j];            // (a_j | nb_j) * c_{j-1}
        const FastDiv dc = a.C.at(j);
        const u32 p = csgn_fastdiv(q, dc), taj = a.ta[j];
        q -= p * dc.d;
        if (p < taj)
            term(0u, j, p);
        else if (p - taj < a.tb[j])
            term(1u, j, p - taj);
    }
    // c_{-1} of SUB: ONE
}

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_arith(ArithArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const SelTile &t = a.tile;
    // sel_block's tile over a 64-bit stream position: (element group, unit chunk, part of the stream)
    const u32 bid = t.xcd ? xcd_contiguous_block(blockIdx.x, t.nblocks) : blockIdx.x;
    const u32 gc = bid / t.qparts, part = bid - gc * t.qparts;
    const u32 group = gc / t.chunks, k0 = (gc - group * t.chunks) * t.KC, kc = min(t.KC, t.U - k0);
    const u64 e0 = (u64)group * t.G, Q0 = (u64)part * t.QP;
    const u32 ne = (u32)min((u64)t.G, t.batch - e0), nq = (u32)min((u64)t.QP, a.start[a.nout] - Q0);
    Unit *tab = reinterpret_cast<Unit *>(smem_raw), *tab2 = reinterpret_cast<Unit *>(smem_raw + t.base2);
    u32 *code = reinterpret_cast<u32 *>(smem_raw + t.lbase);

    u32 o = 0;                  // the output the range begins in
    while (a.start[o + 1] <= Q0)
        ++o;

    if (Fresh) {
        // the range: Sa in the low 16 bits, Sb in the high 16 (published by the tables' closing barrier)
        for (u32 i = threadIdx.x; i < nq; i += 256u) {
            const u64 Q = Q0 + i;
            u32 oo = o;
            while (a.start[oo + 1] <= Q)
                ++oo;
            u32 S[2] = {0u, 0u};
            arith_entry<true>(a, oo, (u32)(Q - a.start[oo]), [&](u32 side, u32 j, u32) { S[side] |= 1u << j; });
            code[i] = S[0] | (S[1] << 16);
        }
        subset_build(tab, a.tabs, a.a, t.G, t.KC, t.dKC, t.U, t.last_mask, e0, ne, k0, kc);
        subset_build(tab2, a.tabs, a.b, t.G, t.KC, t.dKC, t.U, t.last_mask, e0, ne, k0, kc);
    }

    // output by output: lanes take the unit fastest, then the entry and the element, so one store instruction writes
    // 64 consecutive units of one plane
    for (; o < a.nout && a.start[o] < Q0 + nq; ++o) {
        const u64 lo = max(a.start[o], Q0), hi = min(a.start[o + 1], Q0 + nq);
        const u32 n = (u32)(hi - lo), c0 = (u32)(lo - Q0), i0 = (u32)(lo - a.start[o]);
        // the range's share of this output: the whole output or a whole part, whose divisions the host made, or a cut
        const FastDiv dn = n == a.T.d[o] ? a.T.at(o) : n == t.QP ? t.dQP : csgn_fastdiv_make(n);
        const u64 To = a.T.d[o];
        Unit *out = reinterpret_cast<Unit *>(a.out[o]);
        const u32 len = ne * n * t.KC;              // below 2^32 by SelTile::set
        for (u32 l = threadIdx.x; l < len; l += 256u) {
            const u32 en = csgn_fastdiv(l, t.dKC), kk = l - en * t.KC;
            const u32 el = csgn_fastdiv(en, dn), qi = en - el * n;
            if (kk >= kc)
                continue;
            const u32 k = k0 + kk;
            const u64 e = e0 + el;
            Unit v;
            if (Fresh) {
                const u32 cd = code[c0 + qi];
                v = subset_and(tab, a.tabs, el, cd & 0xFFFFu, t.KC, kk) & subset_and(tab2, a.tabs, el, cd >> 16, t.KC, kk);
            } else {
                v = one_unit(Unit(), k, t.U, t.last_mask);
                arith_entry<false>(a, o, i0 + qi, [&](u32 side, u32 j, u32 x) {
                    v &= side == 0u ? reinterpret_cast<const Unit *>(a.a[j])[(e * a.ta[j] + x) * t.U + k]
                                    : reinterpret_cast<const Unit *>(a.b[j])[(e * a.tb[j] + x) * t.U + k];
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

// The terms of every output (T[o], o <= w for ADD / SUB, o = 0 for EQ / NE) and of every carry (C[j] = C_j; ADD / SUB);
// a count of 2^62 or more is kTermLimit.  false for a bad op or width, a null pointer or a plane of no terms or of 2^62
// or more.
bool arith_counts(int op, u64 w, const u64 *ta, const u64 *tb, u64 *T, u64 *C)
{
    if (op < CSGN_UINT_ARITH_ADD || op > CSGN_UINT_ARITH_NE || w < 1 || w > kArithMaxWidth || !ta || !tb)
        return false;
    for (u64 j = 0; j < w; ++j)
        if (ta[j] == 0 || tb[j] == 0 || ta[j] >= kTermLimit || tb[j] >= kTermLimit)
            return false;
    if (op >= CSGN_UINT_ARITH_EQ) {
        u64 e = 1;
        for (u64 j = 0; j < w; ++j)
            e = sat_mul(e, sat_add(sat_add(ta[j], tb[j]), 1));
        T[0] = op == CSGN_UINT_ARITH_NE ? sat_add(e, 1) : e;
        C[0] = e;
        return true;
    }
    const u64 one = op == CSGN_UINT_ARITH_SUB ? 1 : 0;
    u64 c = one;
    for (u64 j = 0; j < w; ++j) {
        const u64 tn = tb[j] + one, ab = sat_add(ta[j], tn);
        T[j] = sat_add(ab, c);
        c = sat_add(sat_mul(ta[j], tn), sat_mul(ab, c));
        C[j] = c;
    }
    T[w] = c;
    return true;
}

u32 arith_outputs(int op, u64 w, bool carry)
{
    return op >= CSGN_UINT_ARITH_EQ ? 1u : (u32)w + (carry ? 1u : 0u);
}

// every requested output below kTermLimit
bool arith_shape_ok(int op, u64 w, const u64 *ta, const u64 *tb, bool carry)
{
    u64 T[kMaxOut], C[kArithMaxWidth];
    if (!arith_counts(op, w, ta, tb, T, C) || (carry && op >= CSGN_UINT_ARITH_EQ))
        return false;
    for (u32 o = 0; o < arith_outputs(op, w, carry); ++o)
        if (T[o] >= kTermLimit)
            return false;
    return true;
}

// Per shape (measured): the one launch.
bool arith_use_fused()
{
    return tune_choose(TUNE_UINT_ARITH_FORM, true);
}

template <typename Unit>
hipError_t arith_fused(u64 n_bits, int op, u64 batch, u64 w, const u64 *const *pa, const u64 *ta, const u64 *const *pb,
                       const u64 *tb, u64 *const *out, u64 *carry, const u64 *T, const u64 *C, u32 U, hipStream_t st)
{
    ArithArgs a = {};
    const bool eq = op >= CSGN_UINT_ARITH_EQ;
    const u64 one = op == CSGN_UINT_ARITH_SUB ? 1 : 0;
    a.op = (u32)op;
    a.w = (u32)w;
    a.nout = arith_outputs(op, w, carry != nullptr);
    a.eq = eq ? (u32)C[0] : 0u;
    bool fresh = true;
    for (u32 j = 0; j < w; ++j) {
        a.ta[j] = (u32)ta[j];
        a.tb[j] = (u32)tb[j];
        a.tn.set(j, (u32)(tb[j] + one));
        // the walk reads P_j and C_{j-1} only on the way down from an output that is written: both are below its terms
        const bool read = !eq && j + 1 < a.nout;
        a.P[j] = read ? (u32)(ta[j] * (tb[j] + one)) : 0u;
        a.C.set(j, read && j ? (u32)C[j - 1] : 1u);
        fresh = fresh && ta[j] == 1 && tb[j] == 1;
    }
    u64 total = 0;
    for (u32 o = 0; o < a.nout; ++o) {
        a.T.set(o, (u32)T[o]);
        a.start[o] = total;
        total += T[o];
    }
    a.start[a.nout] = total;
    // The tables of few planes are cut further until both sets hold no more entries than half the terms an element
    // writes: a sum of four bits writes 34 terms, and two tables of 16 entries would cost as much as the outputs do.
    SubsetPlan sp = subset_plan(fresh ? (u32)w : 0, U, (u32)sizeof(Unit), kTableBudget);
    for (u32 tables = 2; fresh && tables <= kMaxSubsetTables && 4 * sp.entries > total; ++tables)
        sp = subset_plan((u32)w, U, (u32)sizeof(Unit), kTableBudget, tables);
    // The range of entries a workgroup takes: the shortest with which one element gives it part_units to write and four
    // times what its two table sets cost to build, no more than the LDS list holds -- then elements until it has as
    // much.  Planes of several terms have no list: their range grows where the parts would pass a launch's workgroups.
    // A call of few units is cut finer, down to kMinPartUnits a workgroup, so that it still has kFillBlocks of them: a
    // megabyte of outputs in a dozen workgroups took longer than the chain's launches.
    const u64 fill = std::min<u64>(kPartUnits, std::max<u64>(kMinPartUnits, batch * total * U / kFillBlocks));
    const u64 part_units = std::max<u64>(fill, 8 * sp.entries * sp.KC);
    u64 want_QP = std::min<u64>({(part_units + sp.KC - 1) / sp.KC, (u64)kMaxRange, total});
    if (!fresh)
        want_QP = std::max<u64>(want_QP, (total * sp.chunks + kMaxBlocks256 - 1) / kMaxBlocks256);
    const u64 qparts = (total + want_QP - 1) / want_QP;
    const u64 QP = (total + qparts - 1) / qparts;
    const u64 capG = std::min<u64>({sp.max_G, batch, kMaxTile});
    u64 G = 1;
    while (G * QP * sp.KC < part_units && 2 * G <= capG)
        G *= 2;
    SelOutputs<1> stream = {};                      // the tile's view: one stream of one term per entry
    stream.fill(0, [](u32) { return 0; }, true, sp.KC);
    a.tile.set(n_bits, U, sp, QP, total, stream, G);
    const u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.tabs, a.tile.G, &a.tabs) : 0u;    // one layout, both sets
    a.tile.xcd = stream_xcd(batch * total * U);
    return sel_launch(k_uint_arith<Unit, true>, k_uint_arith<Unit, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        for (u32 j = 0; j < w; ++j) {
            a.a[j] = reinterpret_cast<const Unit *>(pa[j]) + e0 * ta[j] * U;
            a.b[j] = reinterpret_cast<const Unit *>(pb[j]) + e0 * tb[j] * U;
        }
        for (u32 o = 0; o < a.nout; ++o)
            a.out[o] = reinterpret_cast<Unit *>(eq || o < w ? out[o] : carry) + e0 * T[o] * U;
    });
}

// The composed form, the chain the classes began with: ADD_HALF / ADD_FULL (SUB: csgn_gate_uniform's NOT of b_j and a
// first carry of ONE) or the XNOR gate and the EQ_STEPs (NE: a closing NOT) through csgn_uint_step's and
// csgn_gate_uniform's launchers.  The running value takes turns between two temporaries; they and the NOT of a plane
// live in one block (scratch_take, csgn_kernels.h).
hipError_t arith_composed(u64 n_bits, int op, u64 batch, u64 w, const u64 *const *pa, const u64 *ta,
                          const u64 *const *pb, const u64 *tb, u64 *const *out, u64 *carry, const u64 *C, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64;
    const bool eq = op >= CSGN_UINT_ARITH_EQ, sub = op == CSGN_UINT_ARITH_SUB, ne = op == CSGN_UINT_ARITH_NE;
    // value j (the carry c_j, or EQ over planes 0..j) lives in run[j & 1] unless it is the call's output; SUB's first
    // carry, ONE, is value -1
    u64 E[kArithMaxWidth], size[2] = {0, sub ? 1u : 0u}, tnot = 0;
    for (u64 j = 0, e = 1; j < w; ++j) {
        e *= ta[j] + tb[j] + 1;
        E[j] = eq ? e : C[j];
        if (j + 1 < w || ne)
            size[j & 1] = std::max(size[j & 1], E[j]);
        if (sub)
            tnot = std::max(tnot, tb[j] + 1);
    }
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_UINT_ARITH, batch * std::max<u64>(1, size[0] + size[1] + tnot) * dL * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *run[2] = {block, block + batch * size[0] * dL}, *nb = run[1] + batch * size[1] * dL;
    if (eq) {
        for (u64 j = 0; j < w && e == hipSuccess; ++j) {
            u64 *dst = j + 1 < w || ne ? run[j & 1] : out[0];
            e = j == 0 ? gate_uniform(n_bits, CSGN_GATE_XNOR, batch, 0, ta[0], tb[0], nullptr, pa[0], pb[0], nullptr, dst, st)
                       : uint_step(n_bits, CSGN_UINT_EQ_STEP, batch, run[(j - 1) & 1], E[j - 1], pa[j], ta[j], pb[j],
                                   tb[j], dst, nullptr, st);
        }
        if (ne && e == hipSuccess)
            e = gate_uniform(n_bits, CSGN_GATE_NOT, batch, 0, E[w - 1], 0, nullptr, run[(w - 1) & 1], nullptr, nullptr,
                             out[0], st);
        return scratch_done(block, owned, e);
    }
    if (sub)
        e = const_fill(n_bits, batch, nullptr, 1, run[1], 0, st);
    for (u64 j = 0; j < w && e == hipSuccess; ++j) {
        const u64 *B = pb[j];
        if (sub) {
            e = gate_uniform(n_bits, CSGN_GATE_NOT, batch, 0, tb[j], 0, nullptr, pb[j], nullptr, nullptr, nb, st);
            B = nb;
        }
        const bool half = !sub && j == 0;
        if (e == hipSuccess)
            e = uint_step(n_bits, half ? CSGN_UINT_ADD_HALF : CSGN_UINT_ADD_FULL, batch, half ? nullptr : run[(j + 1) & 1],
                          half ? 0 : j ? C[j - 1] : 1, pa[j], ta[j], B, tb[j] + (sub ? 1 : 0), out[j],
                          j + 1 < w ? run[j & 1] : carry, st);
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_arith_terms(int op, u64 w, const u64 *ta, const u64 *tb, u64 output)
{
    u64 T[kMaxOut], C[kArithMaxWidth];
    if (!arith_counts(op, w, ta, tb, T, C) || output > (op >= CSGN_UINT_ARITH_EQ ? 0 : w))
        return 0;
    return T[output] >= kTermLimit ? 0 : T[output];
}

const char *uint_arith_kernel_name(u64 n_bits, int op, u64 batch, u64 w, const u64 *ta, const u64 *tb, bool carry)
{
    (void)batch;
    if (n_bits == 0 || !arith_shape_ok(op, w, ta, tb, carry))
        return "";
    return arith_use_fused() ? "k_uint_arith" : "composed";
}

hipError_t uint_arith(u64 n_bits, int op, u64 batch, u64 w, const u64 *const *a, const u64 *ta, const u64 *const *b,
                      const u64 *tb, u64 *const *out, u64 *carry, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    u64 T[kMaxOut], C[kArithMaxWidth];
    if (!arith_shape_ok(op, w, ta, tb, carry != nullptr))
        return hipErrorInvalidValue;
    arith_counts(op, w, ta, tb, T, C);
    if (!arith_use_fused())
        return arith_composed(n_bits, op, batch, w, a, ta, b, tb, out, carry, C, stream);
    const u64 dL = (n_bits + 63) / 64;
    const u64 nplanes = op >= CSGN_UINT_ARITH_EQ ? 1 : w;
    const bool wide = wide_units(dL, ptr_array(a, w), ptr_array(b, w), ptr_array(out, nplanes), carry);
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? arith_fused<unit16>(n_bits, op, batch, w, a, ta, b, tb, out, carry, T, C, U, stream)
                : arith_fused<unit8>(n_bits, op, batch, w, a, ta, b, tb, out, carry, T, C, U, stream);
}

} // namespace csgn
