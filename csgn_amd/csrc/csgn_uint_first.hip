// csgn_uint_first.hip -- the FIRST row of a group whose ENCRYPTED mask bit is set: its value planes, the OR of the mask
// and the planes of its public label, every output in one launch.  Hand-written CDNA4 (gfx950) HIP; the kernel skeleton
// in csgn_selector.h, design notes in DESIGN.md §4.32.
//
// The definition (include/csgn_hip.h, csgn_uint_first): n_r = m_r + ONE, F_r = (((n_0 * n_1) * ...) * n_{r-1}) * m_r,
// out_j = sum over r < g, ascending, of F_r * d_{r,j}, any = sum of F_r, lab_i = sum of the F_r whose label has bit i.
// With H_r = prod over i < r of (s_i + 1), row r's block of the F stream has P_r = s_r * H_r entries and starts at entry
// H_r - 1, so the stream has Q = H_g - 1 entries and the row of entry q is the largest r with H_r <= q + 1.  Inside the
// block the digit of m_r (base s_r) is the fastest, then those of n_{r-1} .. n_0 (base s_i + 1); digit s_i of an n_i
// selects ONE.  Term q * t_j + c of out_j is (entry q) & (term c of d_{r,j}); any is the bare stream; lab_i is the bare
// stream without the blocks of the rows whose label lacks bit i, so entry q of a kept row r lands at q minus the entries
// of the skipped rows below r.
//
// Fresh masks (every s_r = 1) of up to 16 rows, the case this kernel is built for: H_r = 2^r, the row of q is the top
// bit of q + 1, and entry (r, in) is the AND of m_r and of the m_i, i < r, whose binary digit is 0 -- a subset of the g
// rows.  A workgroup owns G elements, a slice of KC units of every term and QP entries, for EVERY output: it builds the
// subset tables of §4.15 (csgn_device.h) over its elements' rows and decodes its entries once into an LDS list (subset
// in the low 16 bits, row in the high 16); a written unit is then 1-3 LDS reads ANDed with one unit of the value row.
// Larger groups and multi-term masks take the digits per unit straight from the rows (correct, not fast).  The row
// starts H, the rows' term counts and one label plane's skips at a time live in 816 B of static LDS, built by the
// workgroup: nothing is read from a device table.
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kFirstMaxFresh = 16;      // rows the subset tables and the 16-bit subsets of the LDS list hold

// By value in the kernel arguments (uniform, scalar loads).  The stream is the F stream of the first R rows (R = g, or,
// with label planes only, the rows up to the last one a requested plane keeps); outputs [0, w) are the value planes,
// output w, where outs has it, is any.  The label planes are bare outputs of their own.
struct FirstArgs {
    SelTile tile;
    SelOutputs<kFirstMaxPlanes + 1> outs;
    const void *mask[kFirstMaxGroup];   // term 0 of row r of the launch's first element
    const void *values[kFirstMaxPlanes];
    void *lab[kFirstMaxLabels];
    u64 keep[kFirstMaxLabels];          // label plane i keeps row r: bit r
    u32 s[kFirstMaxGroup];
    u32 Q;                              // entries of rows [0, R)
    u32 g, R, w, nlab;
    u32 gm;                             // an element's rows lie gm * s_r terms apart: g in the grouped layout, else 1
    SubsetTables tabs;
};
static_assert(sizeof(FirstArgs) <= 4096, "the kernel arguments of k_uint_first pass the 4 KiB limit");

// The row of entry q, and the entry inside the row's block.  Fresh: from the LDS list; else by bisection of the starts.
template <typename Unit, bool Fresh>
__device__ __forceinline__ u32 first_row(const FirstArgs &a, const SelBlock<Unit> &b, const u32 *H, u32 qi, u32 q, u32 &in)
{
    if (Fresh)
        return b.code[qi] >> 16;
    u32 lo = 0, hi = a.R;               // H[lo] <= q + 1 < H[hi]
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (H[mid] <= q + 1u)
            lo = mid;
        else
            hi = mid;
    }
    in = q + 1u - H[lo];
    return lo;
}

// Entry (r, in) at unit k = b.k0 + kk of element e = b.e0 + el
template <typename Unit, bool Fresh>
__device__ __forceinline__ Unit first_entry(const FirstArgs &a, const SelTile &t, const SelBlock<Unit> &b, const u32 *S,
                                            u32 el, u64 e, u32 qi, u32 r, u32 in, u32 k, u32 kk)
{
    if (Fresh)
        return subset_and(b.tab, a.tabs, el, b.code[qi] & 0xFFFFu, t.KC, kk);
    const u64 eg = e * a.gm;
    const u32 sr = S[r], nx = in / sr;
    Unit v = reinterpret_cast<const Unit *>(a.mask[r])[(eg * sr + (in - nx * sr)) * t.U + k];
    in = nx;
    for (u32 i = r; i-- > 0u;) {
        const u32 si = S[i], ny = in / (si + 1u), dg = in - ny * (si + 1u);
        in = ny;
        if (dg < si)
            v &= reinterpret_cast<const Unit *>(a.mask[i])[(eg * si + dg) * t.U + k];
    }
    return v;
}

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_first(FirstArgs a)
{
    // One static array of a multiple of 16 bytes, so that the dynamic LDS behind it (the tables' 16-byte units) stays
    // aligned.  H[r] = prod over i < r of (s_i + 1): row r starts at entry H[r] - 1; S[r] = s_r, for the lanes that index
    // it by their own row; skip[r], of one label plane at a time: the entries of the rows below r that it leaves out.
    __shared__ __align__(16) u32 rowtab[3][kFirstMaxGroup + 4];
    u32 *const H = rowtab[0], *const S = rowtab[1], *const skip = rowtab[2];
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit>(t, a.Q);

    if (threadIdx.x == 0) {
        u32 h = 1;
        for (u32 r = 0; r < a.R; ++r) {
            H[r] = h;
            S[r] = a.s[r];
            h *= a.s[r] + 1u;                   // H[R] = Q + 1 < 2^32
        }
        H[a.R] = h;
    }
    if (Fresh) {
        // the range of q: the subset in the low 16 bits, the row in the high 16 (published by the tables' closing barrier)
        for (u32 i = threadIdx.x; i < b.nq; i += 256u) {
            const u32 q1 = b.q0 + i + 1u, r = 31u - (u32)__clz((int)q1), in = q1 - (1u << r);
            u32 sub = 1u << r;
            for (u32 x = 0; x < r; ++x)         // n_0 is the slowest digit; digit 0 = m_x, 1 = ONE
                if (!((in >> (r - 1u - x)) & 1u))
                    sub |= 1u << x;
            b.code[i] = sub | (r << 16);
        }
        subset_build(b.tab, a.tabs, a.mask, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc, a.gm * t.U);
    } else {
        __syncthreads();
    }

    for (u32 j = 0; j < a.outs.nout; ++j) {
        const u32 tj = a.outs.t[j];
        const u64 Tj = (u64)tj * a.Q;
        const bool has_value = j < a.w;
        const Unit *d = reinterpret_cast<const Unit *>(has_value ? a.values[j] : nullptr);
        sel_walk<Unit>(t, b, a.outs, j, b.ne, [&](u32 el, u32 qi, u32 c, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk, q = b.q0 + qi;
            const u64 e = b.e0 + el;
            u32 in = 0;
            const u32 r = first_row<Unit, Fresh>(a, b, H, qi, q, in);
            v = first_entry<Unit, Fresh>(a, t, b, S, el, e, qi, r, in, k, kk);
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
        if (threadIdx.x <= a.R) {
            u32 sk = 0;
            for (u32 x = 0; x < threadIdx.x; ++x)
                if (!((keep >> x) & 1u))
                    sk += S[x] * H[x];
            skip[threadIdx.x] = sk;
        }
        __syncthreads();
        const u64 Ti = a.Q - skip[a.R];
        lo.out[0] = a.lab[i];
        sel_walk<Unit>(t, b, lo, 0u, b.ne, [&](u32 el, u32 qi, u32, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk, q = b.q0 + qi;
            const u64 e = b.e0 + el;
            u32 in = 0;
            const u32 r = first_row<Unit, Fresh>(a, b, H, qi, q, in);
            if (!((keep >> r) & 1u))
                return false;
            v = first_entry<Unit, Fresh>(a, t, b, S, el, e, qi, r, in, k, kk);
            at = (e * Ti + (q - skip[r])) * t.U + k;
            return true;
        });
    }
}

// ------------------------------------------------------------------------------ host side

// H_r = prod over i < r of (s_i + 1) for r <= rows; false for a row of no terms or a product of 2^62 or more
bool first_starts(const u64 *s, u64 rows, u64 *H)
{
    H[0] = 1;
    for (u64 r = 0; r < rows; ++r)
        if (s[r] == 0 || s[r] >= kTermLimit || !term_mul(H[r], s[r] + 1, H[r + 1]))
            return false;
    return true;
}

template <typename Unit>
hipError_t first_launch(u64 n_bits, u64 batch, u64 g, const u64 *const *mask, u64 n_mask, const u64 *s, u64 w,
                        const u64 *const *values, const u64 *tv, u64 *const *out, u64 *any, u64 nlab, const u64 *keep,
                        const u64 *Tlab, u64 *const *label_out, u64 R, u64 Q, u32 U, hipStream_t st)
{
    FirstArgs a = {};
    a.g = (u32)g;
    a.R = (u32)R;
    a.w = (u32)w;
    a.nlab = (u32)nlab;
    a.Q = (u32)Q;
    a.gm = n_mask == 1 ? (u32)g : 1u;
    bool fresh = R <= kFirstMaxFresh;
    for (u32 r = 0; r < R; ++r) {
        a.s[r] = (u32)s[r];
        fresh = fresh && s[r] == 1;
    }
    const SubsetPlan sp = ReadTile::plan(fresh, R, U, (u32)sizeof(Unit));
    u64 sumt = a.outs.fill(w, [&](u32 j) { return tv[j]; }, any != nullptr, sp.KC);
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
    return sel_launch(k_uint_first<Unit, true>, k_uint_first<Unit, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        for (u32 r = 0; r < R; ++r)
            a.mask[r] = reinterpret_cast<const Unit *>(n_mask == 1 ? mask[0] : mask[r]) +
                        (e0 * a.gm + (n_mask == 1 ? r : 0u)) * s[r] * U;
        for (u32 j = 0; j < nout; ++j) {
            if (j < w)                          // any, output w, has no value plane
                a.values[j] = reinterpret_cast<const Unit *>(values[j]) + e0 * g * tv[j] * U;
            a.outs.out[j] = reinterpret_cast<Unit *>(j < w ? out[j] : any) + e0 * Q * a.outs.t[j] * U;
        }
        for (u32 i = 0; i < nlab; ++i)
            a.lab[i] = reinterpret_cast<Unit *>(label_out[i]) + e0 * Tlab[i] * U;
    });
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_first_terms(u64 g, const u64 *s, u64 row)
{
    if (g < 1 || g > kFirstMaxGroup || !s || row > g)
        return 0;
    for (u64 r = 0; r < g; ++r)
        if (s[r] == 0 || s[r] >= kTermLimit)
            return 0;
    // Q = H_g - 1 may stay below 2^62 where H_g does not: the last factor apart
    const u64 rows = row == g ? g - 1 : row;
    u64 H[kFirstMaxGroup + 1];
    unsigned long long T;
    if (!first_starts(s, rows, H) ||
        __builtin_mul_overflow((unsigned long long)H[rows], (unsigned long long)(s[rows] + (row == g ? 1 : 0)), &T))
        return 0;
    T -= row == g ? 1 : 0;
    return T < kTermLimit ? T : 0;
}

u64 uint_first_label_terms(u64 g, const u64 *s, const u64 *labels, u64 bit)
{
    if (g < 1 || g > kFirstMaxGroup || !s || !labels || bit > 63)
        return 0;
    u64 T = 0;
    for (u64 r = 0; r < g; ++r) {
        if (s[r] == 0 || s[r] >= kTermLimit)
            return 0;
        if (!((labels[r] >> bit) & 1u))
            continue;
        const u64 P = uint_first_terms(g, s, r);
        if (P == 0 || (T += P) >= kTermLimit)
            return 0;
    }
    return T;
}

hipError_t uint_first(u64 n_bits, u64 batch, u64 g, const u64 *const *mask, u64 n_mask, const u64 *s, u64 w,
                      const u64 *const *values, const u64 *t, u64 *const *out, u64 *any, u64 n_labels,
                      const u64 *labels, const u64 *label_bits, u64 *const *label_out, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    // the rows the stream holds: all of them, or, with label planes only, those up to the last row a plane keeps
    u64 keep[kFirstMaxLabels], Tlab[kFirstMaxLabels], R = w || any ? g : 0;
    for (u64 i = 0; i < n_labels; ++i) {
        keep[i] = 0;
        for (u64 r = 0; r < g; ++r)
            if ((labels[r] >> label_bits[i]) & 1u) {
                keep[i] |= 1ull << r;
                R = std::max(R, r + 1);
            }
        Tlab[i] = uint_first_label_terms(g, s, labels, label_bits[i]);
    }
    const u64 Q = uint_first_terms(R, s, R);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(mask, n_mask), ptr_array(values, w), ptr_array(out, w), any,
                                 ptr_array(label_out, n_labels));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? first_launch<unit16>(n_bits, batch, g, mask, n_mask, s, w, values, t, out, any, n_labels, keep, Tlab,
                                       label_out, R, Q, U, stream)
                : first_launch<unit8>(n_bits, batch, g, mask, n_mask, s, w, values, t, out, any, n_labels, keep, Tlab,
                                      label_out, R, Q, U, stream);
}

} // namespace csgn
