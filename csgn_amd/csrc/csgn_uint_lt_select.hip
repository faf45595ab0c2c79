// csgn_uint_lt_select.hip -- selection by an ENCRYPTED comparison: every plane of min, max and both payloads of a
// compare-exchange, and the comparison itself, in one launch.  Hand-written CDNA4 (gfx950) HIP; the kernel skeleton in
// csgn_selector.h, design notes in DESIGN.md §4.22.
//
// The definition (include/csgn_hip.h, csgn_uint_lt_select) is out_i = (L * (X_i + Y_i)) + Y_i with L = lessThan(a, b),
// l_0 = (a_0 + ONE) * b_0 and l_j = ((a_j + b_j) * (b_j + l_{j-1})) + l_{j-1}: the comparison is the LEFT operand of
// every product, so term q * (tx_i + ty_i) + c of output i is (term q of L) & (term c of X_i | Y_i), and the last ty_i
// terms are Y_i's.  Term q of L is decoded from q alone, plane w - 1 first: past (ta_j + tb_j) * (tb_j + L_{j-1}) it
// lies in the tail copy of l_{j-1} (no factor of plane j); else q / (tb_j + L_{j-1}) names a term of a_j or b_j and the
// remainder a term of b_j (which ends the walk) or of l_{j-1}.
//
// Fresh planes (every ta_j = tb_j = 1), the case this kernel is built for: term q is Pa_e[Sa] & Pb_e[Sb], the ANDs of
// subsets of the element's a planes and b planes.  A workgroup owns G elements, a slice of KC units of every term and
// one range of q, for EVERY output and for the comparison: it decodes its range once into an LDS list (Sa | Sb << 16)
// and builds the subset tables of §4.15 (csgn_device.h) twice, for its elements' a planes and their b planes.  A
// written unit is then 2-6 LDS reads ANDed with one unit of X_i or Y_i.  Multi-term a or b planes take the decode per
// unit straight from the planes (correct, not fast); multi-term X and Y stay on the fast path.
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kTableBudget = 20480;     // bytes of subset tables per workgroup, each of the two sets (48 KB with the list)
constexpr u32 kMaxRange = 2048;         // entries of q one workgroup decodes (8 KB of LDS)
constexpr u64 kPartUnits = 8192;        // units a workgroup writes at least, where the shape has them
constexpr u64 kOutUnits = 2048;         // ... and of every output (8 units a lane)
constexpr u32 kMaxTile = 64;            // elements of a workgroup at most

// By value in the kernel arguments (uniform, scalar loads).  The stream is L; output i has the tx_i + ty_i terms of
// X_i | Y_i.  Output nsel, when there is one, is the comparison itself (one term per entry, no value factor, no tail).
struct LtSelArgs {
    SelTile tile;
    SelOutputs<kLtSelMaxOut + 1> outs;
    const void *a[kLtSelMaxWidth];
    const void *b[kLtSelMaxWidth];
    const void *x[kLtSelMaxOut];
    const void *y[kLtSelMaxOut];
    u32 tx[kLtSelMaxOut + 1];                                           // terms of X_i
    u32 ta[kLtSelMaxWidth], tb[kLtSelMaxWidth];
    FastDivTable<kLtSelMaxWidth> inner;                                 // tb_j + L_{j-1}; tb_0 at j = 0
    u32 L, w, nsel;
    SubsetTables tabs;          // the a tables of G elements; the b tables, the tile's second set, have the same layout
};
static_assert(sizeof(LtSelArgs) <= 4096, "the kernel arguments of k_uint_lt_select pass the 4 KiB limit");

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_lt_select(LtSelArgs a)
{
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit>(t, a.L);

    if (Fresh) {
        // the range of q: Sa in the low 16 bits, Sb in the high 16 (published by the tables' closing barrier); with
        // fresh planes inner_j = 3^j, so the term of (a_j + b_j) is a comparison
        for (u32 i = threadIdx.x; i < b.nq; i += 256u) {
            u32 q = b.q0 + i, Sa = 0, Sb = 0;
            bool done = false;
            for (u32 j = a.w - 1u; j > 0u && !done; --j) {
                const u32 in = a.inner.d[j];
                if (q >= 2u * in) {             // the tail copy of l_{j-1}
                    q -= 2u * in;
                    continue;
                }
                const u32 p = q >= in ? 1u : 0u;
                q -= p * in;
                Sa |= (p ^ 1u) << j;
                Sb |= p << j;
                if (q == 0u) {                  // b_j ends the walk
                    Sb |= 1u << j;
                    done = true;
                } else {
                    q -= 1u;
                }
            }
            if (!done) {                        // (a_0 + ONE) * b_0
                Sa |= q == 0u ? 1u : 0u;
                Sb |= 1u;
            }
            b.code[i] = Sa | (Sb << 16);
        }
        subset_build(b.tab, a.tabs, a.a, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc);
        subset_build(b.tab2, a.tabs, a.b, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc);
    }

    for (u32 i = 0; i < a.outs.nout; ++i) {
        const u32 ts = a.outs.t[i], txi = a.tx[i], tyi = ts - txi;
        const bool has_value = i < a.nsel;
        const u64 Ti = has_value ? (u64)a.L * ts + tyi : (u64)a.L;
        const Unit *X = reinterpret_cast<const Unit *>(has_value ? a.x[i] : nullptr);
        const Unit *Y = reinterpret_cast<const Unit *>(has_value ? a.y[i] : nullptr);
        sel_walk<Unit>(t, b, a.outs, i, b.ne, [&](u32 el, u32 qi, u32 c, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk, q = b.q0 + qi;
            const u64 e = b.e0 + el;
            if (Fresh) {
                const u32 cd = b.code[qi];
                v = subset_and(b.tab, a.tabs, el, cd & 0xFFFFu, t.KC, kk) &
                    subset_and(b.tab2, a.tabs, el, cd >> 16, t.KC, kk);
            } else {
                v = one_unit(Unit(), k, t.U, t.last_mask);
                u32 in = q;
                bool done = false;
                for (u32 j = a.w - 1u; j > 0u && !done; --j) {
                    const FastDiv di = a.inner.at(j);
                    const u32 taj = a.ta[j], tbj = a.tb[j], M = (taj + tbj) * di.d;
                    if (in >= M) {
                        in -= M;
                        continue;
                    }
                    const u32 p = csgn_fastdiv(in, di), cc = in - p * di.d;
                    const Unit *B = reinterpret_cast<const Unit *>(a.b[j]);
                    v &= p < taj ? reinterpret_cast<const Unit *>(a.a[j])[(e * taj + p) * t.U + k]
                                 : B[(e * tbj + (p - taj)) * t.U + k];
                    if (cc < tbj) {
                        v &= B[(e * tbj + cc) * t.U + k];
                        done = true;
                    } else {
                        in = cc - tbj;
                    }
                }
                if (!done) {
                    const FastDiv di = a.inner.at(0);
                    const u32 ta0 = a.ta[0], p = csgn_fastdiv(in, di), cc = in - p * di.d;
                    if (p < ta0)
                        v &= reinterpret_cast<const Unit *>(a.a[0])[(e * ta0 + p) * t.U + k];
                    v &= reinterpret_cast<const Unit *>(a.b[0])[(e * di.d + cc) * t.U + k];
                }
            }
            if (has_value)
                v &= c < txi ? X[(e * txi + c) * t.U + k] : Y[(e * tyi + (c - txi)) * t.U + k];
            at = (e * Ti + (u64)q * ts + c) * t.U + k;
            return true;
        });
        if (has_value && b.q0 == 0u) {              // the tail: Y_i's terms, copied
            Unit *o = reinterpret_cast<Unit *>(a.outs.out[i]);
            const u32 tail = b.ne * tyi * t.KC;
            for (u32 l = threadIdx.x; l < tail; l += 256u) {
                const u32 row = csgn_fastdiv(l, t.dKC), kk = l - row * t.KC;
                const u32 el = row / tyi, c = row - el * tyi;
                if (kk >= b.kc)
                    continue;
                const u64 e = b.e0 + el;
                const u32 k = b.k0 + kk;
                unit_store<Unit, true>(o + (e * Ti + (u64)a.L * ts + c) * t.U + k, Y[(e * tyi + c) * t.U + k]);
            }
        }
    }
}

// ------------------------------------------------------------------------------ host side

// L_j of every plane (Ls[j], j < w); false for a bad width, a null pointer, a plane of no terms or a count of 2^62 or more
bool lt_counts(u64 w, const u64 *ta, const u64 *tb, u64 *Ls)
{
    if (w < 1 || w > kLtSelMaxWidth || !ta || !tb)
        return false;
    for (u64 j = 0; j < w; ++j)
        if (ta[j] == 0 || tb[j] == 0 || ta[j] >= kTermLimit || tb[j] >= kTermLimit)
            return false;
    u64 L;
    if (!term_mul(ta[0] + 1, tb[0], L))
        return false;
    Ls[0] = L;
    for (u64 j = 1; j < w; ++j) {
        u64 M;
        if (!term_mul(ta[j] + tb[j], tb[j] + L, M) || M + L >= kTermLimit)
            return false;
        L = M + L;
        Ls[j] = L;
    }
    return true;
}

bool lt_select_shape_ok(u64 w, const u64 *ta, const u64 *tb, u64 n_out, const u64 *tx, const u64 *ty, bool less)
{
    u64 Ls[kLtSelMaxWidth];
    if (n_out > kLtSelMaxOut || (n_out == 0 && !less) || (n_out > 0 && (!tx || !ty)) || !lt_counts(w, ta, tb, Ls))
        return false;
    for (u64 i = 0; i < n_out; ++i)
        if (tx[i] == 0 || ty[i] == 0 || tx[i] >= kTermLimit || ty[i] >= kTermLimit)
            return false;
    return true;
}

// Per shape: the fused kernel.
bool lt_select_use_fused()
{
    return tune_choose(TUNE_UINT_LT_SELECT_FORM, true);
}

template <typename Unit>
hipError_t lt_select_fused(u64 n_bits, u64 batch, u64 w, const u64 *const *pa, const u64 *ta, const u64 *const *pb,
                           const u64 *tb, u64 n_out, const u64 *const *x, const u64 *tx, const u64 *const *y,
                           const u64 *ty, u64 *const *out, u64 *less, const u64 *Ls, u32 U, hipStream_t st)
{
    LtSelArgs a = {};
    const u64 L = Ls[w - 1];
    a.w = (u32)w;
    a.nsel = (u32)n_out;
    a.L = (u32)L;
    bool fresh = true;
    for (u32 j = 0; j < w; ++j) {
        a.ta[j] = (u32)ta[j];
        a.tb[j] = (u32)tb[j];
        a.inner.set(j, (u32)(tb[j] + (j ? Ls[j - 1] : 0)));
        fresh = fresh && ta[j] == 1 && tb[j] == 1;
    }
    const SubsetPlan sp = subset_plan(fresh ? (u32)w : 0, U, (u32)sizeof(Unit), kTableBudget);
    const u64 sumt = a.outs.fill(n_out, [&](u32 i) { return tx[i] + ty[i]; }, less != nullptr, sp.KC);
    for (u32 i = 0; i < n_out; ++i)
        a.tx[i] = (u32)tx[i];
    // The range of q a workgroup decodes: the shortest with which one element gives it kPartUnits to write, kOutUnits
    // per output (each output is a loop of its own, with its own scalar set-up) and four times what its two table sets
    // cost to build (both sets are per element, so that ratio does not depend on G) -- a batch of a few hundred
    // elements has no other source of workgroups -- then elements until it has as much.
    const u64 part_units = std::max<u64>({kPartUnits, kOutUnits * a.outs.nout, 8 * sp.entries * sp.KC});
    const u64 want_QP = std::min<u64>({(part_units + sumt * sp.KC - 1) / (sumt * sp.KC), (u64)kMaxRange, L});
    const u64 qparts = (L + want_QP - 1) / want_QP;
    const u64 QP = (L + qparts - 1) / qparts;
    const u64 capG = std::min<u64>({sp.max_G, batch, kMaxTile});
    const u64 cell = QP * sumt * sp.KC;             // units of one element of a workgroup
    u64 G = 1;
    while (G * cell < part_units && 2 * G <= capG)
        G *= 2;
    a.tile.set(n_bits, U, sp, QP, L, a.outs, G);
    const u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.tabs, a.tile.G, &a.tabs) : 0u;    // one layout, both sets
    a.tile.xcd = stream_xcd(batch * (L * sumt) * U);
    return sel_launch(k_uint_lt_select<Unit, true>, k_uint_lt_select<Unit, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        for (u32 j = 0; j < w; ++j) {
            a.a[j] = reinterpret_cast<const Unit *>(pa[j]) + e0 * ta[j] * U;
            a.b[j] = reinterpret_cast<const Unit *>(pb[j]) + e0 * tb[j] * U;
        }
        for (u32 i = 0; i < a.outs.nout; ++i) {
            if (i < n_out) {                        // the comparison, output n_out, has no value planes
                a.x[i] = reinterpret_cast<const Unit *>(x[i]) + e0 * tx[i] * U;
                a.y[i] = reinterpret_cast<const Unit *>(y[i]) + e0 * ty[i] * U;
                a.outs.out[i] = reinterpret_cast<Unit *>(out[i]) + e0 * (L * a.outs.t[i] + ty[i]) * U;
            } else {
                a.outs.out[i] = reinterpret_cast<Unit *>(less) + e0 * L * U;
            }
        }
    });
}

// The composed form, what select(lessThan(a, b), x, y) issues: LT_FIRST and one LT_STEP per further plane through
// csgn_uint_step's launcher into two temporaries that take turns so that the last lands in the first, then
// csgn_gate_uniform's MUX launcher per output and a copy of the comparison into `less`.  The temporaries live in one
// block (scratch_take, csgn_kernels.h).
hipError_t lt_select_composed(u64 n_bits, u64 batch, u64 w, const u64 *const *pa, const u64 *ta, const u64 *const *pb,
                              const u64 *tb, u64 n_out, const u64 *const *x, const u64 *tx, const u64 *const *y,
                              const u64 *ty, u64 *const *out, u64 *less, const u64 *Ls, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64, L = Ls[w - 1], before_last = w > 1 ? Ls[w - 2] : 0;
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_UINT_LT_SELECT, batch * (L + before_last) * dL * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *lt[2] = {block, block + batch * L * dL};
    u32 cur = (u32)((w - 1) & 1u);                  // plane w - 1 writes lt[0]
    e = uint_step(n_bits, CSGN_UINT_LT_FIRST, batch, nullptr, 0, pa[0], ta[0], pb[0], tb[0], lt[cur], nullptr, st);
    for (u64 j = 1; j < w && e == hipSuccess; ++j) {
        e = uint_step(n_bits, CSGN_UINT_LT_STEP, batch, lt[cur], Ls[j - 1], pa[j], ta[j], pb[j], tb[j], lt[cur ^ 1u],
                      nullptr, st);
        cur ^= 1u;
    }
    for (u64 i = 0; i < n_out && e == hipSuccess; ++i)
        e = gate_uniform(n_bits, CSGN_GATE_MUX, batch, L, tx[i], ty[i], lt[0], x[i], y[i], nullptr, out[i], st);
    if (less && e == hipSuccess)
        e = add_uniform(n_bits, batch, L, 0, lt[0], nullptr, less, st, L * dL);
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_lt_terms(u64 w, const u64 *ta, const u64 *tb)
{
    u64 Ls[kLtSelMaxWidth];
    return lt_counts(w, ta, tb, Ls) ? Ls[w - 1] : 0;
}

const char *uint_lt_select_kernel_name(u64 n_bits, u64 batch, u64 w, const u64 *ta, const u64 *tb, u64 n_out,
                                       const u64 *tx, const u64 *ty, bool less)
{
    (void)batch;
    if (n_bits == 0 || !lt_select_shape_ok(w, ta, tb, n_out, tx, ty, less))
        return "";
    return lt_select_use_fused() ? "k_uint_lt_select" : "composed";
}

hipError_t uint_lt_select(u64 n_bits, u64 batch, u64 w, const u64 *const *a, const u64 *ta, const u64 *const *b,
                          const u64 *tb, u64 n_out, const u64 *const *x, const u64 *tx, const u64 *const *y,
                          const u64 *ty, u64 *const *out, u64 *less, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    u64 Ls[kLtSelMaxWidth];
    if (!lt_counts(w, ta, tb, Ls))
        return hipErrorInvalidValue;
    if (!lt_select_use_fused())
        return lt_select_composed(n_bits, batch, w, a, ta, b, tb, n_out, x, tx, y, ty, out, less, Ls, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(a, w), ptr_array(b, w), ptr_array(x, n_out), ptr_array(y, n_out),
                                 ptr_array(out, n_out), less);
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? lt_select_fused<unit16>(n_bits, batch, w, a, ta, b, tb, n_out, x, tx, y, ty, out, less, Ls, U, stream)
                : lt_select_fused<unit8>(n_bits, batch, w, a, ta, b, tb, n_out, x, tx, y, ty, out, less, Ls, U, stream);
}

} // namespace csgn
