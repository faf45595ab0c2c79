// csgn_uint_lt_select.hip -- selection by an ENCRYPTED comparison: every plane of min, max and both payloads of a
// compare-exchange, and the comparison itself, in one launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in
// csgn_device.h, design notes in DESIGN.md §4.22.
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
// written unit is then 2-6 LDS reads ANDed with one unit of X_i or Y_i.  Lanes walk one output's stream with the unit
// fastest, then the value term, q and the element, so one store instruction writes 64 consecutive units of one plane.
// Multi-term a or b planes take the decode per unit straight from the planes (correct, not fast); multi-term X and Y
// stay on the fast path.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kTableBudget = 20480;     // bytes of subset tables per workgroup, each of the two sets (48 KB with the list)
constexpr u32 kMaxRange = 2048;         // entries of q one workgroup decodes (8 KB of LDS)
constexpr u64 kPartUnits = 8192;        // units a workgroup writes at least, where the shape has them
constexpr u64 kOutUnits = 2048;         // ... and of every output (8 units a lane)
constexpr u32 kMaxTile = 64;            // elements of a workgroup at most

// By value in the kernel arguments (uniform, scalar loads).  A workgroup is (element group, unit chunk, q part):
// elements [group * G, + G), units [chunk * KC, + KC) of every term and entries [qpart * QP, + QP) of L.  Output nsel,
// when there is one, is the comparison itself (one term per entry, no value factor, no tail).
struct LtSelArgs {
    const void *a[kLtSelMaxWidth];
    const void *b[kLtSelMaxWidth];
    const void *x[kLtSelMaxOut];
    const void *y[kLtSelMaxOut];
    void *out[kLtSelMaxOut + 1];
    u32 tx[kLtSelMaxOut + 1];                                           // terms of X_i
    u32 ts[kLtSelMaxOut + 1];                                           // tx_i + ty_i; 1 for the comparison
    FastDivTable<kLtSelMaxOut + 1> tk;                                  // ts_i * KC
    u32 ta[kLtSelMaxWidth], tb[kLtSelMaxWidth];
    FastDivTable<kLtSelMaxWidth> inner;                                 // tb_j + L_{j-1}; tb_0 at j = 0
    u64 last_mask;
    u64 batch;                  // elements of this launch
    u32 L, w, nsel, nout;       // nout = nsel + (the comparison is written)
    u32 U, KC, G, QP, chunks, qparts, nblocks, xcd;
    SubsetTables tabs;          // the a tables of G elements; the b tables have the same layout
    u32 bbase, lbase;           // byte offsets of the b tables and of the decoded range in the LDS
    FastDiv dKC, dQP;
};
static_assert(sizeof(LtSelArgs) <= 4096, "the kernel arguments of k_uint_lt_select pass the 4 KiB limit");

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_lt_select(LtSelArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Unit *taba = reinterpret_cast<Unit *>(smem_raw);
    Unit *tabb = reinterpret_cast<Unit *>(smem_raw + a.bbase);
    u32 *code = reinterpret_cast<u32 *>(smem_raw + a.lbase);
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, a.nblocks) : blockIdx.x;
    const u32 gc = bid / a.qparts, qpart = bid - gc * a.qparts;
    const u32 group = gc / a.chunks, chunk = gc - group * a.chunks;
    const u64 e0 = (u64)group * a.G;
    const u32 ne = (u32)min((u64)a.G, a.batch - e0);
    const u32 k0 = chunk * a.KC, kc = min(a.KC, a.U - k0);
    const u32 q0 = qpart * a.QP, nq = q0 < a.L ? min(a.QP, a.L - q0) : 0u;

    if (Fresh) {
        // the range of q: Sa in the low 16 bits, Sb in the high 16 (published by the tables' closing barrier); with
        // fresh planes inner_j = 3^j, so the term of (a_j + b_j) is a comparison
        for (u32 i = threadIdx.x; i < nq; i += 256u) {
            u32 q = q0 + i, Sa = 0, Sb = 0;
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
            code[i] = Sa | (Sb << 16);
        }
        subset_build(taba, a.tabs, a.a, a.G, a.KC, a.dKC, a.U, a.last_mask, e0, ne, k0, kc);
        subset_build(tabb, a.tabs, a.b, a.G, a.KC, a.dKC, a.U, a.last_mask, e0, ne, k0, kc);
    }

    for (u32 i = 0; i < a.nout; ++i) {
        const FastDiv dtk = a.tk.at(i);
        const u32 ts = a.ts[i], txi = a.tx[i], tyi = ts - txi;
        const bool has_value = i < a.nsel;
        const u64 Ti = has_value ? (u64)a.L * ts + tyi : (u64)a.L;
        const Unit *X = reinterpret_cast<const Unit *>(has_value ? a.x[i] : nullptr);
        const Unit *Y = reinterpret_cast<const Unit *>(has_value ? a.y[i] : nullptr);
        Unit *o = reinterpret_cast<Unit *>(a.out[i]);
        const u32 len = ne * a.QP * dtk.d;          // (element, q, value term, unit), below 2^32 by the plan
        for (u32 l = threadIdx.x; l < len; l += 256u) {
            const u32 eq = csgn_fastdiv(l, dtk), rem = l - eq * dtk.d;
            const u32 c = csgn_fastdiv(rem, a.dKC), kk = rem - c * a.KC;
            const u32 el = csgn_fastdiv(eq, a.dQP), qi = eq - el * a.QP;
            if (qi >= nq || kk >= kc)
                continue;
            const u32 k = k0 + kk, q = q0 + qi;
            const u64 e = e0 + el;
            Unit v;
            if (Fresh) {
                const u32 cd = code[qi];
                v = subset_and(taba, a.tabs, el, cd & 0xFFFFu, a.KC, kk) & subset_and(tabb, a.tabs, el, cd >> 16, a.KC, kk);
            } else {
                v = one_unit(Unit(), k, a.U, a.last_mask);
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
                    v &= p < taj ? reinterpret_cast<const Unit *>(a.a[j])[(e * taj + p) * a.U + k]
                                 : B[(e * tbj + (p - taj)) * a.U + k];
                    if (cc < tbj) {
                        v &= B[(e * tbj + cc) * a.U + k];
                        done = true;
                    } else {
                        in = cc - tbj;
                    }
                }
                if (!done) {
                    const FastDiv di = a.inner.at(0);
                    const u32 ta0 = a.ta[0], p = csgn_fastdiv(in, di), cc = in - p * di.d;
                    if (p < ta0)
                        v &= reinterpret_cast<const Unit *>(a.a[0])[(e * ta0 + p) * a.U + k];
                    v &= reinterpret_cast<const Unit *>(a.b[0])[(e * di.d + cc) * a.U + k];
                }
            }
            if (has_value)
                v &= c < txi ? X[(e * txi + c) * a.U + k] : Y[(e * tyi + (c - txi)) * a.U + k];
            unit_store<Unit, true>(o + (e * Ti + (u64)q * ts + c) * a.U + k, v);
        }
        if (has_value && qpart == 0u) {             // the tail: Y_i's terms, copied
            const u32 tail = ne * tyi * a.KC;
            for (u32 l = threadIdx.x; l < tail; l += 256u) {
                const u32 row = csgn_fastdiv(l, a.dKC), kk = l - row * a.KC;
                const u32 el = row / tyi, c = row - el * tyi;
                if (kk >= kc)
                    continue;
                const u64 e = e0 + el;
                const u32 k = k0 + kk;
                unit_store<Unit, true>(o + (e * Ti + (u64)a.L * ts + c) * a.U + k, Y[(e * tyi + c) * a.U + k]);
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
    a.nout = (u32)(n_out + (less ? 1 : 0));
    a.U = U;
    a.L = (u32)L;
    a.last_mask = last_word_mask(n_bits);
    bool fresh = true;
    for (u32 j = 0; j < w; ++j) {
        a.ta[j] = (u32)ta[j];
        a.tb[j] = (u32)tb[j];
        a.inner.set(j, (u32)(tb[j] + (j ? Ls[j - 1] : 0)));
        fresh = fresh && ta[j] == 1 && tb[j] == 1;
    }
    u64 sumt = 0, maxt = 1;
    for (u32 i = 0; i < a.nout; ++i) {
        a.tx[i] = i < n_out ? (u32)tx[i] : 0u;
        a.ts[i] = i < n_out ? (u32)(tx[i] + ty[i]) : 1u;
        sumt += a.ts[i];
        maxt = std::max<u64>(maxt, a.ts[i]);
    }
    SubsetPlan sp = subset_plan(fresh ? (u32)w : 0, U, (u32)sizeof(Unit), kTableBudget);
    a.KC = sp.KC;
    a.chunks = sp.chunks;
    // The range of q a workgroup decodes: the shortest with which one element gives it kPartUnits to write, kOutUnits
    // per output (each output is a loop of its own, with its own scalar set-up) and four times what its two table sets
    // cost to build (both sets are per element, so that ratio does not depend on G) -- a batch of a few hundred
    // elements has no other source of workgroups -- then elements until it has as much.
    const u64 part_units = std::max<u64>({kPartUnits, kOutUnits * a.nout, 8 * sp.entries * a.KC});
    const u64 want_QP = std::min<u64>({(part_units + sumt * a.KC - 1) / (sumt * a.KC), (u64)kMaxRange, L});
    const u64 qparts = (L + want_QP - 1) / want_QP;
    const u64 QP = (L + qparts - 1) / qparts;
    a.QP = (u32)QP;
    a.qparts = (u32)((L + QP - 1) / QP);
    const u64 capG = std::min<u64>({sp.max_G, batch, kMaxTile});
    const u64 cell = QP * sumt * a.KC;              // units of one element of a workgroup
    u64 G = 1;
    while (G * cell < part_units && 2 * G <= capG)
        G *= 2;
    // one output's stream of a workgroup, G * QP * ts_i * KC, stays below 2^32 (QP * ts_i * KC <= T_i * U < 2^31)
    while (G > 1 && G * QP * maxt * a.KC > 0xFFFFFFFFull)
        G /= 2;
    a.G = (u32)G;
    a.dKC = csgn_fastdiv_make(a.KC);
    a.dQP = csgn_fastdiv_make(a.QP);
    for (u32 i = 0; i < a.nout; ++i)
        a.tk.set(i, a.ts[i] * a.KC);
    u32 lds = 0;
    if (fresh) {
        a.bbase = (sp.layout(a.G) + 15u) & ~15u;
        a.lbase = 2u * a.bbase;
        lds = a.lbase + a.QP * 4u;
        a.tabs = sp.t;
    }
    a.xcd = stream_xcd(batch * (L * sumt) * U);
    const u64 per_group = (u64)a.chunks * a.qparts;
    return launch_groups(launch_blocks(), batch, a.G, per_group, [&](u64 e0, u64 ne, u32 nblocks) {
        a.batch = ne;
        for (u32 j = 0; j < w; ++j) {
            a.a[j] = reinterpret_cast<const Unit *>(pa[j]) + e0 * ta[j] * U;
            a.b[j] = reinterpret_cast<const Unit *>(pb[j]) + e0 * tb[j] * U;
        }
        for (u32 i = 0; i < a.nout; ++i) {
            if (i < n_out) {                        // the comparison, output n_out, has no value planes
                a.x[i] = reinterpret_cast<const Unit *>(x[i]) + e0 * tx[i] * U;
                a.y[i] = reinterpret_cast<const Unit *>(y[i]) + e0 * ty[i] * U;
                a.out[i] = reinterpret_cast<Unit *>(out[i]) + e0 * (L * a.ts[i] + ty[i]) * U;
            } else {
                a.out[i] = reinterpret_cast<Unit *>(less) + e0 * L * U;
            }
        }
        a.nblocks = nblocks;
        if (fresh)
            k_uint_lt_select<Unit, true><<<dim3(a.nblocks), 256, lds, st>>>(a);
        else
            k_uint_lt_select<Unit, false><<<dim3(a.nblocks), 256, 0, st>>>(a);
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
