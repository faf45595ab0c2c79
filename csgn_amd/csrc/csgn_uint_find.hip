// csgn_uint_find.hip -- an ENCRYPTED table looked up by ENCRYPTED key, every output plane and the membership bit in one
// launch.  Hand-written CDNA4 (gfx950) HIP; the kernel skeleton in csgn_selector.h, design notes in DESIGN.md §4.19.
//
// The definition (include/csgn_hip.h, csgn_uint_find) is out_j = sum over r < rows, ascending, of EQ(y_r, x) * d_{r,j}
// and member = sum over r of EQ(y_r, x): the equalTo chain of key row r (left) and the query (right) as the left
// operand, plane j of value row r as the right.  Every row has the same P = prod_k (u_k + s_k + 1) EQ terms, so entry
// Q = r * P + q of the E stream (rows * P entries) is decoded by one division, and q by its mixed-radix digits with
// k = 0 slowest: digit < u_k a term of y_{r,k}, < u_k + s_k a term of x_k, else ONE.  Term Q * t_j + c of output j is
// (entry Q) & (term c of d_{r,j}); member is the E stream itself.
//
// Fresh planes (every u_k = s_k = 1), the case this kernel is built for: entry q is Pk_r[Sk] & Pq_e[Sq], the ANDs of
// the key planes over Sk = {digits 0} and of the query planes over Sq = {digits 1}, and the base-3 decode is the same
// for every row.  A workgroup owns G query elements, RP key rows, a slice of KC units of every term and one range of
// q, for EVERY output: it decodes its range once into an LDS list (Sq | Sk << 16) and builds the subset tables of
// §4.15 (csgn_device.h) twice, for its elements' query planes and -- the "element" being the row -- for its rows' key
// planes.  A written unit is then 2-6 LDS reads ANDed with one unit of the value row, which every query reads, so it
// hits in L2.  Multi-term planes take the digits per unit straight from the planes (correct, not fast).
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kTableBudget = 20480;     // bytes of subset tables per workgroup, each of the two sets (48 KB with the list)
constexpr u32 kMaxRange = 2048;         // entries of q one workgroup decodes (8 KB of LDS)
constexpr u64 kPartUnits = 8192;        // units a workgroup writes at least, where the shape has them
constexpr u32 kMaxTile = 64;            // elements, and rows, of a workgroup at most

// By value in the kernel arguments (uniform, scalar loads).  The tile has one more level, between the unit chunk and
// the q part: rows [rpart * RP, + RP); the stream is every row's block of P entries.  Output w is member (one term per
// entry, no value factor).
struct FindArgs {
    SelTile tile;
    SelOutputs<kFindMaxPlanes + 1> outs;
    const void *keys[kFindMaxKey];
    const void *query[kFindMaxKey];
    const void *values[kFindMaxPlanes];
    u32 u[kFindMaxKey], s[kFindMaxKey];
    u64 E;                      // rows * P of the whole call: T_j = t_j * E
    u32 rows;                   // rows of this launch
    u32 P, v, w;
    u32 RP, rparts;
    SubsetTables tq, tr;        // the query tables of G elements, the key tables of RP rows (the tile's second set)
    FastDiv dRP;
};
static_assert(sizeof(FindArgs) <= 4096, "the kernel arguments of k_uint_find pass the 4 KiB limit");

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_find(FindArgs a)
{
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit, true>(t, a.P, a.rparts);
    const u32 r0 = b.mid * a.RP, nr = min(a.RP, a.rows - r0);

    if (Fresh) {
        // the range of q: Sq in the low 16 bits, Sk in the high 16 (published by the tables' closing barrier)
        for (u32 i = threadIdx.x; i < b.nq; i += 256u) {
            u32 S[2] = {0u, 0u};                // k = 0 is the slowest digit: 0 = y_k, 1 = x_k, 2 = ONE
            eq_digits<true>(b.q0 + i, a.v, a.u, a.s, [&](u32 side, u32 k, u32) { S[side] |= 1u << k; });
            b.code[i] = S[1] | (S[0] << 16);
        }
        subset_build(b.tab, a.tq, a.query, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc);
        subset_build(b.tab2, a.tr, a.keys, a.RP, t.KC, t.dKC, t.U, t.last_mask, (u64)r0, nr, b.k0, b.kc);
    }

    for (u32 j = 0; j < a.outs.nout; ++j) {
        const u32 tj = a.outs.t[j];
        const u64 Tj = (u64)tj * a.E;
        const bool has_value = j < a.w;
        const Unit *d = reinterpret_cast<const Unit *>(has_value ? a.values[j] : nullptr);
        // a tile is (element, row), the row the faster
        sel_walk<Unit>(t, b, a.outs, j, b.ne * a.RP, [&](u32 er, u32 qi, u32 c, u32 kk, u64 &at, Unit &v) {
            const u32 el = csgn_fastdiv(er, a.dRP), rr = er - el * a.RP;
            if (rr >= nr)
                return false;
            const u32 k = b.k0 + kk, r = r0 + rr, q = b.q0 + qi;
            const u64 e = b.e0 + el;
            if (Fresh) {
                const u32 cd = b.code[qi];
                v = subset_and(b.tab, a.tq, el, cd & 0xFFFFu, t.KC, kk) & subset_and(b.tab2, a.tr, rr, cd >> 16, t.KC, kk);
            } else {
                v = one_unit(Unit(), k, t.U, t.last_mask);
                eq_digits<false>(q, a.v, a.u, a.s, [&](u32 side, u32 kb, u32 i) {
                    v &= side == 0u ? reinterpret_cast<const Unit *>(a.keys[kb])[((u64)r * a.u[kb] + i) * t.U + k]
                                    : reinterpret_cast<const Unit *>(a.query[kb])[(e * a.s[kb] + i) * t.U + k];
                });
            }
            if (has_value)
                v &= d[((u64)r * tj + c) * t.U + k];
            at = (e * Tj + ((u64)r * a.P + q) * tj + c) * t.U + k;
            return true;
        });
    }
}

// ------------------------------------------------------------------------------ host side

bool find_shape_ok(u64 v, const u64 *u, const u64 *s, u64 rows, u64 w, const u64 *t, bool member)
{
    if (rows < 1 || w > kFindMaxPlanes || (w == 0 && !member) || (w > 0 && !t) || uint_find_terms(v, u, s) == 0)
        return false;
    for (u64 j = 0; j < w; ++j)
        if (t[j] == 0 || t[j] >= kTermLimit)
            return false;
    return true;
}

// Per shape (measured): the fused kernel.  One launch against rows * (v + w + 3) of the composed form;
// no measured shape has the composed form ahead.
bool find_use_fused()
{
    return tune_choose(TUNE_UINT_FIND_FORM, true);
}

template <typename Unit>
hipError_t find_fused(u64 n_bits, u64 batch, u64 v, const u64 *const *query, const u64 *s, u64 rows,
                      const u64 *const *keys, const u64 *u, u64 w, const u64 *const *values, const u64 *t,
                      u64 *const *out, u64 *member, u64 P, u32 U, hipStream_t st)
{
    FindArgs a = {};
    a.v = (u32)v;
    a.w = (u32)w;
    a.P = (u32)P;
    a.E = rows * P;
    bool fresh = true;
    for (u32 k = 0; k < v; ++k) {
        a.u[k] = (u32)u[k];
        a.s[k] = (u32)s[k];
        fresh = fresh && u[k] == 1 && s[k] == 1;
    }
    const SubsetPlan sp = subset_plan(fresh ? (u32)v : 0, U, (u32)sizeof(Unit), kTableBudget);
    const u64 sumt = a.outs.fill(w, [&](u32 j) { return t[j]; }, member != nullptr, sp.KC);
    // the range of q a workgroup decodes, then elements and rows in turn until it has kPartUnits to write and four
    // times what its tables cost to build
    const u64 qparts = (P + kMaxRange - 1) / kMaxRange;
    const u64 QP = (P + qparts - 1) / qparts;
    const u64 capG = std::min<u64>({sp.max_G, batch, kMaxTile}), capR = std::min<u64>({sp.max_G, rows, kMaxTile});
    const u64 cell = QP * sumt * sp.KC;             // units of one (element, row) of a workgroup
    u64 G = 1, RP = 1;
    for (;;) {
        const u64 build = (G + RP) * sp.entries * sp.KC;
        if (G * RP * cell >= std::max<u64>(kPartUnits, 4 * build))
            break;
        const bool moreG = 2 * G <= capG, moreR = 2 * RP <= capR;
        if (moreR && (RP <= G || !moreG))
            RP *= 2;
        else if (moreG)
            G *= 2;
        else
            break;
    }
    RP = a.tile.set(n_bits, U, sp, QP, P, a.outs, G, RP);      // the guard may halve G (a.tile.G) and RP
    a.RP = (u32)RP;
    a.dRP = csgn_fastdiv_make(a.RP);
    const u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.tq, a.RP, &a.tr) : 0u;
    a.tile.xcd = stream_xcd(batch * rows * P * sumt * U);
    // rows of one launch: as many parts as a launch's workgroups allow (every shape within memory: all of them), or
    // as knob uint_find_rparts says, which is how the tests reach the launches from row rl > 0 on
    const u64 per_rpart = (u64)a.tile.chunks * a.tile.qparts;
    const int forced_rparts = tune(TUNE_UINT_FIND_RPARTS);
    const u64 max_blocks = launch_blocks();
    const u64 launch_rows = (forced_rparts > 0 ? (u64)forced_rparts : std::max<u64>(1, max_blocks / per_rpart)) * RP;
    for (u64 rl = 0; rl < rows; rl += launch_rows) {
        const u64 nrows = std::min(launch_rows, rows - rl);
        a.rows = (u32)nrows;
        a.rparts = (u32)((nrows + RP - 1) / RP);
        const hipError_t err = sel_launch(k_uint_find<Unit, true>, k_uint_find<Unit, false>, a, lds, max_blocks, batch,
                                          per_rpart * a.rparts, st, [&](u64 e0) {
            for (u32 k = 0; k < v; ++k) {
                a.query[k] = reinterpret_cast<const Unit *>(query[k]) + e0 * s[k] * U;
                a.keys[k] = reinterpret_cast<const Unit *>(keys[k]) + rl * u[k] * U;
            }
            for (u32 j = 0; j < a.outs.nout; ++j) {
                if (j < w)                          // member, output w, has no value plane
                    a.values[j] = reinterpret_cast<const Unit *>(values[j]) + rl * t[j] * U;
                a.outs.out[j] = reinterpret_cast<Unit *>(j < w ? out[j] : member) + (e0 * a.E + rl * P) * a.outs.t[j] * U;
            }
        });
        if (err != hipSuccess)
            return err;
    }
    return hipSuccess;
}

// The composed form, row by row through the tuned launchers: row r of every key and value plane broadcast to the batch
// by csgn_gather_planes' tile form, the XNOR gate of plane 0 and one EQ_STEP per further plane (csgn_gate_uniform's and
// csgn_uint_step's launchers) into a temporary, then csgn_mul_uniform of that EQ and every value row into r's slice of
// the output (pitch T_j) and a pitched copy of the EQ into r's slice of member.  The temporaries live in one block
// (scratch_take, csgn_kernels.h): the tiled rows, and two running values that take turns so the last lands in the first.
hipError_t find_composed(u64 n_bits, u64 batch, u64 v, const u64 *const *query, const u64 *s, u64 rows,
                         const u64 *const *keys, const u64 *u, u64 w, const u64 *const *values, const u64 *t,
                         u64 *const *out, u64 *member, u64 P, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64, E = rows * P;
    u64 sumu = 0, sumt = 0;
    for (u64 k = 0; k < v; ++k)
        sumu += u[k];
    for (u64 j = 0; j < w; ++j)
        sumt += t[j];
    const u64 before_last = P / (u[v - 1] + s[v - 1] + 1);          // the EQ terms before the last plane
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_UINT_FIND, batch * (P + before_last + sumu + sumt) * dL * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *eq[2] = {block, block + batch * P * dL};
    u64 at = batch * (P + before_last) * dL;
    const u64 *ksrc[kFindMaxKey], *vsrc[kFindMaxPlanes];
    u64 *krow[kFindMaxKey], *vrow[kFindMaxPlanes];
    for (u64 k = 0; k < v; ++k) {
        krow[k] = block + at;
        at += batch * u[k] * dL;
    }
    for (u64 j = 0; j < w; ++j) {
        vrow[j] = block + at;
        at += batch * t[j] * dL;
    }
    for (u64 r = 0; r < rows && e == hipSuccess; ++r) {
        for (u64 k = 0; k < v; ++k)
            ksrc[k] = keys[k] + r * u[k] * dL;
        for (u64 j = 0; j < w; ++j)
            vsrc[j] = values[j] + r * t[j] * dL;
        e = gather_planes(n_bits, v, ksrc, u, 1, batch, nullptr, krow, st);
        if (e == hipSuccess && w)
            e = gather_planes(n_bits, w, vsrc, t, 1, batch, nullptr, vrow, st);
        // the running value takes turns between the two buffers; plane v - 1 writes eq[0]
        u64 terms = u[0] + s[0] + 1;
        u32 cur = (u32)((v - 1) & 1u);
        if (e == hipSuccess)
            e = gate_uniform(n_bits, CSGN_GATE_XNOR, batch, 0, u[0], s[0], nullptr, krow[0], query[0], nullptr, eq[cur], st);
        for (u64 k = 1; k < v && e == hipSuccess; ++k) {
            e = uint_step(n_bits, CSGN_UINT_EQ_STEP, batch, eq[cur], terms, krow[k], u[k], query[k], s[k], eq[cur ^ 1u],
                          nullptr, st);
            terms *= u[k] + s[k] + 1;
            cur ^= 1u;
        }
        for (u64 j = 0; j < w && e == hipSuccess; ++j)
            e = mul_uniform(n_bits, batch, P, t[j], eq[0], vrow[j], out[j] + r * P * t[j] * dL, 0, st, t[j] * E * dL);
        if (member && e == hipSuccess)
            e = add_uniform(n_bits, batch, P, 0, eq[0], nullptr, member + r * P * dL, st, E * dL);
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_find_terms(u64 v, const u64 *u, const u64 *s)
{
    if (v < 1 || v > kFindMaxKey || !u || !s)
        return 0;
    u64 P = 1;
    for (u64 k = 0; k < v; ++k) {
        if (u[k] == 0 || s[k] == 0 || u[k] >= kTermLimit || s[k] >= kTermLimit || !term_mul(P, u[k] + s[k] + 1, P))
            return 0;
    }
    return P;
}

const char *uint_find_kernel_name(u64 n_bits, u64 batch, u64 v, const u64 *u, const u64 *s, u64 rows, u64 w,
                                  const u64 *t, bool member)
{
    (void)batch;
    if (n_bits == 0 || !find_shape_ok(v, u, s, rows, w, t, member))
        return "";
    return find_use_fused() ? "k_uint_find" : "composed";
}

hipError_t uint_find(u64 n_bits, u64 batch, u64 v, const u64 *const *query, const u64 *s, u64 rows,
                     const u64 *const *keys, const u64 *u, u64 w, const u64 *const *values, const u64 *t,
                     u64 *const *out, u64 *member, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    const u64 P = uint_find_terms(v, u, s);
    if (!find_use_fused())
        return find_composed(n_bits, batch, v, query, s, rows, keys, u, w, values, t, out, member, P, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(query, v), ptr_array(keys, v), ptr_array(values, w), ptr_array(out, w),
                                 member);
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? find_fused<unit16>(n_bits, batch, v, query, s, rows, keys, u, w, values, t, out, member, P, U, stream)
                : find_fused<unit8>(n_bits, batch, v, query, s, rows, keys, u, w, values, t, out, member, P, U, stream);
}

} // namespace csgn
