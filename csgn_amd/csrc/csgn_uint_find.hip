// csgn_uint_find.hip -- an ENCRYPTED table looked up by ENCRYPTED key, every output plane and the membership bit in one
// launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.19.
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
// hits in L2.  Lanes walk one output's stream with the unit fastest, then the value term, q, the row and the element,
// so one store instruction writes 64 consecutive units of one plane.  Multi-term planes take the digits per unit
// straight from the planes (correct, not fast).
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kTableBudget = 20480;     // bytes of subset tables per workgroup, each of the two sets (48 KB with the list)
constexpr u32 kMaxRange = 2048;         // entries of q one workgroup decodes (8 KB of LDS)
constexpr u64 kPartUnits = 8192;        // units a workgroup writes at least, where the shape has them
constexpr u32 kMaxTile = 64;            // elements, and rows, of a workgroup at most

// By value in the kernel arguments (uniform, scalar loads).  A workgroup is (element group, unit chunk, row part, q
// part): elements [group * G, + G), units [chunk * KC, + KC) of every term, rows [rpart * RP, + RP) and entries
// [qpart * QP, + QP) of every row's block.  Output w is member (one term per entry, no value factor).
struct FindArgs {
    const void *keys[kFindMaxKey];
    const void *query[kFindMaxKey];
    const void *values[kFindMaxPlanes];
    void *out[kFindMaxPlanes + 1];
    u32 t[kFindMaxPlanes + 1];                                          // terms of value plane j; 1 for member
    FastDivTable<kFindMaxPlanes + 1> tk;                                // t_j * KC
    u32 u[kFindMaxKey], s[kFindMaxKey];
    u64 last_mask;
    u64 batch;                  // elements of this launch
    u64 E;                      // rows * P of the whole call: T_j = t_j * E
    u32 rows;                   // rows of this launch
    u32 P, v, w, nout;
    u32 U, KC, G, RP, QP, chunks, rparts, qparts, nblocks, xcd;
    SubsetTables tq, tr;        // the query tables of G elements, the key tables of RP rows
    u32 kbase, lbase;           // byte offsets of the key tables and of the decoded range in the LDS
    FastDiv dKC, dQP, dRP;
};

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_find(FindArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Unit *tabq = reinterpret_cast<Unit *>(smem_raw);
    Unit *tabk = reinterpret_cast<Unit *>(smem_raw + a.kbase);
    u32 *code = reinterpret_cast<u32 *>(smem_raw + a.lbase);
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, a.nblocks) : blockIdx.x;
    const u32 gcr = bid / a.qparts, qpart = bid - gcr * a.qparts;
    const u32 gc = gcr / a.rparts, rpart = gcr - gc * a.rparts;
    const u32 group = gc / a.chunks, chunk = gc - group * a.chunks;
    const u64 e0 = (u64)group * a.G;
    const u32 ne = (u32)min((u64)a.G, a.batch - e0);
    const u32 k0 = chunk * a.KC, kc = min(a.KC, a.U - k0);
    const u32 r0 = rpart * a.RP, nr = min(a.RP, a.rows - r0);
    const u32 q0 = qpart * a.QP, nq = min(a.QP, a.P - q0);

    if (Fresh) {
        // the range of q: Sq in the low 16 bits, Sk in the high 16 (published by the tables' closing barrier)
        for (u32 i = threadIdx.x; i < nq; i += 256u) {
            u32 q = q0 + i, Sk = 0, Sq = 0;
            for (u32 k = a.v; k-- > 0u;) {      // k = 0 is the slowest digit: 0 = y_k, 1 = x_k, 2 = ONE
                const u32 nx = q / 3u, dg = q - nx * 3u;
                q = nx;
                Sk |= (dg == 0u ? 1u : 0u) << k;
                Sq |= (dg == 1u ? 1u : 0u) << k;
            }
            code[i] = Sq | (Sk << 16);
        }
        subset_build(tabq, a.tq, a.query, a.G, a.KC, a.dKC, a.U, a.last_mask, e0, ne, k0, kc);
        subset_build(tabk, a.tr, a.keys, a.RP, a.KC, a.dKC, a.U, a.last_mask, (u64)r0, nr, k0, kc);
    }

    for (u32 j = 0; j < a.nout; ++j) {
        const FastDiv dtk = a.tk.at(j);
        const u32 tj = a.t[j];
        const u64 Tj = (u64)tj * a.E;
        const bool has_value = j < a.w;
        const Unit *d = reinterpret_cast<const Unit *>(has_value ? a.values[j] : nullptr);
        Unit *o = reinterpret_cast<Unit *>(a.out[j]);
        const u32 len = ne * a.RP * a.QP * dtk.d;   // (element, row, q, value term, unit), below 2^32 by the plan
        for (u32 l = threadIdx.x; l < len; l += 256u) {
            const u32 erq = csgn_fastdiv(l, dtk), rem = l - erq * dtk.d;
            const u32 c = csgn_fastdiv(rem, a.dKC), kk = rem - c * a.KC;
            const u32 er = csgn_fastdiv(erq, a.dQP), qi = erq - er * a.QP;
            const u32 el = csgn_fastdiv(er, a.dRP), rr = er - el * a.RP;
            if (qi >= nq || kk >= kc || rr >= nr)
                continue;
            const u32 k = k0 + kk, r = r0 + rr, q = q0 + qi;
            const u64 e = e0 + el;
            Unit v;
            if (Fresh) {
                const u32 cd = code[qi];
                v = subset_and(tabq, a.tq, el, cd & 0xFFFFu, a.KC, kk) & subset_and(tabk, a.tr, rr, cd >> 16, a.KC, kk);
            } else {
                v = one_unit(Unit(), k, a.U, a.last_mask);
                u32 in = q;
                for (u32 kb = a.v; kb-- > 0u;) {
                    const u32 uk = a.u[kb], sk = a.s[kb], R = uk + sk + 1u;
                    const u32 nx = in / R, dg = in - nx * R;
                    in = nx;
                    if (dg < uk)
                        v &= reinterpret_cast<const Unit *>(a.keys[kb])[((u64)r * uk + dg) * a.U + k];
                    else if (dg < uk + sk)
                        v &= reinterpret_cast<const Unit *>(a.query[kb])[(e * sk + (dg - uk)) * a.U + k];
                }
            }
            if (has_value)
                v &= d[((u64)r * tj + c) * a.U + k];
            unit_store<Unit, true>(o + (e * Tj + ((u64)r * a.P + q) * tj + c) * a.U + k, v);
        }
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
    a.nout = (u32)(w + (member ? 1 : 0));
    a.U = U;
    a.P = (u32)P;
    a.E = rows * P;
    a.last_mask = last_word_mask(n_bits);
    bool fresh = true;
    for (u32 k = 0; k < v; ++k) {
        a.u[k] = (u32)u[k];
        a.s[k] = (u32)s[k];
        fresh = fresh && u[k] == 1 && s[k] == 1;
    }
    u64 sumt = 0, maxt = 1;
    for (u32 j = 0; j < a.nout; ++j) {
        a.t[j] = j < w ? (u32)t[j] : 1u;
        sumt += a.t[j];
        maxt = std::max<u64>(maxt, a.t[j]);
    }
    SubsetPlan sp = subset_plan(fresh ? (u32)v : 0, U, (u32)sizeof(Unit), kTableBudget);
    a.KC = sp.KC;
    a.chunks = sp.chunks;
    // the range of q a workgroup decodes, then elements and rows in turn until it has kPartUnits to write and four
    // times what its tables cost to build
    const u64 qparts = (P + kMaxRange - 1) / kMaxRange;
    const u64 QP = (P + qparts - 1) / qparts;
    a.QP = (u32)QP;
    a.qparts = (u32)((P + QP - 1) / QP);
    const u64 capG = std::min<u64>({sp.max_G, batch, kMaxTile}), capR = std::min<u64>({sp.max_G, rows, kMaxTile});
    const u64 cell = QP * sumt * a.KC;              // units of one (element, row) of a workgroup
    u64 G = 1, RP = 1;
    for (;;) {
        const u64 build = (G + RP) * sp.entries * a.KC;
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
    // one output's stream of a workgroup, G * RP * QP * t_j * KC, stays below 2^32 (QP * t_j * KC <= T_j * U < 2^31)
    while (G * RP > 1 && G * RP * QP * maxt * a.KC > 0xFFFFFFFFull) {
        if (G >= RP)
            G /= 2;
        else
            RP /= 2;
    }
    a.G = (u32)G;
    a.RP = (u32)RP;
    a.dKC = csgn_fastdiv_make(a.KC);
    a.dQP = csgn_fastdiv_make(a.QP);
    a.dRP = csgn_fastdiv_make(a.RP);
    for (u32 j = 0; j < a.nout; ++j)
        a.tk.set(j, a.t[j] * a.KC);
    u32 lds = 0;
    if (fresh) {
        SubsetPlan spq = sp, spr = sp;
        a.kbase = (spq.layout(a.G) + 15u) & ~15u;
        a.lbase = (a.kbase + spr.layout(a.RP) + 15u) & ~15u;
        lds = a.lbase + a.QP * 4u;
        a.tq = spq.t;
        a.tr = spr.t;
    }
    a.xcd = stream_xcd(batch * rows * P * sumt * U);
    // rows of one launch: as many parts as a launch's workgroups allow (every shape within memory: all of them), or
    // as knob uint_find_rparts says, which is how the tests reach the launches from row rl > 0 on
    const u64 per_rpart = (u64)a.chunks * a.qparts;
    const int forced_rparts = tune(TUNE_UINT_FIND_RPARTS);
    const u64 max_blocks = launch_blocks();
    const u64 launch_rows = (forced_rparts > 0 ? (u64)forced_rparts : std::max<u64>(1, max_blocks / per_rpart)) * RP;
    for (u64 rl = 0; rl < rows; rl += launch_rows) {
        const u64 nrows = std::min(launch_rows, rows - rl);
        a.rows = (u32)nrows;
        a.rparts = (u32)((nrows + RP - 1) / RP);
        const hipError_t err = launch_groups(max_blocks, batch, a.G, per_rpart * a.rparts, [&](u64 e0, u64 ne, u32 nblocks) {
            a.batch = ne;
            for (u32 k = 0; k < v; ++k) {
                a.query[k] = reinterpret_cast<const Unit *>(query[k]) + e0 * s[k] * U;
                a.keys[k] = reinterpret_cast<const Unit *>(keys[k]) + rl * u[k] * U;
            }
            for (u32 j = 0; j < a.nout; ++j) {
                if (j < w)                          // member, output w, has no value plane
                    a.values[j] = reinterpret_cast<const Unit *>(values[j]) + rl * t[j] * U;
                a.out[j] = reinterpret_cast<Unit *>(j < w ? out[j] : member) + (e0 * a.E + rl * P) * a.t[j] * U;
            }
            a.nblocks = nblocks;
            if (fresh)
                k_uint_find<Unit, true><<<dim3(a.nblocks), 256, lds, st>>>(a);
            else
                k_uint_find<Unit, false><<<dim3(a.nblocks), 256, 0, st>>>(a);
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
