// csgn_uint_write.hip -- ENCRYPTED arrays written at ENCRYPTED indices, every output plane in one launch.
// Hand-written CDNA4 (gfx950) HIP; the kernel skeleton in csgn_selector.h, design notes in DESIGN.md §4.26.
//
// The definition (include/csgn_hip.h, csgn_uint_write): element e owns rows e * n .. e * n + n - 1 of every array plane
// (csgn_uint_pick's EACH layout), and row r of plane j becomes
//     logicMux(EQ(index_e, r), value_{e,j}, d_{e*n+r,j})  =  (EQ(index_e, r) * (value_{e,j} + d_{e*n+r,j})) + d_{e*n+r,j}
// with EQ csgn_uint_plain's EQ row with k = r, the LEFT operand.  With t_j = tv_j + td_j, row r is P_r * t_j + td_j
// terms (P_r = prod_k R_k(r), the EQ row's): its EQ entries are the entries [qstart(r), qstart(r) + P_r) of the E stream
// of n rows (csgn_uint_read.hip's; the index arguments, the evaluation of an entry and the tile policy are
// csgn_selector.h's, as for k_uint_read and k_uint_pick), so inside an array of A_j = E * t_j + n * td_j terms
//     term c < t_j of entry q (of row r)   lies at q * t_j + r * td_j + c  and is  entry & (c < tv_j ? value term c
//                                                                                                : row-r term c - tv_j)
//     the raw copy of row r                follows the row's LAST entry: copied term c' lies td_j terms past the product
//                                          term built from row term c' by that entry
// A workgroup owns G arrays, a slice of KC units of every term and one range of the E stream, for EVERY output plane; it
// builds the subset tables and decodes its range once (fresh index planes), as k_uint_read does, and walks every plane
// through sel_walk (unit-fastest lanes, non-temporal stores).  The lane that writes a product term from a row term of a
// row's last entry also writes that term's copy: the tails need no second pass and no second launch, and the workgroup
// that owns the row's last entry and the unit slice writes them.  The last entry of a row is the one whose digits are
// all maximal; with fresh planes it is the decoded entry with S == r, else the next entry (if any) belongs to another
// row.  Multi-term index planes take the walk and the digits per unit straight from the planes (correct, not fast).
// The kernel arguments -- two pointer arrays and the value term counts beside the outputs and the index, 64 planes --
// stay within the 4 KiB limit (asserted below), so a call is never split over the planes; the host splits it over the
// batch only (launch_groups).  This file keeps the array layout, the tails and the composed form.
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>
#include <vector>

namespace csgn {

namespace {

// By value in the kernel arguments (uniform, scalar loads); the stream is the E stream of n rows, output j has
// t_j = tv_j + td_j terms per entry (outs.t) of which the first tv_j come from the value.
struct WriteArgs {
    SelTile tile;
    SelOutputs<kWriteMaxPlanes> outs;
    SelIndex x;
    const void *value[kWriteMaxPlanes];
    const void *arrays[kWriteMaxPlanes];
    u32 tv[kWriteMaxPlanes];
    u32 E, n;
};
static_assert(sizeof(WriteArgs) <= 4096, "the kernel arguments of k_uint_write pass the 4 KiB limit");

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_write(WriteArgs a)
{
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit>(t, a.E);

    if (Fresh) {
        read_decode(a.x, b);
        subset_build(b.tab, a.x.tabs, a.x.index, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc);
    }

    for (u32 j = 0; j < a.outs.nout; ++j) {
        const u32 tj = a.outs.t[j], tv = a.tv[j], td = tj - tv;
        const u64 Aj = (u64)tj * a.E + (u64)td * a.n;
        const Unit *val = reinterpret_cast<const Unit *>(a.value[j]);
        const Unit *arr = reinterpret_cast<const Unit *>(a.arrays[j]);
        Unit *o = reinterpret_cast<Unit *>(a.outs.out[j]);
        sel_walk<Unit>(t, b, a.outs, j, b.ne, [&](u32 el, u32 qi, u32 c, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk;
            const u64 e = b.e0 + el, q = (u64)b.q0 + qi;
            const u32 r = read_entry<Unit, Fresh>(a.x, t, b, el, e, qi, q, k, kk, v);
            at = (e * Aj + q * tj + (u64)r * td + c) * t.U + k;
            if (c < tv) {
                v &= val[(e * tv + c) * t.U + k];
                return true;
            }
            const Unit d = arr[((e * a.n + r) * td + (c - tv)) * t.U + k];
            v &= d;
            bool last;                  // of row r's entries: the row's raw copy follows it
            if (Fresh) {
                const u32 cd = b.code[qi];
                last = (cd & 0xFFFFu) == (cd >> 16);
            } else {
                u64 in;
                last = q + 1 == a.E || read_walk(a.x, q + 1, in) != r;
            }
            if (last)
                unit_store<Unit, true>(o + at + (u64)td * t.U, d);
            return true;
        });
    }
}

// ------------------------------------------------------------------------------ host side

struct WriteShape {
    u64 E, A[kWriteMaxPlanes], sumt, sumA;
};

// false for an invalid shape or a count of 2^62 or more
bool write_shape(u64 v, const u64 *s, u64 rows, u64 w, const u64 *tv, const u64 *td, WriteShape &ws)
{
    ws = {};
    if (w < 1 || w > kWriteMaxPlanes || !tv || !td)
        return false;
    ws.E = uint_read_terms(v, s, rows);
    if (ws.E == 0)
        return false;
    for (u64 j = 0; j < w; ++j) {
        ws.A[j] = uint_write_offset(v, s, rows, rows, tv[j], td[j]);
        if (ws.A[j] == 0)
            return false;
        ws.sumt += tv[j] + td[j];
        ws.sumA += ws.A[j];
        if (ws.sumt >= kTermLimit || ws.sumA >= kTermLimit)
            return false;
    }
    return true;
}

// The composed form's gather of the rows needs the counts below 2^32 (csgn_gather_planes): past that, the fused form.
bool write_use_fused(u64 batch, u64 rows)
{
    if (rows && batch >= ((1ull << 32) + rows - 1) / rows)      // batch * rows >= 2^32
        return true;
    // by shape: one launch for every output, no shape measured where the composed form is faster
    return tune_choose(TUNE_UINT_WRITE_FORM, true);
}

// the tile over the units an element really writes: the products and the tails of one unit slice
ReadTile write_tile(const SubsetPlan &sp, u64 batch, const WriteShape &ws)
{
    return ReadTile::of(sp, batch, ws.E, ws.sumA * sp.KC);
}

template <typename Unit>
hipError_t write_fused(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                       const u64 *const *value, const u64 *tv, const u64 *const *arrays, const u64 *td,
                       u64 *const *out, const WriteShape &ws, u32 U, hipStream_t st)
{
    WriteArgs a = {};
    a.E = (u32)ws.E;
    a.n = (u32)rows;
    const bool fresh = a.x.fill(v, s, rows);
    const SubsetPlan sp = ReadTile::plan(fresh, v, U, (u32)sizeof(Unit));
    a.outs.fill(w, [&](u32 j) { return tv[j] + td[j]; }, false, sp.KC);
    const ReadTile rt = write_tile(sp, batch, ws);
    a.tile.set(n_bits, U, sp, rt.QP, ws.E, a.outs, rt.G);
    const u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.x.tabs) : 0u;
    a.tile.xcd = stream_xcd(batch * ws.sumA * U);
    for (u32 j = 0; j < w; ++j)
        a.tv[j] = (u32)tv[j];
    return sel_launch(k_uint_write<Unit, true>, k_uint_write<Unit, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        a.x.template advance<Unit>(index, e0, U);
        for (u32 j = 0; j < w; ++j) {
            a.value[j] = reinterpret_cast<const Unit *>(value[j]) + e0 * tv[j] * U;
            a.arrays[j] = reinterpret_cast<const Unit *>(arrays[j]) + e0 * rows * td[j] * U;
            a.outs.out[j] = reinterpret_cast<Unit *>(out[j]) + e0 * ws.A[j] * U;
        }
    });
}

// The composed form, row by row through the tuned launchers: EQ(index, r) by csgn_uint_plain into a temporary, row r of
// every element's array by one csgn_gather_planes of the elements e * n + r (the list e * n is uploaded once -- the call
// waits for it -- and row r gathers from r elements on), then per plane csgn_add_uniform of the value and the row,
// csgn_mul_uniform of EQ with that sum into the row's place (pitch A_j) and the strided copy of the row behind it.  The
// temporaries live in one temporary block (scratch_take, csgn_kernels.h), apart from the one csgn_uint_plain's composed
// form may take for EQ.
hipError_t write_composed(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                          const u64 *const *value, const u64 *tv, const u64 *const *arrays, const u64 *td,
                          u64 *const *out, const WriteShape &ws, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64;
    u64 max_eq = 1, sumtd = 0, maxt = 0;    // row 0 has the most EQ terms: every R_k = s_k + 1
    for (u64 k = 0; k < v; ++k)
        max_eq *= s[k] + 1;
    for (u64 j = 0; j < w; ++j) {
        sumtd += td[j];
        maxt = std::max(maxt, tv[j] + td[j]);
    }
    const u64 eq_words = batch * max_eq * dL, sum_words = batch * maxt * dL;
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_UINT_WRITE, (eq_words + sum_words + batch * sumtd * dL + batch) * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *eq = block, *sum = block + eq_words;
    u64 *row[kWriteMaxPlanes];
    const u64 *from[kWriteMaxPlanes];
    u64 at = eq_words + sum_words;
    for (u64 j = 0; j < w; ++j) {
        row[j] = block + at;
        at += batch * td[j] * dL;
    }
    u64 *idx = block + at;
    {
        std::vector<u64> list(batch);
        for (u64 i = 0; i < batch; ++i)
            list[i] = i * rows;
        e = hipMemcpyAsync(idx, list.data(), batch * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);       // the list is the call's own
    }
    u64 off = 0;                        // r's first entry of the E stream
    for (u64 r = 0; r < rows && e == hipSuccess; ++r) {
        const u64 er = uint_plain_terms(CSGN_UINT_PLAIN_EQ, v, r, s);
        e = uint_plain(n_bits, CSGN_UINT_PLAIN_EQ, batch, v, r, index, s, eq, st);
        for (u64 j = 0; j < w; ++j)
            from[j] = arrays[j] + r * td[j] * dL;
        if (e == hipSuccess)
            e = gather_planes(n_bits, w, from, td, batch * rows - r, batch, idx, row, st);
        for (u64 j = 0; j < w && e == hipSuccess; ++j) {
            const u64 tj = tv[j] + td[j], pitch = ws.A[j] * dL;
            u64 *place = out[j] + (off * tj + r * td[j]) * dL;
            e = add_uniform(n_bits, batch, tv[j], td[j], value[j], row[j], sum, st);
            if (e == hipSuccess)
                e = mul_uniform(n_bits, batch, er, tj, eq, sum, place, 0, st, pitch);
            if (e == hipSuccess)
                e = add_uniform(n_bits, batch, 0, td[j], nullptr, row[j], place + er * tj * dL, st, pitch);
        }
        off += er;
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_write_offset(u64 v, const u64 *s, u64 rows, u64 r, u64 tv, u64 td)
{
    if (uint_read_terms(v, s, rows) == 0 || r > rows || tv == 0 || td == 0 || tv >= kTermLimit || td >= kTermLimit)
        return 0;
    const u64 q = r ? uint_read_terms(v, s, r) : 0;     // qstart(r): the entries of the rows below r
    const u64 prod = sat_mul(q, tv + td), tail = sat_mul(r, td);
    return prod + tail >= kTermLimit ? 0 : prod + tail;
}

const char *uint_write_kernel_name(u64 n_bits, u64 batch, u64 v, const u64 *s, u64 rows, u64 w, const u64 *tv,
                                   const u64 *td)
{
    WriteShape ws;
    if (n_bits == 0 || !write_shape(v, s, rows, w, tv, td, ws))
        return "";
    return write_use_fused(batch, rows) ? "k_uint_write" : "composed";
}

bool uint_write_plan(u64 n_bits, u64 batch, u64 v, const u64 *s, u64 rows, u64 w, const u64 *tv, const u64 *td,
                     bool wide, u64 plan[4])
{
    WriteShape ws;
    if (n_bits == 0 || batch == 0 || !write_shape(v, s, rows, w, tv, td, ws))
        return false;
    const u64 dL = (n_bits + 63) / 64;
    wide = wide && dL % 2 == 0;
    const bool fresh = SelIndex().fill(v, s, rows);
    const SubsetPlan sp = ReadTile::plan(fresh, v, (u32)(wide ? dL / 2 : dL), wide ? 16u : 8u);
    const ReadTile rt = write_tile(sp, batch, ws);
    plan[0] = rt.G;
    plan[1] = sp.KC;
    plan[2] = rt.QP;
    plan[3] = (ws.E + rt.QP - 1) / rt.QP;
    return true;
}

hipError_t uint_write(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                      const u64 *const *value, const u64 *tv, const u64 *const *arrays, const u64 *td, u64 *const *out,
                      hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    WriteShape ws;
    if (!write_shape(v, s, rows, w, tv, td, ws))
        return hipErrorInvalidValue;
    if (!write_use_fused(batch, rows))
        return write_composed(n_bits, batch, v, index, s, rows, w, value, tv, arrays, td, out, ws, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(index, v), ptr_array(value, w), ptr_array(arrays, w), ptr_array(out, w));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? write_fused<unit16>(n_bits, batch, v, index, s, rows, w, value, tv, arrays, td, out, ws, U, stream)
                : write_fused<unit8>(n_bits, batch, v, index, s, rows, w, value, tv, arrays, td, out, ws, U, stream);
}

} // namespace csgn
