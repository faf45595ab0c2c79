// csgn_uint_read.hip -- an ENCRYPTED table read at an ENCRYPTED index, every output plane in one launch.
// Hand-written CDNA4 (gfx950) HIP; the kernel skeleton in csgn_selector.h, design notes in DESIGN.md §4.17.
//
// The definition (include/csgn_hip.h, csgn_uint_read) is out_j = sum over r < rows, ascending, of EQ(x, r) * d_{r,j}:
// csgn_uint_plain's EQ row with k = r as the left operand, plane j of table element r as the right.  Term q * t_j + c of
// output j is (term q of the E stream) & (term c of d_{r,j}), where the E stream is the concatenation, ascending in r,
// of the EQ rows.  Nothing of it is tabulated: q is decoded (csgn_selector.h's E-stream section, which holds the index
// arguments, the evaluation of an entry in both forms and the tile policy for this file and csgn_uint_pick.hip) by
//     the walk    from the top index bit down: below a fixed prefix of high bits a whole subtree holds
//                 prod (2 s_k + 1) terms over its free bits, times the R_k of the bits already fixed, so each step
//                 either skips the bit-0 subtree (bit 1) or enters it; while the prefix equals that of rows - 1 and
//                 that bit is 0 there is only the bit-0 subtree
//     the digits  inside row r's block: mixed radix over R_k = r_k ? s_k : s_k + 1 with k = 0 slowest; digit s_k (a
//                 zero bit only) selects ONE, any other digit that term of x_k
//
// Fresh index planes (every s_k = 1), the case this kernel is built for: a term of the E stream is P[S], the AND of x_k
// over S = ones(r) + the zero bits whose digit is 0.  A workgroup owns G elements, a slice of KC units of every term,
// and one range of the E stream, for EVERY output plane: it builds the subset tables of §4.15 (csgn_device.h: one to
// three, the AND of every subset of their planes) for its elements in LDS, decodes its range once into an LDS list of
// (S, r), and every written unit is then 1-3 LDS reads ANDed with one unit of the table row -- a row every element
// reads, so it hits in L2.  The table build and the decode are spent on all `w` outputs.  Multi-term index planes take
// the walk and the digits per unit straight from the planes (correct, not fast).  This file keeps the table address,
// the outputs' term counts and the composed form.
#include "csgn_hip.h"
#include "csgn_selector.h"

namespace csgn {

namespace {

// By value in the kernel arguments (uniform, scalar loads); the stream is the E stream of index x, output j has the terms
// of table plane j.
struct ReadArgs {
    SelTile tile;
    SelOutputs<kReadMaxPlanes> outs;
    SelIndex x;
    const void *table[kReadMaxPlanes];
    u32 E;
};
static_assert(sizeof(ReadArgs) <= 4096, "the kernel arguments of k_uint_read pass the 4 KiB limit");

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_read(ReadArgs a)
{
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit>(t, a.E);

    if (Fresh) {
        read_decode(a.x, b);
        subset_build(b.tab, a.x.tabs, a.x.index, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc);
    }

    for (u32 j = 0; j < a.outs.nout; ++j) {
        const u32 tj = a.outs.t[j];
        const u64 Tj = (u64)tj * a.E;
        const Unit *d = reinterpret_cast<const Unit *>(a.table[j]);
        sel_walk<Unit>(t, b, a.outs, j, b.ne, [&](u32 el, u32 qi, u32 c, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk;
            const u64 e = b.e0 + el, q = (u64)b.q0 + qi;
            const u32 r = read_entry<Unit, Fresh>(a.x, t, b, el, e, qi, q, k, kk, v);
            v &= d[((u64)r * tj + c) * t.U + k];
            at = ((e * Tj) + q * tj + c) * t.U + k;
            return true;
        });
    }
}

// ------------------------------------------------------------------------------ host side

bool read_shape_ok(u64 v, const u64 *s, u64 rows, u64 w, const u64 *t)
{
    if (w < 1 || w > kReadMaxPlanes || !t || uint_read_terms(v, s, rows) == 0)
        return false;
    for (u64 j = 0; j < w; ++j)
        if (t[j] == 0 || t[j] >= kTermLimit)
            return false;
    return true;
}

bool read_use_fused()
{
    // by shape: one launch for every output, no shape measured where the composed form is faster
    return tune_choose(TUNE_UINT_READ_FUSED, true);
}

template <typename Unit>
hipError_t read_fused(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                      const u64 *const *table, const u64 *t, u64 *const *out, u64 E, u32 U, hipStream_t st)
{
    ReadArgs a = {};
    a.E = (u32)E;
    const bool fresh = a.x.fill(v, s, rows);
    const SubsetPlan sp = ReadTile::plan(fresh, v, U, (u32)sizeof(Unit));
    const u64 sumt = a.outs.fill(w, [&](u32 j) { return t[j]; }, false, sp.KC);
    const ReadTile rt = ReadTile::of(sp, batch, E, E * sumt * sp.KC);
    a.tile.set(n_bits, U, sp, rt.QP, E, a.outs, rt.G);
    const u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.x.tabs) : 0u;
    a.tile.xcd = stream_xcd(batch * E * sumt * U);
    for (u32 j = 0; j < w; ++j)
        a.table[j] = table[j];
    return sel_launch(k_uint_read<Unit, true>, k_uint_read<Unit, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        a.x.template advance<Unit>(index, e0, U);
        for (u32 j = 0; j < w; ++j)
            a.outs.out[j] = reinterpret_cast<Unit *>(out[j]) + e0 * t[j] * E * U;
    });
}

// The composed form, row by row through the tuned launchers: EQ(x, r) by csgn_uint_plain into a temporary, row r of
// every table plane broadcast to the batch by one csgn_gather_planes (tile form), then csgn_mul_uniform of the two into
// r's slice of every output (pitch T_j).  The temporaries live in one temporary block (scratch_take,
// csgn_kernels.h), apart from the one csgn_uint_plain's composed form may take for EQ.
hipError_t read_composed(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                         const u64 *const *table, const u64 *t, u64 *const *out, u64 E, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64;
    u64 max_eq = 1, sumt = 0;           // row 0 has the most EQ terms: every R_k = s_k + 1
    for (u64 k = 0; k < v; ++k)
        max_eq *= s[k] + 1;
    for (u64 j = 0; j < w; ++j)
        sumt += t[j];
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_UINT_READ, batch * (max_eq + sumt) * dL * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *eq = block;
    const u64 *src[kReadMaxPlanes];
    u64 *row[kReadMaxPlanes];
    u64 at = batch * max_eq * dL;
    for (u64 j = 0; j < w; ++j) {
        row[j] = block + at;
        at += batch * t[j] * dL;
    }
    u64 off = 0;                        // r's first entry of the E stream
    for (u64 r = 0; r < rows && e == hipSuccess; ++r) {
        const u64 er = uint_plain_terms(CSGN_UINT_PLAIN_EQ, v, r, s);
        e = uint_plain(n_bits, CSGN_UINT_PLAIN_EQ, batch, v, r, index, s, eq, st);
        for (u64 j = 0; j < w; ++j)
            src[j] = table[j] + r * t[j] * dL;
        if (e == hipSuccess)
            e = gather_planes(n_bits, w, src, t, 1, batch, nullptr, row, st);
        for (u64 j = 0; j < w && e == hipSuccess; ++j)
            e = mul_uniform(n_bits, batch, er, t[j], eq, row[j], out[j] + off * t[j] * dL, 0, st, t[j] * E * dL);
        off += er;
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_read_terms(u64 v, const u64 *s, u64 rows)
{
    if (v < 1 || v > kReadMaxIndex || !s || rows < 1 || rows > (1ull << v))
        return 0;
    for (u64 k = 0; k < v; ++k)
        if (s[k] == 0 || s[k] >= kTermLimit)
            return 0;
    // the walk along rows - 1: every bit-0 subtree left of the path is whole, then the row rows - 1 itself
    const u64 last = rows - 1;
    u64 F[kReadMaxIndex], f = 1;
    for (u64 k = 0; k < v; ++k) {
        F[k] = f;
        f = sat_mul(f, 2 * s[k] + 1);
    }
    u64 E = 0, H = 1;
    for (u64 k = v; k-- > 0;) {
        if ((last >> k) & 1u) {
            E += sat_mul(sat_mul(H, s[k] + 1), F[k]);
            H = sat_mul(H, s[k]);
        } else {
            H = sat_mul(H, s[k] + 1);
        }
        if (E >= kTermLimit)
            return 0;
    }
    E += H;
    return E >= kTermLimit ? 0 : E;
}

const char *uint_read_kernel_name(u64 n_bits, u64 batch, u64 v, const u64 *s, u64 rows, u64 w, const u64 *t)
{
    (void)batch;
    if (n_bits == 0 || !read_shape_ok(v, s, rows, w, t))
        return "";
    return read_use_fused() ? "k_uint_read" : "composed";
}

hipError_t uint_read(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 rows, u64 w,
                     const u64 *const *table, const u64 *t, u64 *const *out, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    const u64 E = uint_read_terms(v, s, rows);
    if (!read_use_fused())
        return read_composed(n_bits, batch, v, index, s, rows, w, table, t, out, E, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(index, v), ptr_array(table, w), ptr_array(out, w));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? read_fused<unit16>(n_bits, batch, v, index, s, rows, w, table, t, out, E, U, stream)
                : read_fused<unit8>(n_bits, batch, v, index, s, rows, w, table, t, out, E, U, stream);
}

} // namespace csgn
