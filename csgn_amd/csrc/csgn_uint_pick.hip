// csgn_uint_pick.hip -- an encrypted integer shifted, rotated or indexed by an ENCRYPTED amount, every output plane in
// one launch.  Hand-written CDNA4 (gfx950) HIP; the kernel skeleton in csgn_selector.h, design notes in DESIGN.md §4.24.
//
// The definition (include/csgn_hip.h, csgn_uint_pick) is out_j = sum over r < rows_j, ascending, of EQ(index, r) *
// a_{src(j, r)}: csgn_uint_read's sum with the value taken from the element's OWN planes -- plane j - r (SHL), j + r
// (SHR), (j -+ r) mod w (ROTL / ROTR), or plane j of the element's row r (EACH) -- and with the E stream
// (csgn_uint_read.hip's; its index arguments, entry evaluation and tile policy are csgn_selector.h's, for both files)
// cut per output: rows are concatenated ascending, so the stream of rows_j rows is the first E_j entries of the stream
// of rows_max rows.  This file keeps the row key, the source map, the E_j cut and the staging.  A workgroup decodes its
// range of THAT stream once, against rows_max, and output j drops the entries q >= E_j; term q * t + c of output j is
// (entry q) & (term c of the source).  Fresh index planes build the subset tables once per workgroup and spend them,
// and the decoded list of (S, r), on all w outputs; multi-term index planes take the walk and the digits per unit
// (correct, not fast).  The value units are per element: where a workgroup's slice of them fits (32 KB, the whole LDS
// within 64 KB) it is staged in LDS behind the tables and the decoded range, else they are read with plain global loads
// through the source pointers, which the row selects per lane, from a 512-byte LDS copy of the arguments' array.
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>
#include <vector>

namespace csgn {

namespace {

constexpr u64 kStageBytes = 32768;      // of value units a workgroup stages at most
constexpr u64 kLdsTotal = 65536;        // of LDS a workgroup takes at most, the static pointer table included

// By value in the kernel arguments (uniform, scalar loads); the stream is the E stream of rows_max rows, every output has
// the t terms of a source plane.
struct PickArgs {
    SelTile tile;
    SelOutputs<kPickMaxPlanes> outs;
    SelIndex x;
    const void *src[kPickMaxPlanes];
    u32 E[kPickMaxPlanes];      // E_j: output j takes the entries below it
    u32 Emax;
    u32 op, w, n, tsrc;         // n: rows of an element's array (EACH), else 1
    u32 vbase;                  // byte offset of the staged value slice in the LDS (the Stage kernel)
};
static_assert(sizeof(PickArgs) <= 4096, "the kernel arguments of k_uint_pick pass the 4 KiB limit");

// what a row contributes to the source map: r mod w for the rotates (so that the map is one add and one compare per
// unit), r itself for the others
__device__ inline u32 pick_row_key(u32 op, u32 w, u32 r)
{
    return (op == CSGN_UINT_PICK_ROTL || op == CSGN_UINT_PICK_ROTR) ? r % w : r;
}

// Stage (fresh planes only): the workgroup's slice of the value units -- KC units of every term of every source plane
// (and array row) of its G elements -- is copied into LDS once, behind the tables and the decoded range, and every
// written unit reads its value there instead of from global memory.
template <typename Unit, bool Fresh, bool Stage>
__global__ void __launch_bounds__(256) k_uint_pick(PickArgs a)
{
    __shared__ const Unit *srcs[kPickMaxPlanes];
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit>(t, a.Emax);
    const u32 tc = a.tsrc;
    Unit *vals = reinterpret_cast<Unit *>(reinterpret_cast<unsigned char *>(b.tab) + a.vbase);

    if (threadIdx.x < a.w)
        srcs[threadIdx.x] = reinterpret_cast<const Unit *>(a.src[threadIdx.x]);
    if (Stage) {
        // element el, array row rr, plane p, term c, unit kk at (((el * n + rr) * w + p) * t + c) * KC + kk
        const FastDiv dtk = a.outs.tk.at(0);            // t * KC
        const u32 total = b.ne * a.n * a.w * dtk.d;
        for (u32 x = threadIdx.x; x < total; x += 256u) {
            const u32 pr = csgn_fastdiv(x, dtk), rem = x - pr * dtk.d;
            const u32 c = csgn_fastdiv(rem, t.dKC), kk = rem - c * t.KC;
            if (kk >= b.kc)
                continue;
            const u32 row = pr / a.w, p = pr - row * a.w;       // row = el * n + rr
            vals[x] = reinterpret_cast<const Unit *>(a.src[p])[((b.e0 * a.n + row) * tc + c) * t.U + b.k0 + kk];
        }
    }
    if (Fresh) {
        read_decode(a.x, b);
        for (u32 i = threadIdx.x; i < b.nq; i += 256u) {          // the entries this thread has just decoded
            const u32 cd = b.code[i];
            b.code[i] = (cd & 0xFFFFu) | (pick_row_key(a.op, a.w, cd >> 16) << 16);
        }
        subset_build(b.tab, a.x.tabs, a.x.index, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc);
    } else {
        __syncthreads();
    }

    for (u32 j = 0; j < a.outs.nout; ++j) {
        const u32 Ej = a.E[j];
        if (b.q0 >= Ej)
            continue;                   // the whole range lies past this output's prefix (uniform)
        const u64 Tj = (u64)tc * Ej;
        sel_walk<Unit>(t, b, a.outs, j, b.ne, [&](u32 el, u32 qi, u32 c, u32 kk, u64 &at, Unit &v) {
            const u32 k = b.k0 + kk;
            const u64 e = b.e0 + el, q = (u64)b.q0 + qi;
            if (q >= Ej)
                return false;
            u32 r = read_entry<Unit, Fresh>(a.x, t, b, el, e, qi, q, k, kk, v);
            if (!Fresh)
                r = pick_row_key(a.op, a.w, r);         // the decoded list holds the key already
            u32 p = j;                  // the source plane and element (the op is uniform)
            u64 es = e;
            switch (a.op) {
            case CSGN_UINT_PICK_SHL:
                p = j - r;              // r < rows_j <= j + 1
                break;
            case CSGN_UINT_PICK_SHR:
                p = j + r;              // r < rows_j <= w - j
                break;
            case CSGN_UINT_PICK_ROTL:
                p = j >= r ? j - r : j + a.w - r;
                break;
            case CSGN_UINT_PICK_ROTR:
                p = j + r < a.w ? j + r : j + r - a.w;
                break;
            default:
                es = e * a.n + r;
                break;
            }
            if (Stage)
                v &= vals[(((es - b.e0 * a.n) * a.w + p) * tc + c) * t.KC + kk];
            else
                v &= srcs[p][(es * tc + c) * t.U + k];
            at = ((e * Tj) + q * tc + c) * t.U + k;
            return true;
        });
    }
}

// ------------------------------------------------------------------------------ host side

bool pick_is_shift(int op) { return op >= CSGN_UINT_PICK_SHL && op <= CSGN_UINT_PICK_ROTR; }

// rows_j; 0 for an invalid op, width or row count
u64 pick_rows(int op, u64 v, u64 w, u64 rows, u64 j)
{
    if (v < 1 || v > kPickMaxIndex || w < 1 || w > kPickMaxPlanes || j >= w)
        return 0;
    const u64 full = 1ull << v;
    if (pick_is_shift(op) && rows != 0)
        return 0;
    switch (op) {
    case CSGN_UINT_PICK_SHL:
        return std::min(j + 1, full);
    case CSGN_UINT_PICK_SHR:
        return std::min(w - j, full);
    case CSGN_UINT_PICK_ROTL:
    case CSGN_UINT_PICK_ROTR:
        return full;
    case CSGN_UINT_PICK_EACH:
        return rows >= 1 && rows <= full ? rows : 0;
    default:
        return 0;
    }
}

// the output whose stream is the longest: every other is a prefix of it
u64 pick_longest(int op, u64 w) { return op == CSGN_UINT_PICK_SHR ? 0 : w - 1; }

bool pick_shape_ok(int op, u64 v, const u64 *s, u64 w, u64 rows, u64 t)
{
    return t != 0 && t < kTermLimit && w >= 1 && w <= kPickMaxPlanes &&
           uint_pick_terms(op, v, s, w, rows, pick_longest(op, w)) != 0;
}

// The composed form's gather of the rows needs the counts below 2^32 (csgn_gather_planes): past that, the fused form.
bool pick_use_fused(int op, u64 batch, u64 rows)
{
    // by shape: one launch for every output, no shape measured where the composed form is faster
    if (op == CSGN_UINT_PICK_EACH && rows && batch >= ((1ull << 32) + rows - 1) / rows)      // batch * rows >= 2^32
        return true;
    return tune_choose(TUNE_UINT_PICK_FORM, true);
}

// whether the fused form stages its value units in LDS where they fit (knob uint_pick_stage): by shape it does, level
// with the plain loads or faster on every measured shape
bool pick_stage() { return tune_choose(TUNE_UINT_PICK_STAGE, true); }

struct PickShape {
    u64 E[kPickMaxPlanes], Emax, sumE, rows_max;
};

PickShape pick_shape(int op, u64 v, const u64 *s, u64 w, u64 rows)
{
    PickShape p = {};
    for (u64 j = 0; j < w; ++j) {
        p.E[j] = uint_pick_terms(op, v, s, w, rows, j);
        p.sumE += p.E[j];
    }
    p.rows_max = pick_rows(op, v, w, rows, pick_longest(op, w));
    p.Emax = p.E[pick_longest(op, w)];
    return p;
}

template <typename Unit>
hipError_t pick_fused(u64 n_bits, int op, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 w, u64 rows,
                      const u64 *const *src, u64 t, u64 *const *out, const PickShape &ps, u32 U, hipStream_t st)
{
    PickArgs a = {};
    a.op = (u32)op;
    a.w = (u32)w;
    a.n = op == CSGN_UINT_PICK_EACH ? (u32)rows : 1u;
    a.tsrc = (u32)t;
    a.Emax = (u32)ps.Emax;
    const bool fresh = a.x.fill(v, s, ps.rows_max);
    const SubsetPlan sp = ReadTile::plan(fresh, v, U, (u32)sizeof(Unit));
    a.outs.fill(w, [&](u32) { return t; }, false, sp.KC);
    for (u32 j = 0; j < w; ++j)
        a.E[j] = (u32)ps.E[j];
    // the tile over the units an element really writes, sum_j E_j * t * KC
    const ReadTile rt = ReadTile::of(sp, batch, ps.Emax, ps.sumE * t * sp.KC);
    a.tile.set(n_bits, U, sp, rt.QP, ps.Emax, a.outs, rt.G);
    u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.x.tabs) : 0u;
    // the value slice of a workgroup behind the decoded range, where it fits and the knob or the shape asks for it
    const u64 slice = (u64)a.tile.G * a.n * w * t * sp.KC * sizeof(Unit);
    const bool stage = fresh && slice <= kStageBytes &&
                       lds + 16 + slice + kPickMaxPlanes * sizeof(void *) <= kLdsTotal && pick_stage();
    if (stage) {
        a.vbase = (lds + 15u) & ~15u;
        lds = a.vbase + (u32)slice;
    }
    a.tile.xcd = stream_xcd(batch * ps.sumE * t * U);
    return sel_launch(stage ? k_uint_pick<Unit, true, true> : k_uint_pick<Unit, true, false>,
                      k_uint_pick<Unit, false, false>, a, lds, launch_blocks(), batch,
                      (u64)a.tile.chunks * a.tile.qparts, st, [&](u64 e0) {
        a.x.template advance<Unit>(index, e0, U);
        for (u32 j = 0; j < w; ++j) {
            a.src[j] = reinterpret_cast<const Unit *>(src[j]) + e0 * a.n * t * U;
            a.outs.out[j] = reinterpret_cast<Unit *>(out[j]) + e0 * t * ps.E[j] * U;
        }
    });
}

// The composed form, row by row through the tuned launchers: EQ(index, r) by csgn_uint_plain into a temporary, once for
// every output that has row r, then csgn_mul_uniform of it with the source plane into r's slice of output j (pitch
// t * E_j; r's first entry is the same in every output).  EACH puts a csgn_gather_planes of the elements e * n + r in
// front of the multiplies: the list e * n is uploaded once (the call waits for it) and row r gathers from r elements on.
hipError_t pick_composed(u64 n_bits, int op, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 w, u64 rows,
                         const u64 *const *src, u64 t, u64 *const *out, const PickShape &ps, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64;
    const bool each = op == CSGN_UINT_PICK_EACH;
    u64 max_eq = 1;                     // row 0 has the most EQ terms: every R_k = s_k + 1
    for (u64 k = 0; k < v; ++k)
        max_eq *= s[k] + 1;
    const u64 eq_words = batch * max_eq * dL, row_words = each ? batch * t * dL : 0;
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_UINT_PICK, (eq_words + w * row_words + (each ? batch : 0)) * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *eq = block, *idx = block + eq_words + w * row_words;
    u64 *row[kPickMaxPlanes];
    const u64 *from[kPickMaxPlanes];
    u64 tt[kPickMaxPlanes];
    for (u64 j = 0; j < w; ++j) {
        row[j] = block + eq_words + j * row_words;
        tt[j] = t;
    }
    if (each) {
        std::vector<u64> list(batch);
        for (u64 i = 0; i < batch; ++i)
            list[i] = i * rows;
        e = hipMemcpyAsync(idx, list.data(), batch * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);       // the list is the call's own
    }
    u64 off = 0;                        // r's first entry of the E stream
    for (u64 r = 0; r < ps.rows_max && e == hipSuccess; ++r) {
        const u64 er = uint_plain_terms(CSGN_UINT_PLAIN_EQ, v, r, s);
        e = uint_plain(n_bits, CSGN_UINT_PLAIN_EQ, batch, v, r, index, s, eq, st);
        if (each && e == hipSuccess) {
            for (u64 j = 0; j < w; ++j)
                from[j] = src[j] + r * t * dL;
            e = gather_planes(n_bits, w, from, tt, batch * rows - r, batch, idx, row, st);
        }
        for (u64 j = 0; j < w && e == hipSuccess; ++j) {
            if (r >= pick_rows(op, v, w, rows, j))
                continue;
            const u64 *value = row[j];
            switch (op) {
            case CSGN_UINT_PICK_SHL:
                value = src[j - r];
                break;
            case CSGN_UINT_PICK_SHR:
                value = src[j + r];
                break;
            case CSGN_UINT_PICK_ROTL:
                value = src[(j + w - r % w) % w];
                break;
            case CSGN_UINT_PICK_ROTR:
                value = src[(j + r) % w];
                break;
            default:
                break;
            }
            e = mul_uniform(n_bits, batch, er, t, eq, value, out[j] + off * t * dL, 0, st, t * ps.E[j] * dL);
        }
        off += er;
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_pick_terms(int op, u64 v, const u64 *s, u64 w, u64 rows, u64 j)
{
    const u64 rj = pick_rows(op, v, w, rows, j);
    return rj ? uint_read_terms(v, s, rj) : 0;
}

bool uint_pick_rows_offsets(u64 v, const u64 *s, u64 rows, const u64 *T, u64 *src_off, u64 *out_off)
{
    if (!T || !src_off || !out_off || uint_read_terms(v, s, rows) == 0)
        return false;
    u64 so = 0, oo = 0;
    for (u64 r = 0; r < rows; ++r) {
        src_off[r] = so;
        out_off[r] = oo;
        u64 P = 1, block;               // P_r = prod_k (r_k ? s_k : s_k + 1): the terms of EQ(index, r); at most E
        for (u64 k = 0; k < v; ++k)
            P = sat_mul(P, ((r >> k) & 1u) ? s[k] : s[k] + 1);
        if (T[r] == 0 || T[r] >= kTermLimit || !term_mul(P, T[r], block))
            return false;
        so += T[r];
        oo += block;
        if (so >= kTermLimit || oo >= kTermLimit)
            return false;
    }
    src_off[rows] = so;
    out_off[rows] = oo;
    return true;
}

const char *uint_pick_kernel_name(u64 n_bits, int op, u64 batch, u64 v, const u64 *s, u64 w, u64 rows, u64 t)
{
    if (n_bits == 0 || !pick_shape_ok(op, v, s, w, rows, t))
        return "";
    return pick_use_fused(op, batch, rows) ? "k_uint_pick" : "composed";
}

bool uint_pick_plan(u64 n_bits, int op, u64 batch, u64 v, const u64 *s, u64 w, u64 rows, u64 t, bool wide, u64 plan[4])
{
    if (n_bits == 0 || batch == 0 || !pick_shape_ok(op, v, s, w, rows, t))
        return false;
    const u64 dL = (n_bits + 63) / 64;
    wide = wide && dL % 2 == 0;
    const PickShape ps = pick_shape(op, v, s, w, rows);
    const bool fresh = SelIndex().fill(v, s, ps.rows_max);
    const SubsetPlan sp = ReadTile::plan(fresh, v, (u32)(wide ? dL / 2 : dL), wide ? 16u : 8u);
    const ReadTile rt = ReadTile::of(sp, batch, ps.Emax, ps.sumE * t * sp.KC);
    plan[0] = rt.G;
    plan[1] = sp.KC;
    plan[2] = rt.QP;
    plan[3] = (ps.Emax + rt.QP - 1) / rt.QP;
    return true;
}

hipError_t uint_pick(u64 n_bits, int op, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 w, u64 rows,
                     const u64 *const *src, u64 t, u64 *const *out, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    const PickShape ps = pick_shape(op, v, s, w, rows);
    if (!pick_use_fused(op, batch, rows))
        return pick_composed(n_bits, op, batch, v, index, s, w, rows, src, t, out, ps, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(index, v), ptr_array(src, w), ptr_array(out, w));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? pick_fused<unit16>(n_bits, op, batch, v, index, s, w, rows, src, t, out, ps, U, stream)
                : pick_fused<unit8>(n_bits, op, batch, v, index, s, w, rows, src, t, out, ps, U, stream);
}

} // namespace csgn
