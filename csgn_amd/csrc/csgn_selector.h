// csgn_selector.h -- the skeleton of the selector-stream kernels (csgn_uint_read.hip, csgn_uint_find.hip,
// csgn_uint_lt_select.hip, csgn_uint_pick.hip, csgn_uint_pick_rows.hip, csgn_uint_write.hip, csgn_uint_first.hip,
// csgn_uint_nth.hip; csgn_uint_arith.hip takes the tile, the LDS layout, the launches and eq_digits, §4.28).  Internal
// linkage, like csgn_device.h.
//
// An encrypted SELECTOR STREAM (the EQ rows of an index, the EQ of a key row and a query, the terms of lessThan) is the
// left operand of a product with one unit of a value plane, written for every output plane in one launch: term
// q * t_j + c of output j is (entry q of the stream) & (value term c).  A workgroup of 256 threads owns G elements, a
// slice of KC units of every term and QP entries of the stream, for EVERY output; with fresh planes it builds its
// subset tables (csgn_device.h) and decodes its entries into an LDS list once, for all of them.  An operation supplies
// the decode of an entry, the address of the value unit and how it sizes G and QP.  The operations over the E stream
// of an index, k_uint_read, k_uint_pick, k_uint_pick_rows and k_uint_write, share those as well:
// the index in the arguments, the evaluation of an entry in both forms and the tile policy are in the E-stream section
// below, once.
#pragma once

#include "csgn_device.h"

#include <algorithm>

namespace csgn {

namespace {

// The outputs, by value in the kernel arguments: output j has t[j] value terms per entry of the stream.
template <u32 N>
struct SelOutputs {
    void *out[N];
    u32 t[N];
    FastDivTable<N> tk;         // t_j * KC
    u32 nout;

    // Host: n outputs of terms(j) value terms each and, with `bare`, the stream itself as one more output of one term
    // per entry.  Returns the sum of the term counts.
    template <typename Terms>
    u64 fill(u64 n, Terms terms, bool bare, u32 KC)
    {
        nout = (u32)(n + (bare ? 1 : 0));
        u64 sumt = 0;
        for (u32 j = 0; j < nout; ++j) {
            t[j] = j < n ? (u32)terms(j) : 1u;
            tk.set(j, t[j] * KC);
            sumt += t[j];
        }
        return sumt;
    }
};

// The tile of a workgroup, by value in the kernel arguments (uniform, scalar loads): workgroup (element group, unit
// chunk, q part) owns elements [group * G, + G), units [chunk * KC, + KC) of every term and entries [qpart * QP, + QP).
struct SelTile {
    u64 last_mask;
    u64 batch;                  // elements of this launch
    u32 U, KC, G, QP, chunks, qparts, nblocks, xcd;
    u32 base2, lbase;           // byte offsets of the second table set and of the decoded entries in the LDS
    FastDiv dKC, dQP;

    // Host: the plan's unit slices, parts of QP entries of a stream of Q, and groups of G elements.  G, or the larger of
    // G and `rows` (k_uint_find's second tile dimension), is halved until one output's stream of a workgroup, G * rows *
    // QP * max t_j * KC, stays below 2^32 (QP * t_j * KC <= T_j * U < 2^31: G = rows = 1 fits).  Returns the rows left.
    template <u32 N>
    u64 set(u64 n_bits, u32 units, const SubsetPlan &sp, u64 entries, u64 Q, const SelOutputs<N> &outs, u64 elements,
            u64 rows = 1)
    {
        const u64 maxt = *std::max_element(outs.t, outs.t + outs.nout);
        while (elements * rows > 1 && elements * rows * entries * maxt * sp.KC > 0xFFFFFFFFull)
            elements >= rows ? elements /= 2 : rows /= 2;
        last_mask = last_word_mask(n_bits);
        U = units;
        KC = sp.KC;
        chunks = sp.chunks;
        G = (u32)elements;
        QP = (u32)entries;
        qparts = (u32)((Q + entries - 1) / entries);
        dKC = csgn_fastdiv_make(KC);
        dQP = csgn_fastdiv_make(QP);
        return rows;
    }
};

// What blockIdx.x owns of a stream of Q entries, and its LDS: the tables (two sets at most) and the decoded entries.
// Mid (k_uint_find's rows): the block id holds one more level of `mids` parts, between the unit chunk and the q part.
template <typename Unit>
struct SelBlock {
    u64 e0;
    u32 ne, k0, kc, q0, nq, mid;
    Unit *tab, *tab2;
    u32 *code;
};

template <typename Unit, bool Mid = false>
__device__ inline SelBlock<Unit> sel_block(const SelTile &t, u32 Q, u32 mids = 1u)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const u32 bid = t.xcd ? xcd_contiguous_block(blockIdx.x, t.nblocks) : blockIdx.x;
    u32 gc = bid / t.qparts;
    const u32 q0 = (bid - gc * t.qparts) * t.QP, mid = Mid ? gc % mids : 0u;
    if (Mid)
        gc /= mids;
    const u32 group = gc / t.chunks, k0 = (gc - group * t.chunks) * t.KC;
    const u64 e0 = (u64)group * t.G;
    return {e0, (u32)min((u64)t.G, t.batch - e0), k0, min(t.KC, t.U - k0), q0, min(t.QP, Q - q0), mid,
            reinterpret_cast<Unit *>(smem_raw), reinterpret_cast<Unit *>(smem_raw + t.base2),
            reinterpret_cast<u32 *>(smem_raw + t.lbase)};
}

// The walk of output j's stream of a workgroup of `tiles` (its elements, times its rows in k_uint_find) by QP entries:
// lanes take the unit fastest, then the value term, the entry and the tile, so one store instruction writes 64
// consecutive units of one plane.  body(tile, qi, c, kk, at, v) gives unit kk of the slice of value term c of entry qi
// its value v and its place `at` in the output, in units; false where the tile has none (a short last row part).
template <typename Unit, u32 N, typename Body>
__device__ __forceinline__ void sel_walk(const SelTile &t, const SelBlock<Unit> &b, const SelOutputs<N> &outs, u32 j,
                                         u32 tiles, Body body)
{
    const FastDiv dtk = outs.tk.at(j);
    Unit *o = reinterpret_cast<Unit *>(outs.out[j]);
    const u32 len = tiles * t.QP * dtk.d;           // below 2^32 by SelTile::set
    for (u32 l = threadIdx.x; l < len; l += 256u) {
        const u32 en = csgn_fastdiv(l, dtk), rem = l - en * dtk.d;
        const u32 c = csgn_fastdiv(rem, t.dKC), kk = rem - c * t.KC;
        const u32 tile = csgn_fastdiv(en, t.dQP), qi = en - tile * t.QP;
        if (qi >= b.nq || kk >= b.kc)
            continue;
        u64 at;
        Unit v;
        if (body(tile, qi, c, kk, at, v))
            unit_store<Unit, true>(o + at, v);
    }
}

// ------------------------------------------------------------------------------ the EQ of two integers
// Entry `in` of equalTo(left, right) over v planes (k_uint_find's key row against the query, k_uint_arith's a against
// b): its mixed-radix digits with plane 0 slowest, digit < tl_k a term of left plane k, < tl_k + tr_k a term of right
// plane k, else ONE.  term(side, k, i) takes term i of plane k of the left (side 0) or right (side 1) integer; ONE
// takes nothing.  Fresh: every tl_k = tr_k = 1, the digits are base 3.
template <bool Fresh, typename Term>
__device__ __forceinline__ void eq_digits(u32 in, u32 v, const u32 *tl, const u32 *tr, Term term)
{
    for (u32 kb = v; kb-- > 0u;) {
        const u32 uk = Fresh ? 1u : tl[kb], sk = Fresh ? 1u : tr[kb], R = uk + sk + 1u;
        const u32 nx = in / R, dg = in - nx * R;
        in = nx;
        if (dg < uk)
            term(0u, kb, dg);
        else if (dg < uk + sk)
            term(1u, kb, dg - uk);
    }
}

// ------------------------------------------------------------------------------ the E stream of an index
// The concatenation, ascending in r <= last_row, of the EQ rows of an index (csgn_uint_read.hip's term order), decoded
// from the position.  What k_uint_read and k_uint_pick share: the index in the arguments (SelIndex), the walk, the
// fresh decode, the evaluation of one entry in both forms (read_entry) and the tile policy (ReadTile).

// x * y, saturated at kTermLimit
inline u64 sat_mul(u64 x, u64 y)
{
    u64 p;
    return term_mul(x, y, p) ? p : kTermLimit;
}

// The index of an E stream, by value in the kernel arguments (uniform, scalar loads).
struct SelIndex {
    const void *index[kReadMaxIndex];
    u64 F[kReadMaxIndex];       // prod over i < k of (2 s_i + 1): a whole subtree below bit k (saturated; read only
                                // where the subtree lies below the rows, so at most E)
    u32 s[kReadMaxIndex];
    u32 last_row, v;
    SubsetTables tabs;

    // Host: nv planes of terms[k] terms under `rows` rows.  Returns whether every plane is fresh.
    bool fill(u64 nv, const u64 *terms, u64 rows)
    {
        v = (u32)nv;
        last_row = (u32)(rows - 1);
        bool fresh = true;
        u64 f = 1;
        for (u32 k = 0; k < v; ++k) {
            s[k] = (u32)terms[k];
            F[k] = f;
            f = sat_mul(f, 2 * terms[k] + 1);
            fresh = fresh && terms[k] == 1;
        }
        return fresh;
    }

    // Host: the planes of a launch that begins at element e0
    template <typename Unit>
    void advance(const u64 *const *planes, u64 e0, u32 U)
    {
        for (u32 k = 0; k < v; ++k)
            index[k] = reinterpret_cast<const Unit *>(planes[k]) + e0 * s[k] * U;
    }
};
static_assert(kReadMaxIndex == kPickMaxIndex, "k_uint_read and k_uint_pick share SelIndex");

// q < E: the row r holding entry q of the E stream, and q's index inside r's block (the walk)
__device__ inline u32 read_walk(const SelIndex &x, u64 q, u64 &in)
{
    u32 r = 0;
    u64 H = 1;                  // prod of R_k over the bits fixed so far
    bool tight = true;          // the prefix equals that of rows - 1
    for (u32 k = x.v; k-- > 0u;) {
        const u64 s = x.s[k];
        if (tight && !((x.last_row >> k) & 1u)) {
            H *= s + 1u;
            continue;
        }
        const u64 c0 = H * (s + 1u) * x.F[k];
        if (q < c0) {
            H *= s + 1u;
            tight = false;
        } else {
            q -= c0;
            r |= 1u << k;
            H *= s;
        }
    }
    in = q;
    return r;
}

// Fresh planes: the workgroup's range of the E stream into its LDS list, S in the low 16 bits, r in the high 16
// (published by the tables' closing barrier)
template <typename Unit>
__device__ inline void read_decode(const SelIndex &x, const SelBlock<Unit> &b)
{
    for (u32 i = threadIdx.x; i < b.nq; i += 256u) {
        u64 in;
        const u32 r = read_walk(x, b.q0 + i, in);
        u32 S = r;
        for (u32 k = x.v; k-- > 0u;) {      // zero bits, the highest the fastest binary digit; digit 0 = x_k
            if ((r >> k) & 1u)
                continue;
            if (!(in & 1u))
                S |= 1u << k;
            in >>= 1;
        }
        b.code[i] = S | (r << 16);
    }
}

// Entry q = b.q0 + qi of the E stream at unit k = b.k0 + kk of element e = b.e0 + el: into v the selector unit, and
// returns the row.  Fresh: P[S] from the tables, S and the row from the LDS list (the high 16 bits as the operation
// left them there).  Else the walk, then the digits of q inside the row's block: mixed radix over R_k = r_k ? s_k :
// s_k + 1 with k = 0 slowest; digit s_k (a zero bit only) selects ONE, any other digit that term of x_k.
template <typename Unit, bool Fresh>
__device__ __forceinline__ u32 read_entry(const SelIndex &x, const SelTile &t, const SelBlock<Unit> &b, u32 el, u64 e,
                                          u32 qi, u64 q, u32 k, u32 kk, Unit &v)
{
    if (Fresh) {
        const u32 cd = b.code[qi];
        v = subset_and(b.tab, x.tabs, el, cd & 0xFFFFu, t.KC, kk);
        return cd >> 16;
    }
    u64 in;
    const u32 r = read_walk(x, q, in);
    v = one_unit(Unit(), k, t.U, t.last_mask);
    for (u32 kb = x.v; kb-- > 0u;) {
        const u64 s = x.s[kb], R = ((r >> kb) & 1u) ? s : s + 1u;
        const u64 dg = in % R;
        in /= R;
        if (dg < s)
            v &= reinterpret_cast<const Unit *>(x.index[kb])[(e * s + dg) * t.U + k];
    }
    return r;
}

// ------------------------------------------------------------------------------ host side

// The tile of the E-stream operations over a stream of E entries of which an element writes elem_units units (one
// KC slice of every term of every output): G elements, `parts` parts of QP entries.
struct ReadTile {
    static constexpr u64 kLdsBudget = 32768;    // bytes of subset tables per workgroup
    static constexpr u32 kMaxRange = 2048;      // E-stream entries one workgroup decodes (8 KB of LDS)
    static constexpr u64 kPartUnits = 8192;     // units a workgroup writes at least, where the shape has them
    u64 G, QP, parts;

    // the tables and unit slices of v index planes at U units of unit_bytes
    static SubsetPlan plan(bool fresh, u64 v, u32 U, u32 unit_bytes)
    {
        return subset_plan(fresh ? (u32)v : 0, U, unit_bytes, kLdsBudget);
    }

    static ReadTile of(const SubsetPlan &sp, u64 batch, u64 E, u64 elem_units)
    {
        // elements per workgroup: enough to give it kPartUnits to write, as many as the tables allow
        u64 G = std::max<u64>(1, kPartUnits / elem_units);
        G = std::min<u64>({G, sp.max_G, batch, 64});
        G = std::max<u64>(G, 1);
        // parts of the E stream: each writes kPartUnits or four times its table build, and decodes at most kMaxRange
        const u64 build = G * sp.entries * sp.KC;
        const u64 target = std::max<u64>(kPartUnits, 4 * build);
        u64 parts = std::max<u64>(1, G * elem_units / target);
        parts = std::max<u64>(parts, (E + kMaxRange - 1) / kMaxRange);
        parts = std::min<u64>(parts, E);
        return {G, (E + parts - 1) / parts, parts};
    }
};

// The LDS of fresh planes: the tables of G elements (their layout into `first`), then, with G2, a second set for G2
// elements (into `second`), then the QP decoded entries.  Sets the tile's offsets; returns the bytes.
inline u32 sel_lds_layout(SelTile &t, SubsetPlan sp, SubsetTables &first, u32 G2 = 0, SubsetTables *second = nullptr)
{
    t.base2 = t.lbase = (sp.layout(t.G) + 15u) & ~15u;
    first = sp.t;
    if (G2) {
        t.lbase = (t.base2 + sp.layout(G2) + 15u) & ~15u;
        *second = sp.t;
    }
    return t.lbase + t.QP * 4u;
}

// The launches of per_group workgroups for every G elements of the batch: offset(e0) points the arguments at element
// e0, then the Fresh kernel runs with `lds` bytes (sel_lds_layout; 0: planes of several terms) or the other with none.
template <typename Args, typename Offset>
inline hipError_t sel_launch(void (*fresh)(Args), void (*multi)(Args), Args &a, u32 lds, u64 max_blocks, u64 batch,
                             u64 per_group, hipStream_t st, Offset offset)
{
    return launch_groups(max_blocks, batch, a.tile.G, per_group, [&](u64 e0, u64 ne, u32 nblocks) {
        a.tile.batch = ne;
        a.tile.nblocks = nblocks;
        offset(e0);
        if (lds)
            fresh<<<dim3(nblocks), 256, lds, st>>>(a);
        else
            multi<<<dim3(nblocks), 256, 0, st>>>(a);
    });
}

} // namespace

} // namespace csgn
