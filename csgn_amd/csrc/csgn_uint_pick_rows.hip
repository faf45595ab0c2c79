// csgn_uint_pick_rows.hip -- ENCRYPTED arrays whose rows differ in size read at ENCRYPTED indices, every output plane in
// one launch: the read that follows csgn_uint_write.  Hand-written CDNA4 (gfx950) HIP; the kernel skeleton in
// csgn_selector.h, design notes in DESIGN.md §4.30.
//
// The definition (include/csgn_hip.h, csgn_uint_pick_rows): row r of plane j has T_j[r] terms in every array, an array
// A_j = sum_r T_j[r]; output j is uniform with Tout_j = sum_r P_r * T_j[r] terms per element, row r's block begins at
// out_off_j[r] and its term in * T_j[r] + c is (entry `in` of EQ(x, r)) & (term c of row r of array e).  The EQ entries of
// row r are the entries [qstart(r), qstart(r) + P_r) of the E stream of n rows (csgn_uint_read.hip's; the index
// arguments, the evaluation of an entry and the tile policy are csgn_selector.h's, as for k_uint_read, k_uint_pick and
// k_uint_write).  A workgroup owns G elements, a slice of KC units of every term and one range of the E stream, for EVERY
// output plane; it builds the subset tables and decodes its range once (fresh index planes).  A range of the E stream is a
// contiguous run of rows, so its part of output j is ONE contiguous span of terms: the lanes walk the span flat, the unit
// fastest, and a position finds its row by a binary search over the rows of the range in a device table of 24-byte
// records (PickRow), then (in, c) by one division by the row's T.  Planes with equal rows share one table; the tables
// live in a per-thread cache keyed by the shape, so a repeated call uploads nothing and can be captured into a graph.
// The search and the division are pick_rows_locate / pick_rows_range below, __host__ __device__: the host runs the same
// code over every launch's every workgroup range before the first launch is issued (rows_launch_ok), and
// csgn_uint_pick_rows_decode runs it for one position.  This file keeps the records, the walk, the bounds, the cache and
// the composed form.
#include "csgn_hip.h"
#include "csgn_selector.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

namespace csgn {

namespace {

// One row of one table: T with its FastDiv, the row's first entry of the E stream, its first term inside an array and its
// block's first term inside an output element.  Every count is below 2^32 (the entry points refuse 2^31 words per element).
struct PickRow {
    FastDiv T;
    u32 qstart, src_off, out_off;
};
static_assert(sizeof(PickRow) == 24, "a record is six dwords");

// Entry q of the E stream of n rows: its row (the last whose qstart is at or below q) and q's index inside the row's block.
__host__ __device__ inline u32 pick_rows_row_of(const PickRow *rows, u32 n, u32 q, u32 &in)
{
    u32 lo = 0, hi = n - 1u;
    while (lo < hi) {
        const u32 mid = (lo + hi + 1u) >> 1;
        if (rows[mid].qstart <= q)
            lo = mid;
        else
            hi = mid - 1u;
    }
    in = q - rows[lo].qstart;
    return lo;
}

// Position p of an output whose rows lo..hi hold it (out_off[lo] <= p < out_off[hi + 1]): the row, into `rec` its record,
// and p - out_off[r] = in * T[r] + c.
__host__ __device__ inline u32 pick_rows_locate(const PickRow *rows, u32 lo, u32 hi, u32 p, PickRow &rec, u32 &in, u32 &c)
{
    while (lo < hi) {
        const u32 mid = (lo + hi + 1u) >> 1;
        if (rows[mid].out_off <= p)
            lo = mid;
        else
            hi = mid - 1u;
    }
    rec = rows[lo];
    const u32 rel = p - rec.out_off;
    in = csgn_fastdiv(rel, rec.T);
    c = rel - in * rec.T.d;
    return lo;
}

// The span [p0, p1) of an output that the entries [q0, q0 + nq) of the E stream write: from term 0 of the first entry to
// the last term of the last one.  Rows rlo..rhi with in0 / in1 from pick_rows_row_of(q0) / (q0 + nq - 1).
__host__ __device__ inline void pick_rows_span(const PickRow *rows, u32 rlo, u32 in0, u32 rhi, u32 in1, u32 &p0, u32 &p1)
{
    p0 = rows[rlo].out_off + in0 * rows[rlo].T.d;
    p1 = rows[rhi].out_off + (in1 + 1u) * rows[rhi].T.d;
}

// By value in the kernel arguments (uniform, scalar loads); the stream is the E stream of n rows.
struct PickRowsArgs {
    SelTile tile;
    SelIndex x;
    void *out[kPickMaxPlanes];
    const void *src[kPickMaxPlanes];
    const PickRow *rows[kPickMaxPlanes];        // plane j's table; equal tables are one
    u32 A[kPickMaxPlanes], Tout[kPickMaxPlanes];
    u32 E, n, w;
};
static_assert(sizeof(PickRowsArgs) <= 4096, "the kernel arguments of k_uint_pick_rows pass the 4 KiB limit");

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_pick_rows(PickRowsArgs a)
{
    const SelTile &t = a.tile;
    const SelBlock<Unit> b = sel_block<Unit>(t, a.E);

    if (Fresh) {
        read_decode(a.x, b);
        subset_build(b.tab, a.x.tabs, a.x.index, t.G, t.KC, t.dKC, t.U, t.last_mask, b.e0, b.ne, b.k0, b.kc);
    }

    // the rows of the range (uniform; qstart is the index's, the same in every table)
    u32 in0, in1;
    const u32 rlo = pick_rows_row_of(a.rows[0], a.n, b.q0, in0);
    const u32 rhi = pick_rows_row_of(a.rows[0], a.n, b.q0 + b.nq - 1u, in1);

    for (u32 j = 0; j < a.w; ++j) {
        const PickRow *rows = a.rows[j];
        const Unit *src = reinterpret_cast<const Unit *>(a.src[j]);
        Unit *o = reinterpret_cast<Unit *>(a.out[j]);
        const u64 Aj = a.A[j], Tj = a.Tout[j];
        u32 p0, p1;
        pick_rows_span(rows, rlo, in0, rhi, in1, p0, p1);
        const u32 span = (p1 - p0) * t.KC;              // units of one element's span at this slice
        const FastDiv dsp = csgn_fastdiv_make(span);
        const u32 len = b.ne * span;                    // below 2^32 by the host's tile (rows_tile)
        // The walk's bounds, each enforced on the host for every launch before it is issued (rows_launch_ok):
        //   p < Tout_j            p < p1, and p1 <= out_off_j[rhi + 1] <= Tout_j
        //   src_off[r] + c < A_j  c < T_j[r], and src_off_j[r] + T_j[r] = src_off_j[r + 1] <= A_j
        //   e < ne of the launch  el < b.ne = min(G, t.batch - b.e0), t.batch the launch's elements
        for (u32 l = threadIdx.x; l < len; l += 256u) {
            const u32 el = csgn_fastdiv(l, dsp), rem = l - el * span;
            const u32 pp = csgn_fastdiv(rem, t.dKC), kk = rem - pp * t.KC;
            if (kk >= b.kc)
                continue;
            const u32 p = p0 + pp, k = b.k0 + kk;
            const u64 e = b.e0 + el;
            PickRow rec;
            u32 in, c;
            pick_rows_locate(rows, rlo, rhi, p, rec, in, c);
            const u32 q = rec.qstart + in;              // b.q0 <= q < b.q0 + b.nq: p lies inside the span
            Unit v;
            read_entry<Unit, Fresh>(a.x, t, b, el, e, q - b.q0, q, k, kk, v);
            v &= src[(e * Aj + rec.src_off + c) * t.U + k];
            unit_store<Unit, true>(o + (e * Tj + p) * t.U + k, v);
        }
    }
}

// The composed form's copy of row r: `batch` rows of `words` words each, the source at a pitch, the copy dense.
__global__ void __launch_bounds__(256) k_pick_rows_copy(const u64 *__restrict__ src, u64 pitch, u64 words, u64 total,
                                                        u64 *__restrict__ dst)
{
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < total; i += (u64)gridDim.x * 256u) {
        const u64 e = i / words;
        dst[i] = src[e * pitch + (i - e * words)];
    }
}

// ------------------------------------------------------------------------------ the tables

// One table: the rows of a plane under an index, on the host and (once a launch needs it) on the device.
struct RowsTable {
    std::vector<u64> key;               // v, s_0..s_{v-1}, n, T_0..T_{n-1}
    std::vector<PickRow> rows;
    u64 A = 0, Tout = 0, E = 0;
    bool fits = false;                  // every count below 2^32: the records hold it
    PickRow *dev = nullptr;
    int device = -1;
    bool captured = false;              // dev was handed to a launch on a capturing stream: a graph may hold it
};

// The calling thread's tables, the most recently used last.  A table that leaves takes its device copy with it (hipFree
// waits for the launches that read it) -- unless a capturing stream has seen the copy: a graph may then hold it, and it is
// retired, to be freed when the thread ends (csgn_scratch.cpp's rule for its blocks).  At thread or process exit the
// copies, kept and retired, go the way csgn_scratch.cpp's blocks do.
constexpr size_t kRowsTables = 2 * kPickMaxPlanes;
struct RowsCache {
    std::vector<std::unique_ptr<RowsTable>> v;
    std::vector<PickRow *> retired;
    u64 freed = 0;
    void drop(RowsTable &t)             // t's device copy leaves: the table does, or the device has changed
    {
        if (!t.dev)
            return;
        if (t.captured) {
            retired.push_back(t.dev);
        } else {
            (void)hipFree(t.dev);
            ++freed;
        }
        t.dev = nullptr;
        t.captured = false;
    }
    ~RowsCache()
    {
        for (auto &t : v)
            if (t->dev)
                (void)hipFree(t->dev);
        for (PickRow *p : retired)
            (void)hipFree(p);
    }
};
thread_local RowsCache g_rows;

// The table of (v, s, n, T), built on first use; nullptr for a shape csgn_uint_pick_rows_offsets refuses.  Host only.
RowsTable *rows_table(u64 v, const u64 *s, u64 n, const u64 *T)
{
    if (!s || !T || v < 1 || v > kPickMaxIndex || n < 1 || n > (1ull << v))
        return nullptr;
    auto &list = g_rows.v;
    for (size_t i = list.size(); i-- > 0;) {
        const std::vector<u64> &k = list[i]->key;
        if (k.size() == v + n + 2 && k[0] == v && k[v + 1] == n && memcmp(&k[1], s, v * 8) == 0 &&
            memcmp(&k[v + 2], T, n * 8) == 0) {
            if (i + 1 != list.size())
                std::rotate(list.begin() + i, list.begin() + i + 1, list.end());
            return list.back().get();
        }
    }
    std::vector<u64> so(n + 1), oo(n + 1);
    if (!uint_pick_rows_offsets(v, s, n, T, so.data(), oo.data()))
        return nullptr;
    std::unique_ptr<RowsTable> t(new RowsTable());
    t->key.reserve(v + n + 2);
    t->key.push_back(v);
    t->key.insert(t->key.end(), s, s + v);
    t->key.push_back(n);
    t->key.insert(t->key.end(), T, T + n);
    t->A = so[n];
    t->Tout = oo[n];
    t->E = uint_read_terms(v, s, n);
    t->fits = t->A < (1ull << 32) && t->Tout < (1ull << 32);       // E <= Tout, every T[r] <= A
    if (t->fits) {
        t->rows.resize(n);
        u64 q = 0;
        for (u64 r = 0; r < n; ++r) {
            t->rows[r] = PickRow{csgn_fastdiv_make((u32)T[r]), (u32)q, (u32)so[r], (u32)oo[r]};
            q += (oo[r + 1] - oo[r]) / T[r];                        // P_r
        }
    }
    if (list.size() >= kRowsTables) {
        g_rows.drop(*list.front());
        list.erase(list.begin());
    }
    list.push_back(std::move(t));
    return list.back().get();
}

// the table's device copy on the current device; uploaded (synchronously) on first use, which a capturing stream refuses.
// A copy that a capturing stream uses is marked (RowsCache::drop).
hipError_t rows_upload(RowsTable &t, hipStream_t st)
{
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess)
        return e;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    if (t.dev && t.device == device) {
        t.captured = t.captured || capturing;
        return hipSuccess;
    }
    if (capturing)
        return hipErrorStreamCaptureUnsupported;
    g_rows.drop(t);
    if ((e = hipMalloc(reinterpret_cast<void **>(&t.dev), t.rows.size() * sizeof(PickRow))) != hipSuccess)
        return e;
    t.device = device;
    e = hipMemcpy(t.dev, t.rows.data(), t.rows.size() * sizeof(PickRow), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        g_rows.drop(t);
    return e;
}

// ------------------------------------------------------------------------------ host side

// The planes of a call: plane j's table, the tables' distinct ones first seen.
struct RowsShape {
    RowsTable *table[kPickMaxPlanes];
    std::vector<RowsTable *> distinct;
    u64 E = 0, sumT = 0, sumA = 0;
};

// false for a shape the entry points refuse as invalid.  The tables stay valid for the call: a call has at most
// kPickMaxPlanes of them and the cache keeps twice that.
bool rows_shape(u64 v, const u64 *s, u64 n, u64 w, const u64 *T, RowsShape &rs)
{
    if (w < 1 || w > kPickMaxPlanes || !T)
        return false;
    for (u64 j = 0; j < w; ++j) {
        RowsTable *t = nullptr;
        for (u64 i = 0; i < j && !t; ++i)
            if (memcmp(T + i * n, T + j * n, n * 8) == 0)
                t = rs.table[i];
        if (!t) {
            t = rows_table(v, s, n, T + j * n);
            if (!t)
                return false;
            rs.distinct.push_back(t);
        }
        rs.table[j] = t;
        rs.sumT += t->Tout;
        rs.sumA += t->A;
        if (rs.sumT >= kTermLimit || rs.sumA >= kTermLimit)
            return false;
    }
    rs.E = rs.table[0]->E;
    return true;
}

bool rows_use_fused()
{
    // by shape: one launch for every output, no shape measured where the composed form is faster
    return tune_choose(TUNE_UINT_PICK_ROWS_FORM, true);
}

// The tile: ReadTile's over the units an element really writes, G halved until the longest span of a workgroup,
// G * (p1 - p0) * KC, stays below 2^32 (one element's is below 2^31: Tout_j * U < 2^31).
ReadTile rows_tile(const SubsetPlan &sp, u64 batch, const RowsShape &rs)
{
    ReadTile rt = ReadTile::of(sp, batch, rs.E, rs.sumT * sp.KC);
    u64 longest = 0;
    const u32 n = (u32)rs.table[0]->rows.size();
    for (u64 part = 0; part < rt.parts; ++part) {
        const u64 q0 = part * rt.QP;
        if (q0 >= rs.E)
            break;
        const u32 nq = (u32)std::min<u64>(rt.QP, rs.E - q0);
        u32 in0, in1, p0, p1;
        const u32 rlo = pick_rows_row_of(rs.table[0]->rows.data(), n, (u32)q0, in0);
        const u32 rhi = pick_rows_row_of(rs.table[0]->rows.data(), n, (u32)q0 + nq - 1u, in1);
        for (RowsTable *t : rs.distinct) {
            pick_rows_span(t->rows.data(), rlo, in0, rhi, in1, p0, p1);
            longest = std::max<u64>(longest, p1 - p0);
        }
    }
    while (rt.G > 1 && rt.G * longest * sp.KC > 0xFFFFFFFFull)
        rt.G /= 2;
    return rt;
}

// What one launch of the host's split does, proven on the host before any launch is issued: every workgroup of the launch
// has elements (e < ne), and every range of the E stream walks positions p < Tout_j whose source terms lie inside the
// array, src_off[r] + c < A_j -- by the kernel's own search and division at both ends of every span.
bool rows_launch_ok(const SelTile &tile, const RowsShape &rs, u64 batch, u64 e0, u64 ne, u32 nblocks)
{
    const u64 per_group = (u64)tile.chunks * tile.qparts, groups = (ne + tile.G - 1) / tile.G;
    if (ne == 0 || e0 >= batch || ne > batch - e0 || e0 % tile.G != 0 || nblocks != groups * per_group)
        return false;                   // a workgroup's group g < groups: its e0 = g * G < ne, so 1 <= b.ne and e < ne
    if ((u64)tile.qparts * tile.QP < rs.E || (u64)(tile.qparts - 1u) * tile.QP >= rs.E)
        return false;                   // the q parts cover the stream, and none is empty
    const u32 n = (u32)rs.table[0]->rows.size();
    for (u32 part = 0; part < tile.qparts; ++part) {
        const u32 q0 = part * tile.QP, nq = (u32)std::min<u64>(tile.QP, rs.E - q0);
        u32 in0, in1, p0, p1, in, c;
        const PickRow *first = rs.table[0]->rows.data();
        const u32 rlo = pick_rows_row_of(first, n, q0, in0), rhi = pick_rows_row_of(first, n, q0 + nq - 1u, in1);
        for (RowsTable *t : rs.distinct) {
            const PickRow *rows = t->rows.data();
            PickRow rec;
            pick_rows_span(rows, rlo, in0, rhi, in1, p0, p1);
            if (p0 >= p1 || p1 > t->Tout || std::min<u64>(tile.G, ne) * (p1 - p0) * tile.KC > 0xFFFFFFFFull)
                return false;           // the span is inside the output, and a workgroup's walk of it below 2^32
            // the first position: term 0 of entry q0; the last: the last term of entry q0 + nq - 1
            if (pick_rows_locate(rows, rlo, rhi, p0, rec, in, c) != rlo || in != in0 || c != 0 ||
                rec.qstart + in != q0 || (u64)rec.src_off + c >= t->A)
                return false;
            if (pick_rows_locate(rows, rlo, rhi, p1 - 1u, rec, in, c) != rhi || in != in1 || c != rec.T.d - 1u ||
                rec.qstart + in != q0 + nq - 1u || (u64)rec.src_off + c >= t->A)
                return false;
            // every row between them keeps its terms inside the array
            for (u32 r = rlo; r <= rhi; ++r)
                if ((u64)rows[r].src_off + rows[r].T.d > t->A)
                    return false;
        }
    }
    return true;
}

template <typename Unit>
hipError_t rows_fused(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 n, u64 w,
                      const u64 *const *arrays, u64 *const *out, const RowsShape &rs, u32 U, hipStream_t st)
{
    for (RowsTable *t : rs.distinct) {
        if (!t->fits)
            return hipErrorInvalidValue;
        const hipError_t e = rows_upload(*t, st);
        if (e != hipSuccess)
            return e;
    }
    PickRowsArgs a = {};
    a.E = (u32)rs.E;
    a.n = (u32)n;
    a.w = (u32)w;
    const bool fresh = a.x.fill(v, s, n);
    const SubsetPlan sp = ReadTile::plan(fresh, v, U, (u32)sizeof(Unit));
    const ReadTile rt = rows_tile(sp, batch, rs);
    SelOutputs<1> one = {};
    one.fill(1, [](u32) { return 1u; }, false, sp.KC);
    a.tile.set(n_bits, U, sp, rt.QP, rs.E, one, rt.G);
    const u32 lds = fresh ? sel_lds_layout(a.tile, sp, a.x.tabs) : 0u;
    a.tile.xcd = stream_xcd(batch * rs.sumT * U);
    for (u32 j = 0; j < w; ++j) {
        a.rows[j] = rs.table[j]->dev;
        a.A[j] = (u32)rs.table[j]->A;
        a.Tout[j] = (u32)rs.table[j]->Tout;
    }
    const u64 max_blocks = launch_blocks(), per_group = (u64)a.tile.chunks * a.tile.qparts;
    // every launch of the split, before the first is issued
    bool ok = true;
    (void)launch_groups(max_blocks, batch, a.tile.G, per_group, [&](u64 e0, u64 ne, u32 nblocks) {
        ok = ok && rows_launch_ok(a.tile, rs, batch, e0, ne, nblocks);
    });
    if (!ok)
        return hipErrorInvalidValue;
    return sel_launch(k_uint_pick_rows<Unit, true>, k_uint_pick_rows<Unit, false>, a, lds, max_blocks, batch, per_group,
                      st, [&](u64 e0) {
        a.x.template advance<Unit>(index, e0, U);
        for (u32 j = 0; j < w; ++j) {           // an element is A_j terms of a source and Tout_j terms of an output
            a.src[j] = reinterpret_cast<const Unit *>(arrays[j]) + e0 * rs.table[j]->A * U;
            a.out[j] = reinterpret_cast<Unit *>(out[j]) + e0 * rs.table[j]->Tout * U;
        }
    });
}

// The composed form, row by row through the tuned launchers: EQ(index, r) by csgn_uint_plain into a temporary, once for
// every plane, then per plane the pitched copy of row r (pitch A_j) into a dense temporary and csgn_mul_uniform of EQ with
// it into r's block of output j (pitch Tout_j).  The temporaries live in one block (scratch_take, csgn_kernels.h), apart
// from the one csgn_uint_plain's composed form may take for EQ.
hipError_t rows_composed(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 n, u64 w,
                         const u64 *const *arrays, const u64 *T, u64 *const *out, const RowsShape &rs, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64;
    u64 max_eq = 1, maxT = 0;           // row 0 has the most EQ terms: every R_k = s_k + 1
    for (u64 k = 0; k < v; ++k)
        max_eq *= s[k] + 1;
    for (u64 i = 0; i < w * n; ++i)
        maxT = std::max(maxT, T[i]);
    const u64 eq_words = batch * max_eq * dL;
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_UINT_PICK_ROWS, (eq_words + batch * maxT * dL) * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    u64 *eq = block, *row = block + eq_words;
    for (u64 r = 0; r < n && e == hipSuccess; ++r) {
        const u64 er = uint_plain_terms(CSGN_UINT_PLAIN_EQ, v, r, s);
        e = uint_plain(n_bits, CSGN_UINT_PLAIN_EQ, batch, v, r, index, s, eq, st);
        for (u64 j = 0; j < w && e == hipSuccess; ++j) {
            const RowsTable &t = *rs.table[j];
            const u64 Tr = T[j * n + r], total = batch * Tr * dL;
            const u32 blocks = (u32)std::min<u64>((total + 255) / 256, 8192);
            k_pick_rows_copy<<<blocks, 256, 0, st>>>(arrays[j] + t.rows[r].src_off * dL, t.A * dL, Tr * dL, total, row);
            e = hipGetLastError();
            if (e == hipSuccess)
                e = mul_uniform(n_bits, batch, er, Tr, eq, row, out[j] + t.rows[r].out_off * dL, 0, st, t.Tout * dL);
        }
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

bool uint_pick_rows_sizes(u64 v, const u64 *s, u64 n, u64 w, const u64 *T, u64 *A, u64 *Tout)
{
    RowsShape rs;
    if (!rows_shape(v, s, n, w, T, rs))
        return false;
    for (u64 j = 0; j < w; ++j) {
        A[j] = rs.table[j]->A;
        Tout[j] = rs.table[j]->Tout;
    }
    return true;
}

void uint_pick_rows_stats(u64 out[3])
{
    out[0] = g_rows.v.size();
    out[1] = g_rows.retired.size();
    out[2] = g_rows.freed;
}

const char *uint_pick_rows_kernel_name() { return rows_use_fused() ? "k_uint_pick_rows" : "composed"; }

int uint_pick_rows_decode(u64 v, const u64 *s, u64 n, const u64 *T, u64 position, u64 out[3])
{
    RowsTable *t = rows_table(v, s, n, T);
    if (!t || !out || position >= t->Tout)
        return CSGN_ERR_INVALID;
    if (!t->fits)
        return CSGN_ERR_UNSUPPORTED;
    PickRow rec;
    u32 in, c;
    out[0] = pick_rows_locate(t->rows.data(), 0, (u32)n - 1u, (u32)position, rec, in, c);
    out[1] = in;
    out[2] = c;
    return CSGN_OK;
}

hipError_t uint_pick_rows(u64 n_bits, u64 batch, u64 v, const u64 *const *index, const u64 *s, u64 n, u64 w,
                          const u64 *const *arrays, const u64 *T, u64 *const *out, hipStream_t stream)
{
    if (batch == 0)
        return hipSuccess;
    RowsShape rs;
    if (!rows_shape(v, s, n, w, T, rs))
        return hipErrorInvalidValue;
    if (!rows_use_fused())
        return rows_composed(n_bits, batch, v, index, s, n, w, arrays, T, out, rs, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(index, v), ptr_array(arrays, w), ptr_array(out, w));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? rows_fused<unit16>(n_bits, batch, v, index, s, n, w, arrays, out, rs, U, stream)
                : rows_fused<unit8>(n_bits, batch, v, index, s, n, w, arrays, out, rs, U, stream);
}

} // namespace csgn
