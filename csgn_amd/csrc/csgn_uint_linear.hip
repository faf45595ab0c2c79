// csgn_uint_linear.hip -- a PUBLIC matrix over F2 applied to a bit-sliced encrypted integer, every output plane in one
// launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.36.
//
// The definition (include/csgn_hip.h, csgn_uint_linear): output plane j is the left-nested sum (the reference's
// operator+, concatenation), ascending in i, of the input planes a_i that bit i of the public row mask M_j names, then
// ONE where bit j of the public constant is set; a row that names nothing is the one-term constant.  Nothing is
// multiplied, so an element of an output plane is a sequence of COPY segments, one per set bit of M_j, and at most
// one constant segment: the kernel is a gather whose index is decoded from the lane's position.
//
// One lane writes one unit; lanes run unit-fastest inside one output plane.  Two things differ from k_uint_bitwise:
//   - the segment list is per workgroup (a workgroup belongs to one output plane, so its row is scalar).  When every
//     input plane has the same term count the segment is one fast division and its source plane is the s-th set bit of
//     the mask (linear_nth_set); otherwise the workgroup builds the row's segment ends and planes in LDS once (at most
//     64 entries) and a lane finds its segment by binary search (linear_segment).  The host's decode by position,
//     csgn_uint_linear_decode, calls the same two functions.
//   - the grid is TILE-major.  A tile is G elements of ALL output planes; workgroup -> tile by fast division, then the
//     plane by first[], then the unit.  A dense matrix reads every input plane about out_width / 2 times; in a tile
//     those re-reads are a few KB apart instead of a plane apart, and under the XCD-contiguous block order a tile's
//     workgroups share an XCD, so they hit that XCD's L2.
// A lane issues one load and one store; the load is unconditional (a constant unit loads the element's first unit of
// plane 0 and selects).  No scratch.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kMaxPlanes = kLinearMaxPlanes;

// Units one tile writes, over all output planes: G = kTileUnits / (units per element), one element at least.  Chosen
// by measurement (16 Ki, 64 Ki, 256 Ki and 1 Mi units were timed).  A compile-time constant,
// not a knob: tools/bench_uint_linear.py builds private copies of the library with other values to time them.
#ifndef CSGN_LINEAR_TILE_UNITS
#define CSGN_LINEAR_TILE_UNITS 262144
#endif
constexpr u64 kTileUnits = CSGN_LINEAR_TILE_UNITS;

// By value in the kernel arguments (3.4 KB of the 4 KB limit; uniform indices are scalar loads).
//     in[i], ta[i]   input plane i's first element of this launch, its terms per element
//     out[j]         output plane j's first element of this launch;  rows[j] its mask;  PU.d[j] its units per element
//     first[j]       plane j's first workgroup INSIDE a tile (first[np] = workgroups per tile)
struct LinearArgs {
    const void *in[kMaxPlanes];
    void *out[kMaxPlanes];
    u64 rows[kMaxPlanes];
    u32 ta[kMaxPlanes];
    u32 first[kMaxPlanes + 1];
    FastDivTable<kMaxPlanes> PU;
    u64 constant, last_mask;
    u32 nin, p0, np;          // input planes; the output planes of this launch are p0 .. p0 + np - 1
    u32 U, G, ne;             // units per term, elements per tile, elements of this launch
    u32 eq;                   // every input plane has ta[0] terms: no LDS table
    u32 xcd;
    FastDiv dper, dTU;        // workgroups per tile; ta[0] * U (eq only)
};
static_assert(sizeof(LinearArgs) <= 4096, "kernel arguments past the 4 KB limit");

// The decode by position, shared by the kernel (positions in units) and csgn_uint_linear_decode (positions in terms).
// The segment of position q among nseg segments with ascending ends end(0) .. end(nseg - 1): the smallest s with
// q < end(s), or nseg when q is at or past the last end (the constant term).  At most 7 probes.
template <typename Q, typename Ends>
__host__ __device__ inline u32 linear_segment(u32 nseg, Q q, Ends end)
{
    u32 lo = 0, hi = nseg;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (q < end(mid))
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}

// the position of the s-th set bit of m (s = 0: the lowest); s < popcount(m)
__host__ __device__ inline u32 linear_nth_set(u64 m, u32 s)
{
    u32 pos = 0;
    for (u32 span = 32; span; span >>= 1) {
        const u64 low = (m >> pos) & ((1ull << span) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
        const u32 c = (u32)__popcll(low);
#else
        const u32 c = (u32)__builtin_popcountll(low);
#endif
        if (s >= c) {
            s -= c;
            pos += span;
        }
    }
    return pos;
}

template <typename Unit>
__global__ void __launch_bounds__(256) k_uint_linear(LinearArgs g)
{
    __shared__ u32 s_end[kMaxPlanes], s_plane[kMaxPlanes];
    const u32 bid = g.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const u32 tile = csgn_fastdiv(bid, g.dper), wb = bid - tile * g.dper.d;
    u32 q = 0, hi = g.np;                                 // the plane of this workgroup: first[q] <= wb < first[q + 1]
    while (hi - q > 1u) {
        const u32 mid = (q + hi) >> 1;
        if (g.first[mid] <= wb)
            q = mid;
        else
            hi = mid;
    }
    const u32 p = g.p0 + q, U = g.U;
    const u64 M = g.rows[p];
    const u32 nseg = (u32)__popcll(M);
    if (!g.eq) {                                          // the row's segments, once: end (units) and plane of the s-th
        if (threadIdx.x < kMaxPlanes && ((M >> threadIdx.x) & 1ull)) {
            u32 end = 0;
            for (u32 b = 0; b < g.nin; ++b)               // uniform trip count, scalar loads of ta
                if (b <= threadIdx.x && ((M >> b) & 1ull))
                    end += g.ta[b];
            const u32 s = (u32)__popcll(M & ((1ull << threadIdx.x) - 1ull));
            s_end[s] = end * U;
            s_plane[s] = threadIdx.x;
        }
        __syncthreads();
    }
    const FastDiv dpu = g.PU.at(p);
    const u32 e0 = tile * g.G, ge = min(g.G, g.ne - e0);
    const u32 off = (wb - g.first[q]) * 256u + threadIdx.x;   // unit inside this tile's part of plane p
    if (off >= ge * dpu.d)
        return;
    const u32 el = csgn_fastdiv(off, dpu), r = off - el * dpu.d;
    const u64 e = (u64)e0 + el;
    u32 s, start, plane, span;                            // segment, its first unit, its plane, the plane's units
    if (g.eq) {
        span = g.dTU.d;
        s = csgn_fastdiv(r, g.dTU);
        start = min(s, nseg) * span;
        plane = linear_nth_set(M, min(s, nseg ? nseg - 1u : 0u));
    } else {
        s = linear_segment(nseg, r, [&](u32 i) { return s_end[i]; });
        const u32 at = min(s, nseg ? nseg - 1u : 0u);
        start = s ? s_end[s - 1u] : 0u;
        span = nseg ? s_end[at] - (at ? s_end[at - 1u] : 0u) : 0u;
        plane = nseg ? s_plane[at] : 0u;
    }
    const bool is_const = s >= nseg;                      // ONE or ZERO: its load is the element's first unit of plane 0
    if (is_const) {
        plane = 0;
        span = g.ta[0] * U;
    }
    const Unit *src = reinterpret_cast<const Unit *>(g.in[plane]);
    const Unit v = src[e * span + (is_const ? 0u : r - start)];
    const bool one = (g.constant >> p) & 1ull;
    const Unit w = !is_const ? v : one ? one_unit(Unit(), r - start, U, g.last_mask) : zero_unit(Unit());
    unit_store<Unit, true>(reinterpret_cast<Unit *>(g.out[p]) + ((u64)e0 * dpu.d + off), w);
}

// ------------------------------------------------------------------------------ the definition on the host

struct LinearShape {
    u32 nin = 0, nout = 0;
    u64 ta[kMaxPlanes] = {}, rows[kMaxPlanes] = {}, T[kMaxPlanes] = {};
    u64 constant = 0;
    bool eq = true;
};

// false: an invalid argument or a term count of 2^62 or more
bool linear_shape(u64 nin, const u64 *ta, u64 nout, const u64 *rows, u64 constant, LinearShape &sh)
{
    sh = LinearShape();
    if (nin < 1 || nin > kMaxPlanes || nout < 1 || nout > kMaxPlanes || !ta || !rows)
        return false;
    sh.nin = (u32)nin;
    sh.nout = (u32)nout;
    sh.constant = nout < 64 ? constant & ((1ull << nout) - 1ull) : constant;
    for (u64 i = 0; i < nin; ++i) {
        sh.ta[i] = ta[i];
        sh.eq = sh.eq && ta[i] == ta[0];
    }
    for (u64 j = 0; j < nout; ++j) {
        sh.rows[j] = rows[j];
        sh.T[j] = uint_linear_terms(nin, ta, rows[j], (int)((sh.constant >> j) & 1ull));
        if (sh.T[j] == 0)
            return false;
    }
    return true;
}

// How a call is cut (csgn_uint_linear_plan reports it; the launcher follows it).  A plane GROUP is a run of output planes
// whose workgroups of one tile fit one launch's 2^32 lanes: one group for every shape but those of which ONE element of
// all planes does not fit, which take a launch sequence per group.
struct LinearPlan {
    u32 U = 0, G = 0;
    u64 units = 0;            // per element, all planes
    u64 tiles = 0, per_tile = 0, launches = 0, groups = 0;
    u32 blocks[kMaxPlanes] = {};   // workgroups of plane j in one tile
};

LinearPlan linear_plan(const LinearShape &sh, u64 dL, u64 batch, bool wide, u64 max_blocks)
{
    LinearPlan pl;
    pl.U = (u32)(wide ? dL / 2 : dL);
    for (u32 j = 0; j < sh.nout; ++j)
        pl.units += sh.T[j] * pl.U;
    pl.G = (u32)std::min<u64>(std::max<u64>(1, kTileUnits / pl.units), std::max<u64>(1, batch));
    pl.tiles = (batch + pl.G - 1) / pl.G;
    for (u32 j = 0; j < sh.nout;) {                       // the groups, and the launches of each
        u64 per = 0;
        u32 k = j;
        for (; k < sh.nout; ++k) {
            pl.blocks[k] = ceil_div_u64((u64)pl.G * sh.T[k] * pl.U, 256u);
            if (k > j && per + pl.blocks[k] > kMaxBlocks256)
                break;
            per += pl.blocks[k];
        }
        const u64 tiles_per_launch = std::max<u64>(1, max_blocks / per);
        pl.launches += (pl.tiles + tiles_per_launch - 1) / tiles_per_launch;
        pl.per_tile += per;
        ++pl.groups;
        j = k;
    }
    return pl;
}

template <typename Unit>
hipError_t linear_kernel(const LinearShape &sh, u64 n_bits, u64 batch, const u64 *const *in, u64 *const *out,
                         const LinearPlan &pl, hipStream_t s)
{
    LinearArgs g = {};
    const u32 U = pl.U;
    g.U = U;
    g.G = pl.G;
    g.nin = sh.nin;
    g.eq = sh.eq ? 1u : 0u;
    g.dTU = csgn_fastdiv_make((u32)(sh.ta[0] * U));
    g.constant = sh.constant;
    g.last_mask = last_word_mask(n_bits);
    for (u32 i = 0; i < kMaxPlanes; ++i) {
        g.ta[i] = i < sh.nin ? (u32)sh.ta[i] : 1u;
        g.rows[i] = i < sh.nout ? sh.rows[i] : 0;
        g.PU.set(i, i < sh.nout ? (u32)(sh.T[i] * U) : 1u);
    }
    const u64 max_blocks = launch_blocks();
    for (u32 j = 0; j < sh.nout;) {                       // linear_plan's groups
        u64 per = 0, units = 0;
        u32 k = j;
        for (; k < sh.nout; ++k) {
            if (k > j && per + pl.blocks[k] > kMaxBlocks256)
                break;
            g.first[k - j] = (u32)per;
            per += pl.blocks[k];
            units += sh.T[k] * U;
        }
        g.first[k - j] = (u32)per;
        g.p0 = j;
        g.np = k - j;
        g.dper = csgn_fastdiv_make((u32)per);
        const u64 tiles_per_launch = std::max<u64>(1, max_blocks / per);
        for (u64 t0 = 0; t0 < pl.tiles; t0 += tiles_per_launch) {
            const u64 nt = std::min(tiles_per_launch, pl.tiles - t0), e0 = t0 * pl.G;
            const u64 ne = std::min<u64>(batch - e0, nt * pl.G);
            for (u32 i = 0; i < sh.nin; ++i)
                g.in[i] = reinterpret_cast<const Unit *>(in[i]) + e0 * sh.ta[i] * U;
            for (u32 o = j; o < k; ++o)
                g.out[o] = reinterpret_cast<Unit *>(out[o]) + e0 * sh.T[o] * U;
            g.ne = (u32)ne;
            g.xcd = stream_xcd(ne * units);
            k_uint_linear<Unit><<<dim3((u32)(nt * per)), 256, 0, s>>>(g);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess)
                return e;
        }
        j = k;
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_linear_terms(u64 nin, const u64 *ta, u64 row, int constant_bit)
{
    if (nin < 1 || nin > kMaxPlanes || !ta || (nin < 64 && (row >> nin)) || (constant_bit != 0 && constant_bit != 1))
        return 0;
    u64 total = 0;
    for (u64 i = 0; i < nin; ++i) {
        if (ta[i] == 0 || ta[i] >= kTermLimit)
            return 0;
        if ((row >> i) & 1ull) {
            total += ta[i];
            if (total >= kTermLimit)
                return 0;
        }
    }
    total += (u64)constant_bit;
    if (row == 0)
        total = 1;
    return total < kTermLimit ? total : 0;
}

bool uint_linear_decode(u64 nin, const u64 *ta, u64 row, int constant_bit, u64 q, u64 *plane, u64 *term)
{
    const u64 T = uint_linear_terms(nin, ta, row, constant_bit);
    if (T == 0 || q >= T || !plane || !term)
        return false;
    u64 end[kMaxPlanes];
    u32 nseg = 0;
    for (u64 i = 0, sum = 0; i < nin; ++i)
        if ((row >> i) & 1ull)
            end[nseg++] = sum += ta[i];
    const u32 s = linear_segment(nseg, q, [&](u32 i) { return end[i]; });
    if (s >= nseg) {                                      // the constant term
        *plane = constant_bit ? nin : nin + 1;
        *term = 0;
        return true;
    }
    *plane = linear_nth_set(row, s);
    *term = q - (s ? end[s - 1] : 0);
    return true;
}

bool uint_linear_plan(u64 n_bits, u64 batch, u64 nin, const u64 *ta, u64 nout, const u64 *rows, u64 constant, u64 *plan)
{
    LinearShape sh;
    if (n_bits == 0 || !plan || !linear_shape(nin, ta, nout, rows, constant, sh))
        return false;
    const u64 dL = (n_bits + 63) / 64;
    const LinearPlan pl = linear_plan(sh, dL, batch, dL % 2 == 0, launch_blocks());
    plan[0] = dL % 2 == 0 ? 16 : 8;
    plan[1] = pl.units;
    plan[2] = pl.G;
    plan[3] = pl.tiles;
    plan[4] = pl.per_tile;
    plan[5] = batch ? pl.launches : 0;
    plan[6] = kTileUnits;
    plan[7] = pl.groups;
    return true;
}

hipError_t uint_linear(u64 n_bits, u64 batch, u64 nin, const u64 *const *in, const u64 *ta, u64 nout, const u64 *rows,
                       u64 constant, u64 *const *out, hipStream_t s)
{
    LinearShape sh;
    if (!linear_shape(nin, ta, nout, rows, constant, sh))
        return hipErrorInvalidValue;
    if (batch == 0)
        return hipSuccess;
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(in, sh.nin), ptr_array(out, sh.nout));
    const LinearPlan pl = linear_plan(sh, dL, batch, wide, launch_blocks());
    return wide ? linear_kernel<unit16>(sh, n_bits, batch, in, out, pl, s)
                : linear_kernel<unit8>(sh, n_bits, batch, in, out, pl, s);
}

} // namespace csgn
