// csgn_uint_bilinear.hip -- a PUBLIC bilinear form over F2 of TWO bit-sliced encrypted integers, every output plane in
// one launch: carry-less products, products in GF(2^w), a secret bit matrix applied to a secret vector, parity(a & b).
// Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.38.
//
// The definition (include/csgn_hip.h, csgn_uint_bilinear): output plane x is the left-nested sum (the reference's
// operator+, concatenation) of the products a_left * b_right (the reference's operator*: all pairs of terms, the left
// term slow) of its entries, in the order given, then ONE where bit x of the public constant is set; a plane of no entry
// is the one-term constant.  An element of an output plane is a sequence of SEGMENTS, one per entry, of ta_left *
// tb_right terms each, and at most one constant term; a term is the AND of one term of a_left and one of b_right.
//
// One lane writes one unit at a time and WALKS: the grid is tile-major, a tile is G elements of all output planes, the
// stream inside a tile is (plane, element, term, unit) with the unit fastest, and workgroup s of a tile's S walks the
// positions [s * chunk, (s + 1) * chunk) of that stream, 256 consecutive units a step.  A lane decodes its position:
//   - the plane, by a search of the tile's plane prefix (LDS, 6 probes), then element and term by the plane's FastDiv;
//   - the entry: one fast division when every ta is equal and every tb is equal, else a binary search of the plane's
//     first-term table (bilinear_entry: in LDS when the plan has at most kLdsEntries entries, else through the vector
//     cache); the host's decode by position, csgn_uint_bilinear_decode, calls the same two functions;
//   - the (left term, right term) by the FastDiv of tb_right.
// STAGED shapes (one element's operand planes fit kStageBytes of LDS and the form writes at least kStageMinRatio times
// what it reads): G is as many elements as fit, every workgroup of a tile copies the tile's operand units to LDS once,
// four loads in flight a lane, and S is chosen so that a chunk is at least kStageRatio times the staged units: a
// workgroup writes several times what it stages (DESIGN §4.35 measured what less costs).  Other shapes read both
// operand units from memory, G set by the tile budget so that the re-reads stay close.  No scratch.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>
#include <vector>

namespace csgn {

namespace {

constexpr u32 kMaxPlanes = kBilinearMaxPlanes;

// Compile-time budgets, not knobs: tools/bench_uint_bilinear.py builds private copies of the library with other values
// to time them.
#ifndef CSGN_BILINEAR_STAGE_BYTES
#define CSGN_BILINEAR_STAGE_BYTES 16384
#endif
#ifndef CSGN_BILINEAR_TILE_UNITS
#define CSGN_BILINEAR_TILE_UNITS 262144
#endif
#ifndef CSGN_BILINEAR_STAGE_RATIO
#define CSGN_BILINEAR_STAGE_RATIO 4
#endif
#ifndef CSGN_BILINEAR_MIN_CHUNK
#define CSGN_BILINEAR_MIN_CHUNK 2048
#endif
constexpr u64 kStageBytes = CSGN_BILINEAR_STAGE_BYTES;   // LDS for a tile's operand units
constexpr u64 kTileUnits = CSGN_BILINEAR_TILE_UNITS;     // units an unstaged tile writes, over all planes
constexpr u64 kStageRatio = CSGN_BILINEAR_STAGE_RATIO;   // a staged workgroup writes at least this many times its LDS copy
constexpr u64 kStageMinRatio = 2;                        // written / read per element below which staging cannot pay
constexpr u64 kMinChunk = CSGN_BILINEAR_MIN_CHUNK;       // units a workgroup walks at least; a multiple of 256
constexpr u64 kMaxTile = 1ull << 31;                     // units of one tile of one plane group: positions stay u32
constexpr u32 kLdsEntries = 512;                         // entries whose first terms and pairs a workgroup keeps in LDS
static_assert(kMinChunk % 256 == 0 && kMinChunk >= 256, "a workgroup walks whole steps");
static_assert(kStageBytes % 16 == 0 && kStageBytes + 8192 <= 65536, "static LDS");

// The plan's tables on the device, then start[n_entries] and lr[n_entries].  Indices of input planes are compact:
// a_i is i, b_l is wa + l.
struct BilinearTab {
    u64 Tpre[kMaxPlanes + 1];                 // terms per element of the output planes before x
    u32 T[kMaxPlanes], Tm[kMaxPlanes], Ts[kMaxPlanes];   // T_x and its FastDiv
    u32 efirst[kMaxPlanes + 1];
    u32 tin[2 * kMaxPlanes];                  // terms per element of the input planes
    u32 tbm[kMaxPlanes], tbs[kMaxPlanes];     // the FastDiv of tb_l
    u32 opre[2 * kMaxPlanes + 1];             // terms per element of the input planes before i (saturating)
};

// By value in the kernel arguments (1.7 KB of the 4 KB limit).
//     in[i]     input plane i's first element of this launch (compact index)
//     out[x]    output plane x's first element of this launch
struct BilinearArgs {
    const void *in[2 * kMaxPlanes];
    void *out[kMaxPlanes];
    const BilinearTab *tab;
    const u32 *start, *lr;    // per entry: its first term in its plane; left | right << 8
    u64 constant, last_mask;
    u32 wa, wb, nent;         // input planes; entries of the plan
    u32 p0, np;               // the output planes of this launch are p0 .. p0 + np - 1
    u32 U, G, ne;             // units per term, elements per tile, elements of this launch
    u32 chunk;                // units a workgroup walks
    u32 eq;                   // every a plane has ta[0] terms and every b plane tb[0]: no search
    u32 lds_tab;              // nent <= kLdsEntries
    u32 xcd;
    FastDiv dS, dU, dTT, dtb; // workgroups per tile; U; ta[0] * tb[0] and tb[0] (eq only)
};
static_assert(sizeof(BilinearArgs) <= 4096, "kernel arguments past the 4 KB limit");

// The decode by position, shared by the kernel and csgn_uint_bilinear_decode.  The entry of term `term` of a plane of
// nent entries and eterms entry terms (the plane's constant not counted): nent when term is at or past eterms (the
// constant), else the entry, with q the term inside it.  eq: every entry has dTT.d terms.  Otherwise start(i) is the
// first term of entry i, start(0) = 0, strictly ascending (an entry has a term at least): at most 18 probes.
template <typename Start>
__host__ __device__ inline u32 bilinear_entry(u32 nent, u32 eterms, u32 term, bool eq, const FastDiv &dTT, Start start,
                                              u32 &q)
{
    q = 0;
    if (term >= eterms)
        return nent;
    if (eq) {
        const u32 ent = csgn_fastdiv(term, dTT);
        q = term - ent * dTT.d;
        return ent;
    }
    u32 lo = 0, hi = nent;
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (start(mid) <= term)
            lo = mid;
        else
            hi = mid;
    }
    q = term - start(lo);
    return lo;
}

// term q of a_left * b_right: the left term is slow
__host__ __device__ inline void bilinear_split(u32 q, const FastDiv &dtb, u32 &lt, u32 &rt)
{
    lt = csgn_fastdiv(q, dtb);
    rt = q - lt * dtb.d;
}

template <typename Unit, bool Staged>
__global__ void __launch_bounds__(256) k_uint_bilinear(BilinearArgs g)
{
    __shared__ u32 s_pre[kMaxPlanes + 1];                 // first term of plane p0 + q in this tile; [np]: the tile's terms
    __shared__ u32 s_opre[2 * kMaxPlanes + 1];            // staged: first LDS unit of input plane i; [wa + wb]: the units
    __shared__ u32 s_start[kLdsEntries], s_lr[kLdsEntries];
    __shared__ Unit s_op[Staged && kStageBytes ? kStageBytes / sizeof(Unit) : 1];   // kStageBytes = 0: nothing is staged
    const BilinearTab *__restrict__ t = g.tab;
    const u32 bid = g.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const u32 tile = csgn_fastdiv(bid, g.dS), s = bid - tile * g.dS.d;
    const u32 e0 = tile * g.G, ge = min(g.G, g.ne - e0), U = g.U, nin = g.wa + g.wb;
    const u64 base = t->Tpre[g.p0];
    const u32 total = ge * (u32)(t->Tpre[g.p0 + g.np] - base) * U;   // units of this tile, at most kMaxTile
    const u32 lo = s * g.chunk;                           // below 2^31 + 2^28: s < S and S * chunk < G * units + 256 * S
    if (lo >= total)                                      // the last tile is short: uniform, before any barrier
        return;
    const u32 hi = min(lo + g.chunk, total);
    if (threadIdx.x <= g.np)
        s_pre[threadIdx.x] = ge * (u32)(t->Tpre[g.p0 + threadIdx.x] - base);
    if (Staged && threadIdx.x <= nin)
        s_opre[threadIdx.x] = ge * t->opre[threadIdx.x] * U;
    if (g.lds_tab)
        for (u32 i = threadIdx.x; i < g.nent; i += 256u) {
            s_start[i] = g.start[i];
            s_lr[i] = g.lr[i];
        }
    __syncthreads();
    if (Staged) {                                         // the tile's operand units, plane-major, four loads in flight
        const u32 n = s_opre[nin];                        // ge * operand units per element <= kStageBytes / sizeof(Unit)
        for (u32 j0 = 0; j0 < n; j0 += 1024u) {
            Unit v[4];
#pragma unroll
            for (u32 u = 0; u < 4u; ++u) {
                const u32 j = j0 + u * 256u + threadIdx.x;
                v[u] = zero_unit(Unit());
                if (j < n) {
                    u32 pl = 0, ph = nin;                 // the plane: s_opre[pl] <= j < s_opre[pl + 1]
                    while (ph - pl > 1u) {
                        const u32 mid = (pl + ph) >> 1;
                        if (s_opre[mid] <= j)
                            pl = mid;
                        else
                            ph = mid;
                    }
                    const Unit *src = reinterpret_cast<const Unit *>(g.in[pl]);
                    v[u] = src[(u64)e0 * t->tin[pl] * U + (j - s_opre[pl])];   // < ne * tin * U units of the plane
                }
            }
#pragma unroll
            for (u32 u = 0; u < 4u; ++u) {
                const u32 j = j0 + u * 256u + threadIdx.x;
                if (j < n)
                    s_op[j] = v[u];
            }
        }
        __syncthreads();
    }
    for (u32 pos = lo + threadIdx.x; pos < hi; pos += 256u) {
        const u32 tpos = csgn_fastdiv(pos, g.dU), k = pos - tpos * U;
        u32 q = 0, qh = g.np;                             // the plane: s_pre[q] <= tpos < s_pre[q + 1]
        while (qh - q > 1u) {
            const u32 mid = (q + qh) >> 1;
            if (s_pre[mid] <= tpos)
                q = mid;
            else
                qh = mid;
        }
        const u32 p = g.p0 + q, off = tpos - s_pre[q];    // off < ge * T
        const u32 T = t->T[p];
        const u32 el = csgn_fastdiv(off, FastDiv{T, t->Tm[p], t->Ts[p]}), term = off - el * T;
        const u32 ef = t->efirst[p], nent = t->efirst[p + 1u] - ef;
        const bool one = (g.constant >> p) & 1ull;
        const u32 eterms = T - ((nent == 0u || one) ? 1u : 0u);
        u32 qq;
        const u32 ent = g.lds_tab ? bilinear_entry(nent, eterms, term, g.eq, g.dTT, [&](u32 i) { return s_start[ef + i]; }, qq)
                                  : bilinear_entry(nent, eterms, term, g.eq, g.dTT, [&](u32 i) { return g.start[ef + i]; }, qq);
        Unit w;
        if (ent >= nent) {
            w = one ? one_unit(Unit(), k, U, g.last_mask) : zero_unit(Unit());
        } else {
            const u32 lr = g.lds_tab ? s_lr[ef + ent] : g.lr[ef + ent];
            const u32 L = lr & 0xFFu, R = g.wa + (lr >> 8);          // compact indices: L < wa <= R < wa + wb
            const u32 tl = t->tin[L], tr = t->tin[R];
            u32 lt, rt;
            bilinear_split(qq, g.eq ? g.dtb : FastDiv{tr, t->tbm[R - g.wa], t->tbs[R - g.wa]}, lt, rt);   // lt < tl, rt < tr
            if (Staged) {
                w = s_op[s_opre[L] + (el * tl + lt) * U + k] & s_op[s_opre[R] + (el * tr + rt) * U + k];
            } else {
                const u64 e = (u64)e0 + el;
                w = reinterpret_cast<const Unit *>(g.in[L])[(e * tl + lt) * U + k] &
                    reinterpret_cast<const Unit *>(g.in[R])[(e * tr + rt) * U + k];
            }
        }
        unit_store<Unit, true>(reinterpret_cast<Unit *>(g.out[p]) + (((u64)e0 * T + off) * U + k), w);
    }
}

// ------------------------------------------------------------------------------ the definition on the host

// T of one plane; 0: invalid or 2^62 terms or more.  start (optional) takes every entry's first term while the plane
// stays below 2^31 terms; lr its pair.
u64 bilinear_plane(u64 wa, const u64 *ta, u64 wb, const u64 *tb, u64 n_entries, const u64 *left, const u64 *right,
                   int constant_bit, std::vector<u32> *start, std::vector<u32> *lr)
{
    if (wa < 1 || wa > kMaxPlanes || wb < 1 || wb > kMaxPlanes || !ta || !tb || (n_entries && (!left || !right)) ||
        (constant_bit != 0 && constant_bit != 1))
        return 0;
    for (u64 i = 0; i < wa; ++i)
        if (ta[i] == 0 || ta[i] >= kTermLimit)
            return 0;
    for (u64 l = 0; l < wb; ++l)
        if (tb[l] == 0 || tb[l] >= kTermLimit)
            return 0;
    u64 T = 0;
    for (u64 i = 0; i < n_entries; ++i) {
        u64 p;
        if (left[i] >= wa || right[i] >= wb || !term_mul(ta[left[i]], tb[right[i]], p))
            return 0;
        if (start && T < (1ull << 31)) {
            start->push_back((u32)T);
            lr->push_back((u32)left[i] | ((u32)right[i] << 8));
        }
        T += p;
        if (T >= kTermLimit)
            return 0;
    }
    if (constant_bit || n_entries == 0)
        ++T;
    return T < kTermLimit ? T : 0;
}

bool bilinear_equal(u64 wa, const u64 *ta, u64 wb, const u64 *tb)
{
    u64 p;
    return std::all_of(ta, ta + wa, [&](u64 x) { return x == ta[0]; }) &&
           std::all_of(tb, tb + wb, [&](u64 x) { return x == tb[0]; }) && term_mul(ta[0], tb[0], p) && p < (1ull << 31);
}

// How a call is cut (csgn_uint_bilinear_launches reports it; the launcher follows it).  A plane GROUP is a run of
// output planes of which one tile stays within kMaxTile units: one group for every shape but those of which ONE element
// of all planes does not, which take G = 1 and a launch sequence per group.
struct BilinearCut {
    u32 U = 0, G = 0, groups = 0;
    bool staged = false;
    u64 units = 0, op_units = 0;          // per element: all output planes; all input planes
    u64 tiles = 0, per_tile = 0, launches = 0, first_blocks = 0;
    u32 gfirst[kMaxPlanes + 1] = {};      // group i is the planes gfirst[i] .. gfirst[i + 1] - 1
    u32 S[kMaxPlanes] = {};               // its workgroups per tile
    u32 chunk[kMaxPlanes] = {};           // the units each of them walks: the tile in S even parts, whole steps
    u64 tpl[kMaxPlanes] = {};             // its tiles per launch
};

BilinearCut bilinear_cut(const BilinearPlan &pl, u64 dL, u64 batch, bool wide, u64 max_blocks)
{
    BilinearCut c;
    const u64 ub = wide ? 16 : 8;
    c.U = (u32)(wide ? dL / 2 : dL);
    for (u32 x = 0; x < pl.n_out; ++x)
        c.units += pl.T[x] * c.U;
    u64 op_terms = 0;
    for (u32 i = 0; i < pl.wa; ++i)
        op_terms += std::min<u64>(pl.ta[i], 1ull << 32);
    for (u32 l = 0; l < pl.wb; ++l)
        op_terms += std::min<u64>(pl.tb[l], 1ull << 32);
    c.op_units = op_terms * c.U;
    c.staged = c.op_units * ub <= kStageBytes && c.units >= kStageMinRatio * c.op_units;
    const u64 b1 = std::max<u64>(batch, 1);
    u64 G = c.staged ? kStageBytes / (c.op_units * ub) : std::max<u64>(1, kTileUnits / c.units);
    G = std::min(std::min(G, b1), std::max<u64>(1, kMaxTile / c.units));
    c.G = (u32)G;
    c.tiles = (b1 + G - 1) / G;
    // what a workgroup walks at least: staged, kStageRatio times the units it stages (at most 4 * kStageBytes / 8)
    const u64 least = c.staged ? std::max(kMinChunk, kStageRatio * G * c.op_units) : kMinChunk;
    for (u32 j = 0; j < pl.n_out;) {
        u64 units = 0;
        u32 k = j;
        for (; k < pl.n_out; ++k) {
            if (k > j && G * (units + pl.T[k] * c.U) > kMaxTile)
                break;
            units += pl.T[k] * c.U;
        }
        const u64 S = std::max<u64>(1, G * units / least);   // at most kMaxTile / kMinChunk = 2^20
        c.gfirst[c.groups] = j;
        c.S[c.groups] = (u32)S;
        c.chunk[c.groups] = (u32)(((G * units + S - 1) / S + 255) / 256 * 256);   // below 2 * least + 256
        c.tpl[c.groups] = std::min(std::max<u64>(1, max_blocks / S), 0xFFFFFFFFull / G);   // elements of a launch are u32
        c.launches += (c.tiles + c.tpl[c.groups] - 1) / c.tpl[c.groups];
        if (c.groups == 0)
            c.first_blocks = std::min(c.tiles, c.tpl[0]) * S;
        c.per_tile += S;
        ++c.groups;
        j = k;
    }
    c.gfirst[c.groups] = pl.n_out;
    return c;
}

template <typename Unit, bool Staged>
hipError_t bilinear_kernel(const BilinearPlan &pl, u64 n_bits, u64 batch, const u64 *const *a, const u64 *const *b,
                           u64 *const *out, const BilinearCut &c, hipStream_t s)
{
    BilinearArgs g = {};
    const u32 U = c.U;
    g.tab = reinterpret_cast<const BilinearTab *>(pl.d_tab);
    g.start = reinterpret_cast<const u32 *>(reinterpret_cast<const char *>(pl.d_tab) + sizeof(BilinearTab));
    g.lr = g.start + pl.start.size();
    g.constant = pl.constant;
    g.last_mask = last_word_mask(n_bits);
    g.wa = pl.wa;
    g.wb = pl.wb;
    g.nent = (u32)pl.start.size();
    g.U = U;
    g.G = c.G;
    g.eq = pl.eq ? 1u : 0u;
    g.lds_tab = g.nent <= kLdsEntries ? 1u : 0u;
    g.dU = csgn_fastdiv_make(U);
    g.dTT = csgn_fastdiv_make(pl.eq ? (u32)(pl.ta[0] * pl.tb[0]) : 1u);
    g.dtb = csgn_fastdiv_make(pl.eq ? (u32)pl.tb[0] : 1u);
    for (u32 gi = 0; gi < c.groups; ++gi) {
        const u32 j = c.gfirst[gi], k = c.gfirst[gi + 1];
        u64 units = 0;
        for (u32 x = j; x < k; ++x)
            units += pl.T[x] * U;
        g.p0 = j;
        g.np = k - j;
        g.dS = csgn_fastdiv_make(c.S[gi]);
        g.chunk = c.chunk[gi];
        for (u64 t0 = 0; t0 < c.tiles; t0 += c.tpl[gi]) {
            const u64 nt = std::min(c.tpl[gi], c.tiles - t0), e0 = t0 * c.G;
            const u64 ne = std::min<u64>(batch - e0, nt * c.G);
            for (u32 i = 0; i < pl.wa; ++i)
                g.in[i] = reinterpret_cast<const Unit *>(a[i]) + e0 * pl.ta[i] * U;
            for (u32 l = 0; l < pl.wb; ++l)
                g.in[pl.wa + l] = reinterpret_cast<const Unit *>(b[l]) + e0 * pl.tb[l] * U;
            for (u32 x = j; x < k; ++x)
                g.out[x] = reinterpret_cast<Unit *>(out[x]) + e0 * pl.T[x] * U;
            g.ne = (u32)ne;
            g.xcd = stream_xcd(ne * units);
            k_uint_bilinear<Unit, Staged><<<dim3((u32)(nt * c.S[gi])), 256, 0, s>>>(g);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_bilinear_terms(u64 wa, const u64 *ta, u64 wb, const u64 *tb, u64 n_entries, const u64 *left, const u64 *right,
                        int constant_bit)
{
    return bilinear_plane(wa, ta, wb, tb, n_entries, left, right, constant_bit, nullptr, nullptr);
}

bool uint_bilinear_decode(u64 wa, const u64 *ta, u64 wb, const u64 *tb, u64 n_entries, const u64 *left, const u64 *right,
                          int constant_bit, u64 q, u64 *entry, u64 *left_term, u64 *right_term)
{
    std::vector<u32> start, lr;
    if (n_entries > kBilinearMaxEntries || !entry || !left_term || !right_term)
        return false;
    const u64 T = bilinear_plane(wa, ta, wb, tb, n_entries, left, right, constant_bit, &start, &lr);
    if (T == 0 || T >= (1ull << 31) || q >= T)
        return false;
    const bool eq = bilinear_equal(wa, ta, wb, tb);
    const u32 nent = (u32)n_entries, extra = (nent == 0 || constant_bit) ? 1u : 0u;
    u32 qq;
    const u32 ent = bilinear_entry(nent, (u32)T - extra, (u32)q, eq, csgn_fastdiv_make(eq ? (u32)(ta[0] * tb[0]) : 1u),
                                   [&](u32 i) { return start[i]; }, qq);
    *left_term = *right_term = 0;
    if (ent >= nent) {                                    // the plane's constant
        *entry = constant_bit ? n_entries : n_entries + 1;
        return true;
    }
    u32 lt, rt;
    bilinear_split(qq, csgn_fastdiv_make((u32)tb[lr[ent] >> 8]), lt, rt);
    *entry = ent;
    *left_term = lt;
    *right_term = rt;
    return true;
}

int uint_bilinear_shape(u64 wa, const u64 *ta, u64 wb, const u64 *tb, u64 n_out, const u64 *first, const u64 *left,
                        const u64 *right, u64 constant, BilinearPlan &pl)
{
    pl = BilinearPlan();
    if (wa < 1 || wa > kMaxPlanes || wb < 1 || wb > kMaxPlanes || n_out < 1 || n_out > kMaxPlanes || !ta || !tb || !first ||
        first[0] != 0 || (n_out < 64 && (constant >> n_out) != 0))
        return CSGN_ERR_INVALID;
    for (u64 x = 0; x < n_out; ++x)
        if (first[x + 1] < first[x])
            return CSGN_ERR_INVALID;
    if (first[n_out] && (!left || !right))
        return CSGN_ERR_INVALID;
    if (first[n_out] > kBilinearMaxEntries)
        return CSGN_ERR_UNSUPPORTED;
    pl.wa = (u32)wa;
    pl.wb = (u32)wb;
    pl.n_out = (u32)n_out;
    pl.constant = constant;
    std::copy(ta, ta + wa, pl.ta);
    std::copy(tb, tb + wb, pl.tb);
    int rc = CSGN_OK;
    for (u64 x = 0; x < n_out; ++x) {
        pl.efirst[x] = (u32)first[x];
        pl.start.resize(first[x]);                        // a plane past 2^31 terms leaves entries out: the plan is refused
        pl.lr.resize(first[x]);
        pl.T[x] = bilinear_plane(wa, ta, wb, tb, first[x + 1] - first[x], left + first[x], right + first[x],
                                 (int)((constant >> x) & 1u), &pl.start, &pl.lr);
        if (pl.T[x] == 0)
            return CSGN_ERR_INVALID;
        if (pl.T[x] >= (1ull << 31))
            rc = CSGN_ERR_UNSUPPORTED;
    }
    pl.efirst[n_out] = (u32)first[n_out];
    pl.start.resize(first[n_out]);
    pl.lr.resize(first[n_out]);
    pl.eq = bilinear_equal(wa, ta, wb, tb);
    return rc;
}

int uint_bilinear_create(BilinearPlan &pl, hipError_t &herr)
{
    std::vector<u32> blob(sizeof(BilinearTab) / sizeof(u32));
    BilinearTab *t = reinterpret_cast<BilinearTab *>(blob.data());
    const auto clip = [](u64 x) { return (u32)std::min<u64>(x, 0xFFFFFFFFu); };
    for (u32 x = 0; x < pl.n_out; ++x) {
        const FastDiv d = csgn_fastdiv_make((u32)pl.T[x]);
        t->Tpre[x + 1] = t->Tpre[x] + pl.T[x];
        t->T[x] = d.d;
        t->Tm[x] = d.magic;
        t->Ts[x] = d.shift;
    }
    for (u32 x = 0; x <= kMaxPlanes; ++x) {
        t->Tpre[x] = t->Tpre[std::min(x, pl.n_out)];
        t->efirst[x] = pl.efirst[std::min(x, pl.n_out)];
    }
    for (u32 i = 0; i < pl.wa + pl.wb; ++i) {
        const u64 terms = i < pl.wa ? pl.ta[i] : pl.tb[i - pl.wa];
        t->tin[i] = clip(terms);
        t->opre[i + 1] = clip((u64)t->opre[i] + t->tin[i]);
        if (i >= pl.wa) {
            const FastDiv d = csgn_fastdiv_make(t->tin[i]);
            t->tbm[i - pl.wa] = d.magic;
            t->tbs[i - pl.wa] = d.shift;
        }
    }
    blob.insert(blob.end(), pl.start.begin(), pl.start.end());
    blob.insert(blob.end(), pl.lr.begin(), pl.lr.end());
    herr = hipMalloc(&pl.d_tab, blob.size() * sizeof(u32));
    if (herr == hipSuccess)
        herr = hipMemcpy(pl.d_tab, blob.data(), blob.size() * sizeof(u32), hipMemcpyHostToDevice);
    if (herr != hipSuccess) {
        uint_bilinear_free(pl);
        return CSGN_ERR_HIP;
    }
    return CSGN_OK;
}

void uint_bilinear_free(BilinearPlan &pl)
{
    if (pl.d_tab)
        (void)hipFree(pl.d_tab);
    pl.d_tab = nullptr;
}

void uint_bilinear_launches(const BilinearPlan &pl, u64 n_bits, u64 batch, u64 *plan)
{
    const u64 dL = (n_bits + 63) / 64;
    const BilinearCut c = bilinear_cut(pl, dL, batch, dL % 2 == 0, launch_blocks());
    plan[0] = dL % 2 == 0 ? 16 : 8;
    plan[1] = c.units;
    plan[2] = c.G;
    plan[3] = batch ? c.tiles : 0;
    plan[4] = c.per_tile;
    plan[5] = batch ? c.launches : 0;
    plan[6] = batch ? c.first_blocks : 0;
    plan[7] = c.groups;
    plan[8] = c.staged ? 1 : 0;
    plan[9] = c.chunk[0];
    plan[10] = c.op_units;
    plan[11] = kStageBytes;
}

hipError_t uint_bilinear(const BilinearPlan &pl, u64 n_bits, u64 batch, const u64 *const *a, const u64 *const *b,
                         u64 *const *out, hipStream_t s)
{
    if (batch == 0)
        return hipSuccess;
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(a, pl.wa), ptr_array(b, pl.wb), ptr_array(out, pl.n_out));
    const BilinearCut c = bilinear_cut(pl, dL, batch, wide, launch_blocks());
    if (wide)
        return c.staged ? bilinear_kernel<unit16, true>(pl, n_bits, batch, a, b, out, c, s)
                        : bilinear_kernel<unit16, false>(pl, n_bits, batch, a, b, out, c, s);
    return c.staged ? bilinear_kernel<unit8, true>(pl, n_bits, batch, a, b, out, c, s)
                    : bilinear_kernel<unit8, false>(pl, n_bits, batch, a, b, out, c, s);
}

} // namespace csgn
