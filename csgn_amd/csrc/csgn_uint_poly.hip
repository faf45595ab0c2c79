// csgn_uint_poly.hip -- a PUBLIC polynomial over F2 of bit-sliced encrypted planes, every output plane in one launch:
// SHA-2's Ch and Maj, Keccak's chi, a Simon round, a full adder's carry, a k-way AND, an S-box ANF on wide words.
// Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.39.
//
// The definition (include/csgn_hip.h, csgn_uint_poly): output plane x is the left-nested sum (the reference's
// operator+, concatenation) of its monomials in the order given, then ONE where bit x of the public constant is set; a
// monomial is the left-nested product (the reference's operator*: all pairs of terms, the left term slow) of 1 to 8
// input planes; a plane of no monomial is the one-term constant.  An element of an output plane is a sequence of
// SEGMENTS, one per monomial, of (the product of its factors' term counts) terms each, and at most one constant term; a
// term is the AND of one term of every factor, the first factor's term index slowest.
//
// One lane writes one unit at a time and WALKS, as in k_uint_bilinear: the grid is tile-major, a tile is
// G elements of all output planes, the stream inside a tile is (plane, element, term, unit) with the unit fastest, and
// workgroup s of a tile's S walks the positions [s * chunk, (s + 1) * chunk), 256 consecutive units a step.  A lane
// decodes its position:
//   - the plane, by a search of the tile's plane prefix (LDS, 6 probes), then element and term by the plane's FastDiv;
//   - the monomial: one fast division when every input plane has one term count and every monomial one degree (eq),
//     else a binary search of the plane's first-term table (poly_monomial: the records in LDS when the plan has at most
//     kLdsMonomials monomials, else through the vector cache);
//   - the factors' term indices by mixed-radix division (poly_split): none when every plane has one term, one shared
//     FastDiv when all counts are equal, else the planes' FastDivs from the plan;
//   the host's decode by position, csgn_uint_poly_decode, calls the same two functions.
// A monomial's record is one aligned 16-byte read: first term, degree, eight one-byte factors.  All loads of a term's
// factors are issued before the first AND.  STAGED shapes (one element's input planes fit kStageBytes of LDS and the
// form writes at least kStageMinRatio times what it reads) copy a tile's operand units to LDS once a workgroup; other
// shapes read from memory.  No scratch.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>
#include <vector>

namespace csgn {

namespace {

constexpr u32 kMaxIn = kPolyMaxIn, kMaxOut = kPolyMaxOut, kMaxDeg = kPolyMaxDegree;

// Compile-time budgets, not knobs: tools/bench_uint_poly.py builds private copies of the library with other values to
// time them.  The values k_uint_bilinear ships.
#ifndef CSGN_POLY_STAGE_BYTES
#define CSGN_POLY_STAGE_BYTES 16384
#endif
#ifndef CSGN_POLY_TILE_UNITS
#define CSGN_POLY_TILE_UNITS 262144
#endif
#ifndef CSGN_POLY_STAGE_RATIO
#define CSGN_POLY_STAGE_RATIO 4
#endif
#ifndef CSGN_POLY_MIN_CHUNK
#define CSGN_POLY_MIN_CHUNK 2048
#endif
constexpr u64 kStageBytes = CSGN_POLY_STAGE_BYTES;       // LDS for a tile's operand units
constexpr u64 kTileUnits = CSGN_POLY_TILE_UNITS;         // units an unstaged tile writes, over all planes
constexpr u64 kStageRatio = CSGN_POLY_STAGE_RATIO;       // a staged workgroup writes at least this many times its LDS copy
constexpr u64 kStageMinRatio = 2;                        // written / read per element below which staging cannot pay
constexpr u64 kMinChunk = CSGN_POLY_MIN_CHUNK;           // units a workgroup walks at least; a multiple of 256
constexpr u64 kMaxTile = 1ull << 31;                     // units of one tile of one plane group: positions stay u32
constexpr u32 kLdsMonomials = 512;                       // monomials whose records a workgroup keeps in LDS (8 KiB)
static_assert(kMinChunk % 256 == 0 && kMinChunk >= 256, "a workgroup walks whole steps");
static_assert(kStageBytes % 16 == 0 && kStageBytes + 16 * kLdsMonomials + 4096 <= 65536, "static LDS");
static_assert(kMaxIn <= 256, "a factor is one byte of a monomial's record");

// The plan's tables on the device, then one uint4 record per monomial.
struct alignas(16) PolyTab {
    u64 Tpre[kMaxOut + 1];                    // terms per element of the output planes before x
    u32 T[kMaxOut], Tm[kMaxOut], Ts[kMaxOut]; // T_x and its FastDiv
    u32 mfirst[kMaxOut + 1];
    u32 tin[kMaxIn], tm[kMaxIn], ts[kMaxIn];  // terms per element of the input planes (saturating) and their FastDiv
    u32 opre[kMaxIn + 1];                     // terms per element of the input planes before i (saturating)
};
static_assert(sizeof(PolyTab) % 16 == 0, "the records behind the tables are 16-byte aligned");

// By value in the kernel arguments (2.7 KB of the 4 KB limit).
//     in[i]     input plane i's first element of this launch
//     out[x]    output plane x's first element of this launch
struct PolyArgs {
    const void *in[kMaxIn];
    void *out[kMaxOut];
    const PolyTab *tab;
    const uint4 *rec;         // per monomial: x its first term in its plane, y its degree, z and w its factors
    u64 constant, last_mask;
    u32 nin, nmon;            // input planes; monomials of the plan
    u32 p0, np;               // the output planes of this launch are p0 .. p0 + np - 1
    u32 U, G, ne;             // units per term, elements per tile, elements of this launch
    u32 chunk;                // units a workgroup walks
    u32 eq;                   // one term count, one degree: the monomial by division
    u32 tmode;                // factor terms: 0 every plane has one term, 1 one shared divisor, 2 the planes' divisors
    u32 lds_tab;              // nmon <= kLdsMonomials
    u32 xcd;
    FastDiv dS, dU, dMT, dt;  // workgroups per tile; U; tin[0]^deg (eq only); tin[0] (tmode 1 only)
};
static_assert(sizeof(PolyArgs) <= 4096, "kernel arguments past the 4 KB limit");

// The decode by position, shared by the kernel and csgn_uint_poly_decode.  The monomial of term `term` of a plane of
// nmon monomials and mterms monomial terms (the plane's constant not counted): nmon when term is at or past mterms (the
// constant), else the monomial, with q the term inside it.  eq: every monomial has dMT.d terms.  Otherwise start(i) is
// the first term of monomial i, start(0) = 0, strictly ascending (a monomial has a term at least): at most 18 probes.
template <typename Start>
__host__ __device__ inline u32 poly_monomial(u32 nmon, u32 mterms, u32 term, bool eq, const FastDiv &dMT, Start start,
                                             u32 &q)
{
    q = 0;
    if (term >= mterms)
        return nmon;
    if (eq) {
        const u32 m = csgn_fastdiv(term, dMT);
        q = term - m * dMT.d;
        return m;
    }
    u32 lo = 0, hi = nmon;
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

// factor j of a record, j < 8
__host__ __device__ inline u32 poly_factor(u32 z, u32 w, u32 j) { return ((j < 4u ? z : w) >> (8u * (j & 3u))) & 0xFFu; }

// term q of ((p_f0 * p_f1) * ...) * p_f(deg-1): the first factor's term is slowest.  div(j) is the FastDiv of factor
// j's term count, asked for j = deg - 1 .. 1 only; tmode 0 divides nothing.  idx[j] < the count of factor j; 0 past deg.
template <typename Div>
__host__ __device__ inline void poly_split(u32 q, u32 deg, u32 tmode, Div div, u32 (&idx)[kMaxDeg])
{
#pragma unroll
    for (u32 j = 0; j < kMaxDeg; ++j)
        idx[j] = 0u;
    if (tmode == 0u)
        return;
#pragma unroll
    for (u32 j = kMaxDeg - 1u; j >= 1u; --j)
        if (j < deg) {
            const FastDiv d = div(j);
            const u32 hi = csgn_fastdiv(q, d);
            idx[j] = q - hi * d.d;
            q = hi;
        }
    idx[0] = q;
}

template <typename Unit, bool Staged>
__global__ void __launch_bounds__(256) k_uint_poly(PolyArgs g)
{
    __shared__ u32 s_pre[kMaxOut + 1];                    // first term of plane p0 + q in this tile; [np]: the tile's terms
    __shared__ u32 s_opre[kMaxIn + 1];                    // staged: first LDS unit of input plane i; [nin]: the units
    __shared__ uint4 s_rec[kLdsMonomials];
    __shared__ Unit s_op[Staged && kStageBytes ? kStageBytes / sizeof(Unit) : 1];   // kStageBytes = 0: nothing is staged
    const PolyTab *__restrict__ t = g.tab;
    const u32 bid = g.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const u32 tile = csgn_fastdiv(bid, g.dS), s = bid - tile * g.dS.d;
    const u32 e0 = tile * g.G, ge = min(g.G, g.ne - e0), U = g.U, nin = g.nin;
    const u64 base = t->Tpre[g.p0];
    const u32 total = ge * (u32)(t->Tpre[g.p0 + g.np] - base) * U;   // units of this tile, at most kMaxTile
    const u32 lo = s * g.chunk;                           // below 2^31 + 2^28: s < S and S * chunk < G * units + 256 * S
    if (lo >= total)                                      // the last tile is short: uniform, before any barrier
        return;
    const u32 hi = min(lo + g.chunk, total);
    if (threadIdx.x <= g.np)
        s_pre[threadIdx.x] = ge * (u32)(t->Tpre[g.p0 + threadIdx.x] - base);
    if (Staged)
        for (u32 i = threadIdx.x; i <= nin; i += 256u)    // nin + 1 values, up to 257
            s_opre[i] = ge * t->opre[i] * U;
    if (g.lds_tab)
        for (u32 i = threadIdx.x; i < g.nmon; i += 256u)
            s_rec[i] = g.rec[i];
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
        const u32 mf = t->mfirst[p], nmon = t->mfirst[p + 1u] - mf;
        const bool one = (g.constant >> p) & 1ull;
        const u32 mterms = T - ((nmon == 0u || one) ? 1u : 0u);
        u32 qq;
        const u32 m = g.lds_tab ? poly_monomial(nmon, mterms, term, g.eq, g.dMT, [&](u32 i) { return s_rec[mf + i].x; }, qq)
                                : poly_monomial(nmon, mterms, term, g.eq, g.dMT, [&](u32 i) { return g.rec[mf + i].x; }, qq);
        Unit w;
        if (m >= nmon) {
            w = one ? one_unit(Unit(), k, U, g.last_mask) : zero_unit(Unit());
        } else {
            const uint4 r = g.lds_tab ? s_rec[mf + m] : g.rec[mf + m];   // mf + m < the plan's monomials
            const u32 deg = r.y;                                       // 1 .. 8; every factor below nin
            u32 idx[kMaxDeg];
            poly_split(qq, deg, g.tmode, [&](u32 j) {
                const u32 f = poly_factor(r.z, r.w, j);
                return g.tmode == 1u ? g.dt : FastDiv{t->tin[f], t->tm[f], t->ts[f]};
            }, idx);
            Unit v[kMaxDeg];
#pragma unroll
            for (u32 j = 0; j < kMaxDeg; ++j)                          // every load before the first AND
                if (j < deg) {
                    const u32 f = poly_factor(r.z, r.w, j);
                    const u32 tf = g.tmode == 0u ? 1u : t->tin[f];     // idx[j] < tf
                    if (Staged)
                        v[j] = s_op[s_opre[f] + (el * tf + idx[j]) * U + k];
                    else
                        v[j] = reinterpret_cast<const Unit *>(g.in[f])[(((u64)e0 + el) * tf + idx[j]) * U + k];
                }
            w = v[0];
#pragma unroll
            for (u32 j = 1; j < kMaxDeg; ++j)
                if (j < deg)
                    w = w & v[j];
        }
        unit_store<Unit, true>(reinterpret_cast<Unit *>(g.out[p]) + (((u64)e0 * T + off) * U + k), w);
    }
}

// ------------------------------------------------------------------------------ the definition on the host

// T of one plane; 0: invalid or 2^62 terms or more.  rec (optional) takes every monomial's record while the plane stays
// below 2^31 terms.
u64 poly_plane(u64 n_in, const u64 *terms, u64 n_mon, const u64 *mfirst, const u64 *factor, int constant_bit,
               std::vector<u32> *rec)
{
    if (n_in < 1 || n_in > kMaxIn || !terms || (n_mon && (!mfirst || !factor)) || (constant_bit != 0 && constant_bit != 1))
        return 0;
    for (u64 i = 0; i < n_in; ++i)
        if (terms[i] == 0 || terms[i] >= kTermLimit)
            return 0;
    u64 T = 0;
    for (u64 m = 0; m < n_mon; ++m) {
        if (mfirst[m + 1] < mfirst[m])
            return 0;
        const u64 deg = mfirst[m + 1] - mfirst[m];
        if (deg < 1 || deg > kMaxDeg)
            return 0;
        u64 p = 1;
        u32 z[2] = {0, 0};
        for (u64 j = 0; j < deg; ++j) {
            const u64 f = factor[mfirst[m] + j];
            if (f >= n_in || !term_mul(p, terms[f], p))
                return 0;
            z[j / 4] |= (u32)f << (8 * (j % 4));
        }
        if (rec && T < (1ull << 31)) {
            rec->push_back((u32)T);
            rec->push_back((u32)deg);
            rec->push_back(z[0]);
            rec->push_back(z[1]);
        }
        T += p;
        if (T >= kTermLimit)
            return 0;
    }
    if (constant_bit || n_mon == 0)
        ++T;
    return T < kTermLimit ? T : 0;
}

// How a call is cut (csgn_uint_poly_launches reports it; the launcher follows it).  A plane GROUP is a run of output
// planes of which one tile stays within kMaxTile units: one group for every shape but those of which ONE element of all
// planes does not, which take G = 1 and a launch sequence per group.
struct PolyCut {
    u32 U = 0, G = 0, groups = 0;
    bool staged = false;
    u64 units = 0, op_units = 0;          // per element: all output planes; all input planes
    u64 tiles = 0, per_tile = 0, launches = 0, first_blocks = 0;
    u32 gfirst[kMaxOut + 1] = {};         // group i is the planes gfirst[i] .. gfirst[i + 1] - 1
    u32 S[kMaxOut] = {};                  // its workgroups per tile
    u32 chunk[kMaxOut] = {};              // the units each of them walks: the tile in S even parts, whole steps
    u64 tpl[kMaxOut] = {};                // its tiles per launch
};

PolyCut poly_cut(const PolyPlan &pl, u64 dL, u64 batch, bool wide, u64 max_blocks)
{
    PolyCut c;
    const u64 ub = wide ? 16 : 8;
    c.U = (u32)(wide ? dL / 2 : dL);
    for (u32 x = 0; x < pl.n_out; ++x)
        c.units += pl.T[x] * c.U;
    u64 op_terms = 0;
    for (u32 i = 0; i < pl.n_in; ++i)
        op_terms += std::min<u64>(pl.tin[i], 1ull << 32);
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

u32 poly_tmode(const PolyPlan &pl) { return pl.teq ? (pl.tin[0] == 1 ? 0u : 1u) : 2u; }

template <typename Unit, bool Staged>
hipError_t poly_kernel(const PolyPlan &pl, u64 n_bits, u64 batch, const u64 *const *in, u64 *const *out, const PolyCut &c,
                       hipStream_t s)
{
    PolyArgs g = {};
    const u32 U = c.U;
    g.tab = reinterpret_cast<const PolyTab *>(pl.d_tab);
    g.rec = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(pl.d_tab) + sizeof(PolyTab));
    g.constant = pl.constant;
    g.last_mask = last_word_mask(n_bits);
    g.nin = pl.n_in;
    g.nmon = (u32)(pl.rec.size() / 4);
    g.U = U;
    g.G = c.G;
    g.eq = pl.eq ? 1u : 0u;
    g.tmode = poly_tmode(pl);
    g.lds_tab = g.nmon <= kLdsMonomials ? 1u : 0u;
    g.dU = csgn_fastdiv_make(U);
    u64 mt = 1;
    for (u32 j = 0; pl.eq && j < pl.deg; ++j)
        mt *= pl.tin[0];
    g.dMT = csgn_fastdiv_make((u32)mt);
    g.dt = csgn_fastdiv_make(pl.teq ? (u32)pl.tin[0] : 1u);
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
            for (u32 i = 0; i < pl.n_in; ++i)
                g.in[i] = reinterpret_cast<const Unit *>(in[i]) + e0 * pl.tin[i] * U;
            for (u32 x = j; x < k; ++x)
                g.out[x] = reinterpret_cast<Unit *>(out[x]) + e0 * pl.T[x] * U;
            g.ne = (u32)ne;
            g.xcd = stream_xcd(ne * units);
            k_uint_poly<Unit, Staged><<<dim3((u32)(nt * c.S[gi])), 256, 0, s>>>(g);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

// teq, eq and deg of a shape whose records are `rec`
void poly_modes(u64 n_in, const u64 *terms, const std::vector<u32> &rec, bool &teq, bool &eq, u32 &deg)
{
    teq = std::all_of(terms, terms + n_in, [&](u64 x) { return x == terms[0]; }) && terms[0] < (1ull << 31);
    eq = false;
    deg = 0;
    if (!teq || rec.empty())
        return;
    for (size_t m = 0; m < rec.size(); m += 4)
        if (rec[m + 1] != rec[1])
            return;
    u64 mt = 1;
    for (u32 j = 0; j < rec[1]; ++j)
        if (!term_mul(mt, terms[0], mt))
            return;
    if (mt >= (1ull << 31))
        return;
    eq = true;
    deg = rec[1];
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_poly_terms(u64 n_in, const u64 *terms, u64 n_monomials, const u64 *mfirst, const u64 *factor, int constant_bit)
{
    return poly_plane(n_in, terms, n_monomials, mfirst, factor, constant_bit, nullptr);
}

bool uint_poly_decode(u64 n_in, const u64 *terms, u64 n_monomials, const u64 *mfirst, const u64 *factor, int constant_bit,
                      u64 q, u64 *monomial, u64 *factor_terms)
{
    std::vector<u32> rec;
    if (n_monomials > kPolyMaxMonomials || !monomial || !factor_terms)
        return false;
    const u64 T = poly_plane(n_in, terms, n_monomials, mfirst, factor, constant_bit, &rec);
    if (T == 0 || T >= (1ull << 31) || q >= T)
        return false;
    bool teq, eq;
    u32 deg;
    poly_modes(n_in, terms, rec, teq, eq, deg);
    const u32 tmode = teq ? (terms[0] == 1 ? 0u : 1u) : 2u;
    u64 mt = 1;
    for (u32 j = 0; eq && j < deg; ++j)
        mt *= terms[0];
    const u32 nmon = (u32)n_monomials, extra = (nmon == 0 || constant_bit) ? 1u : 0u;
    u32 qq;
    const u32 m = poly_monomial(nmon, (u32)T - extra, (u32)q, eq, csgn_fastdiv_make((u32)mt),
                                [&](u32 i) { return rec[4 * i]; }, qq);
    std::fill(factor_terms, factor_terms + kMaxDeg, 0);
    if (m >= nmon) {                                      // the plane's constant
        *monomial = constant_bit ? n_monomials : n_monomials + 1;
        return true;
    }
    u32 idx[kMaxDeg];
    poly_split(qq, rec[4 * m + 1], tmode,
               [&](u32 j) { return csgn_fastdiv_make((u32)terms[poly_factor(rec[4 * m + 2], rec[4 * m + 3], j)]); }, idx);
    *monomial = m;
    std::copy(idx, idx + kMaxDeg, factor_terms);
    return true;
}

int uint_poly_shape(u64 n_in, const u64 *terms, u64 n_out, const u64 *first, const u64 *mfirst, const u64 *factor,
                    u64 constant, PolyPlan &pl)
{
    pl = PolyPlan();
    if (n_in < 1 || n_in > kMaxIn || n_out < 1 || n_out > kMaxOut || !terms || !first || first[0] != 0 ||
        (n_out < 64 && (constant >> n_out) != 0))
        return CSGN_ERR_INVALID;
    for (u64 x = 0; x < n_out; ++x)
        if (first[x + 1] < first[x])
            return CSGN_ERR_INVALID;
    if (first[n_out] && (!mfirst || !factor))
        return CSGN_ERR_INVALID;
    if (first[n_out] > kPolyMaxMonomials)
        return CSGN_ERR_UNSUPPORTED;
    pl.n_in = (u32)n_in;
    pl.n_out = (u32)n_out;
    pl.constant = constant;
    std::copy(terms, terms + n_in, pl.tin);
    int rc = CSGN_OK;
    for (u64 x = 0; x < n_out; ++x) {
        pl.mfirst[x] = (u32)first[x];
        pl.rec.resize(4 * first[x]);                      // a plane past 2^31 terms leaves monomials out: the plan is refused
        pl.T[x] = poly_plane(n_in, terms, first[x + 1] - first[x], mfirst ? mfirst + first[x] : nullptr, factor,
                             (int)((constant >> x) & 1u), &pl.rec);
        if (pl.T[x] == 0)
            return CSGN_ERR_INVALID;
        if (pl.T[x] >= (1ull << 31))
            rc = CSGN_ERR_UNSUPPORTED;
    }
    pl.mfirst[n_out] = (u32)first[n_out];
    pl.rec.resize(4 * first[n_out]);
    poly_modes(n_in, terms, pl.rec, pl.teq, pl.eq, pl.deg);
    return rc;
}

int uint_poly_create(PolyPlan &pl, hipError_t &herr)
{
    std::vector<u32> blob(sizeof(PolyTab) / sizeof(u32));
    PolyTab *t = reinterpret_cast<PolyTab *>(blob.data());
    const auto clip = [](u64 x) { return (u32)std::min<u64>(x, 0xFFFFFFFFu); };
    for (u32 x = 0; x < pl.n_out; ++x) {
        const FastDiv d = csgn_fastdiv_make((u32)pl.T[x]);
        t->Tpre[x + 1] = t->Tpre[x] + pl.T[x];
        t->T[x] = d.d;
        t->Tm[x] = d.magic;
        t->Ts[x] = d.shift;
    }
    for (u32 x = 0; x <= kMaxOut; ++x) {
        t->Tpre[x] = t->Tpre[std::min(x, pl.n_out)];
        t->mfirst[x] = pl.mfirst[std::min(x, pl.n_out)];
    }
    for (u32 i = 0; i < pl.n_in; ++i) {
        const FastDiv d = csgn_fastdiv_make(clip(pl.tin[i]));
        t->tin[i] = d.d;
        t->tm[i] = d.magic;
        t->ts[i] = d.shift;
        t->opre[i + 1] = clip((u64)t->opre[i] + t->tin[i]);
    }
    blob.insert(blob.end(), pl.rec.begin(), pl.rec.end());
    herr = hipMalloc(&pl.d_tab, blob.size() * sizeof(u32));
    if (herr == hipSuccess)
        herr = hipMemcpy(pl.d_tab, blob.data(), blob.size() * sizeof(u32), hipMemcpyHostToDevice);
    if (herr != hipSuccess) {
        uint_poly_free(pl);
        return CSGN_ERR_HIP;
    }
    return CSGN_OK;
}

void uint_poly_free(PolyPlan &pl)
{
    if (pl.d_tab)
        (void)hipFree(pl.d_tab);
    pl.d_tab = nullptr;
}

void uint_poly_launches(const PolyPlan &pl, u64 n_bits, u64 batch, u64 *plan)
{
    const u64 dL = (n_bits + 63) / 64;
    const PolyCut c = poly_cut(pl, dL, batch, dL % 2 == 0, launch_blocks());
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
    plan[12] = pl.eq ? 1 : 0;
    plan[13] = poly_tmode(pl);
}

hipError_t uint_poly(const PolyPlan &pl, u64 n_bits, u64 batch, const u64 *const *in, u64 *const *out, hipStream_t s)
{
    if (batch == 0)
        return hipSuccess;
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(in, pl.n_in), ptr_array(out, pl.n_out));
    const PolyCut c = poly_cut(pl, dL, batch, wide, launch_blocks());
    if (wide)
        return c.staged ? poly_kernel<unit16, true>(pl, n_bits, batch, in, out, c, s)
                        : poly_kernel<unit16, false>(pl, n_bits, batch, in, out, c, s);
    return c.staged ? poly_kernel<unit8, true>(pl, n_bits, batch, in, out, c, s)
                    : poly_kernel<unit8, false>(pl, n_bits, batch, in, out, c, s);
}

} // namespace csgn
