// csgn_uint_plain_sum.hip -- sums (the reference's operator+, concatenation) of comparisons of ONE bit-sliced encrypted
// integer against PUBLIC constants, every output plane in one launch: ranges, sets, step functions, sparse tables.
// Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h and csgn_chain.h, design notes in DESIGN.md §4.37.
//
// The definition (include/csgn_hip.h, csgn_uint_plain_sum): output plane x is the left-nested sum of its entries'
// csgn_uint_plain results, in order, then ONE where bit x of the public constant is set; a plane of no entry is the
// one-term constant.  Nothing is multiplied beyond what each comparison multiplies, so an element of an output plane is
// a sequence of SEGMENTS, one per entry, each decoded exactly as k_uint_plain decodes its whole output (csgn_device.h's
// chain_run: the odometer of DESIGN §4.14), and at most one constant term.
//
// A lane item is k_uint_plain's: (element, plane, run of up to 16 consecutive terms, unit).  Runs are cut from each
// entry's first term, so no run straddles two entries and the cut, the key of the levels below it and the radix-1
// factors stay one entry's; the plane's constant is a run of its own.  A workgroup belongs to one plane (found by a
// uniform search of this launch's per-plane workgroup prefix), and finds the entries of its first and last item by a
// uniform search of the plane's run prefix (word R_RUN0 of the level records).  When they are the same entry -- every
// large comparison: an entry of 4096 terms or more fills whole workgroups -- the entry index is uniform and the level
// record is read with scalar loads, as k_uint_plain reads its arguments.  Otherwise each lane searches the run prefix
// for its own entry (9 probes for 300 entries) and reads the record through the vector cache.
//
// The level records (one per entry: base, cut, flags, T, the radix-1 mask, the first run and term, then pend[] and the
// FastDivs of the w levels) are built and uploaded once per plan, csgn_uint_plain_sum_create; a call allocates nothing.
// DEPARTURE from the sketch in the issue: the records of a workgroup's entry range are NOT staged in LDS.  With 8-byte
// units and one word a term a workgroup can span 256 entries, and a w = 64 record is 1056 bytes: the range does not fit
// LDS at the widths where it matters, a second record format would be needed for it, and the records a workgroup
// touches are consecutive words that stay in the vector L1 / L2.  No LDS, no scratch.
#include "csgn_chain.h"
#include "csgn_hip.h"

#include <algorithm>
#include <vector>

namespace csgn {

namespace {

constexpr u32 kMaxPlanes = kPlainSumMaxPlanes;
constexpr u32 kRun = 16;              // terms per lane, k_uint_plain's

// A level record: kRecHeader words, then pend[w], and the FastDivs' d[w], magic[w], shift[w].
enum : u32 { R_BASE, R_CUT, R_FLAGS, R_T, R_UNIT_LO, R_UNIT_HI, R_RUN0, R_TERM0, kRecHeader };
constexpr u32 kFlagZero = 1u, kFlagNeg = 2u;

// By value in the kernel arguments (3.2 KB of the 4 KB limit; uniform indices are scalar loads).
//     plane[j], t[j]   input plane j's first element of this launch, its terms per element
//     out[x], T[x]     output plane x's first element of this launch, its terms per element
//     runs[x]          runs per element of plane x, the constant's included;  IPE.d[x] = runs[x] * U lane items
//     efirst[x]        plane x's first entry (efirst[n_out]: entries of the plan)
//     bfirst[q]        first workgroup of plane p0 + q in this launch (bfirst[np]: the grid)
struct SumArgs {
    const void *plane[kChainMaxLevels];
    void *out[kMaxPlanes];
    u32 t[kChainMaxLevels];
    u32 T[kMaxPlanes];
    u32 runs[kMaxPlanes];
    u32 efirst[kMaxPlanes + 1];
    u32 bfirst[kMaxPlanes + 1];
    FastDivTable<kMaxPlanes> IPE;
    const u32 *rec;
    u64 constant, last_mask;
    u32 w, stride;            // input planes; words of a record
    u32 p0, np;               // the output planes of this launch are p0 .. p0 + np - 1
    u32 U, ne;                // units per term, elements of this launch
    u32 xcd;
    FastDiv dU;
};
static_assert(sizeof(SumArgs) <= 4096, "kernel arguments past the 4 KB limit");

// The entry search, shared by the kernel (positions in runs) and csgn_uint_plain_sum_decode (positions in terms): the
// entry of position q among nent entries whose first positions start(0) = 0 < start(1) < ... ascend and end at `end`;
// nent when q is at or past `end` (the plane's constant).
template <typename Start>
__host__ __device__ inline u32 sum_entry(u32 nent, u32 end, u32 q, Start start)
{
    if (q >= end)
        return nent;
    u32 lo = 0, hi = nent;
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (start(mid) <= q)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// One entry's chain as chain_term / chain_walk_each / chain_run read it: the planes and their terms of the call, and
// the record's level tables.
struct SumRad {
    const u32 *d, *magic, *shift;
    __host__ __device__ FastDiv at(u32 j) const { return FastDiv{d[j], magic[j], shift[j]}; }
};
struct SumView {
    const void *const *plane;
    const u32 *t;
    const u32 *pend;
    SumRad rad;
    u32 base, U;
};

__host__ __device__ inline SumView sum_view(const void *const *plane, const u32 *t, const u32 *rec, u32 w, u32 U)
{
    const u32 *lv = rec + kRecHeader;
    return SumView{plane, t, lv, SumRad{lv + w, lv + 2u * w, lv + 3u * w}, rec[R_BASE], U};
}

// unit k of run `run` of element e of plane p, the run inside entry `ent` of the plane's nent (ent == nent: the constant)
template <typename Unit>
__device__ inline void sum_item(const SumArgs &a, u32 p, u32 ent, u32 nent, u32 e, u32 run, u32 k)
{
    const Unit one = one_unit(Unit(), k, a.U, a.last_mask);
    Unit *out = reinterpret_cast<Unit *>(a.out[p]);
    const u32 T = a.T[p];
    if (ent >= nent) {                                    // ONE, or the ZERO of a plane with no entry
        const Unit v = ((a.constant >> p) & 1ull) ? one : zero_unit(Unit());
        unit_store<Unit, true>(out + ((u64)e * T + (T - 1u)) * a.U + k, v);
        return;
    }
    const u32 *r = a.rec + (u64)(a.efirst[p] + ent) * a.stride;
    const SumView v = sum_view(a.plane, a.t, r, a.w, a.U);
    const u32 Te = r[R_T], R = min(Te, kRun), flags = r[R_FLAGS];
    const u32 t0 = (run - r[R_RUN0]) * R, nt = min(R, Te - t0);
    const u64 unit = (u64)r[R_UNIT_LO] | ((u64)r[R_UNIT_HI] << 32);
    Unit *o = out + ((u64)e * T + r[R_TERM0] + t0) * a.U + k;
    chain_run<Unit>(v, a.w - 1u, r[R_CUT], flags & kFlagZero, flags & kFlagNeg, Te, unit, (u64)e * a.U, k, one, t0, nt, o);
}

template <typename Unit>
__global__ void __launch_bounds__(256) k_uint_plain_sum(SumArgs a)
{
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    u32 q = 0, hi = a.np;                                 // the plane of this workgroup: bfirst[q] <= bid < bfirst[q + 1]
    while (hi - q > 1u) {
        const u32 mid = (q + hi) >> 1;
        if (a.bfirst[mid] <= bid)
            q = mid;
        else
            hi = mid;
    }
    const u32 p = a.p0 + q;
    const FastDiv dipe = a.IPE.at(p);
    const u32 total = a.ne * dipe.d;                      // lane items of plane p in this launch, below 2^32
    const u32 g0 = (bid - a.bfirst[q]) * 256u;            // the workgroup's first item, below total
    const u32 nent = a.efirst[p + 1u] - a.efirst[p];
    const u32 extra = (nent == 0u || ((a.constant >> p) & 1ull)) ? 1u : 0u;
    const u32 eruns = a.runs[p] - extra;                  // the runs of the entries
    const u32 *rec0 = a.rec + (u64)a.efirst[p] * a.stride;
    auto start = [&](u32 i) { return rec0[(u64)i * a.stride + R_RUN0]; };
    // the entries of the workgroup's first and last item (uniform)
    const u32 gl = min(g0 + 255u, total - 1u);
    const u32 ef = csgn_fastdiv(g0, dipe), el = csgn_fastdiv(gl, dipe);
    u32 ent0 = 0;
    bool single = nent + extra == 1u;                     // items of two elements: one entry only if the plane is one
    if (ef == el) {
        ent0 = sum_entry(nent, eruns, csgn_fastdiv(g0 - ef * dipe.d, a.dU), start);
        single = ent0 == sum_entry(nent, eruns, csgn_fastdiv(gl - el * dipe.d, a.dU), start);
    }
    const u32 g = g0 + threadIdx.x;
    if (g >= total)
        return;
    const u32 e = csgn_fastdiv(g, dipe), rem = g - e * dipe.d;
    const u32 run = csgn_fastdiv(rem, a.dU), k = rem - run * a.U;
    if (single)
        sum_item<Unit>(a, p, ent0, nent, e, run, k);      // a uniform entry: the record by scalar loads
    else
        sum_item<Unit>(a, p, sum_entry(nent, eruns, run, start), nent, e, run, k);
}

// ------------------------------------------------------------------------------ the definition on the host

// one entry's record appended to rec; false: csgn_uint_plain_terms refuses it
bool sum_record(int cmp, u64 w, u64 k, const u64 *t, u64 run0, u64 term0, std::vector<u32> *rec, u64 &T, u64 &runs)
{
    PlainShape ps;
    if (!plain_shape(cmp, w, k, t, ps))
        return false;
    T = ps.T;
    const u64 R = std::min<u64>(T, kRun);
    runs = (T + R - 1) / R;
    if (!rec || T >= (1ull << 31))
        return true;
    struct {
        u32 t[kChainMaxLevels], pend[kChainMaxLevels];
        FastDivTable<kChainMaxLevels> rad;
    } lv;
    chain_fill(ps.zero ? nullptr : &ps.c, ps.w, ps.w, t, lv);
    const u64 unit = plain_radix1(ps, t);
    const u32 header[kRecHeader] = {ps.c.base, plain_cut(ps, t, (u32)R), (ps.zero ? kFlagZero : 0u) | (ps.neg ? kFlagNeg : 0u),
                                    (u32)T, (u32)unit, (u32)(unit >> 32), (u32)run0, (u32)term0};
    rec->insert(rec->end(), header, header + kRecHeader);
    rec->insert(rec->end(), lv.pend, lv.pend + w);
    rec->insert(rec->end(), lv.rad.d, lv.rad.d + w);
    rec->insert(rec->end(), lv.rad.magic, lv.rad.magic + w);
    rec->insert(rec->end(), lv.rad.shift, lv.rad.shift + w);
    return true;
}

// T of one plane, its runs and (rec != nullptr) its entries' records; 0: invalid or 2^62 terms or more.  Records stop
// being written once the plane reaches 2^31 terms (no plan holds such a plane).
u64 sum_plane(u64 w, const u64 *t, u64 n_entries, const int *cmp, const u64 *k, int constant_bit, std::vector<u32> *rec,
              u64 &runs)
{
    runs = 0;
    if ((constant_bit != 0 && constant_bit != 1) || (n_entries && (!cmp || !k)) || !chain_arguments(w, 0, t))
        return 0;
    u64 T = 0;
    for (u64 i = 0; i < n_entries; ++i) {
        u64 Te, re;
        if (!sum_record(cmp[i], w, k[i], t, runs, T, T < (1ull << 31) ? rec : nullptr, Te, re))
            return 0;
        T += Te;
        runs += re;
        if (T >= kTermLimit)
            return 0;
    }
    if (constant_bit || n_entries == 0) {
        ++T;
        ++runs;
    }
    return T < kTermLimit ? T : 0;
}

// How a call is cut (csgn_uint_plain_sum_plan reports it; the launcher follows it).  A plane GROUP is a run of output
// planes of which one element's workgroups fit one launch (one group for every shape but those with more than 2^32
// lane items an element); inside a group launches are cut at elements, as many as max_blocks workgroups hold:
// sum over the planes of ceil(ne * IPE_x / 256) <= ne * IPE / 256 + np.  launch(p0, np, e0, ne) returns false to stop.
template <typename Launch>
void sum_launches(const PlainSumPlan &pl, u32 U, u64 batch, u64 max_blocks, Launch launch)
{
    for (u32 j = 0; j < pl.n_out;) {
        u64 per = 0, ipe = 0;
        u32 k = j;
        for (; k < pl.n_out; ++k) {
            const u64 b = ((u64)pl.runs[k] * U + 255u) / 256u;
            if (k > j && per + b > kMaxBlocks256)
                break;
            per += b;
            ipe += (u64)pl.runs[k] * U;
        }
        const u32 np = k - j;
        const u64 epl = max_blocks > np ? std::max<u64>(1, (max_blocks - np) * 256u / ipe) : 1;
        for (u64 e0 = 0; e0 < batch; e0 += epl)
            if (!launch(j, np, e0, std::min(epl, batch - e0)))
                return;
        j = k;
    }
}

template <typename Unit>
hipError_t sum_kernel(const PlainSumPlan &pl, u64 n_bits, u64 batch, const u64 *const *planes, u64 *const *out, u32 U,
                      hipStream_t s)
{
    SumArgs a = {};
    a.U = U;
    a.dU = csgn_fastdiv_make(U);
    a.last_mask = last_word_mask(n_bits);
    a.w = pl.w;
    a.stride = pl.stride;
    a.rec = pl.d_rec;
    a.constant = pl.constant;
    for (u32 j = 0; j < kChainMaxLevels; ++j)
        a.t[j] = j < pl.w ? (u32)pl.t[j] : 1u;
    for (u32 x = 0; x < kMaxPlanes; ++x) {
        a.T[x] = x < pl.n_out ? (u32)pl.T[x] : 1u;
        a.runs[x] = x < pl.n_out ? pl.runs[x] : 1u;
        a.IPE.set(x, a.runs[x] * U);
        a.efirst[x + 1] = pl.efirst[std::min(x + 1, pl.n_out)];
    }
    hipError_t err = hipSuccess;
    sum_launches(pl, U, batch, launch_blocks(), [&](u32 p0, u32 np, u64 e0, u64 ne) {
        u64 blocks = 0, units = 0;
        for (u32 q = 0; q < np; ++q) {
            a.bfirst[q] = (u32)blocks;
            blocks += (ne * a.runs[p0 + q] * U + 255u) / 256u;
            units += ne * pl.T[p0 + q] * U;
            a.out[p0 + q] = reinterpret_cast<Unit *>(out[p0 + q]) + e0 * pl.T[p0 + q] * U;
        }
        a.bfirst[np] = (u32)blocks;
        for (u32 j = 0; j < pl.w; ++j)
            a.plane[j] = reinterpret_cast<const Unit *>(planes[j]) + e0 * pl.t[j] * U;
        a.p0 = p0;
        a.np = np;
        a.ne = (u32)ne;
        a.xcd = stream_xcd(units);
        k_uint_plain_sum<Unit><<<dim3((u32)blocks), 256, 0, s>>>(a);
        err = hipGetLastError();
        return err == hipSuccess;
    });
    return err;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_plain_sum_terms(u64 width, const u64 *terms, u64 n_entries, const int *cmp, const u64 *k, int constant_bit)
{
    u64 runs;
    return sum_plane(width, terms, n_entries, cmp, k, constant_bit, nullptr, runs);
}

bool uint_plain_sum_decode(u64 width, const u64 *terms, u64 n_entries, const int *cmp, const u64 *k, int constant_bit,
                           u64 q, u64 *level_plane, u64 *level_term, u64 *n_factors)
{
    std::vector<u32> rec;
    u64 runs;
    if (n_entries > kPlainSumMaxEntries || !level_plane || !level_term || !n_factors)
        return false;
    const u64 T = sum_plane(width, terms, n_entries, cmp, k, constant_bit, &rec, runs);
    if (T == 0 || T >= (1ull << 31) || q >= T)
        return false;
    const u32 w = (u32)width, stride = kRecHeader + 4u * w, nent = (u32)n_entries;
    const u32 extra = (nent == 0 || constant_bit) ? 1u : 0u;
    const u32 ent = sum_entry(nent, (u32)T - extra, (u32)q, [&](u32 i) { return rec[(u64)i * stride + R_TERM0]; });
    u64 n = 0;
    auto factor = [&](u64 plane, u64 term) {
        level_plane[n] = plane;
        level_term[n++] = term;
    };
    if (ent >= nent) {                                    // the plane's constant
        factor(constant_bit ? width : width + 1, 0);
        *n_factors = n;
        return true;
    }
    const u32 *r = rec.data() + (u64)ent * stride;
    u32 t32[kChainMaxLevels];
    for (u32 j = 0; j < w; ++j)
        t32[j] = (u32)std::min<u64>(terms[j], 0xFFFFFFFFu);
    u32 idx = (u32)q - r[R_TERM0];
    if ((r[R_FLAGS] & kFlagNeg) && idx == r[R_T] - 1u)
        factor(width, 0);                                 // the ONE that NE / LE / GE append
    else if (r[R_FLAGS] & kFlagZero)
        factor(width + 1, 0);
    else
        chain_walk_each(sum_view(nullptr, t32, r, w, 1u), w - 1u, r[R_BASE], idx, [&](u32 j, u32 i) {
            if (i < t32[j])
                factor(j, i);
            else
                factor(width, 0);                         // the ONE of n_j = a_j + ONE
        });
    *n_factors = n;
    return true;
}

int uint_plain_sum_shape(u64 width, const u64 *terms, u64 n_out, const u64 *first, const int *cmp, const u64 *k,
                         u64 constant, bool records, PlainSumPlan &pl)
{
    pl = PlainSumPlan();
    if (width < 1 || width > kChainMaxLevels || n_out < 1 || n_out > kMaxPlanes || !terms || !first || first[0] != 0 ||
        (n_out < 64 && (constant >> n_out) != 0))
        return CSGN_ERR_INVALID;
    for (u64 x = 0; x < n_out; ++x)
        if (first[x + 1] < first[x])
            return CSGN_ERR_INVALID;
    if (first[n_out] && (!cmp || !k))
        return CSGN_ERR_INVALID;
    if (first[n_out] > kPlainSumMaxEntries)
        return CSGN_ERR_UNSUPPORTED;
    pl.w = (u32)width;
    pl.n_out = (u32)n_out;
    pl.stride = kRecHeader + 4u * pl.w;
    pl.constant = constant;
    int rc = CSGN_OK;
    for (u64 x = 0; x < n_out; ++x) {
        u64 runs;
        pl.efirst[x] = (u32)first[x];
        pl.T[x] = sum_plane(width, terms, first[x + 1] - first[x], cmp + first[x], k + first[x], (int)((constant >> x) & 1u),
                            records ? &pl.rec : nullptr, runs);
        if (pl.T[x] == 0)
            return CSGN_ERR_INVALID;
        if (pl.T[x] >= (1ull << 31))
            rc = CSGN_ERR_UNSUPPORTED;
        pl.runs[x] = (u32)std::min<u64>(runs, 0xFFFFFFFFu);
    }
    pl.efirst[n_out] = (u32)first[n_out];
    for (u32 j = 0; j < pl.w; ++j)
        pl.t[j] = terms[j];
    return rc;
}

int uint_plain_sum_create(PlainSumPlan &pl, hipError_t &herr)
{
    const size_t bytes = std::max<size_t>(pl.rec.size(), 1) * sizeof(u32);
    herr = hipMalloc((void **)&pl.d_rec, bytes);
    if (herr == hipSuccess && !pl.rec.empty())
        herr = hipMemcpy(pl.d_rec, pl.rec.data(), pl.rec.size() * sizeof(u32), hipMemcpyHostToDevice);
    if (herr != hipSuccess) {
        uint_plain_sum_free(pl);
        return CSGN_ERR_HIP;
    }
    return CSGN_OK;
}

void uint_plain_sum_free(PlainSumPlan &pl)
{
    if (pl.d_rec)
        (void)hipFree(pl.d_rec);
    pl.d_rec = nullptr;
}

void uint_plain_sum_plan(const PlainSumPlan &pl, u64 n_bits, u64 batch, u64 *plan)
{
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = dL % 2 == 0;
    const u32 U = (u32)(wide ? dL / 2 : dL);
    u64 items = 0, launches = 0, groups = 0, first_ne = 0, first_blocks = 0;
    for (u32 x = 0; x < pl.n_out; ++x)
        items += (u64)pl.runs[x] * U;
    u32 last_p0 = 0xFFFFFFFFu;
    sum_launches(pl, U, std::max<u64>(batch, 1), launch_blocks(), [&](u32 p0, u32 np, u64, u64 ne) {
        if (launches == 0) {
            first_ne = ne;
            for (u32 q = 0; q < np; ++q)
                first_blocks += (ne * pl.runs[p0 + q] * U + 255u) / 256u;
        }
        ++launches;
        if (p0 != last_p0)
            ++groups;
        last_p0 = p0;
        return true;
    });
    plan[0] = wide ? 16 : 8;
    plan[1] = items;
    plan[2] = groups;
    plan[3] = batch ? launches : 0;
    plan[4] = batch ? first_ne : 0;
    plan[5] = batch ? first_blocks : 0;
}

hipError_t uint_plain_sum(const PlainSumPlan &pl, u64 n_bits, u64 batch, const u64 *const *planes, u64 *const *out,
                          hipStream_t s)
{
    if (batch == 0)
        return hipSuccess;
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(planes, pl.w), ptr_array(out, pl.n_out));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? sum_kernel<unit16>(pl, n_bits, batch, planes, out, U, s)
                : sum_kernel<unit8>(pl, n_bits, batch, planes, out, U, s);
}

} // namespace csgn
