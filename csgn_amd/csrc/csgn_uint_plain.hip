// csgn_uint_plain.hip -- comparison of bit-sliced encrypted unsigned integers against one PUBLIC constant k, the whole
// w-bit comparison in one launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in
// DESIGN.md §4.14.
//
// The definitions (include/csgn_hip.h, csgn_uint_plain) are left-nested chains of the reference's operator* / operator+
// over the planes a_j and n_j = a_j + ONE.  Since (X + Y) * Z = X * Z + Y * Z and (X * Y) * Z = X * (Y * Z) in the
// reference's term order (left term slowest), output term idx of level j's value is found by peeling levels from the
// top (the fast digits) down:
//     product level j, factor f (a_j: t_j terms, or n_j: t_j + 1, its last ONE):  d = idx % |f|, idx /= |f|, AND f[d]
//     sum level j (value = below * f + tail):   idx >= |below| * |f|  -> AND tail[idx - |below| * |f|] and stop
//     base level m:                              AND base[idx] and stop
// and the negations append one ONE term.  Each term is the AND of one term per level it passes.
//
// Reads per written unit do not grow with w, by an odometer: a lane writes unit k of a RUN of consecutive terms, walks
// only the top (fast) levels that span a run per term, and keeps the AND of the levels below that cut in registers,
// keyed by the index that reaches the cut; consecutive terms share it until the fast digits wrap.  A fast level of radix
// 1 moves no digit: its factor is a per-lane constant, loaded once per lane, not per term.  The run
// itself is csgn_device.h's chain_run, which csgn_uint_plain_sum.hip calls too; the chain's shape, its cut and its
// radix-1 levels are csgn_chain.h's plain_shape, plain_cut and plain_radix1.
#include "csgn_chain.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kMaxLevels = kChainMaxLevels;
constexpr u32 kRun = 16;              // terms per lane

// The level table, by value in the kernel arguments (uniform, scalar loads).  Level j in [base, top]:
//     plane[j]  a_j of this launch's first element, t[j] terms per element
//     radix[j]  |f_j| as a FastDiv (t_j, or t_j + 1 when the factor is n_j); unused at the base
//     pend[j]   |below| * |f_j| for a sum level (the tail starts there); above every index for a product level
// Mask unit (bit j, j above the base): |f_j| = 1, so the factor is the per-lane constant f_j[0] and the walk loads nothing
// there unless a sum level's tail ends it.
struct PlainArgs {
    const void *plane[kMaxLevels];
    u32 t[kMaxLevels];
    u32 pend[kMaxLevels];
    FastDivTable<kMaxLevels> rad;
    u64 unit;
    void *out;
    u32 base, top, cut;       // levels [cut, top] are walked per term, [base, cut) once per run (cut > top: none)
    u32 zero;                 // the result is ZERO (then ONE when neg): no level is read
    u32 neg;                  // one ONE term appended (term T - 1)
    u32 T, R, runs;           // terms per element, terms per run, runs per element
    u32 U, IPE;               // units per term, lane items per element (runs * U)
    u32 total_items;          // this launch
    u32 xcd;
    FastDiv dU, dIPE;
    u64 last_mask;
};

template <typename Unit>
__global__ void __launch_bounds__(256) k_uint_plain(PlainArgs a)
{
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const u32 g = bid * 256u + threadIdx.x;
    if (g >= a.total_items)
        return;
    const u32 e = csgn_fastdiv(g, a.dIPE), rem = g - e * a.IPE;
    const u32 run = csgn_fastdiv(rem, a.dU), k = rem - run * a.U;
    const u32 t0 = run * a.R, nt = min(a.R, a.T - t0);
    const u64 eu = (u64)e * a.U;                          // element e's first unit of a 1-term-per-element list
    const Unit one = one_unit(Unit(), k, a.U, a.last_mask);
    Unit *o = reinterpret_cast<Unit *>(a.out) + ((u64)e * a.T + t0) * a.U + k;
    chain_run<Unit>(a, a.top, a.cut, a.zero, a.neg, a.T, a.unit, eu, k, one, t0, nt, o);
}

// ------------------------------------------------------------------------------ the definitions on the host

// Fused unless forced, and for w = 1 (one copy and at most one constant: the composed form is those tuned launchers).
bool plain_use_fused(const PlainShape &sh)
{
    return tune_choose(TUNE_UINT_PLAIN_FUSED, sh.w > 1 && !sh.zero);
}

template <typename Unit>
hipError_t plain_fused(const PlainShape &sh, u64 n_bits, u64 batch, const u64 *const *planes, const u64 *t, u64 *out,
                       u32 U, hipStream_t s)
{
    PlainArgs a = {};
    a.U = U;
    a.last_mask = last_word_mask(n_bits);
    a.zero = sh.zero ? 1u : 0u;
    a.neg = sh.neg ? 1u : 0u;
    a.T = (u32)sh.T;
    a.base = sh.c.base;
    a.top = sh.w - 1;
    a.R = (u32)std::min<u64>(sh.T, kRun);
    a.runs = (u32)((sh.T + a.R - 1) / a.R);
    a.IPE = a.runs * U;
    a.dU = csgn_fastdiv_make(U);
    a.dIPE = csgn_fastdiv_make(a.IPE);
    a.cut = plain_cut(sh, t, a.R);
    chain_fill(sh.zero ? nullptr : &sh.c, sh.w, sh.w, t, a);
    a.unit = plain_radix1(sh, t);
    a.xcd = stream_xcd(batch * sh.T * U);
    const u64 per = std::max<u64>(1, 0xFFFFFF00ull / a.IPE);            // elements per launch: < 2^32 lane items
    for (u64 e0 = 0; e0 < batch; e0 += per) {
        const u64 ne = std::min(per, batch - e0);
        if (!sh.zero)
            for (u32 j = 0; j < sh.w; ++j)
                a.plane[j] = reinterpret_cast<const Unit *>(planes[j]) + e0 * t[j] * U;
        a.out = reinterpret_cast<Unit *>(out) + e0 * sh.T * U;
        a.total_items = (u32)(ne * a.IPE);
        k_uint_plain<Unit><<<dim3(ceil_div_u64(a.total_items, 256u)), 256, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// The composed form: csgn_chain.h's, the last level written to d_out; the negation's ONE follows it.
hipError_t plain_composed(const PlainShape &sh, u64 n_bits, u64 batch, const u64 *const *planes, const u64 *t, u64 *out,
                          hipStream_t s)
{
    const u64 dL = (n_bits + 63) / 64;
    const u64 pitchT = sh.T * dL;
    if (sh.zero) {
        hipError_t e = const_fill(n_bits, batch, nullptr, 0, out, pitchT, s);
        if (e == hipSuccess && sh.neg)
            e = const_fill(n_bits, batch, nullptr, 1, out + dL, pitchT, s);
        return e;
    }
    return chain_composed(sh.c, sh.w, SCRATCH_UINT_PLAIN, n_bits, batch, planes, t, false, out, pitchT, s,
                          [&](u32 j, const u64 *) {
                              if (j < sh.w || !sh.neg)
                                  return hipSuccess;
                              return const_fill(n_bits, batch, nullptr, 1, out + (sh.T - 1) * dL, pitchT, s);
                          });
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_plain_terms(int cmp, u64 width, u64 k, const u64 *terms)
{
    PlainShape sh;
    return plain_shape(cmp, width, k, terms, sh) ? sh.T : 0;
}

const char *uint_plain_kernel_name(u64 n_bits, int cmp, u64 batch, u64 width, u64 k, const u64 *terms)
{
    (void)n_bits;
    (void)batch;
    PlainShape sh;
    if (!plain_shape(cmp, width, k, terms, sh))
        return "";
    return plain_use_fused(sh) ? "k_uint_plain" : "composed";
}

hipError_t uint_plain(u64 n_bits, int cmp, u64 batch, u64 width, u64 k, const u64 *const *planes, const u64 *terms,
                      u64 *out, hipStream_t s)
{
    PlainShape sh;
    if (!plain_shape(cmp, width, k, terms, sh))
        return hipErrorInvalidValue;
    if (batch == 0)
        return hipSuccess;
    if (!plain_use_fused(sh))
        return plain_composed(sh, n_bits, batch, planes, terms, out, s);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, out, ptr_array(planes, sh.zero ? 0 : sh.w));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? plain_fused<unit16>(sh, n_bits, batch, planes, terms, out, U, s)
                : plain_fused<unit8>(sh, n_bits, batch, planes, terms, out, U, s);
}

} // namespace csgn
