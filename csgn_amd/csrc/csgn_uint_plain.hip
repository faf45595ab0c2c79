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
// 1 moves no digit: its factor is a per-lane constant, loaded once per lane, not per term.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kMaxLevels = 64;
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
    // the radix-1 factors of the fast levels: every term that passes the cut carries all of them
    Unit fast_unit = one;
    for (u32 j = a.top + 1u; !a.zero && j-- > a.cut;)
        if ((a.unit >> j) & 1u)
            fast_unit &= chain_term<Unit>(a, j, eu, 0u, k, one);
    u32 key = 0xFFFFFFFFu;                                // the index that reached the cut, and the AND below it
    Unit below = one;
    for (u32 q = 0; q < nt; ++q) {
        const u32 idx0 = t0 + q;
        Unit v = one;
        if (a.neg && idx0 == a.T - 1u) {
            // the appended ONE
        } else if (a.zero) {
            v = zero_unit(Unit());
        } else {
            // the fast levels, loading only where the digit moves (|f_j| > 1) or a tail ends the walk
            u32 idx = idx0, stop = 0xFFFFFFFFu;
            for (u32 j = a.top + 1u; j-- > a.cut;) {
                const u32 pe = a.pend[j];
                if (idx >= pe) {                          // a sum level's tail
                    v &= chain_term<Unit>(a, j, eu, idx - pe, k, one);
                    stop = j;
                    break;
                }
                if ((a.unit >> j) & 1u)
                    continue;                             // d = 0, idx unchanged: f_j[0] is in fast_unit
                const FastDiv dr = a.rad.at(j);
                const u32 q = csgn_fastdiv(idx, dr), d = idx - q * dr.d;
                idx = q;
                v &= chain_term<Unit>(a, j, eu, d, k, one);
            }
            const bool done = stop != 0xFFFFFFFFu;
            if (done) {
                // a tail at level `stop` carries the radix-1 factors above it only (a short list: tails are a small
                // share of any large result)
                for (u32 j = a.top + 1u; j-- > stop + 1u;)
                    if ((a.unit >> j) & 1u)
                        v &= chain_term<Unit>(a, j, eu, 0u, k, one);
            } else {
                v &= fast_unit;
                if (idx != key) {
                    key = idx;
                    below = one;
                    chain_walk<Unit>(a, a.cut - 1u, a.base, eu, k, one, idx, below);
                }
                v &= below;
            }
        }
        unit_store<Unit, true>(o + (u64)q * a.U, v);
    }
}

// ------------------------------------------------------------------------------ the definitions on the host

// Level table of one comparison: the chain the kernel decodes and the composed form runs.
struct PlainShape {
    bool zero = false, neg = false;
    u32 w = 0, base = 0;
    u64 nfac = 0, sum = 0, tail_n = 0;     // bit j
    u64 L[kMaxLevels] = {};                // terms of the running value after level j (j >= base)
    u64 T = 0;                             // terms of the result
};

// false: invalid argument or a term count past kTermLimit
bool plain_shape(int cmp, u64 w, u64 k, const u64 *t, PlainShape &sh)
{
    sh = PlainShape();
    if (cmp < CSGN_UINT_PLAIN_EQ || cmp > CSGN_UINT_PLAIN_GE || w < 1 || w > 64 || !t)
        return false;
    if (w < 64 && (k >> w) != 0)
        return false;
    for (u64 j = 0; j < w; ++j)
        if (t[j] == 0 || t[j] >= kTermLimit)
            return false;
    sh.w = (u32)w;
    const u64 all = w == 64 ? ~0ull : (1ull << w) - 1;
    // NE = NOT EQ, LE = NOT GT, GE = NOT LT
    const int base_cmp = cmp == CSGN_UINT_PLAIN_NE ? CSGN_UINT_PLAIN_EQ
                       : cmp == CSGN_UINT_PLAIN_LE ? CSGN_UINT_PLAIN_GT
                       : cmp == CSGN_UINT_PLAIN_GE ? CSGN_UINT_PLAIN_LT : cmp;
    sh.neg = base_cmp != cmp;
    if ((base_cmp == CSGN_UINT_PLAIN_LT && k == 0) || (base_cmp == CSGN_UINT_PLAIN_GT && k == all)) {
        sh.zero = true;
        sh.T = sh.neg ? 2 : 1;
        return true;
    }
    auto bit = [&](u64 j) { return (k >> j) & 1u; };
    if (base_cmp == CSGN_UINT_PLAIN_EQ) {
        sh.base = 0;
        for (u64 j = 0; j < w; ++j)
            if (!bit(j))
                sh.nfac |= 1ull << j;                            // g_j = k_j ? a_j : n_j
    } else if (base_cmp == CSGN_UINT_PLAIN_LT) {
        sh.base = (u32)__builtin_ctzll(k);                       // l = n_m
        sh.nfac |= 1ull << sh.base;
        for (u64 j = sh.base + 1; j < w; ++j) {
            if (bit(j)) {                                        // l = (l * a_j) + n_j
                sh.sum |= 1ull << j;
                sh.tail_n |= 1ull << j;
            } else {
                sh.nfac |= 1ull << j;                            // l = l * n_j
            }
        }
    } else {
        sh.base = (u32)__builtin_ctzll(~k);                      // l = a_m
        for (u64 j = sh.base + 1; j < w; ++j) {
            if (!bit(j)) {                                       // l = (l * n_j) + a_j
                sh.sum |= 1ull << j;
                sh.nfac |= 1ull << j;
            }                                                    // else l = l * a_j
        }
    }
    auto radix = [&](u64 j) { return t[j] + ((sh.nfac >> j) & 1u); };
    u64 l = radix(sh.base);
    sh.L[sh.base] = l;
    for (u64 j = sh.base + 1; j < w; ++j) {
        if (!term_mul(l, radix(j), l))
            return false;
        if ((sh.sum >> j) & 1u)
            l += t[j] + ((sh.tail_n >> j) & 1u);
        if (l >= kTermLimit)
            return false;
        sh.L[j] = l;
    }
    sh.T = l + (sh.neg ? 1 : 0);
    return sh.T < kTermLimit;
}

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
    a.base = sh.base;
    a.top = sh.w - 1;
    a.R = (u32)std::min<u64>(sh.T, kRun);
    a.runs = (u32)((sh.T + a.R - 1) / a.R);
    a.IPE = a.runs * U;
    a.dU = csgn_fastdiv_make(U);
    a.dIPE = csgn_fastdiv_make(a.IPE);
    // the cut: the fewest top levels whose digits cover a run (their product of radices >= R); the rest is kept per run
    a.cut = sh.zero ? 1u : sh.w;
    if (!sh.zero) {
        u64 span = 1;
        while (a.cut > sh.base + 1 && span < a.R) {
            --a.cut;
            span *= t[a.cut] + ((sh.nfac >> a.cut) & 1u);
        }
    }
    for (u32 j = 0; j < kMaxLevels; ++j) {
        u32 d = 1;
        a.pend[j] = 0xFFFFFFFFu;
        if (!sh.zero && j < sh.w) {
            a.t[j] = (u32)t[j];
            if (j > sh.base) {
                const u64 r = t[j] + ((sh.nfac >> j) & 1u);
                d = (u32)r;
                if (r == 1)
                    a.unit |= 1ull << j;
                if ((sh.sum >> j) & 1u)
                    a.pend[j] = (u32)(sh.L[j - 1] * r);
            }
        }
        a.rad.set(j, d);
    }
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

// The composed form: the same chain through the tuned launchers, level by level, each level's value written whole
// before the next reads it.  n_j is the copy of a_j followed by ONE (csgn_gate_uniform NOT's words).  The running values
// ping-pong through one temporary block (scratch_take, csgn_kernels.h); the last level writes d_out.
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
    // a list a_j (+ ONE when n) written at dst with pitch
    auto list = [&](u32 j, bool n, u64 *dst, u64 pitch) {
        hipError_t e = add_uniform(n_bits, batch, t[j], 0, planes[j], nullptr, dst, s, pitch);
        if (e == hipSuccess && n)
            e = const_fill(n_bits, batch, nullptr, 1, dst + t[j] * dL, pitch, s);
        return e;
    };
    const u32 top = sh.w - 1;
    u64 maxL = 0, maxN = 0;
    for (u32 j = sh.base; j < top; ++j)
        maxL = std::max(maxL, sh.L[j]);
    for (u32 j = sh.base + 1; j <= top; ++j)
        if ((sh.nfac >> j) & 1u)
            maxN = std::max(maxN, t[j] + 1);
    const u64 words = batch * dL * (2 * maxL + maxN);
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = words ? scratch_take(SCRATCH_UINT_PLAIN, words * 8, s, owned, e) : nullptr;
    if (e != hipSuccess)
        return e;
    u64 *buf[2] = {block, block ? block + batch * maxL * dL : nullptr};
    u64 *nbuf = block ? block + 2 * batch * maxL * dL : nullptr;
    u64 *cur = sh.base == top ? out : buf[0];
    e = list(sh.base, (sh.nfac >> sh.base) & 1u, cur, (sh.base == top ? sh.T : sh.L[sh.base]) * dL);
    for (u32 j = sh.base + 1; j <= top && e == hipSuccess; ++j) {
        u64 *dst = j == top ? out : buf[(j - sh.base) & 1u];
        const u64 Lb = sh.L[j - 1], pitch = (j == top ? sh.T : sh.L[j]) * dL;
        const bool nf = (sh.nfac >> j) & 1u, sum = (sh.sum >> j) & 1u;
        const u64 r = t[j] + (nf ? 1 : 0);
        const u64 *f = planes[j];
        if (nf) {                                             // n_j materialised
            e = list(j, true, nbuf, r * dL);
            f = nbuf;
        }
        if (e == hipSuccess)
            e = mul_uniform(n_bits, batch, Lb, r, cur, f, dst, 0, s, pitch);
        if (e == hipSuccess && sum)
            e = list(j, (sh.tail_n >> j) & 1u, dst + Lb * r * dL, pitch);
        cur = dst;
    }
    if (e == hipSuccess && sh.neg)
        e = const_fill(n_bits, batch, nullptr, 1, out + (sh.T - 1) * dL, pitchT, s);
    return scratch_done(block, owned, e);
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
