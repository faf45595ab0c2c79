// csgn_chain.h -- the host side of the left-nested chains over the planes a_j and n_j = a_j + ONE that
// csgn_uint_plain.hip, csgn_uint_plain_sum.hip and csgn_uint_addk.hip evaluate: the
// chain's description, its term counts, one comparison's chain (plain_shape) with its cut and radix-1 levels,
// the level table of the fused kernels (decoded by csgn_device.h's chain_term / chain_walk) and the composed form that
// runs it level by level through the tuned launchers.  Host code only.  Internal.
#pragma once

#include "csgn_device.h"
#include "csgn_hip.h"

namespace csgn {

constexpr u32 kChainMaxLevels = 64;

// value(base) = f_base,  value(j) = value(j - 1) * f_j  or  (value(j - 1) * f_j) + tail_j  for base < j <= top, where
// f_j is n_j when bit j of nfac is set and a_j otherwise, level j is a sum when bit j of sum is set, and its tail is
// n_j when bit j of tail_n is set and a_j otherwise.
struct Chain {
    u32 base = 0, top = 0;
    u64 nfac = 0, sum = 0, tail_n = 0;
    u64 L[kChainMaxLevels] = {};           // terms of value(j), base <= j <= top
};

// what every operation over w planes and a public constant asks of its arguments: 1..64 planes of 1..kTermLimit - 1
// terms, and a constant that fits
inline bool chain_arguments(u64 w, u64 k, const u64 *t)
{
    if (w < 1 || w > kChainMaxLevels || !t || (w < 64 && (k >> w) != 0))
        return false;
    for (u64 j = 0; j < w; ++j)
        if (t[j] == 0 || t[j] >= kTermLimit)
            return false;
    return true;
}

// the GT chain of k over w planes, k below 2^w - 1:  l = a_m at the lowest clear bit m of k, then upwards
// l = l * a_j (k_j = 1)  or  (l * n_j) + a_j (k_j = 0)
inline Chain chain_greater(u64 w, u64 k)
{
    Chain c;
    c.base = (u32)__builtin_ctzll(~k);
    c.top = (u32)w - 1;
    for (u64 j = c.base + 1; j < w; ++j)
        if (!((k >> j) & 1u)) {
            c.sum |= 1ull << j;
            c.nfac |= 1ull << j;
        }
    return c;
}

// fills c.L from the planes' terms t; false when a count reaches kTermLimit
inline bool chain_terms(Chain &c, const u64 *t)
{
    auto radix = [&](u32 j) { return t[j] + ((c.nfac >> j) & 1u); };
    u64 l = radix(c.base);
    c.L[c.base] = l;
    for (u32 j = c.base + 1; j <= c.top; ++j) {
        if (!term_mul(l, radix(j), l))
            return false;
        if ((c.sum >> j) & 1u)
            l += t[j] + ((c.tail_n >> j) & 1u);
        if (l >= kTermLimit)
            return false;
        c.L[j] = l;
    }
    return true;
}

// The level table of a fused kernel's arguments (csgn_device.h, chain decode): t of all w planes, and rad / pend of the
// levels in (c.base, end) that the kernel walks; c == nullptr: no level is walked.  Slots no level reads hold radix 1
// and no tail.
template <typename Args>
void chain_fill(const Chain *c, u32 w, u32 end, const u64 *t, Args &a)
{
    for (u32 j = 0; j < kChainMaxLevels; ++j) {
        u32 d = 1;
        a.t[j] = j < w ? (u32)std::min<u64>(t[j], 0xFFFFFFFFu) : 1u;
        a.pend[j] = 0xFFFFFFFFu;
        if (c && j > c->base && j < end) {
            const u64 r = t[j] + ((c->nfac >> j) & 1u);
            d = (u32)r;
            if ((c->sum >> j) & 1u)
                a.pend[j] = (u32)(c->L[j - 1] * r);
        }
        a.rad.set(j, d);
    }
}

// ------------------------------------------------------------------------------ one comparison
// csgn_uint_plain.hip and csgn_uint_plain_sum.hip: the chain the kernels decode and the composed form runs, or ZERO.
struct PlainShape {
    bool zero = false, neg = false;
    u32 w = 0;
    Chain c;
    u64 T = 0;                             // terms of the result
};

// false: invalid argument or a term count past kTermLimit
inline bool plain_shape(int cmp, u64 w, u64 k, const u64 *t, PlainShape &sh)
{
    sh = PlainShape();
    if (cmp < CSGN_UINT_PLAIN_EQ || cmp > CSGN_UINT_PLAIN_GE || !chain_arguments(w, k, t))
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
    Chain &c = sh.c;
    if (base_cmp == CSGN_UINT_PLAIN_EQ) {
        c.nfac = ~k & all;                                       // g_j = k_j ? a_j : n_j, all factors
    } else if (base_cmp == CSGN_UINT_PLAIN_LT) {
        c.base = (u32)__builtin_ctzll(k);                        // l = n_m
        c.sum = c.tail_n = k & (all << c.base << 1);             // l = (l * a_j) + n_j where k_j = 1
        c.nfac = ~k & all & (all << c.base << 1);                // l = l * n_j where k_j = 0
        c.nfac |= 1ull << c.base;
    } else {
        c = chain_greater(w, k);
    }
    c.top = sh.w - 1;
    if (!chain_terms(c, t))
        return false;
    sh.T = c.L[c.top] + (sh.neg ? 1 : 0);
    return sh.T < kTermLimit;
}

// the cut of a run of R terms: the fewest top levels whose digits cover a run (their product of radices >= R); levels
// [cut, top] are walked per term, the rest is kept per run
inline u32 plain_cut(const PlainShape &sh, const u64 *t, u32 R)
{
    if (sh.zero)
        return 1u;
    u32 cut = sh.w;
    u64 span = 1;
    while (cut > sh.c.base + 1 && span < R) {
        --cut;
        span *= t[cut] + ((sh.c.nfac >> cut) & 1u);
    }
    return cut;
}

// the levels above the base whose factor has one term (radix 1): the walk moves no digit there
inline u64 plain_radix1(const PlainShape &sh, const u64 *t)
{
    u64 unit = 0;
    for (u32 j = sh.c.base + 1; !sh.zero && j < sh.w; ++j)
        if (t[j] + ((sh.c.nfac >> j) & 1u) == 1u)
            unit |= 1ull << j;
    return unit;
}

// The composed form: levels [c.base, end) through the tuned launchers, each level's value written whole before the
// next reads it.  n_j is the copy of a_j followed by ONE (csgn_gate_uniform NOT's words).  The running values ping-pong
// through one temporary block of the caller's slot (scratch_take, csgn_kernels.h).  Level end - 1 is written to `last`
// at last_pitch words per element, or kept in the block like the others when last is nullptr.  base_in_place: f_base
// is a_base and is read where it lies (it is still copied when it is the level that goes to `last`).
// each(j, cur) is called for every j <= end, in order and behind the block's allocation: before level j is computed,
// and with j = end behind the last level; cur is value(j - 1), nullptr up to the base.  It returns a hipError_t and
// may launch.
template <typename Each>
hipError_t chain_composed(const Chain &c, u32 end, ScratchSlot slot, u64 n_bits, u64 batch, const u64 *const *planes,
                          const u64 *t, bool base_in_place, u64 *last, u64 last_pitch, hipStream_t s, Each each)
{
    const u64 dL = (n_bits + 63) / 64;
    // a list a_j (+ ONE when n) written at dst with pitch
    auto list = [&](u32 j, bool n, u64 *dst, u64 pitch) {
        hipError_t e = add_uniform(n_bits, batch, t[j], 0, planes[j], nullptr, dst, s, pitch);
        if (e == hipSuccess && n)
            e = const_fill(n_bits, batch, nullptr, 1, dst + t[j] * dL, pitch, s);
        return e;
    };
    auto to_last = [&](u32 j) { return last && j + 1 == end; };
    u64 maxL = 0, maxN = 0;
    for (u32 j = c.base; j < end; ++j) {
        if (!to_last(j) && !(j == c.base && base_in_place))
            maxL = std::max(maxL, c.L[j]);
        if (j > c.base && ((c.nfac >> j) & 1u))
            maxN = std::max(maxN, t[j] + 1);
    }
    const u64 words = batch * dL * (2 * maxL + maxN);
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = words ? scratch_take(slot, words * 8, s, owned, e) : nullptr;
    if (e != hipSuccess)
        return e;
    u64 *buf[2] = {block, block ? block + batch * maxL * dL : nullptr};
    u64 *nbuf = block ? block + 2 * batch * maxL * dL : nullptr;
    const u64 *cur = nullptr;
    for (u32 j = 0; j < end && e == hipSuccess; ++j) {
        if ((e = each(j, cur)) != hipSuccess || j < c.base)
            continue;
        u64 *dst = to_last(j) ? last : buf[(j - c.base) & 1u];
        const u64 pitch = to_last(j) ? last_pitch : c.L[j] * dL;
        if (j == c.base) {
            if (base_in_place && !to_last(j)) {
                cur = planes[j];
                continue;
            }
            e = list(j, (c.nfac >> j) & 1u, dst, pitch);
            cur = dst;
            continue;
        }
        const bool nf = (c.nfac >> j) & 1u;
        const u64 Lb = c.L[j - 1], r = t[j] + (nf ? 1 : 0);
        const u64 *f = planes[j];
        if (nf) {                                             // n_j materialised
            e = list(j, true, nbuf, r * dL);
            f = nbuf;
        }
        if (e == hipSuccess)
            e = mul_uniform(n_bits, batch, Lb, r, cur, f, dst, 0, s, pitch);
        if (e == hipSuccess && ((c.sum >> j) & 1u))
            e = list(j, (c.tail_n >> j) & 1u, dst + Lb * r * dL, pitch);
        cur = dst;
    }
    if (e == hipSuccess)
        e = each(end, cur);
    return scratch_done(block, owned, e);
}

} // namespace csgn
