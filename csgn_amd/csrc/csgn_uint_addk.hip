// csgn_uint_addk.hip -- a bit-sliced encrypted unsigned integer plus one PUBLIC constant k, every output plane (and the
// carry-out) in one launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in
// DESIGN.md §4.18.
//
// The definition (include/csgn_hip.h, csgn_uint_addk): with m the lowest set bit of k, the carry into plane j > m is
// the left-nested chain  c_m = a_m,  c_j = c_{j-1} * a_j (k_j = 0)  or  (c_{j-1} * n_j) + a_j (k_j = 1),  the GT chain
// of csgn_uint_plain with the bits of k complemented, and
//     out_j = [ a_j : t_j terms ][ c_{j-1} : T(c_{j-1}) terms, j > m ][ ONE, k_j = 1 ][ ONE, negate_out ]
// so an element of an output plane is a copy, a prefix of ONE chain decoded by csgn_device.h's chain_walk from level
// j - 1 down to m, and ONEs made in registers.  All w chains share one level table.
//
// One lane writes one unit; a wave's store covers 64 consecutive units of consecutive terms of one plane.  A workgroup
// belongs to one plane (each plane's lane range is rounded up to whole workgroups), so the plane, its sizes and its
// pointers are scalar.
#include "csgn_chain.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kMaxLevels = kChainMaxLevels, kMaxPlanes = kMaxLevels + 1;   // the carry-out is plane `width`

// By value in the kernel arguments (3.7 KB of the 4 KB limit; uniform indices, scalar loads).  The level table is
// k_uint_plain's: level j in [base, width):
//     plane[j]  a_j of this launch's first element, t[j] terms per element
//     rad[j]    |f_j| (t_j, or t_j + 1 when the factor is n_j: k_j = 1); unused at the base
//     pend[j]   T(c_{j-1}) * |f_j| where k_j = 1 (the tail a_j starts there); above every index where k_j = 0
// and per output plane p:
//     out[p]    its first element of this launch;  first[p] its first workgroup;  PU.d[p] its units per element
//     chain[p]  terms of its chain segment c_{p-1} (0: none; the ZERO carry-out of k = 0 counts 1)
struct AddkArgs {
    const void *plane[kMaxLevels];
    u32 t[kMaxLevels];
    u32 pend[kMaxLevels];
    FastDivTable<kMaxLevels> rad;
    void *out[kMaxPlanes];
    u32 first[kMaxPlanes + 1];
    u32 chain[kMaxPlanes];
    FastDivTable<kMaxPlanes> PU;
    u64 last_mask;
    u32 base, width, np;      // np output planes: width, or width + 1 with the carry-out
    u32 zero;                 // k = 0: the carry-out's one term is ZERO
    u32 U, ne;                // units per term, elements of this launch
    u32 xcd;
    FastDiv dU;
};
static_assert(sizeof(AddkArgs) <= 4096, "kernel arguments past the 4 KB limit");

template <typename Unit>
__global__ void __launch_bounds__(256) k_uint_addk(AddkArgs a)
{
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    u32 p = 0, hi = a.np;                                 // the plane of this workgroup: first[p] <= bid < first[p + 1]
    while (hi - p > 1u) {
        const u32 mid = (p + hi) >> 1;
        if (a.first[mid] <= bid)
            p = mid;
        else
            hi = mid;
    }
    const FastDiv dpu = a.PU.at(p);
    const u32 off = (bid - a.first[p]) * 256u + threadIdx.x;   // unit inside the plane's part of this launch
    if (off >= a.ne * dpu.d)
        return;
    const u32 e = csgn_fastdiv(off, dpu), rem = off - e * dpu.d;
    const u32 term = csgn_fastdiv(rem, a.dU), k = rem - term * a.U;
    const u64 eu = (u64)e * a.U;
    const Unit one = one_unit(Unit(), k, a.U, a.last_mask);
    const u32 copy = p < a.width ? a.t[p] : 0u;
    Unit v = one;                                         // past the copy and the chain: the appended ONEs
    if (term < copy) {
        v = chain_term<Unit>(a, p, eu, term, k, one);
    } else if (term - copy < a.chain[p]) {
        u32 idx = term - copy;
        if (a.zero)
            v = zero_unit(Unit());
        else
            chain_walk<Unit>(a, p - 1u, a.base, eu, k, one, idx, v);
    }
    unit_store<Unit, true>(reinterpret_cast<Unit *>(a.out[p]) + (u64)off, v);
}

// ------------------------------------------------------------------------------ the definition on the host

struct AddkShape {
    u32 w = 0;
    bool zero = false;                     // k = 0: no chain
    Chain c;                               // the carries: the GT chain of ~k, c.L[j] = T(c_j)
    u64 T[kMaxPlanes] = {};                // terms of out_j without negate_out; T[w]: the carry-out
};

// false: invalid argument or a term count past kTermLimit
bool addk_shape(u64 w, u64 k, const u64 *t, AddkShape &sh)
{
    sh = AddkShape();
    if (!chain_arguments(w, k, t))
        return false;
    sh.w = (u32)w;
    sh.zero = k == 0;
    std::copy(t, t + w, sh.T);
    sh.T[w] = 1;
    if (sh.zero)
        return true;
    sh.c = chain_greater(w, ~k & (w == 64 ? ~0ull : (1ull << w) - 1));
    if (!chain_terms(sh.c, t))
        return false;
    sh.T[sh.c.base] += 1;
    for (u64 j = sh.c.base + 1; j < w; ++j) {
        sh.T[j] += sh.c.L[j - 1] + ((k >> j) & 1u);
        if (sh.T[j] >= kTermLimit)
            return false;
    }
    sh.T[w] = sh.c.L[w - 1];
    return true;
}

// Per shape, by the measurements of DESIGN §4.18.  A single plane (width 1 without the carry-out) is one copy and at
// most two constants through the tuned launchers.  The fused kernel walks every chain term's levels per written unit
// (p - m loads for plane p), the composed form reads each carry once.  Two measured classes go to the composed form:
// chain terms that walk 8 levels or more on average (a + 1 at 16 bits walks 8 and ties, a + 1 and a + 3 at 32 bits walk
// 16 and lose; the shapes that walk 4 to 6 win), and outputs of 16 GiB or more with over 5 levels walked per term
// written (a + 255 at 8 bits x 2^20).
bool addk_use_fused(const AddkShape &sh, bool carry, u64 n_bits, u64 batch)
{
    const u32 np = sh.w + (carry ? 1u : 0u);
    // one element's planes (at 8-byte units and with negate_out's ONE, the larger count) must fit one launch's lanes
    double lanes = 0;
    for (u32 p = 0; p < np; ++p)
        lanes += ((double)sh.T[p] + 1.0) * (double)((n_bits + 63) / 64);
    if (lanes > (double)(0xFFFFFF00ull - 256ull * kMaxPlanes))
        return false;                                     // whatever the knob says: the kernel cannot index it
    bool fused = sh.w > 1 || carry;
    if (fused && !sh.zero) {
        double walked = 0, written = 0, chained = 0;
        for (u32 p = 0; p < np; ++p) {
            written += (double)sh.T[p];
            if (p > sh.c.base) {
                chained += (double)sh.c.L[p - 1];
                walked += (double)sh.c.L[p - 1] * (p - sh.c.base);
            }
        }
        const double bytes = written * (double)batch * (double)((n_bits + 63) / 64) * 8.0;
        fused = walked < 8.0 * chained && !(bytes >= 17179869184.0 && walked > 5.0 * written);
    }
    return tune_choose(TUNE_UINT_ADDK_FUSED, fused);
}

template <typename Unit>
hipError_t addk_fused(const AddkShape &sh, u64 n_bits, u64 batch, bool neg, const u64 *const *planes, const u64 *t,
                      u64 *const *outs, u64 *carry, u32 U, hipStream_t s)
{
    AddkArgs a = {};
    a.U = U;
    a.dU = csgn_fastdiv_make(U);
    a.last_mask = last_word_mask(n_bits);
    a.base = sh.c.base;
    a.width = sh.w;
    a.np = sh.w + (carry ? 1u : 0u);
    a.zero = sh.zero ? 1u : 0u;
    chain_fill(sh.zero ? nullptr : &sh.c, sh.w, a.np - 1u, t, a);   // levels [base, np - 1) are walked
    u64 units[kMaxPlanes], sum_units = 0;                 // per element
    for (u32 p = 0; p < kMaxPlanes; ++p) {
        units[p] = 1;
        if (p < a.np) {
            const u64 T = sh.T[p] + (neg && p < sh.w ? 1 : 0);
            units[p] = T * U;
            sum_units += units[p];
            a.chain[p] = sh.zero ? (p == sh.w ? 1u : 0u) : p > sh.c.base ? (u32)sh.c.L[p - 1] : 0u;
        }
        a.PU.set(p, (u32)units[p]);
    }
    // elements per launch: every plane's lane range, rounded up to whole workgroups, below 2^32 lanes in all
    const u64 room = 0xFFFFFF00ull - 256ull * a.np;
    if (sum_units > room)
        return hipErrorInvalidValue;                      // addk_use_fused keeps such shapes away
    const u64 per = room / sum_units;
    for (u64 e0 = 0; e0 < batch; e0 += per) {
        const u64 ne = std::min(per, batch - e0);
        u32 blocks = 0;
        for (u32 p = 0; p < a.np; ++p) {
            a.first[p] = blocks;
            blocks += ceil_div_u64(ne * units[p], 256u);
            u64 *o = p < sh.w ? outs[p] : carry;
            a.out[p] = reinterpret_cast<Unit *>(o) + e0 * units[p];
        }
        a.first[a.np] = blocks;
        for (u32 j = 0; j < sh.w; ++j)
            a.plane[j] = reinterpret_cast<const Unit *>(planes[j]) + e0 * t[j] * U;
        a.ne = (u32)ne;
        a.xcd = stream_xcd(ne * sum_units);
        k_uint_addk<Unit><<<dim3(blocks), 256, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// The composed form: csgn_chain.h's over the carries, each output plane written with pitched copies when its carry
// comes in.  c_m is a_m itself, read in place; the last carry is written to `carry` when asked and not computed
// otherwise.
hipError_t addk_composed(const AddkShape &sh, u64 n_bits, u64 batch, bool neg, const u64 *const *planes, const u64 *t,
                         u64 *const *outs, u64 *carry, hipStream_t s)
{
    const u64 dL = (n_bits + 63) / 64;
    auto copy = [&](const u64 *src, u64 terms, u64 *dst, u64 pitch) {
        return add_uniform(n_bits, batch, terms, 0, src, nullptr, dst, s, pitch);
    };
    auto ones = [&](u64 *dst, u64 pitch) { return const_fill(n_bits, batch, nullptr, 1, dst, pitch, s); };
    const u32 w = sh.w, m = sh.zero ? w : sh.c.base;
    // out_j, with cur = c_{j-1} (j > m)
    auto plane = [&](u32 j, const u64 *cur) {
        if (j >= w)
            return hipSuccess;
        const u64 pitch = (sh.T[j] + (neg ? 1 : 0)) * dL;
        u64 at = t[j];
        hipError_t e = copy(planes[j], t[j], outs[j], pitch);
        if (e == hipSuccess && j > m) {
            e = copy(cur, sh.c.L[j - 1], outs[j] + at * dL, pitch);
            at += sh.c.L[j - 1];
        }
        if (e == hipSuccess && at < sh.T[j])                  // the ONE of k_j = 1
            e = ones(outs[j] + at++ * dL, pitch);
        if (e == hipSuccess && neg)
            e = ones(outs[j] + at++ * dL, pitch);
        return e;
    };
    if (sh.zero) {                                            // every plane a copy, the carry-out ZERO
        hipError_t e = hipSuccess;
        for (u32 j = 0; j < w && e == hipSuccess; ++j)
            e = plane(j, nullptr);
        return e == hipSuccess && carry ? const_fill(n_bits, batch, nullptr, 0, carry, dL, s) : e;
    }
    return chain_composed(sh.c, carry ? w : w - 1, SCRATCH_UINT_ADDK, n_bits, batch, planes, t, true, carry,
                          sh.c.L[w - 1] * dL, s, plane);
}

} // namespace

// ------------------------------------------------------------------------------ public

bool uint_addk_terms(u64 width, u64 k, const u64 *terms, u64 *out_terms)
{
    AddkShape sh;
    if (!out_terms || !addk_shape(width, k, terms, sh))
        return false;
    std::copy(sh.T, sh.T + width + 1, out_terms);
    return true;
}

const char *uint_addk_kernel_name(u64 n_bits, u64 batch, u64 width, u64 k, const u64 *terms, bool carry)
{
    AddkShape sh;
    if (n_bits == 0 || !addk_shape(width, k, terms, sh))
        return "";
    return addk_use_fused(sh, carry, n_bits, batch) ? "k_uint_addk" : "composed";
}

hipError_t uint_addk(u64 n_bits, u64 batch, u64 width, u64 k, bool negate_out, const u64 *const *planes, const u64 *terms,
                     u64 *const *outs, u64 *carry, hipStream_t s)
{
    AddkShape sh;
    if (!addk_shape(width, k, terms, sh))
        return hipErrorInvalidValue;
    if (batch == 0)
        return hipSuccess;
    if (addk_use_fused(sh, carry != nullptr, n_bits, batch)) {
        const u64 dL = (n_bits + 63) / 64;
        const bool wide = wide_units(dL, carry, ptr_array(outs, sh.w), ptr_array(planes, sh.w));
        const u32 U = (u32)(wide ? dL / 2 : dL);
        return wide ? addk_fused<unit16>(sh, n_bits, batch, negate_out, planes, terms, outs, carry, U, s)
                    : addk_fused<unit8>(sh, n_bits, batch, negate_out, planes, terms, outs, carry, U, s);
    }
    return addk_composed(sh, n_bits, batch, negate_out, planes, terms, outs, carry, s);
}

} // namespace csgn
