// csgn_uint_lut.hip -- a PUBLIC lookup table applied to a bit-sliced encrypted integer, every output plane in one
// launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md §4.15.
//
// The definition (include/csgn_hip.h, csgn_uint_lut_apply) is the table's algebraic normal form over the planes: output
// j is the left-nested sum, ascending in S, of the monomials M_S = a_{i1} * a_{i2} * ... (ascending i, ONE for S = {})
// with bit j of anf[S] set, ZERO when there is none.  A term of a product is the AND of one term per factor, the last
// factor fastest, so term idx of output j is found by
//     the monomial m whose term range [moff[m], moff[m] + prod t_i) holds idx   (fresh planes: m = idx)
//     r = idx - moff[m];  for i in S, highest first:  d_i = r % t_i,  r /= t_i;  AND a_i[d_i]
//
// Fresh planes (every t_i = 1), the case this kernel is built for, read each plane once per workgroup: the workgroup
// builds, for its elements and its slice of units, subset tables in LDS (csgn_device.h) -- table k holds the AND of
// every subset of its planes [hb[k], hb[k+1]) -- and every written unit is T_0[S_0] & T_1[S_1] & T_2[S_2]: one to three
// LDS reads, whatever |S| is.  Lanes walk one output's contiguous term stream, so one store instruction writes 64
// consecutive units of one plane.  Multi-term planes take the decode above straight from the planes (correct, not
// fast).
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>
#include <vector>

namespace csgn {

namespace {

constexpr u64 kLdsBudget = 32768;       // bytes of subset tables per workgroup: four workgroups per CU
constexpr u64 kPartUnits = 8192;        // units a workgroup writes at least, where the shape has them

// By value in the kernel arguments (uniform, scalar loads).  A workgroup is (element group, unit chunk, part): it owns
// elements [group * G, + G), units [chunk * KC, + KC) of every term, and part `part` of the stream of its units laid
// out output by output -- output j's G * T_j * KC units from seg[j] on, element, then term, then unit.
struct LutArgs {
    const void *plane[kLutMaxIn];
    void *out[kLutMaxOut];
    u64 seg[kLutMaxOut + 1];
    u32 T[kLutMaxOut];
    u32 mbase[kLutMaxOut + 1];
    FastDivTable<kLutMaxOut> tk;                                         // T_j * KC
    u32 t[kLutMaxIn];
    const u32 *mono, *moff;
    u64 zero;                 // bit j: output j has an empty ANF (ZERO)
    u64 last_mask;
    u64 batch;                // elements of this launch
    u32 w, m;
    u32 U, KC, G, chunks, parts, nblocks, xcd;
    SubsetTables tabs;
    FastDiv dKC;
};

template <typename Unit, bool Fresh>
__global__ void __launch_bounds__(256) k_uint_lut(LutArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Unit *tab = reinterpret_cast<Unit *>(smem_raw);
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, a.nblocks) : blockIdx.x;
    const u32 gc = bid / a.parts, part = bid - gc * a.parts;
    const u32 group = gc / a.chunks, chunk = gc - group * a.chunks;
    const u64 e0 = (u64)group * a.G;
    const u32 ne = (u32)min((u64)a.G, a.batch - e0);
    const u32 k0 = chunk * a.KC, kc = min(a.KC, a.U - k0);

    if (Fresh)
        subset_build(tab, a.tabs, a.plane, a.G, a.KC, a.dKC, a.U, a.last_mask, e0, ne, k0, kc);

    const u64 W = a.seg[a.m];
    const u64 lo = W * part / a.parts, hi = W * (part + 1u) / a.parts;
    for (u32 j = 0; j < a.m; ++j) {
        const u64 s0 = max(lo, a.seg[j]), s1 = min(hi, a.seg[j + 1]);
        if (s0 >= s1)
            continue;
        const FastDiv dtk = a.tk.at(j);
        const u32 Tj = a.T[j], mb = a.mbase[j];
        const bool zero = (a.zero >> j) & 1u;
        Unit *o = reinterpret_cast<Unit *>(a.out[j]);
        const u32 l1 = (u32)(s1 - a.seg[j]);
        for (u32 l = (u32)(s0 - a.seg[j]) + threadIdx.x; l < l1; l += 256u) {
            const u32 el = csgn_fastdiv(l, dtk), r = l - el * dtk.d;
            const u32 q = csgn_fastdiv(r, a.dKC), kk = r - q * a.KC;
            if (el >= ne || kk >= kc)
                continue;
            const u32 k = k0 + kk;
            const u64 e = e0 + el;
            Unit v;
            if (zero) {
                v = zero_unit(Unit());
            } else if (Fresh) {
                v = subset_and(tab, a.tabs, el, a.mono[mb + q], a.KC, kk);
            } else {
                // the monomial holding term q: the last one of output j starting at or before it
                u32 lo_m = mb, hi_m = a.mbase[j + 1];
                while (hi_m - lo_m > 1u) {
                    const u32 mid = (lo_m + hi_m) >> 1;
                    if (a.moff[mid] <= q)
                        lo_m = mid;
                    else
                        hi_m = mid;
                }
                const u32 S = a.mono[lo_m];
                u32 rr = q - a.moff[lo_m];
                v = one_unit(Unit(), k, a.U, a.last_mask);
                for (u32 i = a.w; i-- > 0u;) {
                    if (!((S >> i) & 1u))
                        continue;
                    const u32 ti = a.t[i], d = rr % ti;
                    rr /= ti;
                    v &= reinterpret_cast<const Unit *>(a.plane[i])[(e * ti + d) * a.U + k];
                }
            }
            unit_store<Unit, true>(o + (e * Tj + q) * a.U + k, v);
        }
    }
}

// ------------------------------------------------------------------------------ the plan on the host

int lut_check(u64 w, u64 m, const u64 *table)
{
    if (w < 1 || w > kLutMaxIn || m < 1 || m > kLutMaxOut || !table)
        return CSGN_ERR_INVALID;
    for (u64 x = 0; x < (1ull << w); ++x)
        if (m < 64 && (table[x] >> m) != 0)
            return CSGN_ERR_INVALID;
    return CSGN_OK;
}

void lut_mobius(u64 w, const u64 *table, u64 *anf)
{
    const u64 n = 1ull << w;
    std::copy(table, table + n, anf);
    for (u64 i = 0; i < w; ++i)
        for (u64 x = 0; x < n; ++x)
            if ((x >> i) & 1u)
                anf[x] ^= anf[x ^ (1ull << i)];
}

// terms of M_S: the product of t_i over S (1 for the empty set); 0 at 2^62 or more
u64 mono_terms(u64 S, const u64 *t)
{
    u64 p = 1;
    for (u32 i = 0; S >> i; ++i) {
        if (!((S >> i) & 1u))
            continue;
        if (!term_mul(p, t[i], p))
            return 0;
    }
    return p;
}

bool lut_use_fused()
{
    // by shape: one launch for every output, no shape measured where the composed form is faster
    return tune_choose(TUNE_UINT_LUT_FUSED, true);
}

// The workgroup shape of one apply: tables, elements per workgroup, unit chunks, parts.
template <typename Unit>
hipError_t lut_fused(const LutPlan &p, u64 n_bits, u64 batch, const u64 *const *planes, u64 *const *out, u32 U,
                     hipStream_t s)
{
    LutArgs a = {};
    a.w = p.w;
    a.m = p.m;
    a.U = U;
    a.last_mask = last_word_mask(n_bits);
    a.mono = p.d_mono;
    a.moff = p.d_moff;
    for (u32 i = 0; i < p.w; ++i)
        a.t[i] = (u32)p.t[i];
    u64 sumT = 0, maxT = 0;
    for (u32 j = 0; j < p.m; ++j) {
        a.T[j] = (u32)p.T[j];
        if (p.mbase[j + 1] == p.mbase[j])
            a.zero |= 1ull << j;
        sumT += p.T[j];
        maxT = std::max(maxT, p.T[j]);
    }
    for (u32 j = 0; j <= p.m; ++j)
        a.mbase[j] = p.mbase[j];
    SubsetPlan sp = subset_plan(p.fresh ? p.w : 0, U, (u32)sizeof(Unit), kLdsBudget);
    a.KC = sp.KC;
    a.chunks = sp.chunks;
    // elements per workgroup: enough to give it kPartUnits to write, as many as the tables allow
    const u64 elem_units = sumT * a.KC;
    u64 G = std::max<u64>(1, kPartUnits / std::max<u64>(elem_units, 1));
    G = std::min<u64>({G, sp.max_G, batch, 64, 0xFFFFFFFFull / (maxT * a.KC)});
    a.G = (u32)std::max<u64>(G, 1);
    a.dKC = csgn_fastdiv_make(a.KC);
    u64 seg = 0;
    for (u32 j = 0; j < p.m; ++j) {
        a.seg[j] = seg;
        const u64 tk = p.T[j] * a.KC;
        a.tk.set(j, (u32)tk);
        seg += a.G * tk;
    }
    a.seg[p.m] = seg;
    // parts: a workgroup's stream split so each part writes kPartUnits, or four times its table build
    const u64 build = a.G * sp.entries * a.KC;
    const u64 target = std::max<u64>(kPartUnits, 4 * build);
    a.parts = (u32)std::min<u64>(std::max<u64>(1, seg / target), 1u << 16);
    const u32 lds = sp.layout(a.G);
    a.tabs = sp.t;
    a.xcd = stream_xcd(batch * sumT * U);
    return launch_groups(launch_blocks(), batch, a.G, (u64)a.chunks * a.parts, [&](u64 e0, u64 ne, u32 nblocks) {
        a.batch = ne;
        for (u32 i = 0; i < p.w; ++i)
            a.plane[i] = reinterpret_cast<const Unit *>(planes[i]) + e0 * p.t[i] * U;
        for (u32 j = 0; j < p.m; ++j)
            a.out[j] = reinterpret_cast<Unit *>(out[j]) + e0 * p.T[j] * U;
        a.nblocks = nblocks;
        if (p.fresh)
            k_uint_lut<Unit, true><<<dim3(a.nblocks), 256, lds, s>>>(a);
        else
            k_uint_lut<Unit, false><<<dim3(a.nblocks), 256, 0, s>>>(a);
    });
}

// The composed form: every monomial through the tuned launchers, written into its slice of the output (pitch T_j):
// ONE by csgn_const_fill, one plane by the strided copy, a product left to right, the last factor written in place.
// The partial products ping-pong through one temporary block (scratch_take, csgn_kernels.h).
hipError_t lut_composed(const LutPlan &p, u64 n_bits, u64 batch, const u64 *const *planes, u64 *const *out,
                        hipStream_t s)
{
    const u64 dL = (n_bits + 63) / 64;
    const std::vector<u32> &mono = p.mono;
    u64 maxP = 0;             // the largest partial product: 2 .. |S| - 1 factors of a monomial
    for (u32 S : mono) {
        u64 prod = 1;
        u32 f = 0;
        const u32 nf = (u32)__builtin_popcount(S);
        for (u32 i = 0; i < p.w; ++i)
            if ((S >> i) & 1u) {
                prod *= p.t[i];
                if (++f >= 2 && f < nf)
                    maxP = std::max(maxP, prod);
            }
    }
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = maxP ? scratch_take(SCRATCH_UINT_LUT, 2 * batch * maxP * dL * 8, s, owned, e) : nullptr;
    if (e != hipSuccess)
        return e;
    for (u32 j = 0; j < p.m && e == hipSuccess; ++j) {
        const u64 pitch = p.T[j] * dL;
        if (p.mbase[j + 1] == p.mbase[j]) {
            e = const_fill(n_bits, batch, nullptr, 0, out[j], pitch, s);
            continue;
        }
        u64 off = 0;
        for (u32 x = p.mbase[j]; x < p.mbase[j + 1] && e == hipSuccess; ++x) {
            const u32 S = mono[x];
            u64 *dst = out[j] + off * dL;
            off += mono_terms(S, p.t);
            if (S == 0) {
                e = const_fill(n_bits, batch, nullptr, 1, dst, pitch, s);
                continue;
            }
            u32 left = (u32)__builtin_ctz(S);
            const u64 *cur = planes[left];
            u64 tc = p.t[left];
            const u32 rest = S & (S - 1u);
            if (rest == 0) {
                e = add_uniform(n_bits, batch, tc, 0, cur, nullptr, dst, s, pitch);
                continue;
            }
            int flip = 0;
            for (u32 r = rest; r && e == hipSuccess; r &= r - 1u) {
                const u32 i = (u32)__builtin_ctz(r);
                const bool last = (r & (r - 1u)) == 0;
                u64 *to = last ? dst : block + (u64)flip * batch * maxP * dL;
                e = mul_uniform(n_bits, batch, tc, p.t[i], cur, planes[i], to, 0, s, last ? pitch : 0);
                cur = to;
                tc *= p.t[i];
                flip ^= 1;
            }
        }
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

int uint_lut_anf(u64 w, u64 m, const u64 *table, u64 *anf)
{
    if (int rc = lut_check(w, m, table))
        return rc;
    if (!anf)
        return CSGN_ERR_INVALID;
    lut_mobius(w, table, anf);
    return CSGN_OK;
}

int uint_lut_terms(u64 w, u64 m, const u64 *table, const u64 *t, u64 *T)
{
    if (int rc = lut_check(w, m, table))
        return rc;
    if (!t || !T)
        return CSGN_ERR_INVALID;
    for (u64 i = 0; i < w; ++i)
        if (t[i] == 0 || t[i] >= kTermLimit)
            return CSGN_ERR_INVALID;
    std::vector<u64> anf(1ull << w);
    lut_mobius(w, table, anf.data());
    std::vector<u64> out(m, 0);
    std::vector<bool> any(m, false);
    for (u64 S = 0; S < anf.size(); ++S) {
        if (!anf[S])
            continue;
        const u64 c = mono_terms(S, t);
        if (!c)
            return CSGN_ERR_INVALID;
        for (u64 j = 0; j < m; ++j)
            if ((anf[S] >> j) & 1u) {
                out[j] += c;
                any[j] = true;
                if (out[j] >= kTermLimit)
                    return CSGN_ERR_INVALID;
            }
    }
    for (u64 j = 0; j < m; ++j)
        T[j] = any[j] ? out[j] : 1;
    return CSGN_OK;
}

int uint_lut_plan_create(u64 w, u64 m, const u64 *table, const u64 *t, LutPlan &p, hipError_t &herr)
{
    herr = hipSuccess;
    p = LutPlan();
    u64 T[kLutMaxOut];
    if (int rc = uint_lut_terms(w, m, table, t, T))
        return rc;
    for (u64 j = 0; j < m; ++j)
        if (T[j] >= (1ull << 31))
            return CSGN_ERR_UNSUPPORTED;
    p.w = (u32)w;
    p.m = (u32)m;
    p.fresh = true;
    for (u64 i = 0; i < w; ++i) {
        p.t[i] = t[i];
        p.fresh = p.fresh && t[i] == 1;
    }
    std::vector<u64> anf(1ull << w);
    lut_mobius(w, table, anf.data());
    std::vector<u32> mono, moff;
    for (u64 j = 0; j < m; ++j) {
        p.T[j] = T[j];
        p.mbase[j] = (u32)mono.size();
        u64 off = 0;
        for (u64 S = 0; S < anf.size(); ++S)
            if ((anf[S] >> j) & 1u) {
                mono.push_back((u32)S);
                moff.push_back((u32)off);
                off += mono_terms(S, t);
            }
    }
    p.mbase[m] = (u32)mono.size();
    const size_t bytes = std::max<size_t>(mono.size(), 1) * sizeof(u32);
    if ((herr = hipMalloc(reinterpret_cast<void **>(&p.d_mono), bytes)) != hipSuccess ||
        (herr = hipMalloc(reinterpret_cast<void **>(&p.d_moff), bytes)) != hipSuccess ||
        (!mono.empty() && (herr = hipMemcpy(p.d_mono, mono.data(), mono.size() * sizeof(u32), hipMemcpyHostToDevice)) != hipSuccess) ||
        (!moff.empty() && (herr = hipMemcpy(p.d_moff, moff.data(), moff.size() * sizeof(u32), hipMemcpyHostToDevice)) != hipSuccess)) {
        uint_lut_plan_free(p);
        return CSGN_ERR_HIP;
    }
    p.mono = std::move(mono);
    return CSGN_OK;
}

void uint_lut_plan_free(LutPlan &p)
{
    if (p.d_mono)
        (void)hipFree(p.d_mono);
    if (p.d_moff)
        (void)hipFree(p.d_moff);
    p.d_mono = p.d_moff = nullptr;
}

const char *uint_lut_kernel_name(const LutPlan &p, u64 n_bits, u64 batch)
{
    (void)n_bits;
    (void)batch;
    if (p.w == 0)
        return "";
    return lut_use_fused() ? "k_uint_lut" : "composed";
}

hipError_t uint_lut(const LutPlan &p, u64 n_bits, u64 batch, const u64 *const *planes, u64 *const *out, hipStream_t s)
{
    if (batch == 0)
        return hipSuccess;
    if (!lut_use_fused())
        return lut_composed(p, n_bits, batch, planes, out, s);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(planes, p.w), ptr_array(out, p.m));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? lut_fused<unit16>(p, n_bits, batch, planes, out, U, s)
                : lut_fused<unit8>(p, n_bits, batch, planes, out, U, s);
}

} // namespace csgn
