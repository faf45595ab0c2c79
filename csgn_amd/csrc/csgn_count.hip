// csgn_count.hip -- encrypted bits counted into encrypted integers: every term of every requested plane of every
// element in one launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md
// §4.21.
//
// The definition (include/csgn_hip.h, csgn_count): bit j of the number of ones among g bits is the elementary
// symmetric polynomial of degree m = 2^j over F2, so output plane j of element q is the left-nested sum, over the
// m-subsets i_1 < ... < i_m of the element's g inputs in lexicographic order, of the left-nested products
// x_{i_1} * ... * x_{i_m}.  Term p decodes as c = p / t^m (the subset's rank) and the base-t digits d_1 .. d_m of
// p mod t^m, d_1 slowest; its words are the AND over k of term d_k of x_{i_k}.
//
// A workgroup owns one element -- or EG consecutive ones where an element's planes are a few units each --, one plane, a
// range of CP combination ranks and a slice of KC units of every term.  It
// stages its elements' g * t input terms in LDS once (plane 1 uses each g - 1 times, higher planes more), writes the
// subsets of its range into LDS -- every thread unranks the first subset of a run of consecutive ranks from binomials
// it computes, and steps to the successors -- and then walks the stream of its outputs with the unit fastest, then
// the digits and the combination, so one store instruction writes 64 consecutive units of one output element.  The
// range of ranks is cut over workgroups so that a single element fills the chip; every part writes its own slice, so
// nothing is accumulated and no atomics are needed.  Inputs past the LDS budget are staged in unit slices; below a
// useful slice they are read straight from memory (Staged = false).
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kLdsBudget = 57344;       // bytes of staged inputs per workgroup; with the subsets 64 KiB: two a CU
constexpr u32 kSubsBytes = 8192;        // bytes of subset indices (16 bits each) per workgroup
constexpr u32 kMinChunk = 16;           // units of a term slice at least, when terms are cut to fit the LDS
constexpr u64 kTargetUnits = 16384;     // units a workgroup writes at most by choice (256 KiB of 16-byte units)
constexpr u64 kMinUnits = 2048;         // ... and at least, when the range of ranks is cut further to fill the chip
constexpr u64 kFillBlocks = 2048;       // workgroups that fill 256 CUs (eight resident each)
constexpr u64 kMaxStream = 0xFFFFFE00ull;  // units of one workgroup's stream at most: its 32-bit index never wraps
constexpr u32 kMaxPlanes = 7;           // j = 0 .. 6
constexpr u32 kMaxIn = 64;              // input batches of the plane layout

// one requested plane.  A workgroup of an element is (plane, part of the ranks, unit chunk), the chunk fastest.
struct CountPlane {
    void *out;
    u64 bbase;                  // the plane's first workgroup among an element's
    u32 m, D;                   // 2^j, t^m
    u32 ncomb, CP;              // C(g, m); ranks a workgroup takes
    FastDiv dD;
    FastDiv dEl;                // EG > 1: the units of one element of the stream, ncomb * D * KC
};

// By value in the kernel arguments (uniform, scalar loads).
struct CountArgs {
    const void *in[kMaxIn];     // n_in == 1: the grouped batch; else input i's batch
    CountPlane p[kMaxPlanes];
    u64 block0;                 // this launch's first workgroup in the call
    u64 per_elem;               // workgroups of one element (of one group of EG elements)
    u64 count;
    u32 EG;                     // elements of a workgroup; above 1 only with whole terms and every plane in one part
    u32 g, t, U, KC, chunks, n_in, n_out, nblocks, xcd;
    u32 sbase;                  // byte offset of the subsets in the LDS
    FastDiv dKC, dT;
    FastDiv dIn;                // EG > 1: the staged units of one element, g * t * KC
};

// input i of element e: its first unit (term 0, unit 0)
template <typename Unit>
__device__ inline const Unit *count_input(const CountArgs &a, u64 e, u32 i)
{
    if (a.n_in == 1)
        return reinterpret_cast<const Unit *>(a.in[0]) + (e * a.g + i) * a.t * a.U;
    return reinterpret_cast<const Unit *>(a.in[i]) + e * a.t * a.U;
}

template <typename Unit, bool Staged, bool Digits>
__global__ void __launch_bounds__(256) k_count(CountArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Unit *xs = reinterpret_cast<Unit *>(smem_raw);                               // [(i * t + d) * KC + kk]
    unsigned short *subs = reinterpret_cast<unsigned short *>(smem_raw + a.sbase);   // [cc * m + k]
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, a.nblocks) : blockIdx.x;
    const u64 B = a.block0 + bid, eg = B / a.per_elem, r = B - eg * a.per_elem, e = eg * a.EG;
    const u32 ne = (u32)min((u64)a.EG, a.count - e);              // elements e .. e + ne - 1
    u32 x = a.n_out - 1u;
    while (x > 0u && a.p[x].bbase > r)
        --x;
    const CountPlane &P = a.p[x];
    const u32 pc = (u32)(r - P.bbase), part = pc / a.chunks, chunk = pc - part * a.chunks;
    const u32 c0 = part * P.CP, nc = min(P.CP, P.ncomb - c0);
    const u32 k0 = chunk * a.KC, kc = min(a.KC, a.U - k0);
    const u32 m = P.m, g = a.g, t = a.t;

    if (Staged) {
        const u32 n = ne * g * t * a.KC;
        for (u32 s = threadIdx.x; s < n; s += 256u) {
            const u32 el = a.EG > 1u ? csgn_fastdiv(s, a.dIn) : 0u, se = s - el * a.dIn.d;
            const u32 it = csgn_fastdiv(se, a.dKC), kk = se - it * a.KC;
            const u32 i = csgn_fastdiv(it, a.dT), d = it - i * t;
            if (kk < kc)
                xs[s] = count_input<Unit>(a, e + el, i)[(u64)d * a.U + k0 + kk];
        }
    }
    // the subsets of ranks [c0, c0 + nc): thread th takes the run [th * run, th * run + run)
    // (m = 1: the subset is the rank itself; C(g, 2) < 2^31 keeps every index of a wider subset within 16 bits)
    {
        const u32 run = (nc + 255u) / 256u, first = threadIdx.x * run;
        if (m > 1u && first < nc) {
            unsigned short *s = subs + first * m;
            unrank(g, m, (u64)c0 + first, [&](u32 k, u32 v) { s[k] = (unsigned short)v; });
            const u32 end = min(first + run, nc);
            for (u32 cc = first + 1u; cc < end; ++cc, s += m) {
                u32 k = m - 1u;                                  // the last position that can still move up
                while (k > 0u && s[k] == g - m + k)
                    --k;
                for (u32 i = 0; i < k; ++i)
                    s[m + i] = s[i];
                const u32 v = s[k] + 1u;
                for (u32 i = k; i < m; ++i)
                    s[m + i] = (unsigned short)(v + (i - k));
            }
        }
    }
    __syncthreads();

    Unit *__restrict__ out = reinterpret_cast<Unit *>(P.out);
    const u32 len = ne * nc * P.D * a.KC;               // (element, combination, digits, unit), below 2^32 by the plan
    for (u32 l = threadIdx.x; l < len; l += 256u) {
        const u32 el = a.EG > 1u ? csgn_fastdiv(l, P.dEl) : 0u, le = l - el * P.dEl.d;
        const u32 cd = csgn_fastdiv(le, a.dKC), kk = le - cd * a.KC;
        if (kk >= kc)
            continue;
        u32 cc = cd, dd = 0;
        if (Digits) {
            cc = csgn_fastdiv(cd, P.dD);
            dd = cd - cc * P.D;
        }
        const unsigned short *s = subs + cc * m;
        Unit v = ~zero_unit(Unit());
        u32 rest = dd;
        for (u32 k = m; k-- > 0u;) {                             // the last factor's digit is the fastest
            u32 d = 0;
            if (Digits) {
                const u32 q = csgn_fastdiv(rest, a.dT);
                d = rest - q * t;
                rest = q;
            }
            const u32 i = m > 1u ? s[k] : c0 + cc;
            Unit w;
            if (Staged)
                w = xs[el * a.dIn.d + (i * t + d) * a.KC + kk];
            else
                w = count_input<Unit>(a, e + el, i)[(u64)d * a.U + k0 + kk];
            v &= w;
        }
        unit_store<Unit, true>(out + (((e + el) * P.ncomb + c0 + cc) * P.D + dd) * a.U + k0 + kk, v);
    }
}

// the m index lists of the composed form: pair x = p0 + ... is (element q, subset of rank c), q = p / ncomb; list k
// holds the element of the grouped batch that is factor k, q * g + i_k
__global__ void __launch_bounds__(256) k_count_index(u64 p0, u64 np, u32 g, u32 m, u32 ncomb, u64 *__restrict__ idx)
{
    for (u64 x = (u64)blockIdx.x * 256u + threadIdx.x; x < np; x += (u64)gridDim.x * 256u) {
        const u64 p = p0 + x, q = p / ncomb;
        unrank(g, m, p - q * ncomb, [&](u32 k, u32 v) { idx[(u64)k * np + x] = q * g + v; });
    }
}

// ------------------------------------------------------------------------------ host side

// t^m; false when it reaches kTermLimit
bool count_digits(u64 t, u32 m, u64 &D)
{
    D = 1;
    for (u32 k = 0; k < m && t > 1; ++k)
        if (!term_mul(D, t, D))
            return false;
    return true;
}

// C(g, m) below kTermLimit, or 0: the values on the way only grow, so the first that passes the limit settles it
u64 count_binom(u64 g, u64 m)
{
    if (m > g)
        return 0;
    const u64 k = std::min(m, g - m);
    unsigned __int128 c = 1;
    for (u64 i = 1; i <= k; ++i) {
        c = c * (g - k + i) / i;
        if (c >= kTermLimit)
            return 0;
    }
    return (u64)c;
}

struct CountShape {
    u32 n_out;
    u32 m[kMaxPlanes];
    u64 ncomb[kMaxPlanes], D[kMaxPlanes];
};

// the planes of a valid call (count_shape_ok) whose sizes the C ABI has checked: every C(g, m) * t^m * dL below 2^31
CountShape count_shape(u64 group, u64 t, u64 n_out, const u64 *js)
{
    CountShape s = {};
    s.n_out = (u32)n_out;
    for (u32 x = 0; x < s.n_out; ++x) {
        s.m[x] = 1u << js[x];
        s.ncomb[x] = count_binom(group, s.m[x]);
        count_digits(t, s.m[x], s.D[x]);
    }
    return s;
}

// Per shape: the fused kernel.  The composed form goes through the gather launcher, which takes fewer
// than 2^32 elements: a call of 2^32 inputs or more is fused whatever the knob says.
bool count_use_fused(u64 count, u64 group)
{
    unsigned long long inputs;
    if (__builtin_mul_overflow((unsigned long long)count, (unsigned long long)group, &inputs) || inputs >= (1ull << 32))
        return true;
    return tune_choose(TUNE_COUNT_FORM, true);
}

template <typename Unit>
hipError_t count_fused(u64 count, u64 group, u64 t, const u64 *const *in, u64 n_in, const CountShape &s,
                       u64 *const *out, u32 U, hipStream_t st)
{
    const u64 ub = sizeof(Unit);
    CountArgs a = {};
    for (u64 i = 0; i < n_in; ++i)
        a.in[i] = in[i];
    a.g = (u32)group;
    a.t = (u32)t;
    a.U = U;
    a.n_in = (u32)n_in;
    a.n_out = s.n_out;
    // the slice of units: whole terms unless the element's inputs pass the budget; no staging below kMinChunk units
    // a slice
    u64 KC = U;
    bool staged = true;
    unsigned long long in_units;
    if (__builtin_mul_overflow((unsigned long long)group, (unsigned long long)t, &in_units) || in_units > kLdsBudget) {
        staged = false;
    } else if (in_units * U * ub > kLdsBudget) {
        const u64 fit = kLdsBudget / (in_units * ub);
        if (fit >= kMinChunk) {
            const u64 chunks = (U + fit - 1) / fit;
            KC = (U + chunks - 1) / chunks;
        } else {
            staged = false;
        }
    }
    a.KC = (u32)KC;
    a.chunks = (u32)((U + KC - 1) / KC);
    // the ranks of a workgroup, plane by plane: what the subset table holds, no more than kTargetUnits to write, parts
    // enough to fill the chip, evened out over the parts; or what knob count_cpart says, which is how the tests place
    // the split
    const int forced = tune(TUNE_COUNT_CPART);
    u64 per_elem = 0, units = 0;
    u32 sub_bytes = 0;
    bool digits = false;
    for (u32 x = 0; x < s.n_out; ++x) {
        CountPlane &P = a.p[x];
        const u64 m = s.m[x], ncomb = s.ncomb[x], cell = s.D[x] * KC;       // cell: units of one combination here
        const u64 capC = std::min<u64>({ncomb, std::max<u64>(1, kSubsBytes / (2 * m)), std::max<u64>(1, kMaxStream / cell)});
        u64 CP;
        if (forced > 0) {
            CP = std::min<u64>((u64)forced, capC);
        } else {
            CP = std::min<u64>(capC, std::max<u64>(1, (kTargetUnits + cell - 1) / cell));
            while (CP > 1 && count < kFillBlocks && count * a.chunks * ((ncomb + CP - 1) / CP) < kFillBlocks &&
                   ((CP + 1) / 2) * cell >= kMinUnits)
                CP = (CP + 1) / 2;
            const u64 parts = (ncomb + CP - 1) / CP;
            CP = (ncomb + parts - 1) / parts;
        }
        P.out = out[x];
        P.m = (u32)m;
        P.D = (u32)s.D[x];
        P.ncomb = (u32)ncomb;
        P.CP = (u32)CP;
        P.dD = csgn_fastdiv_make(P.D);
        P.bbase = per_elem;
        per_elem += ((ncomb + CP - 1) / CP) * a.chunks;
        units += ncomb * s.D[x] * U;
        if (m > 1)                                      // plane 0's subset is its rank (and g may pass 16 bits there)
            sub_bytes = std::max<u32>(sub_bytes, (u32)(CP * m * 2));
        digits = digits || s.D[x] > 1;
    }
    // several elements a workgroup: where every plane of an element is one workgroup of whole staged terms that writes
    // under half of kTargetUnits, EG doubles while the inputs fit the budget, the largest plane stays within
    // kTargetUnits and the workgroups still fill the chip
    u64 EG = 1;
    if (forced <= 0 && staged && a.chunks == 1 && per_elem == s.n_out) {
        u64 largest = 0;
        for (u32 x = 0; x < s.n_out; ++x)
            largest = std::max(largest, s.ncomb[x] * s.D[x] * U);
        while (2 * EG * largest <= kTargetUnits && 2 * EG * in_units * U * ub <= kLdsBudget &&
               (count + 2 * EG - 1) / (2 * EG) >= kFillBlocks)
            EG *= 2;
    }
    a.EG = (u32)EG;
    a.count = count;
    a.per_elem = per_elem;
    a.dKC = csgn_fastdiv_make(a.KC);
    a.dT = csgn_fastdiv_make(a.t);
    a.dIn = csgn_fastdiv_make((u32)(in_units * KC));
    for (u32 x = 0; x < s.n_out; ++x)
        a.p[x].dEl = csgn_fastdiv_make((u32)(s.ncomb[x] * s.D[x] * KC));
    a.sbase = staged ? (u32)((EG * in_units * KC * ub + 15u) & ~15ull) : 0u;
    const u32 lds = a.sbase + sub_bytes;
    a.xcd = stream_xcd(count * units);
    // the launches: the workgroups of the call in order, launch_blocks() at a time
    const u64 total = ((count + EG - 1) / EG) * per_elem, max_blocks = launch_blocks();
    for (u64 b0 = 0; b0 < total; b0 += max_blocks) {
        a.block0 = b0;
        a.nblocks = (u32)std::min(max_blocks, total - b0);
        const dim3 grid(a.nblocks);
        if (staged && digits)
            k_count<Unit, true, true><<<grid, 256, lds, st>>>(a);
        else if (staged)
            k_count<Unit, true, false><<<grid, 256, lds, st>>>(a);
        else if (digits)
            k_count<Unit, false, true><<<grid, 256, lds, st>>>(a);
        else
            k_count<Unit, false, false><<<grid, 256, lds, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// The composed form through the tuned launchers.  The plane layout is first interleaved into one grouped batch (one
// pitched copy per input).  Then, per plane and per slice of the count * C(g, m) pairs (element, subset): k_count_index
// writes the m index lists, csgn_gather's launcher tiles factor k to one element per pair, and m - 1 uniform multiplies
// build the product left to right, the last straight into the output -- pair c of element q is exactly terms
// [c * t^m, (c + 1) * t^m) of plane j.  Plane 0 is the one gather.  The temporaries (the grouped copy, two tiled
// factors, two running products and the lists) live in one block (scratch_take, csgn_kernels.h); the gather takes fewer
// than 2^32 elements and the block stays near kComposedBytes, so a large plane goes in slices of pairs.
constexpr u64 kComposedSlice = 1ull << 31;
constexpr u64 kComposedBytes = 1ull << 30;

hipError_t count_composed(u64 n_bits, u64 count, u64 group, u64 t, const u64 *const *in, u64 n_in, const CountShape &s,
                          u64 *const *out, hipStream_t st)
{
    const u64 dL = (n_bits + 63) / 64, tw = t * dL;
    const u64 grouped_words = n_in > 1 ? count * group * tw : 0;
    // words a pair needs at most over the planes: two tiled factors, two running products of t^(m-1) terms, m indices
    u64 per_pair = 0, max_pairs = 0;
    for (u32 x = 0; x < s.n_out; ++x) {
        const u64 acc = s.m[x] > 2 ? 2 * (s.D[x] / t) * dL : 0;
        per_pair = std::max(per_pair, 2 * tw + acc + s.m[x]);
        max_pairs = std::max(max_pairs, count * s.ncomb[x]);
    }
    const u64 slice = std::min<u64>({max_pairs, kComposedSlice, std::max<u64>(1, kComposedBytes / (per_pair * 8))});
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *block = scratch_take(SCRATCH_COUNT, (grouped_words + slice * per_pair) * 8, st, owned, e);
    if (e != hipSuccess)
        return e;
    const u64 *grouped = in[0];
    if (n_in > 1) {
        for (u64 i = 0; i < group && e == hipSuccess; ++i)
            e = add_uniform(n_bits, count, t, 0, in[i], nullptr, block + i * tw, st, group * tw);
        grouped = block;
    }
    u64 *const work = block + grouped_words;
    for (u32 x = 0; x < s.n_out && e == hipSuccess; ++x) {
        const u64 m = s.m[x], pairs = count * s.ncomb[x], Dprev = s.D[x] / t;
        u64 *tiled[2] = {work, work + slice * tw};
        u64 *acc[2] = {tiled[1] + slice * tw, tiled[1] + slice * tw + (m > 2 ? slice * Dprev * dL : 0)};
        u64 *idx = acc[1] + (m > 2 ? slice * Dprev * dL : 0);
        for (u64 p0 = 0; p0 < pairs && e == hipSuccess; p0 += slice) {
            const u64 np = std::min(slice, pairs - p0);
            u64 *dst = out[x] + p0 * s.D[x] * dL;
            const u32 blocks = (u32)std::min<u64>((np + 255) / 256, 8192);
            k_count_index<<<blocks, 256, 0, st>>>(p0, np, (u32)group, (u32)m, (u32)s.ncomb[x], idx);
            e = hipGetLastError();
            const u64 *left = nullptr;
            u64 tl = t;
            for (u64 k = 0; k < m && e == hipSuccess; ++k) {
                u64 *factor = m == 1 ? dst : tiled[k == 0 ? 0 : 1];
                e = gather_planes(n_bits, 1, &grouped, &t, count * group, np, idx + k * np, &factor, st);
                if (k == 0) {
                    left = factor;
                    continue;
                }
                if (e != hipSuccess)
                    break;
                u64 *prod = k == m - 1 ? dst : acc[k & 1];
                e = mul_uniform(n_bits, np, tl, t, left, factor, prod, 0, st);
                left = prod;
                tl *= t;
            }
        }
    }
    return scratch_done(block, owned, e);
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 count_terms(u64 group, u64 t, u64 j)
{
    if (group == 0 || t == 0 || t >= kTermLimit || j > 6 || (1ull << j) > group)
        return 0;
    const u64 C = count_binom(group, 1ull << j);
    u64 D, T;
    if (C == 0 || !count_digits(t, 1u << j, D) || !term_mul(C, D, T))
        return 0;
    return T;
}

bool count_shape_ok(u64 count, u64 group, u64 t, u64 n_in, u64 n_out, const u64 *js)
{
    if (count == 0 || group == 0 || t == 0 || t >= kTermLimit || n_out == 0 || !js)
        return false;
    if (n_in != 1 && (n_in != group || n_in > kMaxIn))
        return false;
    for (u64 x = 0; x < n_out; ++x)
        if (js[x] > 6 || (1ull << js[x]) > group || (x && js[x] <= js[x - 1]))
            return false;
    return true;
}

const char *count_kernel_name(u64 n_bits, u64 count, u64 group, u64 t, u64 n_in, u64 n_out, const u64 *js)
{
    if (n_bits == 0 || !count_shape_ok(count, group, t, n_in, n_out, js))
        return "";
    for (u64 x = 0; x < n_out; ++x)
        if (count_terms(group, t, js[x]) == 0)
            return "";
    return count_use_fused(count, group) ? "k_count" : "composed";
}

hipError_t count(u64 n_bits, u64 count, u64 group, u64 t, const u64 *const *in, u64 n_in, u64 n_out, const u64 *js,
                 u64 *const *out, hipStream_t stream)
{
    const CountShape s = count_shape(group, t, n_out, js);
    if (!count_use_fused(count, group))
        return count_composed(n_bits, count, group, t, in, n_in, s, out, stream);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(in, n_in), ptr_array(out, n_out));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? count_fused<unit16>(count, group, t, in, n_in, s, out, U, stream)
                : count_fused<unit8>(count, group, t, in, n_in, s, out, U, stream);
}

} // namespace csgn
