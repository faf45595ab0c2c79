// csgn_wsum.hip -- encrypted integers summed into encrypted integers: every term of every requested plane of every
// element in one launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md
// §4.27.
//
// The definition (include/csgn_hip.h, csgn_wsum): bit j of the sum of bits x_i of public weights 2^{c_i} is the sum,
// over the subsets whose weights add up to exactly 2^j, of the product of their members.  A subset is a count vector
// (m_j .. m_0), m_c members of class c with sum m_c 2^c = 2^j, and a selection: one m_c-subset of every class.  Output
// plane j is the concatenation over the vectors (ascending, m_j most significant), then over the selections (class j
// slowest, every class in lexicographic order) of the left-nested product of the members, classes descending.
//
// The host plan (csgn_wsum_create) enumerates the vectors once and cuts every vector's selection ranks into parts; a
// workgroup owns one element -- or EG consecutive ones where the parts are a few units each --, one plane, one part of
// one vector and a slice of KC units of every term, so the degree and the digit count are workgroup-uniform.  It is
// k_count (csgn_count.hip) with one more level: it stages the inputs of the classes that take part in LDS once, finds
// its vector by a search of the plane's table, decodes the ranks of its part by mixed radix over the classes -- every
// thread unranks the first selection of a run from binomials it computes and steps to the successors, an odometer
// over the classes -- writes the members to LDS as 16-bit indices into the staged inputs, and then walks the stream of
// its outputs with the unit fastest, then the digits and the selection.  Every part writes its own slice: nothing is
// accumulated and there are no atomics.  Inputs past the LDS budget are staged in unit slices; below a useful slice
// they are read straight from memory (Staged = false).
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u64 kLdsBudget = 57344;       // bytes of staged inputs per workgroup (k_count's budget)
constexpr u32 kSubsBytes = 6144;        // bytes of member indices (16 bits each) per workgroup
constexpr u32 kMetaBytes = 2048;        // the unstaged form's class table; with the two above 64 KiB: two a CU
constexpr u32 kMinChunk = 16;           // units of a term slice at least, when terms are cut to fit the LDS
constexpr u64 kPartTerms = 1024;        // terms a part writes at most by choice (16 384 units at 16 units a term)
constexpr u64 kTargetUnits = 16384;     // units a workgroup of several elements writes at most
constexpr u64 kFillBlocks = 2048;       // workgroups that fill 256 CUs (eight resident each)
constexpr u32 kRec = 8;                 // words of a vector's record in front of its m_c and C(n_c, m_c)

// record of a vector in the device table: {first term, selections, degree, D = t^degree, selections a part, first
// part, D's FastDiv magic and shift}, then m_c and then C(n_c, m_c) for c = 0 .. ncls - 1
enum { V_FIRST, V_NSEL, V_DEG, V_D, V_CP, V_PBASE, V_DMAGIC, V_DSHIFT };

// one requested plane.  A workgroup of an element is (part of the plane, unit chunk), the chunk fastest.
struct WsumPlaneArg {
    void *out;
    u64 bbase;                  // the plane's first workgroup among an element's
    u32 vbase;                  // the plane's first record: word offset into the table
    u32 nvec, ncls, T;          // vectors; classes 0 .. ncls - 1 take part; terms of an output element
};

// By value in the kernel arguments (uniform, scalar loads).
struct WsumArgs {
    const void *in[kWsumMaxClasses];
    u32 n[kWsumMaxClasses];
    u32 base[kWsumMaxClasses + 1];      // inputs of the classes below c: the index of class c's first in the LDS
    WsumPlaneArg p[kWsumMaxPlanes];
    const u32 *vt;
    u64 block0;                 // this launch's first workgroup in the call
    u64 per_elem;               // workgroups of one element (of one group of EG elements)
    u64 count;
    u32 EG;                     // elements of a workgroup; above 1 only with whole staged terms
    u32 t, U, KC, chunks, n_out, nblocks, xcd;
    u32 sbase, mbase;           // byte offsets of the member indices and of the class table in the LDS
    u32 in_el;                  // the staged units of one element: inputs of the classes that take part * t * KC
    FastDiv dKC, dT;
};

// the class of staged input ii: the last c with base[c] <= ii (classes of no inputs are passed over)
__device__ inline u32 class_of(const u32 *base, u32 ncls, u32 ii)
{
    u32 lo = 0, hi = ncls;
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (base[mid] <= ii)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

template <typename Unit, bool Staged, bool Digits>
__global__ void __launch_bounds__(256) k_wsum(WsumArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Unit *xs = reinterpret_cast<Unit *>(smem_raw);                               // [el][((base_c + i) * t + d) * KC + kk]
    unsigned short *subs = reinterpret_cast<unsigned short *>(smem_raw + a.sbase);   // [cc * deg + k]
    u32 *mbase = reinterpret_cast<u32 *>(smem_raw + a.mbase);                    // Staged = false: base[], n[], in[]
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, a.nblocks) : blockIdx.x;
    const u64 B = a.block0 + bid, eg = B / a.per_elem, r = B - eg * a.per_elem, e = eg * a.EG;
    const u32 ne = (u32)min((u64)a.EG, a.count - e);              // elements e .. e + ne - 1
    u32 x = a.n_out - 1u;
    while (x > 0u && a.p[x].bbase > r)
        --x;
    const WsumPlaneArg &P = a.p[x];
    const u32 pc = (u32)(r - P.bbase), part = pc / a.chunks, chunk = pc - part * a.chunks;
    const u32 ncls = P.ncls, rec = kRec + 2u * ncls, t = a.t;
    // the vector of this part: the last whose first part is at most `part`
    const u32 *V = a.vt + P.vbase;
    {
        u32 lo = 0, hi = P.nvec;
        while (hi - lo > 1u) {
            const u32 mid = (lo + hi) >> 1;
            if (V[mid * rec + V_PBASE] <= part)
                lo = mid;
            else
                hi = mid;
        }
        V += lo * rec;
    }
    const u32 deg = V[V_DEG], D = V[V_D], CP = V[V_CP];
    const FastDiv dD = {D, V[V_DMAGIC], V[V_DSHIFT]};
    const u32 *vm = V + kRec, *vr = vm + ncls;
    const u32 c0 = (part - V[V_PBASE]) * CP, nc = min(CP, V[V_NSEL] - c0);
    const u32 k0 = chunk * a.KC, kc = min(a.KC, a.U - k0);

    if (Staged) {
        // class c of elements e .. e + ne - 1 is one run of ne * n_c * t terms
        for (u32 c = 0; c < ncls; ++c) {
            const u32 nn = a.n[c];
            if (nn == 0u)
                continue;
            const Unit *src = reinterpret_cast<const Unit *>(a.in[c]) + e * nn * t * a.U;
            const u32 per = nn * t, n = ne * per * a.KC, at = a.base[c] * t;
            for (u32 s = threadIdx.x; s < n; s += 256u) {
                const u32 it = csgn_fastdiv(s, a.dKC), kk = s - it * a.KC;
                const u32 el = a.EG > 1u ? it / per : 0u;
                if (kk < kc)
                    xs[el * a.in_el + (at + it - el * per) * a.KC + kk] = src[(u64)it * a.U + k0 + kk];
            }
        }
    } else {
        for (u32 c = threadIdx.x; c < ncls; c += 256u) {
            mbase[c] = a.base[c];
            mbase[kWsumMaxClasses + c] = a.n[c];
            reinterpret_cast<const void **>(mbase + 2u * kWsumMaxClasses)[c] = a.in[c];
        }
    }
    // the selections of ranks [c0, c0 + nc): thread th takes the run [th * run, th * run + run)
    {
        const u32 run = (nc + 255u) / 256u, first = threadIdx.x * run;
        if (first < nc) {
            unsigned short *s = subs + first * deg;
            u32 rk = c0 + first, pos = deg;
            for (u32 c = 0; c < ncls; ++c) {                     // class 0 is the fastest digit and the last factors
                const u32 m = vm[c];
                if (m == 0u)
                    continue;
                pos -= m;
                const u32 radix = vr[c], q = rk / radix, rc = rk - q * radix, b = a.base[c];
                rk = q;
                unsigned short *sc = s + pos;
                if (m == 1u)
                    sc[0] = (unsigned short)(b + rc);
                else
                    unrank(a.n[c], m, (u64)rc, [&](u32 k, u32 v) { sc[k] = (unsigned short)(b + v); });
            }
            const u32 end = min(first + run, nc);
            for (u32 cc = first + 1u; cc < end; ++cc, s += deg) {
                for (u32 i = 0; i < deg; ++i)
                    s[deg + i] = s[i];
                pos = deg;
                for (u32 c = 0; c < ncls; ++c) {                 // the odometer: the first class that can step does
                    const u32 m = vm[c];
                    if (m == 0u)
                        continue;
                    pos -= m;
                    unsigned short *sc = s + deg + pos;
                    const u32 top = a.base[c] + a.n[c] - m;      // position k of a class's last subset holds top + k
                    u32 k = m - 1u;                              // the last position that can still move up
                    while (k > 0u && sc[k] == top + k)
                        --k;
                    if (sc[k] == top + k) {                      // the last subset: back to the first, carry
                        for (u32 i = 0; i < m; ++i)
                            sc[i] = (unsigned short)(a.base[c] + i);
                        continue;
                    }
                    const u32 v = sc[k] + 1u;
                    for (u32 i = k; i < m; ++i)
                        sc[i] = (unsigned short)(v + (i - k));
                    break;
                }
            }
        }
    }
    __syncthreads();

    Unit *__restrict__ out = reinterpret_cast<Unit *>(P.out);
    const u32 el_len = nc * D * a.KC, len = ne * el_len;        // (element, selection, digits, unit), below 2^32 by the plan
    const FastDiv dEl = a.EG > 1u ? csgn_fastdiv_make(el_len) : FastDiv{el_len, 0u, 0u};
    for (u32 l = threadIdx.x; l < len; l += 256u) {
        const u32 el = a.EG > 1u ? csgn_fastdiv(l, dEl) : 0u, le = l - el * el_len;
        const u32 cd = csgn_fastdiv(le, a.dKC), kk = le - cd * a.KC;
        if (kk >= kc)
            continue;
        u32 cc = cd, dd = 0;
        if (Digits) {
            cc = csgn_fastdiv(cd, dD);
            dd = cd - cc * D;
        }
        const unsigned short *s = subs + cc * deg;
        Unit v = ~zero_unit(Unit());
        u32 rest = dd;
        for (u32 k = deg; k-- > 0u;) {                           // the last factor's digit is the fastest
            u32 d = 0;
            if (Digits) {
                const u32 q = csgn_fastdiv(rest, a.dT);
                d = rest - q * t;
                rest = q;
            }
            const u32 ii = s[k];
            Unit w;
            if (Staged) {
                w = xs[el * a.in_el + (ii * t + d) * a.KC + kk];
            } else {
                const u32 c = class_of(mbase, ncls, ii), nn = mbase[kWsumMaxClasses + c];
                const Unit *src = reinterpret_cast<const Unit *const *>(mbase + 2u * kWsumMaxClasses)[c];
                w = src[(((e + el) * nn + (ii - mbase[c])) * t + d) * a.U + k0 + kk];
            }
            v &= w;
        }
        unit_store<Unit, true>(out + (((e + el) * P.T + V[V_FIRST]) + (u64)(c0 + cc) * D + dd) * a.U + k0 + kk, v);
    }
}

// ------------------------------------------------------------------------------ host side

constexpr u64 kSat = kTermLimit;        // a saturated count: 2^62 "or more"

u64 sat_mul(u64 x, u64 y)
{
    u64 p;
    if (x == 0 || y == 0)
        return 0;
    return term_mul(x, y, p) ? p : kSat;
}

u64 sat_add(u64 x, u64 y) { return std::min(kSat, x + y); }      // both at most 2^62: no wrap

// C(n, m) * t^m for m = 0 .. n, saturated.  The binomials grow up to the middle and mirror: once one saturates, every
// one up to its mirror image does.
std::vector<u64> class_weights(u64 n, u64 t)
{
    std::vector<u64> w(n + 1, kSat);
    unsigned __int128 c = 1;
    for (u64 m = 0; m <= n / 2; ++m) {
        if (m) {
            c = c * (n - m + 1) / m;
            if (c >= kSat)
                break;
        }
        w[m] = w[n - m] = (u64)c;
    }
    u64 p = 1;
    for (u64 m = 0; m <= n; ++m) {
        w[m] = sat_mul(w[m], p);
        p = sat_mul(p, t);
    }
    return w;
}

enum WsumCount { WSUM_BAD, WSUM_EMPTY, WSUM_SATURATED, WSUM_OK };

bool wsum_shape_ok(u64 C, const u64 *n, u64 t)
{
    if (!n || C < 1 || C > kWsumMaxClasses || t == 0 || t >= kTermLimit)
        return false;
    u64 all = 0;
    for (u64 c = 0; c < C; ++c) {
        if (n[c] > kWsumMaxInputs)
            return false;
        all += n[c];
    }
    return all >= 1 && all <= kWsumMaxInputs;
}

// T_j = the coefficient of z^(2^j) in prod_c (1 + t z^(2^c))^(n_c), class by class from the lightest: A[k] is the
// weight of the selections among the classes below c that total k 2^c; only an even k + m_c carries on to class c + 1.
WsumCount wsum_count(u64 C, const u64 *n, u64 t, u64 j, u64 &T)
{
    T = 0;
    if (!wsum_shape_ok(C, n, t) || j > kWsumMaxPlane)
        return WSUM_BAD;
    std::vector<u64> A(1, 1), next;
    const u64 top = std::min<u64>(j, C - 1);
    for (u64 c = 0; c <= top; ++c) {
        const u64 limit = 1ull << (j - c);                      // k + m_c at most: the total stays within 2^j
        const std::vector<u64> w = class_weights(n[c], t);
        if (c == j) {                                            // k + m_j = 1
            const u64 a0 = A[0], a1 = A.size() > 1 ? A[1] : 0;
            T = sat_add(sat_mul(a0, n[c] >= 1 ? w[1] : 0), a1);
            A.clear();
            break;
        }
        const u64 reach = std::min<u64>(limit, A.size() - 1 + n[c]);
        next.assign(reach / 2 + 1, 0);
        for (u64 k = 0; k < A.size(); ++k) {
            if (A[k] == 0)
                continue;
            for (u64 m = k & 1; m <= n[c] && k + m <= limit; m += 2)
                next[(k + m) / 2] = sat_add(next[(k + m) / 2], sat_mul(A[k], w[m]));
        }
        A.swap(next);
    }
    if (!A.empty()) {                                            // the classes C .. j are empty: k 2^C = 2^j
        const u64 k = 1ull << (j - C);
        T = k < A.size() ? A[k] : 0;
    }
    if (T == 0)
        return WSUM_EMPTY;
    return T >= kSat ? WSUM_SATURATED : WSUM_OK;
}

// C(n, m) of a vector's class: below 2^31 like the plane's terms, or 0
u64 small_binom(u64 n, u64 m)
{
    const u64 k = std::min(m, n - m);
    unsigned __int128 c = 1;
    for (u64 i = 1; i <= k; ++i) {
        c = c * (n - k + i) / i;
        if (c >= (1ull << 31))
            return 0;
    }
    return (u64)c;
}

// the vectors of one plane in ascending order, m_j most significant: class c takes m_c = lo .. hi, where the classes
// below can still make up the rest (they can whenever their inputs weigh that much: the rest is a multiple of 2^c)
struct VectorWalk {
    const WsumPlan &p;
    u32 ncls;
    unsigned __int128 below[kWsumMaxClasses + 1];               // the weight of every input of the classes below c
    u32 m[kWsumMaxClasses];
    std::vector<u32> &vt;
    u64 first = 0, vectors = 0, parts = 0, max_part = 0;
    u32 sub_bytes = 0;
    int forced;
    int status = CSGN_OK;

    void emit()
    {
        u64 nsel = 1, deg = 0, radix[kWsumMaxClasses];
        for (u32 c = 0; c < ncls; ++c) {
            radix[c] = small_binom(p.n[c], m[c]);
            nsel = radix[c] ? nsel * radix[c] : 1ull << 31;
            if (nsel >= (1ull << 31)) {
                status = CSGN_ERR_UNSUPPORTED;
                return;
            }
            deg += m[c];
        }
        u64 D = 1;
        for (u64 k = 0; k < deg && p.t > 1; ++k) {
            D *= p.t;
            if (D >= (1ull << 31)) {
                status = CSGN_ERR_UNSUPPORTED;
                return;
            }
        }
        if (nsel * D >= (1ull << 31) || first + nsel * D >= (1ull << 31) || deg * 2 > kSubsBytes ||
            ++vectors > kWsumMaxVectors) {
            status = CSGN_ERR_UNSUPPORTED;
            return;
        }
        // the selections of a part: what the index table holds, no more than kPartTerms terms, evened out over the
        // parts; or what knob wsum_cpart says, which is how the tests place the split
        const u64 cap = std::min<u64>(nsel, kSubsBytes / (2 * deg));
        u64 CP;
        if (forced > 0) {
            CP = std::min<u64>((u64)forced, cap);
        } else {
            CP = std::min<u64>(cap, std::max<u64>(1, kPartTerms / D));
            const u64 np = (nsel + CP - 1) / CP;
            CP = (nsel + np - 1) / np;
        }
        const FastDiv dD = csgn_fastdiv_make((u32)D);
        const u32 head[kRec] = {(u32)first, (u32)nsel, (u32)deg, (u32)D, (u32)CP, (u32)parts, dD.magic, dD.shift};
        vt.insert(vt.end(), head, head + kRec);
        vt.insert(vt.end(), m, m + ncls);
        for (u32 c = 0; c < ncls; ++c)
            vt.push_back((u32)radix[c]);
        first += nsel * D;
        parts += (nsel + CP - 1) / CP;
        max_part = std::max(max_part, CP * D);
        sub_bytes = std::max<u32>(sub_bytes, (u32)(CP * deg * 2));
    }

    void walk(u32 c, u64 rest)                                   // rest: what the classes c .. 0 must add up to
    {
        const u64 w = 1ull << c, most = std::min<u64>(p.n[c], rest >> c);
        if (c == 0) {
            if (rest <= p.n[0]) {
                m[0] = (u32)rest;
                emit();
            }
            return;
        }
        const u64 least = rest > below[c] ? (u64)((rest - below[c] + w - 1) >> c) : 0;
        for (u64 k = least; k <= most && status == CSGN_OK; ++k) {
            m[c] = (u32)k;
            walk(c - 1, rest - (k << c));
        }
    }
};

template <typename Unit>
hipError_t wsum_fused(const WsumPlan &p, u64 count, const u64 *const *in, u64 *const *out, u32 U, hipStream_t st)
{
    const u64 ub = sizeof(Unit), t = p.t;
    WsumArgs a = {};
    u32 top = 0;                                                 // classes that take part in some plane
    for (u32 x = 0; x < p.n_out; ++x)
        top = std::max(top, p.ncls[x]);
    for (u32 c = 0; c < p.C; ++c) {
        a.in[c] = in[c];
        a.n[c] = p.n[c];
        a.base[c + 1] = a.base[c] + p.n[c];
    }
    a.vt = p.d_vt;
    a.t = (u32)t;
    a.U = U;
    a.n_out = p.n_out;
    // the slice of units: whole terms unless the element's inputs pass the budget; no staging below kMinChunk units
    // a slice
    const u64 in_units = (u64)a.base[top] * t;
    u64 KC = U;
    bool staged = true;
    if (in_units > kLdsBudget) {
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
    u64 per_elem = 0, units = 0;
    for (u32 x = 0; x < p.n_out; ++x) {
        WsumPlaneArg &P = a.p[x];
        P.out = out[x];
        P.bbase = per_elem;
        P.vbase = p.vbase[x];
        P.nvec = p.nvec[x];
        P.ncls = p.ncls[x];
        P.T = (u32)p.T[x];
        per_elem += (u64)p.parts[x] * a.chunks;
        units += p.T[x] * U;
    }
    // several elements a workgroup: with whole staged terms, EG doubles while the largest part of EG elements stays
    // within kTargetUnits, the inputs fit the budget and the workgroups still fill the chip
    u64 EG = 1;
    if (staged && a.chunks == 1)
        while (2 * EG * p.max_part * U <= kTargetUnits && 2 * EG * in_units * U * ub <= kLdsBudget &&
               ((count + 2 * EG - 1) / (2 * EG)) * per_elem >= kFillBlocks)
            EG *= 2;
    a.EG = (u32)EG;
    a.count = count;
    a.per_elem = per_elem;
    a.dKC = csgn_fastdiv_make(a.KC);
    a.dT = csgn_fastdiv_make(a.t);
    a.in_el = (u32)(in_units * KC);
    a.sbase = staged ? (u32)((EG * in_units * KC * ub + 15u) & ~15ull) : 0u;
    a.mbase = (a.sbase + p.sub_bytes + 15u) & ~15u;
    const u32 lds = a.mbase + (staged ? 0u : kMetaBytes);
    const bool digits = t > 1;
    a.xcd = stream_xcd(count * units);
    // the launches: the workgroups of the call in order, launch_blocks() at a time
    const u64 total = ((count + EG - 1) / EG) * per_elem, max_blocks = launch_blocks();
    for (u64 b0 = 0; b0 < total; b0 += max_blocks) {
        a.block0 = b0;
        a.nblocks = (u32)std::min(max_blocks, total - b0);
        const dim3 grid(a.nblocks);
        if (staged && digits)
            k_wsum<Unit, true, true><<<grid, 256, lds, st>>>(a);
        else if (staged)
            k_wsum<Unit, true, false><<<grid, 256, lds, st>>>(a);
        else if (digits)
            k_wsum<Unit, false, true><<<grid, 256, lds, st>>>(a);
        else
            k_wsum<Unit, false, false><<<grid, 256, lds, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 wsum_terms(u64 n_classes, const u64 *n, u64 t, u64 j)
{
    u64 T;
    return wsum_count(n_classes, n, t, j, T) == WSUM_OK ? T : 0;
}

int wsum_plan_check(u64 n_classes, const u64 *n, u64 t, u64 n_out, const u64 *js, u64 *T)
{
    if (!wsum_shape_ok(n_classes, n, t) || n_out < 1 || n_out > kWsumMaxPlanes || !js)
        return CSGN_ERR_INVALID;
    for (u64 x = 0; x < n_out; ++x)
        if (js[x] > kWsumMaxPlane || (x && js[x] <= js[x - 1]))
            return CSGN_ERR_INVALID;
    int rc = CSGN_OK;
    for (u64 x = 0; x < n_out; ++x) {
        const WsumCount k = wsum_count(n_classes, n, t, js[x], T[x]);
        if (k == WSUM_EMPTY)
            return CSGN_ERR_INVALID;                            // an empty plane is refused before any size
        if (k == WSUM_SATURATED || T[x] >= (1ull << 31))
            rc = CSGN_ERR_UNSUPPORTED;
    }
    return rc;
}

int wsum_plan_create(u64 n_classes, const u64 *n, u64 t, u64 n_out, const u64 *js, WsumPlan &p, hipError_t &herr)
{
    herr = hipSuccess;
    p.C = (u32)n_classes;
    p.t = t;
    p.n_out = (u32)n_out;
    for (u32 c = 0; c < p.C; ++c)
        p.n[c] = (u32)n[c];
    p.vt.clear();
    p.max_part = 0;
    p.sub_bytes = 0;
    u64 vectors = 0;
    for (u32 x = 0; x < p.n_out; ++x) {
        p.js[x] = (u32)js[x];
        p.ncls[x] = (u32)std::min<u64>(js[x] + 1, n_classes);
        p.vbase[x] = (u32)p.vt.size();
        VectorWalk w = {p, p.ncls[x], {}, {}, p.vt};
        w.forced = tune(TUNE_WSUM_CPART);
        w.vectors = vectors;
        for (u32 c = 0; c < p.ncls[x]; ++c)
            w.below[c + 1] = w.below[c] + ((unsigned __int128)p.n[c] << c);
        // the classes above the last never take part: the top class's walk starts from all of 2^j
        w.walk(p.ncls[x] - 1, 1ull << js[x]);
        if (w.status != CSGN_OK)
            return w.status;
        if (p.vt.size() >= (1ull << 31))
            return CSGN_ERR_UNSUPPORTED;
        vectors = w.vectors;
        p.nvec[x] = (u32)((p.vt.size() - p.vbase[x]) / (kRec + 2 * p.ncls[x]));
        p.parts[x] = (u32)w.parts;
        p.T[x] = w.first;
        p.max_part = std::max(p.max_part, w.max_part);
        p.sub_bytes = std::max(p.sub_bytes, w.sub_bytes);
    }
    herr = hipMalloc((void **)&p.d_vt, p.vt.size() * sizeof(u32));
    if (herr == hipSuccess)
        herr = hipMemcpy(p.d_vt, p.vt.data(), p.vt.size() * sizeof(u32), hipMemcpyHostToDevice);
    if (herr != hipSuccess) {
        wsum_plan_free(p);
        return CSGN_ERR_HIP;
    }
    return CSGN_OK;
}

void wsum_plan_free(WsumPlan &p)
{
    if (p.d_vt)
        (void)hipFree(p.d_vt);
    p.d_vt = nullptr;
}

hipError_t wsum(const WsumPlan &p, u64 n_bits, u64 count, const u64 *const *in, u64 *const *out, hipStream_t stream)
{
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = wide_units(dL, ptr_array(in, p.C), ptr_array(out, p.n_out));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? wsum_fused<unit16>(p, count, in, out, U, stream) : wsum_fused<unit8>(p, count, in, out, U, stream);
}

} // namespace csgn
