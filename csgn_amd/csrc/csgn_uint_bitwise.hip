// csgn_uint_bitwise.hip -- the plane-by-plane operators of the bit-sliced encrypted integers (a & b, a | b, a ^ b, ~a,
// select(s, a, b) and the mask s * a), every plane in one launch.  Hand-written CDNA4 (gfx950) HIP; shared helpers in
// csgn_device.h, design notes in DESIGN.md §4.31.
//
// The definition (include/csgn_hip.h, csgn_uint_bitwise): output plane j is a composition of the reference's operator+
// (concatenation) and operator* (all-pairs AND, the left operand's term the slow index) over plane j of a and b and the
// one selector batch, in the order of the Gates table:
//     AND     [a_j x b_j]
//     OR      [a_j][b_j][a_j x b_j]
//     XOR     [a_j][b_j]
//     NOT     [a_j][ONE]
//     SELECT  [s x (a_j || b_j)][b_j]
//     KEEP    [s x a_j]
// so an element of an output plane is, as in csgn_gates.hip, a sequence of copy, product and constant segments; what
// differs from plane to plane is the term counts alone.
//
// One lane writes one unit.  A workgroup belongs to one plane (each plane's lane range is rounded up to whole
// workgroups, csgn_uint_addk.hip's placement), so the plane, its pointers, its counts and its divisors are scalar; the
// operation is uniform over the launch.  A lane issues its two loads unconditionally from selected bases (a copy
// reads its unit twice: the second load hits the same line) and ANDs them.  No LDS, no scratch.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kMaxPlanes = kBitwiseMaxPlanes;

// By value in the kernel arguments (3.9 KB of the 4 KB limit, so all 64 planes go in ONE launch; uniform indices,
// scalar loads).  Per plane p:
//     a[p], b[p]  the operand planes' first element of this launch (b: null where the operation does not read it)
//     out[p]      the output plane's first element of this launch
//     ta[p], tb[p] terms per element
//     first[p]    its first workgroup;  PU.d[p] its units per element;  row.d[p] the units of one product row
struct BitwiseArgs {
    const void *a[kMaxPlanes];
    const void *b[kMaxPlanes];
    void *out[kMaxPlanes];
    u32 ta[kMaxPlanes], tb[kMaxPlanes];
    u32 first[kMaxPlanes + 1];
    FastDivTable<kMaxPlanes> PU;
    FastDivTable<kMaxPlanes> row;
    const void *sel;
    u64 last_mask;
    u32 ts, op, np;
    u32 U, ne;                // units per term, elements of this launch
    u32 xcd;
    FastDiv dU;
};
static_assert(sizeof(BitwiseArgs) <= 4096, "kernel arguments past the 4 KB limit");

template <typename Unit>
__global__ void __launch_bounds__(256) k_uint_bitwise(BitwiseArgs g)
{
    const u32 bid = g.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    u32 p = 0, hi = g.np;                                 // the plane of this workgroup: first[p] <= bid < first[p + 1]
    while (hi - p > 1u) {
        const u32 mid = (p + hi) >> 1;
        if (g.first[mid] <= bid)
            p = mid;
        else
            hi = mid;
    }
    const FastDiv dpu = g.PU.at(p);
    const u32 off = (bid - g.first[p]) * 256u + threadIdx.x;   // unit inside the plane's part of this launch
    if (off >= g.ne * dpu.d)
        return;
    const u32 e = csgn_fastdiv(off, dpu), r = off - e * dpu.d;
    // the plane's segments in units (scalar): [a) ends at c0, [b) at c1, the product at pend, then SELECT's [b) or ONE
    const u32 U = g.U, op = g.op, ts = g.ts, ta = g.ta[p], tb = g.tb[p];
    const bool by_sel = op == CSGN_UINT_BITWISE_SELECT || op == CSGN_UINT_BITWISE_KEEP;
    const bool two = op == CSGN_UINT_BITWISE_OR || op == CSGN_UINT_BITWISE_XOR;
    const u32 c0 = two || op == CSGN_UINT_BITWISE_NOT ? ta * U : 0u;
    const u32 c1 = c0 + (two ? tb * U : 0u);
    const FastDiv drow = g.row.at(p);
    const u32 rows = op == CSGN_UINT_BITWISE_XOR || op == CSGN_UINT_BITWISE_NOT ? 0u : by_sel ? ts : ta;
    const u32 pend = c1 + rows * drow.d;
    const Unit *A = reinterpret_cast<const Unit *>(g.a[p]), *B = reinterpret_cast<const Unit *>(g.b[p]);
    const u64 eu = (u64)e * U, ea = eu * ta, eb = eu * tb;
    // product coordinates (harmless elsewhere: only selected below)
    const u32 rr = r - c1, i = csgn_fastdiv(rr, drow), c = rr - i * drow.d;
    const u32 k = c - csgn_fastdiv(c, g.dU) * U;
    const Unit *pa = A, *pb;
    u64 ia = ea + r, ib;                                  // r < c0: a copy of a_j
    bool one = false;
    if (r < c1) {
        if (r >= c0) {                                    // a copy of b_j
            pa = B;
            ia = eb + (r - c0);
        }
        pb = pa;
        ib = ia;
    } else if (r < pend) {                                // row i of the left operand against unit c of the row
        pa = by_sel ? reinterpret_cast<const Unit *>(g.sel) : A;
        ia = (by_sel ? eu * ts : ea) + (u64)i * U + k;
        const bool right_a = op == CSGN_UINT_BITWISE_KEEP || (op == CSGN_UINT_BITWISE_SELECT && c < ta * U);
        pb = right_a ? A : B;
        ib = right_a ? ea + c : eb + (op == CSGN_UINT_BITWISE_SELECT ? c - ta * U : c);
    } else {                                              // SELECT's closing b_j, NOT's ONE (its loads: the element's first unit)
        one = op != CSGN_UINT_BITWISE_SELECT;
        pa = one ? A : B;
        ia = one ? ea : eb + (r - pend);
        pb = pa;
        ib = ia;
    }
    const Unit va = pa[ia], vb = pb[ib];
    const Unit v = one ? one_unit(Unit(), r - pend, U, g.last_mask) : va & vb;
    unit_store<Unit, true>(reinterpret_cast<Unit *>(g.out[p]) + (u64)off, v);
}

// ------------------------------------------------------------------------------ the definition on the host

bool reads_b(int op)
{
    return op == CSGN_UINT_BITWISE_AND || op == CSGN_UINT_BITWISE_OR || op == CSGN_UINT_BITWISE_XOR ||
           op == CSGN_UINT_BITWISE_SELECT;
}
bool reads_sel(int op) { return op == CSGN_UINT_BITWISE_SELECT || op == CSGN_UINT_BITWISE_KEEP; }
bool known(int op) { return op >= CSGN_UINT_BITWISE_AND && op <= CSGN_UINT_BITWISE_KEEP; }

struct BitwiseShape {
    u32 w = 0;
    u64 ts = 0;
    u64 ta[kMaxPlanes] = {}, tb[kMaxPlanes] = {}, T[kMaxPlanes] = {};
};

// false: an invalid argument or a term count of 2^62 or more
bool bitwise_shape(int op, u64 w, u64 ts, const u64 *ta, const u64 *tb, BitwiseShape &sh)
{
    sh = BitwiseShape();
    if (!known(op) || w < 1 || w > kMaxPlanes || !ta || (reads_b(op) && !tb))
        return false;
    sh.w = (u32)w;
    sh.ts = reads_sel(op) ? ts : 0;
    for (u64 j = 0; j < w; ++j) {
        sh.ta[j] = ta[j];
        sh.tb[j] = reads_b(op) ? tb[j] : 0;
        sh.T[j] = uint_bitwise_terms(op, sh.ts, sh.ta[j], sh.tb[j]);
        if (sh.T[j] == 0)
            return false;
    }
    return true;
}

// The form by shape, by the measurements of DESIGN §4.31 (widths 8, 32 and 64, outputs of 1 MB to 4 GB).  Two measured
// classes go to the kernel: outputs of at most 128 MiB at 8 planes or more, where the planes form is bound by its
// launches (3 to 50 times faster, growing with the width), and outputs up to 1 GiB at 32 planes or more when no
// selector of several terms is read (level to 1.9 times faster).  Everything else keeps the tuned launchers plane by
// plane: at 8 planes of 128 MB each they are level or ahead, and a product with a selector of thousands of terms is
// the tuned multiply's job once it is large (the kernel takes up to 1.3 times its time there); so does every shape
// that was not measured, narrower integers among them.
bool bitwise_shape_rule(const BitwiseShape &sh, u64 n_bits, u64 batch)
{
    if (sh.w < 8)
        return false;
    const u64 dL = (n_bits + 63) / 64;
    double words = 0;
    for (u32 p = 0; p < sh.w; ++p)
        words += (double)sh.T[p] * (double)dL;
    const double bytes = words * (double)batch * 8.0;
    return bytes <= 134217728.0 || (sh.w >= 32 && sh.ts <= 1 && bytes <= 1073741824.0);
}

bool bitwise_use_kernel(const BitwiseShape &sh, u64 n_bits, u64 batch)
{
    // one element of every plane (at 8-byte units, the larger count) must fit one launch's lanes
    const u64 dL = (n_bits + 63) / 64;
    double lanes = 256.0 * sh.w;
    for (u32 p = 0; p < sh.w; ++p)
        lanes += (double)sh.T[p] * (double)dL;
    if (lanes > (double)0xFFFFFF00ull)
        return false;                                     // whatever the knob says: the kernel cannot index it
    const int form = tune(TUNE_UINT_BITWISE_FORM);
    if (form == 0 || form == 1)
        return form == 1;
    // a forced gate form keeps the tuned launchers, so that csgn_gate_uniform's two forms still run through the
    // integer operators
    const int gates = tune(TUNE_GATE_FUSED);
    if (gates == 0 || gates == 1)
        return false;
    return bitwise_shape_rule(sh, n_bits, batch);
}

template <typename Unit>
hipError_t bitwise_kernel(const BitwiseShape &sh, int op, u64 n_bits, u64 batch, const u64 *sel, const u64 *const *a,
                          const u64 *const *b, u64 *const *out, u32 U, hipStream_t s)
{
    BitwiseArgs g = {};
    g.U = U;
    g.dU = csgn_fastdiv_make(U);
    g.last_mask = last_word_mask(n_bits);
    g.op = (u32)op;
    g.np = sh.w;
    g.ts = (u32)sh.ts;
    u64 units[kMaxPlanes], sum_units = 0;                 // per element
    for (u32 p = 0; p < kMaxPlanes; ++p) {
        units[p] = 1;
        u64 row = 1;
        if (p < sh.w) {
            units[p] = sh.T[p] * U;
            sum_units += units[p];
            g.ta[p] = (u32)sh.ta[p];
            g.tb[p] = (u32)sh.tb[p];
            if (op == CSGN_UINT_BITWISE_AND || op == CSGN_UINT_BITWISE_OR)
                row = sh.tb[p] * U;
            else if (op == CSGN_UINT_BITWISE_SELECT)
                row = (sh.ta[p] + sh.tb[p]) * U;
            else if (op == CSGN_UINT_BITWISE_KEEP)
                row = sh.ta[p] * U;
        }
        g.PU.set(p, (u32)units[p]);
        g.row.set(p, (u32)row);
    }
    // elements per launch: every plane's lane range, rounded up to whole workgroups, below 2^32 lanes in all and
    // within launch_blocks() workgroups (one element at least)
    const u64 room = 0xFFFFFF00ull - 256ull * g.np;
    if (sum_units > room)
        return hipErrorInvalidValue;                      // bitwise_use_kernel keeps such shapes away
    const u64 max_blocks = launch_blocks();
    const u64 lanes = max_blocks > g.np ? std::min(room, (max_blocks - g.np) * 256ull) : 0;
    const u64 per = std::max<u64>(1, lanes / sum_units);
    for (u64 e0 = 0; e0 < batch; e0 += per) {
        const u64 ne = std::min(per, batch - e0);
        u32 blocks = 0;
        for (u32 p = 0; p < g.np; ++p) {
            g.first[p] = blocks;
            blocks += ceil_div_u64(ne * units[p], 256u);
            g.a[p] = reinterpret_cast<const Unit *>(a[p]) + e0 * sh.ta[p] * U;
            g.b[p] = reads_b(op) ? reinterpret_cast<const Unit *>(b[p]) + e0 * sh.tb[p] * U : nullptr;
            g.out[p] = reinterpret_cast<Unit *>(out[p]) + e0 * units[p];
        }
        g.first[g.np] = blocks;
        g.sel = reads_sel(op) ? reinterpret_cast<const Unit *>(sel) + e0 * sh.ts * U : nullptr;
        g.ne = (u32)ne;
        g.xcd = stream_xcd(ne * sum_units);
        k_uint_bitwise<Unit><<<dim3(blocks), 256, 0, s>>>(g);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// The planes form: what the class operators issued plane by plane before this call existed, each launcher writing
// straight into its output plane.
hipError_t bitwise_planes(const BitwiseShape &sh, int op, u64 n_bits, u64 batch, const u64 *sel, const u64 *const *a,
                          const u64 *const *b, u64 *const *out, hipStream_t s)
{
    for (u32 j = 0; j < sh.w; ++j) {
        const u64 ta = sh.ta[j], tb = sh.tb[j];
        hipError_t e = hipSuccess;
        switch (op) {
        case CSGN_UINT_BITWISE_AND: e = mul_uniform(n_bits, batch, ta, tb, a[j], b[j], out[j], 0, s); break;
        case CSGN_UINT_BITWISE_OR:
            e = gate_uniform(n_bits, CSGN_GATE_OR, batch, 0, ta, tb, nullptr, a[j], b[j], nullptr, out[j], s);
            break;
        case CSGN_UINT_BITWISE_XOR: e = add_uniform(n_bits, batch, ta, tb, a[j], b[j], out[j], s); break;
        case CSGN_UINT_BITWISE_NOT:
            e = gate_uniform(n_bits, CSGN_GATE_NOT, batch, 0, ta, 0, nullptr, a[j], nullptr, nullptr, out[j], s);
            break;
        case CSGN_UINT_BITWISE_SELECT:
            e = gate_uniform(n_bits, CSGN_GATE_MUX, batch, sh.ts, ta, tb, sel, a[j], b[j], nullptr, out[j], s);
            break;
        default: e = mul_uniform(n_bits, batch, sh.ts, ta, sel, a[j], out[j], 0, s); break;
        }
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_bitwise_terms(int op, u64 ts, u64 ta, u64 tb)
{
    if (!known(op) || ta == 0 || ta >= kTermLimit)
        return 0;
    if (reads_b(op) && (tb == 0 || tb >= kTermLimit))
        return 0;
    if (reads_sel(op) && (ts == 0 || ts >= kTermLimit))
        return 0;
    u64 p = 0, total = 0;
    switch (op) {
    case CSGN_UINT_BITWISE_AND: return term_mul(ta, tb, p) ? p : 0;
    case CSGN_UINT_BITWISE_OR: total = term_mul(ta, tb, p) ? ta + tb + p : kTermLimit; break;
    case CSGN_UINT_BITWISE_XOR: total = ta + tb; break;
    case CSGN_UINT_BITWISE_NOT: total = ta + 1; break;
    case CSGN_UINT_BITWISE_SELECT: total = term_mul(ts, ta + tb, p) ? p + tb : kTermLimit; break;
    default: return term_mul(ts, ta, p) ? p : 0;
    }
    return total < kTermLimit ? total : 0;
}

const char *uint_bitwise_kernel_name(u64 n_bits, int op, u64 batch, u64 width, u64 ts, const u64 *ta, const u64 *tb)
{
    BitwiseShape sh;
    if (n_bits == 0 || !bitwise_shape(op, width, ts, ta, tb, sh))
        return "";
    return bitwise_use_kernel(sh, n_bits, batch) ? "k_uint_bitwise" : "planes";
}

hipError_t uint_bitwise(u64 n_bits, int op, u64 batch, u64 width, const u64 *sel, u64 ts, const u64 *const *a,
                        const u64 *ta, const u64 *const *b, const u64 *tb, u64 *const *out, hipStream_t s)
{
    BitwiseShape sh;
    if (!bitwise_shape(op, width, ts, ta, tb, sh))
        return hipErrorInvalidValue;
    if (batch == 0)
        return hipSuccess;
    if (!reads_sel(op))
        sel = nullptr;
    if (!bitwise_use_kernel(sh, n_bits, batch))
        return bitwise_planes(sh, op, n_bits, batch, sel, a, b, out, s);
    const u64 dL = (n_bits + 63) / 64;
    const bool wide = reads_b(op) ? wide_units(dL, sel, ptr_array(a, sh.w), ptr_array(b, sh.w), ptr_array(out, sh.w))
                                  : wide_units(dL, sel, ptr_array(a, sh.w), ptr_array(out, sh.w));
    const u32 U = (u32)(wide ? dL / 2 : dL);
    return wide ? bitwise_kernel<unit16>(sh, op, n_bits, batch, sel, a, b, out, U, s)
                : bitwise_kernel<unit8>(sh, op, n_bits, batch, sel, a, b, out, U, s);
}

} // namespace csgn
