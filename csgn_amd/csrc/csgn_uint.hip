// csgn_uint.hip -- the per-bit steps of bit-sliced encrypted unsigned integers (add, subtract, compare) over uniform
// batches.  Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md ("Integers").
//
// Every step is a composition of the reference's operator+ (concatenation) and operator* (all-pairs AND, left term
// slowest) with the all-ones term ONE (csgn_device.h), in the order of the table in include/csgn_hip.h.  One output
// element is a sequence of SEGMENTS:
//     copy of one operand | all-pairs product of one operand (or ONE) with a VIRTUAL concatenation of up to three
//     operands / ONE
// A product whose left side is a concatenation is the product of each of its parts in turn (left term slowest), so a
// virtual left operand is a run of product segments; a virtual right operand ([a | b], [b | l], [a | b | ONE]) is read
// in place by every row.  The fused kernel writes every segment of BOTH outputs of one element in one launch, reading
// each operand from HBM once; ONE is made in registers.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

constexpr u32 kMaxSeg = 6;            // ADD_FULL: three copies, three products
enum { USEG_COPY = 0, USEG_PROD = 1 };
enum { OP_X = 0, OP_A = 1, OP_B = 2, OP_ONE = 3 };

// The segments of one element of both outputs (the carry's last), the table of include/csgn_hip.h.  Packed:
//     bit 0 kind | bit 1 output | bits 2-3 left operand (the copied one for a copy) | bits 4-5 parts of the right
//     operand | bits 6-7, 8-9, 10-11 its parts
// The kernel is instantiated per step, so this table is constant there: only the sizes are launch arguments.
__host__ __device__ constexpr u32 useg_copy(u32 out, u32 x) { return USEG_COPY | out << 1 | x << 2; }
__host__ __device__ constexpr u32 useg_prod(u32 out, u32 l, u32 np, u32 p0, u32 p1 = 0, u32 p2 = 0)
{
    return USEG_PROD | out << 1 | l << 2 | np << 4 | p0 << 6 | p1 << 8 | p2 << 10;
}
__host__ __device__ constexpr u32 step_segments(int step)
{
    return step == CSGN_UINT_ADD_HALF ? 3u : step == CSGN_UINT_ADD_FULL ? 6u : step == CSGN_UINT_EQ_STEP ? 1u
         : step == CSGN_UINT_LT_FIRST ? 2u : step == CSGN_UINT_LT_STEP ? 3u : 0u;
}
__host__ __device__ constexpr u32 step_segment(int step, u32 s)
{
    switch (step) {
    case CSGN_UINT_ADD_HALF:                                   // [a][b] | [a x b]
        return s == 0 ? useg_copy(0, OP_A) : s == 1 ? useg_copy(0, OP_B) : useg_prod(1, OP_A, 1, OP_B);
    case CSGN_UINT_ADD_FULL:                                   // [a][b][c] | (a * b) + ((a + b) * c)
        return s == 0 ? useg_copy(0, OP_A) : s == 1 ? useg_copy(0, OP_B) : s == 2 ? useg_copy(0, OP_X)
             : s == 3 ? useg_prod(1, OP_A, 1, OP_B) : s == 4 ? useg_prod(1, OP_A, 1, OP_X) : useg_prod(1, OP_B, 1, OP_X);
    case CSGN_UINT_EQ_STEP: return useg_prod(0, OP_X, 3, OP_A, OP_B, OP_ONE);              // e * ((a + b) + ONE)
    case CSGN_UINT_LT_FIRST: return s == 0 ? useg_prod(0, OP_A, 1, OP_B) : useg_prod(0, OP_ONE, 1, OP_B);   // (a + ONE) * b
    default:                                                   // ((a + b) * (b + l)) + l
        return s == 0 ? useg_prod(0, OP_A, 2, OP_B, OP_X) : s == 1 ? useg_prod(0, OP_B, 2, OP_B, OP_X) : useg_copy(0, OP_X);
    }
}

// Segment s (step_segment) of an element covers its units [begin[s], end[s]) of the two outputs laid end to end
// (out0's segments first; r >= EU0 is out1); a product's right operand has its part ends pend0 / pend1 (units into a
// row) and its row length (row_*).
struct UintArgs {
    const void *op[3];        // x, a, b (an operand the step does not read may be null: never selected)
    void *out[2];             // out1 null: EU1 = 0, no lane writes it
    u32 t[4];                 // terms per element of x, a, b; t[3] = 1 (ONE)
    u32 begin[kMaxSeg], end[kMaxSeg - 1];
    u32 pend0[kMaxSeg], pend1[kMaxSeg];
    FastDivTable<kMaxSeg> row;                                    // FastDiv of each product's row (units)
    u32 U, EU0, EU1, EU;      // units per term, per element of out0 / out1 / both
    u32 total_units;          // this launch
    u32 xcd;
    FastDiv dEU, dU;
    u64 last_mask;
};

// arr[s] for s < N by a select chain (kernel arguments stay in SGPRs; a dynamic index would copy them to scratch)
template <u32 N>
__device__ inline u32 pick(const u32 (&arr)[kMaxSeg], u32 s)
{
    return s == 0u || N < 2 ? arr[0] : s == 1u || N < 3 ? arr[1] : s == 2u || N < 4 ? arr[2]
         : s == 3u || N < 5 ? arr[3] : s == 4u || N < 6 ? arr[4] : arr[5];
}

// step_segment(STEP, s) for s < N, folded to constants
template <int STEP, u32 N>
__device__ inline u32 segment_of(u32 s)
{
    u32 v = step_segment(STEP, 0);
    v = N > 1 && s == 1u ? step_segment(STEP, 1) : v;
    v = N > 2 && s == 2u ? step_segment(STEP, 2) : v;
    v = N > 3 && s == 3u ? step_segment(STEP, 3) : v;
    v = N > 4 && s == 4u ? step_segment(STEP, 4) : v;
    v = N > 5 && s == 5u ? step_segment(STEP, 5) : v;
    return v;
}

template <typename Unit>
__device__ inline const Unit *uint_op(const UintArgs &a, u32 o)
{
    // ONE is never loaded from: its lane reads a's unit instead (a exists in every step) and discards it
    const void *p = o == OP_X ? a.op[0] : (o == OP_B ? a.op[2] : a.op[1]);
    return reinterpret_cast<const Unit *>(p);
}

// Modelled on k_gate_fused (csgn_gates.hip): one 16-byte (8-byte when dL is odd) output unit per lane, element,
// segment and row by FastDiv, both loads issued unconditionally from selected bases, ONE selected in after the load.
template <typename Unit, int STEP>
__global__ void __launch_bounds__(256) k_uint_step(UintArgs a)
{
    constexpr u32 N = step_segments(STEP);
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const u32 g = bid * 256u + threadIdx.x;
    if (g >= a.total_units)
        return;
    const u32 e = csgn_fastdiv(g, a.dEU), r = g - e * a.EU;
    // the lane's segment (an end past the last segment written -- no carry -- is EU: never reached)
    const u32 s = (N > 1 && r >= a.end[0] ? 1u : 0u) + (N > 2 && r >= a.end[1] ? 1u : 0u) +
                  (N > 3 && r >= a.end[2] ? 1u : 0u) + (N > 4 && r >= a.end[3] ? 1u : 0u) +
                  (N > 5 && r >= a.end[4] ? 1u : 0u);
    const u32 desc = segment_of<STEP, N>(s), rr = r - pick<N>(a.begin, s), U = a.U;
    const bool prod = (desc & 1u) == USEG_PROD;
    const u32 left = (desc >> 2) & 3u;
    const u32 tl = left == OP_X ? a.t[0] : (left == OP_A ? a.t[1] : (left == OP_B ? a.t[2] : 1u));
    // product coordinates (harmless for a copy: only selected below)
    const FastDiv dRow = {pick<N>(a.row.d, s), pick<N>(a.row.magic, s), pick<N>(a.row.shift, s)};
    const u32 i = csgn_fastdiv(rr, dRow), c = rr - i * dRow.d;
    const u32 k = c - csgn_fastdiv(c, a.dU) * U;
    const u32 pe0 = pick<N>(a.pend0, s), pe1 = pick<N>(a.pend1, s);
    const u32 p = (c >= pe0 ? 1u : 0u) + (c >= pe1 ? 1u : 0u);
    const u32 part = (desc >> (6u + 2u * p)) & 3u;
    const u32 pstart = p == 0u ? 0u : (p == 1u ? pe0 : pe1);
    const u32 tp = part == OP_X ? a.t[0] : (part == OP_A ? a.t[1] : (part == OP_B ? a.t[2] : 1u));
    // A: the left operand's term i (a copy: its unit rr); B: the right part's unit (a copy: A again, same line).  32-bit
    // indices: every operand has no more units per element than the outputs together, so none reaches total_units.
    const u32 ea = e * a.t[1] * U + k;           // where a ONE side reads (and discards)
    const Unit *pa = uint_op<Unit>(a, left);
    const u32 ia = left == OP_ONE ? ea : e * tl * U + (prod ? i * U + k : rr);
    const Unit *pb = prod ? uint_op<Unit>(a, part) : pa;
    const u32 ib = !prod ? ia : (part == OP_ONE ? ea : e * tp * U + (c - pstart));
    Unit va = pa[ia], vb = pb[ib];
    const Unit one = one_unit(Unit(), k, U, a.last_mask);
    va = left == OP_ONE ? one : va;
    vb = prod && part == OP_ONE ? one : vb;
    const bool second = r >= a.EU0;
    Unit *o = reinterpret_cast<Unit *>(second ? a.out[1] : a.out[0]) + (second ? e * a.EU1 + (r - a.EU0) : e * a.EU0 + r);
    unit_store<Unit, true>(o, va & vb);
}

struct USeg {
    u32 kind, out, left, np, part[3];
    u64 terms;                // terms per element
};
struct UintShape {
    u32 nseg;
    USeg seg[kMaxSeg];
    u64 terms[2];             // per output element
};

// the segments of one element of both outputs, decoded from step_segment (with_carry: out1 of the ADD steps)
bool uint_shape(int step, bool with_carry, u64 tx, u64 ta, u64 tb, UintShape &sh)
{
    sh = UintShape();
    const u64 t[4] = {tx, ta, tb, 1};
    for (u32 i = 0; i < step_segments(step); ++i) {
        const u32 d = step_segment(step, i);
        USeg g = {d & 1u, (d >> 1) & 1u, (d >> 2) & 3u, (d >> 4) & 3u, {(d >> 6) & 3u, (d >> 8) & 3u, (d >> 10) & 3u}, 0};
        if (g.out == 1 && !with_carry)
            break;                                             // the carry's segments come last
        const u64 right = t[g.part[0]] + (g.np > 1 ? t[g.part[1]] : 0) + (g.np > 2 ? t[g.part[2]] : 0);
        g.terms = g.kind == USEG_PROD ? t[g.left] * right : t[g.left];
        sh.seg[sh.nseg++] = g;
        sh.terms[g.out] += g.terms;
    }
    return sh.nseg != 0;
}

bool step_reads_x(int step) { return step != CSGN_UINT_ADD_HALF && step != CSGN_UINT_LT_FIRST; }

// Fused form: product segments up to this many terms per element (both outputs together).  Past it the pitched form
// (the tuned multiply / add launchers writing into the outputs' slices) takes over.  Measured on MI355X at N=1247
// (DESIGN.md "Integers", tools/bench_uint.py --sweep), fused / pitched microseconds at equal bytes:
//     ADD_FULL  t_x  7, 15, 31 (15..63 product terms):   820 / 912, 755 / 871, 716 / 838; level at 63 and 127
//     LT_STEP   t_x  8 .. 80 (18..162 product terms):     689 / 851 .. 641 / 724
constexpr u64 kUintFusedMaxProductTerms = 64;
constexpr u64 kLtFusedMaxProductTerms = 162;

// the form a call takes: true = fused (the decision ignores whether the carry is wanted)
bool uint_use_fused(int step, u64 tx, u64 ta, u64 tb)
{
    UintShape sh;
    uint_shape(step, true, tx, ta, tb, sh);
    // a virtual right operand under a left operand of more than one term: rows interleave the right's parts, no
    // slice of the output is one launcher's product
    u64 prod_terms = 0;
    for (u32 i = 0; i < sh.nseg; ++i)
        if (sh.seg[i].kind == USEG_PROD) {
            const u64 tl = sh.seg[i].left == OP_X ? tx : (sh.seg[i].left == OP_A ? ta : (sh.seg[i].left == OP_B ? tb : 1));
            if (sh.seg[i].np > 1 && tl > 1)
                return true;
            prod_terms += sh.seg[i].terms;
        }
    return tune_choose(TUNE_UINT_FUSED,
                       prod_terms <= (step == CSGN_UINT_LT_STEP ? kLtFusedMaxProductTerms : kUintFusedMaxProductTerms));
}

template <typename Unit>
hipError_t uint_fused(int step, const UintShape &sh, u64 n_bits, u64 batch, const u64 *t, const u64 *const *ops, u64 *const *outs,
                      u32 U, hipStream_t s)
{
    UintArgs a = {};
    a.U = U;
    a.last_mask = last_word_mask(n_bits);
    for (int o = 0; o < 3; ++o)
        a.t[o] = (u32)t[o];
    a.t[3] = 1;
    u64 run = 0;
    for (u32 i = 0; i < kMaxSeg; ++i) {
        u32 row_div = 1;
        if (i < sh.nseg) {
            const USeg &g = sh.seg[i];
            a.begin[i] = (u32)run;
            run += g.terms * U;
            if (g.kind == USEG_PROD) {
                const u64 e0 = a.t[g.part[0]] * (u64)U, e1 = e0 + (g.np > 1 ? a.t[g.part[1]] * (u64)U : 0);
                const u64 row = e1 + (g.np > 2 ? a.t[g.part[2]] * (u64)U : 0);
                a.pend0[i] = (u32)(g.np > 1 ? e0 : row);
                a.pend1[i] = (u32)(g.np > 2 ? e1 : row);
                row_div = (u32)row;
            }
        }
        a.row.set(i, row_div);
        if (i + 1 < kMaxSeg)
            a.end[i] = (u32)run;                               // completed below for the segments past nseg
    }
    a.EU = (u32)run;
    for (u32 i = sh.nseg ? sh.nseg - 1 : 0; i + 1 < kMaxSeg; ++i)
        a.end[i] = a.EU;
    a.EU0 = (u32)(sh.terms[0] * U);
    a.EU1 = (u32)(sh.terms[1] * U);
    a.dU = csgn_fastdiv_make(U);
    a.dEU = csgn_fastdiv_make(a.EU);
    a.xcd = stream_xcd(batch * run);
    const u64 per = std::max<u64>(1, 0xFFFFFF00ull / run);           // elements per launch: < 2^32 units
    for (u64 e0 = 0; e0 < batch; e0 += per) {
        const u64 ne = std::min(per, batch - e0);
        for (int o = 0; o < 3; ++o)
            a.op[o] = ops[o] ? reinterpret_cast<const Unit *>(ops[o]) + e0 * t[o] * U : nullptr;
        a.out[0] = reinterpret_cast<Unit *>(outs[0]) + e0 * a.EU0;
        a.out[1] = outs[1] ? reinterpret_cast<Unit *>(outs[1]) + e0 * a.EU1 : nullptr;
        a.total_units = (u32)(ne * run);
        const dim3 grid(ceil_div_u64(a.total_units, 256u));
        switch (step) {
        case CSGN_UINT_ADD_HALF: k_uint_step<Unit, CSGN_UINT_ADD_HALF><<<grid, 256, 0, s>>>(a); break;
        case CSGN_UINT_ADD_FULL: k_uint_step<Unit, CSGN_UINT_ADD_FULL><<<grid, 256, 0, s>>>(a); break;
        case CSGN_UINT_EQ_STEP: k_uint_step<Unit, CSGN_UINT_EQ_STEP><<<grid, 256, 0, s>>>(a); break;
        case CSGN_UINT_LT_FIRST: k_uint_step<Unit, CSGN_UINT_LT_FIRST><<<grid, 256, 0, s>>>(a); break;
        default: k_uint_step<Unit, CSGN_UINT_LT_STEP><<<grid, 256, 0, s>>>(a); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 uint_step_terms(int step, int output, u64 tx, u64 ta, u64 tb)
{
    const bool add = step == CSGN_UINT_ADD_HALF || step == CSGN_UINT_ADD_FULL;
    if (step < CSGN_UINT_ADD_HALF || step > CSGN_UINT_LT_STEP || output < 0 || output > (add ? 1 : 0))
        return 0;
    if (!step_reads_x(step))
        tx = 1;                                                          // not read: any count
    if (tx == 0 || ta == 0 || tb == 0)
        return 0;
    if (tx >= kTermLimit || ta >= kTermLimit || tb >= kTermLimit)
        return 0;
    UintShape sh;
    uint_shape(step, true, tx, ta, tb, sh);
    // every product (the segments' term counts) below kTermLimit, and their sum
    u64 total = 0;
    for (u32 i = 0; i < sh.nseg; ++i) {
        const USeg &g = sh.seg[i];
        if (g.out != (u32)output)
            continue;
        if (g.kind == USEG_PROD) {
            const u64 tl = g.left == OP_X ? tx : (g.left == OP_A ? ta : (g.left == OP_B ? tb : 1));
            const u64 tr[4] = {tx, ta, tb, 1};
            const u64 right = tr[g.part[0]] + (g.np > 1 ? tr[g.part[1]] : 0) + (g.np > 2 ? tr[g.part[2]] : 0);
            u64 p;
            if (!term_mul(tl, right, p))
                return 0;
            total += p;
        } else {
            total += g.terms;
        }
        if (total >= kTermLimit)
            return 0;
    }
    return total;
}

const char *uint_step_kernel_name(u64 n_bits, int step, u64 batch, u64 tx, u64 ta, u64 tb)
{
    (void)n_bits;
    (void)batch;
    if (uint_step_terms(step, 0, tx, ta, tb) == 0)
        return "";
    if (!step_reads_x(step))
        tx = 1;
    return uint_use_fused(step, tx, ta, tb) ? "k_uint_step" : "pitched";
}

hipError_t uint_step(u64 n_bits, int step, u64 batch, const u64 *X, u64 tx, const u64 *A, u64 ta, const u64 *B, u64 tb,
                     u64 *out0, u64 *out1, hipStream_t s)
{
    UintShape sh;
    if (batch == 0)
        return hipSuccess;
    if (!step_reads_x(step)) {
        tx = 1;
        X = nullptr;
    }
    if (step != CSGN_UINT_ADD_HALF && step != CSGN_UINT_ADD_FULL)
        out1 = nullptr;
    if (!uint_shape(step, out1 != nullptr, tx, ta, tb, sh))
        return hipErrorInvalidValue;
    const u64 dL = (n_bits + 63) / 64;
    const u64 t[4] = {tx, ta, tb, 1};
    const u64 *ops[3] = {X, A, B};
    u64 *const outs[2] = {out0, out1};
    if (uint_use_fused(step, tx, ta, tb)) {
        const bool wide = wide_units(dL, X, A, B, out0, out1);
        const u32 U = (u32)(wide ? dL / 2 : dL);
        return wide ? uint_fused<unit16>(step, sh, n_bits, batch, t, ops, outs, U, s)
                    : uint_fused<unit8>(step, sh, n_bits, batch, t, ops, outs, U, s);
    }
    // pitched: every segment (and every part of a product's right operand) by its own tuned launcher, straight into
    // the element's slice of its output.  Only reached when each product's left operand has one term or its right
    // operand one part, so every such piece is a contiguous slice.  ONE * y is the copy of y and y * ONE that of y:
    // a canonical term ANDed with ONE is itself.
    const u64 pitch[2] = {sh.terms[0] * dL, sh.terms[1] * dL};
    u64 at[2] = {0, 0};                                                  // words into the element
    for (u32 i = 0; i < sh.nseg; ++i) {
        const USeg &g = sh.seg[i];
        u64 *o = outs[g.out];
        hipError_t e = hipSuccess;
        if (g.kind == USEG_COPY) {
            e = add_uniform(n_bits, batch, t[g.left], 0, ops[g.left], nullptr, o + at[g.out], s, pitch[g.out]);
            at[g.out] += t[g.left] * dL;
        } else {
            for (u32 q = 0; q < g.np && e == hipSuccess; ++q) {
                const u32 y = g.part[q];
                if (g.left == OP_ONE || y == OP_ONE) {                   // never both: ONE always meets an operand
                    const u32 src = g.left == OP_ONE ? y : g.left;
                    e = add_uniform(n_bits, batch, t[src], 0, ops[src], nullptr, o + at[g.out], s, pitch[g.out]);
                } else
                    e = mul_uniform(n_bits, batch, t[g.left], t[y], ops[g.left], ops[y], o + at[g.out], 0, s,
                                    pitch[g.out]);
                at[g.out] += t[g.left] * t[y] * dL;
            }
        }
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace csgn
