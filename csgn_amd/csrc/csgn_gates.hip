// csgn_gates.hip -- plaintext constants and the boolean gates built on them (NOT, XNOR, NAND, OR, NOR, MUX,
// addPlain, mulPlain) over uniform batches.
// Hand-written CDNA4 (gfx950) HIP; shared helpers in csgn_device.h, design notes in DESIGN.md ("Gates").
//
// A term decrypts to the AND of the key's d positions in it (src/SecretKey.cpp:82-147), so the ALL-ONES term (every
// valid bit set, the low bits of the last word zero as in every canonical term) decrypts to 1 under every key and the
// all-zero term to 0.  Every gate is a composition of the reference's own operator+ (concatenation) and operator*
// (all-pairs AND) with such a constant; the output of one element is a sequence of SEGMENTS:
//     copy of one operand | all-pairs product of two operands | one constant term
// e.g. OR(a, b) = (a + b) + (a * b) = [a][b][a x b].  The fused kernel writes every segment of every element in one
// launch, reading each operand from HBM once.
#include "csgn_device.h"
#include "csgn_hip.h"

#include <algorithm>

namespace csgn {

namespace {

// One constant term per element: ONE where plain[e] & 1 (or `bit` when plain is null), ZERO elsewhere, written at
// out + e * pitch (units).  Written by the kernel: no compute path calls hipMemsetAsync (csgn_device.h, zero_words).
template <typename Unit>
__global__ void __launch_bounds__(256) k_const_fill(const uint8_t *__restrict__ plain, u32 bit, Unit *__restrict__ out,
                                                    u32 total_units, u32 U, FastDiv dU, u64 pitch, u64 last_mask)
{
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total_units)
        return;
    const u32 e = csgn_fastdiv(g, dU), k = g - e * U;
    const bool one = (plain ? plain[e] & 1u : bit) != 0u;
    unit_store<Unit, true>(out + (u64)e * pitch + k, one ? one_unit(Unit(), k, U, last_mask) : zero_unit(Unit()));
}

// ---------------------------------------------------------------------------------------
// The fused uniform gate.  Operands: 0 = sel, 1 = a, 2 = b; an element of operand o has t[o] terms.  Segment s covers
// the element's output units [end[s-1], end[s]) and is
//     SEG_COPY  (x):    the terms of operand x
//     SEG_PROD  (x, y): operand x * operand y, all pairs, row i = x's term i against every term of y; y = 3 is the
//                       concatenation a || b (MUX: s * (a + b))
//     SEG_CONST:        one constant term, ONE or -- plain_mode 1 -- the one plain[e] names
// plain_mode 2 (mulPlain): the copy segment is ANDed with plain[e] ? ONE : ZERO.
// Modelled on the flat small-shape multiply (csgn_mul.hip, k_mul_flat): one 16-byte (8-byte when dL is odd) output
// unit per lane, found by FastDiv; a product row's left term is re-read from cache by every lane of the row.  A lane
// issues its two loads unconditionally from selected bases (a branch around each load costs a full wait apiece,
// csgn_add.hip, k_add_ragged_flat) and combines them as (A & B & m) | c.
// ---------------------------------------------------------------------------------------
enum { SEG_COPY = 0, SEG_PROD = 1, SEG_CONST = 2 };

struct GateArgs {
    const void *op[3];        // sel, a, b (unused ones may be null: never selected)
    const uint8_t *plain;
    void *out;
    u32 t[3];                 // terms per element of each operand
    u32 nseg;
    u32 end[4];               // segment ends in units, end[nseg-1] = EU
    u32 kind[4], x[4], y[4];
    u32 U, EU;                // units per term, per output element
    u32 total_units;          // this launch
    u32 plain_mode;           // 0 none, 1 constant chosen by plain[e], 2 copy ANDed with plain[e]
    u32 xcd;
    FastDiv dEU, dU, dRow;    // dRow: units of one product row (t[y] * U, or (t[a] + t[b]) * U for y = 3)
    u64 last_mask;
};

template <typename Unit>
__device__ inline const Unit *gate_op(const GateArgs &a, u32 o)
{
    const void *p = o == 0u ? a.op[0] : (o == 1u ? a.op[1] : a.op[2]);
    return reinterpret_cast<const Unit *>(p);
}

template <typename Unit>
__global__ void __launch_bounds__(256) k_gate_fused(GateArgs a)
{
    const u32 bid = a.xcd ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const u32 g = bid * 256u + threadIdx.x;
    if (g >= a.total_units)
        return;
    const u32 e = csgn_fastdiv(g, a.dEU), r = g - e * a.EU;
    // the lane's segment (every s past nseg has end[s] = EU: never taken)
    const u32 s = (r >= a.end[0] ? 1u : 0u) + (r >= a.end[1] ? 1u : 0u) + (r >= a.end[2] ? 1u : 0u);
    const u32 start = s == 0u ? 0u : (s == 1u ? a.end[0] : (s == 2u ? a.end[1] : a.end[2]));
    const u32 kind = s == 0u ? a.kind[0] : (s == 1u ? a.kind[1] : (s == 2u ? a.kind[2] : a.kind[3]));
    const u32 x = s == 0u ? a.x[0] : (s == 1u ? a.x[1] : (s == 2u ? a.x[2] : a.x[3]));
    const u32 y = s == 0u ? a.y[0] : (s == 1u ? a.y[1] : (s == 2u ? a.y[2] : a.y[3]));
    const u32 U = a.U, rr = r - start;
    const u32 tx = x == 0u ? a.t[0] : (x == 1u ? a.t[1] : a.t[2]);
    // product coordinates (harmless for the other kinds: only selected below)
    const u32 i = csgn_fastdiv(rr, a.dRow), c = rr - i * a.dRow.d;
    const u32 k = c - csgn_fastdiv(c, a.dU) * U;
    // A: operand x, B: operand y (products) or x again (copies; the second load hits the same line)
    const Unit *pa = gate_op<Unit>(a, x);
    u64 ia = (u64)e * tx * U + (kind == SEG_PROD ? i * U + k : (kind == SEG_COPY ? rr : 0u));
    const Unit *pb = pa;
    u64 ib = ia;
    if (kind == SEG_PROD) {                       // (selects, no loads inside)
        const u32 ta = a.t[1] * U;
        const bool concat_b = y == 3u && c >= ta;
        const u32 yo = y == 3u ? (concat_b ? 2u : 1u) : y;
        const u32 ty = yo == 0u ? a.t[0] : (yo == 1u ? a.t[1] : a.t[2]);
        pb = gate_op<Unit>(a, yo);
        ib = (u64)e * ty * U + (concat_b ? c - ta : c);
    }
    const Unit va = pa[ia], vb = pb[ib];
    bool keep = kind != SEG_CONST, one = kind == SEG_CONST;
    if (a.plain_mode) {                           // (launch-uniform)
        const bool p = (a.plain[e] & 1u) != 0u;
        if (a.plain_mode == 1u)
            one = one && p;
        else
            keep = keep && p;
    }
    const Unit v = (keep ? va & vb : zero_unit(Unit())) |
                   (one ? one_unit(Unit(), rr, U, a.last_mask) : zero_unit(Unit()));
    unit_store<Unit, true>(reinterpret_cast<Unit *>(a.out) + g, v);
}

struct GateShape {
    u32 nseg;
    u32 kind[4], x[4], y[4];
    u64 terms[4];             // terms per element of each segment
    int prod;                 // index of the product segment, -1 = none
};

// the table of include/csgn_hip.h: the segments of one output element
bool gate_shape(int gate, u64 ts, u64 ta, u64 tb, GateShape &g)
{
    g = GateShape();
    g.prod = -1;
    auto seg = [&](u32 kind, u32 x, u32 y, u64 terms) {
        const u32 s = g.nseg++;
        g.kind[s] = kind;
        g.x[s] = x;
        g.y[s] = y;
        g.terms[s] = terms;
        if (kind == SEG_PROD)
            g.prod = (int)s;
    };
    switch (gate) {
    case CSGN_GATE_NOT: seg(SEG_COPY, 1, 1, ta); seg(SEG_CONST, 1, 1, 1); break;
    case CSGN_GATE_XNOR: seg(SEG_COPY, 1, 1, ta); seg(SEG_COPY, 2, 2, tb); seg(SEG_CONST, 1, 1, 1); break;
    case CSGN_GATE_NAND: seg(SEG_PROD, 1, 2, ta * tb); seg(SEG_CONST, 1, 1, 1); break;
    case CSGN_GATE_OR: seg(SEG_COPY, 1, 1, ta); seg(SEG_COPY, 2, 2, tb); seg(SEG_PROD, 1, 2, ta * tb); break;
    case CSGN_GATE_NOR:
        seg(SEG_COPY, 1, 1, ta); seg(SEG_COPY, 2, 2, tb); seg(SEG_PROD, 1, 2, ta * tb); seg(SEG_CONST, 1, 1, 1);
        break;
    case CSGN_GATE_MUX: seg(SEG_PROD, 0, 3, ts * (ta + tb)); seg(SEG_COPY, 2, 2, tb); break;
    case CSGN_GATE_ADD_PLAIN: seg(SEG_COPY, 1, 1, ta); seg(SEG_CONST, 1, 1, 1); break;
    case CSGN_GATE_MUL_PLAIN: seg(SEG_COPY, 1, 1, ta); break;
    default: return false;
    }
    return true;
}

// Fused form: product segments up to this many terms per element.  Past it the pitched form (the tuned multiply
// launchers writing into the output's slices) takes over.  Measured on MI355X (OR at N=1247, DESIGN.md "Gates"):
// fused / pitched 6.1 / 4.9 TB/s at 2x2, 5.4 / 4.3 at 4x5, level at 8x8, 4.2 / 4.3 at 16x16, 5.5 / 6.2 at 64x64.
constexpr u64 kFusedMaxProductTerms = 64;

// the form a call takes: true = fused
bool gate_use_fused(int gate, u64 ts, u64 ta, u64 tb)
{
    // mulPlain has no composed form (a per-element select), MUX over a multi-term selector has none without an
    // intermediate buffer (its product rows interleave s_i & a with s_i & b)
    if (gate == CSGN_GATE_MUL_PLAIN || (gate == CSGN_GATE_MUX && ts != 1))
        return true;
    GateShape g;
    gate_shape(gate, ts, ta, tb, g);
    return tune_choose(TUNE_GATE_FUSED, g.prod < 0 || g.terms[g.prod] <= kFusedMaxProductTerms);
}

template <typename Unit>
hipError_t gate_fused(const GateShape &sh, u64 n_bits, u64 batch, const u64 *t, const u64 *const *ops,
                      const uint8_t *plain, u32 plain_mode, u64 *out, u32 U, hipStream_t s)
{
    GateArgs a = {};
    a.plain = plain;
    a.plain_mode = plain_mode;
    a.U = U;
    a.last_mask = last_word_mask(n_bits);
    a.nseg = sh.nseg;
    u64 run = 0;
    for (u32 i = 0; i < 4; ++i) {
        if (i < sh.nseg) {
            run += sh.terms[i] * U;
            a.kind[i] = sh.kind[i];
            a.x[i] = sh.x[i];
            a.y[i] = sh.y[i];
        }
        a.end[i] = (u32)run;
    }
    a.EU = (u32)run;
    for (int o = 0; o < 3; ++o)
        a.t[o] = (u32)t[o];
    u32 row = 1;
    if (sh.prod >= 0)
        row = (sh.y[sh.prod] == 3u ? (u32)(t[1] + t[2]) : (u32)t[sh.y[sh.prod]]) * U;
    a.dRow = csgn_fastdiv_make(row);
    a.dU = csgn_fastdiv_make(U);
    a.dEU = csgn_fastdiv_make(a.EU);
    a.xcd = stream_xcd(batch * run);
    const u64 per = std::max<u64>(1, 0xFFFFFF00ull / run);           // elements per launch: < 2^32 units
    for (u64 e0 = 0; e0 < batch; e0 += per) {
        const u64 ne = std::min(per, batch - e0);
        for (int o = 0; o < 3; ++o)
            a.op[o] = ops[o] ? reinterpret_cast<const Unit *>(ops[o]) + e0 * t[o] * U : nullptr;
        a.plain = plain ? plain + e0 : nullptr;
        a.out = reinterpret_cast<Unit *>(out) + e0 * run;
        a.total_units = (u32)(ne * run);
        k_gate_fused<Unit><<<ceil_div_u64(a.total_units, 256u), 256, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------------------ public

u64 gate_terms(int gate, u64 ts, u64 ta, u64 tb)
{
    GateShape g;
    if (!gate_shape(gate, ts, ta, tb, g))
        return 0;
    // every operand the gate reads needs a term
    const bool uses_s = gate == CSGN_GATE_MUX;
    const bool uses_b = gate == CSGN_GATE_XNOR || gate == CSGN_GATE_NAND || gate == CSGN_GATE_OR ||
                        gate == CSGN_GATE_NOR || gate == CSGN_GATE_MUX;
    if (ta == 0 || (uses_s && ts == 0) || (uses_b && tb == 0))
        return 0;
    if (ta >= kTermLimit || tb >= kTermLimit || ts >= kTermLimit)
        return 0;
    u64 p = 0, total = 0;
    if (uses_s)                                                         // ts * (ta + tb) + tb
        return term_mul(ts, ta + tb, p) && p + tb < kTermLimit ? p + tb : 0;
    if (uses_b && gate != CSGN_GATE_XNOR && !term_mul(ta, tb, p))
        return 0;
    for (u32 i = 0; i < g.nseg; ++i)
        total += g.terms[i];
    return total < kTermLimit ? total : 0;
}

const char *gate_kernel_name(u64 n_bits, int gate, u64 batch, u64 ts, u64 ta, u64 tb)
{
    (void)n_bits;
    (void)batch;
    if (gate_terms(gate, ts, ta, tb) == 0)
        return "";
    return gate_use_fused(gate, ts, ta, tb) ? "k_gate_fused" : "pitched";
}

hipError_t const_fill(u64 n_bits, u64 batch, const uint8_t *plain, int bit, u64 *out, u64 pitch_words,
                      hipStream_t s)
{
    const u64 dL = (n_bits + 63) / 64;
    if (batch == 0)
        return hipSuccess;
    if (pitch_words == 0)
        pitch_words = dL;
    const bool wide = pitch_words % 2 == 0 && wide_units(dL, out);
    const u32 U = (u32)(wide ? dL / 2 : dL);
    const u64 pitch = wide ? pitch_words / 2 : pitch_words;
    const FastDiv dU = csgn_fastdiv_make(U);
    const u64 per = 0xFFFFFF00ull / U;
    for (u64 e0 = 0; e0 < batch; e0 += per) {
        const u64 ne = std::min(per, batch - e0);
        const u32 tot = (u32)(ne * U);
        const uint8_t *p = plain ? plain + e0 : nullptr;
        if (wide)
            k_const_fill<unit16><<<ceil_div_u64(tot, 256u), 256, 0, s>>>(
                p, bit ? 1u : 0u, reinterpret_cast<unit16 *>(out) + e0 * pitch, tot, U, dU, pitch, last_word_mask(n_bits));
        else
            k_const_fill<unit8><<<ceil_div_u64(tot, 256u), 256, 0, s>>>(
                p, bit ? 1u : 0u, out + e0 * pitch, tot, U, dU, pitch, last_word_mask(n_bits));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t gate_uniform(u64 n_bits, int gate, u64 batch, u64 ts, u64 ta, u64 tb, const u64 *S, const u64 *A,
                        const u64 *B, const uint8_t *plain, u64 *out, hipStream_t s)
{
    GateShape sh;
    if (batch == 0)
        return hipSuccess;
    if (!gate_shape(gate, ts, ta, tb, sh))
        return hipErrorInvalidValue;
    const u64 dL = (n_bits + 63) / 64;
    const u64 t[3] = {ts, ta, tb};
    const u64 *ops[3] = {S, A, B};
    if (gate_use_fused(gate, ts, ta, tb)) {
        const bool wide = wide_units(dL, S, A, B, out);
        const u32 U = (u32)(wide ? dL / 2 : dL);
        const u32 pm = gate == CSGN_GATE_ADD_PLAIN ? 1u : (gate == CSGN_GATE_MUL_PLAIN ? 2u : 0u);
        return wide ? gate_fused<unit16>(sh, n_bits, batch, t, ops, plain, pm, out, U, s)
                    : gate_fused<unit8>(sh, n_bits, batch, t, ops, plain, pm, out, U, s);
    }
    // pitched: every segment by its own tuned launcher, straight into the element's slice of the output
    u64 elem = 0;
    for (u32 i = 0; i < sh.nseg; ++i)
        elem += sh.terms[i];
    const u64 pitch = elem * dL;
    u64 at = 0;                                                          // words into the element
    for (u32 i = 0; i < sh.nseg; ++i) {
        hipError_t e = hipSuccess;
        if (sh.kind[i] == SEG_COPY)
            e = add_uniform(n_bits, batch, t[sh.x[i]], 0, ops[sh.x[i]], nullptr, out + at, s, pitch);
        else if (sh.kind[i] == SEG_CONST)
            e = const_fill(n_bits, batch, gate == CSGN_GATE_ADD_PLAIN ? plain : nullptr, 1, out + at, pitch, s);
        else if (sh.y[i] != 3u)
            e = mul_uniform(n_bits, batch, t[sh.x[i]], t[sh.y[i]], ops[sh.x[i]], ops[sh.y[i]], out + at, 0, s, pitch);
        else {                                                           // MUX, 1-term selector: s*a then s*b
            e = mul_uniform(n_bits, batch, 1, ta, S, A, out + at, 0, s, pitch);
            if (e == hipSuccess)
                e = mul_uniform(n_bits, batch, 1, tb, S, B, out + at + ta * dL, 0, s, pitch);
        }
        if (e != hipSuccess)
            return e;
        at += sh.terms[i] * dL;
    }
    return hipSuccess;
}

} // namespace csgn
