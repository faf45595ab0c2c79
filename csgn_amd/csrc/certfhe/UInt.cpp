// UInt.cpp -- encrypted unsigned integers as bit-planes (extension, see UInt.h) over csgn_uint_step and the gates.
#include "UInt.h"

#include "Gates.h"
#include "runtime.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

namespace certFHE {

using detail::BatchAccess;
using detail::ones;

namespace {

const uint64_t kMaxWords = 1ull << 31;   // per element, as in every csgn_*_uniform entry point

void requireWidth(unsigned width, const char *who)
{
    if (width < 1 || width > 64)
        throw std::invalid_argument(std::string("certFHE::UIntBatch::") + who + ": width must be 1..64");
}

std::vector<unsigned char> bitPlane(const std::vector<uint64_t> &values, unsigned j)
{
    std::vector<unsigned char> bits(values.size());
    for (size_t i = 0; i < values.size(); ++i)
        bits[i] = (unsigned char)((values[i] >> j) & 1u);
    return bits;
}

void requireFits(const std::vector<uint64_t> &values, unsigned width, const char *who)
{
    requireWidth(width, who);
    for (size_t i = 0; i < values.size(); ++i)
        if (width < 64 && values[i] >> width)
            throw std::invalid_argument(std::string("certFHE::UIntBatch::") + who + ": a value does not fit in the width");
}

bool sameContext(const Context &x, const Context &y) { return x.getN() == y.getN() && x.getD() == y.getD(); }

void requireSame(const UIntBatch &a, const UIntBatch &b, const char *who)
{
    if (a.width() != b.width() || a.size() != b.size() || !sameContext(a.context(), b.context()))
        throw std::invalid_argument(std::string("certFHE::") + who + ": operands differ in width, count or context");
}

void requireSameBit(const CiphertextBatch &s, const UIntBatch &a, const char *who)
{
    if (s.size() != a.size() || !sameContext(s.context(), a.context()))
        throw std::invalid_argument(std::string("certFHE::") + who + ": selector differs in count or context");
}

// ------------------------------------------------------------------ sizes, before anything is launched

// terms per element of a plane (a ragged plane: its largest element, a bound for everything computed from it)
uint64_t termsOf(const CiphertextBatch &b)
{
    if (b.uniform())
        return b.terms();
    uint64_t m = 0;
    for (uint64_t i = 0; i < b.size(); ++i)
        m = b.termsOf(i) > m ? b.termsOf(i) : m;
    return m;
}

// a step's size, checked against the ABI's limit
uint64_t checked(uint64_t terms, const Context &ctx, const char *who)
{
    if (terms == 0 || terms > (kMaxWords - 1) / ctx.getDefaultN())
        throw std::invalid_argument(std::string("certFHE::") + who +
                                    ": a step's result exceeds 2^31 words per element (the width is too large)");
    return terms;
}

uint64_t stepTerms(int step, int output, uint64_t tx, uint64_t ta, uint64_t tb, const Context &ctx, const char *who)
{
    return checked(csgn_uint_step_terms(step, output, tx, ta, tb), ctx, who);
}

uint64_t gateTerms(int gate, uint64_t ts, uint64_t ta, uint64_t tb, const Context &ctx, const char *who)
{
    return checked(csgn_gate_terms(gate, ts, ta, tb), ctx, who);
}

// ------------------------------------------------------------------ plane lists

// The operand planes of one call: their terms per element (a ragged plane: its largest element, a bound for
// everything computed from it) and whether all of them are uniform, which is when the call is one launch.
struct Planes {
    std::vector<const CiphertextBatch *> list;
    std::vector<uint64_t> terms;
    bool uniform = true;

    void add(const CiphertextBatch &p)
    {
        list.push_back(&p);
        terms.push_back(termsOf(p));
        uniform = uniform && p.uniform();
    }
    explicit Planes(const std::vector<CiphertextBatch> &planes)
    {
        for (size_t j = 0; j < planes.size(); ++j)
            add(planes[j]);
    }
    explicit Planes(const UIntBatch &a)
    {
        for (unsigned j = 0; j < a.width(); ++j)
            add(a.plane(j));
    }
};

std::vector<const uint64_t *> sources(const Planes &p)
{
    std::vector<const uint64_t *> src(p.list.size());
    for (size_t j = 0; j < src.size(); ++j)
        src[j] = p.list[j]->deviceValues();
    return src;
}

// one fresh uniform batch of T[j] terms per element for every j
std::vector<CiphertextBatch> makePlanes(const Context &ctx, uint64_t count, const std::vector<uint64_t> &T)
{
    std::vector<CiphertextBatch> out;
    out.reserve(T.size());
    for (size_t j = 0; j < T.size(); ++j)
        out.push_back(BatchAccess::make(ctx, count, T[j]));
    return out;
}

std::vector<uint64_t *> wordsOf(std::vector<CiphertextBatch> &planes)
{
    std::vector<uint64_t *> dst(planes.size());
    for (size_t j = 0; j < dst.size(); ++j)
        dst[j] = BatchAccess::words(planes[j]);
    return dst;
}

// make(j) for every plane j < n, after check(j) has passed for every plane: nothing is launched before all sizes fit
template <typename Check, typename Make>
std::vector<CiphertextBatch> mapPlanes(unsigned n, Check check, Make make)
{
    for (unsigned j = 0; j < n; ++j)
        check(j);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < n; ++j)
        planes.push_back(make(j));
    return planes;
}

void noCheck(unsigned) {}

// ------------------------------------------------------------------ the plane-by-plane operators

// Whether an operator that works plane by plane is one csgn_uint_bitwise call: every operand plane uniform.  Ragged
// planes (and empty batches) take the CiphertextBatch operators and Gates.h plane by plane, with the same words.
bool bitwiseCall(int op, uint64_t ts, const std::vector<uint64_t> &ta, const std::vector<uint64_t> &tb, bool uniform)
{
    if (!uniform || ta.empty() || ta.size() > 64 || (!tb.empty() && tb.size() != ta.size()))
        return false;
    for (size_t j = 0; j < ta.size(); ++j)
        if (csgn_uint_bitwise_terms(op, ts, ta[j], tb.empty() ? 0 : tb[j]) == 0)
            return false;                                 // a shape the call would refuse
    return true;
}

// Output planes of `op` over the planes pa (and pb, sel where the op reads them): check(j) for every plane first, so
// that nothing is allocated before all sizes fit; then ONE csgn_uint_bitwise call into fresh planes, or make(j) plane
// by plane.
template <typename Check, typename Make>
std::vector<CiphertextBatch> bitwisePlanes(int op, const CiphertextBatch *sel, const Planes &pa, const Planes *pb,
                                           Check check, Make make)
{
    const unsigned w = (unsigned)pa.list.size();
    const uint64_t count = pa.list[0]->size(), ts = sel ? termsOf(*sel) : 0;
    const bool uniform = pa.uniform && (!pb || pb->uniform) && (!sel || sel->uniform());
    if (count == 0 || !bitwiseCall(op, ts, pa.terms, pb ? pb->terms : std::vector<uint64_t>(), uniform))
        return mapPlanes(w, check, make);
    std::vector<uint64_t> T(w);
    for (unsigned j = 0; j < w; ++j) {
        check(j);
        T[j] = csgn_uint_bitwise_terms(op, ts, pa.terms[j], pb ? pb->terms[j] : 0);
    }
    const Context &ctx = pa.list[0]->context();
    std::vector<CiphertextBatch> out = makePlanes(ctx, count, T);
    detail::check(csgn_uint_bitwise(ctx.getN(), op, count, w, sel ? sel->deviceValues() : nullptr, ts, sources(pa).data(),
                                    pa.terms.data(), pb ? sources(*pb).data() : nullptr, pb ? pb->terms.data() : nullptr,
                                    wordsOf(out).data(), detail::stream()),
                  "csgn_uint_bitwise");
    return out;
}

// mask * planes[j] for every plane: the classes of sumWhere and the planes of keepWhere
std::vector<CiphertextBatch> keepPlanes(const CiphertextBatch &mask, const std::vector<CiphertextBatch> &planes, const char *who)
{
    const Planes pa(planes);
    return bitwisePlanes(
        CSGN_UINT_BITWISE_KEEP, &mask, pa, nullptr,
        [&](unsigned j) {
            const uint64_t ts = termsOf(mask), ta = pa.terms[j];
            checked(ta && ts > (kMaxWords / ta) ? 0 : ts * ta, mask.context(), who);
        },
        [&](unsigned j) { return mask * planes[j]; });
}

// ------------------------------------------------------------------ one step

bool allUniform(const CiphertextBatch *x, const CiphertextBatch &a, const CiphertextBatch &b)
{
    return (!x || x->uniform()) && a.uniform() && b.uniform();
}

// out[0] = the step's output 0, out[1] = the carry when `carry` (ADD steps)
std::vector<CiphertextBatch> step(int st, const CiphertextBatch *x, const CiphertextBatch &a, const CiphertextBatch &b,
                                  bool carry)
{
    std::vector<CiphertextBatch> out;
    if (allUniform(x, a, b)) {
        const uint64_t tx = x ? x->terms() : 0, ta = a.terms(), tb = b.terms();
        out.push_back(BatchAccess::make(a.context(), a.size(), csgn_uint_step_terms(st, 0, tx, ta, tb)));
        if (carry)
            out.push_back(BatchAccess::make(a.context(), a.size(), csgn_uint_step_terms(st, 1, tx, ta, tb)));
        if (a.size())
            detail::check(csgn_uint_step(a.context().getN(), st, a.size(), x ? x->deviceValues() : nullptr, tx,
                                         a.deviceValues(), ta, b.deviceValues(), tb, BatchAccess::words(out[0]),
                                         carry ? BatchAccess::words(out[1]) : nullptr, detail::stream()),
                          "csgn_uint_step");
        return out;
    }
    // ragged: the definition itself through the batch operators
    switch (st) {
    case CSGN_UINT_ADD_HALF:
        out.push_back(a + b);
        if (carry)
            out.push_back(a * b);
        break;
    case CSGN_UINT_ADD_FULL: {
        const CiphertextBatch ab = a + b;
        out.push_back(ab + *x);
        if (carry)
            out.push_back((a * b) + (ab * *x));
        break;
    }
    case CSGN_UINT_EQ_STEP: out.push_back(*x * ((a + b) + ones(a))); break;
    case CSGN_UINT_LT_FIRST: out.push_back((a + ones(a)) * b); break;
    default: out.push_back(((a + b) * (b + *x)) + *x); break;
    }
    return out;
}

// ------------------------------------------------------------------ whole operations

// Whether an operation of a and b is one call (csgn_uint_arith, or csgn_uint_lt_select for the comparison) or the
// per-bit chain below: ragged planes and integers wider than 16 bits take the chain.  Knob uint_arith_form decides for
// the rest when it is forced (0 the chain, 1 the one call); left per shape, a forced uint_fused keeps the chain, so
// that csgn_uint_step's two forms can still be run through these operators.
bool oneCall(unsigned width, bool uniform)
{
    if (width > 16 || !uniform)
        return false;
    int form = -1, steps = -1;
    csgn_get_tuning("uint_arith_form", &form);
    csgn_get_tuning("uint_fused", &steps);
    return form == 0 ? false : form == 1 ? true : steps == -1;
}

bool oneCall(const UIntBatch &a, const Planes &pa, const Planes &pb)
{
    return oneCall(a.width(), (pa.uniform && pb.uniform) || a.size() == 0);
}

// csgn_uint_arith into fresh planes of T[j] terms (one result for EQ / NE); *carry_out = the carry of carry_terms terms
std::vector<CiphertextBatch> arithPlanes(int op, const UIntBatch &a, const Planes &pa, const Planes &pb,
                                         const std::vector<uint64_t> &T, uint64_t carry_terms, CiphertextBatch *carry_out)
{
    const Context &ctx = a.context();
    std::vector<CiphertextBatch> out = makePlanes(ctx, a.size(), T);
    CiphertextBatch carry = BatchAccess::make(ctx, carry_out ? a.size() : 0, carry_terms);
    if (a.size())
        detail::check(csgn_uint_arith(ctx.getN(), op, a.size(), a.width(), sources(pa).data(), pa.terms.data(),
                                      sources(pb).data(), pb.terms.data(), wordsOf(out).data(),
                                      carry_out ? BatchAccess::words(carry) : nullptr, detail::stream()),
                      "csgn_uint_arith");
    if (carry_out)
        *carry_out = carry;
    return out;
}

// the planes of a + b; *carry_out (may be null) = the carry out of the top plane
std::vector<CiphertextBatch> add(const UIntBatch &a, const UIntBatch &b, CiphertextBatch *carry_out, const char *who)
{
    const Context &ctx = a.context();
    const unsigned w = a.width();
    std::vector<uint64_t> T(w);
    uint64_t c = T[0] = stepTerms(CSGN_UINT_ADD_HALF, 0, 0, termsOf(a.plane(0)), termsOf(b.plane(0)), ctx, who);
    if (w > 1 || carry_out)
        c = stepTerms(CSGN_UINT_ADD_HALF, 1, 0, termsOf(a.plane(0)), termsOf(b.plane(0)), ctx, who);
    for (unsigned j = 1; j < w; ++j) {
        const uint64_t ta = termsOf(a.plane(j)), tb = termsOf(b.plane(j));
        T[j] = stepTerms(CSGN_UINT_ADD_FULL, 0, c, ta, tb, ctx, who);
        if (j + 1 < w || carry_out)
            c = stepTerms(CSGN_UINT_ADD_FULL, 1, c, ta, tb, ctx, who);
    }
    const Planes pa(a), pb(b);
    if (oneCall(a, pa, pb))
        return arithPlanes(CSGN_UINT_ARITH_ADD, a, pa, pb, T, c, carry_out);
    std::vector<CiphertextBatch> r = step(CSGN_UINT_ADD_HALF, nullptr, a.plane(0), b.plane(0), w > 1 || carry_out);
    std::vector<CiphertextBatch> out(1, r[0]);
    for (unsigned j = 1; j < w; ++j) {
        const CiphertextBatch carry = r[1];
        r = step(CSGN_UINT_ADD_FULL, &carry, a.plane(j), b.plane(j), j + 1 < w || carry_out);
        out.push_back(r[0]);
    }
    if (carry_out)
        *carry_out = r[1];
    return out;
}

// the planes of a - b = a + ~b + 1; *carry_out (may be null) = the carry out of the top plane: 1 where a >= b
std::vector<CiphertextBatch> sub(const UIntBatch &a, const UIntBatch &b, CiphertextBatch *carry_out, const char *who)
{
    const Context &ctx = a.context();
    const unsigned w = a.width();
    std::vector<uint64_t> T(w);
    uint64_t c = 1;
    for (unsigned j = 0; j < w; ++j) {
        const uint64_t ta = termsOf(a.plane(j)), tnb = gateTerms(CSGN_GATE_NOT, 0, termsOf(b.plane(j)), 0, ctx, who);
        T[j] = stepTerms(CSGN_UINT_ADD_FULL, 0, c, ta, tnb, ctx, who);
        if (j + 1 < w || carry_out)
            c = stepTerms(CSGN_UINT_ADD_FULL, 1, c, ta, tnb, ctx, who);
    }
    const Planes pa(a), pb(b);
    if (oneCall(a, pa, pb))
        return arithPlanes(CSGN_UINT_ARITH_SUB, a, pa, pb, T, c, carry_out);
    CiphertextBatch carry = ones(a.plane(0));                // a + ~b + 1: the first carry in is ONE
    std::vector<CiphertextBatch> out;
    for (unsigned j = 0; j < w; ++j) {
        const bool more = j + 1 < w || carry_out;
        const std::vector<CiphertextBatch> r = step(CSGN_UINT_ADD_FULL, &carry, a.plane(j), logicNot(b.plane(j)), more);
        out.push_back(r[0]);
        if (more)
            carry = r[1];
    }
    if (carry_out)
        *carry_out = carry;
    return out;
}

// sizes of lessThan(a, b)'s steps, checked; returns the result's terms
uint64_t lessThanTerms(const UIntBatch &a, const UIntBatch &b, const char *who)
{
    const Context &ctx = a.context();
    uint64_t l = stepTerms(CSGN_UINT_LT_FIRST, 0, 0, termsOf(a.plane(0)), termsOf(b.plane(0)), ctx, who);
    for (unsigned j = 1; j < a.width(); ++j)
        l = stepTerms(CSGN_UINT_LT_STEP, 0, l, termsOf(a.plane(j)), termsOf(b.plane(j)), ctx, who);
    return l;
}

// lessThan(a, b) after lessThanTerms, of `terms` terms when the caller has them (0: the chain alone): the comparison
// alone from csgn_uint_lt_select (no requests, d_less), or the chain
CiphertextBatch lessThanUnchecked(const UIntBatch &a, const UIntBatch &b, uint64_t terms = 0)
{
    if (terms) {
        const Planes pa(a), pb(b);
        if (oneCall(a, pa, pb)) {
            CiphertextBatch out = BatchAccess::make(a.context(), a.size(), terms);
            if (a.size())
                detail::check(csgn_uint_lt_select(a.context().getN(), a.size(), a.width(), sources(pa).data(),
                                                  pa.terms.data(), sources(pb).data(), pb.terms.data(), 0, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr, BatchAccess::words(out), detail::stream()),
                              "csgn_uint_lt_select");
            return out;
        }
    }
    CiphertextBatch l = step(CSGN_UINT_LT_FIRST, nullptr, a.plane(0), b.plane(0), false)[0];
    for (unsigned j = 1; j < a.width(); ++j)
        l = step(CSGN_UINT_LT_STEP, &l, a.plane(j), b.plane(j), false)[0];
    return l;
}

uint64_t equalToTerms(const UIntBatch &a, const UIntBatch &b, const char *who)
{
    const Context &ctx = a.context();
    uint64_t e = gateTerms(CSGN_GATE_XNOR, 0, termsOf(a.plane(0)), termsOf(b.plane(0)), ctx, who);
    for (unsigned j = 1; j < a.width(); ++j)
        e = stepTerms(CSGN_UINT_EQ_STEP, 0, e, termsOf(a.plane(j)), termsOf(b.plane(j)), ctx, who);
    return e;
}

// equalTo(a, b) after equalToTerms, or its logicNot when `negate`; `terms`: the result's
CiphertextBatch equalToUnchecked(const UIntBatch &a, const UIntBatch &b, uint64_t terms, bool negate)
{
    const Planes pa(a), pb(b);
    if (oneCall(a, pa, pb))
        return arithPlanes(negate ? CSGN_UINT_ARITH_NE : CSGN_UINT_ARITH_EQ, a, pa, pb, std::vector<uint64_t>(1, terms), 0,
                           nullptr)[0];
    CiphertextBatch e = logicXnor(a.plane(0), b.plane(0));
    for (unsigned j = 1; j < a.width(); ++j)
        e = step(CSGN_UINT_EQ_STEP, &e, a.plane(j), b.plane(j), false)[0];
    return negate ? logicNot(e) : e;
}

// ------------------------------------------------------------------ comparisons with a public constant

CiphertextBatch comparePlain(int cmp, const UIntBatch &a, uint64_t k, const char *who)
{
    const unsigned w = a.width();
    if (w < 64 && (k >> w) != 0)
        throw std::invalid_argument(std::string("certFHE::") + who + ": the constant does not fit in the width");
    const Context &ctx = a.context();
    const Planes in(a);
    const uint64_t total = checked(csgn_uint_plain_terms(cmp, w, k, in.terms.data()), ctx, who);
    if (in.uniform) {
        CiphertextBatch out = BatchAccess::make(ctx, a.size(), total);
        if (a.size())
            detail::check(csgn_uint_plain(ctx.getN(), cmp, a.size(), w, k, sources(in).data(), in.terms.data(),
                                          BatchAccess::words(out), detail::stream()),
                          "csgn_uint_plain");
        return out;
    }
    // ragged: the definition itself through the batch operators (every intermediate is no larger than the result)
    const int base = cmp == CSGN_UINT_PLAIN_NE ? CSGN_UINT_PLAIN_EQ : cmp == CSGN_UINT_PLAIN_LE ? CSGN_UINT_PLAIN_GT
                   : cmp == CSGN_UINT_PLAIN_GE ? CSGN_UINT_PLAIN_LT : cmp;
    auto bit = [&](unsigned j) { return (k >> j) & 1u; };
    auto n = [&](unsigned j) { return logicNot(a.plane(j)); };
    const uint64_t all = w == 64 ? ~0ull : (1ull << w) - 1;
    CiphertextBatch r = a.plane(0);
    if ((base == CSGN_UINT_PLAIN_LT && k == 0) || (base == CSGN_UINT_PLAIN_GT && k == all)) {
        r = constantBatch(ctx, std::vector<unsigned char>(a.size(), 0));
    } else if (base == CSGN_UINT_PLAIN_EQ) {
        r = bit(0) ? a.plane(0) : n(0);
        for (unsigned j = 1; j < w; ++j)
            r = r * (bit(j) ? a.plane(j) : n(j));
    } else if (base == CSGN_UINT_PLAIN_LT) {
        const unsigned m = (unsigned)__builtin_ctzll(k);
        r = n(m);
        for (unsigned j = m + 1; j < w; ++j)
            r = bit(j) ? (r * a.plane(j)) + n(j) : r * n(j);
    } else {
        const unsigned m = (unsigned)__builtin_ctzll(~k);
        r = a.plane(m);
        for (unsigned j = m + 1; j < w; ++j)
            r = bit(j) ? r * a.plane(j) : (r * n(j)) + a.plane(j);
    }
    return base != cmp ? logicNot(r) : r;
}

// ------------------------------------------------------------------ arithmetic with a public constant

void requireConstant(const UIntBatch &a, uint64_t k, const char *who)
{
    if (a.width() < 64 && (k >> a.width()) != 0)
        throw std::invalid_argument(std::string("certFHE::") + who + ": the constant does not fit in the width");
}

uint64_t maskOf(unsigned w) { return w == 64 ? ~0ull : (1ull << w) - 1; }

// the planes of a + k (csgn_uint_addk's definition), each followed by ONE when `negate`; *carry_out = the last carry
std::vector<CiphertextBatch> addPlain(const UIntBatch &a, uint64_t k, bool negate, CiphertextBatch *carry_out,
                                      const char *who)
{
    requireConstant(a, k, who);
    const unsigned w = a.width();
    const Context &ctx = a.context();
    const Planes in(a);
    std::vector<uint64_t> T(w + 1);
    if (!csgn_uint_addk_terms(w, k, in.terms.data(), T.data()))
        checked(0, ctx, who);
    for (unsigned j = 0; j < w; ++j)
        T[j] = checked(T[j] + (negate ? 1 : 0), ctx, who);
    if (carry_out)
        checked(T[w], ctx, who);
    if (in.uniform) {
        const uint64_t carry_terms = T[w];
        T.pop_back();
        std::vector<CiphertextBatch> out = makePlanes(ctx, a.size(), T);
        CiphertextBatch carry = BatchAccess::make(ctx, carry_out ? a.size() : 0, carry_terms);
        if (a.size())
            detail::check(csgn_uint_addk(ctx.getN(), a.size(), w, k, negate ? 1 : 0, sources(in).data(), in.terms.data(),
                                         wordsOf(out).data(), carry_out ? BatchAccess::words(carry) : nullptr,
                                         detail::stream()),
                          "csgn_uint_addk");
        if (carry_out)
            *carry_out = carry;
        return out;
    }
    std::vector<CiphertextBatch> out;
    // ragged: the definition itself through the batch operators
    if (k == 0) {
        for (unsigned j = 0; j < w; ++j)
            out.push_back(negate ? logicNot(a.plane(j)) : a.plane(j));
        if (carry_out)
            *carry_out = constantBatch(ctx, std::vector<unsigned char>(a.size(), 0));
        return out;
    }
    const unsigned m = (unsigned)__builtin_ctzll(k);
    CiphertextBatch c = a.plane(m);
    for (unsigned j = 0; j < w; ++j) {
        const bool bit = (k >> j) & 1u;
        CiphertextBatch o = a.plane(j);
        if (j == m) {
            o = logicNot(o);
        } else if (j > m) {
            o = o + c;
            if (bit)
                o = logicNot(o);
            if (j + 1 < w || carry_out)
                c = bit ? (c * logicNot(a.plane(j))) + a.plane(j) : c * a.plane(j);
        }
        out.push_back(negate ? logicNot(o) : o);
    }
    if (carry_out)
        *carry_out = c;
    return out;
}

CiphertextBatch zeros(const UIntBatch &a)
{
    return constantBatch(a.context(), std::vector<unsigned char>(a.size(), 0));
}

} // namespace

// ------------------------------------------------------------------ UIntBatch

UIntBatch::UIntBatch(const std::vector<CiphertextBatch> &planes) : planes_(planes) {}

namespace {
// the bit bytes of every plane, plane after plane, in one pass over the values
std::vector<unsigned char> bitPlanes(const std::vector<uint64_t> &values, unsigned width)
{
    const size_t count = values.size();
    std::vector<unsigned char> bits((size_t)width * count);
    for (size_t i = 0; i < count; ++i)
        for (unsigned j = 0; j < width; ++j)
            bits[(size_t)j * count + i] = (unsigned char)((values[i] >> j) & 1u);
    return bits;
}
} // namespace

UIntBatch UIntBatch::encrypt(const SecretKey &key, const std::vector<uint64_t> &values, unsigned width)
{
    requireFits(values, width, "encrypt");
    return UIntBatch(BatchAccess::encryptPlanes(key, bitPlanes(values, width), values.size(), width, nullptr));
}

UIntBatch UIntBatch::encrypt(const SecretKey &key, const std::vector<uint64_t> &values, unsigned width, uint64_t seed)
{
    requireFits(values, width, "encrypt");
    return UIntBatch(BatchAccess::encryptPlanes(key, bitPlanes(values, width), values.size(), width, &seed));
}

UIntBatch UIntBatch::constant(const Context &context, const std::vector<uint64_t> &values, unsigned width)
{
    requireFits(values, width, "constant");
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < width; ++j)
        planes.push_back(constantBatch(context, bitPlane(values, j)));
    return UIntBatch(planes);
}

UIntBatch UIntBatch::fromPlanes(const std::vector<CiphertextBatch> &planes)
{
    requireWidth((unsigned)(planes.size() > 64 ? 65 : planes.size()), "fromPlanes");
    for (size_t j = 1; j < planes.size(); ++j)
        if (planes[j].size() != planes[0].size() || !sameContext(planes[j].context(), planes[0].context()))
            throw std::invalid_argument("certFHE::UIntBatch::fromPlanes: planes differ in count or context");
    return UIntBatch(planes);
}

const CiphertextBatch &UIntBatch::plane(unsigned j) const
{
    if (j >= planes_.size())
        throw std::out_of_range("certFHE::UIntBatch::plane");
    return planes_[j];
}

UIntBatch UIntBatch::compact() const
{
    return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return planes_[j].compact(); }));
}

namespace {
// every plane uniform: one csgn_gather_planes launch (d_idx nullptr: the tile form) into fresh uniform planes
std::vector<CiphertextBatch> gatherUniformPlanes(const std::vector<CiphertextBatch> &planes, uint64_t count_out,
                                                 const uint64_t *d_idx)
{
    const Context &ctx = planes[0].context();
    const Planes in(planes);
    std::vector<CiphertextBatch> out = makePlanes(ctx, count_out, in.terms);
    if (count_out)
        detail::check(csgn_gather_planes(ctx.getN(), planes.size(), sources(in).data(), in.terms.data(), planes[0].size(),
                                         count_out, d_idx, wordsOf(out).data(), detail::stream()),
                      "csgn_gather_planes");
    return out;
}

bool allUniform(const std::vector<CiphertextBatch> &planes)
{
    for (size_t j = 0; j < planes.size(); ++j)
        if (!planes[j].uniform())
            return false;
    return true;
}
} // namespace

UIntBatch UIntBatch::gather(const std::vector<uint64_t> &indices) const
{
    for (size_t e = 0; e < indices.size(); ++e)
        if (indices[e] >= size())
            throw std::out_of_range("certFHE::UIntBatch::gather: index " + std::to_string(indices[e]) +
                                    " past a batch of " + std::to_string(size()));
    if (!allUniform(planes_))
        return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return planes_[j].gather(indices); }));
    if (indices.empty())
        return UIntBatch(gatherUniformPlanes(planes_, 0, nullptr));
    std::shared_ptr<detail::DevicePayload> d_idx = detail::uploadWords(indices.data(), indices.size());
    return UIntBatch(gatherUniformPlanes(planes_, indices.size(), d_idx->data()));
}

UIntBatch UIntBatch::slice(uint64_t begin, uint64_t end) const
{
    if (begin > end || end > size())
        throw std::out_of_range("certFHE::UIntBatch::slice: [" + std::to_string(begin) + ", " + std::to_string(end) +
                                ") of a batch of " + std::to_string(size()));
    return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return planes_[j].slice(begin, end); }));
}

UIntBatch UIntBatch::broadcast(uint64_t count) const
{
    if (size() != 1)
        throw std::invalid_argument("certFHE::UIntBatch::broadcast: the batch holds " + std::to_string(size()) +
                                    " integers, not 1");
    if (count >= (1ull << 32))
        throw std::invalid_argument("certFHE::UIntBatch::broadcast: 2^32 integers or more");
    if (!allUniform(planes_))
        return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return planes_[j].broadcast(count); }));
    return UIntBatch(gatherUniformPlanes(planes_, count, nullptr));
}

UIntBatch UIntBatch::concat(const std::vector<UIntBatch> &parts)
{
    if (parts.empty())
        throw std::invalid_argument("certFHE::UIntBatch::concat: no parts");
    for (size_t k = 1; k < parts.size(); ++k)
        if (parts[k].width() != parts[0].width() || !sameContext(parts[k].context(), parts[0].context()))
            throw std::invalid_argument("certFHE::UIntBatch::concat: parts differ in width or context");
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < parts[0].width(); ++j) {
        std::vector<CiphertextBatch> pieces;
        for (size_t k = 0; k < parts.size(); ++k)
            pieces.push_back(parts[k].planes_[j]);
        planes.push_back(CiphertextBatch::concat(pieces));
    }
    return UIntBatch(planes);
}

namespace {
// Whether a list of one-bit batches is decrypted by one csgn_uint_decrypt or batch by batch: knob uint_decrypt_form at 0
// says batch by batch, and so does a ragged batch with an element past the call's bound for ragged planes (4096 terms,
// include/csgn_hip.h).  Left per shape (-1) the one call is taken: DESIGN 4.29.
const uint64_t kPackedRaggedBound = 4096;

bool packedCall(const std::vector<CiphertextBatch> &bits)
{
    int form = -1;
    csgn_get_tuning("uint_decrypt_form", &form);
    if (form == 0)
        return false;
    for (size_t j = 0; j < bits.size(); ++j)
        if (!bits[j].uniform() && termsOf(bits[j]) > kPackedRaggedBound)
            return false;
    return true;
}
} // namespace

std::vector<uint64_t> decryptPacked(const std::vector<CiphertextBatch> &bits, const SecretKey &key)
{
    if (bits.empty() || bits.size() > 64)
        throw std::invalid_argument("certFHE::decryptPacked: 1..64 batches");
    for (size_t j = 1; j < bits.size(); ++j)
        if (bits[j].size() != bits[0].size() || !sameContext(bits[j].context(), bits[0].context()))
            throw std::invalid_argument("certFHE::decryptPacked: batches differ in count or context");
    if (packedCall(bits))
        return BatchAccess::decryptPlanes(bits, key);
    std::vector<uint64_t> values(bits[0].size(), 0);
    for (size_t j = 0; j < bits.size(); ++j) {
        const std::vector<unsigned char> plane = bits[j].decrypt(key);
        for (size_t i = 0; i < values.size(); ++i)
            values[i] |= (uint64_t)(plane[i] & 1u) << j;
    }
    return values;
}

const char *decryptRoute(const UIntBatch &a)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < a.width(); ++j)
        planes.push_back(a.plane(j));
    return packedCall(planes) ? "call" : "planes";
}

std::vector<uint64_t> UIntBatch::decrypt(const SecretKey &key) const { return decryptPacked(planes_, key); }

UIntBatch UIntBatch::operator+(const UIntBatch &rhs) const
{
    requireSame(*this, rhs, "UIntBatch::operator+");
    return UIntBatch(certFHE::add(*this, rhs, nullptr, "operator+"));   // the helper above, not the member
}

UIntBatch UIntBatch::operator-(const UIntBatch &rhs) const
{
    requireSame(*this, rhs, "UIntBatch::operator-");
    return UIntBatch(certFHE::sub(*this, rhs, nullptr, "operator-"));
}

UIntBatch UIntBatch::add(const UIntBatch &rhs, CiphertextBatch *carry_out) const
{
    requireSame(*this, rhs, "UIntBatch::add");
    return UIntBatch(certFHE::add(*this, rhs, carry_out, "UIntBatch::add"));
}

UIntBatch UIntBatch::sub(const UIntBatch &rhs, CiphertextBatch *carry_out) const
{
    requireSame(*this, rhs, "UIntBatch::sub");
    return UIntBatch(certFHE::sub(*this, rhs, carry_out, "UIntBatch::sub"));
}

UIntBatch UIntBatch::operator+(uint64_t k) const { return UIntBatch(addPlain(*this, k, false, nullptr, "UIntBatch::operator+")); }

UIntBatch UIntBatch::add(uint64_t k, CiphertextBatch *carry_out) const
{
    return UIntBatch(addPlain(*this, k, false, carry_out, "UIntBatch::add"));
}

UIntBatch UIntBatch::operator-(uint64_t k) const
{
    requireConstant(*this, k, "UIntBatch::operator-");
    return UIntBatch(addPlain(*this, (0 - k) & maskOf(width()), false, nullptr, "UIntBatch::operator-"));
}

UIntBatch operator-(uint64_t k, const UIntBatch &a)
{
    requireConstant(a, k, "operator-");
    return UIntBatch(addPlain(a, ~k & maskOf(a.width()), true, nullptr, "operator-"));
}

UIntBatch UIntBatch::operator-() const { return UIntBatch(addPlain(*this, maskOf(width()), true, nullptr, "UIntBatch::operator-")); }

UIntBatch UIntBatch::operator~() const
{
    return UIntBatch(bitwisePlanes(
        CSGN_UINT_BITWISE_NOT, nullptr, Planes(*this), nullptr,
        [&](unsigned j) { gateTerms(CSGN_GATE_NOT, 0, termsOf(planes_[j]), 0, context(), "UIntBatch::operator~"); },
        [&](unsigned j) { return logicNot(planes_[j]); }));
}

UIntBatch UIntBatch::operator&(const UIntBatch &rhs) const
{
    requireSame(*this, rhs, "UIntBatch::operator&");
    const Planes pb(rhs);
    return UIntBatch(bitwisePlanes(
        CSGN_UINT_BITWISE_AND, nullptr, Planes(*this), &pb,
        [&](unsigned j) {
            const uint64_t ta = termsOf(planes_[j]), tb = termsOf(rhs.planes_[j]);
            checked(tb && ta > (kMaxWords / tb) ? 0 : ta * tb, context(), "UIntBatch::operator&");
        },
        [&](unsigned j) { return planes_[j] * rhs.planes_[j]; }));
}

UIntBatch UIntBatch::operator|(const UIntBatch &rhs) const
{
    requireSame(*this, rhs, "UIntBatch::operator|");
    const Planes pb(rhs);
    return UIntBatch(bitwisePlanes(
        CSGN_UINT_BITWISE_OR, nullptr, Planes(*this), &pb,
        [&](unsigned j) {
            gateTerms(CSGN_GATE_OR, 0, termsOf(planes_[j]), termsOf(rhs.planes_[j]), context(), "UIntBatch::operator|");
        },
        [&](unsigned j) { return logicOr(planes_[j], rhs.planes_[j]); }));
}

UIntBatch UIntBatch::operator^(const UIntBatch &rhs) const
{
    requireSame(*this, rhs, "UIntBatch::operator^");
    const Planes pb(rhs);
    return UIntBatch(bitwisePlanes(
        CSGN_UINT_BITWISE_XOR, nullptr, Planes(*this), &pb,
        [&](unsigned j) { checked(termsOf(planes_[j]) + termsOf(rhs.planes_[j]), context(), "UIntBatch::operator^"); },
        [&](unsigned j) { return planes_[j] + rhs.planes_[j]; }));
}

UIntBatch UIntBatch::operator&(uint64_t k) const
{
    requireConstant(*this, k, "UIntBatch::operator&");
    const CiphertextBatch zero = zeros(*this);            // one shared payload for every cleared plane
    return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return (k >> j) & 1u ? planes_[j] : zero; }));
}

UIntBatch UIntBatch::operator|(uint64_t k) const
{
    requireConstant(*this, k, "UIntBatch::operator|");
    const CiphertextBatch one = ones(planes_[0]);         // one shared payload for every set plane
    return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return (k >> j) & 1u ? one : planes_[j]; }));
}

UIntBatch UIntBatch::operator^(uint64_t k) const
{
    requireConstant(*this, k, "UIntBatch::operator^");
    // only the planes with a set bit of k are computed (one call); the others share the source's payload
    std::vector<CiphertextBatch> flip;
    std::vector<unsigned> at(width(), 0);
    for (unsigned j = 0; j < width(); ++j)
        if ((k >> j) & 1u) {
            at[j] = (unsigned)flip.size();
            flip.push_back(planes_[j]);
        }
    if (flip.empty())
        return *this;
    const std::vector<CiphertextBatch> flipped = bitwisePlanes(
        CSGN_UINT_BITWISE_NOT, nullptr, Planes(flip), nullptr,
        [&](unsigned i) { gateTerms(CSGN_GATE_NOT, 0, termsOf(flip[i]), 0, context(), "UIntBatch::operator^"); },
        [&](unsigned i) { return logicNot(flip[i]); });
    return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return (k >> j) & 1u ? flipped[at[j]] : planes_[j]; }));
}

UIntBatch UIntBatch::shiftLeft(unsigned s) const
{
    const CiphertextBatch zero = zeros(*this);            // one shared payload for every filled plane
    return UIntBatch(mapPlanes(width(), noCheck, [&](unsigned j) { return j >= s ? planes_[j - s] : zero; }));
}

UIntBatch UIntBatch::shiftRight(unsigned s) const
{
    const CiphertextBatch zero = zeros(*this);
    return UIntBatch(
        mapPlanes(width(), noCheck, [&](unsigned j) { return s < width() && j < width() - s ? planes_[j + s] : zero; }));
}

UIntBatch UIntBatch::rotateLeft(unsigned s) const
{
    const unsigned w = width();
    return UIntBatch(mapPlanes(w, noCheck, [&](unsigned j) { return planes_[(j + w - s % w) % w]; }));
}

UIntBatch UIntBatch::rotateRight(unsigned s) const { return rotateLeft(width() - s % width()); }

// ------------------------------------------------------------------ comparisons and select

const char *arithRoute(unsigned width, bool uniform_planes) { return oneCall(width, uniform_planes) ? "call" : "chain"; }

CiphertextBatch equalTo(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "equalTo");
    return equalToUnchecked(a, b, equalToTerms(a, b, "equalTo"), false);
}

CiphertextBatch notEqualTo(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "notEqualTo");
    return equalToUnchecked(a, b, gateTerms(CSGN_GATE_NOT, 0, equalToTerms(a, b, "notEqualTo"), 0, a.context(), "notEqualTo"),
                            true);
}

CiphertextBatch lessThan(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "lessThan");
    return lessThanUnchecked(a, b, lessThanTerms(a, b, "lessThan"));
}

CiphertextBatch greaterThan(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "greaterThan");
    return lessThanUnchecked(b, a, lessThanTerms(b, a, "greaterThan"));
}

CiphertextBatch lessEqual(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "lessEqual");
    gateTerms(CSGN_GATE_NOT, 0, lessThanTerms(b, a, "lessEqual"), 0, a.context(), "lessEqual");
    return logicNot(lessThanUnchecked(b, a));
}

CiphertextBatch greaterEqual(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "greaterEqual");
    gateTerms(CSGN_GATE_NOT, 0, lessThanTerms(a, b, "greaterEqual"), 0, a.context(), "greaterEqual");
    return logicNot(lessThanUnchecked(a, b));
}

CiphertextBatch equalTo(const UIntBatch &a, uint64_t k) { return comparePlain(CSGN_UINT_PLAIN_EQ, a, k, "equalTo"); }
CiphertextBatch notEqualTo(const UIntBatch &a, uint64_t k) { return comparePlain(CSGN_UINT_PLAIN_NE, a, k, "notEqualTo"); }
CiphertextBatch lessThan(const UIntBatch &a, uint64_t k) { return comparePlain(CSGN_UINT_PLAIN_LT, a, k, "lessThan"); }
CiphertextBatch lessEqual(const UIntBatch &a, uint64_t k) { return comparePlain(CSGN_UINT_PLAIN_LE, a, k, "lessEqual"); }
CiphertextBatch greaterThan(const UIntBatch &a, uint64_t k) { return comparePlain(CSGN_UINT_PLAIN_GT, a, k, "greaterThan"); }
CiphertextBatch greaterEqual(const UIntBatch &a, uint64_t k)
{
    return comparePlain(CSGN_UINT_PLAIN_GE, a, k, "greaterEqual");
}

UIntBatch select(const CiphertextBatch &sel, const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "select");
    requireSameBit(sel, a, "select");
    const Planes pb(b);
    return UIntBatch::fromPlanes(bitwisePlanes(
        CSGN_UINT_BITWISE_SELECT, &sel, Planes(a), &pb,
        [&](unsigned j) {
            gateTerms(CSGN_GATE_MUX, termsOf(sel), termsOf(a.plane(j)), termsOf(b.plane(j)), a.context(), "select");
        },
        [&](unsigned j) { return logicMux(sel, a.plane(j), b.plane(j)); }));
}

UIntBatch keepWhere(const CiphertextBatch &mask, const UIntBatch &a)
{
    requireSameBit(mask, a, "keepWhere");
    if (a.size() == 0)
        return UIntBatch::fromPlanes(std::vector<CiphertextBatch>(a.width(), BatchAccess::make(a.context(), 0, 1)));
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < a.width(); ++j)
        planes.push_back(a.plane(j));
    return UIntBatch::fromPlanes(keepPlanes(mask, planes, "keepWhere"));
}

const char *bitwiseRoute(int op, uint64_t sel_terms, const std::vector<uint64_t> &a_terms, const std::vector<uint64_t> &b_terms,
                         bool uniform_planes)
{
    return bitwiseCall(op, sel_terms, a_terms, b_terms, uniform_planes) ? "call" : "planes";
}

// ------------------------------------------------------------------ a public constant where an encrypted flag is set

namespace {

// Whether addWhere is one csgn_uint_add_where call or the loop below: a ragged mask or plane and integers wider than 32
// bits take the loop.  Knob uint_add_where_form decides for the rest when it is forced (0 the loop, 1 the call); per
// shape (measured): the call, but for the class addWhereLoses names.
bool addWhereCall(unsigned width, bool uniform)
{
    if (width > 32 || !uniform)
        return false;
    int form = -1;
    csgn_get_tuning("uint_add_where_form", &form);
    return form != 0;
}

// The shape class the one launch lost to the loop's launches (0.60 and 0.62 of the loop's speed at 32 and
// 16 fresh planes, k = 1, 0.7 and 1.4 GB of outputs; level at 8 planes): one-term planes and flag, ONE set bit in k with 16
// planes or more above it -- every entry a long prefix product, two terms written for every term staged -- and outputs
// of 256 MiB or more, where the loop is no longer bound by its launches.  Only where the knob leaves the choice open.
bool addWhereLoses(const std::vector<uint64_t> &ta, uint64_t ts, uint64_t k, uint64_t count, const Context &ctx)
{
    int form = -1;
    csgn_get_tuning("uint_add_where_form", &form);
    const unsigned w = (unsigned)ta.size();
    if (form != -1 || ts != 1 || (k & (k - 1)) != 0 || w - (unsigned)__builtin_ctzll(k) < 16)
        return false;
    for (unsigned j = 0; j < w; ++j)
        if (ta[j] != 1)
            return false;
    return count * (2 * (uint64_t)w + 1) * ctx.getDefaultN() * 8 >= (256ull << 20);
}

// the planes of a + (mask ? k : 0) (csgn_uint_add_where's definition); *carry_out = the last carry
std::vector<CiphertextBatch> addWherePlanes(const CiphertextBatch &mask, const UIntBatch &a, uint64_t k,
                                            CiphertextBatch *carry_out, const char *who)
{
    requireSameBit(mask, a, who);
    requireConstant(a, k, who);
    const unsigned w = a.width();
    const Context &ctx = a.context();
    if (a.size() == 0) {
        if (carry_out)
            *carry_out = BatchAccess::make(ctx, 0, 1);
        return std::vector<CiphertextBatch>(w, BatchAccess::make(ctx, 0, 1));
    }
    std::vector<CiphertextBatch> out;
    if (k == 0) {                                         // the source payloads themselves
        for (unsigned j = 0; j < w; ++j)
            out.push_back(a.plane(j));
        if (carry_out)
            *carry_out = zeros(a);
        return out;
    }
    // every size first: T_j = ta_j + tn_j + C_{j-1}, C_j = ta_j * tn_j + (ta_j + tn_j) * C_{j-1}, each held at 2^31, past
    // which `checked` refuses it (the products of two such counts fit 64 bits)
    const Planes in(a);
    const uint64_t ts = termsOf(mask);
    const auto sat = [](uint64_t x) { return x < kMaxWords ? x : kMaxWords; };
    std::vector<uint64_t> T(w);
    uint64_t c = 0;
    for (unsigned j = 0; j < w; ++j) {
        const uint64_t ta = sat(in.terms[j]), tn = ((k >> j) & 1u) ? sat(ts) : 0, ab = sat(ta + tn);
        T[j] = checked(sat(ab + c), ctx, who);
        if (j + 1 < w || carry_out)
            c = sat(sat(ta * tn) + sat(ab * c));
    }
    if (carry_out)
        checked(c, ctx, who);
    if (addWhereCall(w, in.uniform && mask.uniform()) && !addWhereLoses(in.terms, ts, k, a.size(), ctx)) {
        out = makePlanes(ctx, a.size(), T);
        CiphertextBatch carry = BatchAccess::make(ctx, carry_out ? a.size() : 0, carry_out ? c : 1);
        detail::check(csgn_uint_add_where(ctx.getN(), a.size(), w, k, mask.deviceValues(), ts, sources(in).data(),
                                          in.terms.data(), wordsOf(out).data(),
                                          carry_out ? BatchAccess::words(carry) : nullptr, detail::stream()),
                      "csgn_uint_add_where");
        if (carry_out)
            *carry_out = carry;
        return out;
    }
    // the loop: the definition itself through the batch operators
    const unsigned m = (unsigned)__builtin_ctzll(k);
    CiphertextBatch carry = mask;                         // c_{j-1}, from plane m on
    for (unsigned j = 0; j < w; ++j) {
        const CiphertextBatch &aj = a.plane(j);
        const bool more = j + 1 < w || carry_out;
        if (j < m) {
            out.push_back(aj);
        } else if (j == m) {
            out.push_back(aj + mask);
            if (more)
                carry = aj * mask;
        } else if ((k >> j) & 1u) {
            const CiphertextBatch ab = aj + mask;
            out.push_back(ab + carry);
            if (more)
                carry = (aj * mask) + (ab * carry);
        } else {
            out.push_back(aj + carry);
            if (more)
                carry = aj * carry;
        }
    }
    if (carry_out)
        *carry_out = carry;
    return out;
}

} // namespace

UIntBatch addWhere(const CiphertextBatch &mask, const UIntBatch &a, uint64_t k, CiphertextBatch *carry_out)
{
    return UIntBatch::fromPlanes(addWherePlanes(mask, a, k, carry_out, "addWhere"));
}

UIntBatch subWhere(const CiphertextBatch &mask, const UIntBatch &a, uint64_t k)
{
    requireConstant(a, k, "subWhere");
    return UIntBatch::fromPlanes(addWherePlanes(mask, a, (0 - k) & maskOf(a.width()), nullptr, "subWhere"));
}

UIntBatch incrementWhere(const CiphertextBatch &mask, const UIntBatch &a, CiphertextBatch *carry_out)
{
    return UIntBatch::fromPlanes(addWherePlanes(mask, a, 1, carry_out, "incrementWhere"));
}

UIntBatch decrementWhere(const CiphertextBatch &mask, const UIntBatch &a)
{
    return UIntBatch::fromPlanes(addWherePlanes(mask, a, maskOf(a.width()), nullptr, "decrementWhere"));
}

const char *addWhereRoute(unsigned width, bool uniform_operands) { return addWhereCall(width, uniform_operands) ? "call" : "loop"; }

const char *addWhereRoute(const CiphertextBatch &mask, const UIntBatch &a, uint64_t k)
{
    const Planes in(a);
    return k != 0 && a.size() != 0 && addWhereCall(a.width(), in.uniform && mask.uniform()) &&
                   !addWhereLoses(in.terms, termsOf(mask), k, a.size(), a.context())
               ? "call"
               : "loop";
}

// ------------------------------------------------------------------ public linear maps over F2 (csgn_uint_linear)

namespace {

void requireMatrixWidth(unsigned w, const char *who)
{
    if (w < 1 || w > 64)
        throw std::invalid_argument(std::string("certFHE::F2Matrix::") + who + ": width must be 1..64");
}

void requireMatrixConstant(unsigned w, uint64_t k, const char *who)
{
    requireMatrixWidth(w, who);
    if (w < 64 && (k >> w))
        throw std::invalid_argument(std::string("certFHE::F2Matrix::") + who + ": the constant does not fit in the width");
}

uint64_t lowBits(unsigned w) { return w >= 64 ? ~0ull : (1ull << w) - 1; }

// rows[j] = the mask of the input bits i with source(j) == i, for the maps that move bits (-1: none)
template <typename Source>
std::vector<uint64_t> movedRows(unsigned w, Source source)
{
    std::vector<uint64_t> rows(w, 0);
    for (unsigned j = 0; j < w; ++j) {
        const int i = source(j);
        if (i >= 0)
            rows[j] = 1ull << i;
    }
    return rows;
}

} // namespace

F2Matrix F2Matrix::fromRows(const std::vector<uint64_t> &rows, unsigned in_width)
{
    requireMatrixWidth(in_width, "fromRows");
    requireMatrixWidth((unsigned)(rows.size() > 64 ? 65 : rows.size()), "fromRows");
    for (size_t j = 0; j < rows.size(); ++j)
        if (rows[j] & ~lowBits(in_width))
            throw std::invalid_argument("certFHE::F2Matrix::fromRows: a row names a bit at or above the input width");
    return F2Matrix(rows, in_width);
}

F2Matrix F2Matrix::identity(unsigned w)
{
    requireMatrixWidth(w, "identity");
    return F2Matrix(movedRows(w, [](unsigned j) { return (int)j; }), w);
}

F2Matrix F2Matrix::shiftLeft(unsigned w, unsigned s)
{
    requireMatrixWidth(w, "shiftLeft");
    return F2Matrix(movedRows(w, [&](unsigned j) { return j >= s ? (int)(j - s) : -1; }), w);
}

F2Matrix F2Matrix::shiftRight(unsigned w, unsigned s)
{
    requireMatrixWidth(w, "shiftRight");
    return F2Matrix(movedRows(w, [&](unsigned j) { return s < w && j < w - s ? (int)(j + s) : -1; }), w);
}

F2Matrix F2Matrix::rotateLeft(unsigned w, unsigned s)
{
    requireMatrixWidth(w, "rotateLeft");
    return F2Matrix(movedRows(w, [&](unsigned j) { return (int)((j + w - s % w) % w); }), w);
}

F2Matrix F2Matrix::rotateRight(unsigned w, unsigned s)
{
    requireMatrixWidth(w, "rotateRight");
    return rotateLeft(w, w - s % w);
}

F2Matrix F2Matrix::mask(unsigned w, uint64_t k)
{
    requireMatrixConstant(w, k, "mask");
    return F2Matrix(movedRows(w, [&](unsigned j) { return (k >> j) & 1u ? (int)j : -1; }), w);
}

F2Matrix F2Matrix::clmul(unsigned w, uint64_t k)
{
    requireMatrixConstant(w, k, "clmul");
    std::vector<uint64_t> rows(w, 0);
    for (unsigned j = 0; j < w; ++j)
        for (unsigned i = 0; i <= j; ++i)                 // bit j of the product: the XOR of x_{j-i} over the set k_i
            if ((k >> i) & 1u)
                rows[j] |= 1ull << (j - i);
    return F2Matrix(rows, w);
}

F2Matrix F2Matrix::gfMul(unsigned w, uint64_t k, uint64_t poly)
{
    requireMatrixConstant(w, k, "gfMul");
    if (w < 64 && (poly >> w) > 1)
        throw std::invalid_argument("certFHE::F2Matrix::gfMul: the polynomial has a term above X^w");
    const uint64_t low = poly & lowBits(w);
    std::vector<uint64_t> rows(w, 0);
    uint64_t c = k;                                       // k * X^i mod poly: column i
    for (unsigned i = 0; i < w; ++i) {
        for (unsigned j = 0; j < w; ++j)
            if ((c >> j) & 1u)
                rows[j] |= 1ull << i;
        const bool carry = (c >> (w - 1)) & 1u;
        c = (c << 1) & lowBits(w);
        if (carry)
            c ^= low;
    }
    return F2Matrix(rows, w);
}

F2Matrix F2Matrix::gfSquare(unsigned w, uint64_t poly)
{
    requireMatrixWidth(w, "gfSquare");
    if (w < 64 && (poly >> w) > 1)
        throw std::invalid_argument("certFHE::F2Matrix::gfSquare: the polynomial has a term above X^w");
    const uint64_t low = poly & lowBits(w);
    std::vector<uint64_t> rows(w, 0);
    uint64_t c = 1;                                       // X^(2i) mod poly: column i, since (sum x_i X^i)^2 = sum x_i X^(2i)
    for (unsigned i = 0; i < w; ++i) {
        for (unsigned j = 0; j < w; ++j)
            if ((c >> j) & 1u)
                rows[j] |= 1ull << i;
        for (int twice = 0; twice < 2; ++twice) {
            const bool carry = (c >> (w - 1)) & 1u;
            c = (c << 1) & lowBits(w);
            if (carry)
                c ^= low;
        }
    }
    return F2Matrix(rows, w);
}

F2Matrix F2Matrix::grayEncode(unsigned w)
{
    requireMatrixWidth(w, "grayEncode");
    return identity(w) ^ shiftRight(w, 1);
}

F2Matrix F2Matrix::grayDecode(unsigned w)
{
    requireMatrixWidth(w, "grayDecode");
    std::vector<uint64_t> rows(w);
    for (unsigned j = 0; j < w; ++j)
        rows[j] = lowBits(w) & ~lowBits(j);
    return F2Matrix(rows, w);
}

uint64_t F2Matrix::apply(uint64_t x) const
{
    uint64_t y = 0;
    for (size_t j = 0; j < rows_.size(); ++j)
        y |= (uint64_t)(__builtin_popcountll(rows_[j] & x) & 1) << j;
    return y;
}

F2Matrix F2Matrix::operator^(const F2Matrix &rhs) const
{
    if (in_ != rhs.in_ || rows_.size() != rhs.rows_.size())
        throw std::invalid_argument("certFHE::F2Matrix::operator^: the maps differ in shape");
    std::vector<uint64_t> rows(rows_);
    for (size_t j = 0; j < rows.size(); ++j)
        rows[j] ^= rhs.rows_[j];
    return F2Matrix(rows, in_);
}

F2Matrix F2Matrix::operator*(const F2Matrix &rhs) const
{
    if (in_ != rhs.outWidth())
        throw std::invalid_argument("certFHE::F2Matrix::operator*: the left map's input width is not the right map's output width");
    std::vector<uint64_t> rows(rows_.size(), 0);
    for (size_t j = 0; j < rows.size(); ++j)
        for (unsigned i = 0; i < in_; ++i)
            if ((rows_[j] >> i) & 1u)
                rows[j] ^= rhs.rows_[i];                  // a bit both branches contribute cancels here
    return F2Matrix(rows, rhs.in_);
}

namespace {

// what linearMap does with row j: the constant batch, the source plane's own payload, or a computed plane
enum { LINEAR_CONSTANT, LINEAR_SHARED, LINEAR_COMPUTED };

int linearKind(uint64_t row, bool one)
{
    if (row == 0)
        return LINEAR_CONSTANT;
    return (row & (row - 1)) == 0 && !one ? LINEAR_SHARED : LINEAR_COMPUTED;
}

void requireLinear(const UIntBatch &a, const F2Matrix &m, uint64_t constant, const char *who)
{
    if (a.width() != m.inWidth())
        throw std::invalid_argument(std::string("certFHE::") + who + ": the integer's width is not the map's input width");
    if (m.outWidth() < 64 && (constant >> m.outWidth()))
        throw std::invalid_argument(std::string("certFHE::") + who + ": the constant does not fit in the map's output width");
}

bool linearComputes(const F2Matrix &m, uint64_t constant)
{
    for (unsigned j = 0; j < m.outWidth(); ++j)
        if (linearKind(m.rows()[j], (constant >> j) & 1u) == LINEAR_COMPUTED)
            return true;
    return false;
}

} // namespace

UIntBatch linearMap(const UIntBatch &a, const F2Matrix &m, uint64_t constant)
{
    requireLinear(a, m, constant, "linearMap");
    const unsigned w = a.width(), mw = m.outWidth();
    const Context &ctx = a.context();
    if (a.size() == 0)
        return UIntBatch::fromPlanes(std::vector<CiphertextBatch>(mw, BatchAccess::make(ctx, 0, 1)));
    // every size first
    const Planes in(a);
    std::vector<uint64_t> rows, T;                        // the computed rows, their counts
    std::vector<unsigned> at(mw, 0);
    uint64_t ones_of = 0;                                 // their constant bits
    for (unsigned j = 0; j < mw; ++j) {
        const uint64_t row = m.rows()[j];
        const bool one = (constant >> j) & 1u;
        if (linearKind(row, one) != LINEAR_COMPUTED)
            continue;
        at[j] = (unsigned)rows.size();
        ones_of |= (uint64_t)one << rows.size();
        rows.push_back(row);
        T.push_back(checked(csgn_uint_linear_terms(w, in.terms.data(), row, one ? 1 : 0), ctx, "linearMap"));
    }
    std::vector<CiphertextBatch> computed;
    if (!rows.empty() && in.uniform) {
        computed = makePlanes(ctx, a.size(), T);
        detail::check(csgn_uint_linear(ctx.getN(), a.size(), w, sources(in).data(), in.terms.data(), rows.size(),
                                       rows.data(), ones_of, wordsOf(computed).data(), detail::stream()),
                      "csgn_uint_linear");
    } else if (!rows.empty()) {                           // the loop: the definition through the batch operators
        const CiphertextBatch one = ones(a.plane(0));
        for (size_t r = 0; r < rows.size(); ++r) {
            unsigned i = (unsigned)__builtin_ctzll(rows[r]);
            CiphertextBatch sum = a.plane(i);
            for (++i; i < w; ++i)
                if ((rows[r] >> i) & 1u)
                    sum = sum + a.plane(i);
            computed.push_back((ones_of >> r) & 1u ? sum + one : sum);
        }
    }
    std::vector<CiphertextBatch> out;
    bool have_zero = false, have_one = false;
    CiphertextBatch zero = a.plane(0), one = a.plane(0);  // one shared payload for every constant plane of a kind
    for (unsigned j = 0; j < mw; ++j) {
        const uint64_t row = m.rows()[j];
        const bool bit = (constant >> j) & 1u;
        switch (linearKind(row, bit)) {
        case LINEAR_SHARED: out.push_back(a.plane((unsigned)__builtin_ctzll(row))); break;
        case LINEAR_COMPUTED: out.push_back(computed[at[j]]); break;
        default:
            if (bit && !have_one) {
                one = ones(a.plane(0));
                have_one = true;
            } else if (!bit && !have_zero) {
                zero = zeros(a);
                have_zero = true;
            }
            out.push_back(bit ? one : zero);
        }
    }
    return UIntBatch::fromPlanes(out);
}

CiphertextBatch parity(const UIntBatch &a, uint64_t mask)
{
    requireConstant(a, mask, "parity");
    return linearMap(a, F2Matrix::fromRows(std::vector<uint64_t>(1, mask), a.width())).plane(0);
}

const char *linearRoute(const UIntBatch &a, const F2Matrix &m, uint64_t constant)
{
    requireLinear(a, m, constant, "linearRoute");
    return a.size() != 0 && Planes(a).uniform && linearComputes(m, constant) ? "call" : "loop";
}

// ------------------------------------------------------------------ public bilinear forms over F2 (csgn_uint_bilinear)

namespace {

typedef F2Bilinear::Pair BilinearPair;
typedef std::vector<std::vector<BilinearPair> > BilinearRows;

void requireFormWidth(unsigned w, const char *who)
{
    if (w < 1 || w > 64)
        throw std::invalid_argument(std::string("certFHE::F2Bilinear::") + who + ": width must be 1..64");
}

// the pairs named an odd number of times, sorted by (left, right)
std::vector<BilinearPair> cancelPairs(std::vector<BilinearPair> pairs)
{
    std::sort(pairs.begin(), pairs.end());
    std::vector<BilinearPair> kept;
    for (size_t i = 0; i < pairs.size();) {
        size_t j = i;
        while (j < pairs.size() && pairs[j] == pairs[i])
            ++j;
        if ((j - i) & 1u)
            kept.push_back(pairs[i]);
        i = j;
    }
    return kept;
}

} // namespace

F2Bilinear F2Bilinear::fromPairs(const BilinearRows &rows, unsigned left_width, unsigned right_width)
{
    requireFormWidth(left_width, "fromPairs");
    requireFormWidth(right_width, "fromPairs");
    requireFormWidth((unsigned)(rows.size() > 64 ? 65 : rows.size()), "fromPairs");
    BilinearRows kept;
    for (size_t j = 0; j < rows.size(); ++j) {
        for (size_t i = 0; i < rows[j].size(); ++i)
            if (rows[j][i].first >= left_width || rows[j][i].second >= right_width)
                throw std::invalid_argument("certFHE::F2Bilinear::fromPairs: a pair names a bit at or above its width");
        kept.push_back(cancelPairs(rows[j]));
    }
    return F2Bilinear(kept, left_width, right_width);
}

F2Bilinear F2Bilinear::clmulWide(unsigned w)
{
    requireFormWidth(w, "clmulWide");
    if (w > 32)
        throw std::invalid_argument("certFHE::F2Bilinear::clmulWide: the product of a width above 32 has more than 64 planes");
    BilinearRows rows(2 * w - 1);
    for (unsigned i = 0; i < w; ++i)                      // ascending (i, l) in every row
        for (unsigned l = 0; l < w; ++l)
            rows[i + l].push_back(BilinearPair(i, l));
    return F2Bilinear(rows, w, w);
}

F2Bilinear F2Bilinear::clmul(unsigned w)
{
    requireFormWidth(w, "clmul");
    BilinearRows rows(w);
    for (unsigned i = 0; i < w; ++i)
        for (unsigned l = 0; i + l < w; ++l)
            rows[i + l].push_back(BilinearPair(i, l));
    return F2Bilinear(rows, w, w);
}

F2Bilinear F2Bilinear::gfMul(unsigned w, uint64_t poly)
{
    requireFormWidth(w, "gfMul");
    if (w < 64 && (poly >> w) > 1)
        throw std::invalid_argument("certFHE::F2Bilinear::gfMul: the polynomial has a term above X^w");
    const uint64_t low = poly & lowBits(w);
    std::vector<uint64_t> red(2 * w - 1);                 // X^k mod poly
    uint64_t c = 1;
    for (unsigned k = 0; k < 2 * w - 1; ++k) {
        red[k] = c;
        const bool carry = (c >> (w - 1)) & 1u;
        c = (c << 1) & lowBits(w);
        if (carry)
            c ^= low;
    }
    BilinearRows rows(w);
    for (unsigned i = 0; i < w; ++i)
        for (unsigned l = 0; l < w; ++l)
            for (unsigned j = 0; j < w; ++j)
                if ((red[i + l] >> j) & 1u)
                    rows[j].push_back(BilinearPair(i, l));
    return F2Bilinear(rows, w, w);
}

F2Bilinear F2Bilinear::bitwiseAnd(unsigned w)
{
    requireFormWidth(w, "bitwiseAnd");
    BilinearRows rows(w);
    for (unsigned j = 0; j < w; ++j)
        rows[j].push_back(BilinearPair(j, j));
    return F2Bilinear(rows, w, w);
}

F2Bilinear F2Bilinear::dotBits(unsigned w)
{
    requireFormWidth(w, "dotBits");
    BilinearRows rows(1);
    for (unsigned j = 0; j < w; ++j)
        rows[0].push_back(BilinearPair(j, j));
    return F2Bilinear(rows, w, w);
}

uint64_t F2Bilinear::apply(uint64_t x, uint64_t y) const
{
    uint64_t z = 0;
    for (size_t j = 0; j < rows_.size(); ++j) {
        uint64_t bit = 0;
        for (size_t i = 0; i < rows_[j].size(); ++i)
            bit ^= (x >> rows_[j][i].first) & (y >> rows_[j][i].second) & 1u;
        z |= bit << j;
    }
    return z;
}

F2Bilinear F2Bilinear::operator^(const F2Bilinear &rhs) const
{
    if (left_ != rhs.left_ || right_ != rhs.right_ || rows_.size() != rhs.rows_.size())
        throw std::invalid_argument("certFHE::F2Bilinear::operator^: the forms differ in shape");
    BilinearRows rows(rows_);
    for (size_t j = 0; j < rows.size(); ++j) {
        rows[j].insert(rows[j].end(), rhs.rows_[j].begin(), rhs.rows_[j].end());
        rows[j] = cancelPairs(rows[j]);                   // a pair both forms contribute cancels here
    }
    return F2Bilinear(rows, left_, right_);
}

F2Bilinear F2Bilinear::compose(const F2Matrix &on_a, const F2Matrix &on_b) const
{
    if (on_a.outWidth() != left_ || on_b.outWidth() != right_)
        throw std::invalid_argument("certFHE::F2Bilinear::compose: a map's output width is not the form's width");
    BilinearRows rows(rows_.size());
    for (size_t j = 0; j < rows.size(); ++j) {
        for (size_t p = 0; p < rows_[j].size(); ++p) {
            const uint64_t ma = on_a.rows()[rows_[j][p].first], mb = on_b.rows()[rows_[j][p].second];
            for (unsigned i = 0; i < on_a.inWidth(); ++i)
                if ((ma >> i) & 1u)
                    for (unsigned l = 0; l < on_b.inWidth(); ++l)
                        if ((mb >> l) & 1u)
                            rows[j].push_back(BilinearPair(i, l));
        }
        rows[j] = cancelPairs(rows[j]);
    }
    return F2Bilinear(rows, on_a.inWidth(), on_b.inWidth());
}

F2Bilinear operator*(const F2Matrix &m, const F2Bilinear &form)
{
    if (m.inWidth() != form.outWidth())
        throw std::invalid_argument("certFHE::operator*: the map's input width is not the form's output width");
    BilinearRows rows(m.outWidth());
    for (size_t j = 0; j < rows.size(); ++j) {
        for (unsigned x = 0; x < m.inWidth(); ++x)
            if ((m.rows()[j] >> x) & 1u)
                rows[j].insert(rows[j].end(), form.rows()[x].begin(), form.rows()[x].end());
    }
    return F2Bilinear::fromPairs(rows, form.leftWidth(), form.rightWidth());
}

namespace {

// device plans per (terms, rows, constant), kept until the process ends
const csgn_uint_bilinear_plan *bilinearPlan(const std::vector<uint64_t> &ta, const std::vector<uint64_t> &tb,
                                            const std::vector<uint64_t> &first, const std::vector<uint64_t> &left,
                                            const std::vector<uint64_t> &right, uint64_t constant)
{
    static std::mutex mutex;
    static std::map<std::vector<uint64_t>, csgn_uint_bilinear_plan *> *plans =
        new std::map<std::vector<uint64_t>, csgn_uint_bilinear_plan *>();
    std::vector<uint64_t> key(1, constant);
    key.push_back(ta.size());
    key.push_back(tb.size());
    key.insert(key.end(), ta.begin(), ta.end());
    key.insert(key.end(), tb.begin(), tb.end());
    key.insert(key.end(), first.begin(), first.end());
    key.insert(key.end(), left.begin(), left.end());
    key.insert(key.end(), right.begin(), right.end());
    std::lock_guard<std::mutex> lock(mutex);
    auto it = plans->find(key);
    if (it != plans->end())
        return it->second;
    csgn_uint_bilinear_plan *p = nullptr;
    detail::check(csgn_uint_bilinear_create(ta.size(), ta.data(), tb.size(), tb.data(), first.size() - 1, first.data(),
                                            left.data(), right.data(), constant, &p),
                  "csgn_uint_bilinear_create");
    (*plans)[key] = p;
    return p;
}

void requireBilinear(const UIntBatch &a, const UIntBatch &b, const F2Bilinear &form, uint64_t constant, const char *who)
{
    if (a.width() != form.leftWidth() || b.width() != form.rightWidth())
        throw std::invalid_argument(std::string("certFHE::") + who + ": an integer's width is not the form's");
    if (a.size() != b.size() || !sameContext(a.context(), b.context()))
        throw std::invalid_argument(std::string("certFHE::") + who + ": operands differ in count or context");
    if (form.outWidth() < 64 && (constant >> form.outWidth()))
        throw std::invalid_argument(std::string("certFHE::") + who + ": the constant does not fit in the form's output width");
}

unsigned requireOneWidth(const UIntBatch &a, const UIntBatch &b, const char *who)
{
    if (a.width() != b.width())
        throw std::invalid_argument(std::string("certFHE::") + who + ": operands differ in width");
    return a.width();
}

} // namespace

UIntBatch bilinearMap(const UIntBatch &a, const UIntBatch &b, const F2Bilinear &form, uint64_t constant)
{
    requireBilinear(a, b, form, constant, "bilinearMap");
    const unsigned m = form.outWidth();
    const Context &ctx = a.context();
    // every size first
    const Planes pa(a), pb(b);
    std::vector<uint64_t> first(1, 0), left, right, T;
    for (unsigned x = 0; x < m; ++x) {
        const std::vector<F2Bilinear::Pair> &row = form.rows()[x];
        for (size_t i = 0; i < row.size(); ++i) {
            left.push_back(row[i].first);
            right.push_back(row[i].second);
        }
        T.push_back(checked(csgn_uint_bilinear_terms(pa.terms.size(), pa.terms.data(), pb.terms.size(), pb.terms.data(),
                                                     row.size(), left.data() + first.back(), right.data() + first.back(),
                                                     (int)((constant >> x) & 1u)),
                            ctx, "bilinearMap"));
        first.push_back(left.size());
    }
    if (a.size() == 0)
        return UIntBatch::fromPlanes(std::vector<CiphertextBatch>(m, BatchAccess::make(ctx, 0, 1)));
    if (pa.uniform && pb.uniform) {
        if (left.empty()) {                               // csgn_uint_bilinear_create reads no entry array then
            left.push_back(0);
            right.push_back(0);
        }
        const csgn_uint_bilinear_plan *plan = bilinearPlan(pa.terms, pb.terms, first, left, right, constant);
        std::vector<CiphertextBatch> out = makePlanes(ctx, a.size(), T);
        detail::check(csgn_uint_bilinear(plan, ctx.getN(), a.size(), sources(pa).data(), sources(pb).data(),
                                         wordsOf(out).data(), detail::stream()),
                      "csgn_uint_bilinear");
        return UIntBatch::fromPlanes(out);
    }
    // the loop: each integer's planes in one batch (plane i's element e at i * count + e), then per output plane the
    // named operand planes gathered pair by pair, ONE element-wise product, and sumGroups, which copies nothing
    const uint64_t count = a.size();
    std::vector<CiphertextBatch> parts_a, parts_b;
    for (unsigned i = 0; i < a.width(); ++i)
        parts_a.push_back(a.plane(i));
    for (unsigned l = 0; l < b.width(); ++l)
        parts_b.push_back(b.plane(l));
    const CiphertextBatch all_a = CiphertextBatch::concat(parts_a), all_b = CiphertextBatch::concat(parts_b);
    std::vector<CiphertextBatch> out;
    for (unsigned x = 0; x < m; ++x) {
        const std::vector<F2Bilinear::Pair> &row = form.rows()[x];
        const bool one = (constant >> x) & 1u;
        if (row.empty()) {
            out.push_back(one ? ones(a.plane(0)) : zeros(a));
            continue;
        }
        std::vector<uint64_t> li, ri;
        li.reserve(count * row.size());
        ri.reserve(count * row.size());
        for (uint64_t e = 0; e < count; ++e)
            for (size_t i = 0; i < row.size(); ++i) {
                li.push_back(row[i].first * count + e);
                ri.push_back(row[i].second * count + e);
            }
        const CiphertextBatch sum = (all_a.gather(li) * all_b.gather(ri)).sumGroups(row.size());
        out.push_back(one ? sum + ones(a.plane(0)) : sum);
    }
    return UIntBatch::fromPlanes(out);
}

UIntBatch clmul(const UIntBatch &a, const UIntBatch &b)
{
    return bilinearMap(a, b, F2Bilinear::clmul(requireOneWidth(a, b, "clmul")));
}

UIntBatch clmulWide(const UIntBatch &a, const UIntBatch &b)
{
    return bilinearMap(a, b, F2Bilinear::clmulWide(requireOneWidth(a, b, "clmulWide")));
}

UIntBatch gfMul(const UIntBatch &a, const UIntBatch &b, uint64_t poly)
{
    return bilinearMap(a, b, F2Bilinear::gfMul(requireOneWidth(a, b, "gfMul"), poly));
}

CiphertextBatch dotBits(const UIntBatch &a, const UIntBatch &b)
{
    return bilinearMap(a, b, F2Bilinear::dotBits(requireOneWidth(a, b, "dotBits"))).plane(0);
}

const char *bilinearRoute(const UIntBatch &a, const UIntBatch &b, const F2Bilinear &form, uint64_t constant)
{
    requireBilinear(a, b, form, constant, "bilinearRoute");
    if (a.size() == 0)
        return "none";
    return Planes(a).uniform && Planes(b).uniform ? "k_uint_bilinear" : "loop";
}

// ------------------------------------------------------------------ public polynomial maps over F2 (csgn_uint_poly)

namespace {

typedef F2Polynomial::Monomial PolyMonomial;
typedef F2Polynomial::Rows PolyRows;

const unsigned kPolyMaxDegree = 8, kPolyMaxVariables = 256;
const size_t kPolyMaxMonomials = 262144;

// ascending by (degree, then the variables)
bool monomialLess(const PolyMonomial &x, const PolyMonomial &y)
{
    return x.size() != y.size() ? x.size() < y.size() : x < y;
}

// One row in canonical form: the variables of a monomial ascending with none twice, the monomials named an odd number
// of times ascending; an empty monomial flips *constant.  std::invalid_argument past degree 8.
std::vector<PolyMonomial> cancelMonomials(std::vector<PolyMonomial> monomials, bool *constant, const char *who)
{
    for (size_t i = 0; i < monomials.size(); ++i) {
        PolyMonomial &m = monomials[i];
        std::sort(m.begin(), m.end());
        m.erase(std::unique(m.begin(), m.end()), m.end());
        if (m.size() > kPolyMaxDegree)
            throw std::invalid_argument(std::string("certFHE::F2Polynomial::") + who + ": a monomial of degree above 8");
    }
    std::sort(monomials.begin(), monomials.end(), monomialLess);
    std::vector<PolyMonomial> kept;
    for (size_t i = 0; i < monomials.size();) {
        size_t j = i;
        while (j < monomials.size() && monomials[j] == monomials[i])
            ++j;
        if ((j - i) & 1u) {
            if (monomials[i].empty())
                *constant = !*constant;
            else
                kept.push_back(monomials[i]);
        }
        i = j;
    }
    return kept;
}

unsigned requirePolyWidths(const std::vector<unsigned> &widths, const char *who)
{
    unsigned total = 0;
    if (widths.empty())
        throw std::invalid_argument(std::string("certFHE::F2Polynomial::") + who + ": no operand");
    for (size_t o = 0; o < widths.size(); ++o) {
        if (widths[o] < 1 || widths[o] > 64)
            throw std::invalid_argument(std::string("certFHE::F2Polynomial::") + who + ": width must be 1..64");
        total += widths[o];
        if (total > kPolyMaxVariables)
            throw std::invalid_argument(std::string("certFHE::F2Polynomial::") + who + ": more than 256 bits of operands");
    }
    return total;
}

void requirePolyCount(const PolyRows &rows, const char *who)
{
    size_t n = 0;
    for (size_t j = 0; j < rows.size(); ++j)
        n += rows[j].size();
    if (n > kPolyMaxMonomials)
        throw std::invalid_argument(std::string("certFHE::F2Polynomial::") + who + ": more than 262144 monomials");
}

// the rows with an empty monomial added where the constant has a bit: fromMonomials folds it back
F2Polynomial polynomialOf(PolyRows rows, const std::vector<unsigned> &widths, uint64_t constant)
{
    for (size_t j = 0; j < rows.size() && j < 64; ++j)
        if ((constant >> j) & 1u)
            rows[j].push_back(PolyMonomial());
    return F2Polynomial::fromMonomials(rows, widths);
}

// variable of bit i of operand o
std::vector<unsigned> polyBases(const std::vector<unsigned> &widths)
{
    std::vector<unsigned> base(widths.size() + 1, 0);
    for (size_t o = 0; o < widths.size(); ++o)
        base[o + 1] = base[o] + widths[o];
    return base;
}

PolyMonomial monomialOf(unsigned a)
{
    return PolyMonomial(1, a);
}

PolyMonomial monomialOf(unsigned a, unsigned b)
{
    PolyMonomial m(1, a);
    m.push_back(b);
    return m;
}

void requirePolyWidth(unsigned w, const char *who)
{
    if (w < 1 || w > 64)
        throw std::invalid_argument(std::string("certFHE::F2Polynomial::") + who + ": width must be 1..64");
}

} // namespace

F2Polynomial F2Polynomial::fromMonomials(const Rows &rows, const std::vector<unsigned> &widths)
{
    const char *who = "fromMonomials";
    const unsigned variables = requirePolyWidths(widths, who);
    if (rows.size() < 1 || rows.size() > 64)
        throw std::invalid_argument("certFHE::F2Polynomial::fromMonomials: 1..64 rows");
    Rows kept;
    uint64_t constant = 0;
    for (size_t j = 0; j < rows.size(); ++j) {
        for (size_t i = 0; i < rows[j].size(); ++i)
            for (size_t k = 0; k < rows[j][i].size(); ++k)
                if (rows[j][i][k] >= variables)
                    throw std::invalid_argument(
                        "certFHE::F2Polynomial::fromMonomials: a monomial names a variable at or above the operands' bits");
        bool one = false;
        kept.push_back(cancelMonomials(rows[j], &one, who));
        constant |= (uint64_t)one << j;
    }
    requirePolyCount(kept, who);
    return F2Polynomial(kept, widths, constant);
}

F2Polynomial F2Polynomial::linear(const F2Matrix &m)
{
    Rows rows(m.outWidth());
    for (unsigned j = 0; j < m.outWidth(); ++j)
        for (unsigned i = 0; i < m.inWidth(); ++i)
            if ((m.rows()[j] >> i) & 1u)
                rows[j].push_back(monomialOf(i));
    return fromMonomials(rows, std::vector<unsigned>(1, m.inWidth()));
}

F2Polynomial F2Polynomial::bilinear(const F2Bilinear &f)
{
    Rows rows(f.outWidth());
    for (unsigned j = 0; j < f.outWidth(); ++j)
        for (size_t i = 0; i < f.rows()[j].size(); ++i)
            rows[j].push_back(monomialOf(f.rows()[j][i].first, f.leftWidth() + f.rows()[j][i].second));
    std::vector<unsigned> widths(1, f.leftWidth());
    widths.push_back(f.rightWidth());
    return fromMonomials(rows, widths);
}

F2Polynomial F2Polynomial::fromLookupTable(const LookupTable &f)
{
    const unsigned w = f.inWidth();
    Rows rows(f.outWidth());
    const std::vector<uint64_t> &anf = f.anf();
    for (uint64_t s = 0; s < anf.size(); ++s) {
        if (anf[s] == 0)
            continue;
        Monomial mono;
        for (unsigned i = 0; i < w; ++i)
            if ((s >> i) & 1u)
                mono.push_back(i);
        for (unsigned j = 0; j < f.outWidth(); ++j)
            if ((anf[s] >> j) & 1u)
                rows[j].push_back(mono);
    }
    return fromMonomials(rows, std::vector<unsigned>(1, w));
}

F2Polynomial F2Polynomial::ch(unsigned w)
{
    requirePolyWidth(w, "ch");
    Rows rows(w);
    for (unsigned j = 0; j < w; ++j) {
        rows[j].push_back(monomialOf(j, w + j));
        rows[j].push_back(monomialOf(j, 2 * w + j));
        rows[j].push_back(monomialOf(2 * w + j));
    }
    return fromMonomials(rows, std::vector<unsigned>(3, w));
}

F2Polynomial F2Polynomial::maj(unsigned w)
{
    requirePolyWidth(w, "maj");
    Rows rows(w);
    for (unsigned j = 0; j < w; ++j) {
        rows[j].push_back(monomialOf(j, w + j));
        rows[j].push_back(monomialOf(j, 2 * w + j));
        rows[j].push_back(monomialOf(w + j, 2 * w + j));
    }
    return fromMonomials(rows, std::vector<unsigned>(3, w));
}

F2Polynomial F2Polynomial::chi(unsigned w)
{
    requirePolyWidth(w, "chi");
    Rows rows(w);
    for (unsigned j = 0; j < w; ++j) {
        rows[j].push_back(monomialOf(j));
        rows[j].push_back(monomialOf(2 * w + j));
        rows[j].push_back(monomialOf(w + j, 2 * w + j));
    }
    return fromMonomials(rows, std::vector<unsigned>(3, w));
}

F2Polynomial F2Polynomial::andAll(unsigned w, unsigned k)
{
    requirePolyWidth(w, "andAll");
    if (k < 1 || k > kPolyMaxDegree)
        throw std::invalid_argument("certFHE::F2Polynomial::andAll: 1..8 operands");
    Rows rows(w);
    for (unsigned j = 0; j < w; ++j) {
        Monomial m;
        for (unsigned o = 0; o < k; ++o)
            m.push_back(o * w + j);
        rows[j].push_back(m);
    }
    return fromMonomials(rows, std::vector<unsigned>(k, w));
}

F2Polynomial F2Polynomial::mux(unsigned w)
{
    requirePolyWidth(w, "mux");
    Rows rows(w);
    for (unsigned j = 0; j < w; ++j) {
        rows[j].push_back(monomialOf(0, 1 + j));
        rows[j].push_back(monomialOf(0, 1 + w + j));
        rows[j].push_back(monomialOf(1 + w + j));
    }
    std::vector<unsigned> widths(1, 1);
    widths.push_back(w);
    widths.push_back(w);
    return fromMonomials(rows, widths);
}

unsigned F2Polynomial::variables() const
{
    unsigned total = 0;
    for (size_t o = 0; o < widths_.size(); ++o)
        total += widths_[o];
    return total;
}

uint64_t F2Polynomial::apply(const std::vector<uint64_t> &operands) const
{
    if (operands.size() != widths_.size())
        throw std::invalid_argument("certFHE::F2Polynomial::apply: the number of operands is not the form's");
    std::vector<unsigned char> bit;
    for (size_t o = 0; o < widths_.size(); ++o)
        for (unsigned i = 0; i < widths_[o]; ++i)
            bit.push_back((unsigned char)((operands[o] >> i) & 1u));
    uint64_t z = 0;
    for (size_t j = 0; j < rows_.size(); ++j) {
        uint64_t sum = 0;
        for (size_t i = 0; i < rows_[j].size(); ++i) {
            uint64_t p = 1;
            for (size_t k = 0; k < rows_[j][i].size(); ++k)
                p &= bit[rows_[j][i][k]];
            sum ^= p;
        }
        z |= sum << j;
    }
    return z ^ constant_;
}

F2Polynomial F2Polynomial::operator^(const F2Polynomial &rhs) const
{
    if (widths_ != rhs.widths_ || rows_.size() != rhs.rows_.size())
        throw std::invalid_argument("certFHE::F2Polynomial::operator^: the forms differ in shape");
    Rows rows(rows_);
    for (size_t j = 0; j < rows.size(); ++j)
        rows[j].insert(rows[j].end(), rhs.rows_[j].begin(), rhs.rows_[j].end());
    return polynomialOf(rows, widths_, constant_ ^ rhs.constant_);
}

F2Polynomial F2Polynomial::operator&(const F2Polynomial &rhs) const
{
    if (widths_ != rhs.widths_ || rows_.size() != rhs.rows_.size())
        throw std::invalid_argument("certFHE::F2Polynomial::operator&: the forms differ in shape");
    Rows rows(rows_.size());
    for (size_t j = 0; j < rows.size(); ++j) {
        std::vector<Monomial> p(rows_[j]), q(rhs.rows_[j]);
        if ((constant_ >> j) & 1u)
            p.push_back(Monomial());
        if ((rhs.constant_ >> j) & 1u)
            q.push_back(Monomial());
        if (p.size() * q.size() > 16 * kPolyMaxMonomials)
            throw std::invalid_argument("certFHE::F2Polynomial::operator&: more than 262144 monomials");
        for (size_t a = 0; a < p.size(); ++a)
            for (size_t b = 0; b < q.size(); ++b) {
                Monomial m(p[a]);
                m.insert(m.end(), q[b].begin(), q[b].end());
                rows[j].push_back(m);
            }
    }
    return fromMonomials(rows, widths_);
}

F2Polynomial F2Polynomial::compose(const std::vector<F2Matrix> &on) const
{
    if (on.size() != widths_.size())
        throw std::invalid_argument("certFHE::F2Polynomial::compose: one map per operand");
    std::vector<unsigned> widths;
    for (size_t o = 0; o < on.size(); ++o) {
        if (on[o].outWidth() != widths_[o])
            throw std::invalid_argument("certFHE::F2Polynomial::compose: a map's output width is not the operand's width");
        widths.push_back(on[o].inWidth());
    }
    requirePolyWidths(widths, "compose");
    const std::vector<unsigned> old_base = polyBases(widths_), new_base = polyBases(widths);
    std::vector<std::vector<unsigned> > image(variables());   // old variable -> the new variables it is the sum of
    for (size_t o = 0; o < on.size(); ++o)
        for (unsigned i = 0; i < widths_[o]; ++i)
            for (unsigned k = 0; k < on[o].inWidth(); ++k)
                if ((on[o].rows()[i] >> k) & 1u)
                    image[old_base[o] + i].push_back(new_base[o] + k);
    Rows rows(rows_.size());
    size_t total = 0;
    for (size_t j = 0; j < rows.size(); ++j) {
        for (size_t i = 0; i < rows_[j].size(); ++i) {
            std::vector<Monomial> acc(1, Monomial());         // the product of the factors' sums, expanded
            for (size_t k = 0; k < rows_[j][i].size(); ++k) {
                const std::vector<unsigned> &sum = image[rows_[j][i][k]];
                if (acc.size() * sum.size() > 16 * kPolyMaxMonomials)
                    throw std::invalid_argument("certFHE::F2Polynomial::compose: more than 262144 monomials");
                std::vector<Monomial> next;
                next.reserve(acc.size() * sum.size());
                for (size_t a = 0; a < acc.size(); ++a)
                    for (size_t v = 0; v < sum.size(); ++v) {
                        next.push_back(acc[a]);
                        next.back().push_back(sum[v]);
                    }
                acc.swap(next);
            }
            rows[j].insert(rows[j].end(), acc.begin(), acc.end());
            if (rows[j].size() > 16 * kPolyMaxMonomials) {    // cancel what has gathered before going on
                bool one = false;
                rows[j] = cancelMonomials(rows[j], &one, "compose");
                if (one)
                    rows[j].push_back(Monomial());
                if (rows[j].size() > kPolyMaxMonomials)
                    throw std::invalid_argument("certFHE::F2Polynomial::compose: more than 262144 monomials");
            }
        }
        bool one = false;
        rows[j] = cancelMonomials(rows[j], &one, "compose");
        if (one)
            rows[j].push_back(Monomial());
        total += rows[j].size();
        if (total > kPolyMaxMonomials)
            throw std::invalid_argument("certFHE::F2Polynomial::compose: more than 262144 monomials");
    }
    return polynomialOf(rows, widths, constant_);
}

F2Polynomial operator*(const F2Matrix &m, const F2Polynomial &form)
{
    if (m.inWidth() != form.outWidth())
        throw std::invalid_argument("certFHE::operator*: the map's input width is not the form's output width");
    PolyRows rows(m.outWidth());
    uint64_t constant = 0;
    for (size_t j = 0; j < rows.size(); ++j)
        for (unsigned x = 0; x < m.inWidth(); ++x)
            if ((m.rows()[j] >> x) & 1u) {
                rows[j].insert(rows[j].end(), form.rows()[x].begin(), form.rows()[x].end());
                constant ^= ((form.constant() >> x) & 1u) << j;
            }
    return polynomialOf(rows, form.widths(), constant);
}

namespace {

// device plans per (terms, rows, constant), kept until the process ends
const csgn_uint_poly_plan *polyPlan(const std::vector<uint64_t> &terms, const std::vector<uint64_t> &first,
                                    const std::vector<uint64_t> &mfirst, const std::vector<uint64_t> &factor,
                                    uint64_t constant)
{
    static std::mutex mutex;
    static std::map<std::vector<uint64_t>, csgn_uint_poly_plan *> *plans =
        new std::map<std::vector<uint64_t>, csgn_uint_poly_plan *>();
    std::vector<uint64_t> key(1, constant);
    key.push_back(terms.size());
    key.push_back(first.size());
    key.insert(key.end(), terms.begin(), terms.end());
    key.insert(key.end(), first.begin(), first.end());
    key.insert(key.end(), mfirst.begin(), mfirst.end());
    key.insert(key.end(), factor.begin(), factor.end());
    std::lock_guard<std::mutex> lock(mutex);
    auto it = plans->find(key);
    if (it != plans->end())
        return it->second;
    csgn_uint_poly_plan *p = nullptr;
    detail::check(csgn_uint_poly_create(terms.size(), terms.data(), first.size() - 1, first.data(), mfirst.data(),
                                        factor.data(), constant, &p),
                  "csgn_uint_poly_create");
    (*plans)[key] = p;
    return p;
}

// what polyMap does with row j: the constant batch, the source plane's own payload, or a computed plane
enum { POLY_CONSTANT, POLY_SHARED, POLY_COMPUTED };

int polyKind(const std::vector<PolyMonomial> &row, bool one)
{
    if (row.empty())
        return POLY_CONSTANT;
    return row.size() == 1 && row[0].size() == 1 && !one ? POLY_SHARED : POLY_COMPUTED;
}

// the constant of a call: the form's own XOR the caller's
uint64_t requirePoly(const std::vector<UIntBatch> &operands, const F2Polynomial &f, uint64_t constant, const char *who)
{
    if (operands.size() != f.widths().size())
        throw std::invalid_argument(std::string("certFHE::") + who + ": the number of operands is not the form's");
    for (size_t o = 0; o < operands.size(); ++o) {
        if (operands[o].width() != f.widths()[o])
            throw std::invalid_argument(std::string("certFHE::") + who + ": an integer's width is not the form's");
        if (operands[o].size() != operands[0].size() || !sameContext(operands[o].context(), operands[0].context()))
            throw std::invalid_argument(std::string("certFHE::") + who + ": operands differ in count or context");
    }
    if (f.outWidth() < 64 && (constant >> f.outWidth()))
        throw std::invalid_argument(std::string("certFHE::") + who + ": the constant does not fit in the form's output width");
    return constant ^ f.constant();
}

std::vector<CiphertextBatch> polyPlanes(const std::vector<UIntBatch> &operands)
{
    std::vector<CiphertextBatch> planes;
    for (size_t o = 0; o < operands.size(); ++o)
        for (unsigned i = 0; i < operands[o].width(); ++i)
            planes.push_back(operands[o].plane(i));
    return planes;
}

bool polyComputes(const F2Polynomial &f, uint64_t constant)
{
    for (unsigned j = 0; j < f.outWidth(); ++j)
        if (polyKind(f.rows()[j], (constant >> j) & 1u) == POLY_COMPUTED)
            return true;
    return false;
}

unsigned requireOneWidthOf(const std::vector<UIntBatch> &operands, const char *who)
{
    if (operands.empty() || operands.size() > kPolyMaxDegree)
        throw std::invalid_argument(std::string("certFHE::") + who + ": 1..8 operands");
    for (size_t o = 1; o < operands.size(); ++o)
        if (operands[o].width() != operands[0].width())
            throw std::invalid_argument(std::string("certFHE::") + who + ": operands differ in width");
    return operands[0].width();
}

std::vector<UIntBatch> three(const UIntBatch &a, const UIntBatch &b, const UIntBatch &c)
{
    std::vector<UIntBatch> v(1, a);
    v.push_back(b);
    v.push_back(c);
    return v;
}

} // namespace

UIntBatch polyMap(const std::vector<UIntBatch> &operands, const F2Polynomial &f, uint64_t constant)
{
    constant = requirePoly(operands, f, constant, "polyMap");
    const unsigned m = f.outWidth();
    const Context &ctx = operands[0].context();
    const uint64_t count = operands[0].size();
    // every size first
    const std::vector<CiphertextBatch> planes = polyPlanes(operands);
    const Planes in(planes);
    std::vector<uint64_t> first(1, 0), mfirst(1, 0), factor, T;
    std::vector<unsigned> at(m, 0), computed_rows;
    uint64_t ones_of = 0;                                 // the computed rows' constant bits
    for (unsigned x = 0; x < m; ++x) {
        const std::vector<PolyMonomial> &row = f.rows()[x];
        const bool one = (constant >> x) & 1u;
        if (polyKind(row, one) != POLY_COMPUTED)
            continue;
        const size_t m0 = mfirst.size() - 1;
        for (size_t i = 0; i < row.size(); ++i) {
            factor.insert(factor.end(), row[i].begin(), row[i].end());
            mfirst.push_back(factor.size());
        }
        at[x] = (unsigned)computed_rows.size();
        ones_of |= (uint64_t)one << computed_rows.size();
        computed_rows.push_back(x);
        T.push_back(checked(csgn_uint_poly_terms(in.terms.size(), in.terms.data(), row.size(), mfirst.data() + m0,
                                                 factor.data(), one ? 1 : 0),
                            ctx, "polyMap"));
        first.push_back(mfirst.size() - 1);
    }
    if (count == 0)
        return UIntBatch::fromPlanes(std::vector<CiphertextBatch>(m, BatchAccess::make(ctx, 0, 1)));
    std::vector<CiphertextBatch> computed;
    if (!computed_rows.empty() && in.uniform) {
        const csgn_uint_poly_plan *plan = polyPlan(in.terms, first, mfirst, factor, ones_of);
        computed = makePlanes(ctx, count, T);
        detail::check(csgn_uint_poly(plan, ctx.getN(), count, sources(in).data(), wordsOf(computed).data(), detail::stream()),
                      "csgn_uint_poly");
    } else if (!computed_rows.empty()) {
        // the loop: every operand plane in one batch (plane v's element e at v * count + e), then per output plane and
        // per degree d present, ascending, the d named planes gathered monomial by monomial, d - 1 element-wise
        // products and sumGroups, which copies nothing; operator+ between the degree groups, then + ONE
        const CiphertextBatch all = CiphertextBatch::concat(planes);
        for (size_t r = 0; r < computed_rows.size(); ++r) {
            const std::vector<PolyMonomial> &row = f.rows()[computed_rows[r]];
            std::vector<CiphertextBatch> sum;             // at most one: the running sum
            for (size_t i = 0; i < row.size();) {
                const size_t d = row[i].size();
                size_t j = i;
                while (j < row.size() && row[j].size() == d)
                    ++j;
                std::vector<CiphertextBatch> prod;        // at most one: the running product
                for (size_t k = 0; k < d; ++k) {
                    std::vector<uint64_t> idx;
                    idx.reserve(count * (j - i));
                    for (uint64_t e = 0; e < count; ++e)
                        for (size_t q = i; q < j; ++q)
                            idx.push_back(row[q][k] * count + e);
                    const CiphertextBatch g = all.gather(idx);
                    if (prod.empty())
                        prod.push_back(g);
                    else
                        prod[0] = prod[0] * g;
                }
                const CiphertextBatch group = prod[0].sumGroups(j - i);
                if (sum.empty())
                    sum.push_back(group);
                else
                    sum[0] = sum[0] + group;
                i = j;
            }
            computed.push_back((ones_of >> r) & 1u ? sum[0] + ones(planes[0]) : sum[0]);
        }
    }
    std::vector<CiphertextBatch> out;
    bool have_zero = false, have_one = false;
    CiphertextBatch zero = planes[0], one = planes[0];    // one shared payload for every constant plane of a kind
    for (unsigned x = 0; x < m; ++x) {
        const bool bit = (constant >> x) & 1u;
        switch (polyKind(f.rows()[x], bit)) {
        case POLY_SHARED: out.push_back(planes[f.rows()[x][0][0]]); break;
        case POLY_COMPUTED: out.push_back(computed[at[x]]); break;
        default:
            if (bit && !have_one) {
                one = ones(planes[0]);
                have_one = true;
            } else if (!bit && !have_zero) {
                zero = zeros(operands[0]);
                have_zero = true;
            }
            out.push_back(bit ? one : zero);
        }
    }
    return UIntBatch::fromPlanes(out);
}

UIntBatch ch(const UIntBatch &e, const UIntBatch &f, const UIntBatch &g)
{
    const std::vector<UIntBatch> ops = three(e, f, g);
    return polyMap(ops, F2Polynomial::ch(requireOneWidthOf(ops, "ch")));
}

UIntBatch maj(const UIntBatch &a, const UIntBatch &b, const UIntBatch &c)
{
    const std::vector<UIntBatch> ops = three(a, b, c);
    return polyMap(ops, F2Polynomial::maj(requireOneWidthOf(ops, "maj")));
}

UIntBatch chi(const UIntBatch &a, const UIntBatch &b, const UIntBatch &c)
{
    const std::vector<UIntBatch> ops = three(a, b, c);
    return polyMap(ops, F2Polynomial::chi(requireOneWidthOf(ops, "chi")));
}

UIntBatch andAll(const std::vector<UIntBatch> &operands)
{
    const unsigned w = requireOneWidthOf(operands, "andAll");
    return polyMap(operands, F2Polynomial::andAll(w, (unsigned)operands.size()));
}

const char *polyRoute(const std::vector<UIntBatch> &operands, const F2Polynomial &f, uint64_t constant)
{
    constant = requirePoly(operands, f, constant, "polyRoute");
    if (operands[0].size() == 0 || !polyComputes(f, constant))
        return "none";
    return Planes(polyPlanes(operands)).uniform ? "k_uint_poly" : "loop";
}

// ------------------------------------------------------------------ ranges, sets, step functions (csgn_uint_plain_sum)

namespace {

typedef std::pair<int, uint64_t> PlainEntry;              // (CSGN_UINT_PLAIN_*, k)
typedef std::vector<PlainEntry> PlainEntries;

// device plans per (width, terms, entries, constant), kept until the process ends
const csgn_uint_plain_sum_plan *plainSumPlan(const std::vector<uint64_t> &terms, const std::vector<uint64_t> &first,
                                             const std::vector<int> &cmp, const std::vector<uint64_t> &k, uint64_t constant)
{
    static std::mutex mutex;
    static std::map<std::vector<uint64_t>, csgn_uint_plain_sum_plan *> *plans =
        new std::map<std::vector<uint64_t>, csgn_uint_plain_sum_plan *>();
    std::vector<uint64_t> key(1, constant);
    key.push_back(terms.size());
    key.insert(key.end(), terms.begin(), terms.end());
    key.insert(key.end(), first.begin(), first.end());
    key.insert(key.end(), cmp.begin(), cmp.end());
    key.insert(key.end(), k.begin(), k.end());
    std::lock_guard<std::mutex> lock(mutex);
    auto it = plans->find(key);
    if (it != plans->end())
        return it->second;
    csgn_uint_plain_sum_plan *p = nullptr;
    detail::check(csgn_uint_plain_sum_create(terms.size(), terms.data(), first.size() - 1, first.data(), cmp.data(), k.data(),
                                             constant, &p),
                  "csgn_uint_plain_sum_create");
    (*plans)[key] = p;
    return p;
}

// what plainSum does with a plane: the constant batch, one comparison's own call, or a computed plane
enum { SUM_CONSTANT, SUM_SINGLE, SUM_COMPUTED };

int plainSumKind(const PlainEntries &entries, bool one)
{
    if (entries.empty())
        return SUM_CONSTANT;
    return entries.size() == 1 && !one ? SUM_SINGLE : SUM_COMPUTED;
}

const char *whoOf(int cmp)
{
    static const char *const names[] = {"", "equalTo", "notEqualTo", "lessThan", "lessEqual", "greaterThan", "greaterEqual"};
    return names[cmp];
}

// The planes of csgn_uint_plain_sum's definition over a: plane x sums the comparisons planes[x], + ONE where bit x of
// `constant` is set.  Every size first; one plan and one launch for the computed planes of uniform inputs, else the
// definition through the batch operators.
std::vector<CiphertextBatch> plainSum(const UIntBatch &a, const std::vector<PlainEntries> &planes, uint64_t constant,
                                      const char *who)
{
    const unsigned w = a.width(), m = (unsigned)planes.size();
    const Context &ctx = a.context();
    const Planes in(a);
    std::vector<uint64_t> first(1, 0), k, T;
    std::vector<int> cmp;
    uint64_t ones_of = 0;
    for (unsigned x = 0; x < m; ++x) {
        const bool one = (constant >> x) & 1u;
        std::vector<int> c;
        std::vector<uint64_t> ks;
        for (size_t i = 0; i < planes[x].size(); ++i) {
            c.push_back(planes[x][i].first);
            ks.push_back(planes[x][i].second);
        }
        checked(csgn_uint_plain_sum_terms(w, in.terms.data(), c.size(), c.data(), ks.data(), one ? 1 : 0), ctx, who);
        if (plainSumKind(planes[x], one) != SUM_COMPUTED)
            continue;
        ones_of |= (uint64_t)one << T.size();
        T.push_back(csgn_uint_plain_sum_terms(w, in.terms.data(), c.size(), c.data(), ks.data(), one ? 1 : 0));
        cmp.insert(cmp.end(), c.begin(), c.end());
        k.insert(k.end(), ks.begin(), ks.end());
        first.push_back(cmp.size());
    }
    if (cmp.size() > 65536)
        throw std::invalid_argument(std::string("certFHE::") + who + ": more than 65536 comparisons in one call");
    if (a.size() == 0)
        return std::vector<CiphertextBatch>(m, BatchAccess::make(ctx, 0, 1));
    std::vector<CiphertextBatch> computed;
    if (!T.empty() && in.uniform) {
        const csgn_uint_plain_sum_plan *plan = plainSumPlan(in.terms, first, cmp, k, ones_of);
        computed = makePlanes(ctx, a.size(), T);
        detail::check(csgn_uint_plain_sum(plan, ctx.getN(), a.size(), sources(in).data(), wordsOf(computed).data(),
                                          detail::stream()),
                      "csgn_uint_plain_sum");
    }
    std::vector<CiphertextBatch> out;
    size_t next = 0;
    for (unsigned x = 0; x < m; ++x) {
        const bool one = (constant >> x) & 1u;
        switch (plainSumKind(planes[x], one)) {
        case SUM_CONSTANT: out.push_back(one ? ones(a.plane(0)) : zeros(a)); break;
        case SUM_SINGLE:
            out.push_back(comparePlain(planes[x][0].first, a, planes[x][0].second, whoOf(planes[x][0].first)));
            break;
        default:
            if (in.uniform) {
                out.push_back(computed[next++]);
                break;
            }
            CiphertextBatch sum = comparePlain(planes[x][0].first, a, planes[x][0].second, who);
            for (size_t i = 1; i < planes[x].size(); ++i)
                sum = sum + comparePlain(planes[x][i].first, a, planes[x][i].second, who);
            out.push_back(one ? sum + ones(a.plane(0)) : sum);
        }
    }
    return out;
}

void requireBelow(const UIntBatch &a, uint64_t v, const char *who, const char *what)
{
    if (a.width() < 64 && (v >> a.width()) != 0)
        throw std::invalid_argument(std::string("certFHE::") + who + ": " + what + " does not fit in the width");
}

// the entries of lo <= a <= hi appended; returns true when the range is everything (+ ONE)
bool rangeEntries(const UIntBatch &a, uint64_t lo, uint64_t hi, const char *who, PlainEntries &entries)
{
    if (lo > hi)
        throw std::invalid_argument(std::string("certFHE::") + who + ": lo is above hi");
    requireBelow(a, hi, who, "a bound");
    const uint64_t top = maskOf(a.width());
    if (lo == 0 && hi == top)
        return true;
    if (lo == 0) {
        entries.push_back(PlainEntry(CSGN_UINT_PLAIN_LE, hi));
    } else if (hi == top) {
        entries.push_back(PlainEntry(CSGN_UINT_PLAIN_GE, lo));
    } else {
        entries.push_back(PlainEntry(CSGN_UINT_PLAIN_LT, hi + 1));
        entries.push_back(PlainEntry(CSGN_UINT_PLAIN_LT, lo));
    }
    return false;
}

PlainEntries setEntries(const UIntBatch &a, const std::vector<uint64_t> &set, const char *who)
{
    std::vector<uint64_t> keys(set);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    PlainEntries entries;
    for (size_t i = 0; i < keys.size(); ++i) {
        requireBelow(a, keys[i], who, "a value of the set");
        entries.push_back(PlainEntry(CSGN_UINT_PLAIN_EQ, keys[i]));
    }
    return entries;
}

void requireOutWidth(unsigned out_width, const std::vector<uint64_t> &values, const char *who)
{
    if (out_width < 1 || out_width > 64)
        throw std::invalid_argument(std::string("certFHE::") + who + ": out_width must be 1..64");
    for (size_t i = 0; i < values.size(); ++i)
        if (out_width < 64 && (values[i] >> out_width) != 0)
            throw std::invalid_argument(std::string("certFHE::") + who + ": a value does not fit in out_width");
}

// planes and constant of the step function
uint64_t stepEntries(const UIntBatch &a, const std::vector<uint64_t> &thresholds, const std::vector<uint64_t> &values,
                     unsigned out_width, const char *who, std::vector<PlainEntries> &planes)
{
    requireOutWidth(out_width, values, who);
    if (values.size() != thresholds.size() + 1)
        throw std::invalid_argument(std::string("certFHE::") + who + ": m thresholds take m + 1 values");
    for (size_t i = 0; i < thresholds.size(); ++i) {
        requireBelow(a, thresholds[i], who, "a threshold");
        if (thresholds[i] == 0 || (i && thresholds[i] <= thresholds[i - 1]))
            throw std::invalid_argument(std::string("certFHE::") + who + ": thresholds must ascend strictly from 1 on");
    }
    planes.assign(out_width, PlainEntries());
    for (unsigned j = 0; j < out_width; ++j)
        for (size_t i = 0; i < thresholds.size(); ++i)
            if (((values[i] ^ values[i + 1]) >> j) & 1u)
                planes[j].push_back(PlainEntry(CSGN_UINT_PLAIN_LT, thresholds[i]));
    return values.back();
}

std::vector<uint64_t> bucketValues(const std::vector<uint64_t> &thresholds, unsigned planes, const char *who)
{
    if (planes < 1 || planes > 64 || (planes < 64 && (thresholds.size() >> planes) != 0))
        throw std::invalid_argument(std::string("certFHE::") + who + ": the bucket index does not fit in the planes");
    std::vector<uint64_t> values(thresholds.size() + 1);
    for (size_t i = 0; i < values.size(); ++i)
        values[i] = i;
    return values;
}

} // namespace

CiphertextBatch inRange(const UIntBatch &a, uint64_t lo, uint64_t hi)
{
    std::vector<PlainEntries> planes(1);
    const bool all = rangeEntries(a, lo, hi, "inRange", planes[0]);
    return plainSum(a, planes, all ? 1 : 0, "inRange")[0];
}

CiphertextBatch outOfRange(const UIntBatch &a, uint64_t lo, uint64_t hi)
{
    std::vector<PlainEntries> planes(1);
    if (rangeEntries(a, lo, hi, "outOfRange", planes[0])) {
        const CiphertextBatch one = plainSum(a, planes, 1, "outOfRange")[0];
        return a.size() ? one + ones(a.plane(0)) : one;
    }
    return plainSum(a, planes, 1, "outOfRange")[0];
}

CiphertextBatch inRanges(const UIntBatch &a, const std::vector<std::pair<uint64_t, uint64_t> > &intervals)
{
    std::vector<PlainEntries> planes(1);
    uint64_t constant = 0;
    for (size_t i = 0; i < intervals.size(); ++i) {
        if (i && intervals[i].first <= intervals[i - 1].second)
            throw std::invalid_argument("certFHE::inRanges: the intervals must be disjoint and ascend");
        if (rangeEntries(a, intervals[i].first, intervals[i].second, "inRanges", planes[0]))
            constant = 1;
    }
    return plainSum(a, planes, constant, "inRanges")[0];
}

CiphertextBatch isIn(const UIntBatch &a, const std::vector<uint64_t> &set)
{
    return plainSum(a, std::vector<PlainEntries>(1, setEntries(a, set, "isIn")), 0, "isIn")[0];
}

CiphertextBatch notIn(const UIntBatch &a, const std::vector<uint64_t> &set)
{
    return plainSum(a, std::vector<PlainEntries>(1, setEntries(a, set, "notIn")), 1, "notIn")[0];
}

UIntBatch stepFunction(const UIntBatch &a, const std::vector<uint64_t> &thresholds, const std::vector<uint64_t> &values,
                       unsigned out_width)
{
    std::vector<PlainEntries> planes;
    const uint64_t constant = stepEntries(a, thresholds, values, out_width, "stepFunction", planes);
    return UIntBatch::fromPlanes(plainSum(a, planes, constant, "stepFunction"));
}

UIntBatch bucketOf(const UIntBatch &a, const std::vector<uint64_t> &thresholds, unsigned planes)
{
    const std::vector<uint64_t> values = bucketValues(thresholds, planes, "bucketOf");
    std::vector<PlainEntries> entries;
    const uint64_t constant = stepEntries(a, thresholds, values, planes, "bucketOf", entries);
    return UIntBatch::fromPlanes(plainSum(a, entries, constant, "bucketOf"));
}

UIntBatch lookupSparse(const UIntBatch &a, const std::vector<uint64_t> &keys, const std::vector<uint64_t> &values,
                       unsigned out_width, uint64_t otherwise)
{
    requireOutWidth(out_width, values, "lookupSparse");
    requireOutWidth(out_width, std::vector<uint64_t>(1, otherwise), "lookupSparse");
    if (keys.size() != values.size())
        throw std::invalid_argument("certFHE::lookupSparse: every key takes one value");
    std::map<uint64_t, uint64_t> table;                   // distinct keys ascending; the first of equal keys counts
    for (size_t i = 0; i < keys.size(); ++i) {
        requireBelow(a, keys[i], "lookupSparse", "a key");
        table.insert(std::make_pair(keys[i], values[i]));
    }
    std::vector<PlainEntries> planes(out_width);
    for (unsigned j = 0; j < out_width; ++j)
        for (std::map<uint64_t, uint64_t>::const_iterator it = table.begin(); it != table.end(); ++it)
            if (((it->second ^ otherwise) >> j) & 1u)
                planes[j].push_back(PlainEntry(CSGN_UINT_PLAIN_EQ, it->first));
    return UIntBatch::fromPlanes(plainSum(a, planes, otherwise, "lookupSparse"));
}

const char *plainSumRoute(const UIntBatch &a, const std::vector<uint64_t> &thresholds, const std::vector<uint64_t> &values,
                          unsigned out_width)
{
    std::vector<PlainEntries> planes;
    const uint64_t constant = stepEntries(a, thresholds, values, out_width, "plainSumRoute", planes);
    bool computes = false;
    for (unsigned j = 0; j < out_width; ++j)
        computes = computes || plainSumKind(planes[j], (constant >> j) & 1u) == SUM_COMPUTED;
    return a.size() != 0 && Planes(a).uniform && computes ? "call" : "loop";
}

// ------------------------------------------------------------------ selection by a < b (csgn_uint_lt_select)

namespace {

// out_i = logicMux(lessThan(a, b), xs[i], ys[i]) for every request
std::vector<CiphertextBatch> selectLessPlanes(const UIntBatch &a, const UIntBatch &b, const std::vector<CiphertextBatch> &xs,
                                              const std::vector<CiphertextBatch> &ys, const char *who)
{
    requireSame(a, b, who);
    const Context &ctx = a.context();
    const uint64_t m = a.size(), n = xs.size();
    for (size_t i = 0; i < n; ++i)
        if (xs[i].size() != m || ys[i].size() != m || !sameContext(xs[i].context(), ctx) || !sameContext(ys[i].context(), ctx))
            throw std::invalid_argument(std::string("certFHE::") + who +
                                        ": the selected operands differ from the compared ones in count or context");
    // every size before anything is allocated
    const uint64_t L = lessThanTerms(a, b, who);
    const Planes pa(a), pb(b), px(xs), py(ys);
    std::vector<uint64_t> T(n);
    for (size_t i = 0; i < n; ++i)
        T[i] = gateTerms(CSGN_GATE_MUX, L, px.terms[i], py.terms[i], ctx, who);
    if (a.width() <= 16 && ((pa.uniform && pb.uniform && px.uniform && py.uniform) || m == 0)) {
        std::vector<CiphertextBatch> out = makePlanes(ctx, m, T);
        if (m) {
            const std::vector<const uint64_t *> sa = sources(pa), sb = sources(pb), sx = sources(px), sy = sources(py);
            const std::vector<uint64_t *> dst = wordsOf(out);
            for (uint64_t i0 = 0; i0 < n; i0 += 64)                   // 64 requests a launch
                detail::check(csgn_uint_lt_select(ctx.getN(), m, a.width(), sa.data(), pa.terms.data(), sb.data(),
                                                  pb.terms.data(), std::min<uint64_t>(64, n - i0), sx.data() + i0,
                                                  px.terms.data() + i0, sy.data() + i0, py.terms.data() + i0,
                                                  dst.data() + i0, nullptr, detail::stream()),
                              "csgn_uint_lt_select");
        }
        return out;
    }
    // ragged, or wider than 16 bits: the definition itself through lessThan(a, b) and select's gate
    std::vector<CiphertextBatch> out;
    const CiphertextBatch l = lessThanUnchecked(a, b);
    for (size_t i = 0; i < n; ++i)
        out.push_back(logicMux(l, xs[i], ys[i]));
    return out;
}

void appendPlanes(std::vector<CiphertextBatch> &list, const UIntBatch &a)
{
    for (unsigned j = 0; j < a.width(); ++j)
        list.push_back(a.plane(j));
}

UIntBatch takePlanes(const std::vector<CiphertextBatch> &planes, size_t first, unsigned width)
{
    return UIntBatch::fromPlanes(std::vector<CiphertextBatch>(planes.begin() + first, planes.begin() + first + width));
}

} // namespace

UIntBatch selectLess(const UIntBatch &a, const UIntBatch &b, const UIntBatch &x, const UIntBatch &y)
{
    requireSame(x, y, "selectLess");
    std::vector<CiphertextBatch> xs, ys;
    appendPlanes(xs, x);
    appendPlanes(ys, y);
    return UIntBatch::fromPlanes(selectLessPlanes(a, b, xs, ys, "selectLess"));
}

CiphertextBatch selectLess(const UIntBatch &a, const UIntBatch &b, const CiphertextBatch &x, const CiphertextBatch &y)
{
    return selectLessPlanes(a, b, std::vector<CiphertextBatch>(1, x), std::vector<CiphertextBatch>(1, y), "selectLess")[0];
}

UIntBatch min(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "min");
    std::vector<CiphertextBatch> xs, ys;
    appendPlanes(xs, a);
    appendPlanes(ys, b);
    return UIntBatch::fromPlanes(selectLessPlanes(a, b, xs, ys, "min"));
}

UIntBatch max(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "max");
    std::vector<CiphertextBatch> xs, ys;
    appendPlanes(xs, b);
    appendPlanes(ys, a);
    return UIntBatch::fromPlanes(selectLessPlanes(a, b, xs, ys, "max"));
}

void compareExchange(const UIntBatch &a, const UIntBatch &b, const UIntBatch &pa, const UIntBatch &pb, UIntBatch *lo,
                     UIntBatch *hi, UIntBatch *plo, UIntBatch *phi)
{
    requireSame(a, b, "compareExchange");
    requireSame(pa, pb, "compareExchange");
    std::vector<CiphertextBatch> xs, ys;
    if (lo) {
        appendPlanes(xs, a);
        appendPlanes(ys, b);
    }
    if (hi) {
        appendPlanes(xs, b);
        appendPlanes(ys, a);
    }
    if (plo) {
        appendPlanes(xs, pa);
        appendPlanes(ys, pb);
    }
    if (phi) {
        appendPlanes(xs, pb);
        appendPlanes(ys, pa);
    }
    const std::vector<CiphertextBatch> out = selectLessPlanes(a, b, xs, ys, "compareExchange");
    size_t at = 0;
    UIntBatch *const dst[4] = {lo, hi, plo, phi};
    for (int k = 0; k < 4; ++k)
        if (dst[k]) {
            const unsigned width = k < 2 ? a.width() : pa.width();
            *dst[k] = takePlanes(out, at, width);
            at += width;
        }
}

std::pair<UIntBatch, UIntBatch> minMax(const UIntBatch &a, const UIntBatch &b)
{
    requireSame(a, b, "minMax");
    std::vector<CiphertextBatch> xs, ys;
    appendPlanes(xs, a);
    appendPlanes(xs, b);
    appendPlanes(ys, b);
    appendPlanes(ys, a);
    const std::vector<CiphertextBatch> out = selectLessPlanes(a, b, xs, ys, "minMax");
    return std::make_pair(takePlanes(out, 0, a.width()), takePlanes(out, a.width(), a.width()));
}

} // namespace certFHE

namespace certFHE {

// ------------------------------------------------------------------ public lookup tables

struct LookupTable::Impl {
    unsigned w = 0, m = 0;
    std::vector<uint64_t> table, anf;
    std::mutex mutex;
    std::map<std::vector<uint64_t>, csgn_uint_lut *> plans;     // device plans per vector of plane term counts

    ~Impl()
    {
        for (auto &p : plans)
            csgn_uint_lut_destroy(p.second);
    }

    const csgn_uint_lut *plan(const std::vector<uint64_t> &terms)
    {
        std::lock_guard<std::mutex> lock(mutex);
        auto it = plans.find(terms);
        if (it != plans.end())
            return it->second;
        csgn_uint_lut *p = nullptr;
        detail::check(csgn_uint_lut_create(w, m, table.data(), terms.data(), &p), "csgn_uint_lut_create");
        plans[terms] = p;
        return p;
    }
};

LookupTable::LookupTable(const std::vector<uint64_t> &table, unsigned in_width, unsigned out_width)
    : impl_(std::make_shared<Impl>())
{
    if (in_width < 1 || in_width > 16 || out_width < 1 || out_width > 64)
        throw std::invalid_argument("certFHE::LookupTable: in_width must be 1..16 and out_width 1..64");
    if (table.size() != (size_t(1) << in_width))
        throw std::invalid_argument("certFHE::LookupTable: the table must have 2^in_width entries");
    impl_->w = in_width;
    impl_->m = out_width;
    impl_->table = table;
    impl_->anf.resize(table.size());
    if (csgn_uint_lut_anf(in_width, out_width, table.data(), impl_->anf.data()) != CSGN_OK)
        throw std::invalid_argument("certFHE::LookupTable: an entry does not fit in out_width bits");
}

unsigned LookupTable::inWidth() const { return impl_->w; }
unsigned LookupTable::outWidth() const { return impl_->m; }
const std::vector<uint64_t> &LookupTable::table() const { return impl_->table; }
const std::vector<uint64_t> &LookupTable::anf() const { return impl_->anf; }

namespace {

// M_S = ((a_{i1} * a_{i2}) * ...) over i in S ascending; ONE for the empty set
CiphertextBatch monomial(const UIntBatch &a, uint64_t S)
{
    if (S == 0)
        return ones(a.plane(0));
    CiphertextBatch r = a.plane((unsigned)__builtin_ctzll(S));
    for (S &= S - 1; S; S &= S - 1)
        r = r * a.plane((unsigned)__builtin_ctzll(S));
    return r;
}

} // namespace

UIntBatch lookup(const UIntBatch &a, const LookupTable &f)
{
    LookupTable::Impl &L = *f.impl();
    if (a.width() != L.w)
        throw std::invalid_argument("certFHE::lookup: the operand's width differs from the table's in_width");
    const Context &ctx = a.context();
    const Planes in(a);
    std::vector<uint64_t> T(L.m);
    if (csgn_uint_lut_terms(L.w, L.m, L.table.data(), in.terms.data(), T.data()) != CSGN_OK)
        throw std::invalid_argument("certFHE::lookup: an output's result exceeds 2^31 words per element");
    for (unsigned j = 0; j < L.m; ++j)
        checked(T[j], ctx, "lookup");
    if (in.uniform) {
        const csgn_uint_lut *plan = L.plan(in.terms);
        std::vector<CiphertextBatch> out = makePlanes(ctx, a.size(), T);
        if (a.size())
            detail::check(csgn_uint_lut_apply(plan, ctx.getN(), a.size(), sources(in).data(), wordsOf(out).data(),
                                              detail::stream()),
                          "csgn_uint_lut_apply");
        return UIntBatch::fromPlanes(out);
    }
    std::vector<CiphertextBatch> out;
    // ragged: the definition itself through the batch operators
    for (unsigned j = 0; j < L.m; ++j) {
        std::vector<CiphertextBatch> acc;                 // empty until the first monomial
        for (uint64_t S = 0; S < L.anf.size(); ++S) {
            if (!((L.anf[S] >> j) & 1u))
                continue;
            const CiphertextBatch mono = monomial(a, S);
            if (acc.empty())
                acc.push_back(mono);
            else
                acc[0] = acc[0] + mono;
        }
        out.push_back(acc.empty() ? constantBatch(ctx, std::vector<unsigned char>(a.size(), 0)) : acc[0]);
    }
    return UIntBatch::fromPlanes(out);
}

UIntBatch lookup(const UIntBatch &a, const UIntBatch &b, const LookupTable &f)
{
    if (a.size() != b.size() || !sameContext(a.context(), b.context()))
        throw std::invalid_argument("certFHE::lookup: operands differ in count or context");
    if (a.width() + b.width() != f.inWidth())
        throw std::invalid_argument("certFHE::lookup: the operands' widths do not add up to the table's in_width");
    std::vector<CiphertextBatch> planes;
    for (unsigned i = 0; i < a.width(); ++i)
        planes.push_back(a.plane(i));
    for (unsigned i = 0; i < b.width(); ++i)
        planes.push_back(b.plane(i));
    return lookup(UIntBatch::fromPlanes(planes), f);
}

} // namespace certFHE

namespace certFHE {

// ------------------------------------------------------------------ encrypted tables at encrypted indices

namespace {

// every table plane read at the index: out_j = sum over r < rows of equalTo(index, r) * row r of plane j
std::vector<CiphertextBatch> readPlanes(const std::vector<CiphertextBatch> &table, const UIntBatch &index)
{
    const Context &ctx = index.context();
    const uint64_t v = index.width(), rows = table[0].size(), m = index.size();
    for (size_t j = 0; j < table.size(); ++j)
        if (!sameContext(table[j].context(), ctx) || table[j].size() != rows)
            throw std::invalid_argument("certFHE::readAt: the table and the index differ in context, or the table planes in rows");
    if (v > 16)
        throw std::invalid_argument("certFHE::readAt: the index is wider than 16 bits");
    if (rows == 0 || rows > (1ull << v))
        throw std::invalid_argument("certFHE::readAt: the table has " + std::to_string(rows) + " rows, not 1..2^" +
                                    std::to_string(v));
    const Planes x(index), d(table);
    const std::vector<uint64_t> &t = d.terms;
    std::vector<uint64_t> T(table.size());
    const uint64_t E = csgn_uint_read_terms(v, x.terms.data(), rows);
    for (size_t j = 0; j < table.size(); ++j) {
        if (E == 0 || t[j] == 0 || t[j] > kMaxWords / E)
            throw std::invalid_argument("certFHE::readAt: an output plane exceeds 2^31 words per element (the index "
                                        "is too wide or has too many terms)");
        T[j] = checked(t[j] * E, ctx, "readAt");
    }
    if ((x.uniform && d.uniform) || m == 0) {
        std::vector<CiphertextBatch> out = makePlanes(ctx, m, T);
        if (m)
            detail::check(csgn_uint_read(ctx.getN(), m, v, sources(x).data(), x.terms.data(), rows, table.size(),
                                         sources(d).data(), t.data(), wordsOf(out).data(), detail::stream()),
                          "csgn_uint_read");
        return out;
    }
    std::vector<CiphertextBatch> out;
    // ragged: the definition itself through the batch operators
    for (uint64_t r = 0; r < rows; ++r) {
        const CiphertextBatch eq = equalTo(index, r);
        for (size_t j = 0; j < table.size(); ++j) {
            const CiphertextBatch p = eq * table[j].slice(r, r + 1).broadcast(m);
            if (r == 0)
                out.push_back(p);
            else
                out[j] = out[j] + p;
        }
    }
    return out;
}

} // namespace

UIntBatch readAt(const UIntBatch &table, const UIntBatch &index)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < table.width(); ++j)
        planes.push_back(table.plane(j));
    return UIntBatch::fromPlanes(readPlanes(planes, index));
}

CiphertextBatch readAt(const CiphertextBatch &table, const UIntBatch &index)
{
    return readPlanes(std::vector<CiphertextBatch>(1, table), index)[0];
}

// ------------------------------------------------------------------ encrypted tables by encrypted key

namespace {

// every value plane looked up by the query: out_j = sum over r of equalTo(key row r, query) * row r of plane j, and,
// with want_member, the sum of the equalities as the last plane of the result
std::vector<CiphertextBatch> findPlanes(const UIntBatch &keys, const std::vector<CiphertextBatch> &values,
                                        const UIntBatch &query, bool want_member)
{
    const Context &ctx = query.context();
    const uint64_t v = keys.width(), rows = keys.size(), m = query.size();
    if (!sameContext(keys.context(), ctx))
        throw std::invalid_argument("certFHE::readWhere: the keys and the query differ in context");
    if (query.width() != v)
        throw std::invalid_argument("certFHE::readWhere: the keys and the query differ in width");
    if (v > 16)
        throw std::invalid_argument("certFHE::readWhere: the keys are wider than 16 bits");
    for (size_t j = 0; j < values.size(); ++j)
        if (!sameContext(values[j].context(), ctx) || values[j].size() != rows)
            throw std::invalid_argument("certFHE::readWhere: the values differ from the keys in context or in rows");
    if (rows == 0)
        throw std::invalid_argument("certFHE::readWhere: the table has no rows");
    const Planes y(keys), x(query), d(values);
    const std::vector<uint64_t> &t = d.terms;
    const uint64_t P = csgn_uint_find_terms(v, y.terms.data(), x.terms.data());
    const char *too_large = "certFHE::readWhere: an output plane exceeds 2^31 words per element (the keys are too wide, "
                            "have too many terms, or the table too many rows)";
    if (P == 0 || rows > kMaxWords / P)
        throw std::invalid_argument(too_large);
    std::vector<uint64_t> T(values.size() + (want_member ? 1 : 0));
    for (size_t j = 0; j < T.size(); ++j) {
        const uint64_t tj = j < values.size() ? t[j] : 1;
        if (tj == 0 || tj > kMaxWords / (rows * P))
            throw std::invalid_argument(too_large);
        T[j] = checked(tj * rows * P, ctx, "readWhere");
    }
    if ((y.uniform && x.uniform && d.uniform) || m == 0) {
        std::vector<CiphertextBatch> out = makePlanes(ctx, m, T);
        if (m) {
            std::vector<uint64_t *> dst = wordsOf(out);
            uint64_t *member = want_member ? dst.back() : nullptr;
            detail::check(csgn_uint_find(ctx.getN(), m, v, sources(x).data(), x.terms.data(), rows, sources(y).data(),
                                         y.terms.data(), values.size(), sources(d).data(), t.data(), dst.data(), member,
                                         detail::stream()),
                          "csgn_uint_find");
        }
        return out;
    }
    std::vector<CiphertextBatch> out;
    // ragged: the definition itself through the batch operators
    for (uint64_t r = 0; r < rows; ++r) {
        const CiphertextBatch eq = equalTo(keys.slice(r, r + 1).broadcast(m), query);
        for (size_t j = 0; j < T.size(); ++j) {
            const CiphertextBatch p = j < values.size() ? eq * values[j].slice(r, r + 1).broadcast(m) : eq;
            if (r == 0)
                out.push_back(p);
            else
                out[j] = out[j] + p;
        }
    }
    return out;
}

std::vector<CiphertextBatch> planesOf(const UIntBatch &a)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < a.width(); ++j)
        planes.push_back(a.plane(j));
    return planes;
}

} // namespace

UIntBatch readWhere(const UIntBatch &keys, const UIntBatch &values, const UIntBatch &query)
{
    return UIntBatch::fromPlanes(findPlanes(keys, planesOf(values), query, false));
}

CiphertextBatch readWhere(const UIntBatch &keys, const CiphertextBatch &values, const UIntBatch &query)
{
    return findPlanes(keys, std::vector<CiphertextBatch>(1, values), query, false)[0];
}

UIntBatch readWhere(const UIntBatch &keys, const UIntBatch &values, const UIntBatch &query, CiphertextBatch *member)
{
    std::vector<CiphertextBatch> out = findPlanes(keys, planesOf(values), query, member != nullptr);
    if (member) {
        *member = out.back();
        out.pop_back();
    }
    return UIntBatch::fromPlanes(out);
}

CiphertextBatch matches(const UIntBatch &keys, const UIntBatch &query)
{
    return findPlanes(keys, std::vector<CiphertextBatch>(), query, true)[0];
}

// ------------------------------------------------------------------ shifts, rotates and own arrays by encrypted amounts

namespace {

uint64_t pickRows(int op, uint64_t v, uint64_t w, uint64_t n, uint64_t j)
{
    const uint64_t full = v >= 64 ? ~0ull : 1ull << v;
    switch (op) {
    case CSGN_UINT_PICK_SHL:
        return std::min<uint64_t>(j + 1, full);
    case CSGN_UINT_PICK_SHR:
        return std::min<uint64_t>(w - j, full);
    case CSGN_UINT_PICK_EACH:
        return n;
    default:
        return full;
    }
}

unsigned pickSource(int op, unsigned w, unsigned j, uint64_t r)
{
    switch (op) {
    case CSGN_UINT_PICK_SHL:
        return j - (unsigned)r;
    case CSGN_UINT_PICK_SHR:
        return j + (unsigned)r;
    case CSGN_UINT_PICK_ROTL:
        return (j + w - (unsigned)(r % w)) % w;
    case CSGN_UINT_PICK_ROTR:
        return (unsigned)((j + r % w) % w);
    default:
        return j;
    }
}

// terms of output j by the definition itself, row by row: sum over r < rows of EQ(d, r)'s terms times the source's; 0
// once it passes kMaxWords (no output that large fits 2^31 words)
uint64_t pickTermsByRows(int op, const std::vector<uint64_t> &s, const std::vector<uint64_t> &t, uint64_t rows, unsigned j)
{
    if (rows > kMaxWords)
        return 0;                                   // every row has at least one term
    uint64_t T = 0;
    for (uint64_t r = 0; r < rows; ++r) {
        uint64_t p = t[pickSource(op, (unsigned)t.size(), j, r)];
        for (size_t k = 0; k < s.size() && p <= kMaxWords; ++k)
            p *= (k < 64 && ((r >> k) & 1u)) ? s[k] : s[k] + 1;
        T += p;
        if (p > kMaxWords || T > kMaxWords)
            return 0;
    }
    return T;
}

// Whether the terms of a plane's elements have period n over m arrays -- termsOf(e * n + r) == termsOf(r) for every e,
// read from the host offsets --, and the n counts into rows.  A uniform plane has it, with a constant.
bool periodRows(const CiphertextBatch &p, uint64_t n, uint64_t m, uint64_t *rows)
{
    if (p.uniform()) {
        std::fill(rows, rows + n, p.terms());
        return true;
    }
    for (uint64_t r = 0; r < n; ++r)
        rows[r] = p.termsOf(r);
    for (uint64_t e = 1; e < m; ++e)
        for (uint64_t r = 0; r < n; ++r)
            if (p.termsOf(e * n + r) != rows[r])
                return false;
    return true;
}

// The route of readAtEach (readAtEachRoute): "pick" -- uniform planes of one count under a uniform index of at most 16
// bits: csgn_uint_pick --, "rows" -- a uniform index of at most 16 bits over planes of period n, what writeAtEach
// returns: csgn_uint_pick_rows, the rows' counts plane-major into *rows --, else "loop", the class-level loop of
// pickPlanes.  No device work.
const char *eachRoute(const std::vector<CiphertextBatch> &a, uint64_t n, const UIntBatch &d, std::vector<uint64_t> *rows)
{
    const uint64_t v = d.width(), m = d.size();
    if (a.empty() || v > 16 || n == 0 || n > (1ull << v) || (m != 0 && n > ~0ull / m))
        return "loop";
    for (unsigned k = 0; k < v; ++k)
        if (!d.plane(k).uniform())
            return "loop";
    bool one_count = true;
    for (size_t j = 0; j < a.size(); ++j)
        one_count = one_count && a[j].uniform() && a[j].terms() == a[0].terms();
    if (one_count)
        return "pick";
    std::vector<uint64_t> T(a.size() * n);
    for (size_t j = 0; j < a.size(); ++j)
        if (a[j].size() != n * m || !periodRows(a[j], n, m, &T[j * n]))
            return "loop";
    if (rows)
        rows->swap(T);
    return "rows";
}

// every output plane of one operation: out_j = sum over r < rows_j of equalTo(d, r) * source(j, r)
std::vector<CiphertextBatch> pickPlanes(int op, const std::vector<CiphertextBatch> &a, uint64_t n, const UIntBatch &d,
                                        const char *who)
{
    const Context &ctx = d.context();
    const uint64_t v = d.width(), m = d.size();
    const unsigned w = (unsigned)a.size();
    const bool each = op == CSGN_UINT_PICK_EACH;
    const std::string name = std::string("certFHE::") + who;
    if (each && (n == 0 || (v < 64 && n > (1ull << v))))
        throw std::invalid_argument(name + ": " + std::to_string(n) + " rows an element, not 1..2^" + std::to_string(v));
    if (each && m != 0 && n > ~0ull / m)
        throw std::invalid_argument(name + ": the arrays do not hold n rows for every index");
    for (unsigned j = 0; j < w; ++j)
        if (!sameContext(a[j].context(), ctx) || a[j].size() != (each ? n * m : m))
            throw std::invalid_argument(name + (each ? ": the arrays and the index differ in context, or arrays.size() != n * index.size()"
                                                     : ": the integer and the distance differ in context or count"));
    const Planes x(d), src(a);
    const std::vector<uint64_t> &t = src.terms;
    bool one_count = true;
    for (unsigned j = 1; j < w; ++j)
        one_count = one_count && t[j] == t[0];
    const bool fused = x.uniform && src.uniform && one_count && v <= 16;
    // planes of period n, what writeAtEach returns: one csgn_uint_pick_rows, uniform outputs
    std::vector<uint64_t> row_terms;
    const bool rows = each && !fused && m != 0 && w != 0 && std::string(eachRoute(a, n, d, &row_terms)) == "rows";
    std::vector<uint64_t> T(w);
    for (unsigned j = 0; j < w; ++j) {
        uint64_t terms = 0;
        if (m == 0) {
            terms = 1;                              // an empty batch has no sizes to check: empty planes
        } else if (fused) {
            const uint64_t E = csgn_uint_pick_terms(op, v, x.terms.data(), w, each ? n : 0, j);
            terms = (E == 0 || t[0] == 0 || t[0] > kMaxWords / E) ? 0 : t[0] * E;
        } else if (rows) {
            std::vector<uint64_t> so(n + 1), oo(n + 1);
            if (csgn_uint_pick_rows_offsets(v, x.terms.data(), n, &row_terms[j * n], so.data(), oo.data()) == CSGN_OK)
                terms = oo[n] > kMaxWords ? 0 : oo[n];
        } else {
            terms = pickTermsByRows(op, x.terms, t, pickRows(op, v, w, n, j), j);
        }
        if (terms == 0)
            throw std::invalid_argument(name + ": an output plane exceeds 2^31 words per element (the distance is too "
                                               "wide or has too many terms)");
        T[j] = checked(terms, ctx, who);
    }
    if (fused || m == 0) {
        std::vector<CiphertextBatch> out = makePlanes(ctx, m, T);
        if (m)
            detail::check(csgn_uint_pick(ctx.getN(), op, m, v, sources(x).data(), x.terms.data(), w, each ? n : 0,
                                         sources(src).data(), t[0], wordsOf(out).data(), detail::stream()),
                          "csgn_uint_pick");
        return out;
    }
    if (rows) {
        // every size before anything is allocated: the check is the launching call's own, on the host
        detail::check(csgn_uint_pick_rows_check(ctx.getN(), m, v, x.terms.data(), n, w, row_terms.data()),
                      "csgn_uint_pick_rows_check");
        std::vector<CiphertextBatch> out = makePlanes(ctx, m, T);
        detail::check(csgn_uint_pick_rows(ctx.getN(), m, v, sources(x).data(), x.terms.data(), n, w, sources(src).data(),
                                          row_terms.data(), wordsOf(out).data(), detail::stream()),
                      "csgn_uint_pick_rows");
        return out;
    }
    // ragged planes without a period, planes of different term counts under a wider distance: the definition itself
    // through the operators
    uint64_t rows_max = 0;
    for (unsigned j = 0; j < w; ++j)
        rows_max = std::max(rows_max, pickRows(op, v, w, n, j));
    std::vector<CiphertextBatch> out;
    for (uint64_t r = 0; r < rows_max; ++r) {
        const CiphertextBatch eq = equalTo(d, r);
        std::vector<uint64_t> idx;
        if (each) {
            idx.resize(m);
            for (uint64_t e = 0; e < m; ++e)
                idx[e] = e * n + r;
        }
        for (unsigned j = 0; j < w; ++j) {
            if (r >= pickRows(op, v, w, n, j))
                continue;
            const CiphertextBatch p = eq * (each ? a[j].gather(idx) : a[pickSource(op, w, j, r)]);
            if (r == 0)
                out.push_back(p);
            else
                out[j] = out[j] + p;
        }
    }
    return out;
}

} // namespace

UIntBatch UIntBatch::shiftLeft(const UIntBatch &d) const
{
    return UIntBatch(pickPlanes(CSGN_UINT_PICK_SHL, planes_, 0, d, "UIntBatch::shiftLeft"));
}

UIntBatch UIntBatch::shiftRight(const UIntBatch &d) const
{
    return UIntBatch(pickPlanes(CSGN_UINT_PICK_SHR, planes_, 0, d, "UIntBatch::shiftRight"));
}

UIntBatch UIntBatch::rotateLeft(const UIntBatch &d) const
{
    return UIntBatch(pickPlanes(CSGN_UINT_PICK_ROTL, planes_, 0, d, "UIntBatch::rotateLeft"));
}

UIntBatch UIntBatch::rotateRight(const UIntBatch &d) const
{
    return UIntBatch(pickPlanes(CSGN_UINT_PICK_ROTR, planes_, 0, d, "UIntBatch::rotateRight"));
}

UIntBatch readAtEach(const UIntBatch &arrays, uint64_t n, const UIntBatch &index)
{
    return UIntBatch::fromPlanes(pickPlanes(CSGN_UINT_PICK_EACH, planesOf(arrays), n, index, "readAtEach"));
}

const char *readAtEachRoute(const UIntBatch &arrays, uint64_t n, const UIntBatch &index)
{
    return eachRoute(planesOf(arrays), n, index, nullptr);
}

CiphertextBatch readAtEach(const CiphertextBatch &arrays, uint64_t n, const UIntBatch &index)
{
    return pickPlanes(CSGN_UINT_PICK_EACH, std::vector<CiphertextBatch>(1, arrays), n, index, "readAtEach")[0];
}

// ------------------------------------------------------------------ encrypted arrays written at encrypted indices

namespace {

// terms of row r by the definition itself: EQ(index, r)'s terms times (tv + td), plus td; 0 once it passes kMaxWords
uint64_t writeRowTerms(const std::vector<uint64_t> &s, uint64_t r, uint64_t tv, uint64_t td)
{
    uint64_t p = tv + td;
    for (size_t k = 0; k < s.size() && p <= kMaxWords; ++k)
        p *= (k < 64 && ((r >> k) & 1u)) ? s[k] : s[k] + 1;
    return p > kMaxWords ? 0 : p + td;
}

// every plane of the arrays with row index[e] of array e replaced by value[e]
std::vector<CiphertextBatch> writePlanes(const std::vector<CiphertextBatch> &arrays, uint64_t n, const UIntBatch &index,
                                         const std::vector<CiphertextBatch> &value, const char *who)
{
    const Context &ctx = index.context();
    const uint64_t v = index.width(), m = index.size();
    const unsigned w = (unsigned)arrays.size();
    const std::string name = std::string("certFHE::") + who;
    if (value.size() != w)
        throw std::invalid_argument(name + ": the arrays and the value differ in width");
    if (n == 0 || (v < 64 && n > (1ull << v)))
        throw std::invalid_argument(name + ": " + std::to_string(n) + " rows an array, not 1..2^" + std::to_string(v));
    if (m != 0 && n > ~0ull / m)
        throw std::invalid_argument(name + ": the arrays do not hold n rows for every index");
    for (unsigned j = 0; j < w; ++j)
        if (!sameContext(arrays[j].context(), ctx) || !sameContext(value[j].context(), ctx) || value[j].size() != m ||
            arrays[j].size() != n * m)
            throw std::invalid_argument(name + ": the arrays, the index and the value differ in context or count, or "
                                               "arrays.size() != n * index.size()");
    if (m == 0)
        return makePlanes(ctx, 0, std::vector<uint64_t>(w, 1));     // an empty batch has no sizes to check: empty planes
    const Planes x(index), val(value), d(arrays);
    const bool fused = x.uniform && val.uniform && d.uniform && v <= 16;
    const uint64_t limit = (kMaxWords - 1) / ctx.getDefaultN();      // terms of one array
    const std::string too_large = name + ": an array exceeds 2^31 words (the index is too wide or has too many terms)";
    if (fused) {
        // row offsets of period n, on the host in closed form
        std::vector<CiphertextBatch> out;
        std::vector<std::vector<uint64_t> > offsets(w, std::vector<uint64_t>(n * m + 1));
        for (unsigned j = 0; j < w; ++j) {
            const uint64_t A = csgn_uint_write_offset(v, x.terms.data(), n, n, val.terms[j], d.terms[j]);
            if (A == 0 || A > limit || m > (1ull << 60) / (A * ctx.getDefaultN()))
                throw std::invalid_argument(too_large);
            std::vector<uint64_t> &off = offsets[j];
            for (uint64_t r = 0; r < n; ++r)
                off[r] = csgn_uint_write_offset(v, x.terms.data(), n, r, val.terms[j], d.terms[j]);
            for (uint64_t e = 1; e < m; ++e)
                for (uint64_t r = 0; r < n; ++r)
                    off[e * n + r] = e * A + off[r];
            off[n * m] = m * A;
        }
        for (unsigned j = 0; j < w; ++j)
            out.push_back(BatchAccess::makeRagged(ctx, offsets[j]));
        detail::check(csgn_uint_write(ctx.getN(), m, v, sources(x).data(), x.terms.data(), n, w, sources(val).data(),
                                      val.terms.data(), sources(d).data(), d.terms.data(), wordsOf(out).data(),
                                      detail::stream()),
                      "csgn_uint_write");
        return out;
    }
    // ragged planes or a wider index: the definition itself through the operators.  Sizes first, by the planes' bounds
    for (unsigned j = 0; j < w; ++j) {
        uint64_t A = 0;
        for (uint64_t r = 0; r < n; ++r) {
            const uint64_t row = writeRowTerms(x.terms, r, val.terms[j], d.terms[j]);
            A += row;
            if (row == 0 || A > limit)
                throw std::invalid_argument(too_large);
        }
    }
    std::vector<std::vector<CiphertextBatch> > rows(w);
    std::vector<uint64_t> idx(m);
    for (uint64_t r = 0; r < n; ++r) {
        const CiphertextBatch eq = equalTo(index, r);
        for (uint64_t e = 0; e < m; ++e)
            idx[e] = e * n + r;
        for (unsigned j = 0; j < w; ++j)
            rows[j].push_back(logicMux(eq, value[j], arrays[j].gather(idx)));
    }
    // row-major over r to the arrays' layout: element e * n + r is element r * m + e of the concatenation
    std::vector<uint64_t> perm(n * m);
    for (uint64_t e = 0; e < m; ++e)
        for (uint64_t r = 0; r < n; ++r)
            perm[e * n + r] = r * m + e;
    std::vector<CiphertextBatch> out;
    for (unsigned j = 0; j < w; ++j)
        out.push_back(CiphertextBatch::concat(rows[j]).gather(perm));
    return out;
}

} // namespace

UIntBatch writeAtEach(const UIntBatch &arrays, uint64_t n, const UIntBatch &index, const UIntBatch &value)
{
    return UIntBatch::fromPlanes(writePlanes(planesOf(arrays), n, index, planesOf(value), "writeAtEach"));
}

CiphertextBatch writeAtEach(const CiphertextBatch &arrays, uint64_t n, const UIntBatch &index, const CiphertextBatch &value)
{
    return writePlanes(std::vector<CiphertextBatch>(1, arrays), n, index, std::vector<CiphertextBatch>(1, value),
                       "writeAtEach")[0];
}

UIntBatch writeAt(const UIntBatch &table, const UIntBatch &index, const UIntBatch &value)
{
    if (index.size() != 1)
        throw std::invalid_argument("certFHE::writeAt: one index and one value write one table");
    return UIntBatch::fromPlanes(writePlanes(planesOf(table), table.size(), index, planesOf(value), "writeAt"));
}

// ------------------------------------------------------------------ counting (csgn_count)

namespace {

// Terms per element of the planes js for inputs of t terms; 0: 2^j > group, the plane is ZERO.  Throws past 2^31 words.
std::vector<uint64_t> countSizes(const Context &ctx, uint64_t group, uint64_t t, const std::vector<unsigned> &js,
                                 const char *who)
{
    std::vector<uint64_t> T(js.size(), 0);
    for (size_t x = 0; x < js.size(); ++x) {
        if (js[x] > 6 || (1ull << js[x]) > group)
            continue;
        T[x] = csgn_count_terms(group, t, js[x]);
        if (T[x] == 0 || T[x] > (kMaxWords - 1) / ctx.getDefaultN())
            throw std::invalid_argument(std::string("certFHE::") + who + ": plane " + std::to_string(js[x]) +
                                        " of groups of " + std::to_string(group) + " exceeds 2^31 words per element");
    }
    return T;
}

std::vector<unsigned> firstPlanes(unsigned planes)
{
    std::vector<unsigned> js(planes);
    for (unsigned j = 0; j < planes; ++j)
        js[j] = j;
    return js;
}

// The planes js of the number of ones among every element's `group` inputs.  in: one batch, the grouped layout (input i
// of element q is element q * group + i), or `group` batches of one element count, the plane layout.  Every size
// first; then one csgn_count for uniform inputs of one term count, else the definition through the batch operators.
std::vector<CiphertextBatch> countPlanes(const std::vector<CiphertextBatch> &in, uint64_t group,
                                         const std::vector<unsigned> &js, const char *who)
{
    const std::string name = std::string("certFHE::") + who;
    const Context &ctx = in[0].context();
    const bool grouped = in.size() == 1;
    const uint64_t count = grouped ? in[0].size() / group : in[0].size();
    std::vector<CiphertextBatch> out;
    if (count == 0) {
        for (size_t x = 0; x < js.size(); ++x)
            out.push_back(BatchAccess::make(ctx, 0, 1));
        return out;
    }
    const Planes p(in);
    uint64_t t = 0;
    bool one_t = true;
    for (size_t i = 0; i < p.terms.size(); ++i) {
        one_t = one_t && p.terms[i] == p.terms[0];
        t = p.terms[i] > t ? p.terms[i] : t;
    }
    // sizes, from the largest term count: a bound for every element of a ragged or mixed operand
    const std::vector<uint64_t> T = countSizes(ctx, group, t, js, who);
    const CiphertextBatch zero = constantBatch(ctx, std::vector<unsigned char>(count, 0));
    out.assign(js.size(), zero);
    if (p.uniform && one_t) {
        std::vector<uint64_t> h_js, Ts;
        std::vector<size_t> at;
        for (size_t x = 0; x < js.size(); ++x) {
            if (T[x] == 0)
                continue;
            if (grouped && js[x] == 0) {
                out[x] = in[0].sumGroups(group);                 // a sum is a concatenation: the same payload
                continue;
            }
            h_js.push_back(js[x]);
            Ts.push_back(T[x]);
            at.push_back(x);
        }
        if (h_js.empty())
            return out;
        std::vector<CiphertextBatch> made = makePlanes(ctx, count, Ts);
        detail::check(csgn_count(ctx.getN(), count, group, t, sources(p).data(), in.size(), h_js.size(), h_js.data(),
                                 wordsOf(made).data(), detail::stream()),
                      "csgn_count");
        for (size_t k = 0; k < at.size(); ++k)
            out[at[k]] = made[k];
        return out;
    }
    // ragged or mixed: the definition itself, from gather, operator* and sumGroups over one grouped batch
    const CiphertextBatch all = grouped ? in[0] : CiphertextBatch::concat(in);
    for (size_t x = 0; x < js.size(); ++x)
        if (T[x] != 0 && count >= (1ull << 32) / csgn_count_terms(group, 1, js[x]))      // count * C(group, 2^j)
            throw std::invalid_argument(name + ": ragged operands of 2^32 products or more");
    for (size_t x = 0; x < js.size(); ++x) {
        if (T[x] == 0)
            continue;
        if (grouped && js[x] == 0) {
            out[x] = in[0].sumGroups(group);
            continue;
        }
        const uint64_t m = 1ull << js[x], ncomb = csgn_count_terms(group, 1, js[x]);
        std::vector<std::vector<uint64_t> > idx(m, std::vector<uint64_t>(count * ncomb));
        std::vector<uint64_t> s(m);
        for (uint64_t q = 0; q < count; ++q) {
            for (uint64_t k = 0; k < m; ++k)
                s[k] = k;
            for (uint64_t c = 0; c < ncomb; ++c) {
                for (uint64_t k = 0; k < m; ++k)
                    idx[k][q * ncomb + c] = grouped ? q * group + s[k] : s[k] * count + q;
                uint64_t k = m - 1;                              // the successor in lexicographic order
                while (k > 0 && s[k] == group - m + k)
                    --k;
                ++s[k];
                for (uint64_t i = k + 1; i < m; ++i)
                    s[i] = s[i - 1] + 1;
            }
        }
        CiphertextBatch prod = all.gather(idx[0]);
        for (uint64_t k = 1; k < m; ++k)
            prod = prod * all.gather(idx[k]);
        out[x] = prod.sumGroups(ncomb);
    }
    return out;
}

void requirePlanes(unsigned planes, const char *who)
{
    if (planes < 1 || planes > 64)
        throw std::invalid_argument(std::string("certFHE::") + who + ": planes must be 1..64");
}

void requireGroup(const CiphertextBatch &bits, uint64_t group, const char *who)
{
    if (group == 0 || bits.size() % group != 0)
        throw std::invalid_argument(std::string("certFHE::") + who + ": groups of " + std::to_string(group) +
                                    " in a batch of " + std::to_string(bits.size()));
}

} // namespace

UIntBatch countOnes(const CiphertextBatch &bits, uint64_t group, unsigned planes)
{
    requirePlanes(planes, "countOnes");
    requireGroup(bits, group, "countOnes");
    return UIntBatch::fromPlanes(countPlanes(std::vector<CiphertextBatch>(1, bits), group, firstPlanes(planes), "countOnes"));
}

CiphertextBatch countBit(const CiphertextBatch &bits, uint64_t group, unsigned j)
{
    requireGroup(bits, group, "countBit");
    return countPlanes(std::vector<CiphertextBatch>(1, bits), group, std::vector<unsigned>(1, j), "countBit")[0];
}

// the planes of a are the plane layout's inputs (a width of 1: the one plane is a grouped batch of groups of 1)
UIntBatch popcount(const UIntBatch &a, unsigned planes)
{
    requirePlanes(planes, "popcount");
    return UIntBatch::fromPlanes(countPlanes(planesOf(a), a.width(), firstPlanes(planes), "popcount"));
}

CiphertextBatch popcountBit(const UIntBatch &a, unsigned j)
{
    return countPlanes(planesOf(a), a.width(), std::vector<unsigned>(1, j), "popcountBit")[0];
}

UIntBatch hammingDistance(const UIntBatch &a, const UIntBatch &b, unsigned planes)
{
    requirePlanes(planes, "hammingDistance");
    requireSame(a, b, "hammingDistance");
    uint64_t t = 0;                                              // of a ^ b, before it is computed
    for (unsigned j = 0; j < a.width() && a.size(); ++j)
        t = std::max(t, termsOf(a.plane(j)) + termsOf(b.plane(j)));
    if (a.size())
        countSizes(a.context(), a.width(), t, firstPlanes(planes), "hammingDistance");
    return popcount(a ^ b, planes);
}

UIntBatch countMatches(const UIntBatch &keys, const UIntBatch &query, unsigned planes)
{
    requirePlanes(planes, "countMatches");
    const Context &ctx = query.context();
    const uint64_t v = keys.width(), rows = keys.size(), m = query.size();
    if (!sameContext(keys.context(), ctx))
        throw std::invalid_argument("certFHE::countMatches: the keys and the query differ in context");
    if (query.width() != v)
        throw std::invalid_argument("certFHE::countMatches: the keys and the query differ in width");
    if (rows == 0)
        throw std::invalid_argument("certFHE::countMatches: the table has no rows");
    // sizes first: an equality has P = prod_k (u_k + s_k + 1) terms, plane j then C(rows, 2^j) * P^(2^j)
    const Planes y(keys), x(query);
    unsigned long long P = 1;
    for (uint64_t k = 0; k < v; ++k)
        if (__builtin_mul_overflow(P, (unsigned long long)(y.terms[k] + x.terms[k] + 1), &P) || P >= kMaxWords)
            throw std::invalid_argument("certFHE::countMatches: an equality exceeds 2^31 words per element");
    for (unsigned j = 0; j < planes && j <= 6 && (1ull << j) <= rows && m; ++j) {
        const uint64_t T = csgn_count_terms(rows, P, j);
        if (T == 0 || T > (kMaxWords - 1) / ctx.getDefaultN())
            throw std::invalid_argument("certFHE::countMatches: plane " + std::to_string(j) + " of " +
                                        std::to_string(rows) + " rows exceeds 2^31 words per element");
    }
    if (m == 0)
        return UIntBatch::fromPlanes(std::vector<CiphertextBatch>(planes, BatchAccess::make(ctx, 0, 1)));
    if (m >= (1ull << 32) / rows)
        throw std::invalid_argument("certFHE::countMatches: 2^32 comparisons or more");
    std::vector<uint64_t> ik(m * rows), iq(m * rows);
    for (uint64_t e = 0; e < m; ++e)
        for (uint64_t r = 0; r < rows; ++r) {
            ik[e * rows + r] = r;
            iq[e * rows + r] = e;
        }
    const CiphertextBatch eq = equalTo(keys.gather(ik), query.gather(iq));
    return UIntBatch::fromPlanes(countPlanes(std::vector<CiphertextBatch>(1, eq), rows, firstPlanes(planes), "countMatches"));
}

// ------------------------------------------------------------------ running counts (csgn_count_prefix)

namespace {

bool prefixCall(bool uniform_operands) { return uniform_operands; }

// rows[r][x]: plane js[x] of the number of ones among the first r + 1 - exclusive inputs of every element (countPlanes'
// layouts).  Every size first; then one csgn_count_prefix for uniform inputs of one term count -- one block a plane, the
// rows views into it --, else the definition row by row: the gathered prefix through countPlanes.
std::vector<std::vector<CiphertextBatch> > prefixPlanes(const std::vector<CiphertextBatch> &in, uint64_t group,
                                                        const std::vector<unsigned> &js, bool exclusive, const char *who)
{
    const std::string name = std::string("certFHE::") + who;
    const Context &ctx = in[0].context();
    const bool grouped = in.size() == 1;
    const uint64_t count = grouped ? in[0].size() / group : in[0].size(), ex = exclusive ? 1 : 0, dl = ctx.getDefaultN();
    std::vector<std::vector<CiphertextBatch> > rows(group);
    if (count == 0) {
        for (uint64_t r = 0; r < group; ++r)
            rows[r].assign(js.size(), BatchAccess::make(ctx, 0, 1));
        return rows;
    }
    const Planes p(in);
    uint64_t t = 0;
    bool one_t = true;
    for (size_t i = 0; i < p.terms.size(); ++i) {
        one_t = one_t && p.terms[i] == p.terms[0];
        t = p.terms[i] > t ? p.terms[i] : t;
    }
    // sizes, of the last row, the longest, and from the largest term count: a bound for every row and element
    const std::vector<uint64_t> T = countSizes(ctx, group - ex, t, js, who);
    const CiphertextBatch zero = constantBatch(ctx, std::vector<unsigned char>(count, 0));
    for (uint64_t r = 0; r < group; ++r)
        rows[r].assign(js.size(), zero);
    if (prefixCall(p.uniform && one_t)) {
        std::vector<uint64_t> h_js, words;
        std::vector<size_t> at;
        for (size_t x = 0; x < js.size(); ++x) {
            if (T[x] == 0)
                continue;
            const uint64_t A = csgn_count_prefix_offset(group, t, js[x], ex, group);
            unsigned long long w;
            if (A == 0 || __builtin_mul_overflow((unsigned long long)count, (unsigned long long)A, &w) ||
                __builtin_mul_overflow(w, (unsigned long long)dl, &w) || w >= (1ull << 60))
                throw std::invalid_argument(name + ": plane " + std::to_string(js[x]) + " of the rows of groups of " +
                                            std::to_string(group) + " exceeds 2^60 words");
            h_js.push_back(js[x]);
            words.push_back(w);
            at.push_back(x);
        }
        if (h_js.empty())
            return rows;
        std::vector<std::shared_ptr<detail::DevicePayload> > blocks;
        std::vector<uint64_t *> dst;
        for (size_t k = 0; k < h_js.size(); ++k) {
            blocks.push_back(detail::allocWords(words[k]));
            dst.push_back(blocks[k]->data());
        }
        detail::check(csgn_count_prefix(ctx.getN(), count, group, t, ex, sources(p).data(), in.size(), h_js.size(),
                                        h_js.data(), dst.data(), detail::stream()),
                      "csgn_count_prefix");
        for (size_t k = 0; k < at.size(); ++k)
            for (uint64_t r = 0; r < group; ++r) {
                const uint64_t off = csgn_count_prefix_offset(group, t, h_js[k], ex, r);
                const uint64_t next = csgn_count_prefix_offset(group, t, h_js[k], ex, r + 1);
                if (r + 1 - ex >= (1ull << h_js[k]))             // a shorter row keeps the ZERO of constantBatch
                    rows[r][at[k]] = BatchAccess::makeView(ctx, count, next - off, blocks[k], count * off * dl);
            }
        return rows;
    }
    // ragged or mixed: the definition itself, the count of the gathered prefix row by row
    for (uint64_t r = 0; r < group; ++r) {
        const uint64_t nr = r + 1 - ex;
        if (nr == 0)
            continue;
        if (grouped) {
            std::vector<uint64_t> idx(count * nr);
            for (uint64_t q = 0; q < count; ++q)
                for (uint64_t i = 0; i < nr; ++i)
                    idx[q * nr + i] = q * group + i;
            rows[r] = countPlanes(std::vector<CiphertextBatch>(1, in[0].gather(idx)), nr, js, who);
        } else {
            rows[r] = countPlanes(std::vector<CiphertextBatch>(in.begin(), in.begin() + nr), nr, js, who);
        }
    }
    return rows;
}

std::vector<UIntBatch> asIntegers(const std::vector<std::vector<CiphertextBatch> > &rows)
{
    std::vector<UIntBatch> out;
    out.reserve(rows.size());
    for (size_t r = 0; r < rows.size(); ++r)
        out.push_back(UIntBatch::fromPlanes(rows[r]));
    return out;
}

} // namespace

std::vector<UIntBatch> runningCount(const CiphertextBatch &bits, uint64_t group, unsigned planes, bool exclusive)
{
    requirePlanes(planes, "runningCount");
    requireGroup(bits, group, "runningCount");
    return asIntegers(prefixPlanes(std::vector<CiphertextBatch>(1, bits), group, firstPlanes(planes), exclusive,
                                   "runningCount"));
}

std::vector<CiphertextBatch> runningCountBit(const CiphertextBatch &bits, uint64_t group, unsigned j, bool exclusive)
{
    requireGroup(bits, group, "runningCountBit");
    const std::vector<std::vector<CiphertextBatch> > rows =
        prefixPlanes(std::vector<CiphertextBatch>(1, bits), group, std::vector<unsigned>(1, j), exclusive, "runningCountBit");
    std::vector<CiphertextBatch> out;
    for (size_t r = 0; r < rows.size(); ++r)
        out.push_back(rows[r][0]);
    return out;
}

// the planes of a are the plane layout's inputs (a width of 1: the one plane is a grouped batch of groups of 1)
std::vector<UIntBatch> prefixPopcount(const UIntBatch &a, unsigned planes, bool exclusive)
{
    requirePlanes(planes, "prefixPopcount");
    return asIntegers(prefixPlanes(planesOf(a), a.width(), firstPlanes(planes), exclusive, "prefixPopcount"));
}

const char *runningCountRoute(uint64_t group, bool uniform_operands)
{
    return group != 0 && prefixCall(uniform_operands) ? "csgn_count_prefix" : "loop";
}

// ------------------------------------------------------------------ sums of integers (csgn_wsum)

namespace {

// does plane j have a count vector: can the classes make up 2^j?  Taking all a class can give, heaviest first, settles
// it (what is left is a multiple of every lighter weight)
bool planeHasVector(const std::vector<uint64_t> &n, unsigned j)
{
    if (j > 62)
        return false;
    uint64_t rest = 1ull << j;
    for (size_t c = std::min<size_t>(j, n.size() - 1) + 1; c-- > 0 && rest;)
        rest -= std::min<uint64_t>(n[c], rest >> c) << c;
    return rest == 0;
}

// Terms per element of the planes js for classes of n[c] inputs of t terms; 0: the plane has no count vector, it is
// ZERO.  Throws past 2^31 words.
std::vector<uint64_t> wsumSizes(const Context &ctx, const std::vector<uint64_t> &n, uint64_t t,
                                const std::vector<unsigned> &js, const char *who)
{
    uint64_t all = 0;
    for (size_t c = 0; c < n.size(); ++c)
        all = n[c] > 65536 ? 65537 : all + n[c];
    if (n.empty() || n.size() > 64 || all > 65536)
        throw std::invalid_argument(std::string("certFHE::") + who + ": more than 65536 partial products an element");
    std::vector<uint64_t> T(js.size(), 0);
    for (size_t x = 0; x < js.size(); ++x) {
        if (all == 0 || !planeHasVector(n, js[x]))
            continue;
        T[x] = csgn_wsum_terms(n.size(), n.data(), t, js[x]);
        if (T[x] == 0 || T[x] > (kMaxWords - 1) / ctx.getDefaultN())
            throw std::invalid_argument(std::string("certFHE::") + who + ": plane " + std::to_string(js[x]) +
                                        " exceeds 2^31 words per element");
    }
    return T;
}

// device plans per (classes, t, planes), kept until the process ends
const csgn_wsum_plan *wsumPlan(const std::vector<uint64_t> &n, uint64_t t, const std::vector<uint64_t> &js)
{
    static std::mutex mutex;
    static std::map<std::vector<uint64_t>, csgn_wsum_plan *> *plans = new std::map<std::vector<uint64_t>, csgn_wsum_plan *>();
    std::vector<uint64_t> key(1, t);
    key.push_back(n.size());
    key.insert(key.end(), n.begin(), n.end());
    key.insert(key.end(), js.begin(), js.end());
    std::lock_guard<std::mutex> lock(mutex);
    auto it = plans->find(key);
    if (it != plans->end())
        return it->second;
    csgn_wsum_plan *p = nullptr;
    detail::check(csgn_wsum_create(n.size(), n.data(), t, js.size(), js.data(), &p), "csgn_wsum_create");
    (*plans)[key] = p;
    return p;
}

// the count vectors of plane j in the definition's order, m[c] for c = 0 .. j
void countVectors(const std::vector<uint64_t> &n, unsigned c, uint64_t rest, std::vector<uint64_t> &m,
                  std::vector<std::vector<uint64_t> > &out)
{
    const uint64_t nc = c < n.size() ? n[c] : 0;
    if (c == 0) {
        if (rest <= nc) {
            m[0] = rest;
            out.push_back(m);
        }
        return;
    }
    for (uint64_t k = 0; k <= std::min<uint64_t>(nc, rest >> c); ++k) {
        m[c] = k;
        countVectors(n, c - 1, rest - (k << c), m, out);
    }
}

// The planes js of the sum of every element's inputs: class c is cls[c], n[c] inputs of weight 2^c an element, input i
// of element q its element q * n[c] + i (n[c] = 0: cls[c] is not looked at).  T: wsumSizes of the largest term count.
// One csgn_wsum for uniform classes of one term count, else the definition through the batch operators.
std::vector<CiphertextBatch> wsumPlanes(const Context &ctx, uint64_t count, const std::vector<CiphertextBatch> &cls,
                                        const std::vector<uint64_t> &n, const std::vector<unsigned> &js,
                                        const std::vector<uint64_t> &T, const char *who)
{
    const std::string name = std::string("certFHE::") + who;
    std::vector<CiphertextBatch> out(js.size(), constantBatch(ctx, std::vector<unsigned char>(count, 0)));
    bool uniform = true;
    uint64_t t = 0;
    for (size_t c = 0; c < n.size(); ++c) {
        if (n[c] == 0)
            continue;
        uniform = uniform && cls[c].uniform() && (t == 0 || cls[c].terms() == t);
        t = cls[c].uniform() ? cls[c].terms() : t;
    }
    for (size_t x = 0; x < js.size(); ++x)
        if (T[x] != 0 && js[x] == 0)
            out[x] = cls[0].sumGroups(n[0]);                     // a sum is a concatenation: the same payload, no launch
    if (uniform) {
        std::vector<uint64_t> h_js, Ts;
        std::vector<size_t> at;
        for (size_t x = 0; x < js.size(); ++x) {
            if (T[x] == 0 || js[x] == 0)
                continue;
            h_js.push_back(js[x]);
            at.push_back(x);
        }
        if (h_js.empty())
            return out;
        const csgn_wsum_plan *plan = wsumPlan(n, t, h_js);
        for (size_t k = 0; k < h_js.size(); ++k)                 // the classes' own term count, not the bound T came from
            Ts.push_back(csgn_wsum_plan_terms(plan, k));
        std::vector<CiphertextBatch> made = makePlanes(ctx, count, Ts);
        std::vector<const uint64_t *> src(n.size(), nullptr);
        for (size_t c = 0; c < n.size(); ++c)
            if (n[c])
                src[c] = cls[c].deviceValues();
        detail::check(csgn_wsum(plan, ctx.getN(), count, src.data(), wordsOf(made).data(), detail::stream()), "csgn_wsum");
        for (size_t k = 0; k < at.size(); ++k)
            out[at[k]] = made[k];
        return out;
    }
    // ragged or mixed: the definition itself, vector by vector, from gather, operator*, sumGroups and operator+
    for (size_t x = 0; x < js.size(); ++x)                       // count * the selections of the plane's vectors
        if (T[x] != 0 && count >= (1ull << 32) / csgn_wsum_terms(n.size(), n.data(), 1, js[x]))
            throw std::invalid_argument(name + ": ragged operands of 2^32 products or more");
    for (size_t x = 0; x < js.size(); ++x) {
        if (T[x] == 0 || js[x] == 0)
            continue;
        std::vector<std::vector<uint64_t> > vectors;
        std::vector<uint64_t> m(js[x] + 1, 0);
        countVectors(n, js[x], 1ull << js[x], m, vectors);
        bool first = true;
        for (size_t v = 0; v < vectors.size(); ++v) {
            // the factors of a selection: classes descending, indices ascending; the odometer steps class 0 fastest
            std::vector<unsigned> fc;                            // class of factor k
            std::vector<uint64_t> sel;                           // its index within the class
            std::vector<size_t> start;                           // the first factor of its class
            for (unsigned c = js[x] + 1; c-- > 0;)
                for (uint64_t i = 0; i < vectors[v][c]; ++i) {
                    start.push_back(fc.size() - i);
                    fc.push_back(c);
                    sel.push_back(i);
                }
            const size_t deg = fc.size();
            std::vector<std::vector<uint64_t> > idx(deg);
            uint64_t found = 0;
            for (bool more = true; more; ++found) {
                for (size_t k = 0; k < deg; ++k)
                    idx[k].push_back(sel[k]);
                more = false;
                for (size_t k = deg; k-- > 0 && !more;) {        // the last factor that can still move up, class by class
                    const uint64_t c = fc[k], mc = vectors[v][c], pos = k - start[k];
                    if (sel[k] < n[c] - mc + pos) {
                        ++sel[k];
                        for (size_t i = k + 1; i < start[k] + mc; ++i)
                            sel[i] = sel[i - 1] + 1;
                        for (size_t i = start[k] + mc; i < deg; ++i)    // the lighter classes start over
                            sel[i] = i - start[i];
                        more = true;
                    }
                }
            }
            // selection s of element q: factor k is element q * n_c + sel of class c's batch
            CiphertextBatch prod = cls[0];
            for (size_t k = 0; k < deg; ++k) {
                std::vector<uint64_t> all(count * found);
                for (uint64_t q = 0; q < count; ++q)
                    for (uint64_t s = 0; s < found; ++s)
                        all[q * found + s] = q * n[fc[k]] + idx[k][s];
                const CiphertextBatch factor = cls[fc[k]].gather(all);
                prod = k == 0 ? factor : prod * factor;
            }
            const CiphertextBatch part = prod.sumGroups(found);
            out[x] = first ? part : out[x] + part;
            first = false;
        }
    }
    return out;
}

// the largest term count among the planes that take part: planes 0 .. planes - 1
uint64_t maxTerms(const UIntBatch &a, size_t planes)
{
    uint64_t t = 0;
    for (unsigned j = 0; j < a.width() && j < planes; ++j)
        t = std::max(t, termsOf(a.plane(j)));
    return t;
}

std::vector<CiphertextBatch> emptyPlanes(const Context &ctx, size_t planes)
{
    return std::vector<CiphertextBatch>(planes, BatchAccess::make(ctx, 0, 1));
}

std::vector<CiphertextBatch> sumPlanes(const UIntBatch &a, uint64_t group, const std::vector<unsigned> &js, const char *who)
{
    requireGroup(a.plane(0), group, who);
    if (a.size() == 0)
        return emptyPlanes(a.context(), js.size());
    // classes above the last plane never take part
    const std::vector<uint64_t> n(std::min<size_t>(a.width(), *std::max_element(js.begin(), js.end()) + 1), group);
    const std::vector<uint64_t> T = wsumSizes(a.context(), n, maxTerms(a, n.size()), js, who);
    return wsumPlanes(a.context(), a.size() / group, planesOf(a), n, js, T, who);
}

// The classes of sum_r a_r * b_r over every `group` consecutive elements, up to class `top`: class c holds, row r
// slowest, a_i * b_{c-i}, i ascending, a on the left; built from concat, gather and the batch operator*.
std::vector<CiphertextBatch> productClasses(const UIntBatch &a, const UIntBatch &b, uint64_t group, const std::vector<uint64_t> &n)
{
    const uint64_t size = a.size(), count = size / group;
    const CiphertextBatch L = CiphertextBatch::concat(planesOf(a)), R = CiphertextBatch::concat(planesOf(b));
    std::vector<CiphertextBatch> cls;
    for (size_t c = 0; c < n.size(); ++c) {
        std::vector<uint64_t> il, ir;
        for (uint64_t q = 0; q < count; ++q)
            for (uint64_t r = 0; r < group; ++r)
                for (uint64_t i = 0; i < a.width(); ++i)
                    if (c >= i && c - i < b.width()) {
                        il.push_back(i * size + q * group + r);
                        ir.push_back((c - i) * size + q * group + r);
                    }
        cls.push_back(n[c] ? L.gather(il) * R.gather(ir) : L.slice(0, 0));
    }
    return cls;
}

UIntBatch productPlanes(const UIntBatch &a, const UIntBatch &b, uint64_t group, unsigned planes, const char *who)
{
    requirePlanes(planes, who);
    if (a.size() != b.size() || !sameContext(a.context(), b.context()))
        throw std::invalid_argument(std::string("certFHE::") + who + ": operands differ in count or context");
    requireGroup(a.plane(0), group, who);
    const Context &ctx = a.context();
    if (a.size() == 0)
        return UIntBatch::fromPlanes(emptyPlanes(ctx, planes));
    // classes above the last plane never take part
    std::vector<uint64_t> n(std::min<size_t>(planes, a.width() + b.width() - 1), 0);
    for (size_t c = 0; c < n.size(); ++c)
        for (uint64_t i = 0; i < a.width(); ++i)
            n[c] += (c >= i && c - i < b.width()) ? group : 0;
    unsigned long long t;
    if (__builtin_mul_overflow((unsigned long long)maxTerms(a, n.size()), (unsigned long long)maxTerms(b, n.size()), &t) || t >= kMaxWords)
        throw std::invalid_argument(std::string("certFHE::") + who + ": a partial product exceeds 2^31 words per element");
    const std::vector<unsigned> js = firstPlanes(planes);
    const std::vector<uint64_t> T = wsumSizes(ctx, n, t, js, who);
    return UIntBatch::fromPlanes(wsumPlanes(ctx, a.size() / group, productClasses(a, b, group, n), n, js, T, who));
}

} // namespace

UIntBatch sumValues(const UIntBatch &a, uint64_t group, unsigned planes)
{
    requirePlanes(planes, "sumValues");
    return UIntBatch::fromPlanes(sumPlanes(a, group, firstPlanes(planes), "sumValues"));
}

CiphertextBatch sumBit(const UIntBatch &a, uint64_t group, unsigned j)
{
    return sumPlanes(a, group, std::vector<unsigned>(1, j), "sumBit")[0];
}

UIntBatch sumWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, unsigned planes)
{
    requirePlanes(planes, "sumWhere");
    requireSameBit(mask, values, "sumWhere");
    requireGroup(mask, group, "sumWhere");
    const Context &ctx = values.context();
    if (values.size() == 0)
        return UIntBatch::fromPlanes(emptyPlanes(ctx, planes));
    const std::vector<uint64_t> n(std::min<size_t>(values.width(), planes), group);       // classes above the last plane never take part
    unsigned long long t;
    if (__builtin_mul_overflow((unsigned long long)termsOf(mask), (unsigned long long)maxTerms(values, n.size()), &t) || t >= kMaxWords)
        throw std::invalid_argument("certFHE::sumWhere: a masked value exceeds 2^31 words per element");
    const std::vector<unsigned> js = firstPlanes(planes);
    const std::vector<uint64_t> T = wsumSizes(ctx, n, t, js, "sumWhere");
    std::vector<CiphertextBatch> low;
    for (size_t c = 0; c < n.size(); ++c)
        low.push_back(values.plane((unsigned)c));
    const std::vector<CiphertextBatch> cls = keepPlanes(mask, low, "sumWhere");
    return UIntBatch::fromPlanes(wsumPlanes(ctx, values.size() / group, cls, n, js, T, "sumWhere"));
}

UIntBatch mul(const UIntBatch &a, const UIntBatch &b, unsigned planes) { return productPlanes(a, b, 1, planes, "mul"); }

UIntBatch UIntBatch::operator*(const UIntBatch &rhs) const { return mul(*this, rhs, width()); }

UIntBatch innerProduct(const UIntBatch &a, const UIntBatch &b, uint64_t group, unsigned planes)
{
    return productPlanes(a, b, group, planes, "innerProduct");
}

// ------------------------------------------------------------------ the first row whose mask bit is set

namespace {

// Per shape (measured): the call for every group it takes.
bool firstCall(uint64_t group, bool uniform_operands) { return uniform_operands && group >= 1 && group <= 64; }

struct Priority {
    std::vector<CiphertextBatch> values, any, labels;    // one per value plane; none or one; one per label plane
};

// Of every element's `group` rows the first whose mask bit is set: its value planes, with want_any the OR of the mask
// and, with label_planes, planes 0 .. label_planes - 1 of its public label.  mask: one batch, the grouped layout (row r
// of element q is element q * group + r), or `group` batches of one element count, the plane layout; values: grouped.
// Every size first; then ONE csgn_uint_first for uniform operands, else the definition through the batch operators.
Priority priority(const std::vector<CiphertextBatch> &mask, uint64_t group, const std::vector<CiphertextBatch> &values,
                  bool want_any, const std::vector<uint64_t> &labels, unsigned label_planes, const char *who)
{
    const std::string name = std::string("certFHE::") + who;
    const Context &ctx = mask[0].context();
    const bool grouped = mask.size() == 1;
    if (group == 0 || group > 64 || (grouped && mask[0].size() % group != 0))
        throw std::invalid_argument(name + ": groups of " + std::to_string(group) + " (1..64) in a batch of " +
                                    std::to_string(mask[0].size()));
    const uint64_t count = grouped ? mask[0].size() / group : mask[0].size();
    for (size_t r = 0; r < mask.size(); ++r)
        if (!sameContext(mask[r].context(), ctx) || mask[r].size() != mask[0].size())
            throw std::invalid_argument(name + ": the mask rows differ in count or context");
    for (size_t j = 0; j < values.size(); ++j)
        if (!sameContext(values[j].context(), ctx) || values[j].size() != count * group)
            throw std::invalid_argument(name + ": the values differ from the mask in count or context");
    Priority out;
    if (count == 0) {
        out.values = emptyPlanes(ctx, values.size());
        out.any = emptyPlanes(ctx, want_any ? 1 : 0);
        out.labels = emptyPlanes(ctx, label_planes);
        return out;
    }
    // sizes, from the largest term count of a ragged operand: a bound for every element of it
    const Planes pm(mask), pv(values);
    std::vector<uint64_t> s(group);
    bool one_s = true;
    for (uint64_t r = 0; r < group; ++r) {
        s[r] = std::max<uint64_t>(pm.terms[grouped ? 0 : r], 1);
        one_s = one_s && s[r] == s[0];
    }
    const std::string too_large = name + ": an output exceeds 2^31 words per element (the group is too large or the mask "
                                         "has too many terms)";
    const uint64_t Q = values.empty() && !want_any ? 0 : csgn_uint_first_terms(group, s.data(), group);
    if ((!values.empty() || want_any) && (Q == 0 || Q >= kMaxWords))
        throw std::invalid_argument(too_large);
    std::vector<uint64_t> T(values.size() + (want_any ? 1 : 0)), Tlab, bits;
    for (size_t j = 0; j < T.size(); ++j) {
        const uint64_t tj = j < values.size() ? std::max<uint64_t>(pv.terms[j], 1) : 1;
        if (tj > kMaxWords / Q)
            throw std::invalid_argument(too_large);
        T[j] = checked(tj * Q, ctx, who);
    }
    std::vector<size_t> at;                                     // the label planes that exist
    for (unsigned i = 0; i < label_planes; ++i) {
        bool reached = false;
        for (uint64_t r = 0; r < group; ++r)
            reached = reached || ((labels[r] >> i) & 1u);
        if (!reached)
            continue;
        const uint64_t Ti = csgn_uint_first_label_terms(group, s.data(), labels.data(), i);
        if (Ti == 0 || Ti >= kMaxWords)
            throw std::invalid_argument(too_large);
        Tlab.push_back(checked(Ti, ctx, who));
        bits.push_back(i);
        at.push_back(i);
    }
    out.labels.assign(label_planes, constantBatch(ctx, std::vector<unsigned char>(count, 0)));
    const bool uniform = pm.uniform && pv.uniform && (!grouped || one_s);
    if (firstCall(group, uniform)) {
        std::vector<CiphertextBatch> made = makePlanes(ctx, count, T), lab = makePlanes(ctx, count, Tlab);
        std::vector<uint64_t *> dst = wordsOf(made);
        uint64_t *any = want_any ? dst.back() : nullptr;
        if (!T.empty() || !Tlab.empty())
            detail::check(csgn_uint_first(ctx.getN(), count, group, sources(pm).data(), mask.size(), s.data(), values.size(),
                                          sources(pv).data(), pv.terms.data(), dst.data(), any, bits.size(), labels.data(),
                                          bits.data(), wordsOf(lab).data(), detail::stream()),
                          "csgn_uint_first");
        if (want_any) {
            out.any.push_back(made.back());
            made.pop_back();
        }
        out.values = made;
        for (size_t k = 0; k < at.size(); ++k)
            out.labels[at[k]] = lab[k];
        return out;
    }
    // ragged: the definition itself through the batch operators, row by row
    std::vector<CiphertextBatch> lab(at.size(), mask[0]);
    std::vector<bool> started(at.size(), false);
    std::vector<uint64_t> idx(count);
    CiphertextBatch run = mask[0];
    for (uint64_t r = 0; r < group; ++r) {
        for (uint64_t q = 0; q < count; ++q)
            idx[q] = q * group + r;
        const CiphertextBatch m = grouped ? mask[0].gather(idx) : mask[r];
        const CiphertextBatch F = r == 0 ? m : run * m;
        if (r + 1 < group)
            run = r == 0 ? logicNot(m) : run * logicNot(m);
        for (size_t j = 0; j < values.size(); ++j) {
            const CiphertextBatch p = F * values[j].gather(idx);
            if (r == 0)
                out.values.push_back(p);
            else
                out.values[j] = out.values[j] + p;
        }
        if (want_any) {
            if (r == 0)
                out.any.push_back(F);
            else
                out.any[0] = out.any[0] + F;
        }
        for (size_t k = 0; k < at.size(); ++k) {
            if (!((labels[r] >> at[k]) & 1u))
                continue;
            lab[k] = started[k] ? lab[k] + F : F;
            started[k] = true;
        }
    }
    for (size_t k = 0; k < at.size(); ++k)
        out.labels[at[k]] = lab[k];
    return out;
}

std::vector<uint64_t> indexLabels(uint64_t group)
{
    std::vector<uint64_t> L(group);
    for (uint64_t r = 0; r < group; ++r)
        L[r] = r;
    return L;
}

// the planes of a as mask rows, bit 0 first (the plane layout; a width of 1: one grouped batch of groups of 1)
std::vector<CiphertextBatch> rowsOf(const UIntBatch &a, bool from_top)
{
    std::vector<CiphertextBatch> rows = planesOf(a);
    if (from_top)
        std::reverse(rows.begin(), rows.end());
    return rows;
}

} // namespace

const char *firstRoute(uint64_t group, bool uniform_operands) { return firstCall(group, uniform_operands) ? "call" : "loop"; }

UIntBatch firstWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, CiphertextBatch *any)
{
    const Priority p = priority(std::vector<CiphertextBatch>(1, mask), group, planesOf(values), any != nullptr,
                                std::vector<uint64_t>(), 0, "firstWhere");
    if (any)
        *any = p.any[0];
    return UIntBatch::fromPlanes(p.values);
}

CiphertextBatch firstWhere(const CiphertextBatch &mask, const CiphertextBatch &values, uint64_t group, CiphertextBatch *any)
{
    const Priority p = priority(std::vector<CiphertextBatch>(1, mask), group, std::vector<CiphertextBatch>(1, values),
                                any != nullptr, std::vector<uint64_t>(), 0, "firstWhere");
    if (any)
        *any = p.any[0];
    return p.values[0];
}

CiphertextBatch anyOf(const CiphertextBatch &bits, uint64_t group)
{
    return priority(std::vector<CiphertextBatch>(1, bits), group, std::vector<CiphertextBatch>(), true,
                    std::vector<uint64_t>(), 0, "anyOf").any[0];
}

UIntBatch firstIndex(const CiphertextBatch &mask, uint64_t group, unsigned planes, CiphertextBatch *any)
{
    requirePlanes(planes, "firstIndex");
    const Priority p = priority(std::vector<CiphertextBatch>(1, mask), group, std::vector<CiphertextBatch>(), any != nullptr,
                                indexLabels(std::min<uint64_t>(group, 64)), planes, "firstIndex");
    if (any)
        *any = p.any[0];
    return UIntBatch::fromPlanes(p.labels);
}

UIntBatch lowestSetIndex(const UIntBatch &a, unsigned planes, CiphertextBatch *nonzero)
{
    requirePlanes(planes, "lowestSetIndex");
    const Priority p = priority(rowsOf(a, false), a.width(), std::vector<CiphertextBatch>(), nonzero != nullptr,
                                indexLabels(a.width()), planes, "lowestSetIndex");
    if (nonzero)
        *nonzero = p.any[0];
    return UIntBatch::fromPlanes(p.labels);
}

UIntBatch lowestSetBit(const UIntBatch &a)
{
    std::vector<uint64_t> L(a.width());
    for (unsigned r = 0; r < a.width(); ++r)
        L[r] = 1ull << r;
    return UIntBatch::fromPlanes(priority(rowsOf(a, false), a.width(), std::vector<CiphertextBatch>(), false, L, a.width(),
                                          "lowestSetBit").labels);
}

UIntBatch bitLength(const UIntBatch &a, unsigned planes)
{
    requirePlanes(planes, "bitLength");
    std::vector<uint64_t> L(a.width());
    for (unsigned r = 0; r < a.width(); ++r)
        L[r] = a.width() - r;
    return UIntBatch::fromPlanes(priority(rowsOf(a, true), a.width(), std::vector<CiphertextBatch>(), false, L, planes,
                                          "bitLength").labels);
}

// ------------------------------------------------------------------ the k-th row whose mask bit is set

namespace {

// Per shape (measured): the call for every group it takes.
bool nthCall(uint64_t group, bool uniform_operands) { return uniform_operands && group >= 1 && group <= 64; }

// Of every element's `group` rows the (slot + 1)-th whose mask bit is set: its value planes, with want_valid "more than
// slot bits are set" and, with label_planes, planes 0 .. label_planes - 1 of its public label (Priority's any holds
// valid).  mask: one batch, the grouped layout, or `group` batches of one element count, the plane layout; values:
// grouped.  Every size first (check_only: nothing else); then ONE csgn_uint_nth for uniform operands of one mask term
// count, else the definition through the batch operators.
Priority selectNth(const std::vector<CiphertextBatch> &mask, uint64_t group, uint64_t slot,
                   const std::vector<CiphertextBatch> &values, bool want_valid, const std::vector<uint64_t> &labels,
                   unsigned label_planes, const char *who, bool check_only = false)
{
    const std::string name = std::string("certFHE::") + who;
    const Context &ctx = mask[0].context();
    const bool grouped = mask.size() == 1;
    if (group == 0 || group > 64 || (grouped && mask[0].size() % group != 0))
        throw std::invalid_argument(name + ": groups of " + std::to_string(group) + " (1..64) in a batch of " +
                                    std::to_string(mask[0].size()));
    if (slot >= group)
        throw std::invalid_argument(name + ": slot " + std::to_string(slot) + " of a group of " + std::to_string(group));
    const uint64_t count = grouped ? mask[0].size() / group : mask[0].size();
    for (size_t r = 0; r < mask.size(); ++r)
        if (!sameContext(mask[r].context(), ctx) || mask[r].size() != mask[0].size())
            throw std::invalid_argument(name + ": the mask rows differ in count or context");
    for (size_t j = 0; j < values.size(); ++j)
        if (!sameContext(values[j].context(), ctx) || values[j].size() != count * group)
            throw std::invalid_argument(name + ": the values differ from the mask in count or context");
    Priority out;
    if (count == 0) {
        out.values = emptyPlanes(ctx, values.size());
        out.any = emptyPlanes(ctx, want_valid ? 1 : 0);
        out.labels = emptyPlanes(ctx, label_planes);
        return out;
    }
    // sizes, from the largest term count of any row and of a ragged operand: a bound for every element
    const Planes pm(mask), pv(values);
    uint64_t tm = 1;
    bool one_t = true;
    for (size_t r = 0; r < mask.size(); ++r) {
        tm = std::max(tm, pm.terms[r]);
        one_t = one_t && pm.terms[r] == pm.terms[0];
    }
    const std::string too_large = name + ": an output exceeds 2^31 words per element (the group is too large for the "
                                         "slot or the mask has too many terms)";
    const uint64_t Q = csgn_uint_nth_terms(group, tm, slot, group);
    if (Q == 0 || Q >= kMaxWords)
        throw std::invalid_argument(too_large);
    checked(Q, ctx, who);                                       // the stream itself, whatever is asked for
    std::vector<uint64_t> T(values.size() + (want_valid ? 1 : 0)), Tlab, bits;
    for (size_t j = 0; j < T.size(); ++j) {
        const uint64_t tj = j < values.size() ? std::max<uint64_t>(pv.terms[j], 1) : 1;
        if (tj > kMaxWords / Q)
            throw std::invalid_argument(too_large);
        T[j] = checked(tj * Q, ctx, who);
    }
    std::vector<size_t> at;                                     // the label planes that exist
    for (unsigned i = 0; i < label_planes; ++i) {
        bool reached = false;
        for (uint64_t r = slot; r < group; ++r)
            reached = reached || ((labels[r] >> i) & 1u);
        if (!reached)
            continue;
        const uint64_t Ti = csgn_uint_nth_label_terms(group, tm, slot, labels.data(), i);
        if (Ti == 0 || Ti >= kMaxWords)
            throw std::invalid_argument(too_large);
        Tlab.push_back(checked(Ti, ctx, who));
        bits.push_back(i);
        at.push_back(i);
    }
    if (check_only)
        return out;
    out.labels.assign(label_planes, constantBatch(ctx, std::vector<unsigned char>(count, 0)));
    if (nthCall(group, pm.uniform && pv.uniform && one_t)) {
        std::vector<CiphertextBatch> made = makePlanes(ctx, count, T), lab = makePlanes(ctx, count, Tlab);
        std::vector<uint64_t *> dst = wordsOf(made);
        uint64_t *valid = want_valid ? dst.back() : nullptr;
        if (!T.empty() || !Tlab.empty())
            detail::check(csgn_uint_nth(ctx.getN(), count, group, slot, sources(pm).data(), mask.size(), tm, values.size(),
                                        sources(pv).data(), pv.terms.data(), dst.data(), valid, bits.size(), labels.data(),
                                        bits.data(), wordsOf(lab).data(), detail::stream()),
                          "csgn_uint_nth");
        if (want_valid) {
            out.any.push_back(made.back());
            made.pop_back();
        }
        out.values = made;
        for (size_t k = 0; k < at.size(); ++k)
            out.labels[at[k]] = lab[k];
        return out;
    }
    // ragged operands or rows of different term counts: the definition itself through the batch operators
    std::vector<CiphertextBatch> rows;                          // m_r
    std::vector<uint64_t> idx(count);
    for (uint64_t r = 0; r < group; ++r) {
        for (uint64_t q = 0; q < count; ++q)
            idx[q] = q * group + r;
        rows.push_back(grouped ? mask[0].gather(idx) : mask[r]);
    }
    std::vector<CiphertextBatch> lab(at.size(), mask[0]);
    std::vector<bool> started(at.size(), false);
    bool first_row = true;
    for (uint64_t r = slot; r < group; ++r, first_row = false) {
        CiphertextBatch G = rows[r];
        bool first_term = true;
        for (uint64_t d = slot; d <= r; ++d) {
            if ((slot & ~d) != 0)                               // C(d, slot) is even
                continue;
            std::vector<uint64_t> sub(d);                       // the d-subsets of the rows below r, lexicographic
            for (uint64_t k = 0; k < d; ++k)
                sub[k] = k;
            for (bool more = true; more;) {
                CiphertextBatch p = d == 0 ? rows[r] : rows[sub[0]];
                for (uint64_t k = 1; k < d; ++k)
                    p = p * rows[sub[k]];
                if (d != 0)
                    p = p * rows[r];
                G = first_term ? p : G + p;
                first_term = false;
                more = false;
                for (uint64_t k = d; k-- > 0;)
                    if (sub[k] != r - d + k) {                  // the last position that can still move up
                        ++sub[k];
                        for (uint64_t i = k + 1; i < d; ++i)
                            sub[i] = sub[i - 1] + 1;
                        more = true;
                        break;
                    }
            }
        }
        for (uint64_t q = 0; q < count; ++q)
            idx[q] = q * group + r;
        for (size_t j = 0; j < values.size(); ++j) {
            const CiphertextBatch p = G * values[j].gather(idx);
            if (first_row)
                out.values.push_back(p);
            else
                out.values[j] = out.values[j] + p;
        }
        if (want_valid) {
            if (first_row)
                out.any.push_back(G);
            else
                out.any[0] = out.any[0] + G;
        }
        for (size_t k = 0; k < at.size(); ++k) {
            if (!((labels[r] >> at[k]) & 1u))
                continue;
            lab[k] = started[k] ? lab[k] + G : G;
            started[k] = true;
        }
    }
    for (size_t k = 0; k < at.size(); ++k)
        out.labels[at[k]] = lab[k];
    return out;
}

} // namespace

const char *nthRoute(uint64_t group, bool uniform_operands) { return nthCall(group, uniform_operands) ? "call" : "loop"; }

UIntBatch nthWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, uint64_t slot, CiphertextBatch *valid)
{
    const Priority p = selectNth(std::vector<CiphertextBatch>(1, mask), group, slot, planesOf(values), valid != nullptr,
                                 std::vector<uint64_t>(), 0, "nthWhere");
    if (valid)
        *valid = p.any[0];
    return UIntBatch::fromPlanes(p.values);
}

CiphertextBatch nthWhere(const CiphertextBatch &mask, const CiphertextBatch &values, uint64_t group, uint64_t slot,
                         CiphertextBatch *valid)
{
    const Priority p = selectNth(std::vector<CiphertextBatch>(1, mask), group, slot, std::vector<CiphertextBatch>(1, values),
                                 valid != nullptr, std::vector<uint64_t>(), 0, "nthWhere");
    if (valid)
        *valid = p.any[0];
    return p.values[0];
}

std::vector<UIntBatch> takeWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, uint64_t k,
                                 std::vector<CiphertextBatch> *valid)
{
    if (k == 0 || k > group)
        throw std::invalid_argument("certFHE::takeWhere: " + std::to_string(k) + " rows of groups of " +
                                    std::to_string(group));
    const std::vector<CiphertextBatch> m(1, mask), v = planesOf(values);
    for (uint64_t s = 0; s < k; ++s)                            // every slot's sizes before the first launch
        selectNth(m, group, s, v, valid != nullptr, std::vector<uint64_t>(), 0, "takeWhere", true);
    std::vector<UIntBatch> out;
    if (valid)
        valid->clear();
    for (uint64_t s = 0; s < k; ++s) {
        const Priority p = selectNth(m, group, s, v, valid != nullptr, std::vector<uint64_t>(), 0, "takeWhere");
        out.push_back(UIntBatch::fromPlanes(p.values));
        if (valid)
            valid->push_back(p.any[0]);
    }
    return out;
}

UIntBatch nthIndex(const CiphertextBatch &mask, uint64_t group, uint64_t slot, unsigned planes, CiphertextBatch *valid)
{
    requirePlanes(planes, "nthIndex");
    const Priority p = selectNth(std::vector<CiphertextBatch>(1, mask), group, slot, std::vector<CiphertextBatch>(),
                                 valid != nullptr, indexLabels(std::min<uint64_t>(group, 64)), planes, "nthIndex");
    if (valid)
        *valid = p.any[0];
    return UIntBatch::fromPlanes(p.labels);
}

UIntBatch nthSetIndex(const UIntBatch &a, uint64_t slot, unsigned planes, CiphertextBatch *valid)
{
    requirePlanes(planes, "nthSetIndex");
    const Priority p = selectNth(rowsOf(a, false), a.width(), slot, std::vector<CiphertextBatch>(), valid != nullptr,
                                 indexLabels(a.width()), planes, "nthSetIndex");
    if (valid)
        *valid = p.any[0];
    return UIntBatch::fromPlanes(p.labels);
}

CiphertextBatch atLeast(const CiphertextBatch &bits, uint64_t group, uint64_t k)
{
    const std::vector<CiphertextBatch> m(1, bits);
    if (k == 0 || k > group) {                                  // a public answer: ONE, or ZERO; the group is still checked
        if (group == 0 || group > 64 || bits.size() % group != 0)
            throw std::invalid_argument("certFHE::atLeast: groups of " + std::to_string(group) + " (1..64) in a batch of " +
                                        std::to_string(bits.size()));
        if (bits.size() == 0)
            return emptyPlanes(bits.context(), 1)[0];
        return constantBatch(bits.context(), std::vector<unsigned char>(bits.size() / group, k == 0 ? 1 : 0));
    }
    return selectNth(m, group, k - 1, std::vector<CiphertextBatch>(), true, std::vector<uint64_t>(), 0, "atLeast").any[0];
}

CiphertextBatch popcountAtLeast(const UIntBatch &a, uint64_t k)
{
    if (a.size() == 0)
        return emptyPlanes(a.context(), 1)[0];
    if (k == 0 || k > a.width())
        return constantBatch(a.context(), std::vector<unsigned char>(a.size(), k == 0 ? 1 : 0));
    return selectNth(rowsOf(a, false), a.width(), k - 1, std::vector<CiphertextBatch>(), true, std::vector<uint64_t>(), 0,
                     "popcountAtLeast").any[0];
}

} // namespace certFHE
