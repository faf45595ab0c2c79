// uint_bitwise_driver.cpp -- user-style C++ over a & b, a | b, a ^ b, ~a, a ^ k, select, keepWhere, hammingDistance and
// sumWhere of include/certfhe/UInt.h (tests/test_uint_bitwise_cpp.py builds and runs it).
//   uint_bitwise_driver words     widths 1, 3, 8, 32 and 64 at N=1247, fresh integers and computed ones (a + b: planes of
//                                 different term counts), selectors of one and of several terms: words == the
//                                 CiphertextBatch operators and Gates.h plane by plane, decryptions == the clear values
//   uint_bitwise_driver ragged    compact()ed (ragged) operands take the old route: the same words and values
//   uint_bitwise_driver oversize  planes whose results pass 2^31 words throw before anything is allocated; mismatched
//                                 widths, counts and contexts throw; an empty batch is empty
//   uint_bitwise_driver forms     "<shape> -> <route> <form>": the route the classes take (bitwiseRoute) and the form
//                                 csgn_uint_bitwise_kernel names, under the process's knobs
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Case {
    unsigned w;
    size_t count;
};
const Case kCases[] = {{1, 40}, {3, 1000}, {8, 256}, {32, 7}, {64, 3}};

std::vector<uint64_t> draw(unsigned w, size_t count)
{
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = rnd(w);
    return v;
}

uint64_t maskOf(unsigned w) { return w == 64 ? ~0ull : (1ull << w) - 1; }

template <typename F>
std::vector<uint64_t> clear(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b, const std::vector<unsigned char> &s,
                            F f)
{
    std::vector<uint64_t> v(a.size());
    for (size_t i = 0; i < a.size(); ++i)
        v[i] = f(a[i], b[i], s[i]);
    return v;
}

// plane by plane through the CiphertextBatch operators and Gates.h: what the class operators were before the one call
template <typename F>
UIntBatch perPlane(const UIntBatch &a, F f)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < a.width(); ++j)
        planes.push_back(f(j));
    return UIntBatch::fromPlanes(planes);
}

// every operator against the per-plane composition, and against the clear values when va is given
void checkAll(const SecretKey &key, const UIntBatch &a, const UIntBatch &b, const CiphertextBatch &sel,
              const std::vector<uint64_t> *va, const std::vector<uint64_t> *vb, const std::vector<unsigned char> *vs,
              const std::string &tag)
{
    const unsigned w = a.width();
    const uint64_t m = maskOf(w);
    const UIntBatch x_and = a & b, x_or = a | b, x_xor = a ^ b, x_not = ~a, x_sel = select(sel, a, b), x_keep = keepWhere(sel, a);
    expect(sameWords(x_and, perPlane(a, [&](unsigned j) { return a.plane(j) * b.plane(j); })), "a & b == a_j * b_j" + tag);
    expect(sameWords(x_or, perPlane(a, [&](unsigned j) { return logicOr(a.plane(j), b.plane(j)); })), "a | b == logicOr" + tag);
    expect(sameWords(x_xor, perPlane(a, [&](unsigned j) { return a.plane(j) + b.plane(j); })), "a ^ b == a_j + b_j" + tag);
    expect(sameWords(x_not, perPlane(a, [&](unsigned j) { return logicNot(a.plane(j)); })), "~a == logicNot" + tag);
    expect(sameWords(x_sel, perPlane(a, [&](unsigned j) { return logicMux(sel, a.plane(j), b.plane(j)); })),
           "select == logicMux" + tag);
    expect(sameWords(x_keep, perPlane(a, [&](unsigned j) { return sel * a.plane(j); })), "keepWhere == mask * a_j" + tag);
    const uint64_t k = rnd(w);
    const UIntBatch x_k = a ^ k;
    expect(sameWords(x_k, perPlane(a, [&](unsigned j) { return (k >> j) & 1u ? logicNot(a.plane(j)) : a.plane(j); })),
           "a ^ k == logicNot where k_j" + tag);
    for (unsigned j = 0; j < w; ++j)
        if (!((k >> j) & 1u))
            expect(x_k.plane(j).deviceValues() == a.plane(j).deviceValues(), "a ^ k: a kept plane shares the payload" + tag);
    expect(sameWords(a ^ 0, a) && (a ^ 0).plane(0).deviceValues() == a.plane(0).deviceValues(), "a ^ 0 is a" + tag);
    if (!va)
        return;
    const std::vector<uint64_t> &A = *va, &B = *vb;
    const std::vector<unsigned char> &S = *vs;
    checkValues(x_and.decrypt(key), clear(A, B, S, [](uint64_t x, uint64_t y, int) { return x & y; }), "a & b" + tag);
    checkValues(x_or.decrypt(key), clear(A, B, S, [](uint64_t x, uint64_t y, int) { return x | y; }), "a | b" + tag);
    checkValues(x_xor.decrypt(key), clear(A, B, S, [](uint64_t x, uint64_t y, int) { return x ^ y; }), "a ^ b" + tag);
    checkValues(x_not.decrypt(key), clear(A, B, S, [m](uint64_t x, uint64_t, int) { return ~x & m; }), "~a" + tag);
    checkValues(x_sel.decrypt(key), clear(A, B, S, [](uint64_t x, uint64_t y, int s) { return s ? x : y; }), "select" + tag);
    checkValues(x_keep.decrypt(key), clear(A, B, S, [](uint64_t x, uint64_t, int s) { return s ? x : 0; }), "keepWhere" + tag);
    checkValues(x_k.decrypt(key), clear(A, B, S, [k](uint64_t x, uint64_t, int) { return x ^ k; }), "a ^ k" + tag);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (const Case &c : kCases) {
        const std::vector<uint64_t> va = draw(c.w, c.count), vb = draw(c.w, c.count);
        const std::vector<unsigned char> vs = randomBits(c.count);
        const UIntBatch a = UIntBatch::encrypt(key, va, c.w, 30 + c.count), b = UIntBatch::encrypt(key, vb, c.w, 31 + c.count);
        const CiphertextBatch sel = CiphertextBatch::encrypt(key, vs);
        checkAll(key, a, b, sel, &va, &vb, &vs, " w=" + std::to_string(c.w) + " count=" + std::to_string(c.count));
    }
    // the operands alias: a with itself, b = a rotated by one plane, the selector a plane of a
    const std::vector<uint64_t> v5 = draw(5, 30);
    const UIntBatch a5 = UIntBatch::encrypt(key, v5, 5, 50);
    std::vector<uint64_t> r5(30);
    std::vector<unsigned char> s5(30);
    for (size_t i = 0; i < 30; ++i) {
        r5[i] = ((v5[i] << 1) | (v5[i] >> 4)) & 31;
        s5[i] = (unsigned char)(v5[i] & 1);
    }
    checkAll(key, a5, a5, a5.plane(0), &v5, &v5, &s5, " a with itself");
    checkAll(key, a5, a5.rotateLeft(1), a5.plane(0), &v5, &r5, &s5, " a with a rotated");
    // computed integers: the planes of a + b have 2, 3, 5 and 9 terms; a selector of 8 terms (a 2-bit lessThan)
    const size_t n = 50;
    const std::vector<uint64_t> p = draw(4, n), q = draw(4, n);
    const UIntBatch p4 = UIntBatch::encrypt(key, p, 4, 60), q4 = UIntBatch::encrypt(key, q, 4, 61);
    const UIntBatch x = p4 + q4, y = q4 - 3;
    std::vector<uint64_t> vx(n), vy(n);
    std::vector<unsigned char> lt(n);
    for (size_t i = 0; i < n; ++i) {
        vx[i] = (p[i] + q[i]) & 15;
        vy[i] = (q[i] - 3) & 15;
        lt[i] = (unsigned char)((p[i] & 3) < (q[i] & 3));
    }
    const CiphertextBatch less = lessThan(UIntBatch::fromPlanes({p4.plane(0), p4.plane(1)}),
                                          UIntBatch::fromPlanes({q4.plane(0), q4.plane(1)}));
    expect(less.terms() == 8 && x.plane(3).terms() == 9, "the computed operands have the counts the case is about");
    checkAll(key, x, y, less, &vx, &vy, &lt, " computed planes");
    checkAll(key, y, x, p4.plane(2) + q4.plane(2), nullptr, nullptr, nullptr, " computed planes, a 2-term selector");
    // hammingDistance is popcount(a ^ b); sumWhere's classes are keepWhere's planes
    const std::vector<uint64_t> h1 = draw(6, 40), h2 = draw(6, 40);
    const UIntBatch g1 = UIntBatch::encrypt(key, h1, 6, 70), g2 = UIntBatch::encrypt(key, h2, 6, 71);
    const UIntBatch hd = hammingDistance(g1, g2, 2);
    expect(sameWords(hd, popcount(perPlane(g1, [&](unsigned j) { return g1.plane(j) + g2.plane(j); }), 2)),
           "hammingDistance == popcount of the per-plane sums");
    std::vector<uint64_t> hv(40);
    for (size_t i = 0; i < 40; ++i)
        hv[i] = (uint64_t)__builtin_popcountll(h1[i] ^ h2[i]) & 3;
    checkValues(hd.decrypt(key), hv, "hammingDistance");
    const std::vector<uint64_t> sv = draw(3, 24);
    const std::vector<unsigned char> sm = randomBits(24);
    const UIntBatch s3 = UIntBatch::encrypt(key, sv, 3, 80);
    const CiphertextBatch mask = CiphertextBatch::encrypt(key, sm);
    const UIntBatch sw = sumWhere(mask, s3, 4, 4);
    expect(sameWords(sw, sumValues(perPlane(s3, [&](unsigned j) { return mask * s3.plane(j); }), 4, 4)),
           "sumWhere == the sum of the masked planes");
    std::vector<uint64_t> want(6, 0);
    for (size_t i = 0; i < 24; ++i)
        want[i / 4] = (want[i / 4] + (sm[i] ? sv[i] : 0)) & 15;
    checkValues(sw.decrypt(key), want, "sumWhere");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 4; ++w) {
        const size_t count = 60;
        const std::vector<uint64_t> va = draw(w, count), vb = draw(w, count);
        const std::vector<unsigned char> vs = randomBits(count);
        const UIntBatch a0 = UIntBatch::encrypt(key, va, w, 50 + w), b0 = UIntBatch::encrypt(key, vb, w, 60 + w);
        const CiphertextBatch sel = CiphertextBatch::encrypt(key, vs);
        // plane + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO
        // twice, which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
        std::vector<unsigned char> q0(count, 0), q1(count, 0);
        q0[0] = 1;
        auto raggedOf = [&](const CiphertextBatch &x) { return addPlain(addPlain(x, q0), q1).compact(); };
        const UIntBatch ar = perPlane(a0, [&](unsigned j) { return raggedOf(a0.plane(j)); });
        const CiphertextBatch sr = raggedOf(sel);
        const std::string tag = " w=" + std::to_string(w);
        expect(!ar.plane(0).uniform() && !sr.uniform(), "compact() gave ragged planes" + tag);
        const std::vector<uint64_t> one(w, 1);
        expect(std::string(bitwiseRoute(CSGN_UINT_BITWISE_AND, 0, one, one, false)) == "planes",
               "a ragged operand takes the planes" + tag);
        std::vector<uint64_t> fa = va;                              // element 0 of a ragged operand has every bit flipped
        fa[0] ^= maskOf(w);
        std::vector<unsigned char> fs = vs;
        fs[0] ^= 1;
        checkAll(key, ar, b0, sel, &fa, &vb, &vs, " ragged a" + tag);
        checkAll(key, b0, ar, sel, &vb, &fa, &vs, " ragged b" + tag);
        checkAll(key, a0, b0, sr, &va, &vb, &fs, " ragged selector" + tag);
    }
    return 0;
}

// Planes of 2^14 terms at N=1247: a product of 2^28 terms of 20 words is past 2^31 words per element.  The size check
// comes first, so the call throws std::invalid_argument at once, before any allocation or launch.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 4;
    const UIntBatch x0 = UIntBatch::encrypt(key, draw(2, count), 2, 1);
    CiphertextBatch big = x0.plane(0);
    for (int i = 0; i < 14; ++i)
        big = big + big;
    expect(big.terms() == 16384, "the operand has 2^14 terms");
    const UIntBatch wide = UIntBatch::fromPlanes({x0.plane(0), big});
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { wide & wide; });
    thrown += throws<std::invalid_argument>([&] { wide | wide; });
    thrown += throws<std::invalid_argument>([&] { select(big, wide, x0); });
    thrown += throws<std::invalid_argument>([&] { keepWhere(big, wide); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 4, "oversize throws (" + std::to_string(thrown) + " of 4)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    expect((wide ^ wide).plane(1).terms() == 32768 && (~wide).plane(1).terms() == 16385, "what fits is computed");
    // widths, counts, contexts
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    const UIntBatch b5 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 5, 4);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o4 = UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 1), 4, 7);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { a4 & b5; });                                         // widths
    thrown += throws<std::invalid_argument>([&] { a4 | a4.slice(0, 9); });                             // counts
    thrown += throws<std::invalid_argument>([&] { a4 ^ o4; });                                         // contexts
    thrown += throws<std::invalid_argument>([&] { select(a4.plane(0), a4, b5); });
    thrown += throws<std::invalid_argument>([&] { select(o4.plane(0), a4, a4); });
    thrown += throws<std::invalid_argument>([&] { select(a4.plane(0).slice(0, 9), a4, a4); });
    thrown += throws<std::invalid_argument>([&] { keepWhere(o4.plane(0), a4); });
    thrown += throws<std::invalid_argument>([&] { keepWhere(a4.plane(0).slice(0, 9), a4); });
    thrown += throws<std::invalid_argument>([&] { a4 ^ 16; });                                         // the constant
    expect(thrown == 9, "bad widths, counts, contexts and constants throw (" + std::to_string(thrown) + " of 9)");
    // an empty batch: empty planes
    const UIntBatch e4 = a4.slice(0, 0);
    const CiphertextBatch es = a4.plane(0).slice(0, 0);
    expect((e4 & e4).size() == 0 && (e4 | e4).size() == 0 && (e4 ^ e4).size() == 0 && (~e4).size() == 0 && (e4 ^ 5).size() == 0,
           "an empty batch gives empty results");
    const UIntBatch ek = keepWhere(es, e4), esel = select(es, e4, e4);
    expect(ek.width() == 4 && ek.size() == 0 && esel.width() == 4 && esel.size() == 0, "an empty batch gives empty planes");
    return 0;
}

// No device work: the route of the classes and the form csgn_uint_bitwise_kernel names for the shapes of words, under
// the knobs the process was started with.
int forms()
{
    const char *names[] = {"and", "or", "xor", "not", "select", "keep"};
    const std::vector<uint64_t> none;
    for (const Case &c : kCases) {
        const std::vector<uint64_t> one(c.w, 1);
        for (int op = CSGN_UINT_BITWISE_AND; op <= CSGN_UINT_BITWISE_KEEP; ++op) {
            const bool with_b = op != CSGN_UINT_BITWISE_NOT && op != CSGN_UINT_BITWISE_KEEP;
            const char *form = csgn_uint_bitwise_kernel(1247, op, c.count, c.w, 1, one.data(), with_b ? one.data() : nullptr);
            expect(form && *form, "the operation has a form");
            printf("%s w=%u count=%zu -> %s %s\n", names[op - 1], c.w, c.count,
                   bitwiseRoute(op, 1, one, with_b ? one : none, true), form ? form : "");
        }
    }
    // the planes of a + b under an 8-term selector
    const std::vector<uint64_t> ta = {2, 3, 5, 9}, tb = {2, 3, 4, 6};
    for (int op = CSGN_UINT_BITWISE_AND; op <= CSGN_UINT_BITWISE_KEEP; ++op) {
        const char *form = csgn_uint_bitwise_kernel(1247, op, 50, 4, 8, ta.data(), tb.data());
        expect(form && *form, "the operation has a form");
        printf("%s computed w=4 count=50 -> %s %s\n", names[op - 1], bitwiseRoute(op, 8, ta, tb, true), form ? form : "");
    }
    expect(std::string(bitwiseRoute(CSGN_UINT_BITWISE_AND, 0, ta, tb, false)) == "planes", "ragged planes take the planes");
    expect(std::string(bitwiseRoute(CSGN_UINT_BITWISE_AND, 0, none, none, true)) == "planes", "no planes: no call");
    expect(std::string(bitwiseRoute(0, 1, ta, tb, true)) == "planes" && std::string(bitwiseRoute(7, 1, ta, tb, true)) == "planes",
           "an unknown op: no call");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 5131, "uint_bitwise_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
