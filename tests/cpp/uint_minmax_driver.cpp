// uint_minmax_driver.cpp -- user-style C++ over min / max / minMax / selectLess / compareExchange of
// include/certfhe/UInt.h: selection by an encrypted comparison (tests/test_uint_minmax_cpp.py builds and runs it).
//   uint_minmax_driver words     widths 1, 4 and 8 at N=1247, ties included: words == select(lessThan(a, b), ...) bit for
//                                bit, decryptions == the plaintext min, max and payloads; null outputs are skipped
//   uint_minmax_driver ragged    compacted (ragged) operands take the composed route: the same words as the definition
//                                and the same decryptions
//   uint_minmax_driver oversize  width 16 with 3-term planes throws before anything is allocated; mismatched widths,
//                                counts and contexts throw; an empty batch is empty
//   uint_minmax_driver forms     "<shape> -> <form>": the form csgn_uint_lt_select_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Case {
    unsigned w, pw;
    size_t count;
};
const Case kCases[] = {{1, 2, 40}, {4, 3, 200}, {8, 2, 6}, {4, 1, 3}, {2, 8, 1000}};

struct Plain {
    std::vector<uint64_t> a, b, pa, pb, lo, hi, plo, phi;
};

// every third element a tie; a tie takes the second operand
Plain draw(const Case &c)
{
    Plain p;
    for (size_t i = 0; i < c.count; ++i) {
        const uint64_t a = rnd(c.w), b = i % 3 == 0 ? a : rnd(c.w), pa = rnd(c.pw), pb = pa ^ 1u;
        const bool less = a < b;
        p.a.push_back(a);
        p.b.push_back(b);
        p.pa.push_back(pa);
        p.pb.push_back(pb);
        p.lo.push_back(less ? a : b);
        p.hi.push_back(less ? b : a);
        p.plo.push_back(less ? pa : pb);
        p.phi.push_back(less ? pb : pa);
    }
    return p;
}

// every entry point against select(lessThan(a, b), ...), and against the plaintext when `p` is given
void checkAll(const SecretKey &key, const UIntBatch &a, const UIntBatch &b, const UIntBatch &pa, const UIntBatch &pb,
              const Plain *p, const std::string &tag)
{
    const CiphertextBatch l = lessThan(a, b);
    const UIntBatch wlo = select(l, a, b), whi = select(l, b, a), wplo = select(l, pa, pb), wphi = select(l, pb, pa);
    const UIntBatch mn = min(a, b), mx = max(a, b);
    expect(sameWords(mn, wlo), "min == select(lessThan)" + tag);
    expect(sameWords(mx, whi), "max == select(lessThan)" + tag);
    const std::pair<UIntBatch, UIntBatch> mm = minMax(a, b);
    expect(sameWords(mm.first, wlo) && sameWords(mm.second, whi), "minMax == (min, max)" + tag);
    expect(sameWords(selectLess(a, b, pa, pb), wplo), "selectLess == select(lessThan)" + tag);
    expect(sameBatchWords(selectLess(a, b, pa.plane(0), pb.plane(0)), logicMux(l, pa.plane(0), pb.plane(0))),
           "selectLess of bits == logicMux" + tag);
    UIntBatch lo = a, hi = a, plo = pa, phi = pa;
    compareExchange(a, b, pa, pb, &lo, &hi, &plo, &phi);
    expect(sameWords(lo, wlo) && sameWords(hi, whi), "compareExchange keys" + tag);
    expect(sameWords(plo, wplo) && sameWords(phi, wphi), "compareExchange payloads" + tag);
    UIntBatch hi2 = a, plo2 = pa;
    compareExchange(a, b, pa, pb, nullptr, &hi2, &plo2, nullptr);
    expect(sameWords(hi2, whi) && sameWords(plo2, wplo), "compareExchange with null outputs" + tag);
    compareExchange(a, b, pa, pb, nullptr, nullptr, nullptr, nullptr);
    if (p) {
        checkValues(mn.decrypt(key), p->lo, "min" + tag);
        checkValues(mx.decrypt(key), p->hi, "max" + tag);
        checkValues(lo.decrypt(key), p->lo, "lo" + tag);
        checkValues(hi.decrypt(key), p->hi, "hi" + tag);
        checkValues(plo.decrypt(key), p->plo, "plo" + tag);
        checkValues(phi.decrypt(key), p->phi, "phi" + tag);
    }
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (const Case &c : kCases) {
        const Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 30 + c.count), b = UIntBatch::encrypt(key, p.b, c.w, 31 + c.count);
        const UIntBatch pa = UIntBatch::encrypt(key, p.pa, c.pw, 32 + c.count), pb = UIntBatch::encrypt(key, p.pb, c.pw, 33 + c.count);
        checkAll(key, a, b, pa, pb, &p, " w=" + std::to_string(c.w) + " count=" + std::to_string(c.count));
    }
    // multi-term planes (sums with a trivial ZERO): the multi-term path, the same values
    const Case c = {3, 2, 50};
    const Plain p = draw(c);
    const UIntBatch a0 = UIntBatch::encrypt(key, p.a, c.w, 40), b0 = UIntBatch::encrypt(key, p.b, c.w, 41);
    const UIntBatch pa = UIntBatch::encrypt(key, p.pa, c.pw, 42), pb = UIntBatch::encrypt(key, p.pb, c.pw, 43);
    const UIntBatch zero = UIntBatch::constant(ctx, std::vector<uint64_t>(c.count, 0), c.w);
    checkAll(key, a0 ^ zero, b0, pa, pb, &p, " multi-term a");
    checkAll(key, a0, b0 ^ zero, pa ^ UIntBatch::constant(ctx, std::vector<uint64_t>(c.count, 0), c.pw), pb, &p, " multi-term b and pa");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 4; ++w) {
        const Case c = {w, 2, 60};
        Plain p = draw(c);
        const UIntBatch a0 = UIntBatch::encrypt(key, p.a, w, 50 + w), b0 = UIntBatch::encrypt(key, p.b, w, 60 + w);
        const UIntBatch pa0 = UIntBatch::encrypt(key, p.pa, 2, 70 + w), pb0 = UIntBatch::encrypt(key, p.pb, 2, 80 + w);
        // plane + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO
        // twice, which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
        auto raggedOf = [&](const UIntBatch &x) {
            std::vector<unsigned char> q0(x.size(), 0), q1(x.size(), 0);
            q0[0] = 1;
            std::vector<CiphertextBatch> pr;
            for (unsigned j = 0; j < x.width(); ++j)
                pr.push_back(addPlain(addPlain(x.plane(j), q0), q1).compact());
            return UIntBatch::fromPlanes(pr);
        };
        const std::string tag = " w=" + std::to_string(w);
        const UIntBatch ar = raggedOf(a0), par = raggedOf(pa0);
        expect(!ar.plane(0).uniform() && !par.plane(0).uniform(), "compact() gave ragged planes" + tag);
        // element 0 of a ragged operand has every bit flipped
        auto redo = [&](Plain q) {
            for (size_t i = 0; i < q.a.size(); ++i) {
                const bool less = q.a[i] < q.b[i];
                q.lo[i] = less ? q.a[i] : q.b[i];
                q.hi[i] = less ? q.b[i] : q.a[i];
                q.plo[i] = less ? q.pa[i] : q.pb[i];
                q.phi[i] = less ? q.pb[i] : q.pa[i];
            }
            return q;
        };
        Plain pk = p, pp = p;
        pk.a[0] ^= (1ull << w) - 1;
        pp.pa[0] ^= 3;
        const Plain wk = redo(pk), wp = redo(pp);
        checkAll(key, ar, b0, pa0, pb0, &wk, " ragged a" + tag);
        checkAll(key, a0, b0, par, pb0, &wp, " ragged pa" + tag);
        checkAll(key, b0, ar, pb0, pa0, nullptr, " ragged b" + tag);
    }
    return 0;
}

// 16-bit integers of 3 terms a plane at N=1247: about 7^16 terms.  The size check comes first, so the call throws
// std::invalid_argument at once, before any allocation or launch.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 1000;
    std::vector<uint64_t> x(count);
    for (size_t i = 0; i < count; ++i)
        x[i] = rnd(16);
    const UIntBatch x0 = UIntBatch::encrypt(key, x, 16, 1);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < 16; ++j)
        planes.push_back((x0.plane(j) + x0.plane(j)) + x0.plane(j));
    const UIntBatch wide = UIntBatch::fromPlanes(planes);
    const UIntBatch pay = UIntBatch::encrypt(key, std::vector<uint64_t>(count, 3), 2, 2);
    UIntBatch lo = pay, plo = pay;
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { min(wide, wide); });
    thrown += throws<std::invalid_argument>([&] { max(wide, x0); });
    thrown += throws<std::invalid_argument>([&] { minMax(x0, wide); });
    thrown += throws<std::invalid_argument>([&] { selectLess(wide, wide, pay, pay); });
    thrown += throws<std::invalid_argument>([&] { selectLess(wide, wide, pay.plane(0), pay.plane(1)); });
    thrown += throws<std::invalid_argument>([&] { compareExchange(wide, wide, pay, pay, &lo, nullptr, &plo, nullptr); });
    thrown += throws<std::invalid_argument>([&] { selectLess(x0, x0, wide, wide); });     // 3^16 * 6 terms an output
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 7, "oversize throws (" + std::to_string(thrown) + " of 7)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // widths, counts, contexts
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    const UIntBatch b5 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 5, 4);
    const UIntBatch p2 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 1), 2, 5);
    const UIntBatch p3 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 1), 3, 6);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o4 = UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 1), 4, 7);
    UIntBatch out = a4;
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { min(a4, b5); });                                     // widths
    thrown += throws<std::invalid_argument>([&] { max(a4, a4.slice(0, 9)); });                         // counts
    thrown += throws<std::invalid_argument>([&] { minMax(a4, o4); });                                  // contexts
    thrown += throws<std::invalid_argument>([&] { selectLess(a4, a4, p2, p3); });                      // payload widths
    thrown += throws<std::invalid_argument>([&] { selectLess(a4, a4, p2.slice(0, 9), p2.slice(0, 9)); });
    thrown += throws<std::invalid_argument>([&] { selectLess(a4, a4, o4, o4); });
    thrown += throws<std::invalid_argument>([&] { selectLess(a4, a4, p2.plane(0), o4.plane(0)); });
    thrown += throws<std::invalid_argument>([&] { compareExchange(a4, a4, p2, p3, &out, nullptr, nullptr, nullptr); });
    thrown += throws<std::invalid_argument>([&] { compareExchange(a4, b5, p2, p2, nullptr, nullptr, &out, nullptr); });
    expect(thrown == 9, "bad widths, counts and contexts throw (" + std::to_string(thrown) + " of 9)");
    // an empty batch: empty planes
    const UIntBatch e4 = a4.slice(0, 0), e2 = p2.slice(0, 0);
    UIntBatch hi = a4, phi = p2;
    compareExchange(e4, e4, e2, e2, nullptr, &hi, nullptr, &phi);
    expect(hi.width() == 4 && hi.size() == 0 && phi.width() == 2 && phi.size() == 0, "an empty batch gives empty planes");
    expect(min(e4, e4).size() == 0 && minMax(e4, e4).second.width() == 4, "an empty batch gives empty planes (min)");
    return 0;
}

// No device work: the form csgn_uint_lt_select_kernel names for the shapes of words (fresh planes, a whole
// compare-exchange), under the knob the process was started with.
int forms()
{
    for (const Case &c : kCases) {
        const unsigned n_out = 2 * c.w + 2 * c.pw;
        const std::vector<uint64_t> one(std::max(16u, n_out), 1);
        const char *form = csgn_uint_lt_select_kernel(1247, c.count, c.w, one.data(), one.data(), n_out, one.data(), one.data(), 0);
        expect(form && *form, "the selection has a form");
        printf("w=%u outputs=%u count=%zu -> %s\n", c.w, n_out, c.count, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4722, "uint_minmax_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
