// uint_addk_driver.cpp -- user-style C++ over the arithmetic with public constants, the bitwise operators and the shifts
// of include/certfhe/UInt.h (tests/test_uint_addk_cpp.py builds and runs it).
//   uint_addk_driver ops       every operator decrypts to its clear value for random integers at w = 8 and w = 32;
//                              a + 1 at w = 32 has 2-term planes; a + k's words == the definition composed from the
//                              CiphertextBatch operators (csgn_uint_addk's words)
//   uint_addk_driver ragged    compacted (ragged) planes: the same decryptions, words == the definition
//   uint_addk_driver errors    a constant past the width, mismatched operands and an oversize result throw
//                              std::invalid_argument before anything is allocated
//   uint_addk_driver shared    the planes a shift, a rotate or a constant mask keeps are the source's payloads
//   uint_addk_driver nodevice  without a GPU the classes throw
//   uint_addk_driver forms   "<shape> -> <form>": the form csgn_uint_addk_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

uint64_t maskOf(unsigned w) { return w == 64 ? ~0ull : (1ull << w) - 1; }

// the definition of include/csgn_hip.h (csgn_uint_addk), by hand from the batch operators
UIntBatch definition(const UIntBatch &a, uint64_t k, bool negate, std::vector<CiphertextBatch> *carry)
{
    const unsigned w = a.width();
    std::vector<CiphertextBatch> out;
    if (k == 0) {
        for (unsigned j = 0; j < w; ++j)
            out.push_back(negate ? logicNot(a.plane(j)) : a.plane(j));
        if (carry)
            carry->push_back(constantBatch(a.context(), std::vector<unsigned char>(a.size(), 0)));
        return UIntBatch::fromPlanes(out);
    }
    const unsigned m = (unsigned)__builtin_ctzll(k);
    CiphertextBatch c = a.plane(m);
    for (unsigned j = 0; j < w; ++j) {
        CiphertextBatch o = a.plane(j);
        if (j == m) {
            o = logicNot(o);
        } else if (j > m) {
            o = o + c;
            if ((k >> j) & 1u) {
                o = logicNot(o);
                c = (c * logicNot(a.plane(j))) + a.plane(j);
            } else {
                c = c * a.plane(j);
            }
        }
        out.push_back(negate ? logicNot(o) : o);
    }
    if (carry)
        carry->push_back(c);
    return UIntBatch::fromPlanes(out);
}

std::vector<uint64_t> randomValues(size_t count, unsigned w)
{
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = i == 0 ? 0 : i == 1 ? maskOf(w) : rnd(w);
    return v;
}

template <typename F>
std::vector<uint64_t> mapped(const std::vector<uint64_t> &x, unsigned w, F f)
{
    std::vector<uint64_t> r(x.size());
    for (size_t i = 0; i < x.size(); ++i)
        r[i] = f(x[i]) & maskOf(w);
    return r;
}

// ks: constants added; sub_ks: subtracted (a - k adds 2^w - k); rsub_ks: subtracted from (k - a adds ~k).  Over fresh
// planes the carry grows with the set bits of the constant ADDED, so the wide cases pick each list for that.
void checkOperators(const SecretKey &key, const UIntBatch &a, const UIntBatch &b, const std::vector<uint64_t> &x,
                    const std::vector<uint64_t> &y, const std::vector<uint64_t> &ks, const std::vector<uint64_t> &sub_ks,
                    const std::vector<uint64_t> &rsub_ks, bool negation, const std::string &tag)
{
    const unsigned w = a.width();
    for (uint64_t k : ks) {
        const std::string t = tag + " k=" + std::to_string(k);
        checkValues((a + k).decrypt(key), mapped(x, w, [&](uint64_t v) { return v + k; }), "a + k" + t);
        checkValues((a & k).decrypt(key), mapped(x, w, [&](uint64_t v) { return v & k; }), "a & k" + t);
        checkValues((a | k).decrypt(key), mapped(x, w, [&](uint64_t v) { return v | k; }), "a | k" + t);
        checkValues((a ^ k).decrypt(key), mapped(x, w, [&](uint64_t v) { return v ^ k; }), "a ^ k" + t);
        CiphertextBatch carry = a.plane(0);
        const UIntBatch s = a.add(k, &carry);
        checkValues(s.decrypt(key), mapped(x, w, [&](uint64_t v) { return v + k; }), "add(k, carry)" + t);
        const std::vector<unsigned char> cb = carry.decrypt(key);
        for (size_t i = 0; i < x.size(); ++i) {
            const bool left = w == 64 ? x[i] + k < x[i] : ((x[i] + k) >> w) != 0;
            if ((cb[i] & 1u) != (left ? 1u : 0u)) {
                expect(false, "carry-out" + t + " element " + std::to_string(i));
                break;
            }
        }
    }
    for (uint64_t k : sub_ks)
        checkValues((a - k).decrypt(key), mapped(x, w, [&](uint64_t v) { return v - k; }), "a - k" + tag + " k=" + std::to_string(k));
    for (uint64_t k : rsub_ks)
        checkValues((k - a).decrypt(key), mapped(x, w, [&](uint64_t v) { return k - v; }), "k - a" + tag + " k=" + std::to_string(k));
    if (negation)
        checkValues((-a).decrypt(key), mapped(x, w, [](uint64_t v) { return 0 - v; }), "-a" + tag);
    checkValues((~a).decrypt(key), mapped(x, w, [](uint64_t v) { return ~v; }), "~a" + tag);
    std::vector<uint64_t> ra(x.size());
    for (size_t e = 0; e < x.size(); ++e)
        ra[e] = x[e] & y[e];
    checkValues((a & b).decrypt(key), ra, "a & b" + tag);
    std::vector<uint64_t> ro(x.size()), rx(x.size());
    for (size_t e = 0; e < x.size(); ++e) {
        ro[e] = x[e] | y[e];
        rx[e] = x[e] ^ y[e];
    }
    checkValues((a | b).decrypt(key), ro, "a | b" + tag);
    checkValues((a ^ b).decrypt(key), rx, "a ^ b" + tag);
    const unsigned shifts[] = {0, 1, 3, w - 1, w, w + 5};
    for (unsigned s : shifts) {
        const std::string t = tag + " s=" + std::to_string(s);
        checkValues(a.shiftLeft(s).decrypt(key), mapped(x, w, [&](uint64_t v) { return s >= w ? 0 : v << s; }), "shiftLeft" + t);
        checkValues(a.shiftRight(s).decrypt(key), mapped(x, w, [&](uint64_t v) { return s >= w ? 0 : v >> s; }), "shiftRight" + t);
        const unsigned r = s % w;
        checkValues(a.rotateLeft(s).decrypt(key),
                    mapped(x, w, [&](uint64_t v) { return r ? (v << r) | (v >> (w - r)) : v; }), "rotateLeft" + t);
    }
}

// the constants ops adds, shared with forms: their carries stay small over fresh planes (few set bits above the lowest)
std::vector<uint64_t> addConstants(unsigned w)
{
    const uint64_t all = maskOf(w);
    return {0, 1, 2, 1ull << (w - 1), all & ~(all >> 6), 100, (1ull << (w - 1)) | 5};
}

int ops()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 64;
    for (unsigned w : {8u, 32u}) {
        const std::vector<uint64_t> x = randomValues(count, w), y = randomValues(count, w);
        const UIntBatch a = UIntBatch::encrypt(key, x, w, 100 + w), b = UIntBatch::encrypt(key, y, w, 200 + w);
        const std::string tag = " w=" + std::to_string(w);
        // constants whose carries stay small over fresh planes: few set bits above the lowest
        const uint64_t all = maskOf(w);
        std::vector<uint64_t> ks = addConstants(w);
        std::vector<uint64_t> sub_ks = {0, all, 1ull << (w - 1), all - 99}, rsub_ks = {all, all ^ 1, all ^ 100, all >> 1};
        if (w == 8) {
            ks.push_back(255);
            sub_ks = rsub_ks = ks;
        }
        checkOperators(key, a, b, x, y, ks, sub_ks, rsub_ks, w == 8, tag);
        // a + 1: two terms in every plane (a_j + a_0 * ... * a_{j-1}); one term in plane 0 plus ONE
        const UIntBatch inc = a + 1;
        for (unsigned j = 0; j < w; ++j)
            expect(inc.plane(j).uniform() && inc.plane(j).terms() == 2,
                   "a + 1: plane " + std::to_string(j) + " has " + std::to_string(inc.plane(j).terms()) + " terms" + tag);
        if (w == 8)                                        // a - 1 = a + (2^w - 1): plane j has 1 + (2^j - 1) + 1 terms
            for (unsigned j = 1; j < w; ++j)
                expect((a - 1).plane(j).terms() == (1ull << j) + 1, "a - 1: plane " + std::to_string(j) + " terms" + tag);
        // words: the class's planes and carry against the definition, a few elements
        const UIntBatch small = UIntBatch::encrypt(key, std::vector<uint64_t>(x.begin(), x.begin() + 5), w, 7);
        for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)100, (uint64_t)((1ull << (w - 1)) | 5)}) {
            std::vector<CiphertextBatch> want_carry;
            CiphertextBatch carry = small.plane(0);
            const UIntBatch got = small.add(k, &carry), want = definition(small, k, false, &want_carry);
            expect(sameWords(got, want), "a + k words == definition k=" + std::to_string(k) + tag);
            expect(sameBatchWords(carry, want_carry[0]), "carry words == definition k=" + std::to_string(k) + tag);
            expect(sameWords(small + k, want), "operator+ words == add's k=" + std::to_string(k) + tag);
            expect(sameWords((all ^ k) - small, definition(small, k, true, nullptr)),
                   "k - a words == definition k=" + std::to_string(all ^ k) + tag);
        }
        if (w == 8)
            expect(sameWords(-small, definition(small, all, true, nullptr)), "-a words == definition" + tag);
    }
    return 0;
}

// plane + p + q, compacted: element 0 keeps [a, ONE, ZERO] (its bit flips), every other element adds ZERO twice, which
// cancels: it holds exactly the uniform plane's term.  The planes are ragged.
UIntBatch raggedOf(const UIntBatch &a)
{
    std::vector<unsigned char> p(a.size(), 0), q(a.size(), 0);
    p[0] = 1;
    std::vector<CiphertextBatch> pr;
    for (unsigned j = 0; j < a.width(); ++j)
        pr.push_back(addPlain(addPlain(a.plane(j), p), q).compact());
    return UIntBatch::fromPlanes(pr);
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const size_t count = 60;
    for (unsigned w : {3u, 8u}) {
        std::vector<uint64_t> x = randomValues(count, w), y = randomValues(count, w);
        const UIntBatch a0 = UIntBatch::encrypt(key, x, w, 300 + w), b0 = UIntBatch::encrypt(key, y, w, 400 + w);
        const UIntBatch a = raggedOf(a0), b = raggedOf(b0);
        expect(!a.plane(0).uniform(), "compact() gave ragged planes");
        x[0] ^= maskOf(w);
        y[0] ^= maskOf(w);
        const std::string tag = " ragged w=" + std::to_string(w);
        const std::vector<uint64_t> ks = {0, 1, 5, 1ull << (w - 1), maskOf(w)};
        checkOperators(key, a, b, x, y, ks, ks, ks, true, tag);
        for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)6, maskOf(w)}) {
            std::vector<CiphertextBatch> want_carry;
            CiphertextBatch carry = a.plane(0);
            const UIntBatch got = a.add(k, &carry);
            expect(sameWords(got, definition(a, k, false, &want_carry)), "words == definition k=" + std::to_string(k) + tag);
            expect(sameBatchWords(carry, want_carry[0]), "carry words == definition k=" + std::to_string(k) + tag);
            expect(sameWords(k - a, definition(a, ~k & maskOf(w), true, nullptr)), "k - a words k=" + std::to_string(k) + tag);
            // elements 1.. hold the uniform planes' terms: the same words as the uniform route
            const UIntBatch u = a0 + k;
            for (unsigned j = 0; j < w; ++j) {
                bool same = true;
                for (uint64_t i = 1; i < count && same; ++i)
                    same = sameWords(u.plane(j).at(i), got.plane(j).at(i));
                expect(same, "ragged words == uniform words k=" + std::to_string(k) + tag);
            }
        }
    }
    return 0;
}

int errors()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const UIntBatch a = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 5), 4, 1);
    const UIntBatch wide = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 5), 5, 2);
    const UIntBatch longer = UIntBatch::encrypt(key, std::vector<uint64_t>(11, 5), 4, 3);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch foreign = UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 5), 4, 4);
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { a + 16; });
    thrown += throws<std::invalid_argument>([&] { a - 16; });
    thrown += throws<std::invalid_argument>([&] { 16 - a; });
    thrown += throws<std::invalid_argument>([&] { a.add(1ull << 40, nullptr); });
    thrown += throws<std::invalid_argument>([&] { a & 16; });
    thrown += throws<std::invalid_argument>([&] { a | 16; });
    thrown += throws<std::invalid_argument>([&] { a ^ 16; });
    expect(thrown == 7, "a constant past the width throws (" + std::to_string(thrown) + " of 7)");
    thrown = 0;
    for (const UIntBatch *b : {&wide, &longer, &foreign}) {
        thrown += throws<std::invalid_argument>([&] { a & *b; });
        thrown += throws<std::invalid_argument>([&] { a | *b; });
        thrown += throws<std::invalid_argument>([&] { a ^ *b; });
    }
    expect(thrown == 9, "mismatched operands throw (" + std::to_string(thrown) + " of 9)");
    // 32 fresh planes minus 1: the top plane's carry has 2^31 - 1 terms, past 2^31 words per element at N=1247.  The
    // size check comes first, so the call throws at once, before any allocation or launch.
    const UIntBatch big = UIntBatch::encrypt(key, std::vector<uint64_t>(1000, 77), 32, 5);
    const auto t0 = std::chrono::steady_clock::now();
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { big - 1; });
    thrown += throws<std::invalid_argument>([&] { -big; });
    thrown += throws<std::invalid_argument>([&] { CiphertextBatch c = big.plane(0); big.add(0xFFFFFFFFu, &c); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 3, "oversize throws (" + std::to_string(thrown) + " of 3)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    expect(!throws<std::invalid_argument>([&] { a + 15; }), "a + 15 fits");
    return 0;
}

int shared()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const unsigned w = 8;
    const UIntBatch a = UIntBatch::encrypt(key, randomValues(20, w), w, 9);
    for (unsigned s : {0u, 1u, 3u, 7u}) {
        const UIntBatch l = a.shiftLeft(s), r = a.shiftRight(s), o = a.rotateLeft(s);
        for (unsigned j = 0; j < w; ++j) {
            if (j >= s)
                expect(l.plane(j).deviceValues() == a.plane(j - s).deviceValues(), "shiftLeft shares plane payloads");
            else
                expect(l.plane(j).terms() == 1 && l.plane(j).deviceValues() != a.plane(j).deviceValues(), "shiftLeft fills ZERO");
            if (j + s < w)
                expect(r.plane(j).deviceValues() == a.plane(j + s).deviceValues(), "shiftRight shares plane payloads");
            expect(o.plane(j).deviceValues() == a.plane((j + w - s) % w).deviceValues(), "rotateLeft shares plane payloads");
        }
    }
    const UIntBatch m = a & 0xA5, o = a | 0xA5, x = a ^ 0xA5;
    for (unsigned j = 0; j < w; ++j) {
        const bool bit = (0xA5 >> j) & 1;
        expect((m.plane(j).deviceValues() == a.plane(j).deviceValues()) == bit, "a & k keeps the planes where k_j = 1");
        expect((o.plane(j).deviceValues() == a.plane(j).deviceValues()) == !bit, "a | k keeps the planes where k_j = 0");
        expect((x.plane(j).deviceValues() == a.plane(j).deviceValues()) == !bit, "a ^ k keeps the planes where k_j = 0");
        expect(m.plane(j).terms() == 1 && o.plane(j).terms() == 1 && x.plane(j).terms() == (bit ? 2u : 1u), "term counts");
    }
    return 0;
}

// no GPU: the classes throw (nothing is computed on the CPU)
int nodevice()
{
    bool thrown = false;
    try {
        Context ctx(127, 8);
        SecretKey key(ctx);
        const UIntBatch a = UIntBatch::encrypt(key, std::vector<uint64_t>(4, 3), 4, 1);
        (a + 1).decrypt(key);
    } catch (const std::exception &) {
        thrown = true;
    }
    expect(thrown, "without a GPU the classes throw");
    return 0;
}

// No device work: the form csgn_uint_addk_kernel names for the shapes of ops (64 elements at N=1247, fresh planes, with
// and without the carry-out) and for one shape past a launch's 2^32 lanes, under the knob the process was started with.
int forms()
{
    for (unsigned w : {8u, 32u}) {
        const std::vector<uint64_t> terms(w, 1);
        std::vector<uint64_t> ks = addConstants(w);
        if (w == 8)
            ks.push_back(255);
        for (uint64_t k : ks)
            for (int carry = 0; carry <= 1; ++carry) {
                const char *form = csgn_uint_addk_kernel(1247, 64, w, k, terms.data(), carry);
                expect(form && *form, "a + " + std::to_string(k) + " has a form");
                printf("w=%u k=%llu carry=%d -> %s\n", w, (unsigned long long)k, carry, form ? form : "");
            }
    }
    // a + (2^28 - 1) over fresh planes: plane j has 2^j + 1 terms, 2^28 terms of 20 words in all, past 2^32 lanes
    const std::vector<uint64_t> terms(28, 1);
    const char *form = csgn_uint_addk_kernel(1247, 1, 28, (1ull << 28) - 1, terms.data(), 0);
    printf("w=28 k=%llu carry=0 -> %s\n", (unsigned long long)((1ull << 28) - 1), form ? form : "");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4718, "uint_addk_driver",
                    {{"ops", ops}, {"ragged", ragged}, {"errors", errors}, {"shared", shared}, {"nodevice", nodevice}, {"forms", forms}});
}
