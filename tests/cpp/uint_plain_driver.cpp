// uint_plain_driver.cpp -- user-style C++ over the public-constant comparisons of include/certfhe/UInt.h
// (tests/test_uint_plain_cpp.py builds and runs it).
//   uint_plain_driver ops       1..16-bit comparisons against edge and random constants: decryptions == clear
//                               comparisons, words == the definition composed from CiphertextBatch operators and Gates.h
//   uint_plain_driver ragged    compacted (ragged) planes: elements holding the same terms as the uniform planes give
//                               the same words; every word == the definition; decryptions == clear comparisons
//   uint_plain_driver oversize  a comparison past 2^31 words per element throws before anything is allocated
//   uint_plain_driver forms     "<shape> -> <form>" for the shapes of ops (fresh planes, the edge constants): the form
//                               csgn_uint_plain_kernel names under the knob the process was started with
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

enum Cmp { EQ, NE, LT, LE, GT, GE };
const char *kNames[] = {"equalTo", "notEqualTo", "lessThan", "lessEqual", "greaterThan", "greaterEqual"};

CiphertextBatch compare(Cmp c, const UIntBatch &a, uint64_t k)
{
    switch (c) {
    case EQ: return equalTo(a, k);
    case NE: return notEqualTo(a, k);
    case LT: return lessThan(a, k);
    case LE: return lessEqual(a, k);
    case GT: return greaterThan(a, k);
    default: return greaterEqual(a, k);
    }
}

bool clear(Cmp c, uint64_t v, uint64_t k)
{
    switch (c) {
    case EQ: return v == k;
    case NE: return v != k;
    case LT: return v < k;
    case LE: return v <= k;
    case GT: return v > k;
    default: return v >= k;
    }
}

// the definition of UInt.h, by hand from the batch operators and Gates.h
CiphertextBatch definition(Cmp c, const UIntBatch &a, uint64_t k)
{
    const unsigned w = a.width();
    const Cmp base = c == NE ? EQ : c == LE ? GT : c == GE ? LT : c;
    const uint64_t all = (1ull << w) - 1;
    CiphertextBatch r = a.plane(0);
    if ((base == LT && k == 0) || (base == GT && k == all)) {
        r = constantBatch(a.context(), std::vector<unsigned char>(a.size(), 0));
    } else if (base == EQ) {
        r = (k & 1) ? a.plane(0) : logicNot(a.plane(0));
        for (unsigned j = 1; j < w; ++j)
            r = r * (((k >> j) & 1) ? a.plane(j) : logicNot(a.plane(j)));
    } else if (base == LT) {
        unsigned m = 0;
        while (!((k >> m) & 1))
            ++m;
        r = logicNot(a.plane(m));
        for (unsigned j = m + 1; j < w; ++j)
            r = ((k >> j) & 1) ? (r * a.plane(j)) + logicNot(a.plane(j)) : r * logicNot(a.plane(j));
    } else {
        unsigned m = 0;
        while ((k >> m) & 1)
            ++m;
        r = a.plane(m);
        for (unsigned j = m + 1; j < w; ++j)
            r = ((k >> j) & 1) ? r * a.plane(j) : (r * logicNot(a.plane(j))) + a.plane(j);
    }
    return base != c ? logicNot(r) : r;
}

// the shapes of ops, shared with forms: widths 1..kMaxWidth, countOf(w) elements, the edge constants (ops adds a random
// constant and the first value)
const unsigned kMaxWidth = 16;
size_t countOf(unsigned w) { return w <= 8 ? 300 : 20; }

std::vector<uint64_t> edgeConstants(unsigned w)
{
    const uint64_t all = (1ull << w) - 1;
    return {0, 1, all, 1ull << (w - 1), all ^ 1, 0x5555 & all};
}

std::vector<uint64_t> constants(unsigned w, const std::vector<uint64_t> &v)
{
    std::vector<uint64_t> ks = edgeConstants(w);
    ks.push_back(rnd(w));
    ks.push_back(v[0]);
    return ks;
}

uint64_t termsOf(const CiphertextBatch &b) { return b.uniform() ? b.terms() : b.termsOf(0); }

void checkOne(Cmp c, const UIntBatch &a, uint64_t k, const SecretKey &key, const std::vector<uint64_t> &v, bool words,
              const std::string &tag)
{
    const CiphertextBatch got = compare(c, a, k);
    const std::vector<unsigned char> bits = got.decrypt(key);
    for (size_t i = 0; i < v.size(); ++i)
        if ((bits[i] & 1u) != (clear(c, v[i], k) ? 1u : 0u)) {
            expect(false, std::string(kNames[c]) + " k=" + std::to_string(k) + " v=" + std::to_string(v[i]) + tag);
            break;
        }
    if (words)
        expect(sameBatchWords(got, definition(c, a, k)), std::string(kNames[c]) + " words k=" + std::to_string(k) + tag);
}

int ops()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= kMaxWidth; ++w) {
        const size_t count = countOf(w);
        std::vector<uint64_t> v(count);
        for (size_t i = 0; i < count; ++i)
            v[i] = rnd(w);
        const UIntBatch a = UIntBatch::encrypt(key, v, w, 7 + w);
        for (uint64_t k : constants(w, v))
            for (int c = EQ; c <= GE; ++c) {
                // the hand-made definition runs level by level: kept to the small widths and results
                CiphertextBatch probe = compare((Cmp)c, a, k);
                const bool words = w <= 8 || termsOf(probe) <= 512;
                checkOne((Cmp)c, a, k, key, v, words, " w=" + std::to_string(w));
            }
        // the fresh-plane size of the issue: 2^(zeros of k) terms for equalTo
        expect(termsOf(equalTo(a, 0)) == (1ull << w), "equalTo(a, 0) terms w=" + std::to_string(w));
    }
    // argument checks: k >= 2^w
    const UIntBatch a = UIntBatch::encrypt(key, std::vector<uint64_t>(5, 3), 4, 1);
    bool caught = false;
    try {
        lessThan(a, 16);
    } catch (const std::invalid_argument &) {
        caught = true;
    }
    expect(caught, "k >= 2^w throws");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const size_t count = 200;
    for (unsigned w = 1; w <= 6; ++w) {
        std::vector<uint64_t> v(count);
        for (size_t i = 0; i < count; ++i)
            v[i] = rnd(w);
        const UIntBatch a0 = UIntBatch::encrypt(key, v, w, 40 + w);
        // plane j + x + y, compacted: element 0 keeps [a, ONE, ZERO] (its bit flips), every other element adds ZERO
        // twice, which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
        std::vector<unsigned char> x(count, 0), y(count, 0);
        x[0] = 1;
        std::vector<CiphertextBatch> pr;
        for (unsigned j = 0; j < w; ++j)
            pr.push_back(addPlain(addPlain(a0.plane(j), x), y).compact());
        expect(!pr[0].uniform(), "compact() gave a ragged plane");
        const UIntBatch a = UIntBatch::fromPlanes(pr);
        std::vector<uint64_t> vr = v;
        vr[0] ^= (1ull << w) - 1;
        for (uint64_t k : constants(w, v))
            for (int c = EQ; c <= GE; ++c) {
                const std::string tag = std::string(kNames[c]) + " k=" + std::to_string(k) + " w=" + std::to_string(w);
                const CiphertextBatch u = compare((Cmp)c, a0, k), r = compare((Cmp)c, a, k);
                bool same = true;
                for (uint64_t i = 1; i < count && same; ++i) {
                    const Ciphertext ci = u.at(i), ri = r.at(i);
                    same = ci.getLen() == ri.getLen() && memcmp(ci.getValues(), ri.getValues(), ci.getLen() * 8) == 0;
                }
                expect(same, "ragged words == uniform words " + tag);
                expect(sameBatchWords(r, definition((Cmp)c, a, k)), "ragged words == definition " + tag);
                const std::vector<unsigned char> bits = r.decrypt(key);
                for (size_t i = 0; i < count; ++i)
                    if ((bits[i] & 1u) != (clear((Cmp)c, vr[i], k) ? 1u : 0u)) {
                        expect(false, "ragged bits " + tag);
                        break;
                    }
            }
    }
    return 0;
}

// 32-bit values over 100 000 elements at N=1247: equalTo(a, 0) has 2^32 terms per element.  The size check comes
// first, so every call throws std::invalid_argument at once, before any allocation or launch.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 100000;
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = rnd(31);
    const UIntBatch a = UIntBatch::encrypt(key, v, 32, 1);
    const auto t0 = std::chrono::steady_clock::now();
    for (int c = EQ; c <= GE; ++c) {
        const uint64_t k = c == EQ || c == NE ? 0 : 1;      // 2^32 terms, and at least 2^31 for the others
        bool caught = false;
        try {
            compare((Cmp)c, a, k);
        } catch (const std::invalid_argument &) {
            caught = true;
        }
        expect(caught, std::string(kNames[c]) + " oversize throws");
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(s < 1.0, "the size checks ran before any launch (" + std::to_string(s) + " s)");
    return 0;
}

// No device work: the library's own answer to "which form does this call take".
int forms()
{
    const int cmps[] = {CSGN_UINT_PLAIN_EQ, CSGN_UINT_PLAIN_NE, CSGN_UINT_PLAIN_LT,
                        CSGN_UINT_PLAIN_LE, CSGN_UINT_PLAIN_GT, CSGN_UINT_PLAIN_GE};
    for (unsigned w = 1; w <= kMaxWidth; ++w) {
        const std::vector<uint64_t> terms(w, 1);
        for (uint64_t k : edgeConstants(w))
            for (int c = EQ; c <= GE; ++c) {
                const char *form = csgn_uint_plain_kernel(1247, cmps[c], countOf(w), w, k, terms.data());
                expect(form && *form, std::string(kNames[c]) + " has a form");
                printf("w=%u %s k=%llu -> %s\n", w, kNames[c], (unsigned long long)k, form ? form : "");
            }
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4711, "uint_plain_driver", {{"ops", ops}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
