// count_driver.cpp -- user-style C++ over countOnes / countBit / popcount / popcountBit / hammingDistance / countMatches
// of include/certfhe/UInt.h: encrypted bits counted into encrypted integers (tests/test_count_cpp.py builds and runs it).
//   count_driver words     seeded encryptions, then every operation: words == the same thing composed here from gather,
//                          operator*, sumGroups and equalTo (and, for one element, from single Ciphertext operators in
//                          the nested loops of the definition); decryptions == the count modulo 2^planes
//   count_driver ragged    a compact()-ed (ragged) operand takes the composed path: the same words as the composition
//                          here, and decryptions alike
//   count_driver oversize  every bad argument throws std::invalid_argument before anything is allocated, an empty batch
//                          gives empty planes, and a later valid call still works
//   count_driver forms     "<shape> -> <form>": the form csgn_count_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

uint64_t ones(uint64_t v)
{
    uint64_t c = 0;
    for (; v; v &= v - 1)
        ++c;
    return c;
}

uint64_t maskOf(unsigned planes) { return planes >= 64 ? ~0ull : (1ull << planes) - 1; }

// the m-subsets of {0 .. g-1} in lexicographic order, m indices each
std::vector<std::vector<uint64_t> > subsets(uint64_t g, uint64_t m)
{
    std::vector<std::vector<uint64_t> > all;
    std::vector<uint64_t> s(m);
    for (uint64_t k = 0; k < m; ++k)
        s[k] = k;
    for (;;) {
        all.push_back(s);
        uint64_t k = m;
        while (k > 0 && s[k - 1] == g - m + (k - 1))
            --k;
        if (k == 0)
            return all;
        ++s[k - 1];
        for (uint64_t i = k; i < m; ++i)
            s[i] = s[i - 1] + 1;
    }
}

// Plane j of the count, composed: `all` holds input i of element q at q * g + i (grouped) or at i * count + q (the
// planes of an integer, concatenated).  ZERO where 2^j > g.
CiphertextBatch composedPlane(const CiphertextBatch &all, uint64_t count, uint64_t g, bool grouped, unsigned j)
{
    if (j > 6 || (1ull << j) > g)
        return constantBatch(all.context(), std::vector<unsigned char>(count, 0));
    const uint64_t m = 1ull << j;
    const std::vector<std::vector<uint64_t> > sub = subsets(g, m);
    std::vector<std::vector<uint64_t> > idx(m);
    for (uint64_t q = 0; q < count; ++q)
        for (size_t c = 0; c < sub.size(); ++c)
            for (uint64_t k = 0; k < m; ++k)
                idx[k].push_back(grouped ? q * g + sub[c][k] : sub[c][k] * count + q);
    CiphertextBatch prod = all.gather(idx[0]);
    for (uint64_t k = 1; k < m; ++k)
        prod = prod * all.gather(idx[k]);
    return prod.sumGroups(sub.size());
}

CiphertextBatch planesOf(const UIntBatch &a)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < a.width(); ++j)
        planes.push_back(a.plane(j));
    return CiphertextBatch::concat(planes);
}

// the definition by hand for ONE element: single ciphertexts in the nested loops
Ciphertext definition(const std::vector<Ciphertext> &x, uint64_t m)
{
    const std::vector<std::vector<uint64_t> > sub = subsets(x.size(), m);
    auto product = [&](size_t c) {
        Ciphertext prod = x[sub[c][0]];
        for (uint64_t k = 1; k < m; ++k)
            prod = prod * x[sub[c][k]];
        return prod;
    };
    Ciphertext acc = product(0);
    for (size_t c = 1; c < sub.size(); ++c)
        acc = acc + product(c);
    return acc;
}

void checkCount(const UIntBatch &got, const CiphertextBatch &all, uint64_t count, uint64_t g, bool grouped,
                const std::vector<uint64_t> &want, const SecretKey &key, const std::string &tag)
{
    expect(got.size() == count, tag + ": elements");
    for (unsigned j = 0; j < got.width(); ++j)
        expect(sameBatchWords(got.plane(j), composedPlane(all, count, g, grouped, j)),
               tag + ": words of plane " + std::to_string(j) + " == the composition");
    std::vector<uint64_t> masked(want);
    for (size_t i = 0; i < masked.size(); ++i)
        masked[i] &= maskOf(got.width());
    checkValues(got.decrypt(key), masked, tag);
}

void checkBit(const CiphertextBatch &got, const CiphertextBatch &all, uint64_t count, uint64_t g, bool grouped, unsigned j,
              const std::vector<uint64_t> &want, const SecretKey &key, const std::string &tag)
{
    expect(sameBatchWords(got, composedPlane(all, count, g, grouped, j)), tag + ": words == the composition");
    const std::vector<unsigned char> bits = got.decrypt(key);
    expect(bits.size() == want.size(), tag + ": size");
    for (size_t i = 0; i < want.size() && i < bits.size(); ++i)
        if (bits[i] != ((want[i] >> j) & 1)) {
            expect(false, tag + " element " + std::to_string(i));
            return;
        }
}

std::vector<uint64_t> groupCounts(const std::vector<unsigned char> &bits, uint64_t g)
{
    std::vector<uint64_t> c(bits.size() / g, 0);
    for (size_t i = 0; i < bits.size(); ++i)
        c[i / g] += bits[i];
    return c;
}

UIntBatch twoTerms(const UIntBatch &a, const SecretKey &key, uint64_t seed)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < a.width(); ++j)
        planes.push_back(a.plane(j) + CiphertextBatch::encrypt(key, std::vector<unsigned char>(a.size(), 0), seed + j));
    return UIntBatch::fromPlanes(planes);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    // groups of 5 bits, fresh and of two terms: every pattern and more
    const uint64_t g = 5, count = 40;
    std::vector<unsigned char> bits(count * g);
    for (uint64_t q = 0; q < count; ++q)
        for (uint64_t i = 0; i < g; ++i)
            bits[q * g + i] = (unsigned char)((q < 32 ? q >> i : (uint64_t)rand()) & 1);
    const std::vector<uint64_t> want5 = groupCounts(bits, g);
    const CiphertextBatch b1 = CiphertextBatch::encrypt(key, bits, 11);
    const CiphertextBatch b2 = b1 + CiphertextBatch::encrypt(key, std::vector<unsigned char>(bits.size(), 0), 12);
    const CiphertextBatch *both[2] = {&b1, &b2};
    for (int v = 0; v < 2; ++v) {
        const CiphertextBatch &b = *both[v];
        const std::string tag = " g=5 t=" + std::to_string(v + 1);
        const UIntBatch c = countOnes(b, g, 4);                          // plane 3: 2^3 > 5, ZERO
        expect(c.width() == 4 && c.plane(1).terms() == 10 * b.terms() * b.terms(), "countOnes shapes" + tag);
        expect(c.plane(0).deviceValues() == b.deviceValues(), "plane 0 shares the payload" + tag);
        expect(c.plane(3).terms() == 1, "a plane past the group is the one-term ZERO" + tag);
        checkCount(c, b, count, g, true, want5, key, "countOnes" + tag);
        for (unsigned j = 0; j < 4; ++j)
            checkBit(countBit(b, g, j), b, count, g, true, j, want5, key, "countBit " + std::to_string(j) + tag);
        // one element against the nested loops over single ciphertexts
        std::vector<Ciphertext> x;
        for (uint64_t i = 0; i < g; ++i)
            x.push_back(b.at(7 * g + i));
        for (unsigned j = 0; j < 3; ++j)
            expect(sameWords(c.plane(j).at(7), definition(x, 1ull << j)), "plane " + std::to_string(j) + " == the nested loops" + tag);
    }
    // 8-bit integers: popcount, popcountBit, hammingDistance
    {
        std::vector<uint64_t> a(37), b(37), pa(37), hd(37);
        for (size_t i = 0; i < a.size(); ++i) {
            a[i] = i == 0 ? 0 : i == 1 ? 255 : rnd(8);
            b[i] = rnd(8);
            pa[i] = ones(a[i]);
            hd[i] = ones(a[i] ^ b[i]);
        }
        const UIntBatch ea = UIntBatch::encrypt(key, a, 8, 21), eb = UIntBatch::encrypt(key, b, 8, 22);
        const UIntBatch ea2 = twoTerms(ea, key, 23);
        checkCount(popcount(ea, 3), planesOf(ea), a.size(), 8, false, pa, key, "popcount w=8");
        checkCount(popcount(ea2, 2), planesOf(ea2), a.size(), 8, false, pa, key, "popcount w=8 t=2");
        checkBit(popcountBit(ea, 3), planesOf(ea), a.size(), 8, false, 3, pa, key, "popcountBit(a, 3) w=8");
        checkBit(popcountBit(ea, 4), planesOf(ea), a.size(), 8, false, 4, pa, key, "popcountBit(a, 4) w=8: ZERO");
        const UIntBatch x = ea ^ eb;
        checkCount(hammingDistance(ea, eb, 3), planesOf(x), a.size(), 8, false, hd, key, "hammingDistance w=8");
        expect(sameWords(hammingDistance(ea, eb, 2), popcount(x, 2)), "hammingDistance == popcount(a ^ b)");
        // a width of 1: the count is the bit
        const UIntBatch one = UIntBatch::fromPlanes(std::vector<CiphertextBatch>(1, ea.plane(0)));
        const UIntBatch p1 = popcount(one, 2);
        expect(sameBatchWords(p1.plane(0), ea.plane(0)) && p1.plane(1).terms() == 1, "popcount of one plane");
    }
    // 64-bit words: planes 0 and 1 in one launch, and bit 6 alone, the AND of all 64
    {
        std::vector<uint64_t> a = {~0ull, rnd(64), 0x8000000000000001ull}, pa(3);
        for (size_t i = 0; i < a.size(); ++i)
            pa[i] = ones(a[i]);
        const UIntBatch ea = UIntBatch::encrypt(key, a, 64, 31);
        const UIntBatch p = popcount(ea, 2);
        expect(p.plane(0).terms() == 64 && p.plane(1).terms() == 2016, "popcount w=64 terms");
        checkCount(p, planesOf(ea), a.size(), 64, false, pa, key, "popcount w=64");
        const CiphertextBatch top = popcountBit(ea, 6);
        expect(top.terms() == 1, "popcountBit(a, 6) is one term");
        checkBit(top, planesOf(ea), a.size(), 64, false, 6, pa, key, "popcountBit(a, 6) w=64");
    }
    // COUNT(*) of matching rows: equal keys are counted, where matches() only has their parity
    {
        const std::vector<uint64_t> keys = {1, 2, 1, 3, 1, 2}, query = {1, 2, 3, 0};
        const UIntBatch ek = UIntBatch::encrypt(key, keys, 2, 41), eq = UIntBatch::encrypt(key, query, 2, 42);
        std::vector<uint64_t> want(query.size(), 0), ik, iq;
        for (size_t e = 0; e < query.size(); ++e)
            for (size_t r = 0; r < keys.size(); ++r) {
                want[e] += keys[r] == query[e];
                ik.push_back(r);
                iq.push_back(e);
            }
        const UIntBatch c = countMatches(ek, eq, 3);
        const CiphertextBatch all = equalTo(ek.gather(ik), eq.gather(iq));
        checkCount(c, all, query.size(), keys.size(), true, want, key, "countMatches");
        expect(sameBatchWords(c.plane(0), matches(ek, eq)), "plane 0 of countMatches has the words of matches");
    }
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    // x + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO twice, which
    // cancels: the batch is ragged
    auto raggedOf = [&](const CiphertextBatch &x) {
        std::vector<unsigned char> p(x.size(), 0), q(x.size(), 0);
        p[0] = 1;
        return addPlain(addPlain(x, p), q).compact();
    };
    const uint64_t g = 5, count = 6;
    std::vector<unsigned char> bits = randomBits(count * g);
    const CiphertextBatch b = CiphertextBatch::encrypt(key, bits, 51), br = raggedOf(b);
    expect(!br.uniform(), "compact() gave a ragged batch");
    bits[0] ^= 1;
    const std::vector<uint64_t> want = groupCounts(bits, g);
    checkCount(countOnes(br, g, 3), br, count, g, true, want, key, "ragged countOnes");
    checkBit(countBit(br, g, 2), br, count, g, true, 2, want, key, "ragged countBit");
    // the groups that hold no changed element have the uniform count's words
    const UIntBatch u = countOnes(b, g, 3), r = countOnes(br, g, 3);
    for (unsigned j = 0; j < 3; ++j)
        for (uint64_t q = 1; q < count; ++q)
            expect(sameWords(u.plane(j).at(q), r.plane(j).at(q)), "ragged words == uniform words, element " + std::to_string(q));
    // an integer with one ragged plane, and one with planes of different term counts
    std::vector<uint64_t> a(9), pa(9);
    for (size_t i = 0; i < a.size(); ++i)
        a[i] = rnd(6);
    const UIntBatch ea = UIntBatch::encrypt(key, a, 6, 52);
    std::vector<CiphertextBatch> planes, mixed;
    for (unsigned j = 0; j < 6; ++j) {
        planes.push_back(j == 2 ? raggedOf(ea.plane(j)) : ea.plane(j));
        mixed.push_back(j == 4 ? ea.plane(j) + CiphertextBatch::encrypt(key, std::vector<unsigned char>(a.size(), 0), 53) : ea.plane(j));
    }
    const UIntBatch er = UIntBatch::fromPlanes(planes), em = UIntBatch::fromPlanes(mixed);
    for (size_t i = 0; i < a.size(); ++i)
        pa[i] = ones(a[i]);
    checkCount(popcount(em, 3), planesOf(em), a.size(), 6, false, pa, key, "popcount of mixed term counts");
    pa[0] = ones(a[0] ^ 4);
    checkCount(popcount(er, 3), planesOf(er), a.size(), 6, false, pa, key, "popcount of a ragged plane");
    return 0;
}

int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const CiphertextBatch b = CiphertextBatch::encrypt(key, randomBits(128), 61);
    const UIntBatch a = UIntBatch::encrypt(key, {1, 2, 3}, 64, 62), a8 = UIntBatch::encrypt(key, {1, 2, 3}, 8, 63);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o8 = UIntBatch::encrypt(okey, {1, 2, 3}, 8, 64);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { countOnes(b, 64, 4); });                   // plane 3: C(64, 8) terms
    thrown += throws<std::invalid_argument>([&] { countBit(b, 64, 3); });
    thrown += throws<std::invalid_argument>([&] { popcount(a, 4); });
    thrown += throws<std::invalid_argument>([&] { popcountBit(a, 5); });
    thrown += throws<std::invalid_argument>([&] { hammingDistance(a, a, 64); });
    thrown += throws<std::invalid_argument>([&] { countOnes(b, 0, 2); });                    // groups
    thrown += throws<std::invalid_argument>([&] { countOnes(b, 5, 2); });
    thrown += throws<std::invalid_argument>([&] { countBit(b, 256, 0); });
    thrown += throws<std::invalid_argument>([&] { countOnes(b, 4, 0); });                    // planes
    thrown += throws<std::invalid_argument>([&] { countOnes(b, 4, 65); });
    thrown += throws<std::invalid_argument>([&] { popcount(a8, 0); });
    thrown += throws<std::invalid_argument>([&] { hammingDistance(a8, a, 2); });             // widths
    thrown += throws<std::invalid_argument>([&] { hammingDistance(a8, o8, 2); });            // contexts
    thrown += throws<std::invalid_argument>([&] { countMatches(a8, a, 2); });
    thrown += throws<std::invalid_argument>([&] { countMatches(a8, o8, 2); });
    thrown += throws<std::invalid_argument>([&] { countMatches(a8.slice(0, 0), a8, 2); });   // no rows
    thrown += throws<std::invalid_argument>([&] { countMatches(a8, a8, 2); });               // pairs of 3^8-term equalities
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 17, "bad arguments throw (" + std::to_string(thrown) + " of 17)");
    expect(s < 1.0, "the checks ran before any launch (" + std::to_string(s) + " s)");
    // an empty batch: empty planes
    const UIntBatch none = countOnes(b.slice(0, 0), 4, 3);
    expect(none.width() == 3 && none.size() == 0, "an empty batch gives empty planes");
    expect(countMatches(a8, a8.slice(0, 0), 2).size() == 0, "an empty query gives empty planes");
    // a later valid call still works
    const UIntBatch c = countOnes(b, 64, 2);
    expect(c.size() == 2 && c.plane(1).terms() == 2016, "a valid call after the refused ones");
    expect(sameBatchWords(c.plane(1), composedPlane(b, 2, 64, true, 1)), "... with the composition's words");
    return 0;
}

// No device work: the form csgn_count_kernel names for the shapes of words, under the knob the process was started with.
int forms()
{
    struct Shape {
        uint64_t count, g, t, n_in;
        std::vector<uint64_t> js;
    };
    const Shape shapes[] = {{40, 5, 1, 1, {1, 2}}, {40, 5, 2, 1, {1, 2}}, {37, 8, 1, 8, {0, 1, 2}}, {37, 8, 2, 8, {0, 1}},
                            {3, 64, 1, 64, {0, 1}}, {3, 64, 1, 64, {6}}, {4, 6, 27, 1, {1, 2}}};
    for (const Shape &s : shapes) {
        const char *form = csgn_count_kernel(1247, s.count, s.g, s.t, s.n_in, s.js.size(), s.js.data());
        expect(form && *form, "the count has a form");
        printf("%llux%llu t=%llu in=%llu -> %s\n", (unsigned long long)s.count, (unsigned long long)s.g,
               (unsigned long long)s.t, (unsigned long long)s.n_in, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4721, "count_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
