// count_prefix_driver.cpp -- user-style C++ over runningCount / runningCountBit / prefixPopcount of
// include/certfhe/UInt.h: running counts of encrypted bits (tests/test_count_prefix_cpp.py builds and runs it).
//   count_prefix_driver words    seeded encryptions, then every operation, inclusive and exclusive: entry r == countOnes /
//                                popcount of the gathered prefix, word for word, ZERO planes included; decryptions == the
//                                prefix count modulo 2^planes; the entries of a plane are views into one block
//   count_prefix_driver ragged   a compact()-ed (ragged) operand, and planes of different term counts, take the loop:
//                                the same words as countOnes of the gathered prefix, and decryptions alike
//   count_prefix_driver errors   every bad argument throws std::invalid_argument before anything is allocated, an empty
//                                batch gives empty planes, the routes' names, and a later valid call still works
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <cstring>
#include <stdexcept>

using namespace certFHE;

namespace {

uint64_t maskOf(unsigned planes) { return planes >= 64 ? ~0ull : (1ull << planes) - 1; }

// rows 0 .. nr - 1 of every group of g
CiphertextBatch prefixOf(const CiphertextBatch &bits, uint64_t g, uint64_t nr)
{
    std::vector<uint64_t> idx;
    for (uint64_t q = 0; q < bits.size() / g; ++q)
        for (uint64_t i = 0; i < nr; ++i)
            idx.push_back(q * g + i);
    return bits.gather(idx);
}

UIntBatch lowPlanes(const UIntBatch &a, uint64_t nr)
{
    std::vector<CiphertextBatch> planes;
    for (uint64_t j = 0; j < nr; ++j)
        planes.push_back(a.plane((unsigned)j));
    return UIntBatch::fromPlanes(planes);
}

bool isZero(const CiphertextBatch &p, uint64_t count)
{
    return p.size() == count && p.terms() == 1 &&
           sameBatchWords(p, constantBatch(p.context(), std::vector<unsigned char>(count, 0)));
}

// want[q * g + i]: bit i of group q
void checkRunning(const std::vector<UIntBatch> &got, const CiphertextBatch &bits, uint64_t g, unsigned planes, bool ex,
                  const std::vector<unsigned char> &clear, const SecretKey &key, const std::string &tag)
{
    const uint64_t count = bits.size() / g;
    expect(got.size() == g, tag + ": one entry a row");
    for (uint64_t r = 0; r < got.size(); ++r) {
        const uint64_t nr = r + 1 - (ex ? 1 : 0);
        const std::string at = tag + " row " + std::to_string(r);
        expect(got[r].width() == planes && got[r].size() == count, at + ": shape");
        if (nr == 0) {
            for (unsigned j = 0; j < planes; ++j)
                expect(isZero(got[r].plane(j), count), at + ": an empty prefix is ZERO");
        } else {
            expect(sameWords(got[r], countOnes(prefixOf(bits, g, nr), nr, planes)), at + ": words == countOnes of the prefix");
        }
        std::vector<uint64_t> want(count, 0);
        for (uint64_t q = 0; q < count; ++q) {
            for (uint64_t i = 0; i < nr; ++i)
                want[q] += clear[q * g + i];
            want[q] &= maskOf(planes);
        }
        checkValues(got[r].decrypt(key), want, at);
    }
}

void checkPopcount(const std::vector<UIntBatch> &got, const UIntBatch &a, unsigned planes, bool ex,
                   const std::vector<uint64_t> &clear, const SecretKey &key, const std::string &tag)
{
    expect(got.size() == a.width(), tag + ": one entry a bit");
    for (uint64_t i = 0; i < got.size(); ++i) {
        const uint64_t nr = i + 1 - (ex ? 1 : 0);
        const std::string at = tag + " bit " + std::to_string(i);
        if (nr == 0) {
            for (unsigned j = 0; j < planes; ++j)
                expect(isZero(got[i].plane(j), a.size()), at + ": an empty prefix is ZERO");
        } else {
            expect(sameWords(got[i], popcount(lowPlanes(a, nr), planes)), at + ": words == popcount of the low bits");
        }
        std::vector<uint64_t> want(a.size());
        for (size_t e = 0; e < want.size(); ++e)
            want[e] = (uint64_t)__builtin_popcountll(nr >= 64 ? clear[e] : clear[e] & ((1ull << nr) - 1)) & maskOf(planes);
        checkValues(got[i].decrypt(key), want, at);
    }
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
    expect(!strcmp(runningCountRoute(5, true), "csgn_count_prefix"), "uniform inputs take the call");
    // groups of 5 bits, fresh and of two terms: every pattern and more
    const uint64_t g = 5, count = 40;
    std::vector<unsigned char> bits(count * g);
    for (uint64_t q = 0; q < count; ++q)
        for (uint64_t i = 0; i < g; ++i)
            bits[q * g + i] = (unsigned char)((q < 32 ? q >> i : (uint64_t)rand()) & 1);
    const CiphertextBatch b1 = CiphertextBatch::encrypt(key, bits, 11);
    const CiphertextBatch b2 = b1 + CiphertextBatch::encrypt(key, std::vector<unsigned char>(bits.size(), 0), 12);
    const CiphertextBatch *both[2] = {&b1, &b2};
    for (int v = 0; v < 2; ++v)
        for (int ex = 0; ex < 2; ++ex) {
            const CiphertextBatch &b = *both[v];
            const std::string tag = " g=5 t=" + std::to_string(v + 1) + (ex ? " exclusive" : "");
            const std::vector<UIntBatch> c = runningCount(b, g, 4, ex != 0);         // plane 3: 2^3 > 5, ZERO
            checkRunning(c, b, g, 4, ex != 0, bits, key, "runningCount" + tag);
            // the rows of a plane lie one after the other in one block
            const uint64_t dl = ctx.getDefaultN();
            for (uint64_t r = ex ? 2 : 1; r + 1 < g; ++r)
                expect(c[r + 1].plane(0).deviceValues() ==
                           c[r].plane(0).deviceValues() + count * c[r].plane(0).terms() * dl,
                       "row " + std::to_string(r + 1) + " of plane 0 follows row " + std::to_string(r) + tag);
            for (unsigned j = 0; j < 4; ++j) {
                const std::vector<CiphertextBatch> bit = runningCountBit(b, g, j, ex != 0);
                expect(bit.size() == g, "runningCountBit: one entry a row" + tag);
                for (uint64_t r = 0; r < bit.size(); ++r)
                    expect(sameBatchWords(bit[r], c[r].plane(j)),
                           "runningCountBit " + std::to_string(j) + " row " + std::to_string(r) + " == the plane" + tag);
            }
        }
    // 8-bit integers, fresh and of two terms: the rank function of a bit vector
    {
        std::vector<uint64_t> a(37);
        for (size_t i = 0; i < a.size(); ++i)
            a[i] = i == 0 ? 0 : i == 1 ? 255 : rnd(8);
        const UIntBatch ea = UIntBatch::encrypt(key, a, 8, 21), ea2 = twoTerms(ea, key, 23);
        checkPopcount(prefixPopcount(ea, 4), ea, 4, false, a, key, "prefixPopcount w=8");
        checkPopcount(prefixPopcount(ea, 3, true), ea, 3, true, a, key, "prefixPopcount w=8 exclusive");
        checkPopcount(prefixPopcount(ea2, 2), ea2, 2, false, a, key, "prefixPopcount w=8 t=2");
        // a width of 1: the count is the bit, and before it there is nothing
        const UIntBatch one = lowPlanes(ea, 1);
        const std::vector<UIntBatch> p1 = prefixPopcount(one, 2), x1 = prefixPopcount(one, 2, true);
        expect(p1.size() == 1 && sameBatchWords(p1[0].plane(0), ea.plane(0)) && isZero(p1[0].plane(1), a.size()),
               "prefixPopcount of one plane");
        expect(x1.size() == 1 && isZero(x1[0].plane(0), a.size()), "exclusive prefixPopcount of one plane");
    }
    // 64-bit words: planes 0 and 1 in one launch
    {
        const std::vector<uint64_t> a = {~0ull, rnd(64), 0x8000000000000001ull};
        const UIntBatch ea = UIntBatch::encrypt(key, a, 64, 31);
        const std::vector<UIntBatch> p = prefixPopcount(ea, 2);
        expect(p.size() == 64 && p[63].plane(0).terms() == 64 && p[63].plane(1).terms() == 2016 &&
                   p[1].plane(1).terms() == 1 && p[0].plane(1).terms() == 1,
               "prefixPopcount w=64 terms");
        checkPopcount(p, ea, 2, false, a, key, "prefixPopcount w=64");
    }
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    expect(!strcmp(runningCountRoute(5, false), "loop"), "ragged inputs take the loop");
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
    const std::vector<UIntBatch> u = runningCount(b, g, 3), ux = runningCount(b, g, 3, true);
    bits[0] ^= 1;
    const std::vector<UIntBatch> r = runningCount(br, g, 3), rx = runningCount(br, g, 3, true);
    checkRunning(r, br, g, 3, false, bits, key, "ragged runningCount");
    checkRunning(rx, br, g, 3, true, bits, key, "ragged exclusive runningCount");
    // the groups that hold no changed element have the call's words
    for (uint64_t row = 0; row < g; ++row)
        for (unsigned j = 0; j < 3; ++j)
            for (uint64_t q = 1; q < count; ++q) {
                expect(sameWords(u[row].plane(j).at(q), r[row].plane(j).at(q)),
                       "ragged words == uniform words, row " + std::to_string(row) + " element " + std::to_string(q));
                expect(sameWords(ux[row].plane(j).at(q), rx[row].plane(j).at(q)),
                       "ragged words == uniform words, exclusive, row " + std::to_string(row) + " element " + std::to_string(q));
            }
    // an integer with one ragged plane, and one with planes of different term counts
    std::vector<uint64_t> a(9);
    for (size_t i = 0; i < a.size(); ++i)
        a[i] = rnd(6);
    const UIntBatch ea = UIntBatch::encrypt(key, a, 6, 52);
    std::vector<CiphertextBatch> planes, mixed;
    for (unsigned j = 0; j < 6; ++j) {
        planes.push_back(j == 2 ? raggedOf(ea.plane(j)) : ea.plane(j));
        mixed.push_back(j == 4 ? ea.plane(j) + CiphertextBatch::encrypt(key, std::vector<unsigned char>(a.size(), 0), 53) : ea.plane(j));
    }
    const UIntBatch er = UIntBatch::fromPlanes(planes), em = UIntBatch::fromPlanes(mixed);
    checkPopcount(prefixPopcount(em, 3), em, 3, false, a, key, "prefixPopcount of mixed term counts");
    checkPopcount(prefixPopcount(em, 3, true), em, 3, true, a, key, "exclusive prefixPopcount of mixed term counts");
    a[0] ^= 4;
    checkPopcount(prefixPopcount(er, 3), er, 3, false, a, key, "prefixPopcount of a ragged plane");
    return 0;
}

int errors()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const CiphertextBatch b = CiphertextBatch::encrypt(key, randomBits(128), 61);
    const UIntBatch a = UIntBatch::encrypt(key, {1, 2, 3}, 64, 62), a8 = UIntBatch::encrypt(key, {1, 2, 3}, 8, 63);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { runningCount(b, 64, 4); });                // plane 3: C(64, 8) terms
    thrown += throws<std::invalid_argument>([&] { runningCount(b, 64, 4, true); });          // C(63, 8)
    thrown += throws<std::invalid_argument>([&] { runningCountBit(b, 64, 3); });
    thrown += throws<std::invalid_argument>([&] { prefixPopcount(a, 4); });
    thrown += throws<std::invalid_argument>([&] { runningCount(b, 0, 2); });                 // groups
    thrown += throws<std::invalid_argument>([&] { runningCount(b, 5, 2); });
    thrown += throws<std::invalid_argument>([&] { runningCountBit(b, 256, 0); });
    thrown += throws<std::invalid_argument>([&] { runningCount(b, 4, 0); });                 // planes
    thrown += throws<std::invalid_argument>([&] { runningCount(b, 4, 65); });
    thrown += throws<std::invalid_argument>([&] { prefixPopcount(a8, 0); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 10, "bad arguments throw (" + std::to_string(thrown) + " of 10)");
    expect(s < 1.0, "the checks ran before any launch (" + std::to_string(s) + " s)");
    expect(!strcmp(runningCountRoute(64, true), "csgn_count_prefix") && !strcmp(runningCountRoute(64, false), "loop") &&
               !strcmp(runningCountRoute(0, true), "loop"),
           "the routes");
    // an empty batch: empty planes
    const std::vector<UIntBatch> none = runningCount(b.slice(0, 0), 4, 3);
    expect(none.size() == 4 && none[3].width() == 3 && none[3].size() == 0, "an empty batch gives empty planes");
    // planes past the group are ZERO without a launch; bit 6 of 64 rows is one term in the last row alone
    const std::vector<CiphertextBatch> top = runningCountBit(b, 64, 6), past = runningCountBit(b, 64, 6, true);
    expect(isZero(top[62], 2) && top[63].terms() == 1 && sameBatchWords(top[63], countBit(b, 64, 6)), "bit 6 of 64 rows");
    expect(isZero(past[63], 2) && isZero(runningCountBit(b, 4, 7)[3], 32), "planes past the rows are ZERO");
    // a later valid call still works
    const std::vector<UIntBatch> c = runningCount(b, 64, 2);
    expect(c.size() == 64 && c[63].plane(1).terms() == 2016, "a valid call after the refused ones");
    expect(sameWords(c[63], countOnes(b, 64, 2)), "... whose last row is the count of the group");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4734, "count_prefix_driver", {{"words", words}, {"ragged", ragged}, {"errors", errors}});
}
