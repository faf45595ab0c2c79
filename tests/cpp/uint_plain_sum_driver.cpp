// uint_plain_sum_driver.cpp -- user-style C++ over inRange, outOfRange, inRanges, isIn, notIn, stepFunction, bucketOf
// and lookupSparse of include/certfhe/UInt.h (tests/test_uint_plain_sum_cpp.py builds and runs it).
//   uint_plain_sum_driver words    every function against the composition through the public comparisons and
//                                  CiphertextBatch::operator+, word for word, and decrypted against the clear function
//                                  for every a below 2^w at w = 1 .. 6; at N=1247 a 32-bit range, a set of 16 keys at
//                                  w = 16, an 8-threshold bucketOf and a sparse table at w = 32
//   uint_plain_sum_driver ragged   a compact()ed (ragged) operand takes the loop: the same words and decryptions
//   uint_plain_sum_driver errors   every std::invalid_argument; oversize before any launch; an empty batch
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <stdexcept>

using namespace certFHE;

namespace {

typedef std::pair<uint64_t, uint64_t> Interval;

uint64_t topOf(unsigned w) { return w == 64 ? ~0ull : (1ull << w) - 1; }

CiphertextBatch one(const UIntBatch &a) { return constantBatch(a.context(), std::vector<unsigned char>(a.size(), 1)); }
CiphertextBatch zero(const UIntBatch &a) { return constantBatch(a.context(), std::vector<unsigned char>(a.size(), 0)); }

// the definitions of include/certfhe/UInt.h through the public comparisons and operator+
CiphertextBatch rangeByOperators(const UIntBatch &a, uint64_t lo, uint64_t hi)
{
    const uint64_t top = topOf(a.width());
    if (lo == 0 && hi == top)
        return one(a);
    if (lo == 0)
        return lessEqual(a, hi);
    if (hi == top)
        return greaterEqual(a, lo);
    return lessThan(a, hi + 1) + lessThan(a, lo);
}

CiphertextBatch rangesByOperators(const UIntBatch &a, const std::vector<Interval> &iv)
{
    if (iv.empty())
        return zero(a);
    CiphertextBatch sum = rangeByOperators(a, iv[0].first, iv[0].second);
    for (size_t i = 1; i < iv.size(); ++i) {
        const uint64_t lo = iv[i].first, hi = iv[i].second, top = topOf(a.width());
        if (lo == 0)
            sum = sum + lessEqual(a, hi);
        else if (hi == top)
            sum = sum + greaterEqual(a, lo);
        else
            sum = (sum + lessThan(a, hi + 1)) + lessThan(a, lo);
    }
    return sum;
}

CiphertextBatch setByOperators(const UIntBatch &a, std::vector<uint64_t> keys, bool negate)
{
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (keys.empty())
        return negate ? one(a) : zero(a);
    CiphertextBatch sum = equalTo(a, keys[0]);
    for (size_t i = 1; i < keys.size(); ++i)
        sum = sum + equalTo(a, keys[i]);
    return negate ? sum + one(a) : sum;
}

// a plane that sums cmp(a, ks[i]) in order, + ONE when `bit`
template <typename Cmp>
CiphertextBatch planeByOperators(const UIntBatch &a, const std::vector<uint64_t> &ks, bool bit, Cmp cmp)
{
    if (ks.empty())
        return bit ? one(a) : zero(a);
    CiphertextBatch sum = cmp(a, ks[0]);
    for (size_t i = 1; i < ks.size(); ++i)
        sum = sum + cmp(a, ks[i]);
    return bit ? sum + one(a) : sum;
}

UIntBatch stepByOperators(const UIntBatch &a, const std::vector<uint64_t> &t, const std::vector<uint64_t> &v, unsigned ow)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < ow; ++j) {
        std::vector<uint64_t> ks;
        for (size_t i = 0; i < t.size(); ++i)
            if (((v[i] ^ v[i + 1]) >> j) & 1u)
                ks.push_back(t[i]);
        planes.push_back(planeByOperators(a, ks, (v.back() >> j) & 1u, [](const UIntBatch &x, uint64_t k) { return lessThan(x, k); }));
    }
    return UIntBatch::fromPlanes(planes);
}

UIntBatch sparseByOperators(const UIntBatch &a, const std::vector<uint64_t> &keys, const std::vector<uint64_t> &values,
                            unsigned ow, uint64_t otherwise)
{
    std::map<uint64_t, uint64_t> table;
    for (size_t i = 0; i < keys.size(); ++i)
        table.insert(std::make_pair(keys[i], values[i]));
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < ow; ++j) {
        std::vector<uint64_t> ks;
        for (std::map<uint64_t, uint64_t>::const_iterator it = table.begin(); it != table.end(); ++it)
            if (((it->second ^ otherwise) >> j) & 1u)
                ks.push_back(it->first);
        planes.push_back(planeByOperators(a, ks, (otherwise >> j) & 1u, [](const UIntBatch &x, uint64_t k) { return equalTo(x, k); }));
    }
    return UIntBatch::fromPlanes(planes);
}

// the clear functions
uint64_t stepClear(const std::vector<uint64_t> &t, const std::vector<uint64_t> &v, uint64_t x)
{
    size_t i = 0;
    while (i < t.size() && x >= t[i])
        ++i;
    return v[i];
}

uint64_t sparseClear(const std::vector<uint64_t> &keys, const std::vector<uint64_t> &values, uint64_t otherwise, uint64_t x)
{
    for (size_t i = 0; i < keys.size(); ++i)
        if (keys[i] == x)
            return values[i];
    return otherwise;
}

void checkBit(const SecretKey &key, const CiphertextBatch &got, const CiphertextBatch &want, const std::vector<unsigned char> &clear,
              const std::string &tag)
{
    expect(sameBatchWords(got, want), tag + " == the CiphertextBatch operators");
    expect(got.decrypt(key) == clear, tag + " decrypted");
}

void checkInt(const SecretKey &key, const UIntBatch &got, const UIntBatch &want, const std::vector<uint64_t> &clear,
              const std::string &tag)
{
    expect(sameWords(got, want), tag + " == the CiphertextBatch operators");
    checkValues(got.decrypt(key), clear, tag + " decrypted");
}

std::vector<uint64_t> ascending(unsigned w, size_t m, uint64_t from)
{
    std::vector<uint64_t> t;
    const uint64_t top = topOf(w), step = std::max<uint64_t>(1, (top - from) / (m + 1));
    for (size_t i = 0; i < m && from + i * step <= top; ++i)
        t.push_back(from + i * step + (i ? rnd(w) % step : 0));
    return t;
}

// every function over `a` (values va) at width w
void checkAll(const SecretKey &key, const UIntBatch &a, const std::vector<uint64_t> &va, const std::string &tag)
{
    const unsigned w = a.width();
    const uint64_t top = topOf(w);
    auto bits = [&](std::function<bool(uint64_t)> f) {
        std::vector<unsigned char> v(va.size());
        for (size_t i = 0; i < va.size(); ++i)
            v[i] = f(va[i]) ? 1 : 0;
        return v;
    };
    std::vector<Interval> ranges = {{0, top}, {0, top / 2}, {top / 2, top}, {top / 3, top / 3}};
    if (w >= 2)
        ranges.push_back(Interval(1, top - 1));
    if (w >= 3)
        ranges.push_back(Interval(2, 5));
    for (size_t r = 0; r < ranges.size(); ++r) {
        const uint64_t lo = ranges[r].first, hi = ranges[r].second;
        const std::string t = tag + " [" + std::to_string(lo) + ", " + std::to_string(hi) + "]";
        checkBit(key, inRange(a, lo, hi), rangeByOperators(a, lo, hi), bits([&](uint64_t x) { return lo <= x && x <= hi; }), "inRange" + t);
        checkBit(key, outOfRange(a, lo, hi), rangeByOperators(a, lo, hi) + one(a), bits([&](uint64_t x) { return x < lo || x > hi; }),
                 "outOfRange" + t);
    }
    std::vector<std::vector<Interval> > unions = {{}, {{0, top}}, {{0, 0}, {top, top}}};
    if (w >= 3)
        unions.push_back({{0, 1}, {3, 3}, {5, top - 1}});
    if (w >= 4)
        unions.push_back({{1, 2}, {4, 9}, {11, 11}, {top - 2, top}});
    for (size_t u = 0; u < unions.size(); ++u) {
        const std::vector<Interval> &iv = unions[u];
        checkBit(key, inRanges(a, iv), rangesByOperators(a, iv), bits([&](uint64_t x) {
                     for (size_t i = 0; i < iv.size(); ++i)
                         if (iv[i].first <= x && x <= iv[i].second)
                             return true;
                     return false;
                 }),
                 "inRanges" + tag + " #" + std::to_string(u));
    }
    std::vector<std::vector<uint64_t> > sets = {{}, {0}, {top}, {top, 0, top}, {rnd(w), rnd(w), rnd(w), rnd(w), rnd(w)}};
    for (size_t s = 0; s < sets.size(); ++s) {
        const std::vector<uint64_t> &set = sets[s];
        auto in = [&](uint64_t x) { return std::find(set.begin(), set.end(), x) != set.end(); };
        checkBit(key, isIn(a, set), setByOperators(a, set, false), bits(in), "isIn" + tag + " #" + std::to_string(s));
        checkBit(key, notIn(a, set), setByOperators(a, set, true), bits([&](uint64_t x) { return !in(x); }),
                 "notIn" + tag + " #" + std::to_string(s));
    }
    for (size_t m = 0; m <= 3 && m <= top; ++m) {
        const std::vector<uint64_t> t = ascending(w, m, 1);
        std::vector<uint64_t> v(t.size() + 1);
        for (size_t i = 0; i < v.size(); ++i)
            v[i] = rnd(5);
        std::vector<uint64_t> clear(va.size()), bucket(va.size());
        for (size_t i = 0; i < va.size(); ++i) {
            clear[i] = stepClear(t, v, va[i]);
            bucket[i] = 0;
            for (size_t k = 0; k < t.size(); ++k)
                bucket[i] += va[i] >= t[k] ? 1 : 0;
        }
        const std::string st = tag + " m=" + std::to_string(t.size());
        checkInt(key, stepFunction(a, t, v, 5), stepByOperators(a, t, v, 5), clear, "stepFunction" + st);
        std::vector<uint64_t> idx(t.size() + 1);
        for (size_t i = 0; i < idx.size(); ++i)
            idx[i] = i;
        checkInt(key, bucketOf(a, t, 2), stepByOperators(a, t, idx, 2), bucket, "bucketOf" + st);
    }
    for (uint64_t otherwise = 0; otherwise <= 0x16; otherwise += 0x16) {
        std::vector<uint64_t> keys = {rnd(w), rnd(w), 0, top, rnd(w)}, values = {rnd(5), rnd(5), rnd(5), rnd(5), rnd(5)};
        std::vector<uint64_t> clear(va.size());
        for (size_t i = 0; i < va.size(); ++i)
            clear[i] = sparseClear(keys, values, otherwise, va[i]);
        checkInt(key, lookupSparse(a, keys, values, 5, otherwise), sparseByOperators(a, keys, values, 5, otherwise), clear,
                 "lookupSparse" + tag + " otherwise=" + std::to_string(otherwise));
    }
}

int words()
{
    {
        Context ctx(127, 8);
        SecretKey key(ctx);
        for (unsigned w = 1; w <= 6; ++w) {
            std::vector<uint64_t> va(1ull << w);
            for (size_t i = 0; i < va.size(); ++i)
                va[i] = i;
            const UIntBatch a = UIntBatch::encrypt(key, va, w, 60 + w);
            checkAll(key, a, va, " w=" + std::to_string(w));
        }
    }
    Context ctx(1247, 16);
    SecretKey key(ctx);
    // routes and payloads at w = 8
    std::vector<uint64_t> v8(256);
    for (size_t i = 0; i < 256; ++i)
        v8[i] = i;
    const UIntBatch a8 = UIntBatch::encrypt(key, v8, 8, 71);
    checkAll(key, a8, v8, " N=1247 w=8");
    expect(std::string(plainSumRoute(a8, {10, 20}, {0, 1, 0}, 1)) == "call", "two thresholds in a plane take the call");
    expect(std::string(plainSumRoute(a8, {10}, {1, 0}, 1)) == "loop", "one comparison alone is csgn_uint_plain's call");
    expect(std::string(plainSumRoute(a8, {10, 20}, {3, 3, 3}, 2)) == "loop", "constant planes launch nothing");
    expect(inRange(a8, 17, 200).terms() == lessThan(a8, 201).terms() + lessThan(a8, 17).terms(), "a range has its two comparisons' terms");
    expect(isIn(a8, {255, 255, 254}).terms() == 1 + 2, "the set is deduplicated: EQ 254 has 2 terms, EQ 255 one");
    // the shapes of tools/bench_uint_plain_sum.py, small batches
    const std::vector<uint64_t> v32 = {0, 1, 0x12345678, 0x80000000u, 0xFFFFFFFFu, 0x7FFFFFFF, 0x00FF00FF};
    const UIntBatch a32 = UIntBatch::encrypt(key, v32, 32, 73);
    const uint64_t lo = 0x00FF0000u, hi = 0x7FFFFFFFu;     // LT 2^31: 2 terms; LT lo: 4096
    std::vector<unsigned char> in(v32.size());
    for (size_t i = 0; i < v32.size(); ++i)
        in[i] = lo <= v32[i] && v32[i] <= hi;
    checkBit(key, inRange(a32, lo, hi), rangeByOperators(a32, lo, hi), in, "a 32-bit range");
    const std::vector<uint64_t> some = {0xFFFFFFFFu, 0xFFFFFFFEu, 0x7FFFFFFF, 0xFFFF7FFFu};
    std::vector<uint64_t> sv = {1, 2, 3, 4}, sclear(v32.size());
    for (size_t i = 0; i < v32.size(); ++i)
        sclear[i] = sparseClear(some, sv, 0, v32[i]);
    checkInt(key, lookupSparse(a32, some, sv, 3), sparseByOperators(a32, some, sv, 3, 0), sclear, "a sparse table at w = 32");
    std::vector<uint64_t> v16 = {0, 1, 65535, 4096, 4095, 32768, 40000, 12345, 60000};
    const UIntBatch a16 = UIntBatch::encrypt(key, v16, 16, 75);
    const std::vector<uint64_t> t16 = {4096, 8192, 16384, 24576, 32768, 40960, 49152, 57344};
    std::vector<uint64_t> bucket(v16.size()), idx(9);
    for (size_t i = 0; i < 9; ++i)
        idx[i] = i;
    for (size_t i = 0; i < v16.size(); ++i) {
        bucket[i] = 0;
        for (size_t k = 0; k < t16.size(); ++k)
            bucket[i] += v16[i] >= t16[k] ? 1 : 0;
    }
    checkInt(key, bucketOf(a16, t16, 4), stepByOperators(a16, t16, idx, 4), bucket, "an 8-threshold bucketOf at w = 16");
    std::vector<uint64_t> set16;
    for (unsigned i = 0; i < 16; ++i)
        set16.push_back(0xFFFF ^ (1u << i));
    std::vector<unsigned char> member(v16.size());
    for (size_t i = 0; i < v16.size(); ++i)
        member[i] = std::find(set16.begin(), set16.end(), v16[i]) != set16.end();
    checkBit(key, isIn(a16, set16), setByOperators(a16, set16, false), member, "isIn with 16 keys at w = 16");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 5; ++w) {
        const size_t count = 1ull << w;
        std::vector<uint64_t> va(count);
        for (size_t i = 0; i < count; ++i)
            va[i] = i;
        const UIntBatch a0 = UIntBatch::encrypt(key, va, w, 80 + w);
        // plane + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO
        // twice, which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
        std::vector<unsigned char> q0(count, 0), q1(count, 0);
        q0[0] = 1;
        std::vector<CiphertextBatch> planes;
        for (unsigned j = 0; j < w; ++j)
            planes.push_back(addPlain(addPlain(a0.plane(j), q0), q1).compact());
        const UIntBatch ar = UIntBatch::fromPlanes(planes);
        const std::string tag = " ragged w=" + std::to_string(w);
        expect(!ar.plane(0).uniform(), "compact() gave ragged planes" + tag);
        std::vector<uint64_t> fa = va;                    // element 0 of the ragged operand has every bit flipped
        fa[0] ^= (1ull << w) - 1;
        if (w >= 2)
            expect(std::string(plainSumRoute(ar, {1, 2}, {0, 1, 0}, 1)) == "loop" &&
                       std::string(plainSumRoute(a0, {1, 2}, {0, 1, 0}, 1)) == "call",
                   "a ragged operand takes the loop" + tag);
        checkAll(key, ar, fa, tag);
    }
    return 0;
}

int errors()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { inRange(a4, 5, 4); });                       // lo above hi
    thrown += throws<std::invalid_argument>([&] { inRange(a4, 0, 16); });                      // outside the width
    thrown += throws<std::invalid_argument>([&] { outOfRange(a4, 17, 18); });
    thrown += throws<std::invalid_argument>([&] { inRanges(a4, {{4, 6}, {1, 2}}); });          // unsorted
    thrown += throws<std::invalid_argument>([&] { inRanges(a4, {{1, 4}, {4, 6}}); });          // overlapping
    thrown += throws<std::invalid_argument>([&] { inRanges(a4, {{1, 4}, {7, 6}}); });
    thrown += throws<std::invalid_argument>([&] { isIn(a4, {1, 16}); });
    thrown += throws<std::invalid_argument>([&] { notIn(a4, {99}); });
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {0, 3}, {1, 2, 3}, 2); });  // a threshold of 0
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {3, 16}, {1, 2, 3}, 2); }); // outside the width
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {3, 3}, {1, 2, 3}, 2); });  // not strictly ascending
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {5, 3}, {1, 2, 3}, 2); });
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {3, 5}, {1, 2}, 2); });     // a wrong number of values
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {3, 5}, {1, 2, 3, 0}, 2); });
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {3, 5}, {1, 2, 3}, 0); });  // out_width
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {3, 5}, {1, 2, 3}, 65); });
    thrown += throws<std::invalid_argument>([&] { stepFunction(a4, {3, 5}, {1, 2, 4}, 2); });  // a value past out_width
    thrown += throws<std::invalid_argument>([&] { bucketOf(a4, {3, 5, 7, 9}, 2); });           // 5 buckets in 2 planes
    thrown += throws<std::invalid_argument>([&] { bucketOf(a4, {3, 5}, 0); });
    thrown += throws<std::invalid_argument>([&] { lookupSparse(a4, {1, 2}, {1}, 2); });
    thrown += throws<std::invalid_argument>([&] { lookupSparse(a4, {1, 16}, {1, 2}, 2); });
    thrown += throws<std::invalid_argument>([&] { lookupSparse(a4, {1, 2}, {1, 4}, 2); });
    thrown += throws<std::invalid_argument>([&] { lookupSparse(a4, {1, 2}, {1, 2}, 2, 4); });
    thrown += throws<std::invalid_argument>([&] { lookupSparse(a4, {1, 2}, {1, 2}, 65); });
    thrown += throws<std::invalid_argument>([&] { plainSumRoute(a4, {3, 5}, {1, 2}, 2); });
    expect(thrown == 25, "the argument checks throw (" + std::to_string(thrown) + " of 25)");
    expect(bucketOf(a4, {3, 5, 7}, 2).width() == 2 && stepFunction(a4, {15}, {0, ~0ull}, 64).width() == 64, "the limits themselves fit");
    // oversize: ONE element whose planes share a payload of 2^21 terms; a sum of two comparisons is past 2^31 words
    CiphertextBatch big = a4.plane(0).slice(0, 1);
    for (int i = 0; i < 21; ++i)
        big = big + big;
    const UIntBatch wide = UIntBatch::fromPlanes(std::vector<CiphertextBatch>(4, big));
    const auto t0 = std::chrono::steady_clock::now();
    thrown = throws<std::invalid_argument>([&] { inRange(wide, 1, 14); });
    thrown += throws<std::invalid_argument>([&] { isIn(wide, {1, 2, 15}); });
    thrown += throws<std::invalid_argument>([&] { bucketOf(wide, {8, 12}, 2); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 3, "oversize throws (" + std::to_string(thrown) + " of 3)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // an empty batch: empty planes of the output width
    const UIntBatch e = stepFunction(a4.slice(0, 0), {3, 5}, {1, 2, 3}, 2);
    expect(e.width() == 2 && e.size() == 0 && inRange(a4.slice(0, 0), 1, 2).size() == 0 &&
               std::string(plainSumRoute(a4.slice(0, 0), {3, 5}, {1, 2, 1}, 2)) == "loop",
           "an empty batch gives empty planes");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 3737, "uint_plain_sum_driver", {{"words", words}, {"ragged", ragged}, {"errors", errors}});
}
