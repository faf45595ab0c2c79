// uint_readback_driver.cpp -- user-style C++ over readAtEach of what writeAtEach returns, include/certfhe/UInt.h's "read
// that follows" (tests/test_uint_readback_cpp.py builds and runs it).
//   uint_readback_driver routes   readAtEachRoute: "rows" for writeAtEach's results, written once and twice, and for
//                                 uniform planes of different term counts; "pick" for uniform arrays of one count; "loop"
//                                 for a compact()ed index and for arrays without a period
//   uint_readback_driver words    readAtEach(writeAtEach(a, n, i, x), n, j) by the "rows" route at N=1247 against the loop
//                                 over the same operands with the public operators -- per row r equalTo(j, r) * the
//                                 gathered row, summed left to right -- word for word; the result is uniform(); the
//                                 decryptions against plain arrays, every read index included; multi-term planes; a table
//                                 written twice; the bit overload
//   uint_readback_driver oversize a read past 2^31 words per element throws std::invalid_argument before anything is
//                                 allocated; an empty batch is empty
//   uint_readback_driver forms    "<shape> -> <form>": the form csgn_uint_pick_rows_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Case {
    unsigned w, v;
    uint64_t n;         // rows of an element's array
    size_t count;       // arrays
};
const Case kCases[] = {
    {3, 2, 3, 8}, {4, 3, 5, 12}, {1, 2, 4, 20}, {8, 4, 16, 3}, {4, 3, 8, 10}, {1, 1, 1, 5}, {2, 1, 2, 9},
};
const size_t kNumCases = sizeof(kCases) / sizeof(kCases[0]);

std::vector<uint64_t> rowIndices(uint64_t m, uint64_t n, uint64_t r)
{
    std::vector<uint64_t> idx(m);
    for (uint64_t e = 0; e < m; ++e)
        idx[e] = e * n + r;
    return idx;
}

// the definition with the public operators, the loop readAtEach itself takes for planes without a period: output j is
// the left-nested sum, ascending in r, of equalTo(index, r) * (row r of every array, plane j)
UIntBatch viaLoop(uint64_t n, const UIntBatch &arrays, const UIntBatch &index)
{
    const uint64_t m = index.size();
    std::vector<CiphertextBatch> planes;
    for (uint64_t r = 0; r < n; ++r) {
        const CiphertextBatch eq = equalTo(index, r);
        for (unsigned j = 0; j < arrays.width(); ++j) {
            const CiphertextBatch p = eq * arrays.plane(j).gather(rowIndices(m, n, r));
            if (r == 0)
                planes.push_back(p);
            else
                planes[j] = planes[j] + p;
        }
    }
    return UIntBatch::fromPlanes(planes);
}

struct Plain {
    std::vector<uint64_t> a, wi, ri, x, want;
};

// every (write index, read index) pair among the first arrays where they fit, random ones behind them
Plain draw(const Case &c)
{
    Plain p;
    const uint64_t full = 1ull << c.v;
    for (size_t e = 0; e < c.count; ++e) {
        p.wi.push_back(e < full * full ? e / full : rnd(c.v));
        p.ri.push_back(e < full * full ? e % full : rnd(c.v));
        for (uint64_t r = 0; r < c.n; ++r)
            p.a.push_back(rnd(c.w));
        p.x.push_back(rnd(c.w));
    }
    for (size_t e = 0; e < c.count; ++e) {
        uint64_t got = p.ri[e] < c.n ? p.a[e * c.n + p.ri[e]] : 0;
        if (p.ri[e] < c.n && p.ri[e] == p.wi[e])
            got = p.x[e];
        p.want.push_back(got);
    }
    return p;
}

std::string tagOf(const Case &c)
{
    return " w=" + std::to_string(c.w) + " v=" + std::to_string(c.v) + " n=" + std::to_string(c.n) + " count=" +
           std::to_string(c.count);
}

bool is(const char *route, const char *want) { return route && std::string(route) == want; }

// the read of `written` at `index`: by the "rows" route, uniform, the loop's words, the wanted values
void check(const SecretKey &key, const Case &c, const UIntBatch &written, const UIntBatch &index,
           const std::vector<uint64_t> &want, const std::string &tag)
{
    expect(is(readAtEachRoute(written, c.n, index), "rows"), "the read of written planes takes the rows route" + tag);
    const UIntBatch got = readAtEach(written, c.n, index);
    expect(got.size() == c.count && got.width() == c.w, "the result has one element an array" + tag);
    for (unsigned j = 0; j < got.width(); ++j)
        expect(got.plane(j).uniform(), "the result is uniform" + tag);
    expect(sameWords(got, viaLoop(c.n, written, index)), "readAtEach == the loop over the same operands" + tag);
    checkValues(got.decrypt(key), want, "decryption" + tag);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (size_t i = 0; i < kNumCases; ++i) {
        const Case &c = kCases[i];
        const Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 30 + i), wi = UIntBatch::encrypt(key, p.wi, c.v, 60 + i);
        const UIntBatch ri = UIntBatch::encrypt(key, p.ri, c.v, 75 + i), x = UIntBatch::encrypt(key, p.x, c.w, 90 + i);
        const UIntBatch written = writeAtEach(a, c.n, wi, x);
        check(key, c, written, ri, p.want, tagOf(c));
        expect(sameBatchWords(readAtEach(written.plane(0), c.n, ri), readAtEach(written, c.n, ri).plane(0)),
               "readAtEach of bits == plane 0" + tagOf(c));
    }
    // multi-term planes (XOR with a trivial ZERO: two terms a plane)
    for (size_t i = 0; i < kNumCases; i += 2) {
        Case c = kCases[i];
        c.count = std::min<size_t>(c.count, 6);
        const Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 120 + i), wi = UIntBatch::encrypt(key, p.wi, c.v, 150 + i);
        const UIntBatch ri = UIntBatch::encrypt(key, p.ri, c.v, 165 + i), x = UIntBatch::encrypt(key, p.x, c.w, 180 + i);
        const UIntBatch za = UIntBatch::constant(ctx, std::vector<uint64_t>(p.a.size(), 0), c.w);
        const UIntBatch zd = UIntBatch::constant(ctx, std::vector<uint64_t>(p.ri.size(), 0), c.v);
        check(key, c, writeAtEach(a ^ za, c.n, wi, x), ri, p.want, " multi-term arrays" + tagOf(c));
        check(key, c, writeAtEach(a, c.n, wi ^ zd, x), ri, p.want, " multi-term write index" + tagOf(c));
        check(key, c, writeAtEach(a, c.n, wi, x), ri ^ zd, p.want, " multi-term read index" + tagOf(c));
    }
    // a table written twice: the second write takes the ragged planes of the first, and its result still has period n
    {
        const Case c = {2, 2, 3, 16};
        Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 220), wi = UIntBatch::encrypt(key, p.wi, c.v, 221);
        const UIntBatch ri = UIntBatch::encrypt(key, p.ri, c.v, 222), x = UIntBatch::encrypt(key, p.x, c.w, 223);
        std::vector<uint64_t> wi2(c.count), x2(c.count);
        for (size_t e = 0; e < c.count; ++e) {
            wi2[e] = rnd(c.v);
            x2[e] = rnd(c.w);
            if (wi2[e] < c.n && wi2[e] == p.ri[e])
                p.want[e] = x2[e];
        }
        const UIntBatch twice = writeAtEach(writeAtEach(a, c.n, wi, x), c.n, UIntBatch::encrypt(key, wi2, c.v, 224),
                                            UIntBatch::encrypt(key, x2, c.w, 225));
        check(key, c, twice, ri, p.want, " written twice" + tagOf(c));
    }
    return 0;
}

int routes()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const Case c = {3, 2, 3, 8};
    const Plain p = draw(c);
    const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 250), wi = UIntBatch::encrypt(key, p.wi, c.v, 251);
    const UIntBatch ri = UIntBatch::encrypt(key, p.ri, c.v, 252), x = UIntBatch::encrypt(key, p.x, c.w, 253);
    const UIntBatch written = writeAtEach(a, c.n, wi, x);
    expect(!written.plane(0).uniform(), "writeAtEach gives ragged planes");
    expect(is(readAtEachRoute(written, c.n, ri), "rows"), "written planes: rows");
    expect(is(readAtEachRoute(writeAtEach(written, c.n, ri, x), c.n, wi), "rows"), "planes written twice: rows");
    expect(is(readAtEachRoute(a, c.n, ri), "pick"), "uniform arrays of one count: pick");
    // uniform planes of different counts: a period with a constant each
    std::vector<CiphertextBatch> mixed;
    for (unsigned j = 0; j < c.w; ++j)
        mixed.push_back(j == 1 ? a.plane(j) + a.plane(j) : a.plane(j));
    expect(is(readAtEachRoute(UIntBatch::fromPlanes(mixed), c.n, ri), "rows"), "uniform planes of different counts: rows");
    // a compact()ed index: element 0 keeps [x, ONE, ZERO], every other element its one term -- ragged
    std::vector<unsigned char> q0(c.count, 0), q1(c.count, 0);
    q0[0] = 1;
    std::vector<CiphertextBatch> pr;
    for (unsigned k = 0; k < c.v; ++k)
        pr.push_back(addPlain(addPlain(ri.plane(k), q0), q1).compact());
    const UIntBatch ragged_index = UIntBatch::fromPlanes(pr);
    expect(!ragged_index.plane(0).uniform(), "compact() gave a ragged index");
    expect(is(readAtEachRoute(written, c.n, ragged_index), "loop"), "a compact()ed index: loop");
    expect(is(readAtEachRoute(a, c.n, ragged_index), "loop"), "a compact()ed index over uniform arrays: loop");
    // arrays without a period: element 0 alone grows
    std::vector<unsigned char> a0(c.n * c.count, 0), a1(c.n * c.count, 0);
    a0[0] = 1;
    std::vector<CiphertextBatch> ar;
    for (unsigned j = 0; j < c.w; ++j)
        ar.push_back(addPlain(addPlain(a.plane(j), a0), a1).compact());
    expect(is(readAtEachRoute(UIntBatch::fromPlanes(ar), c.n, ri), "loop"), "arrays without a period: loop");
    // the loop still reads them, and the written planes under the ragged index
    std::vector<uint64_t> flipped = p.want;
    flipped[0] = p.ri[0] ^ 3u;                          // element 0's read index has both bits flipped
    flipped[0] = flipped[0] < c.n ? (flipped[0] == p.wi[0] ? p.x[0] : p.a[flipped[0]]) : 0;
    checkValues(readAtEach(written, c.n, ragged_index).decrypt(key), flipped, "the loop over a compact()ed index");
    return 0;
}

// The size checks come first: the call throws std::invalid_argument at once, before any allocation or launch.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    // 16 index planes of 3 terms over one row of 1 and 2 terms a plane (period 1): row 0 has 4^16 EQ entries
    const UIntBatch d16 = UIntBatch::encrypt(key, std::vector<uint64_t>(1, 5), 16, 1);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < 16; ++j)
        planes.push_back((d16.plane(j) + d16.plane(j)) + d16.plane(j));
    const UIntBatch three = UIntBatch::fromPlanes(planes);
    std::vector<CiphertextBatch> rows;
    rows.push_back(d16.plane(0));
    rows.push_back(d16.plane(1) + d16.plane(1));
    const UIntBatch arrays = UIntBatch::fromPlanes(rows);
    expect(is(readAtEachRoute(arrays, 1, three), "rows"), "uniform planes of different counts: rows");
    const auto t0 = std::chrono::steady_clock::now();
    const int thrown = throws<std::invalid_argument>([&] { readAtEach(arrays, 1, three); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 1, "an output past 2^31 words per element throws");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // an empty batch: empty planes
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(12, 3), 4, 4);
    const UIntBatch i2 = UIntBatch::encrypt(key, std::vector<uint64_t>(3, 1), 2, 6);
    const UIntBatch x4 = UIntBatch::encrypt(key, std::vector<uint64_t>(3, 9), 4, 8);
    const UIntBatch written = writeAtEach(a4, 4, i2, x4);
    const UIntBatch none = readAtEach(written.slice(0, 0), 4, i2.slice(0, 0));
    expect(none.size() == 0 && none.width() == 4, "an empty batch gives empty planes");
    return 0;
}

// No device work: the form csgn_uint_pick_rows_kernel names for the shapes of words (tables written once from fresh
// planes: row r has 2^zeros(r) * 2 + 1 terms), under the knob the process was started with.
int forms()
{
    for (size_t i = 0; i < kNumCases; ++i) {
        const Case &c = kCases[i];
        const std::vector<uint64_t> one(64, 1);
        std::vector<uint64_t> T;
        for (unsigned j = 0; j < c.w; ++j)
            for (uint64_t r = 0; r < c.n; ++r) {
                unsigned zeros = 0;
                for (unsigned k = 0; k < c.v; ++k)
                    zeros += ((r >> k) & 1u) ? 0 : 1;
                T.push_back((1ull << zeros) * 2 + 1);
            }
        const char *form = csgn_uint_pick_rows_kernel(1247, c.count, c.v, one.data(), c.n, c.w, T.data());
        expect(form && *form, "the operation has a form");
        printf("w=%u v=%u n=%llu count=%zu -> %s\n", c.w, c.v, (unsigned long long)c.n, c.count, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4730, "uint_readback_driver",
                    {{"routes", routes}, {"words", words}, {"oversize", oversize}, {"forms", forms}});
}
