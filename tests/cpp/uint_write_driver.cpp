// uint_write_driver.cpp -- user-style C++ over writeAtEach / writeAt of include/certfhe/UInt.h
// (tests/test_uint_write_cpp.py builds and runs it).
//   uint_write_driver words     writeAtEach at N=1247 against the same arrays written with the public operators -- per row
//                               r logicMux(equalTo(index, r), value, the gathered row), concatenated and permuted into
//                               the arrays' layout -- word for word; every row's termsOf against the closed form; the
//                               decryptions against plain arrays, every index included; multi-term planes; writeAt; the
//                               read-back readAtEach(writeAtEach(a, n, i, x), n, i)
//   uint_write_driver ragged    compact()ed operands take the composed route: the same words and the same decryptions
//   uint_write_driver oversize  an array past 2^31 words throws before anything is allocated; mismatched widths, counts
//                               and contexts and bad row counts throw; an empty batch is empty
//   uint_write_driver forms     "<shape> -> <form>": the form csgn_uint_write_kernel names under the process's knob
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

uint64_t maskOf(unsigned w) { return w == 64 ? ~0ull : (1ull << w) - 1; }

std::vector<uint64_t> rowIndices(uint64_t m, uint64_t n, uint64_t r)
{
    std::vector<uint64_t> idx(m);
    for (uint64_t e = 0; e < m; ++e)
        idx[e] = e * n + r;
    return idx;
}

// the definition with the public operators: row r of every array is logicMux(equalTo(index, r), value, row r), and the
// rows go back to the arrays' layout (element e * n + r) by concat and a permuting gather
UIntBatch viaOperators(const Case &c, const UIntBatch &arrays, const UIntBatch &index, const UIntBatch &value)
{
    const uint64_t m = index.size();
    std::vector<uint64_t> perm(c.n * m);
    for (uint64_t e = 0; e < m; ++e)
        for (uint64_t r = 0; r < c.n; ++r)
            perm[e * c.n + r] = r * m + e;
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < c.w; ++j) {
        std::vector<CiphertextBatch> rows;
        for (uint64_t r = 0; r < c.n; ++r)
            rows.push_back(logicMux(equalTo(index, r), value.plane(j), arrays.plane(j).gather(rowIndices(m, c.n, r))));
        planes.push_back(CiphertextBatch::concat(rows).gather(perm));
    }
    return UIntBatch::fromPlanes(planes);
}

struct Plain {
    std::vector<uint64_t> a, i, x, want;
};

// every index among the first arrays; the first value has every bit of the row it replaces flipped
Plain draw(const Case &c)
{
    Plain p;
    for (size_t e = 0; e < c.count; ++e) {
        p.i.push_back(e < (1ull << c.v) ? e : rnd(c.v));
        for (uint64_t r = 0; r < c.n; ++r)
            p.a.push_back(rnd(c.w));
        p.x.push_back(e == 0 ? p.a[0] ^ maskOf(c.w) : rnd(c.w));
    }
    return p;
}

void fillWant(const Case &c, Plain &p)
{
    p.want = p.a;
    for (size_t e = 0; e < c.count; ++e)
        if (p.i[e] < c.n)
            p.want[e * c.n + p.i[e]] = p.x[e];
}

std::string tagOf(const Case &c)
{
    return " w=" + std::to_string(c.w) + " v=" + std::to_string(c.v) + " n=" + std::to_string(c.n) + " count=" +
           std::to_string(c.count);
}

void check(const SecretKey &key, const Case &c, const UIntBatch &arrays, const UIntBatch &index, const UIntBatch &value,
           const std::vector<uint64_t> &want, const std::string &tag)
{
    const UIntBatch got = writeAtEach(arrays, c.n, index, value);
    expect(got.size() == c.n * c.count && got.width() == c.w, "the result has the arrays' shape" + tag);
    expect(sameWords(got, viaOperators(c, arrays, index, value)), "writeAtEach == the rows of logicMux" + tag);
    checkValues(got.decrypt(key), want, "decryption" + tag);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (size_t i = 0; i < kNumCases; ++i) {
        const Case &c = kCases[i];
        Plain p = draw(c);
        fillWant(c, p);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 30 + i), d = UIntBatch::encrypt(key, p.i, c.v, 60 + i);
        const UIntBatch x = UIntBatch::encrypt(key, p.x, c.w, 90 + i);
        check(key, c, a, d, x, p.want, tagOf(c));
        // fresh planes: row r has 2^zeros(r) * (1 + 1) + 1 terms, in every array
        const UIntBatch got = writeAtEach(a, c.n, d, x);
        for (unsigned j = 0; j < c.w; ++j) {
            expect(!got.plane(j).uniform(), "the planes are ragged" + tagOf(c));
            for (uint64_t e = 0; e < c.count; ++e)
                for (uint64_t r = 0; r < c.n; ++r) {
                    unsigned zeros = 0;
                    for (unsigned k = 0; k < c.v; ++k)
                        zeros += ((r >> k) & 1u) ? 0 : 1;
                    expect(got.plane(j).termsOf(e * c.n + r) == (1ull << zeros) * 2 + 1,
                           "termsOf(e * n + r) is the closed form" + tagOf(c));
                }
        }
        expect(sameBatchWords(writeAtEach(a.plane(0), c.n, d, x.plane(0)), got.plane(0)),
               "writeAtEach of bits == plane 0" + tagOf(c));
    }
    // multi-term planes (XOR with a trivial ZERO: two terms a plane): the multi-term path, the same values
    for (size_t i = 0; i < kNumCases; i += 2) {
        Case c = kCases[i];
        c.count = std::min<size_t>(c.count, 6);
        Plain p = draw(c);
        fillWant(c, p);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 120 + i), d = UIntBatch::encrypt(key, p.i, c.v, 150 + i);
        const UIntBatch x = UIntBatch::encrypt(key, p.x, c.w, 180 + i);
        const UIntBatch za = UIntBatch::constant(ctx, std::vector<uint64_t>(p.a.size(), 0), c.w);
        const UIntBatch zd = UIntBatch::constant(ctx, std::vector<uint64_t>(p.i.size(), 0), c.v);
        const UIntBatch zx = UIntBatch::constant(ctx, std::vector<uint64_t>(p.x.size(), 0), c.w);
        check(key, c, a ^ za, d, x, p.want, " multi-term arrays" + tagOf(c));
        check(key, c, a, d ^ zd, x, p.want, " multi-term index" + tagOf(c));
        check(key, c, a, d, x ^ zx, p.want, " multi-term value" + tagOf(c));
    }
    // writeAt: one index and value, the whole batch one table
    {
        const Case c = {4, 3, 6, 1};
        Plain p = draw(c);
        p.i[0] = 4;
        fillWant(c, p);
        const UIntBatch table = UIntBatch::encrypt(key, p.a, c.w, 210), d = UIntBatch::encrypt(key, p.i, c.v, 211);
        const UIntBatch x = UIntBatch::encrypt(key, p.x, c.w, 212);
        expect(sameWords(writeAt(table, d, x), writeAtEach(table, c.n, d, x)), "writeAt == writeAtEach with n = table.size()");
        checkValues(writeAt(table, d, x).decrypt(key), p.want, "writeAt");
    }
    // the read-back through the composed read of ragged planes: what was written is what is read where i < n
    {
        const Case c = kCases[0];                   // v = 2, n = 3, w = 3
        Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 220), d = UIntBatch::encrypt(key, p.i, c.v, 221);
        const UIntBatch x = UIntBatch::encrypt(key, p.x, c.w, 222);
        std::vector<uint64_t> back(c.count);
        for (size_t e = 0; e < c.count; ++e)
            back[e] = p.i[e] < c.n ? p.x[e] : 0;
        checkValues(readAtEach(writeAtEach(a, c.n, d, x), c.n, d).decrypt(key), back, "readAtEach(writeAtEach(a, n, i, x), n, i)");
    }
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    // plane + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO twice,
    // which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
    auto raggedOf = [&](const UIntBatch &x) {
        std::vector<unsigned char> q0(x.size(), 0), q1(x.size(), 0);
        q0[0] = 1;
        std::vector<CiphertextBatch> pr;
        for (unsigned j = 0; j < x.width(); ++j)
            pr.push_back(addPlain(addPlain(x.plane(j), q0), q1).compact());
        return UIntBatch::fromPlanes(pr);
    };
    for (size_t i = 0; i < kNumCases; ++i) {
        Case c = kCases[i];
        if (c.n > 8)
            continue;
        c.count = std::min<size_t>(c.count, 8);
        if (c.count < 2)
            continue;
        const Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 250 + i), d = UIntBatch::encrypt(key, p.i, c.v, 280 + i);
        const UIntBatch x = UIntBatch::encrypt(key, p.x, c.w, 310 + i);
        const UIntBatch ar = raggedOf(a), dr = raggedOf(d), xr = raggedOf(x);
        expect(!ar.plane(0).uniform() && !dr.plane(0).uniform() && !xr.plane(0).uniform(),
               "compact() gave ragged planes" + tagOf(c));
        // element 0 of a ragged operand has every bit flipped
        Plain pa = p, pd = p, px = p;
        pa.a[0] ^= maskOf(c.w);
        pd.i[0] ^= maskOf(c.v);
        px.x[0] ^= maskOf(c.w);
        fillWant(c, pa);
        fillWant(c, pd);
        fillWant(c, px);
        check(key, c, ar, d, x, pa.want, " ragged arrays" + tagOf(c));
        check(key, c, a, dr, x, pd.want, " ragged index" + tagOf(c));
        check(key, c, a, d, xr, px.want, " ragged value" + tagOf(c));
    }
    return 0;
}

// The size checks come first: the calls throw std::invalid_argument at once, before any allocation or launch.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 1000;
    std::vector<uint64_t> x(count);
    for (size_t i = 0; i < count; ++i)
        x[i] = rnd(16);
    const UIntBatch d16 = UIntBatch::encrypt(key, x, 16, 1);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < 16; ++j)
        planes.push_back((d16.plane(j) + d16.plane(j)) + d16.plane(j));
    const UIntBatch three = UIntBatch::fromPlanes(planes);          // 16 planes of 3 terms
    const UIntBatch one16 = d16.slice(0, 1), three16 = three.slice(0, 1);
    const UIntBatch d27 = UIntBatch::encrypt(key, std::vector<uint64_t>(1, 5), 27, 3);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    // one array of one row under a 16-bit index: row 0 has 2^16 entries of EQ
    thrown += throws<std::invalid_argument>([&] { writeAtEach(three16, 1, three16, three16); });   // 4^16 * 6 terms
    thrown += throws<std::invalid_argument>([&] { writeAt(three16, three16, one16); });
    thrown += throws<std::invalid_argument>([&] { writeAtEach(three16.plane(0), 1, three16, one16.plane(0)); });
    // an index past 16 bits takes the composed route: 2^27 entries of two terms and 20 words each
    thrown += throws<std::invalid_argument>([&] { writeAtEach(d27.plane(0), 1, d27, d27.plane(0)); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 4, "oversize throws (" + std::to_string(thrown) + " of 4)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // widths, counts, contexts, rows
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(12, 3), 4, 4);
    const UIntBatch i2 = UIntBatch::encrypt(key, std::vector<uint64_t>(3, 1), 2, 6);
    const UIntBatch x4 = UIntBatch::encrypt(key, std::vector<uint64_t>(3, 9), 4, 8);
    const UIntBatch x3 = UIntBatch::encrypt(key, std::vector<uint64_t>(3, 5), 3, 9);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o2 = UIntBatch::encrypt(okey, std::vector<uint64_t>(3, 1), 2, 7);
    const UIntBatch o4 = UIntBatch::encrypt(okey, std::vector<uint64_t>(3, 1), 4, 10);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 4, i2, x3); });                   // widths
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 4, i2, x4.slice(0, 2)); });       // counts
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 4, i2.slice(0, 2), x4.slice(0, 2)); });
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 4, o2, x4); });                   // contexts
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 4, i2, o4); });
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 0, i2, x4); });                   // n of 0
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 5, i2, x4); });                   // n past 2^2
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4, 3, i2, x4); });                   // 12 != 3 * 3
    thrown += throws<std::invalid_argument>([&] { writeAtEach(a4.plane(0), 3, i2, x4.plane(0)); });
    thrown += throws<std::invalid_argument>([&] { writeAt(a4, i2, x4); });                          // several indices
    expect(thrown == 10, "bad widths, counts, contexts and rows throw (" + std::to_string(thrown) + " of 10)");
    expect(writeAtEach(a4, 4, i2, x4).size() == 12 && writeAtEach(a4, 4, i2, x4).width() == 4, "3 arrays of 4 rows written");
    // an empty batch: empty planes
    const UIntBatch e4 = a4.slice(0, 0), e2 = i2.slice(0, 0), ex = x4.slice(0, 0);
    expect(writeAtEach(e4, 3, e2, ex).size() == 0 && writeAtEach(e4, 3, e2, ex).width() == 4,
           "an empty batch gives empty planes (writeAtEach)");
    return 0;
}

// No device work: the form csgn_uint_write_kernel names for the shapes of words (fresh planes), under the knob the
// process was started with.
int forms()
{
    for (size_t i = 0; i < kNumCases; ++i) {
        const Case &c = kCases[i];
        const std::vector<uint64_t> one(64, 1);
        const char *form = csgn_uint_write_kernel(1247, c.count, c.v, one.data(), c.n, c.w, one.data(), one.data());
        expect(form && *form, "the operation has a form");
        printf("w=%u v=%u n=%llu count=%zu -> %s\n", c.w, c.v, (unsigned long long)c.n, c.count, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4726, "uint_write_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
