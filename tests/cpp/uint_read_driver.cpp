// uint_read_driver.cpp -- user-style C++ over readAt of include/certfhe/UInt.h: encrypted tables read at encrypted
// indices (tests/test_uint_read_cpp.py builds and runs it).
//   uint_read_driver words     UIntBatch tables (full and partial) at encrypted 8- and 4-bit indices: decryptions ==
//                              table[x] (0 past the table), words == the definition composed from CiphertextBatch
//                              operators; the CiphertextBatch form likewise
//   uint_read_driver ragged    compacted (ragged) index and table planes: elements holding the same terms as the
//                              uniform planes give the same words; every word == the definition; decryptions
//   uint_read_driver oversize  a read past 2^31 words per element throws before anything is allocated; bad row counts
//                              and mismatched contexts throw
//   uint_read_driver forms   "<shape> -> <form>": the form csgn_uint_read_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

// the definition of UInt.h, by hand from the batch operators
CiphertextBatch definition(const CiphertextBatch &table, const UIntBatch &index)
{
    std::vector<CiphertextBatch> acc;
    for (uint64_t r = 0; r < table.size(); ++r) {
        const CiphertextBatch p = equalTo(index, r) * table.slice(r, r + 1).broadcast(index.size());
        if (acc.empty())
            acc.push_back(p);
        else
            acc[0] = acc[0] + p;
    }
    return acc[0];
}

UIntBatch definition(const UIntBatch &table, const UIntBatch &index)
{
    std::vector<CiphertextBatch> out;
    for (unsigned j = 0; j < table.width(); ++j)
        out.push_back(definition(table.plane(j), index));
    return UIntBatch::fromPlanes(out);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    struct Case {
        unsigned v, w;
        size_t rows, count;
    } cases[] = {{8, 8, 256, 300}, {8, 8, 200, 300}, {4, 3, 16, 500}, {4, 5, 9, 500}, {1, 2, 1, 20}};
    for (const Case &c : cases) {
        std::vector<uint64_t> values(c.rows), x(c.count), want(c.count);
        for (auto &t : values)
            t = rnd(c.w);
        for (size_t i = 0; i < c.count; ++i) {
            x[i] = i < (1u << c.v) ? i : rnd(c.v);
            want[i] = x[i] < c.rows ? values[x[i]] : 0;
        }
        const UIntBatch table = UIntBatch::encrypt(key, values, c.w, 31 + c.rows);
        const UIntBatch index = UIntBatch::encrypt(key, x, c.v, 32 + c.rows);
        const std::string tag = " v=" + std::to_string(c.v) + " rows=" + std::to_string(c.rows);
        const UIntBatch r = readAt(table, index);
        expect(r.width() == c.w, "width" + tag);
        checkValues(r.decrypt(key), want, "uint" + tag);
        // the CiphertextBatch form: plane 0 alone
        const CiphertextBatch b = readAt(table.plane(0), index);
        const std::vector<unsigned char> bits = b.decrypt(key);
        for (size_t i = 0; i < c.count; ++i)
            if (bits[i] != (want[i] & 1u)) {
                expect(false, "bit" + tag + " element " + std::to_string(i));
                break;
            }
        // words: a few elements against the definition
        const UIntBatch small = UIntBatch::encrypt(key, std::vector<uint64_t>(x.begin(), x.begin() + 8), c.v, 5);
        expect(sameWords(readAt(table, small), definition(table, small)), "words == definition" + tag);
        expect(sameBatchWords(readAt(table.plane(c.w - 1), small), definition(table.plane(c.w - 1), small)),
               "batch words == definition" + tag);
    }
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const size_t count = 100;
    for (unsigned v = 1; v <= 4; ++v) {
        const size_t rows = std::min<size_t>((size_t)1 << v, 2 + rnd(v));   // two rows at least: a ragged table
        std::vector<uint64_t> values(rows), x(count);
        for (auto &t : values)
            t = rnd(3);
        for (size_t i = 0; i < count; ++i)
            x[i] = rnd(v);
        const UIntBatch t0 = UIntBatch::encrypt(key, values, 3, 60 + v), x0 = UIntBatch::encrypt(key, x, v, 70 + v);
        // plane + p + q, compacted: element 0 keeps [a, ONE, ZERO] (its bit flips), every other element adds ZERO
        // twice, which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
        auto raggedOf = [&](const UIntBatch &a) {
            std::vector<unsigned char> p(a.size(), 0), q(a.size(), 0);
            p[0] = 1;
            std::vector<CiphertextBatch> pr;
            for (unsigned j = 0; j < a.width(); ++j)
                pr.push_back(addPlain(addPlain(a.plane(j), p), q).compact());
            return UIntBatch::fromPlanes(pr);
        };
        const UIntBatch xr = raggedOf(x0), tr = raggedOf(t0);
        expect(!xr.plane(0).uniform() && !tr.plane(0).uniform(), "compact() gave ragged planes");
        std::vector<uint64_t> xv = x, vv = values;
        xv[0] ^= (1ull << v) - 1;
        vv[0] ^= 7;
        const std::string tag = " v=" + std::to_string(v) + " rows=" + std::to_string(rows);
        // a ragged index over the uniform table: elements 1.. hold the uniform index's terms, so the same words
        const UIntBatch u = readAt(t0, x0), r = readAt(t0, xr);
        for (unsigned j = 0; j < 3; ++j) {
            bool same = true;
            for (uint64_t i = 1; i < count && same; ++i) {
                const Ciphertext ci = u.plane(j).at(i), ri = r.plane(j).at(i);
                same = ci.getLen() == ri.getLen() && memcmp(ci.getValues(), ri.getValues(), ci.getLen() * 8) == 0;
            }
            expect(same, "ragged words == uniform words" + tag);
        }
        expect(sameWords(r, definition(t0, xr)), "ragged index: words == definition" + tag);
        const UIntBatch rt = readAt(tr, x0);
        expect(sameWords(rt, definition(tr, x0)), "ragged table: words == definition" + tag);
        std::vector<uint64_t> want(count), want_t(count);
        for (size_t i = 0; i < count; ++i) {
            want[i] = xv[i] < rows ? values[xv[i]] : 0;
            want_t[i] = x[i] < rows ? vv[x[i]] : 0;
        }
        checkValues(r.decrypt(key), want, "ragged index" + tag);
        checkValues(rt.decrypt(key), want_t, "ragged table" + tag);
    }
    return 0;
}

// 16-bit indices of 2 terms a plane at N=1247: 5^16 terms per element.  The size check comes first, so the call
// throws std::invalid_argument at once, before any allocation or launch.
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
        planes.push_back(x0.plane(j) + x0.plane(j));
    const UIntBatch index = UIntBatch::fromPlanes(planes);
    const UIntBatch table = UIntBatch::encrypt(key, std::vector<uint64_t>(1000, 3), 2, 2);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    try {
        readAt(table, index);
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    try {
        readAt(table.plane(0), index);
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 2, "oversize throws (" + std::to_string(thrown) + " of 2)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // bad row counts and contexts
    const UIntBatch x4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    thrown = 0;
    try {
        readAt(UIntBatch::encrypt(key, std::vector<uint64_t>(17, 1), 2, 4), x4);      // 17 rows for a 4-bit index
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    try {
        readAt(table.plane(0).slice(0, 0), x4);                                       // no rows
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    Context other(127, 8);
    SecretKey okey(other);
    try {
        readAt(UIntBatch::encrypt(okey, std::vector<uint64_t>(16, 1), 2, 5), x4);    // another context
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    expect(thrown == 3, "bad rows and contexts throw (" + std::to_string(thrown) + " of 3)");
    return 0;
}

// No device work: the form csgn_uint_read_kernel names for the shapes of words (fresh planes), under the knob the
// process was started with.
int forms()
{
    const struct {
        unsigned v, w;
        size_t rows, count;
    } cases[] = {{8, 8, 256, 300}, {8, 8, 200, 300}, {4, 3, 16, 500}, {4, 5, 9, 500}, {1, 2, 1, 20}};
    for (const auto &c : cases) {
        const std::vector<uint64_t> s(c.v, 1), t(c.w, 1);
        const char *form = csgn_uint_read_kernel(1247, c.count, c.v, s.data(), c.rows, c.w, t.data());
        expect(form && *form, "the read has a form");
        printf("v=%u rows=%zu w=%u -> %s\n", c.v, c.rows, c.w, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4713, "uint_read_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
