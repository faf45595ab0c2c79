// uint_find_driver.cpp -- user-style C++ over readWhere / matches of include/certfhe/UInt.h: encrypted tables looked up
// by encrypted key (tests/test_uint_find_cpp.py builds and runs it).
//   uint_find_driver words     tables of distinct encrypted keys (full and partial) under encrypted queries: decryptions
//                              == the matching value (0 and member 0 without a match), a duplicated key XORs; words ==
//                              the definition composed from the batch operators; the CiphertextBatch form and matches
//   uint_find_driver ragged    compacted (ragged) keys, values and query, each against the definition; decryptions
//   uint_find_driver oversize  a lookup past 2^31 words per element throws before anything is allocated; mismatched
//                              widths, row counts and contexts, and a table of no rows, throw; an empty query is empty
//   uint_find_driver forms     "<shape> -> <form>": the form csgn_uint_find_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <algorithm>
#include <chrono>
#include <map>
#include <stdexcept>

using namespace certFHE;

namespace {

// the definition of UInt.h, by hand from the batch operators: plane j of the values, or (values null) member
CiphertextBatch definition(const UIntBatch &keys, const CiphertextBatch *values, const UIntBatch &query)
{
    std::vector<CiphertextBatch> acc;
    for (uint64_t r = 0; r < keys.size(); ++r) {
        const CiphertextBatch eq = equalTo(keys.slice(r, r + 1).broadcast(query.size()), query);
        const CiphertextBatch p = values ? eq * values->slice(r, r + 1).broadcast(query.size()) : eq;
        if (acc.empty())
            acc.push_back(p);
        else
            acc[0] = acc[0] + p;
    }
    return acc[0];
}

UIntBatch definition(const UIntBatch &keys, const UIntBatch &values, const UIntBatch &query)
{
    std::vector<CiphertextBatch> out;
    for (unsigned j = 0; j < values.width(); ++j)
        out.push_back(definition(keys, &values.plane(j), query));
    return UIntBatch::fromPlanes(out);
}

// `rows` distinct keys of v bits
std::vector<uint64_t> distinctKeys(unsigned v, size_t rows)
{
    std::vector<uint64_t> all((size_t)1 << v);
    for (size_t i = 0; i < all.size(); ++i)
        all[i] = i;
    for (size_t i = 0; i < rows; ++i)
        std::swap(all[i], all[i + rnd(32) % (all.size() - i)]);
    all.resize(rows);
    return all;
}

struct Case {
    unsigned v, w;
    size_t rows, count;
};
const Case kCases[] = {{8, 8, 40, 6}, {6, 8, 64, 20}, {4, 3, 16, 500}, {4, 5, 9, 500}, {1, 2, 1, 20}};

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (const Case &c : kCases) {
        const std::vector<uint64_t> ks = distinctKeys(c.v, c.rows);
        std::vector<uint64_t> values(c.rows), x(c.count), want(c.count), in(c.count);
        std::map<uint64_t, uint64_t> table;
        for (size_t r = 0; r < c.rows; ++r)
            table[ks[r]] = values[r] = rnd(c.w);
        for (size_t i = 0; i < c.count; ++i) {
            x[i] = i % 2 ? ks[(i / 2) % c.rows] : (i < (1u << c.v) ? i : rnd(c.v));       // every other one is a key
            in[i] = table.count(x[i]);
            want[i] = in[i] ? table[x[i]] : 0;
        }
        const UIntBatch keys = UIntBatch::encrypt(key, ks, c.v, 30 + c.rows);
        const UIntBatch vals = UIntBatch::encrypt(key, values, c.w, 31 + c.rows);
        const UIntBatch query = UIntBatch::encrypt(key, x, c.v, 32 + c.rows);
        const std::string tag = " v=" + std::to_string(c.v) + " rows=" + std::to_string(c.rows);
        CiphertextBatch member = query.plane(0);
        const UIntBatch r = readWhere(keys, vals, query, &member);
        expect(r.width() == c.w, "width" + tag);
        checkValues(r.decrypt(key), want, "uint" + tag);
        const std::vector<unsigned char> mbits = member.decrypt(key), bits = readWhere(keys, vals.plane(0), query).decrypt(key);
        for (size_t i = 0; i < c.count; ++i)
            if (mbits[i] != in[i] || bits[i] != (want[i] & 1u)) {
                expect(false, "member or bit" + tag + " element " + std::to_string(i));
                break;
            }
        // words: a few elements against the definition
        const UIntBatch small = UIntBatch::encrypt(key, std::vector<uint64_t>(x.begin(), x.begin() + 6), c.v, 5);
        CiphertextBatch m2 = small.plane(0);
        expect(sameWords(readWhere(keys, vals, small, &m2), definition(keys, vals, small)), "words == definition" + tag);
        expect(sameBatchWords(m2, definition(keys, nullptr, small)), "member words == definition" + tag);
        expect(sameBatchWords(matches(keys, small), m2), "matches == member" + tag);
        expect(sameWords(readWhere(keys, vals, small), readWhere(keys, vals, small, nullptr)), "null member" + tag);
        expect(sameBatchWords(readWhere(keys, vals.plane(c.w - 1), small), definition(keys, &vals.plane(c.w - 1), small)),
               "batch words == definition" + tag);
    }
    // a duplicated key: the XOR of its two values, member 0
    const UIntBatch keys = UIntBatch::encrypt(key, {5, 2, 5, 7}, 3, 41), vals = UIntBatch::encrypt(key, {9, 3, 12, 6}, 4, 42);
    const UIntBatch query = UIntBatch::encrypt(key, {5, 2, 0}, 3, 43);
    CiphertextBatch member = query.plane(0);
    checkValues(readWhere(keys, vals, query, &member).decrypt(key), {9 ^ 12, 3, 0}, "duplicated key");
    const std::vector<unsigned char> mbits = member.decrypt(key);
    expect(mbits[0] == 0 && mbits[1] == 1 && mbits[2] == 0, "duplicated key: member is the parity");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const size_t count = 60;
    for (unsigned v = 1; v <= 4; ++v) {
        const size_t rows = std::min<size_t>((size_t)1 << v, 2 + rnd(v));   // two rows at least: a ragged table
        const std::vector<uint64_t> ks = distinctKeys(v, rows);
        std::vector<uint64_t> values(rows), x(count);
        for (auto &t : values)
            t = rnd(3);
        for (size_t i = 0; i < count; ++i)
            x[i] = rnd(v);
        const UIntBatch k0 = UIntBatch::encrypt(key, ks, v, 50 + v), t0 = UIntBatch::encrypt(key, values, 3, 60 + v),
                        x0 = UIntBatch::encrypt(key, x, v, 70 + v);
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
        const UIntBatch kr = raggedOf(k0), tr = raggedOf(t0), xr = raggedOf(x0);
        expect(!kr.plane(0).uniform() && !tr.plane(0).uniform() && !xr.plane(0).uniform(), "compact() gave ragged planes");
        const std::string tag = " v=" + std::to_string(v) + " rows=" + std::to_string(rows);
        const uint64_t flip = (1ull << v) - 1;
        auto wanted = [&](const std::vector<uint64_t> &kk, const std::vector<uint64_t> &vv, const std::vector<uint64_t> &xx) {
            std::vector<uint64_t> want(xx.size(), 0);
            for (size_t i = 0; i < xx.size(); ++i)
                for (size_t r = 0; r < kk.size(); ++r)
                    if (kk[r] == xx[i])
                        want[i] ^= vv[r];
            return want;
        };
        std::vector<uint64_t> kf = ks, vf = values, xf = x;
        kf[0] ^= flip;
        vf[0] ^= 7;
        xf[0] ^= flip;
        CiphertextBatch member = x0.plane(0);
        const UIntBatch rq = readWhere(k0, t0, xr, &member);
        expect(sameWords(rq, definition(k0, t0, xr)), "ragged query: words == definition" + tag);
        expect(sameBatchWords(member, definition(k0, nullptr, xr)), "ragged query: member == definition" + tag);
        checkValues(rq.decrypt(key), wanted(ks, values, xf), "ragged query" + tag);
        const UIntBatch rk = readWhere(kr, t0, x0);
        expect(sameWords(rk, definition(kr, t0, x0)), "ragged keys: words == definition" + tag);
        checkValues(rk.decrypt(key), wanted(kf, values, x), "ragged keys" + tag);
        const UIntBatch rt = readWhere(k0, tr, x0);
        expect(sameWords(rt, definition(k0, tr, x0)), "ragged values: words == definition" + tag);
        checkValues(rt.decrypt(key), wanted(ks, vf, x), "ragged values" + tag);
        // elements 1.. of a ragged query hold the uniform query's terms, so the same words
        const UIntBatch uq = readWhere(k0, t0, x0);
        for (unsigned j = 0; j < 3; ++j) {
            bool same = true;
            for (uint64_t i = 1; i < count && same; ++i)
                same = sameWords(uq.plane(j).at(i), rq.plane(j).at(i));
            expect(same, "ragged words == uniform words" + tag);
        }
    }
    return 0;
}

// 16-bit keys and queries of 2 terms a plane at N=1247: 5^16 terms per row.  The size check comes first, so the call
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
    const UIntBatch wide = UIntBatch::fromPlanes(planes);
    const UIntBatch vals = UIntBatch::encrypt(key, std::vector<uint64_t>(count, 3), 2, 2);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { readWhere(wide, vals, wide); });
    thrown += throws<std::invalid_argument>([&] { readWhere(wide, vals.plane(0), wide); });
    thrown += throws<std::invalid_argument>([&] { matches(wide, wide); });
    thrown += throws<std::invalid_argument>([&] { readWhere(x0, vals, x0); });      // 1000 rows of 3^16 terms
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 4, "oversize throws (" + std::to_string(thrown) + " of 4)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // widths, row counts, contexts, no rows
    const UIntBatch k4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    const UIntBatch v10 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 1), 2, 4);
    const UIntBatch x4 = UIntBatch::encrypt(key, std::vector<uint64_t>(7, 3), 4, 5);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { readWhere(k4, v10, UIntBatch::encrypt(key, {1, 2}, 5, 6)); });   // widths
    thrown += throws<std::invalid_argument>([&] { readWhere(k4, v10.slice(0, 9), x4); });                          // rows
    thrown += throws<std::invalid_argument>([&] { readWhere(k4.slice(0, 0), v10.slice(0, 0), x4); });              // no rows
    thrown += throws<std::invalid_argument>([&] { matches(k4.slice(0, 0), x4); });
    thrown += throws<std::invalid_argument>([&] { readWhere(UIntBatch::encrypt(key, {1}, 17, 7), v10.slice(0, 1),
                                                            UIntBatch::encrypt(key, {1}, 17, 8)); });              // 17 bits
    Context other(127, 8);
    SecretKey okey(other);
    thrown += throws<std::invalid_argument>([&] { readWhere(UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 1), 4, 9),
                                                            v10, x4); });
    thrown += throws<std::invalid_argument>([&] { readWhere(k4, UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 1), 2, 9),
                                                            x4); });
    expect(thrown == 7, "bad widths, rows and contexts throw (" + std::to_string(thrown) + " of 7)");
    // an empty query batch: empty planes
    CiphertextBatch member = x4.plane(0);
    const UIntBatch none = readWhere(k4, v10, x4.slice(0, 0), &member);
    expect(none.width() == 2 && none.size() == 0 && member.size() == 0, "an empty query gives empty planes");
    return 0;
}

// No device work: the form csgn_uint_find_kernel names for the shapes of words (fresh planes), under the knob the
// process was started with.
int forms()
{
    for (const Case &c : kCases) {
        const std::vector<uint64_t> one(c.v, 1), t(c.w, 1);
        const char *form = csgn_uint_find_kernel(1247, c.count, c.v, one.data(), one.data(), c.rows, c.w, t.data(), 1);
        expect(form && *form, "the lookup has a form");
        printf("v=%u rows=%zu w=%u -> %s\n", c.v, c.rows, c.w, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4719, "uint_find_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
