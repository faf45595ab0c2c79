// uint_sum_driver.cpp -- user-style C++ over sumValues / sumBit / sumWhere / mul / operator* / innerProduct of
// include/certfhe/UInt.h: encrypted integers summed and multiplied into encrypted integers (tests/test_uint_sum_cpp.py
// builds and runs it).
//   uint_sum_driver values    encrypt, run, decrypt: sums of 4 three-bit integers, a masked sum with a mask from equalTo,
//                             every pair of 4-bit integers multiplied, inner products of 2 rows of 3 x 3 bits
//   uint_sum_driver words     each function, for single elements, against the definition's nested loops written here over
//                             the single-ciphertext operator* and operator+, bit for bit
//   uint_sum_driver ragged    compact()-ed (ragged) operands take the composed route: the same words as the nested loops,
//                             and the same values
//   uint_sum_driver oversize  every bad argument throws std::invalid_argument before anything is allocated, an empty
//                             batch gives empty planes, and a later valid call still works
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include <stdexcept>

using namespace certFHE;

namespace {

typedef std::vector<std::vector<Ciphertext> > Classes;           // [class c][input i] of ONE element

// The definition by hand for ONE element: the nested loops over the count vectors (m_j outermost, m_0 the remainder),
// over the selections (class j slowest, each class's subsets in lexicographic order) and over the members (classes
// descending, indices ascending), in single-ciphertext operators.  run() is false for a plane with no count vector.
struct Definition {
    const Classes &cls;
    unsigned j;
    std::vector<uint64_t> m;
    std::vector<Ciphertext> acc;                                 // empty, or the sum so far

    Definition(const Classes &classes, unsigned plane) : cls(classes), j(plane), m(plane + 1, 0) {}

    uint64_t inputs(unsigned c) const { return c < cls.size() ? cls[c].size() : 0; }

    // the subsets of class c (m[c] members from `from` on), then the lighter classes; prod: the product so far
    void members(unsigned c, uint64_t left, uint64_t from, const std::vector<Ciphertext> &prod)
    {
        if (left == 0) {
            if (c == 0) {
                if (acc.empty())
                    acc.push_back(prod[0]);
                else
                    acc[0] = acc[0] + prod[0];
                return;
            }
            members(c - 1, m[c - 1], 0, prod);
            return;
        }
        for (uint64_t i = from; i + left <= inputs(c); ++i) {
            std::vector<Ciphertext> next(1, prod.empty() ? cls[c][i] : prod[0] * cls[c][i]);
            members(c, left - 1, i + 1, next);
        }
    }

    void vectors(unsigned c, uint64_t rest)
    {
        if (c == 0) {
            if (rest <= inputs(0)) {
                m[0] = rest;
                members(j, m[j], 0, std::vector<Ciphertext>());
            }
            return;
        }
        for (uint64_t k = 0; k <= inputs(c) && (k << c) <= rest; ++k) {
            m[c] = k;
            vectors(c - 1, rest - (k << c));
        }
    }

    bool run()
    {
        vectors(j, 1ull << j);
        return !acc.empty();
    }
};

// plane j of `got` at element q against the nested loops over that element's classes
void checkElement(const UIntBatch &got, uint64_t q, const Classes &cls, const std::string &tag)
{
    for (unsigned j = 0; j < got.width(); ++j) {
        Definition d(cls, j);
        const Ciphertext mine = got.plane(j).at(q);
        if (d.run())
            expect(sameWords(mine, d.acc[0]), tag + ": plane " + std::to_string(j) + " == the nested loops");
        else
            expect(mine.getLen() == got.context().getDefaultN(), tag + ": plane " + std::to_string(j) + " is the one-term ZERO");
    }
}

// the classes of element q of sumValues / sumWhere: class c is plane c (times the mask) of the group's rows
Classes sumClasses(const UIntBatch &a, uint64_t group, uint64_t q, const CiphertextBatch *mask)
{
    Classes cls(a.width());
    for (unsigned c = 0; c < a.width(); ++c)
        for (uint64_t r = 0; r < group; ++r) {
            const Ciphertext bit = a.plane(c).at(q * group + r);
            cls[c].push_back(mask ? mask->at(q * group + r) * bit : bit);
        }
    return cls;
}

// the classes of element q of innerProduct (group = 1: mul): row r slowest, a_i * b_{c-i}, i ascending
Classes productClasses(const UIntBatch &a, const UIntBatch &b, uint64_t group, uint64_t q)
{
    Classes cls(a.width() + b.width() - 1);
    for (unsigned c = 0; c < cls.size(); ++c)
        for (uint64_t r = 0; r < group; ++r)
            for (unsigned i = 0; i < a.width(); ++i)
                if (c >= i && c - i < b.width())
                    cls[c].push_back(a.plane(i).at(q * group + r) * b.plane(c - i).at(q * group + r));
    return cls;
}

std::vector<uint64_t> randomValues(size_t n, unsigned w)
{
    std::vector<uint64_t> v(n);
    for (size_t i = 0; i < n; ++i)
        v[i] = rnd(w);
    return v;
}

struct Inputs {
    Context ctx;
    SecretKey key;
    std::vector<uint64_t> v, tags, x, y, p, q;
    UIntBatch ev, etags, ex, ey, ep, eq;

    Inputs(uint64_t n, uint64_t d)
        : ctx(n, d), key(ctx), v(randomValues(24, 3)), tags(randomValues(24, 2)), x(256), y(256), p(randomValues(12, 3)),
          q(randomValues(12, 3)), ev(UIntBatch::encrypt(key, fix(v), 3, 11)), etags(UIntBatch::encrypt(key, tags, 2, 12)),
          ex(UIntBatch::encrypt(key, pairs(x, y, true), 4, 13)), ey(UIntBatch::encrypt(key, pairs(x, y, false), 4, 14)),
          ep(UIntBatch::encrypt(key, p, 3, 15)), eq(UIntBatch::encrypt(key, q, 3, 16))
    {
    }

    // the first group all sevens, the second all zeros: the largest and the smallest sum
    static const std::vector<uint64_t> &fix(std::vector<uint64_t> &v)
    {
        for (size_t i = 0; i < 4; ++i) {
            v[i] = 7;
            v[4 + i] = 0;
        }
        return v;
    }

    // every pair of 4-bit integers: element e is (e / 16, e % 16)
    static const std::vector<uint64_t> &pairs(std::vector<uint64_t> &x, std::vector<uint64_t> &y, bool first)
    {
        for (size_t e = 0; e < 256; ++e) {
            x[e] = e / 16;
            y[e] = e % 16;
        }
        return first ? x : y;
    }
};

int values()
{
    Inputs in(1247, 16);
    // sums of 4 three-bit integers: at most 28, all five planes
    {
        const UIntBatch s = sumValues(in.ev, 4, 5);
        std::vector<uint64_t> want(6, 0);
        for (size_t i = 0; i < in.v.size(); ++i)
            want[i / 4] += in.v[i];
        expect(s.width() == 5 && s.size() == 6, "sumValues shape");
        const uint64_t T[5] = {4, 10, 35, 161, 315};
        for (unsigned j = 0; j < 5; ++j)
            expect(s.plane(j).terms() == T[j], "sumValues terms of plane " + std::to_string(j));
        expect(s.plane(0).deviceValues() == in.ev.plane(0).deviceValues(), "plane 0 shares the payload");
        checkValues(s.decrypt(in.key), want, "sumValues");
        for (unsigned j = 0; j < 6; ++j) {
            const std::vector<unsigned char> bit = sumBit(in.ev, 4, j).decrypt(in.key);
            for (size_t e = 0; e < want.size(); ++e)
                expect(bit[e] == ((want[e] >> j) & 1), "sumBit " + std::to_string(j) + " element " + std::to_string(e));
        }
        for (size_t e = 0; e < want.size(); ++e)
            want[e] &= 3;
        checkValues(sumValues(in.ev, 4, 2).decrypt(in.key), want, "sumValues modulo 4");
    }
    // SUM(value) WHERE tag == 2, over groups of 3 rows, modulo 16
    {
        const CiphertextBatch mask = equalTo(in.etags, 2);
        const UIntBatch s = sumWhere(mask, in.ev, 3, 4);
        std::vector<uint64_t> want(8, 0);
        for (size_t i = 0; i < in.v.size(); ++i)
            want[i / 3] += in.tags[i] == 2 ? in.v[i] : 0;
        for (size_t e = 0; e < want.size(); ++e)
            want[e] &= 15;
        checkValues(s.decrypt(in.key), want, "sumWhere");
    }
    // every pair of 4-bit integers, to 8 planes and modulo 16
    {
        const UIntBatch full = mul(in.ex, in.ey, 8), low = in.ex * in.ey;
        std::vector<uint64_t> want(256), want16(256);
        for (size_t e = 0; e < 256; ++e) {
            want[e] = in.x[e] * in.y[e];
            want16[e] = want[e] & 15;
        }
        const uint64_t T[8] = {1, 2, 4, 10, 34, 129, 383, 511};
        for (unsigned j = 0; j < 8; ++j)
            expect(full.plane(j).terms() == T[j], "mul terms of plane " + std::to_string(j));
        checkValues(full.decrypt(in.key), want, "mul");
        expect(low.width() == 4, "operator* keeps the width");
        checkValues(low.decrypt(in.key), want16, "operator*");
        for (unsigned j = 0; j < 4; ++j)
            expect(sameBatchWords(low.plane(j), full.plane(j)), "operator* has mul's low planes");
    }
    // inner products of 2 rows of 3 x 3 bits: at most 98, seven planes
    {
        const UIntBatch s = innerProduct(in.ep, in.eq, 2, 7);
        std::vector<uint64_t> want(6, 0);
        for (size_t i = 0; i < in.p.size(); ++i)
            want[i / 2] += in.p[i] * in.q[i];
        checkValues(s.decrypt(in.key), want, "innerProduct");
    }
    return 0;
}

int words()
{
    Inputs in(1247, 16);
    // fresh operands, and operands of two terms a plane
    std::vector<CiphertextBatch> two;
    for (unsigned j = 0; j < 3; ++j)
        two.push_back(in.ev.plane(j) + CiphertextBatch::encrypt(in.key, std::vector<unsigned char>(in.ev.size(), 0), 21 + j));
    const UIntBatch ev2 = UIntBatch::fromPlanes(two);
    const UIntBatch *both[2] = {&in.ev, &ev2};
    for (int v = 0; v < 2; ++v) {
        const UIntBatch &a = *both[v];
        const std::string tag = " t=" + std::to_string(v + 1);
        const unsigned planes = v == 0 ? 6 : 4;                  // plane 5 of 4 three-bit integers has no count vector
        const UIntBatch s = sumValues(a, 4, planes);
        for (uint64_t q = 0; q < 3; ++q)
            checkElement(s, q, sumClasses(a, 4, q, nullptr), "sumValues" + tag + " element " + std::to_string(q));
        for (unsigned j = 0; j < planes; ++j)
            expect(sameBatchWords(sumBit(a, 4, j), s.plane(j)), "sumBit == the plane of sumValues" + tag);
    }
    {
        const CiphertextBatch mask = equalTo(in.etags, 2);
        const UIntBatch s = sumWhere(mask, in.ev, 3, 4);
        for (uint64_t q = 0; q < 2; ++q)
            checkElement(s, q, sumClasses(in.ev, 3, q, &mask), "sumWhere element " + std::to_string(q));
    }
    // the top plane, which takes no part in the low two planes of the sum, has two terms: the sizes are the low planes'
    {
        const UIntBatch top = UIntBatch::fromPlanes(std::vector<CiphertextBatch>{in.ev.plane(0), in.ev.plane(1), ev2.plane(2)});
        const UIntBatch s = sumValues(top, 4, 2);
        expect(s.plane(1).terms() == 10, "a plane that takes no part does not size the sum");
        for (uint64_t q = 0; q < 3; ++q)
            checkElement(s, q, sumClasses(UIntBatch::fromPlanes(std::vector<CiphertextBatch>{in.ev.plane(0), in.ev.plane(1)}), 4, q, nullptr),
                         "sumValues under a wider top plane, element " + std::to_string(q));
        expect(sameBatchWords(sumBit(top, 4, 1), s.plane(1)), "sumBit under a wider top plane");
        const CiphertextBatch mask = CiphertextBatch::encrypt(in.key, randomBits(in.ev.size()), 31);
        const UIntBatch w = sumWhere(mask, top, 3, 2);
        expect(w.plane(1).terms() == 3 + 3, "sumWhere under a wider top plane: terms");
        checkElement(w, 1, sumClasses(UIntBatch::fromPlanes(std::vector<CiphertextBatch>{in.ev.plane(0), in.ev.plane(1)}), 3, 1, &mask),
                     "sumWhere under a wider top plane");
    }
    {
        const UIntBatch full = mul(in.ex, in.ey, 8), low = in.ex * in.ey;
        const uint64_t some[2] = {0x5b, 0xff};
        for (int k = 0; k < 2; ++k)
            checkElement(full, some[k], productClasses(in.ex, in.ey, 1, some[k]), "mul element " + std::to_string(some[k]));
        for (unsigned j = 0; j < 4; ++j)
            expect(sameBatchWords(low.plane(j), full.plane(j)), "operator* has mul's low planes");
        // different widths: 4 bits by 2 bits
        const UIntBatch narrow = UIntBatch::fromPlanes(std::vector<CiphertextBatch>{in.ey.plane(0), in.ey.plane(1)});
        const UIntBatch m = mul(in.ex, narrow, 6);
        checkElement(m, 0x5b, productClasses(in.ex, narrow, 1, 0x5b), "mul 4 x 2 bits");
    }
    {
        const UIntBatch s = innerProduct(in.ep, in.eq, 2, 7);
        for (uint64_t q = 0; q < 2; ++q)
            checkElement(s, q, productClasses(in.ep, in.eq, 2, q), "innerProduct element " + std::to_string(q));
    }
    return 0;
}

int ragged()
{
    Inputs in(127, 8);
    // x + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO twice, which
    // cancels: the batch is ragged
    auto raggedOf = [&](const CiphertextBatch &x) {
        std::vector<unsigned char> p(x.size(), 0), q(x.size(), 0);
        p[0] = 1;
        return addPlain(addPlain(x, p), q).compact();
    };
    auto withRaggedPlane = [&](const UIntBatch &a, unsigned which) {
        std::vector<CiphertextBatch> planes;
        for (unsigned j = 0; j < a.width(); ++j)
            planes.push_back(j == which ? raggedOf(a.plane(j)) : a.plane(j));
        expect(!planes[which].uniform(), "compact() gave a ragged plane");
        return UIntBatch::fromPlanes(planes);
    };
    // sums: element 0 of plane 1 flipped, value 0 changes by 2
    {
        const UIntBatch er = withRaggedPlane(in.ev, 1);
        std::vector<uint64_t> v(in.v), want(6, 0);
        v[0] ^= 2;
        for (size_t i = 0; i < v.size(); ++i)
            want[i / 4] += v[i];
        const UIntBatch s = sumValues(er, 4, 5), u = sumValues(in.ev, 4, 5);
        checkValues(s.decrypt(in.key), want, "ragged sumValues");
        for (uint64_t q = 0; q < 2; ++q)
            checkElement(s, q, sumClasses(er, 4, q, nullptr), "ragged sumValues element " + std::to_string(q));
        for (unsigned j = 0; j < 5; ++j)
            for (uint64_t q = 1; q < 6; ++q)
                expect(sameWords(s.plane(j).at(q), u.plane(j).at(q)), "ragged words == uniform words, element " + std::to_string(q));
        // a ragged mask
        const CiphertextBatch mask = raggedOf(equalTo(in.etags, 2));
        std::vector<uint64_t> wantw(8, 0);
        for (size_t i = 0; i < in.v.size(); ++i)
            wantw[i / 3] += ((in.tags[i] == 2) != (i == 0)) ? in.v[i] : 0;
        for (size_t e = 0; e < wantw.size(); ++e)
            wantw[e] &= 15;
        const UIntBatch w = sumWhere(mask, in.ev, 3, 4);
        checkValues(w.decrypt(in.key), wantw, "ragged sumWhere");
        checkElement(w, 0, sumClasses(in.ev, 3, 0, &mask), "ragged sumWhere element 0");
    }
    // products of a few pairs: bit 2 of the first x flipped
    {
        const std::vector<uint64_t> some = {0x30, 0x5b, 0xff, 0x37, 0xc4, 0x9e};
        const UIntBatch xr = withRaggedPlane(in.ex.gather(some), 2), ys = in.ey.gather(some);
        std::vector<uint64_t> want(some.size()), want16(some.size());
        for (size_t e = 0; e < some.size(); ++e) {
            want[e] = (in.x[some[e]] ^ (e == 0 ? 4 : 0)) * in.y[some[e]];
            want16[e] = want[e] & 15;
        }
        const UIntBatch full = mul(xr, ys, 8);
        checkValues(full.decrypt(in.key), want, "ragged mul");
        checkValues((xr * ys).decrypt(in.key), want16, "ragged operator*");
        checkElement(full, 0, productClasses(xr, ys, 1, 0), "ragged mul element 0");
        checkElement(full, 1, productClasses(xr, ys, 1, 1), "ragged mul element 1");
        const UIntBatch pr = withRaggedPlane(in.ep, 0);
        std::vector<uint64_t> wanti(6, 0);
        for (size_t i = 0; i < in.p.size(); ++i)
            wanti[i / 2] += (in.p[i] ^ (i == 0 ? 1 : 0)) * in.q[i];
        for (size_t e = 0; e < wanti.size(); ++e)
            wanti[e] &= 15;
        // sizes are bounded by the largest element (three terms): the low four planes
        const UIntBatch s = innerProduct(pr, in.eq, 2, 4);
        checkValues(s.decrypt(in.key), wanti, "ragged innerProduct");
        checkElement(s, 0, productClasses(pr, in.eq, 2, 0), "ragged innerProduct element 0");
    }
    return 0;
}

int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const UIntBatch a8 = UIntBatch::encrypt(key, randomValues(128, 8), 8, 61), a3 = UIntBatch::encrypt(key, randomValues(128, 3), 3, 62);
    const CiphertextBatch mask = CiphertextBatch::encrypt(key, randomBits(128), 63);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o3 = UIntBatch::encrypt(okey, randomValues(128, 3), 3, 64);
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { sumValues(a8, 64, 8); });                  // plane 3: C(64, 8) terms and more
    thrown += throws<std::invalid_argument>([&] { sumBit(a8, 64, 3); });
    thrown += throws<std::invalid_argument>([&] { sumWhere(mask, a8, 64, 4); });
    thrown += throws<std::invalid_argument>([&] { innerProduct(a8, a8, 64, 4); });
    thrown += throws<std::invalid_argument>([&] { mul(a8, a8, 16); });                       // the top planes of 8 x 8 bits
    thrown += throws<std::invalid_argument>([&] { sumValues(a3, 0, 2); });                   // groups
    thrown += throws<std::invalid_argument>([&] { sumValues(a3, 5, 2); });
    thrown += throws<std::invalid_argument>([&] { sumWhere(mask, a3, 3, 2); });
    thrown += throws<std::invalid_argument>([&] { innerProduct(a3, a3, 256, 2); });
    thrown += throws<std::invalid_argument>([&] { sumValues(a3, 4, 0); });                   // planes
    thrown += throws<std::invalid_argument>([&] { sumValues(a3, 4, 65); });
    thrown += throws<std::invalid_argument>([&] { mul(a3, a3, 0); });
    thrown += throws<std::invalid_argument>([&] { sumWhere(mask.slice(0, 64), a3, 4, 2); }); // counts
    thrown += throws<std::invalid_argument>([&] { mul(a3, a3.slice(0, 64), 3); });
    thrown += throws<std::invalid_argument>([&] { mul(a3, o3, 3); });                        // contexts
    thrown += throws<std::invalid_argument>([&] { innerProduct(a3, o3, 2, 3); });
    expect(thrown == 16, "bad arguments throw (" + std::to_string(thrown) + " of 16)");
    // an empty batch: empty planes
    const UIntBatch none = sumValues(a3.slice(0, 0), 4, 3);
    expect(none.width() == 3 && none.size() == 0, "an empty batch gives empty planes");
    expect(mul(a3.slice(0, 0), a3.slice(0, 0), 5).size() == 0, "an empty product gives empty planes");
    // a later valid call still works
    const UIntBatch c = sumValues(a8, 64, 2);
    expect(c.size() == 2 && c.plane(1).terms() == 2016 + 64, "a valid call after the refused ones");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4727, "uint_sum_driver",
                    {{"values", values}, {"words", words}, {"ragged", ragged}, {"oversize", oversize}});
}
