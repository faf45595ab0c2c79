// uint_bilinear_driver.cpp -- user-style C++ over F2Bilinear, bilinearMap, clmul, clmulWide, gfMul, dotBits,
// bilinearRoute and F2Matrix::gfSquare of include/certfhe/UInt.h (tests/test_uint_bilinear_cpp.py builds and runs it).
//   uint_bilinear_driver words    at N=1247: the class results word for word against the composed form written out with
//                                 concat / gather / operator* / sumGroups and against the chain of operator* and
//                                 operator+; clmul, clmulWide, gfMul(8, 0x11B), bitwiseAnd against a & b, dotBits;
//                                 constants, empty rows, planes of several terms, squares (b IS a); the host algebra;
//                                 the inverses of GF(16) as x^14 = x^2 * x^4 * x^8, end to end
//   uint_bilinear_driver ragged   a compact()ed (ragged) operand takes the loop: the same words as the chain of
//                                 operators and as the gather form, and the same decryptions
//   uint_bilinear_driver errors   every std::invalid_argument of F2Bilinear, bilinearMap and its kin; oversize before
//                                 any launch; an empty batch
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

typedef F2Bilinear::Pair Pair;
typedef std::vector<std::vector<Pair> > Rows;

std::vector<uint64_t> draw(unsigned w, size_t count)
{
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = rnd(w);
    return v;
}

uint64_t lowMask(unsigned w) { return w >= 64 ? ~0ull : (1ull << w) - 1; }

uint64_t clmulClear(uint64_t a, uint64_t b)
{
    uint64_t r = 0;
    for (unsigned i = 0; i < 64; ++i)
        if ((b >> i) & 1u)
            r ^= a << i;
    return r;
}

uint64_t gfMulClear(unsigned w, uint64_t a, uint64_t b, uint64_t poly)
{
    uint64_t r = 0;
    for (unsigned i = 0; i < w; ++i) {
        if (b & 1u)
            r ^= a;
        b >>= 1;
        const bool carry = (a >> (w - 1)) & 1u;
        a = (a << 1) & lowMask(w);
        if (carry)
            a ^= poly & lowMask(w);
    }
    return r;
}

// bit j of X^k mod poly in row j, k < 2w - 1: the reduction of the wide product
F2Matrix reduction(unsigned w, uint64_t poly)
{
    std::vector<uint64_t> rows(w, 0);
    uint64_t c = 1;
    for (unsigned k = 0; k < 2 * w - 1; ++k) {
        for (unsigned j = 0; j < w; ++j)
            if ((c >> j) & 1u)
                rows[j] |= 1ull << k;
        c = gfMulClear(w, c, 2, poly);
    }
    return F2Matrix::fromRows(rows, 2 * w - 1);
}

CiphertextBatch constantOf(const UIntBatch &a, bool bit)
{
    return constantBatch(a.context(), std::vector<unsigned char>(a.size(), bit ? 1 : 0));
}

// the definition through the chain of CiphertextBatch operators: what the loop route issues
UIntBatch byOperators(const UIntBatch &a, const UIntBatch &b, const F2Bilinear &f, uint64_t constant)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned x = 0; x < f.outWidth(); ++x) {
        const std::vector<Pair> &row = f.rows()[x];
        const bool bit = (constant >> x) & 1u;
        if (row.empty()) {
            planes.push_back(constantOf(a, bit));
            continue;
        }
        CiphertextBatch sum = a.plane(row[0].first) * b.plane(row[0].second);
        for (size_t i = 1; i < row.size(); ++i)
            sum = sum + a.plane(row[i].first) * b.plane(row[i].second);
        planes.push_back(bit ? logicNot(sum) : sum);
    }
    return UIntBatch::fromPlanes(planes);
}

// the best a user could write before: two concats, then per plane two gathers, one operator* and sumGroups
UIntBatch byComposed(const UIntBatch &a, const UIntBatch &b, const F2Bilinear &f, uint64_t constant)
{
    const uint64_t count = a.size();
    std::vector<CiphertextBatch> pa, pb;
    for (unsigned j = 0; j < a.width(); ++j)
        pa.push_back(a.plane(j));
    for (unsigned j = 0; j < b.width(); ++j)
        pb.push_back(b.plane(j));
    const CiphertextBatch A = CiphertextBatch::concat(pa), B = CiphertextBatch::concat(pb);
    std::vector<CiphertextBatch> planes;
    for (unsigned x = 0; x < f.outWidth(); ++x) {
        const std::vector<Pair> &row = f.rows()[x];
        const bool bit = (constant >> x) & 1u;
        if (row.empty()) {
            planes.push_back(constantOf(a, bit));
            continue;
        }
        std::vector<uint64_t> li, ri;
        for (uint64_t e = 0; e < count; ++e)
            for (size_t i = 0; i < row.size(); ++i) {
                li.push_back(row[i].first * count + e);
                ri.push_back(row[i].second * count + e);
            }
        const CiphertextBatch sum = (A.gather(li) * B.gather(ri)).sumGroups(row.size());
        planes.push_back(bit ? logicNot(sum) : sum);
    }
    return UIntBatch::fromPlanes(planes);
}

template <typename F>
std::vector<uint64_t> mapped2(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b, F f)
{
    std::vector<uint64_t> v(a.size());
    for (size_t i = 0; i < a.size(); ++i)
        v[i] = f(a[i], b[i]);
    return v;
}

// bilinearMap against both written-out forms word for word (composed = false leaves the gather form out), and the
// clear form
void checkForm(const SecretKey &key, const UIntBatch &a, const std::vector<uint64_t> &va, const UIntBatch &b,
               const std::vector<uint64_t> &vb, const F2Bilinear &f, uint64_t constant, bool composed, const std::string &tag)
{
    const UIntBatch y = bilinearMap(a, b, f, constant);
    expect(y.width() == f.outWidth() && y.size() == a.size(), "the result has the form's output width" + tag);
    expect(sameWords(y, byOperators(a, b, f, constant)), "bilinearMap == the chain of operators" + tag);
    if (composed)
        expect(sameWords(y, byComposed(a, b, f, constant)), "bilinearMap == concat / gather / operator* / sumGroups" + tag);
    checkValues(y.decrypt(key), mapped2(va, vb, [&](uint64_t p, uint64_t q) { return f.apply(p, q) ^ constant; }),
                "bilinearMap decrypted" + tag);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const std::vector<uint64_t> va = draw(8, 40), vb = draw(8, 40);
    const UIntBatch a8 = UIntBatch::encrypt(key, va, 8, 61), b8 = UIntBatch::encrypt(key, vb, 8, 62);
    const F2Bilinear cl = F2Bilinear::clmul(8), wide = F2Bilinear::clmulWide(8), gf = F2Bilinear::gfMul(8, 0x11B);
    expect(std::string(bilinearRoute(a8, b8, cl)) == "k_uint_bilinear", "uniform planes take the launch");
    checkForm(key, a8, va, b8, vb, cl, 0, true, " clmul");
    checkForm(key, a8, va, b8, vb, cl, 0xA5, true, " clmul ^ constant");
    checkForm(key, a8, va, b8, vb, wide, 0x4001, true, " clmulWide");
    checkForm(key, a8, va, b8, vb, gf, 0, true, " gfMul(8, 0x11B)");
    checkForm(key, a8, va, b8, vb, F2Bilinear::dotBits(8), 1, true, " dotBits");
    checkForm(key, a8, va, a8, va, gf, 0, true, " squares: b is a");
    checkValues(clmul(a8, b8).decrypt(key), mapped2(va, vb, [](uint64_t p, uint64_t q) { return clmulClear(p, q) & 0xFF; }), "clmul == the clear product");
    checkValues(clmulWide(a8, b8).decrypt(key), mapped2(va, vb, [](uint64_t p, uint64_t q) { return clmulClear(p, q); }), "clmulWide == the clear product");
    checkValues(gfMul(a8, b8, 0x11B).decrypt(key), mapped2(va, vb, [](uint64_t p, uint64_t q) { return gfMulClear(8, p, q, 0x11B); }),
                "gfMul == the clear product in AES's field");
    expect(clmul(a8, b8).plane(7).terms() == 8 && clmulWide(a8, b8).width() == 15 && clmulWide(a8, b8).plane(14).terms() == 1,
           "clmul: j + 1 terms in plane j; 2w - 1 planes");
    expect(sameWords(bilinearMap(a8, b8, F2Bilinear::bitwiseAnd(8)), a8 & b8), "bitwiseAnd == a & b, word for word");
    std::vector<unsigned char> dot(va.size());
    for (size_t i = 0; i < va.size(); ++i)
        dot[i] = (unsigned char)(__builtin_popcountll(va[i] & vb[i]) & 1);
    expect(dotBits(a8, b8).decrypt(key) == dot && dotBits(a8, b8).terms() == 8, "dotBits == parity(a & b), 8 terms");
    // rows in any order with repetitions, an empty row, widths that differ
    const UIntBatch a3 = UIntBatch::encrypt(key, draw(3, 40), 3, 63);
    const std::vector<uint64_t> v3 = a3.decrypt(key);
    const Rows rows = {{Pair(2, 7), Pair(0, 0), Pair(2, 7), Pair(1, 3)}, {}, {Pair(2, 0), Pair(0, 7), Pair(1, 1)}, {}, {Pair(0, 5)}};
    const F2Bilinear odd = F2Bilinear::fromPairs(rows, 3, 8);
    expect(odd.rows()[0].size() == 2 && odd.rows()[0][0] == Pair(0, 0) && odd.rows()[2][0] == Pair(0, 7),
           "fromPairs sorts by (left, right) and cancels what is named twice");
    checkForm(key, a3, v3, b8, vb, odd, 0b01010, true, " 5 rows over 3 x 8");
    // planes of several terms on either side: the table instead of the divisions
    const UIntBatch g8 = linearMap(a8, F2Matrix::grayDecode(8));          // planes of 8 .. 1 terms
    std::vector<uint64_t> vg(va.size());
    for (size_t i = 0; i < va.size(); ++i)
        vg[i] = F2Matrix::grayDecode(8).apply(va[i]);
    checkForm(key, g8, vg, b8, vb, cl, 0x11, true, " planes of 8 .. 1 terms on the left");
    checkForm(key, b8, vb, g8, vg, gf, 0, true, " on the right");
    const std::vector<uint64_t> v32a = draw(32, 3), v32b = draw(32, 3);
    const UIntBatch a32 = UIntBatch::encrypt(key, v32a, 32, 64), b32 = UIntBatch::encrypt(key, v32b, 32, 65);
    checkForm(key, a32, v32a, b32, v32b, F2Bilinear::clmulWide(32), 0, true, " clmulWide(32)");
    const std::vector<uint64_t> v64a = draw(64, 2), v64b = draw(64, 2);
    const UIntBatch a64 = UIntBatch::encrypt(key, v64a, 64, 66), b64 = UIntBatch::encrypt(key, v64b, 64, 67);
    checkValues(gfMul(a64, b64, 0x1B).decrypt(key), mapped2(v64a, v64b, [](uint64_t p, uint64_t q) { return gfMulClear(64, p, q, 0x1B); }),
                "gfMul(64, x^64 + x^4 + x^3 + x + 1)");
    // the host algebra
    for (unsigned w : {1u, 2u, 4u, 8u, 32u}) {
        const uint64_t poly = w == 1 ? 1 : w == 2 ? 7 : w == 4 ? 0x13 : w == 8 ? 0x11B : 0x8D;
        expect(reduction(w, poly) * F2Bilinear::clmulWide(w) == F2Bilinear::gfMul(w, poly), "gfMul == reduction * clmulWide, w=" + std::to_string(w));
        const F2Matrix sq = F2Matrix::gfSquare(w, poly);
        const F2Bilinear f = F2Bilinear::gfMul(w, poly);
        for (int i = 0; i < 20; ++i) {
            const uint64_t x = rnd(w), y = rnd(w), k = rnd(w);
            expect(sq.apply(x) == f.apply(x, x) && f.apply(x, y) == gfMulClear(w, x, y, poly), "gfSquare(x) == gfMul(x, x)");
            const F2Bilinear scaled = f.compose(F2Matrix::gfMul(w, k, poly), F2Matrix::identity(w));
            expect(scaled == F2Matrix::gfMul(w, k, poly) * f && scaled.apply(x, y) == gfMulClear(w, gfMulClear(w, k, x, poly), y, poly),
                   "a public factor: compose on an argument == the map after the form");
        }
        expect((f ^ f) == F2Bilinear::fromPairs(Rows(w), w, w) && (F2Bilinear::clmul(w) ^ f).apply(3 & lowMask(w), 1) == 0, "operator^ cancels");
    }
    expect(F2Bilinear::gfMul(8, 0x1B) == gf && gf.apply(0x57, 0x83) == 0xC1 && gf.apply(0x53, 0xCA) == 1, "AES's field");
    // end to end: the inverses of GF(16), x^14 = x^2 * x^4 * x^8, squarings linear
    std::vector<uint64_t> v16(16), inv(16, 0);
    for (uint64_t x = 0; x < 16; ++x) {
        v16[x] = x;
        for (uint64_t y = 1; y < 16; ++y)
            if (gfMulClear(4, x, y, 0x13) == 1)
                inv[x] = y;
    }
    const UIntBatch x1 = UIntBatch::encrypt(key, v16, 4, 68);
    const F2Matrix sq = F2Matrix::gfSquare(4, 0x13);
    const UIntBatch x2 = linearMap(x1, sq), x4 = linearMap(x2, sq), x8 = linearMap(x4, sq);
    const UIntBatch x6 = gfMul(x2, x4, 0x13), x14 = gfMul(x6, x8, 0x13);
    checkValues(x14.decrypt(key), inv, "x^14 is the inverse in GF(16)");
    std::vector<uint64_t> unit(16, 1);
    unit[0] = 0;
    checkValues(gfMul(x14, x1, 0x13).decrypt(key), unit, "x^14 * x == 1 but at 0");
    expect(sameWords(x6, byOperators(x2, x4, F2Bilinear::gfMul(4, 0x13), 0)), "x^2 * x^4 == the chain of operators");
    uint64_t most = 0;
    for (unsigned j = 0; j < 4; ++j)
        most = std::max<uint64_t>(most, x14.plane(j).terms());
    expect(most > 256 && most < 8192, "the planes of x^14 have " + std::to_string(most) + " terms");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 5; ++w) {
        const size_t count = 40;
        const std::vector<uint64_t> va = draw(w, count), vb = draw(w, count);
        const UIntBatch a0 = UIntBatch::encrypt(key, va, w, 70 + w), b0 = UIntBatch::encrypt(key, vb, w, 80 + w);
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
        const F2Bilinear f = F2Bilinear::clmulWide(w);
        expect(std::string(bilinearRoute(ar, b0, f, 1)) == "loop" && std::string(bilinearRoute(b0, ar, f, 1)) == "loop" &&
                   std::string(bilinearRoute(a0, b0, f, 1)) == "k_uint_bilinear",
               "a ragged operand on either side takes the loop" + tag);
        checkForm(key, ar, fa, b0, vb, f, 1, true, tag + " left");
        checkForm(key, b0, vb, ar, fa, f, 1, true, tag + " right");
        checkForm(key, ar, fa, ar, fa, F2Bilinear::gfMul(w, w == 1 ? 1 : w == 2 ? 7 : w == 3 ? 0xB : w == 4 ? 0x13 : 0x25), 0, true, tag + " squares");
        checkForm(key, a0, va, b0, vb, f, 1, true, " uniform w=" + std::to_string(w));
    }
    return 0;
}

int errors()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    int thrown = 0;
    thrown += throws<std::invalid_argument>([] { F2Bilinear::clmul(0); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::clmul(65); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::clmulWide(33); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::clmulWide(0); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::gfMul(0, 1); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::gfMul(8, 0x21B); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::bitwiseAnd(65); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::dotBits(0); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::fromPairs(Rows(), 8, 8); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::fromPairs(Rows(65), 8, 8); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::fromPairs(Rows(1), 0, 8); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::fromPairs(Rows(1), 8, 65); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::fromPairs(Rows(1, std::vector<Pair>(1, Pair(8, 0))), 8, 8); });
    thrown += throws<std::invalid_argument>([] { F2Bilinear::fromPairs(Rows(1, std::vector<Pair>(1, Pair(0, 3))), 8, 3); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::gfSquare(0, 1); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::gfSquare(8, 0x21B); });
    expect(thrown == 16, "the builders throw (" + std::to_string(thrown) + " of 16)");
    const F2Bilinear f8 = F2Bilinear::clmul(8), f4 = F2Bilinear::clmul(4), w4 = F2Bilinear::clmulWide(4);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { f8 ^ f4; });
    thrown += throws<std::invalid_argument>([&] { f4 ^ w4; });
    thrown += throws<std::invalid_argument>([&] { F2Matrix::identity(8) * f4; });
    thrown += throws<std::invalid_argument>([&] { f4.compose(F2Matrix::identity(8), F2Matrix::identity(4)); });
    thrown += throws<std::invalid_argument>([&] { f4.compose(F2Matrix::identity(4), F2Matrix::identity(8)); });
    expect(thrown == 5, "mismatched shapes throw (" + std::to_string(thrown) + " of 5)");
    expect((F2Matrix::identity(7) * w4) == w4 && f4.compose(F2Matrix::identity(4), F2Matrix::identity(4)) == f4 &&
               f4.compose(F2Matrix::fromRows({1, 2, 4, 8}, 6), F2Matrix::identity(4)).leftWidth() == 6,
           "the identity maps change nothing; compose takes the maps' input widths");
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3), b4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 5), 4, 4);
    const UIntBatch a8 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 8, 5), b4s = b4.slice(0, 9);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o4 = UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 3), 4, 6);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { bilinearMap(a8, b4, f4); });            // the widths
    thrown += throws<std::invalid_argument>([&] { bilinearMap(a4, a8, f4); });
    thrown += throws<std::invalid_argument>([&] { bilinearMap(a4, b4s, f4); });           // the counts
    thrown += throws<std::invalid_argument>([&] { bilinearMap(a4, o4, f4); });            // the contexts
    thrown += throws<std::invalid_argument>([&] { bilinearMap(a4, b4, f4, 16); });        // the constant
    thrown += throws<std::invalid_argument>([&] { bilinearRoute(a4, b4, f8); });
    thrown += throws<std::invalid_argument>([&] { clmul(a4, a8); });
    thrown += throws<std::invalid_argument>([&] { clmulWide(a8, b4); });
    thrown += throws<std::invalid_argument>([&] { gfMul(a4, a8, 0x13); });
    thrown += throws<std::invalid_argument>([&] { gfMul(a4, b4, 0x33); });
    thrown += throws<std::invalid_argument>([&] { dotBits(a4, a8); });
    expect(thrown == 11, "bilinearMap and its kin throw (" + std::to_string(thrown) + " of 11)");
    expect(bilinearMap(a4, b4, w4, 0x7F).width() == 7, "a constant of the output width fits");
    // oversize: ONE element whose planes share a payload of 2^14 terms; a product of two of them has 2^28 terms of 20
    // words, past 2^31 words per element.  The size check comes before any allocation or launch.
    CiphertextBatch big = a4.plane(0).slice(0, 1);
    for (int i = 0; i < 14; ++i)
        big = big + big;
    expect(big.terms() == (1u << 14), "the operand has 2^14 terms");
    const UIntBatch wide = UIntBatch::fromPlanes(std::vector<CiphertextBatch>(4, big));
    const auto t0 = std::chrono::steady_clock::now();
    thrown = throws<std::invalid_argument>([&] { bilinearMap(wide, wide, f4); });
    thrown += throws<std::invalid_argument>([&] { dotBits(wide, wide); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 2, "oversize throws (" + std::to_string(thrown) + " of 2)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // an empty batch: empty planes of the output width
    const UIntBatch e = bilinearMap(a4.slice(0, 0), b4.slice(0, 0), w4, 5);
    expect(e.width() == 7 && e.size() == 0 && std::string(bilinearRoute(a4.slice(0, 0), b4.slice(0, 0), w4)) == "none",
           "an empty batch gives empty planes and launches nothing");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 3832, "uint_bilinear_driver", {{"words", words}, {"ragged", ragged}, {"errors", errors}});
}
