// uint_poly_driver.cpp -- user-style C++ over F2Polynomial, polyMap, ch, maj, chi, andAll and polyRoute of
// include/certfhe/UInt.h (tests/test_uint_poly_cpp.py builds and runs it).
//   uint_poly_driver words    at N=1247: the class results word for word against the chain of operator* and operator+
//                             written out; ch, maj, chi, andAll and mux against the boolean operators' values; constants,
//                             empty rows, single-bit rows (the source's payload), planes of several terms, operands that
//                             are the same integer; linear and bilinear forms against linearMap and bilinearMap word for
//                             word; the host algebra; a 4-bit S-box from its table
//   uint_poly_driver ragged   a compact()ed (ragged) operand takes the loop: the same words as the chain of operators,
//                             the same decryptions
//   uint_poly_driver errors   every std::invalid_argument of F2Polynomial, polyMap and its kin; oversize before any
//                             launch; an empty batch
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

typedef F2Polynomial::Monomial Mono;
typedef F2Polynomial::Rows Rows;

std::vector<uint64_t> draw(unsigned w, size_t count)
{
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = rnd(w);
    return v;
}

uint64_t lowMask(unsigned w) { return w >= 64 ? ~0ull : (1ull << w) - 1; }

CiphertextBatch constantOf(const UIntBatch &a, bool bit)
{
    return constantBatch(a.context(), std::vector<unsigned char>(a.size(), bit ? 1 : 0));
}

std::vector<CiphertextBatch> planesOf(const std::vector<UIntBatch> &ops)
{
    std::vector<CiphertextBatch> planes;
    for (size_t o = 0; o < ops.size(); ++o)
        for (unsigned i = 0; i < ops[o].width(); ++i)
            planes.push_back(ops[o].plane(i));
    return planes;
}

// the definition through the chain of CiphertextBatch operators, monomial by monomial in the row's order
UIntBatch byOperators(const std::vector<UIntBatch> &ops, const F2Polynomial &f, uint64_t constant)
{
    const std::vector<CiphertextBatch> in = planesOf(ops);
    constant ^= f.constant();
    std::vector<CiphertextBatch> planes;
    for (unsigned x = 0; x < f.outWidth(); ++x) {
        const std::vector<Mono> &row = f.rows()[x];
        const bool bit = (constant >> x) & 1u;
        if (row.empty()) {
            planes.push_back(constantOf(ops[0], bit));
            continue;
        }
        std::vector<CiphertextBatch> sum;
        for (size_t i = 0; i < row.size(); ++i) {
            CiphertextBatch p = in[row[i][0]];
            for (size_t k = 1; k < row[i].size(); ++k)
                p = p * in[row[i][k]];
            if (sum.empty())
                sum.push_back(p);
            else
                sum[0] = sum[0] + p;
        }
        planes.push_back(bit ? logicNot(sum[0]) : sum[0]);
    }
    return UIntBatch::fromPlanes(planes);
}

std::vector<uint64_t> clearOf(const F2Polynomial &f, const std::vector<std::vector<uint64_t> > &values, uint64_t constant)
{
    std::vector<uint64_t> v(values[0].size());
    for (size_t i = 0; i < v.size(); ++i) {
        std::vector<uint64_t> at;
        for (size_t o = 0; o < values.size(); ++o)
            at.push_back(values[o][i]);
        v[i] = f.apply(at) ^ constant;
    }
    return v;
}

// polyMap against the written-out chain word for word, and the clear form
void checkForm(const SecretKey &key, const std::vector<UIntBatch> &ops, const std::vector<std::vector<uint64_t> > &values,
               const F2Polynomial &f, uint64_t constant, const std::string &tag)
{
    const UIntBatch y = polyMap(ops, f, constant);
    expect(y.width() == f.outWidth() && y.size() == ops[0].size(), "the result has the form's output width" + tag);
    expect(sameWords(y, byOperators(ops, f, constant)), "polyMap == the chain of operators" + tag);
    checkValues(y.decrypt(key), clearOf(f, values, constant), "polyMap decrypted" + tag);
}

template <typename F>
std::vector<uint64_t> mapped3(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b, const std::vector<uint64_t> &c, F f)
{
    std::vector<uint64_t> v(a.size());
    for (size_t i = 0; i < a.size(); ++i)
        v[i] = f(a[i], b[i], c[i]);
    return v;
}

Mono mono(std::initializer_list<unsigned> v) { return Mono(v); }

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const std::vector<uint64_t> va = draw(8, 40), vb = draw(8, 40), vc = draw(8, 40);
    const UIntBatch a = UIntBatch::encrypt(key, va, 8, 71), b = UIntBatch::encrypt(key, vb, 8, 72), c = UIntBatch::encrypt(key, vc, 8, 73);
    const std::vector<UIntBatch> abc = {a, b, c};
    const std::vector<std::vector<uint64_t> > vabc = {va, vb, vc};
    const F2Polynomial fch = F2Polynomial::ch(8), fmaj = F2Polynomial::maj(8), fchi = F2Polynomial::chi(8);
    expect(std::string(polyRoute(abc, fch)) == "k_uint_poly", "uniform planes take the launch");
    checkForm(key, abc, vabc, fch, 0, " ch");
    checkForm(key, abc, vabc, fch, 0xA5, " ch ^ constant");
    checkForm(key, abc, vabc, fmaj, 0x81, " maj");
    checkForm(key, abc, vabc, fchi, 0, " chi");
    checkForm(key, abc, vabc, F2Polynomial::andAll(8, 3), 0x10, " andAll");
    checkValues(ch(a, b, c).decrypt(key), mapped3(va, vb, vc, [](uint64_t e, uint64_t f, uint64_t g) { return (e & f) ^ (~e & g & 0xFF); }), "ch == (e & f) ^ (~e & g)");
    checkValues(maj(a, b, c).decrypt(key), mapped3(va, vb, vc, [](uint64_t x, uint64_t y, uint64_t z) { return (x & y) | (x & z) | (y & z); }), "maj == the majority");
    checkValues(chi(a, b, c).decrypt(key), mapped3(va, vb, vc, [](uint64_t x, uint64_t y, uint64_t z) { return x ^ (~y & z & 0xFF); }), "chi == a ^ (~b & c)");
    checkValues(andAll(abc).decrypt(key), mapped3(va, vb, vc, [](uint64_t x, uint64_t y, uint64_t z) { return x & y & z; }), "andAll == a & b & c");
    checkValues(ch(a, b, c).decrypt(key), ((a & b) ^ (~a & c)).decrypt(key), "ch == the chain of bitwise operators, decrypted");
    expect(ch(a, b, c).plane(3).terms() == 3 && maj(a, b, c).plane(0).terms() == 3 && chi(a, b, c).plane(7).terms() == 3 &&
               andAll(abc).plane(5).terms() == 1,
           "ch, maj and chi have 3 terms a plane over fresh planes, andAll 1");
    checkForm(key, {a, a, a}, {va, va, va}, fmaj, 0, " maj(a, a, a): every operand the same integer");
    // mux: a one-bit selector
    const std::vector<uint64_t> vs = draw(1, 40);
    const UIntBatch s = UIntBatch::encrypt(key, vs, 1, 74);
    checkForm(key, {s, a, b}, {vs, va, vb}, F2Polynomial::mux(8), 0, " mux");
    checkValues(polyMap({s, a, b}, F2Polynomial::mux(8)).decrypt(key),
                mapped3(vs, va, vb, [](uint64_t q, uint64_t x, uint64_t y) { return q ? x : y; }), "mux == s ? x : y");
    // rows in any order with repetitions, a repeated variable, an empty monomial, an empty row, single-bit rows
    const Rows rows = {{mono({9, 0}), mono({3}), mono({0, 9}), mono({17, 2, 9, 2})}, {}, {mono({5})}, {mono({}), mono({23, 1})}, {mono({4}), mono({})},
                       {mono({0, 1, 2, 3, 8, 9, 10, 11})}};
    const F2Polynomial odd = F2Polynomial::fromMonomials(rows, {8, 8, 8});
    expect(odd.rows()[0].size() == 2 && odd.rows()[0][0] == mono({3}) && odd.rows()[0][1] == mono({2, 9, 17}) && odd.constant() == 0b011000,
           "fromMonomials sorts by (degree, variables), names a variable once, cancels what is named twice, folds the constant");
    checkForm(key, abc, vabc, odd, 0b000010, " 6 rows over 3 x 8");
    const UIntBatch y = polyMap(abc, odd, 0b000010);
    expect(y.plane(2).deviceValues() == a.plane(5).deviceValues(), "a row of one bit and no constant shares the source's payload");
    expect(y.plane(4).deviceValues() != a.plane(4).deviceValues() && y.plane(4).terms() == 2, "with the constant it is computed");
    expect(y.plane(1).terms() == 1 && y.plane(5).terms() == 1, "an empty row is the constant; degree 8 over fresh planes is one term");
    const F2Polynomial only = F2Polynomial::fromMonomials({{mono({5})}, {}}, {8, 8, 8});
    expect(std::string(polyRoute(abc, only, 0b10)) == "none" && polyMap(abc, only, 0b10).plane(0).deviceValues() == a.plane(5).deviceValues(),
           "nothing left to compute: nothing is launched");
    // planes of several terms: the planes' divisors
    const UIntBatch g8 = linearMap(a, F2Matrix::grayDecode(8));            // planes of 8 .. 1 terms
    std::vector<uint64_t> vg(va.size());
    for (size_t i = 0; i < va.size(); ++i)
        vg[i] = F2Matrix::grayDecode(8).apply(va[i]);
    checkForm(key, {g8, b, c}, {vg, vb, vc}, fch, 0x11, " ch with planes of 8 .. 1 terms");
    checkForm(key, {b, g8, g8}, {vb, vg, vg}, fmaj, 0, " maj with two such operands");
    // linear and bilinear forms: the shipped words
    const F2Matrix sigma = F2Matrix::rotateRight(8, 1) ^ F2Matrix::rotateRight(8, 3) ^ F2Matrix::shiftRight(8, 2);
    expect(sameWords(polyMap({a}, F2Polynomial::linear(sigma), 0x21), linearMap(a, sigma, 0x21)), "linear(m) has linearMap's words");
    const F2Bilinear gf = F2Bilinear::gfMul(8, 0x11B);
    expect(sameWords(polyMap({a, b}, F2Polynomial::bilinear(gf), 0x3), bilinearMap(a, b, gf, 0x3)), "bilinear(f) has bilinearMap's words");
    expect(sameWords(polyMap({g8, b}, F2Polynomial::bilinear(F2Bilinear::clmul(8))), bilinearMap(g8, b, F2Bilinear::clmul(8))),
           "and over planes of several terms");
    // wide operands: 96 and 192 planes
    const std::vector<uint64_t> v32a = draw(32, 3), v32b = draw(32, 3), v32c = draw(32, 3);
    const std::vector<UIntBatch> o32 = {UIntBatch::encrypt(key, v32a, 32, 75), UIntBatch::encrypt(key, v32b, 32, 76), UIntBatch::encrypt(key, v32c, 32, 77)};
    checkForm(key, o32, {v32a, v32b, v32c}, F2Polynomial::ch(32), 0, " ch(32)");
    checkForm(key, o32, {v32a, v32b, v32c}, F2Polynomial::maj(32), 0x80000001u, " maj(32)");
    const std::vector<uint64_t> v64a = draw(64, 2), v64b = draw(64, 2), v64c = draw(64, 2);
    const std::vector<UIntBatch> o64 = {UIntBatch::encrypt(key, v64a, 64, 78), UIntBatch::encrypt(key, v64b, 64, 79), UIntBatch::encrypt(key, v64c, 64, 80)};
    checkForm(key, o64, {v64a, v64b, v64c}, F2Polynomial::chi(64), 1ull << 63, " chi(64)");
    // the host algebra
    for (unsigned w : {1u, 2u, 4u, 8u, 32u}) {
        const F2Polynomial fc = F2Polynomial::ch(w), fm = F2Polynomial::maj(w);
        expect(F2Polynomial::fromMonomials(F2Polynomial::andAll(w, 2).rows(), {w, w}) == F2Polynomial::andAll(w, 2),
               "fromMonomials of a canonical form's rows is the form");
        for (int i = 0; i < 20; ++i) {
            const uint64_t x = rnd(w), y = rnd(w), z = rnd(w);
            expect(fc.apply({x, y, z}) == ((x & y) ^ (~x & z & lowMask(w))) && fm.apply({x, y, z}) == ((x & y) | (x & z) | (y & z)) &&
                       F2Polynomial::chi(w).apply({x, y, z}) == (x ^ (~y & z & lowMask(w))),
                   "ch, maj and chi apply as their definitions");
            expect((fc ^ fm).apply({x, y, z}) == (fc.apply({x, y, z}) ^ fm.apply({x, y, z})) && (fc & fm).apply({x, y, z}) == (fc.apply({x, y, z}) & fm.apply({x, y, z})),
                   "operator^ and operator& are pointwise");
            const F2Matrix rot = F2Matrix::rotateLeft(w, 1), id = F2Matrix::identity(w);
            expect(fc.compose({rot, id, id}).apply({x, y, z}) == fc.apply({rot.apply(x), y, z}), "compose applies a map to an operand");
            expect((rot * fm).apply({x, y, z}) == rot.apply(fm.apply({x, y, z})), "a map after the form");
        }
        expect((fc ^ fc) == F2Polynomial::fromMonomials(Rows(w), {w, w, w}) && (fm & fm) == fm, "f ^ f is empty; f & f is f");
        expect(fc.compose({F2Matrix::identity(w), F2Matrix::identity(w), F2Matrix::identity(w)}) == fc, "the identity maps change nothing");
    }
    // a & b & ~c = ab + abc by the pointwise product with a complemented form: the constant multiplies too
    const F2Polynomial ab = F2Polynomial::fromMonomials(F2Polynomial::andAll(4, 2).rows(), {4, 4, 4});
    Rows crows(4);
    for (unsigned j = 0; j < 4; ++j)
        crows[j] = {mono({8 + j}), mono({})};
    const F2Polynomial andnot = ab & F2Polynomial::fromMonomials(crows, {4, 4, 4});
    expect(andnot.constant() == 0 && andnot.rows()[1].size() == 2 && andnot.rows()[1][1] == mono({1, 5, 9}), "a & b & ~c is ab + abc");
    for (uint64_t x = 0; x < 4096; x += 5)
        expect(andnot.apply({x & 15, (x >> 4) & 15, x >> 8}) == ((x & 15) & ((x >> 4) & 15) & ~(x >> 8) & 15), "a & b & ~c applies");
    // a 4-bit S-box (PRESENT) from its table: the ANF equals the table on all inputs, and polyMap equals lookup
    const std::vector<uint64_t> present = {0xC, 5, 6, 0xB, 9, 0, 0xA, 0xD, 3, 0xE, 0xF, 8, 4, 7, 1, 2};
    const LookupTable box(present, 4, 4);
    const F2Polynomial fbox = F2Polynomial::fromLookupTable(box);
    for (uint64_t x = 0; x < 16; ++x)
        expect(fbox.apply({x}) == present[x], "the S-box form equals the table");
    std::vector<uint64_t> v16(16);
    for (uint64_t x = 0; x < 16; ++x)
        v16[x] = x;
    const UIntBatch x4 = UIntBatch::encrypt(key, v16, 4, 81);
    checkForm(key, {x4}, {v16}, fbox, 0, " the PRESENT S-box");
    checkValues(polyMap({x4}, fbox).decrypt(key), lookup(x4, box).decrypt(key), "polyMap(fromLookupTable) == lookup, decrypted");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 4; ++w) {
        const size_t count = 40;
        const std::vector<uint64_t> va = draw(w, count), vb = draw(w, count), vc = draw(w, count);
        const UIntBatch a0 = UIntBatch::encrypt(key, va, w, 90 + w), b0 = UIntBatch::encrypt(key, vb, w, 100 + w),
                        c0 = UIntBatch::encrypt(key, vc, w, 110 + w);
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
        const F2Polynomial fch = F2Polynomial::ch(w), fmaj = F2Polynomial::maj(w);
        expect(std::string(polyRoute({ar, b0, c0}, fch, 1)) == "loop" && std::string(polyRoute({b0, c0, ar}, fch, 1)) == "loop" &&
                   std::string(polyRoute({a0, b0, c0}, fch, 1)) == "k_uint_poly",
               "a ragged operand anywhere takes the loop" + tag);
        checkForm(key, {ar, b0, c0}, {fa, vb, vc}, fch, 1, tag + " ch, first");
        checkForm(key, {b0, c0, ar}, {vb, vc, fa}, fch, 0, tag + " ch, last");
        checkForm(key, {ar, ar, b0}, {fa, fa, vb}, fmaj, 1, tag + " maj, twice");
        checkForm(key, {ar, b0, c0}, {fa, vb, vc}, F2Polynomial::chi(w), 0, tag + " chi");
        checkForm(key, {ar, b0, c0}, {fa, vb, vc}, F2Polynomial::andAll(w, 3), 1, tag + " andAll");
        Rows rows(2);
        rows[0] = {mono({0}), mono({w, 0, 2 * w}), mono({2 * w}), mono({0, w})};
        rows[1] = {mono({3 * w - 1})};
        const F2Polynomial mixed = F2Polynomial::fromMonomials(rows, {w, w, w});
        checkForm(key, {ar, b0, c0}, {fa, vb, vc}, mixed, 0b01, tag + " degrees 1, 2 and 3 in one row");
        expect(polyMap({ar, b0, c0}, mixed, 0b01).plane(1).deviceValues() == c0.plane(w - 1).deviceValues(),
               "a single-bit row shares the payload on the loop too" + tag);
        checkForm(key, {a0, b0, c0}, {va, vb, vc}, mixed, 0b11, " uniform w=" + std::to_string(w));
    }
    return 0;
}

int errors()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    int thrown = 0;
    thrown += throws<std::invalid_argument>([] { F2Polynomial::ch(0); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::ch(65); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::maj(0); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::chi(65); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::andAll(8, 0); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::andAll(8, 9); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::andAll(64, 5); });            // 320 bits of operands
    thrown += throws<std::invalid_argument>([] { F2Polynomial::mux(0); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials(Rows(), {8}); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials(Rows(65), {8}); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials(Rows(1), {}); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials(Rows(1), {0}); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials(Rows(1), {65}); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials(Rows(1), {64, 64, 64, 64, 1}); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials({{mono({16})}}, {8, 8}); });
    thrown += throws<std::invalid_argument>([] { F2Polynomial::fromMonomials({{mono({0, 1, 2, 3, 4, 5, 6, 7, 8})}}, {16}); });
    expect(thrown == 16, "the builders throw (" + std::to_string(thrown) + " of 16)");
    expect(F2Polynomial::fromMonomials({{mono({0, 1, 2, 3, 4, 5, 6, 7, 7, 0})}}, {16}).rows()[0][0].size() == 8,
           "a repeated variable does not count towards the degree");
    const F2Polynomial c8 = F2Polynomial::ch(8), c4 = F2Polynomial::ch(4), a4 = F2Polynomial::andAll(4, 2);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { c8 ^ c4; });
    thrown += throws<std::invalid_argument>([&] { c4 ^ a4; });
    thrown += throws<std::invalid_argument>([&] { c4 & a4; });
    thrown += throws<std::invalid_argument>([&] { F2Matrix::identity(8) * c4; });
    thrown += throws<std::invalid_argument>([&] { c4.compose({F2Matrix::identity(4), F2Matrix::identity(4)}); });
    thrown += throws<std::invalid_argument>([&] { c4.compose({F2Matrix::identity(8), F2Matrix::identity(4), F2Matrix::identity(4)}); });
    thrown += throws<std::invalid_argument>([&] { c4.apply({1, 2}); });
    // degree 9 by the pointwise product: nine distinct variables
    thrown += throws<std::invalid_argument>([] {
        const F2Polynomial x = F2Polynomial::fromMonomials({{mono({0, 1, 2, 3, 4})}}, {16}), y = F2Polynomial::fromMonomials({{mono({5, 6, 7, 8})}}, {16});
        x & y;
    });
    // compose past 262144 monomials: a degree-4 monomial whose every variable becomes a sum of 64
    thrown += throws<std::invalid_argument>([] {
        const F2Matrix all = F2Matrix::fromRows(std::vector<uint64_t>(4, ~0ull), 64);
        F2Polynomial::andAll(4, 4).compose({all, all, all, all});
    });
    expect(thrown == 9, "mismatched shapes, degree 9 and too many monomials throw (" + std::to_string(thrown) + " of 9)");
    const UIntBatch e4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3), f4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 5), 4, 4),
                    g4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 9), 4, 5);
    const UIntBatch e8 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 8, 6), g4s = g4.slice(0, 9);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o4 = UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 3), 4, 7);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { polyMap({e8, f4, g4}, c4); });             // the widths
    thrown += throws<std::invalid_argument>([&] { polyMap({e4, f4}, c4); });                 // the number of operands
    thrown += throws<std::invalid_argument>([&] { polyMap({}, c4); });
    thrown += throws<std::invalid_argument>([&] { polyMap({e4, f4, g4s}, c4); });            // the counts
    thrown += throws<std::invalid_argument>([&] { polyMap({e4, f4, o4}, c4); });             // the contexts
    thrown += throws<std::invalid_argument>([&] { polyMap({e4, f4, g4}, c4, 16); });         // the constant
    thrown += throws<std::invalid_argument>([&] { polyRoute({e4, f4, g4}, c8); });
    thrown += throws<std::invalid_argument>([&] { ch(e4, e8, g4); });
    thrown += throws<std::invalid_argument>([&] { maj(e8, f4, g4); });
    thrown += throws<std::invalid_argument>([&] { chi(e4, f4, e8); });
    thrown += throws<std::invalid_argument>([&] { andAll({e4, e8}); });
    thrown += throws<std::invalid_argument>([&] { andAll({}); });
    thrown += throws<std::invalid_argument>([&] { andAll(std::vector<UIntBatch>(9, e4)); });
    expect(thrown == 13, "polyMap and its kin throw (" + std::to_string(thrown) + " of 13)");
    expect(polyMap({e4, f4, g4}, c4, 0xF).width() == 4, "a constant of the output width fits");
    // oversize: ONE element whose planes share a payload of 2^14 terms; a product of two of them has 2^28 terms of 20
    // words, past 2^31 words per element.  The size check comes before any allocation or launch.
    CiphertextBatch big = e4.plane(0).slice(0, 1);
    for (int i = 0; i < 14; ++i)
        big = big + big;
    expect(big.terms() == (1u << 14), "the operand has 2^14 terms");
    const UIntBatch wide = UIntBatch::fromPlanes(std::vector<CiphertextBatch>(4, big));
    const auto t0 = std::chrono::steady_clock::now();
    thrown = throws<std::invalid_argument>([&] { polyMap({wide, wide, wide}, c4); });
    thrown += throws<std::invalid_argument>([&] { maj(wide, wide, wide); });
    thrown += throws<std::invalid_argument>([&] { andAll({wide, wide}); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 3, "oversize throws (" + std::to_string(thrown) + " of 3)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // an empty batch: empty planes of the output width
    const UIntBatch e = polyMap({e4.slice(0, 0), f4.slice(0, 0), g4.slice(0, 0)}, c4, 5);
    expect(e.width() == 4 && e.size() == 0 && std::string(polyRoute({e4.slice(0, 0), f4.slice(0, 0), g4.slice(0, 0)}, c4)) == "none",
           "an empty batch gives empty planes and launches nothing");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 3939, "uint_poly_driver", {{"words", words}, {"ragged", ragged}, {"errors", errors}});
}
