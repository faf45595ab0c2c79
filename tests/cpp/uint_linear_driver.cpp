// uint_linear_driver.cpp -- user-style C++ over F2Matrix, linearMap, parity and linearRoute of include/certfhe/UInt.h
// (tests/test_uint_linear_cpp.py builds and runs it).
//   uint_linear_driver words    at N=1247: SHA-256's sigma 0 against the chain of public rotates and a ^ b; Gray encode
//                               and decode, apart and as ONE composed matrix (the source payloads); xtime for all 256
//                               values; MixColumns on a 32-bit column; clmul; parity against popcountBit(a, 0); rows
//                               of one bit share the source plane's payload; constants
//   uint_linear_driver ragged   a compact()ed (ragged) operand takes the loop: the same words and decryptions
//   uint_linear_driver errors   every std::invalid_argument of F2Matrix, linearMap and parity; oversize before any
//                               launch; an empty batch
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

std::vector<uint64_t> draw(unsigned w, size_t count)
{
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = rnd(w);
    return v;
}

template <typename F>
std::vector<uint64_t> mapped(const std::vector<uint64_t> &a, F f)
{
    std::vector<uint64_t> v(a.size());
    for (size_t i = 0; i < a.size(); ++i)
        v[i] = f(a[i]);
    return v;
}

uint32_t rotr(uint32_t x, unsigned s) { return (x >> s) | (x << (32 - s)); }

uint8_t xtime(uint8_t x) { return (uint8_t)((x << 1) ^ ((x & 0x80) ? 0x1B : 0)); }

// AES MixColumns on one column, byte c at bits 8c .. 8c + 7
uint32_t mixColumn(uint32_t x)
{
    uint8_t a[4], o[4];
    for (int c = 0; c < 4; ++c)
        a[c] = (uint8_t)(x >> (8 * c));
    for (int c = 0; c < 4; ++c)
        o[c] = (uint8_t)(xtime(a[c]) ^ (xtime(a[(c + 1) % 4]) ^ a[(c + 1) % 4]) ^ a[(c + 2) % 4] ^ a[(c + 3) % 4]);
    return (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
}

F2Matrix mixColumns()
{
    const F2Matrix two = F2Matrix::gfMul(8, 2, 0x11B), three = F2Matrix::gfMul(8, 3, 0x11B);
    std::vector<uint64_t> rows(32, 0);
    for (unsigned r = 0; r < 4; ++r)                      // out byte r = 2 a_r ^ 3 a_{r+1} ^ a_{r+2} ^ a_{r+3}
        for (unsigned j = 0; j < 8; ++j)
            rows[8 * r + j] = (two.rows()[j] << (8 * r)) | (three.rows()[j] << (8 * ((r + 1) % 4))) |
                              (1ull << (8 * ((r + 2) % 4) + j)) | (1ull << (8 * ((r + 3) % 4) + j));
    return F2Matrix::fromRows(rows, 32);
}

uint64_t clmulClear(uint64_t a, uint64_t k, unsigned w)
{
    uint64_t r = 0;
    for (unsigned i = 0; i < w; ++i)
        if ((k >> i) & 1u)
            r ^= a << i;
    return w == 64 ? r : r & ((1ull << w) - 1);
}

// the definition through the CiphertextBatch operators: what the loop route issues
UIntBatch byOperators(const UIntBatch &a, const F2Matrix &m, uint64_t constant)
{
    const std::vector<unsigned char> zero(a.size(), 0), one(a.size(), 1);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < m.outWidth(); ++j) {
        const uint64_t row = m.rows()[j];
        const bool bit = (constant >> j) & 1u;
        if (row == 0) {
            planes.push_back(constantBatch(a.context(), bit ? one : zero));
            continue;
        }
        unsigned i = (unsigned)__builtin_ctzll(row);
        CiphertextBatch sum = a.plane(i);
        for (++i; i < a.width(); ++i)
            if ((row >> i) & 1u)
                sum = sum + a.plane(i);
        planes.push_back(bit ? logicNot(sum) : sum);
    }
    return UIntBatch::fromPlanes(planes);
}

// linearMap against the operators word for word, against the clear map, and the shared payloads
void checkMap(const SecretKey &key, const UIntBatch &a, const std::vector<uint64_t> &va, const F2Matrix &m, uint64_t constant,
              const std::string &tag)
{
    const UIntBatch y = linearMap(a, m, constant);
    expect(y.width() == m.outWidth() && y.size() == a.size(), "the result has the map's output width" + tag);
    expect(sameWords(y, byOperators(a, m, constant)), "linearMap == the CiphertextBatch operators" + tag);
    checkValues(y.decrypt(key), mapped(va, [&](uint64_t x) { return m.apply(x) ^ constant; }), "linearMap decrypted" + tag);
    for (unsigned j = 0; j < m.outWidth(); ++j) {
        const uint64_t row = m.rows()[j];
        if (row && !(row & (row - 1)) && !((constant >> j) & 1u))
            expect(y.plane(j).deviceValues() == a.plane((unsigned)__builtin_ctzll(row)).deviceValues(),
                   "a row of one bit shares the source plane's payload" + tag);
    }
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    // sigma 0 of SHA-256
    const std::vector<uint64_t> v32 = draw(32, 9);
    const UIntBatch a32 = UIntBatch::encrypt(key, v32, 32, 41);
    const F2Matrix s0 = F2Matrix::rotateRight(32, 7) ^ F2Matrix::rotateRight(32, 18) ^ F2Matrix::shiftRight(32, 3);
    expect(std::string(linearRoute(a32, s0)) == "call", "uniform planes take the call");
    const UIntBatch sig = linearMap(a32, s0);
    const std::vector<uint64_t> chain = (a32.rotateRight(7) ^ a32.rotateRight(18) ^ a32.shiftRight(3)).decrypt(key);
    checkValues(sig.decrypt(key), chain, "sigma0 == the chain, decrypted");
    checkValues(chain, mapped(v32, [](uint64_t x) { return (uint64_t)(rotr((uint32_t)x, 7) ^ rotr((uint32_t)x, 18) ^ ((uint32_t)x >> 3)); }),
                "the chain == the clear function");
    expect(sig.plane(0).terms() == 3 && sig.plane(31).terms() == 2 && sig.plane(29).terms() == 2, "sigma0: 3 terms a plane, 2 in the top three");
    checkMap(key, a32, v32, s0, 0, " sigma0");
    checkMap(key, a32, v32, s0, 0x80000001u, " sigma0 ^ constant");
    // MixColumns on a column
    const F2Matrix mc = mixColumns();
    checkMap(key, a32, v32, mc, 0, " MixColumns");
    checkValues(linearMap(a32, mc).decrypt(key), mapped(v32, [](uint64_t x) { return (uint64_t)mixColumn((uint32_t)x); }),
                "MixColumns == the clear function");
    expect(mc.apply(0x455313DBu) == 0xBCA14D8Eu, "MixColumns: the specification's column");
    // Gray codes: apart, and as one matrix
    const F2Matrix ge = F2Matrix::grayEncode(32), gd = F2Matrix::grayDecode(32);
    checkMap(key, a32, v32, ge, 0, " grayEncode");
    checkMap(key, a32, v32, gd, 0, " grayDecode");
    const UIntBatch back = linearMap(linearMap(a32, ge), gd);
    checkValues(back.decrypt(key), v32, "Gray encode then decode is the identity");
    expect(back.plane(0).terms() == 63 && back.plane(31).terms() == 1, "two calls keep the duplicates: 63 terms in plane 0");
    expect(gd * ge == F2Matrix::identity(32) && ge * gd == F2Matrix::identity(32), "composed over F2 the duplicates cancel");
    const UIntBatch same = linearMap(a32, gd * ge);
    expect(std::string(linearRoute(a32, gd * ge)) == "loop", "the identity launches nothing");
    for (unsigned j = 0; j < 32; ++j)
        expect(same.plane(j).deviceValues() == a32.plane(j).deviceValues(), "the composed identity returns the source payloads");
    // xtime for all 256 values
    std::vector<uint64_t> v8(256);
    for (size_t i = 0; i < 256; ++i)
        v8[i] = i;
    const UIntBatch a8 = UIntBatch::encrypt(key, v8, 8, 43);
    const F2Matrix x2 = F2Matrix::gfMul(8, 2, 0x11B);
    checkMap(key, a8, v8, x2, 0, " gfMul(8, 2)");
    checkValues(linearMap(a8, x2).decrypt(key), mapped(v8, [](uint64_t x) { return (uint64_t)xtime((uint8_t)x); }), "gfMul(8, 2, 0x11B) == xtime");
    expect(F2Matrix::gfMul(8, 2, 0x1B) == x2 && x2 * x2 == F2Matrix::gfMul(8, 4, 0x11B), "gfMul: X^w implied; 2 * 2 == 4");
    expect((F2Matrix::gfMul(8, 0x53, 0x11B) * F2Matrix::gfMul(8, 0xCA, 0x11B)) == F2Matrix::identity(8), "0x53 * 0xCA == 1 in AES's field");
    // clmul, masks, shifts as matrices, widths that differ
    const uint64_t k8 = 0x9D;
    checkMap(key, a8, v8, F2Matrix::clmul(8, k8), 0x0F, " clmul");
    checkValues(linearMap(a8, F2Matrix::clmul(8, k8)).decrypt(key), mapped(v8, [&](uint64_t x) { return clmulClear(x, k8, 8); }), "clmul == the clear product");
    checkMap(key, a8, v8, F2Matrix::mask(8, 0xA5), 0xF0, " mask");
    checkMap(key, a8, v8, F2Matrix::shiftLeft(8, 3) ^ F2Matrix::rotateLeft(8, 1), 0, " shiftLeft ^ rotateLeft");
    checkMap(key, a8, v8, F2Matrix::fromRows({0xFF, 0, 0x81, 0x81, 0x10}, 8), 0x0A, " 5 rows of 8");
    const std::vector<uint64_t> v64 = draw(64, 3);
    const UIntBatch a64 = UIntBatch::encrypt(key, v64, 64, 45);
    std::vector<uint64_t> dense(64);
    for (unsigned j = 0; j < 64; ++j)
        dense[j] = rnd(64);
    checkMap(key, a64, v64, F2Matrix::fromRows(dense, 64), rnd(64), " 64 x 64");
    // planes of several terms: the map of a map
    checkMap(key, linearMap(a8, F2Matrix::grayDecode(8)), mapped(v8, [](uint64_t x) { return F2Matrix::grayDecode(8).apply(x); }),
             F2Matrix::clmul(8, 7), 1, " planes of 8 .. 1 terms");
    // parity
    const UIntBatch cnt = a8;
    const CiphertextBatch par = parity(a8, 0xFF);
    expect(par.terms() == 8, "parity of 8 fresh planes has 8 terms");
    std::vector<unsigned char> pb = par.decrypt(key), want(256), low(256);
    const std::vector<unsigned char> pc = popcountBit(cnt, 0).decrypt(key);
    for (size_t i = 0; i < 256; ++i) {
        want[i] = (unsigned char)(__builtin_popcountll(i) & 1);
        low[i] = (unsigned char)(__builtin_popcountll(i & 0x16) & 1);
    }
    expect(pb == want && pc == want, "parity == popcountBit(a, 0) == the clear parity");
    expect(parity(a8, 0x16).decrypt(key) == low, "a masked parity");
    expect(parity(a8, 0x10).deviceValues() == a8.plane(4).deviceValues(), "the parity of one bit is that plane");
    expect(parity(a8, 0).decrypt(key) == std::vector<unsigned char>(256, 0), "the parity of nothing is ZERO");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 6; ++w) {
        const size_t count = 40;
        const std::vector<uint64_t> va = draw(w, count);
        const UIntBatch a0 = UIntBatch::encrypt(key, va, w, 50 + w);
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
        std::vector<uint64_t> rows(w + 2);
        for (unsigned j = 0; j < w + 2; ++j)
            rows[j] = j == 1 ? 0 : j == 0 ? (1ull << w) - 1 : rnd(w);
        const F2Matrix m = F2Matrix::fromRows(rows, w);
        expect(std::string(linearRoute(ar, m, 3)) == "loop" && std::string(linearRoute(a0, m, 3)) == "call",
               "a ragged operand takes the loop" + tag);
        checkMap(key, ar, fa, m, 3, tag);
        checkMap(key, a0, va, m, 3, " uniform w=" + std::to_string(w));
        checkMap(key, ar, fa, F2Matrix::grayDecode(w), 0, tag + " grayDecode");
    }
    return 0;
}

int errors()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    int thrown = 0;
    thrown += throws<std::invalid_argument>([] { F2Matrix::identity(0); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::identity(65); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::shiftLeft(0, 1); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::shiftRight(65, 1); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::rotateLeft(0, 1); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::rotateRight(70, 1); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::grayEncode(0); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::grayDecode(65); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::mask(8, 0x100); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::mask(0, 0); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::clmul(8, 0x100); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::gfMul(8, 0x100, 0x11B); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::gfMul(8, 2, 0x21B); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::fromRows({}, 8); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::fromRows(std::vector<uint64_t>(65, 1), 8); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::fromRows({1, 2}, 0); });
    thrown += throws<std::invalid_argument>([] { F2Matrix::fromRows({1, 0x100}, 8); });
    expect(thrown == 17, "F2Matrix's builders throw (" + std::to_string(thrown) + " of 17)");
    const F2Matrix m8 = F2Matrix::identity(8), m4 = F2Matrix::identity(4), m84 = F2Matrix::fromRows({1, 2, 4, 8, 3, 5, 9, 15}, 4);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { m8 ^ m4; });
    thrown += throws<std::invalid_argument>([&] { m8 ^ m84; });
    thrown += throws<std::invalid_argument>([&] { m4 * m8; });
    thrown += throws<std::invalid_argument>([&] { m84 * m8; });
    expect(thrown == 4, "mismatched shapes throw (" + std::to_string(thrown) + " of 4)");
    expect((m8 * m84).outWidth() == 8 && (m8 * m84).inWidth() == 4 && (m84 * m4) == m84, "composition keeps the outer shape");
    expect(F2Matrix::shiftLeft(8, 9) == F2Matrix::fromRows(std::vector<uint64_t>(8, 0), 8) && F2Matrix::rotateLeft(8, 8) == m8 &&
               F2Matrix::shiftRight(64, 1).apply(~0ull) == ~0ull >> 1 && F2Matrix::rotateRight(64, 1).apply(1) == 1ull << 63,
           "shifts past the width, whole rotations, width 64");
    // linearMap and parity
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { linearMap(a4, m8); });                  // the width
    thrown += throws<std::invalid_argument>([&] { linearMap(a4, m4, 16); });              // the constant
    thrown += throws<std::invalid_argument>([&] { linearMap(a4, m84, 0x100); });
    thrown += throws<std::invalid_argument>([&] { linearRoute(a4, m8); });
    thrown += throws<std::invalid_argument>([&] { parity(a4, 16); });
    expect(thrown == 5, "linearMap, linearRoute and parity throw (" + std::to_string(thrown) + " of 5)");
    expect(linearMap(a4, m84, 0xFF).width() == 8, "a constant of the output width fits");
    // oversize: ONE element whose 64 planes share a payload of 2^21 terms (335 MB); a row of all of them has 2^27 terms
    // of 20 words, past 2^31 words per element.  The size check comes before any allocation or launch.
    CiphertextBatch big = a4.plane(0).slice(0, 1);
    for (int i = 0; i < 21; ++i)
        big = big + big;
    expect(big.terms() == (1u << 21), "the operand has 2^21 terms");
    std::vector<CiphertextBatch> planes(64, big);
    const UIntBatch wide = UIntBatch::fromPlanes(planes);
    const auto t0 = std::chrono::steady_clock::now();
    thrown = throws<std::invalid_argument>([&] { linearMap(wide, F2Matrix::fromRows({3, ~0ull, 5}, 64)); });
    thrown += throws<std::invalid_argument>([&] { parity(wide, ~0ull); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 2, "oversize throws (" + std::to_string(thrown) + " of 2)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // an empty batch: empty planes of the output width
    const UIntBatch e = linearMap(a4.slice(0, 0), m84, 5);
    expect(e.width() == 8 && e.size() == 0 && std::string(linearRoute(a4.slice(0, 0), m84)) == "loop", "an empty batch gives empty planes");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 3631, "uint_linear_driver", {{"words", words}, {"ragged", ragged}, {"errors", errors}});
}
