// matmul_driver.cpp -- user-style C++ over matMul / matMulTransposed / dot / sumGroups of include/certfhe/Batch.h:
// products of encrypted bit matrices over F2 (tests/test_matmul_cpp.py builds and runs it).
//   matmul_driver words     seeded encryptions, then matMul, matMulTransposed and dot: words == a loop of single
//                           Ciphertext operator* / operator+ on at(i); decryptions == the product over F2; sumGroups
//                           shares the payload
//   matmul_driver ragged    a compact()-ed (ragged) operand on either side: decryptions equal, words == the
//                           composition from gather, operator* and sumGroups
//   matmul_driver oversize  every bad argument throws std::invalid_argument before anything is allocated, and a later
//                           valid call still works
//   matmul_driver forms     "<shape> -> <form>": the form csgn_matmul_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Case {
    uint64_t rows, inner, cols;
};
const Case kCases[] = {{1, 1, 1}, {1, 40, 1}, {3, 5, 2}, {9, 4, 10}, {2, 33, 3}};

// (A x B) mod 2 of row-major bit matrices
std::vector<unsigned char> productBits(const std::vector<unsigned char> &a, const std::vector<unsigned char> &b,
                                       const Case &c)
{
    std::vector<unsigned char> out(c.rows * c.cols, 0);
    for (uint64_t i = 0; i < c.rows; ++i)
        for (uint64_t k = 0; k < c.cols; ++k)
            for (uint64_t e = 0; e < c.inner; ++e)
                out[i * c.cols + k] ^= a[i * c.inner + e] & b[e * c.cols + k];
    return out;
}

std::vector<unsigned char> transposeBits(const std::vector<unsigned char> &b, const Case &c)
{
    std::vector<unsigned char> bt(b.size());
    for (uint64_t e = 0; e < c.inner; ++e)
        for (uint64_t k = 0; k < c.cols; ++k)
            bt[k * c.inner + e] = b[e * c.cols + k];
    return bt;
}

// the definition by hand: single ciphertexts, operator* and operator+
Ciphertext definition(const CiphertextBatch &a, const CiphertextBatch &b, const Case &c, uint64_t i, uint64_t k,
                      bool transposed)
{
    Ciphertext acc = a.at(i * c.inner) * b.at(transposed ? k * c.inner : k);
    for (uint64_t e = 1; e < c.inner; ++e)
        acc = acc + a.at(i * c.inner + e) * b.at(transposed ? k * c.inner + e : e * c.cols + k);
    return acc;
}

void checkBits(const std::vector<unsigned char> &got, const std::vector<unsigned char> &want, const std::string &tag)
{
    expect(got.size() == want.size(), tag + ": size");
    for (size_t i = 0; i < want.size() && i < got.size(); ++i)
        if (got[i] != want[i]) {
            expect(false, tag + " element " + std::to_string(i));
            return;
        }
}

void checkWords(const CiphertextBatch &got, const CiphertextBatch &a, const CiphertextBatch &b, const Case &c,
                bool transposed, const std::string &tag)
{
    expect(got.size() == c.rows * c.cols, tag + ": elements");
    for (uint64_t i = 0; i < c.rows; ++i)
        for (uint64_t k = 0; k < c.cols; ++k)
            if (!sameWords(got.at(i * c.cols + k), definition(a, b, c, i, k, transposed))) {
                expect(false, tag + ": words of element (" + std::to_string(i) + ", " + std::to_string(k) + ")");
                return;
            }
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (const Case &c : kCases) {
        const std::vector<unsigned char> abits = randomBits(c.rows * c.inner), bbits = randomBits(c.inner * c.cols);
        const std::vector<unsigned char> want = productBits(abits, bbits, c);
        const CiphertextBatch a = CiphertextBatch::encrypt(key, abits, 11 + c.inner);
        const CiphertextBatch b = CiphertextBatch::encrypt(key, bbits, 12 + c.inner);
        const CiphertextBatch bt = CiphertextBatch::encrypt(key, transposeBits(bbits, c), 13 + c.inner);
        const std::string tag = " " + std::to_string(c.rows) + "x" + std::to_string(c.inner) + "x" + std::to_string(c.cols);
        const CiphertextBatch p = matMul(a, b, c.rows, c.inner, c.cols);
        expect(p.uniform() && p.terms() == c.inner, "terms" + tag);
        checkBits(p.decrypt(key), want, "matMul" + tag);
        checkWords(p, a, b, c, false, "matMul" + tag);
        const CiphertextBatch pt = matMulTransposed(a, bt, c.rows, c.inner, c.cols);
        checkBits(pt.decrypt(key), want, "matMulTransposed" + tag);
        checkWords(pt, a, bt, c, true, "matMulTransposed" + tag);
        // multi-term operands: sums of two encryptions
        const CiphertextBatch a2 = a + CiphertextBatch::encrypt(key, std::vector<unsigned char>(abits.size(), 0), 14);
        const CiphertextBatch b3 = (b + b) + b;
        const CiphertextBatch p6 = matMul(a2, b3, c.rows, c.inner, c.cols);
        expect(p6.terms() == 6 * c.inner, "multi-term terms" + tag);
        checkBits(p6.decrypt(key), want, "multi-term matMul" + tag);
        checkWords(p6, a2, b3, c, false, "multi-term matMul" + tag);
    }
    // dot: one element, the parity of the common ones
    const uint64_t len = 77;
    const std::vector<unsigned char> x = randomBits(len), y = randomBits(len);
    unsigned char parity = 0;
    for (uint64_t i = 0; i < len; ++i)
        parity ^= x[i] & y[i];
    const CiphertextBatch ex = CiphertextBatch::encrypt(key, x, 21), ey = CiphertextBatch::encrypt(key, y, 22);
    const CiphertextBatch d = dot(ex, ey);
    expect(d.size() == 1 && d.terms() == len, "dot: one element of `len` terms");
    expect(d.decrypt(key)[0] == parity, "dot decrypts to the parity");
    const Case one = {1, len, 1};
    checkWords(d, ex, ey, one, true, "dot");
    expect(sameBatchWords(d, matMulTransposed(ex, ey, 1, len, 1)), "dot == matMulTransposed(a, b, 1, n, 1)");
    // sumGroups shares the payload, and is the sum of its group
    const CiphertextBatch prod = ex * ey, s = prod.sumGroups(len), s7 = prod.sumGroups(7);
    expect(s.deviceValues() == prod.deviceValues() && s7.deviceValues() == prod.deviceValues(), "sumGroups shares the payload");
    expect(s.size() == 1 && s.terms() == len && s7.size() == 11 && s7.terms() == 7, "sumGroups shapes");
    expect(sameBatchWords(s, d), "sumGroups of the element-wise product == dot");
    Ciphertext acc = prod.at(7);
    for (uint64_t i = 8; i < 14; ++i)
        acc = acc + prod.at(i);
    expect(sameWords(s7.at(1), acc), "sumGroups element == the left-nested sum of its group");
    expect(sameBatchWords(prod.sumGroups(1), prod), "sumGroups(1) is the batch");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const Case c = {3, 6, 4};
    const std::vector<unsigned char> abits = randomBits(c.rows * c.inner), bbits = randomBits(c.inner * c.cols);
    const CiphertextBatch a = CiphertextBatch::encrypt(key, abits, 31), b = CiphertextBatch::encrypt(key, bbits, 32);
    const CiphertextBatch bt = CiphertextBatch::encrypt(key, transposeBits(bbits, c), 33);
    // x + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO twice, which
    // cancels: the batch is ragged
    auto raggedOf = [&](const CiphertextBatch &x) {
        std::vector<unsigned char> p(x.size(), 0), q(x.size(), 0);
        p[0] = 1;
        return addPlain(addPlain(x, p), q).compact();
    };
    const CiphertextBatch ar = raggedOf(a), br = raggedOf(b), btr = raggedOf(bt);
    expect(!ar.uniform() && !br.uniform() && !btr.uniform(), "compact() gave ragged batches");
    std::vector<unsigned char> af = abits, bf = bbits;
    af[0] ^= 1;
    bf[0] ^= 1;
    std::vector<uint64_t> ia, ib, ibt;
    for (uint64_t i = 0; i < c.rows; ++i)
        for (uint64_t k = 0; k < c.cols; ++k)
            for (uint64_t e = 0; e < c.inner; ++e) {
                ia.push_back(i * c.inner + e);
                ib.push_back(e * c.cols + k);
                ibt.push_back(k * c.inner + e);
            }
    const CiphertextBatch ra = matMul(ar, b, c.rows, c.inner, c.cols);
    checkBits(ra.decrypt(key), productBits(af, bbits, c), "ragged left");
    expect(sameBatchWords(ra, (ar.gather(ia) * b.gather(ib)).sumGroups(c.inner)), "ragged left: words == composition");
    const CiphertextBatch rb = matMul(a, br, c.rows, c.inner, c.cols);
    checkBits(rb.decrypt(key), productBits(abits, bf, c), "ragged right");
    expect(sameBatchWords(rb, (a.gather(ia) * br.gather(ib)).sumGroups(c.inner)), "ragged right: words == composition");
    const CiphertextBatch rt = matMulTransposed(ar, btr, c.rows, c.inner, c.cols);
    checkBits(rt.decrypt(key), productBits(af, bf, c), "ragged both, transposed");
    expect(sameBatchWords(rt, (ar.gather(ia) * btr.gather(ibt)).sumGroups(c.inner)), "ragged both: words == composition");
    checkWords(rt, ar, btr, c, true, "ragged both: words == the definition");
    // the rows that hold no changed element have the uniform product's words
    const CiphertextBatch u = matMul(a, b, c.rows, c.inner, c.cols);
    for (uint64_t x = c.cols; x < c.rows * c.cols; ++x)
        expect(sameWords(u.at(x), ra.at(x)), "ragged words == uniform words, element " + std::to_string(x));
    // sumGroups of a ragged batch: every group-th offset, the words shared
    const CiphertextBatch sr = ar.sumGroups(c.inner);
    expect(!sr.uniform() && sr.size() == c.rows && sr.deviceValues() == ar.deviceValues(), "ragged sumGroups shares the words");
    expect(sr.termsOf(0) == c.inner + 2 && sr.termsOf(1) == c.inner, "ragged sumGroups term counts");
    Ciphertext acc = ar.at(0);
    for (uint64_t e = 1; e < c.inner; ++e)
        acc = acc + ar.at(e);
    expect(sameWords(sr.at(0), acc), "ragged sumGroups element == the sum of its group");
    return 0;
}

int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const CiphertextBatch a = CiphertextBatch::encrypt(key, randomBits(12), 41), b = CiphertextBatch::encrypt(key, randomBits(12), 42);
    Context other(127, 8);
    SecretKey okey(other);
    const CiphertextBatch o = CiphertextBatch::encrypt(okey, randomBits(12), 43);
    // 2^21 terms a side: 12 * 2^42 terms per output element.  The batches are described, never allocated: a shared
    // payload read with another shape (sumGroups) keeps the driver within memory.
    const CiphertextBatch big = CiphertextBatch::encrypt(key, randomBits(1 << 16), 44);
    const CiphertextBatch wide = big.sumGroups(1 << 14);                 // 4 elements of 2^14 terms
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { matMul(a, o, 3, 4, 3); });                 // contexts
    thrown += throws<std::invalid_argument>([&] { matMul(a, b, 0, 4, 3); });                 // a zero dimension
    thrown += throws<std::invalid_argument>([&] { matMul(a, b, 3, 0, 3); });
    thrown += throws<std::invalid_argument>([&] { matMul(a, b, 3, 4, 0); });
    thrown += throws<std::invalid_argument>([&] { matMul(a, b, 3, 5, 3); });                 // a.size() != rows * inner
    thrown += throws<std::invalid_argument>([&] { matMul(a, b, 3, 4, 4); });                 // b.size() != inner * cols
    thrown += throws<std::invalid_argument>([&] { matMulTransposed(a, b, 2, 6, 3); });
    thrown += throws<std::invalid_argument>([&] { matMul(a, b, 1ull << 62, 4, 3); });        // rows * inner wraps
    thrown += throws<std::invalid_argument>([&] { dot(a, big); });                           // lengths differ
    thrown += throws<std::invalid_argument>([&] { matMul(wide, wide, 2, 2, 2); });           // 2 * 2^28 terms * 20 words
    thrown += throws<std::invalid_argument>([&] { dot(wide, wide); });
    thrown += throws<std::invalid_argument>([&] { a.sumGroups(0); });
    thrown += throws<std::invalid_argument>([&] { a.sumGroups(5); });
    thrown += throws<std::invalid_argument>([&] { a.sumGroups(24); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 14, "bad arguments throw (" + std::to_string(thrown) + " of 14)");
    expect(s < 1.0, "the checks ran before any launch (" + std::to_string(s) + " s)");
    // a later valid call still works
    const CiphertextBatch p = matMul(a, b, 3, 4, 3);
    const Case c = {3, 4, 3};
    checkWords(p, a, b, c, false, "a valid call after the refused ones");
    expect(a.sumGroups(12).size() == 1 && a.sumGroups(12).terms() == 12, "sumGroups of the whole batch");
    return 0;
}

// No device work: the form csgn_matmul_kernel names for the shapes of words, under the knob the process was started with.
int forms()
{
    for (const Case &c : kCases) {
        const char *form = csgn_matmul_kernel(1247, c.rows, c.inner, c.cols, 1, 1, 0);
        expect(form && *form, "the product has a form");
        printf("%llux%llux%llu -> %s\n", (unsigned long long)c.rows, (unsigned long long)c.inner,
               (unsigned long long)c.cols, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4720, "matmul_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
