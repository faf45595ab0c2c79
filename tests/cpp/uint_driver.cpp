// uint_driver.cpp -- user-style C++ over include/certfhe/UInt.h (tests/test_uint_cpp.py builds and runs it).
//   uint_driver ops       1..8-bit add, sub, the six comparisons and select over 1000 random pairs: decryptions ==
//                         clear arithmetic, words == the definition composed from CiphertextBatch operators and Gates.h
//   uint_driver ragged    the same from compacted (ragged) planes: same decryptions, words == the composition
//   uint_driver encrypt   reproducible encrypt == CiphertextBatch::encrypt plane by plane; argument checks
//   uint_driver oversize  a width whose steps exceed 2^31 words per element throws before anything is allocated
//   uint_driver forms     "<shape> -> <form>": the form csgn_uint_step_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

// -- the definitions of UInt.h, composed by hand from the batch operators and Gates.h
CiphertextBatch ones(const Context &ctx, uint64_t n) { return constantBatch(ctx, std::vector<unsigned char>(n, 1)); }

std::vector<CiphertextBatch> refAddSub(const UIntBatch &a, const UIntBatch &b, bool sub)
{
    const CiphertextBatch one = ones(a.context(), a.size());
    std::vector<CiphertextBatch> out;
    CiphertextBatch c = one;
    for (unsigned j = 0; j < a.width(); ++j) {
        const CiphertextBatch bj = sub ? logicNot(b.plane(j)) : b.plane(j);
        const CiphertextBatch ab = a.plane(j) + bj;
        if (j == 0 && !sub) {                                      // ADD_HALF
            out.push_back(ab);
            c = a.plane(j) * bj;
            continue;
        }
        out.push_back(ab + c);                                     // ADD_FULL
        c = (a.plane(j) * bj) + (ab * c);
    }
    return out;
}

CiphertextBatch refEq(const UIntBatch &a, const UIntBatch &b)
{
    const CiphertextBatch one = ones(a.context(), a.size());
    CiphertextBatch e = logicXnor(a.plane(0), b.plane(0));
    for (unsigned j = 1; j < a.width(); ++j)
        e = e * ((a.plane(j) + b.plane(j)) + one);
    return e;
}

CiphertextBatch refLt(const UIntBatch &a, const UIntBatch &b)
{
    const CiphertextBatch one = ones(a.context(), a.size());
    CiphertextBatch l = (a.plane(0) + one) * b.plane(0);
    for (unsigned j = 1; j < a.width(); ++j)
        l = ((a.plane(j) + b.plane(j)) * (b.plane(j) + l)) + l;
    return l;
}

void checkBits(const CiphertextBatch &r, SecretKey &key, const std::vector<uint64_t> &want, const std::string &what)
{
    const std::vector<unsigned char> got = r.decrypt(key);
    bool ok = got.size() == want.size();
    for (size_t i = 0; ok && i < want.size(); ++i)
        ok = got[i] == want[i];
    expect(ok, what);
}

void checkPlanes(const UIntBatch &r, const std::vector<CiphertextBatch> &want, const std::string &what)
{
    bool ok = r.width() == want.size();
    for (unsigned j = 0; ok && j < r.width(); ++j)
        ok = sameBatchWords(r.plane(j), want[j]);
    expect(ok, what);
}

// every operation of UInt.h on (a, b, s) against clear values and, with `words`, against the compositions
void checkAll(const UIntBatch &a, const UIntBatch &b, const CiphertextBatch &s, SecretKey &key,
              const std::vector<uint64_t> &va, const std::vector<uint64_t> &vb, const std::vector<uint64_t> &vs,
              unsigned w, bool words, const std::string &tag)
{
    const size_t n = va.size();
    const uint64_t mask = w == 64 ? ~0ull : (1ull << w) - 1;
    std::vector<uint64_t> sum(n), diff(n), eq(n), ne(n), lt(n), le(n), gt(n), ge(n), sel(n);
    for (size_t i = 0; i < n; ++i) {
        sum[i] = (va[i] + vb[i]) & mask;
        diff[i] = (va[i] - vb[i]) & mask;
        eq[i] = va[i] == vb[i];
        ne[i] = va[i] != vb[i];
        lt[i] = va[i] < vb[i];
        le[i] = va[i] <= vb[i];
        gt[i] = va[i] > vb[i];
        ge[i] = va[i] >= vb[i];
        sel[i] = vs[i] ? va[i] : vb[i];
    }
    const UIntBatch rs = a + b, rd = a - b, rsel = select(s, a, b);
    const CiphertextBatch req = equalTo(a, b), rlt = lessThan(a, b), rgt = greaterThan(a, b);
    checkValues(rs.decrypt(key), sum, "add" + tag);
    checkValues(rd.decrypt(key), diff, "sub" + tag);
    checkBits(req, key, eq, "equalTo" + tag);
    checkBits(notEqualTo(a, b), key, ne, "notEqualTo" + tag);
    checkBits(rlt, key, lt, "lessThan" + tag);
    checkBits(lessEqual(a, b), key, le, "lessEqual" + tag);
    checkBits(rgt, key, gt, "greaterThan" + tag);
    checkBits(greaterEqual(a, b), key, ge, "greaterEqual" + tag);
    checkValues(rsel.decrypt(key), sel, "select" + tag);
    if (!words)
        return;
    checkPlanes(rs, refAddSub(a, b, false), "add words" + tag);
    checkPlanes(rd, refAddSub(a, b, true), "sub words" + tag);
    const CiphertextBatch e = refEq(a, b), l = refLt(a, b), g = refLt(b, a);
    expect(sameBatchWords(req, e), "equalTo words" + tag);
    expect(sameBatchWords(notEqualTo(a, b), logicNot(e)), "notEqualTo words" + tag);
    expect(sameBatchWords(rlt, l), "lessThan words" + tag);
    expect(sameBatchWords(rgt, g), "greaterThan words" + tag);
    expect(sameBatchWords(lessEqual(a, b), logicNot(g)), "lessEqual words" + tag);
    expect(sameBatchWords(greaterEqual(a, b), logicNot(l)), "greaterEqual words" + tag);
    std::vector<CiphertextBatch> m;
    for (unsigned j = 0; j < w; ++j)
        m.push_back((s * (a.plane(j) + b.plane(j))) + b.plane(j));
    checkPlanes(rsel, m, "select words" + tag);
}

struct Inputs {
    std::vector<uint64_t> va, vb, vs;
};

Inputs randomInputs(size_t count, unsigned w)
{
    Inputs in;
    for (size_t i = 0; i < count; ++i) {
        in.va.push_back(rnd(w));
        in.vb.push_back(i % 7 == 0 ? in.va.back() : rnd(w));        // some equal pairs
        in.vs.push_back(rand() & 1);
    }
    return in;
}

std::vector<unsigned char> low(const std::vector<uint64_t> &v)
{
    std::vector<unsigned char> b(v.size());
    for (size_t i = 0; i < v.size(); ++i)
        b[i] = (unsigned char)(v[i] & 1);
    return b;
}

int ops()
{
    Context ctx(127, 8);               // small terms: an 8-bit equality has 3^8 terms a value
    SecretKey key(ctx);
    const size_t count = 1000;
    for (unsigned w = 1; w <= 8; ++w) {
        const Inputs in = randomInputs(count, w);
        const UIntBatch a = UIntBatch::encrypt(key, in.va, w), b = UIntBatch::encrypt(key, in.vb, w, 1000 + w);
        const CiphertextBatch s = CiphertextBatch::encrypt(key, low(in.vs), 77);
        checkAll(a, b, s, key, in.va, in.vb, in.vs, w, true, " w=" + std::to_string(w));
    }
    // a constant operand (public values) mixes with encrypted ones
    const Inputs in = randomInputs(count, 4);
    const UIntBatch a = UIntBatch::encrypt(key, in.va, 4, 5), k = UIntBatch::constant(ctx, in.vb, 4);
    checkAll(a, k, CiphertextBatch::encrypt(key, low(in.vs), 6), key, in.va, in.vb, in.vs, 4, true, " constant");
    return 0;
}

// planes made ragged: p_j + C(x) + C(y), compacted -- the constants cancel where x == y (1 term), stay where not
// (3 terms); the value is unchanged when x == y everywhere and flips bit j where they differ, so the clear values
// follow from the flips
int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const size_t count = 400;
    for (unsigned w = 1; w <= 5; ++w) {
        Inputs in = randomInputs(count, w);
        const UIntBatch a0 = UIntBatch::encrypt(key, in.va, w, 10), b0 = UIntBatch::encrypt(key, in.vb, w, 20);
        std::vector<CiphertextBatch> pa, pb;
        for (unsigned j = 0; j < w; ++j) {
            std::vector<unsigned char> x(count), y(count);
            for (size_t i = 0; i < count; ++i) {
                x[i] = (unsigned char)(rand() & 1);
                y[i] = (unsigned char)(rand() & 1);
                in.va[i] ^= (uint64_t)(x[i] ^ y[i]) << j;
            }
            pa.push_back(addPlain(addPlain(a0.plane(j), x), y).compact());
            pb.push_back(j % 2 ? b0.plane(j) : addPlain(addPlain(b0.plane(j), y), y).compact());   // uniform again
        }
        expect(!pa[0].uniform(), "compact() gave a ragged plane");
        const UIntBatch a = UIntBatch::fromPlanes(pa), b = UIntBatch::fromPlanes(pb);
        checkAll(a, b, CiphertextBatch::encrypt(key, low(in.vs), 30), key, in.va, in.vb, in.vs, w, true,
                 " ragged w=" + std::to_string(w));
        // compact() of a whole integer keeps its value
        checkValues(a.compact().decrypt(key), in.va, "compact" + std::to_string(w));
    }
    return 0;
}

int encrypt()
{
    Context ctx(1247, 16), other(1247, 8);
    SecretKey key(ctx), key2(other);
    const size_t count = 257;
    const Inputs in = randomInputs(count, 13);
    const UIntBatch a = UIntBatch::encrypt(key, in.va, 13, 99);
    expect(a.width() == 13 && a.size() == count, "width / size");
    for (unsigned j = 0; j < 13; ++j) {
        std::vector<unsigned char> bits(count);
        for (size_t i = 0; i < count; ++i)
            bits[i] = (unsigned char)((in.va[i] >> j) & 1);
        expect(sameBatchWords(a.plane(j), CiphertextBatch::encrypt(key, bits, 99, (uint64_t)j * count)),
               "plane " + std::to_string(j));
    }
    checkValues(a.decrypt(key), in.va, "decrypt");
    checkValues(UIntBatch::encrypt(key, in.va, 13).decrypt(key), in.va, "OS-keyed encrypt");
    checkValues(UIntBatch::constant(ctx, in.va, 13).decrypt(key), in.va, "constant");
    std::vector<uint64_t> big(3, ~0ull);
    checkValues(UIntBatch::encrypt(key, big, 64, 3).decrypt(key), big, "64-bit values");
    // argument checks
    expect(throws<std::invalid_argument>([&] { UIntBatch::encrypt(key, in.va, 0); }), "width 0");
    expect(throws<std::invalid_argument>([&] { UIntBatch::encrypt(key, in.va, 65, 1); }), "width 65");
    expect(throws<std::invalid_argument>([&] { UIntBatch::encrypt(key, std::vector<uint64_t>(1, 8), 3, 1); }),
           "value >= 2^width");
    expect(throws<std::invalid_argument>([&] { UIntBatch::constant(ctx, std::vector<uint64_t>(1, 2), 1); }),
           "constant >= 2^width");
    expect(throws<std::invalid_argument>([&] { UIntBatch::fromPlanes(std::vector<CiphertextBatch>()); }), "no planes");
    const UIntBatch b12 = UIntBatch::encrypt(key, std::vector<uint64_t>(count, 1), 12, 1);
    const UIntBatch c13 = UIntBatch::encrypt(key, std::vector<uint64_t>(count - 1, 1), 13, 1);
    const UIntBatch d13 = UIntBatch::encrypt(key2, std::vector<uint64_t>(count, 1), 13, 1);
    expect(throws<std::invalid_argument>([&] { a + b12; }), "width mismatch");
    expect(throws<std::invalid_argument>([&] { a - c13; }), "count mismatch");
    expect(throws<std::invalid_argument>([&] { equalTo(a, d13); }), "context mismatch");
    expect(throws<std::invalid_argument>([&] { select(c13.plane(0), a, a); }), "selector count mismatch");
    expect(throws<std::invalid_argument>(
               [&] { UIntBatch::fromPlanes(std::vector<CiphertextBatch>(1, c13.plane(0))) + a; }),
           "fromPlanes width mismatch");
    bool caught = false;
    try {
        a.plane(13);
    } catch (const std::out_of_range &) {
        caught = true;
    }
    expect(caught, "plane(width) out of range");
    return 0;
}

// 24-bit values over 100 000 elements at N=1247: equality needs 3^24 terms (far above 2^31 words per element), and
// its first steps alone would need more HBM than the device has.  The check comes first, so each call throws
// std::invalid_argument at once; a check made step by step would fail on an allocation instead.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 100000;
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = rnd(24);
    const UIntBatch a = UIntBatch::encrypt(key, v, 24, 1), b = UIntBatch::encrypt(key, v, 24, 2);
    const auto t0 = std::chrono::steady_clock::now();
    expect(throws<std::invalid_argument>([&] { equalTo(a, b); }), "equalTo");
    expect(throws<std::invalid_argument>([&] { notEqualTo(a, b); }), "notEqualTo");
    expect(throws<std::invalid_argument>([&] { lessThan(a, b); }), "lessThan");
    expect(throws<std::invalid_argument>([&] { greaterEqual(a, b); }), "greaterEqual");
    expect(throws<std::invalid_argument>([&] { a - b; }), "operator-");
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(s < 1.0, "the size checks ran before any launch (" + std::to_string(s) + " s)");
    return 0;
}

// No device work: the form csgn_uint_step_kernel names for the steps of ops (1000 elements at N=127, fresh planes, the
// running carry / accumulator of the sizes the chains reach), under the knob the process was started with.
int forms()
{
    const char *names[] = {"", "ADD_HALF", "ADD_FULL", "EQ_STEP", "LT_FIRST", "LT_STEP"};
    const uint64_t tx[] = {1, 3, 9, 27, 200};
    for (uint64_t x : tx)
        for (int s = CSGN_UINT_ADD_HALF; s <= CSGN_UINT_LT_STEP; ++s) {
            const char *form = csgn_uint_step_kernel(127, s, 1000, x, 1, 1);
            expect(form && *form, std::string(names[s]) + " has a form");
            printf("%s tx=%llu ta=1 tb=1 -> %s\n", names[s], (unsigned long long)x, form ? form : "");
        }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4242, "uint_driver",
                    {{"ops", ops}, {"ragged", ragged}, {"encrypt", encrypt}, {"oversize", oversize}, {"forms", forms}});
}
