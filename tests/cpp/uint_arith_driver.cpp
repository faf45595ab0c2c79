// uint_arith_driver.cpp -- user-style C++ over a + b, a - b, add / sub with the carry, equalTo, notEqualTo, lessThan and
// greaterThan of include/certfhe/UInt.h (tests/test_uint_arith_cpp.py builds and runs it).
//   uint_arith_driver words     widths 1, 3, 4, 8 and 10 at N=1247, ties included: words == the per-bit definition composed
//                               from the CiphertextBatch operators bit for bit, decryptions == the plaintext sums,
//                               differences, carries and comparisons; multi-term planes; a 17-bit sum (the chain)
//   uint_arith_driver ragged    a compact()ed (ragged) operand takes the chain: the same words and decryptions
//   uint_arith_driver oversize  width 16 with 3-term planes throws before anything is allocated; mismatched widths,
//                               counts and contexts throw; an empty batch is empty
//   uint_arith_driver forms     "<shape> -> <route> <form>": the route the classes take (arithRoute) and the form
//                               csgn_uint_arith_kernel names, under the process's knobs
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Case {
    unsigned w;
    size_t count;
};
const Case kCases[] = {{1, 40}, {4, 200}, {8, 6}, {10, 2}, {3, 1000}};

struct Plain {
    std::vector<uint64_t> a, b, sum, diff, cadd, csub, eq, ne, lt, gt;
};

// every third element a tie
Plain draw(unsigned w, size_t count)
{
    Plain p;
    const uint64_t mask = (1ull << w) - 1;
    for (size_t i = 0; i < count; ++i) {
        const uint64_t a = rnd(w), b = i % 3 == 0 ? a : rnd(w);
        p.a.push_back(a);
        p.b.push_back(b);
    }
    for (size_t i = 0; i < count; ++i) {
        const uint64_t a = p.a[i], b = p.b[i];
        p.sum.push_back((a + b) & mask);
        p.diff.push_back((a - b) & mask);
        p.cadd.push_back((a + b) >> w);
        p.csub.push_back(a >= b);
        p.eq.push_back(a == b);
        p.ne.push_back(a != b);
        p.lt.push_back(a < b);
        p.gt.push_back(a > b);
    }
    return p;
}

std::vector<uint64_t> bits(const SecretKey &key, const CiphertextBatch &x)
{
    const std::vector<unsigned char> d = x.decrypt(key);
    return std::vector<uint64_t>(d.begin(), d.end());
}

CiphertextBatch oneBatch(const UIntBatch &a)
{
    return constantBatch(a.context(), std::vector<unsigned char>(a.size(), 1));
}

// The definition, composed from the CiphertextBatch operators in the order of include/csgn_hip.h's step table.
struct Composed {
    std::vector<CiphertextBatch> sum, diff;
    CiphertextBatch cadd, csub, eq, ne, lt, gt;
};

CiphertextBatch composedLess(const UIntBatch &a, const UIntBatch &b)
{
    CiphertextBatch l = logicNot(a.plane(0)) * b.plane(0);
    for (unsigned j = 1; j < a.width(); ++j)
        l = ((a.plane(j) + b.plane(j)) * (b.plane(j) + l)) + l;
    return l;
}

Composed compose(const UIntBatch &a, const UIntBatch &b)
{
    const unsigned w = a.width();
    CiphertextBatch c = a.plane(0) * b.plane(0);
    std::vector<CiphertextBatch> sum(1, a.plane(0) + b.plane(0));
    for (unsigned j = 1; j < w; ++j) {
        const CiphertextBatch ab = a.plane(j) + b.plane(j);
        sum.push_back(ab + c);
        c = (a.plane(j) * b.plane(j)) + (ab * c);
    }
    CiphertextBatch d = oneBatch(a);
    std::vector<CiphertextBatch> diff;
    for (unsigned j = 0; j < w; ++j) {
        const CiphertextBatch nb = logicNot(b.plane(j)), ab = a.plane(j) + nb;
        diff.push_back(ab + d);
        d = (a.plane(j) * nb) + (ab * d);
    }
    CiphertextBatch e = logicXnor(a.plane(0), b.plane(0));
    for (unsigned j = 1; j < w; ++j)
        e = e * logicXnor(a.plane(j), b.plane(j));
    return Composed{sum, diff, c, d, e, logicNot(e), composedLess(a, b), composedLess(b, a)};
}

// the sum alone, for widths whose difference and equality are past every limit
std::vector<CiphertextBatch> compose17(const UIntBatch &a, const UIntBatch &b, CiphertextBatch *carry)
{
    CiphertextBatch c = a.plane(0) * b.plane(0);
    std::vector<CiphertextBatch> sum(1, a.plane(0) + b.plane(0));
    for (unsigned j = 1; j < a.width(); ++j) {
        const CiphertextBatch ab = a.plane(j) + b.plane(j);
        sum.push_back(ab + c);
        if (j + 1 < a.width() || carry)
            c = (a.plane(j) * b.plane(j)) + (ab * c);
    }
    if (carry)
        *carry = c;
    return sum;
}

bool samePlanes(const UIntBatch &x, const std::vector<CiphertextBatch> &y)
{
    if (x.width() != y.size())
        return false;
    for (unsigned j = 0; j < x.width(); ++j)
        if (!sameBatchWords(x.plane(j), y[j]))
            return false;
    return true;
}

// every entry point against the composition, and against the plaintext when `p` is given
void checkAll(const SecretKey &key, const UIntBatch &a, const UIntBatch &b, const Plain *p, const std::string &tag)
{
    const Composed want = compose(a, b);
    const UIntBatch s = a + b, d = a - b;
    expect(samePlanes(s, want.sum), "a + b == the ADD steps" + tag);
    expect(samePlanes(d, want.diff), "a - b == the ADD steps over ~b" + tag);
    CiphertextBatch cs = a.plane(0), cd = a.plane(0);
    const UIntBatch s2 = a.add(b, &cs), d2 = a.sub(b, &cd);
    expect(samePlanes(s2, want.sum) && sameBatchWords(cs, want.cadd), "add with its carry" + tag);
    expect(samePlanes(d2, want.diff) && sameBatchWords(cd, want.csub), "sub with its carry" + tag);
    expect(samePlanes(a.add(b, nullptr), want.sum) && samePlanes(a.sub(b, nullptr), want.diff), "a null carry" + tag);
    const CiphertextBatch eq = equalTo(a, b), ne = notEqualTo(a, b), lt = lessThan(a, b), gt = greaterThan(a, b);
    expect(sameBatchWords(eq, want.eq), "equalTo == XNOR and the EQ steps" + tag);
    expect(sameBatchWords(ne, want.ne), "notEqualTo == logicNot(equalTo)" + tag);
    expect(sameBatchWords(lt, want.lt), "lessThan == the LT steps" + tag);
    expect(sameBatchWords(gt, want.gt), "greaterThan == lessThan(b, a)" + tag);
    expect(sameBatchWords(lessEqual(a, b), logicNot(want.gt)) && sameBatchWords(greaterEqual(a, b), logicNot(want.lt)),
           "lessEqual and greaterEqual keep their logicNot" + tag);
    if (p) {
        checkValues(s.decrypt(key), p->sum, "a + b" + tag);
        checkValues(d.decrypt(key), p->diff, "a - b" + tag);
        checkValues(bits(key, cs), p->cadd, "the carry of add" + tag);
        checkValues(bits(key, cd), p->csub, "the carry of sub (a >= b)" + tag);
        checkValues(bits(key, eq), p->eq, "equalTo" + tag);
        checkValues(bits(key, ne), p->ne, "notEqualTo" + tag);
        checkValues(bits(key, lt), p->lt, "lessThan" + tag);
        checkValues(bits(key, gt), p->gt, "greaterThan" + tag);
    }
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (const Case &c : kCases) {
        const Plain p = draw(c.w, c.count);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 30 + c.count), b = UIntBatch::encrypt(key, p.b, c.w, 31 + c.count);
        checkAll(key, a, b, &p, " w=" + std::to_string(c.w) + " count=" + std::to_string(c.count));
    }
    // a + a, a - a, equalTo(a, a): the operands alias
    const Plain q = draw(5, 30);
    const UIntBatch a5 = UIntBatch::encrypt(key, q.a, 5, 50);
    checkAll(key, a5, a5, nullptr, " a with itself");
    checkValues((a5 - a5).decrypt(key), std::vector<uint64_t>(30, 0), "a - a");
    // multi-term planes (sums with a trivial ZERO): the multi-term path, the same values
    const Plain p = draw(3, 50);
    const UIntBatch a0 = UIntBatch::encrypt(key, p.a, 3, 40), b0 = UIntBatch::encrypt(key, p.b, 3, 41);
    const UIntBatch zero = UIntBatch::constant(ctx, std::vector<uint64_t>(50, 0), 3);
    checkAll(key, a0 ^ zero, b0, &p, " multi-term a");
    checkAll(key, a0, (b0 ^ zero) ^ zero, &p, " multi-term b");
    // wider than 16 bits: the chain; the sum alone (a fresh 17-bit difference or equality is 3^17 terms an element)
    const Plain wide = draw(17, 3);
    const UIntBatch aw = UIntBatch::encrypt(key, wide.a, 17, 60), bw = UIntBatch::encrypt(key, wide.b, 17, 61);
    expect(std::string(arithRoute(17, true)) == "chain", "17 bits take the chain");
    CiphertextBatch cw = aw.plane(0);
    const UIntBatch sw = aw.add(bw, &cw);
    expect(samePlanes(sw, compose17(aw, bw, nullptr)), "a + b at 17 bits == the ADD steps");
    checkValues(sw.decrypt(key), wide.sum, "a + b at 17 bits");
    checkValues(bits(key, cw), wide.cadd, "the carry of add at 17 bits");
    checkValues((aw + bw).decrypt(key), wide.sum, "operator+ at 17 bits");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 4; ++w) {
        Plain p = draw(w, 60);
        const UIntBatch a0 = UIntBatch::encrypt(key, p.a, w, 50 + w), b0 = UIntBatch::encrypt(key, p.b, w, 60 + w);
        // plane + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO
        // twice, which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
        auto raggedOf = [&](const UIntBatch &x) {
            std::vector<unsigned char> q0(x.size(), 0), q1(x.size(), 0);
            q0[0] = 1;
            std::vector<CiphertextBatch> pr;
            for (unsigned j = 0; j < x.width(); ++j)
                pr.push_back(addPlain(addPlain(x.plane(j), q0), q1).compact());
            return UIntBatch::fromPlanes(pr);
        };
        const std::string tag = " w=" + std::to_string(w);
        const UIntBatch ar = raggedOf(a0);
        expect(!ar.plane(0).uniform(), "compact() gave ragged planes" + tag);
        expect(std::string(arithRoute(w, false)) == "chain", "a ragged operand takes the chain" + tag);
        // element 0 of the ragged operand has every bit flipped
        std::vector<uint64_t> fa = p.a;
        fa[0] ^= (1ull << w) - 1;
        Plain pa = draw(w, 0), pb = draw(w, 0);
        const uint64_t mask = (1ull << w) - 1;
        for (size_t i = 0; i < fa.size(); ++i) {
            const uint64_t x = fa[i], y = p.b[i];
            pa.sum.push_back((x + y) & mask), pa.diff.push_back((x - y) & mask), pa.cadd.push_back((x + y) >> w);
            pa.csub.push_back(x >= y), pa.eq.push_back(x == y), pa.ne.push_back(x != y), pa.lt.push_back(x < y), pa.gt.push_back(x > y);
            pb.sum.push_back((y + x) & mask), pb.diff.push_back((y - x) & mask), pb.cadd.push_back((y + x) >> w);
            pb.csub.push_back(y >= x), pb.eq.push_back(y == x), pb.ne.push_back(y != x), pb.lt.push_back(y < x), pb.gt.push_back(y > x);
        }
        checkAll(key, ar, b0, &pa, " ragged a" + tag);
        checkAll(key, b0, ar, &pb, " ragged b" + tag);
    }
    return 0;
}

// 16-bit integers of 3 terms a plane at N=1247: an equality of 7^16 terms, a carry of about 6^16.  The size check comes
// first, so the call throws std::invalid_argument at once, before any allocation or launch.
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
        planes.push_back((x0.plane(j) + x0.plane(j)) + x0.plane(j));
    const UIntBatch wide = UIntBatch::fromPlanes(planes);
    CiphertextBatch carry = x0.plane(0);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { wide + wide; });
    thrown += throws<std::invalid_argument>([&] { wide - x0; });
    thrown += throws<std::invalid_argument>([&] { wide.add(wide, &carry); });
    thrown += throws<std::invalid_argument>([&] { x0.sub(wide, &carry); });
    thrown += throws<std::invalid_argument>([&] { equalTo(wide, wide); });
    thrown += throws<std::invalid_argument>([&] { notEqualTo(x0, wide); });
    thrown += throws<std::invalid_argument>([&] { lessThan(wide, wide); });
    thrown += throws<std::invalid_argument>([&] { greaterThan(wide, x0); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 8, "oversize throws (" + std::to_string(thrown) + " of 8)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    expect(carry.size() == count && carry.uniform() && carry.terms() == 1, "a refused call leaves the carry alone");
    // widths, counts, contexts
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    const UIntBatch b5 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 5, 4);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o4 = UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 1), 4, 7);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { a4 + b5; });                                         // widths
    thrown += throws<std::invalid_argument>([&] { a4 - a4.slice(0, 9); });                             // counts
    thrown += throws<std::invalid_argument>([&] { a4.add(o4, &carry); });                              // contexts
    thrown += throws<std::invalid_argument>([&] { a4.sub(b5, nullptr); });
    thrown += throws<std::invalid_argument>([&] { equalTo(a4, o4); });
    thrown += throws<std::invalid_argument>([&] { notEqualTo(a4, b5); });
    thrown += throws<std::invalid_argument>([&] { lessThan(a4, a4.slice(0, 9)); });
    thrown += throws<std::invalid_argument>([&] { greaterThan(o4, a4); });
    expect(thrown == 8, "bad widths, counts and contexts throw (" + std::to_string(thrown) + " of 8)");
    // an empty batch: empty planes
    const UIntBatch e4 = a4.slice(0, 0);
    const UIntBatch es = e4.add(e4, &carry);
    expect(es.width() == 4 && es.size() == 0 && carry.size() == 0, "an empty batch gives empty planes and an empty carry");
    expect((e4 - e4).size() == 0 && equalTo(e4, e4).size() == 0 && notEqualTo(e4, e4).size() == 0 && lessThan(e4, e4).size() == 0,
           "an empty batch gives empty results");
    return 0;
}

// No device work: the route of the classes and the form csgn_uint_arith_kernel names for the shapes of words (fresh
// planes), under the knobs the process was started with.
int forms()
{
    const char *names[] = {"add", "sub", "eq", "ne"};
    for (const Case &c : kCases) {
        const std::vector<uint64_t> one(16, 1);
        for (int op = CSGN_UINT_ARITH_ADD; op <= CSGN_UINT_ARITH_NE; ++op) {
            const char *form = csgn_uint_arith_kernel(1247, op, c.count, c.w, one.data(), one.data(), op <= CSGN_UINT_ARITH_SUB);
            expect(form && *form, "the operation has a form");
            printf("%s w=%u count=%zu -> %s %s\n", names[op - 1], c.w, c.count, arithRoute(c.w, true), form ? form : "");
        }
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4728, "uint_arith_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
