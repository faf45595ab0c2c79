// uint_shift_driver.cpp -- user-style C++ over shiftLeft / shiftRight / rotateLeft / rotateRight by an ENCRYPTED distance
// and readAtEach of include/certfhe/UInt.h (tests/test_uint_shift_cpp.py builds and runs it).
//   uint_shift_driver words     every method at N=1247 against the same sum written with the public operators -- the
//                               left-nested sum over r of equalTo(d, r) * (the source plane) -- word for word, and its
//                               decryptions against plain integer arithmetic, every distance included; multi-term planes;
//                               the public-distance rotateRight
//   uint_shift_driver ragged    compact()ed operands and planes of different term counts take the composed route: the
//                               same words as that sum and the same decryptions
//   uint_shift_driver oversize  an output past 2^31 words per element throws before anything is allocated; mismatched
//                               counts and contexts and bad row counts throw; an empty batch is empty
//   uint_shift_driver forms     "<shape> -> <form>": the form csgn_uint_pick_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

struct Case {
    int op;
    unsigned w, v;
    uint64_t n;         // rows of an element's array (readAtEach), else 0
    size_t count;
};
const Case kCases[] = {
    {CSGN_UINT_PICK_SHL, 8, 3, 0, 40},  {CSGN_UINT_PICK_SHR, 8, 3, 0, 40},  {CSGN_UINT_PICK_ROTL, 8, 3, 0, 40},
    {CSGN_UINT_PICK_ROTR, 8, 3, 0, 40}, {CSGN_UINT_PICK_SHL, 5, 3, 0, 17},  {CSGN_UINT_PICK_SHR, 3, 2, 0, 100},
    {CSGN_UINT_PICK_ROTL, 5, 3, 0, 17}, {CSGN_UINT_PICK_ROTR, 16, 4, 0, 6}, {CSGN_UINT_PICK_SHL, 1, 1, 0, 9},
    {CSGN_UINT_PICK_EACH, 4, 3, 5, 12}, {CSGN_UINT_PICK_EACH, 1, 2, 4, 33}, {CSGN_UINT_PICK_EACH, 8, 4, 16, 3},
};
const size_t kNumCases = sizeof(kCases) / sizeof(kCases[0]);

uint64_t maskOf(unsigned w) { return w == 64 ? ~0ull : (1ull << w) - 1; }

uint64_t rowsOf(const Case &c, unsigned j)
{
    const uint64_t full = 1ull << c.v;
    switch (c.op) {
    case CSGN_UINT_PICK_SHL:
        return std::min<uint64_t>(j + 1, full);
    case CSGN_UINT_PICK_SHR:
        return std::min<uint64_t>(c.w - j, full);
    case CSGN_UINT_PICK_EACH:
        return c.n;
    default:
        return full;
    }
}

unsigned sourceOf(const Case &c, unsigned j, uint64_t r)
{
    switch (c.op) {
    case CSGN_UINT_PICK_SHL:
        return j - (unsigned)r;
    case CSGN_UINT_PICK_SHR:
        return j + (unsigned)r;
    case CSGN_UINT_PICK_ROTL:
        return (unsigned)((j + c.w - r % c.w) % c.w);
    case CSGN_UINT_PICK_ROTR:
        return (unsigned)((j + r) % c.w);
    default:
        return j;
    }
}

// plain integer arithmetic: a (or, for readAtEach, the element's array) by the distance d
uint64_t clear(const Case &c, uint64_t a, const uint64_t *array, uint64_t d)
{
    const unsigned w = c.w;
    switch (c.op) {
    case CSGN_UINT_PICK_SHL:
        return d < w ? (a << d) & maskOf(w) : 0;
    case CSGN_UINT_PICK_SHR:
        return d < w ? a >> d : 0;
    case CSGN_UINT_PICK_ROTL:
        d %= w;
        return d ? ((a << d) | (a >> (w - d))) & maskOf(w) : a;
    case CSGN_UINT_PICK_ROTR:
        d %= w;
        return d ? ((a >> d) | (a << (w - d))) & maskOf(w) : a;
    default:
        return d < c.n ? array[d] : 0;
    }
}

UIntBatch method(const Case &c, const UIntBatch &a, const UIntBatch &d)
{
    switch (c.op) {
    case CSGN_UINT_PICK_SHL:
        return a.shiftLeft(d);
    case CSGN_UINT_PICK_SHR:
        return a.shiftRight(d);
    case CSGN_UINT_PICK_ROTL:
        return a.rotateLeft(d);
    case CSGN_UINT_PICK_ROTR:
        return a.rotateRight(d);
    default:
        return readAtEach(a, c.n, d);
    }
}

// the definition with the public operators: equalTo(d, r) the left operand, a left-nested sum ascending in r
UIntBatch viaOperators(const Case &c, const UIntBatch &a, const UIntBatch &d)
{
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < c.w; ++j) {
        CiphertextBatch sum = a.plane(0);
        for (uint64_t r = 0; r < rowsOf(c, j); ++r) {
            CiphertextBatch value = a.plane(sourceOf(c, j, r));
            if (c.op == CSGN_UINT_PICK_EACH) {
                std::vector<uint64_t> idx(d.size());
                for (size_t e = 0; e < idx.size(); ++e)
                    idx[e] = e * c.n + r;
                value = value.gather(idx);
            }
            const CiphertextBatch p = equalTo(d, r) * value;
            sum = r == 0 ? p : sum + p;
        }
        planes.push_back(sum);
    }
    return UIntBatch::fromPlanes(planes);
}

struct Plain {
    std::vector<uint64_t> a, d, want;
};

// every distance among the first elements; the first integer has every bit set
Plain draw(const Case &c)
{
    Plain p;
    const uint64_t per = c.op == CSGN_UINT_PICK_EACH ? c.n : 1;
    for (size_t i = 0; i < c.count; ++i) {
        p.d.push_back(i < (1ull << c.v) ? i : rnd(c.v));
        for (uint64_t r = 0; r < per; ++r)
            p.a.push_back(i == 0 ? maskOf(c.w) : rnd(c.w));
        p.want.push_back(clear(c, p.a[i * per], &p.a[i * per], p.d[i]));
    }
    return p;
}

std::string tagOf(const Case &c)
{
    return " op=" + std::to_string(c.op) + " w=" + std::to_string(c.w) + " v=" + std::to_string(c.v) + " n=" +
           std::to_string(c.n) + " count=" + std::to_string(c.count);
}

void check(const SecretKey &key, const Case &c, const UIntBatch &a, const UIntBatch &d, const std::vector<uint64_t> *want,
           const std::string &tag)
{
    const UIntBatch got = method(c, a, d);
    expect(sameWords(got, viaOperators(c, a, d)), "method == the sum of equalTo(d, r) * source" + tag);
    if (want)
        checkValues(got.decrypt(key), *want, "decryption" + tag);
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    for (size_t i = 0; i < kNumCases; ++i) {
        const Case &c = kCases[i];
        const Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 30 + i), d = UIntBatch::encrypt(key, p.d, c.v, 60 + i);
        check(key, c, a, d, &p.want, tagOf(c));
        if (c.op == CSGN_UINT_PICK_EACH)
            expect(sameBatchWords(readAtEach(a.plane(0), c.n, d), readAtEach(a, c.n, d).plane(0)),
                   "readAtEach of bits == plane 0" + tagOf(c));
    }
    // multi-term planes (XOR with a trivial ZERO: two terms a plane, one count): the multi-term path, the same values
    for (size_t i = 0; i < kNumCases; i += 3) {
        Case c = kCases[i];
        c.count = std::min<size_t>(c.count, 10);
        const Plain p = draw(c);
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 90 + i), d = UIntBatch::encrypt(key, p.d, c.v, 120 + i);
        const UIntBatch za = UIntBatch::constant(ctx, std::vector<uint64_t>(p.a.size(), 0), c.w);
        const UIntBatch zd = UIntBatch::constant(ctx, std::vector<uint64_t>(p.d.size(), 0), c.v);
        check(key, c, a ^ za, d, &p.want, " multi-term a" + tagOf(c));
        check(key, c, a, d ^ zd, &p.want, " multi-term d" + tagOf(c));
    }
    // the public-distance sibling
    const std::vector<uint64_t> x(5, 0xB1);
    const UIntBatch a = UIntBatch::encrypt(key, x, 8, 7);
    for (unsigned s = 0; s < 20; ++s) {
        expect(sameWords(a.rotateRight(s), a.rotateLeft(8 - s % 8)), "rotateRight(s) == rotateLeft(width - s mod width)");
        const unsigned k = s % 8;
        checkValues(a.rotateRight(s).decrypt(key), std::vector<uint64_t>(5, k ? ((0xB1u >> k) | (0xB1u << (8 - k))) & 0xFF : 0xB1),
                    "rotateRight " + std::to_string(s));
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
        if (c.w > 8)
            continue;
        c.count = std::min<size_t>(c.count, 20);
        const Plain p = draw(c);
        const uint64_t per = c.op == CSGN_UINT_PICK_EACH ? c.n : 1;
        const UIntBatch a = UIntBatch::encrypt(key, p.a, c.w, 150 + i), d = UIntBatch::encrypt(key, p.d, c.v, 180 + i);
        const UIntBatch ar = raggedOf(a), dr = raggedOf(d);
        expect(!ar.plane(0).uniform() && !dr.plane(0).uniform(), "compact() gave ragged planes" + tagOf(c));
        // element 0 of a ragged operand has every bit flipped
        Plain pa = p, pd = p;
        pa.a[0] ^= maskOf(c.w);
        pd.d[0] ^= maskOf(c.v);
        for (size_t e = 0; e < c.count; ++e) {
            pa.want[e] = clear(c, pa.a[e * per], &pa.a[e * per], pa.d[e]);
            pd.want[e] = clear(c, pd.a[e * per], &pd.a[e * per], pd.d[e]);
        }
        check(key, c, ar, d, &pa.want, " ragged a" + tagOf(c));
        check(key, c, a, dr, &pd.want, " ragged d" + tagOf(c));
        // uniform planes of different term counts: plane 0 of two terms, the others of one
        if (c.w > 1) {
            std::vector<CiphertextBatch> planes;
            for (unsigned j = 0; j < c.w; ++j)
                planes.push_back(j == 0 ? a.plane(0) + UIntBatch::constant(ctx, std::vector<uint64_t>(p.a.size(), 0), 1).plane(0)
                                        : a.plane(j));
            const UIntBatch mixed = UIntBatch::fromPlanes(planes);
            expect(mixed.plane(0).uniform() && mixed.plane(0).terms() == 2 && mixed.plane(1).terms() == 1,
                   "planes of different term counts" + tagOf(c));
            check(key, c, mixed, d, &p.want, " different term counts" + tagOf(c));
        }
    }
    // a distance wider than 16 bits: only the low rows can be reached by a shift of 3 planes
    const Case c = {CSGN_UINT_PICK_SHL, 3, 18, 0, 6};
    Plain p = draw(c);
    for (size_t e = 0; e < c.count; ++e) {
        p.d[e] = e < 4 ? e : (1ull << 17) | e;
        p.want[e] = clear(c, p.a[e], nullptr, p.d[e]);
    }
    check(key, c, UIntBatch::encrypt(key, p.a, 3, 210), UIntBatch::encrypt(key, p.d, 18, 211), &p.want, " 18-bit distance");
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
    const UIntBatch d16 = UIntBatch::encrypt(key, x, 16, 1), a16 = UIntBatch::encrypt(key, x, 16, 2).slice(0, count);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < 16; ++j)
        planes.push_back((d16.plane(j) + d16.plane(j)) + d16.plane(j));
    const UIntBatch three = UIntBatch::fromPlanes(planes);          // 16 planes of 3 terms
    const UIntBatch d20 = UIntBatch::encrypt(key, std::vector<uint64_t>(count, 5), 20, 3);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { three.rotateLeft(d16); });     // 3^16 * 3 terms a plane
    thrown += throws<std::invalid_argument>([&] { three.rotateRight(d16); });
    thrown += throws<std::invalid_argument>([&] { a16.rotateLeft(three); });      // 7^16 terms
    thrown += throws<std::invalid_argument>([&] { a16.shiftLeft(three); });       // the top plane: 16 rows of 3-term planes
    thrown += throws<std::invalid_argument>([&] { a16.rotateLeft(d20); });        // 2^20 rows
    thrown += throws<std::invalid_argument>([&] { readAtEach(three.slice(0, 1), 1, three.slice(0, 1)); });   // 4^16 * 3
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 6, "oversize throws (" + std::to_string(thrown) + " of 6)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // counts, contexts, rows
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(12, 3), 4, 4);
    const UIntBatch d2 = UIntBatch::encrypt(key, std::vector<uint64_t>(12, 1), 2, 5);
    const UIntBatch i2 = UIntBatch::encrypt(key, std::vector<uint64_t>(3, 1), 2, 6);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o2 = UIntBatch::encrypt(okey, std::vector<uint64_t>(12, 1), 2, 7);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { a4.shiftLeft(d2.slice(0, 11)); });                // counts
    thrown += throws<std::invalid_argument>([&] { a4.shiftRight(d2.slice(0, 0)); });
    thrown += throws<std::invalid_argument>([&] { a4.rotateLeft(o2); });                            // contexts
    thrown += throws<std::invalid_argument>([&] { a4.rotateRight(o2); });
    thrown += throws<std::invalid_argument>([&] { readAtEach(a4, 0, i2); });                        // n of 0
    thrown += throws<std::invalid_argument>([&] { readAtEach(a4, 5, i2); });                        // n past 2^2
    thrown += throws<std::invalid_argument>([&] { readAtEach(a4, 3, i2); });                        // 12 != 3 * 3
    thrown += throws<std::invalid_argument>([&] { readAtEach(a4.plane(0), 3, i2); });
    thrown += throws<std::invalid_argument>([&] { readAtEach(a4, 4, o2.slice(0, 3)); });
    expect(thrown == 9, "bad counts, contexts and rows throw (" + std::to_string(thrown) + " of 9)");
    expect(readAtEach(a4, 4, i2).size() == 3 && readAtEach(a4, 4, i2).width() == 4, "readAtEach of 3 arrays of 4 rows");
    // an empty batch: empty planes
    const UIntBatch e4 = a4.slice(0, 0), e2 = d2.slice(0, 0);
    expect(e4.shiftLeft(e2).size() == 0 && e4.shiftLeft(e2).width() == 4, "an empty batch gives empty planes (shiftLeft)");
    expect(e4.rotateRight(e2).size() == 0 && e4.rotateRight(e2).width() == 4, "an empty batch gives empty planes (rotateRight)");
    expect(readAtEach(e4, 3, e2).size() == 0 && readAtEach(e4, 3, e2).width() == 4, "an empty batch gives empty planes (readAtEach)");
    return 0;
}

// No device work: the form csgn_uint_pick_kernel names for the shapes of words (fresh planes), under the knob the process
// was started with.
int forms()
{
    for (size_t i = 0; i < kNumCases; ++i) {
        const Case &c = kCases[i];
        const std::vector<uint64_t> one(16, 1);
        const char *form = csgn_uint_pick_kernel(1247, c.op, c.count, c.v, one.data(), c.w, c.n, 1);
        expect(form && *form, "the operation has a form");
        printf("op=%d w=%u v=%u n=%llu count=%zu -> %s\n", c.op, c.w, c.v, (unsigned long long)c.n, c.count, form ? form : "");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4724, "uint_shift_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
