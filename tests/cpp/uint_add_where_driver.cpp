// uint_add_where_driver.cpp -- user-style C++ over addWhere, subWhere, incrementWhere and decrementWhere of
// include/certfhe/UInt.h (tests/test_uint_add_where_cpp.py builds and runs it).
//   uint_add_where_driver words     widths 8, 32 and 40 at N=1247: the route of the process's knob, the call route and the
//                                   loop give the same words, those of the definition composed from the CiphertextBatch
//                                   operators; decryptions == the plaintext, and at width 8 == what
//                                   a + keepWhere(mask, constant) decrypts to; multi-term planes; k = 0 shares payloads;
//                                   the route addWhereRoute(mask, a, k) names on both sides of the measured rule
//   uint_add_where_driver ragged    a compact()ed (ragged) mask or plane takes the loop: the same words and decryptions
//   uint_add_where_driver oversize  a 32-bit decrement and 3-term planes throw before anything is allocated; k >= 2^w,
//                                   mismatched counts and contexts throw; an empty batch is empty
//   uint_add_where_driver forms     "<shape> -> <route>": the route the classes take (addWhereRoute) under the
//                                   process's knobs
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

const char *kKnob = "uint_add_where_form";

uint64_t maskOf(unsigned w) { return w == 64 ? ~0ull : (1ull << w) - 1; }

std::vector<uint64_t> bits(const SecretKey &key, const CiphertextBatch &x)
{
    const std::vector<unsigned char> d = x.decrypt(key);
    return std::vector<uint64_t>(d.begin(), d.end());
}

// The definition, composed from the CiphertextBatch operators in the order of include/csgn_hip.h's table.
std::vector<CiphertextBatch> compose(const CiphertextBatch &s, const UIntBatch &a, uint64_t k, CiphertextBatch *carry)
{
    std::vector<CiphertextBatch> out;
    if (k == 0) {
        for (unsigned j = 0; j < a.width(); ++j)
            out.push_back(a.plane(j));
        if (carry)
            *carry = constantBatch(a.context(), std::vector<unsigned char>(a.size(), 0));
        return out;
    }
    const unsigned m = (unsigned)__builtin_ctzll(k);
    CiphertextBatch c = s;
    for (unsigned j = 0; j < a.width(); ++j) {
        const CiphertextBatch &aj = a.plane(j);
        if (j < m) {
            out.push_back(aj);
        } else if (j == m) {
            out.push_back(aj + s);
            c = aj * s;
        } else if ((k >> j) & 1u) {
            const CiphertextBatch ab = aj + s;
            out.push_back(ab + c);
            c = (aj * s) + (ab * c);
        } else {
            out.push_back(aj + c);
            c = aj * c;
        }
    }
    if (carry)
        *carry = c;
    return out;
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

// addWhere(mask, a, k) under the process's knob, forced to the loop and forced to the call: the same words, those of
// the definition; decryptions against the plaintext
void checkAdd(const SecretKey &key, const CiphertextBatch &mask, const UIntBatch &a, uint64_t k, const std::vector<uint64_t> *A,
              const std::vector<uint64_t> *S, const std::string &tag)
{
    const unsigned w = a.width();
    CiphertextBatch wc = mask, c0 = mask, c1 = mask, c2 = mask;
    const std::vector<CiphertextBatch> want = compose(mask, a, k, &wc);
    int form0 = -1;
    csgn_get_tuning(kKnob, &form0);
    const UIntBatch r0 = addWhere(mask, a, k, &c0);
    csgn_set_tuning(kKnob, 0);
    const UIntBatch r1 = addWhere(mask, a, k, &c1);
    csgn_set_tuning(kKnob, 1);
    const UIntBatch r2 = addWhere(mask, a, k, &c2);
    csgn_set_tuning(kKnob, form0);
    expect(samePlanes(r0, want) && sameBatchWords(c0, wc), "addWhere == the definition" + tag);
    expect(samePlanes(r1, want) && sameBatchWords(c1, wc), "the loop == the definition" + tag);
    expect(samePlanes(r2, want) && sameBatchWords(c2, wc), "the call == the definition" + tag);
    expect(samePlanes(addWhere(mask, a, k), want), "a null carry" + tag);
    if (A) {
        std::vector<uint64_t> v, c;
        for (size_t i = 0; i < A->size(); ++i) {
            const unsigned __int128 sum = (unsigned __int128)(*A)[i] + ((*S)[i] ? k : 0);
            v.push_back((uint64_t)sum & maskOf(w));
            c.push_back((uint64_t)(sum >> w));
        }
        checkValues(r0.decrypt(key), v, "addWhere" + tag);
        checkValues(bits(key, c0), c, "the carry of addWhere" + tag);
    }
}

struct Drawn {
    std::vector<uint64_t> a, s;
};

Drawn draw(unsigned w, size_t count)
{
    Drawn d;
    for (size_t i = 0; i < count; ++i) {
        d.a.push_back(i == 0 ? maskOf(w) : i == 1 ? maskOf(w) - 1 : rnd(w));      // the carry leaves, and does not
        d.s.push_back(i < 2 ? 1 : (uint64_t)(rand() & 1));
    }
    return d;
}

CiphertextBatch encryptBits(const SecretKey &key, const std::vector<uint64_t> &s)
{
    return CiphertextBatch::encrypt(key, std::vector<unsigned char>(s.begin(), s.end()));
}

int words()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const struct {
        unsigned w;
        size_t count;
        uint64_t ks[3];
    } cases[] = {{8, 60, {0xA5, 0x80, 0}}, {32, 24, {0x80000001ull, 0x10, 0}}, {40, 10, {0x8000000001ull, 5, 0}}};
    for (const auto &c : cases) {
        const Drawn d = draw(c.w, c.count);
        const UIntBatch a = UIntBatch::encrypt(key, d.a, c.w, 70 + c.w);
        const CiphertextBatch mask = encryptBits(key, d.s);
        const std::string tag = " w=" + std::to_string(c.w);
        expect(std::string(addWhereRoute(c.w, true)) == (c.w <= 32 ? "call" : "loop") || getenv("CSGN_UINT_ADD_WHERE_FORM"),
               "the route by shape" + tag);
        for (uint64_t k : c.ks)
            checkAdd(key, mask, a, k, &d.a, &d.s, tag + " k=" + std::to_string(k));
        // the derived operations
        CiphertextBatch ci = mask, cw = mask;
        const UIntBatch inc = incrementWhere(mask, a, &ci);
        expect(samePlanes(inc, compose(mask, a, 1, &cw)) && sameBatchWords(ci, cw), "incrementWhere == k = 1" + tag);
        const uint64_t ksub = maskOf(c.w) - 4;                   // a - (s ? 2^w - 5 : 0) = a + (s ? 5 : 0)
        const UIntBatch sub = subWhere(mask, a, ksub);
        expect(samePlanes(sub, compose(mask, a, 5, nullptr)), "subWhere == addWhere of the two's complement" + tag);
        expect(samePlanes(subWhere(mask, a, 0), compose(mask, a, 0, nullptr)), "subWhere of 0" + tag);
        std::vector<uint64_t> vi, vs, vc;
        for (size_t i = 0; i < c.count; ++i) {
            vi.push_back((d.a[i] + d.s[i]) & maskOf(c.w));
            vc.push_back(d.s[i] && d.a[i] == maskOf(c.w));
            vs.push_back((d.a[i] - (d.s[i] ? ksub : 0)) & maskOf(c.w));
        }
        checkValues(inc.decrypt(key), vi, "incrementWhere" + tag);
        checkValues(bits(key, ci), vc, "the carry of incrementWhere" + tag);
        checkValues(sub.decrypt(key), vs, "subWhere" + tag);
        // a second increment: the planes are no longer fresh (two terms each); 2^8 terms at the top of 8 bits
        if (c.w == 8) {
            checkAdd(key, mask, inc, 1, &vi, &d.s, tag + " incremented twice");
            const UIntBatch dec = decrementWhere(mask, a);
            expect(samePlanes(dec, compose(mask, a, 0xFF, nullptr)), "decrementWhere == k = 2^w - 1" + tag);
            const UIntBatch sub1 = subWhere(mask, a, 1);
            expect(sameWords(sub1, dec), "subWhere of 1 == decrementWhere" + tag);
            std::vector<uint64_t> vd;
            for (size_t i = 0; i < c.count; ++i)
                vd.push_back((d.a[i] - d.s[i]) & 0xFF);
            checkValues(dec.decrypt(key), vd, "decrementWhere" + tag);
            // what a user writes today: a + keepWhere(mask, constant); different words, the same values
            for (uint64_t k : {(uint64_t)0xA5, (uint64_t)1}) {
                const UIntBatch today = a + keepWhere(mask, UIntBatch::constant(ctx, std::vector<uint64_t>(c.count, k), 8));
                checkValues(addWhere(mask, a, k).decrypt(key), today.decrypt(key), "addWhere against a + keepWhere" + tag);
            }
        }
        // k = 0: the source payloads themselves
        const UIntBatch same = addWhere(mask, a, 0);
        bool shared = true;
        for (unsigned j = 0; j < c.w; ++j)
            shared = shared && same.plane(j).deviceValues() == a.plane(j).deviceValues();
        expect(shared, "k = 0 returns the source payloads" + tag);
    }
    // the per-shape rule (no operation runs): a fresh 32-bit increment of 256 MiB of outputs or more stays on the loop
    // unless the knob forces the call; a second set bit, a smaller batch or a flag of two terms take the call
    {
        int form = -1;
        csgn_get_tuning(kKnob, &form);
        const size_t big = 26000;                            // 65 terms of 160 bytes an element: 270 MB
        const UIntBatch ab = UIntBatch::encrypt(key, std::vector<uint64_t>(big, 7), 32, 90);
        const CiphertextBatch mb = ab.plane(3);
        const std::string call = form == 0 ? "loop" : "call";
        expect(std::string(addWhereRoute(mb, ab, 1)) == (form == 1 ? "call" : "loop"), "a large fresh increment: the loop");
        expect(std::string(addWhereRoute(mb, ab, 0x10000)) == (form == 1 ? "call" : "loop"), "one set bit, 16 planes above it");
        expect(std::string(addWhereRoute(mb, ab, 0x20000)) == call, "one set bit, 15 planes above it: the call");
        expect(std::string(addWhereRoute(mb, ab, 3)) == call, "two set bits: the call");
        expect(std::string(addWhereRoute(mb + mb, ab, 1)) == call, "a flag of two terms: the call");
        expect(std::string(addWhereRoute(mb.slice(0, 25000), ab.slice(0, 25000), 1)) == call, "under 256 MiB: the call");
        expect(std::string(addWhereRoute(mb, ab, 0)) == "loop", "k = 0 launches nothing");
    }
    // the mask IS a plane of a
    const Drawn d = draw(5, 30);
    const UIntBatch a5 = UIntBatch::encrypt(key, d.a, 5, 50);
    std::vector<uint64_t> s0;
    for (size_t i = 0; i < d.a.size(); ++i)
        s0.push_back(d.a[i] & 1);
    checkAdd(key, a5.plane(0), a5, 0x13, &d.a, &s0, " the mask is plane 0");
    // multi-term planes and mask (sums with a trivial ZERO)
    const UIntBatch zero = UIntBatch::constant(ctx, std::vector<uint64_t>(30, 0), 5);
    const CiphertextBatch m5 = encryptBits(key, d.s);
    checkAdd(key, m5, a5 ^ zero, 0x15, &d.a, &d.s, " multi-term a");
    checkAdd(key, m5 + zero.plane(0), a5, 0x16, &d.a, &d.s, " multi-term mask");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    for (unsigned w = 1; w <= 5; ++w) {
        const Drawn d = draw(w, 60);
        const UIntBatch a0 = UIntBatch::encrypt(key, d.a, w, 50 + w);
        const CiphertextBatch m0 = encryptBits(key, d.s);
        // x + p + q, compacted: element 0 keeps [x, ONE, ZERO] (its bit flips), every other element adds ZERO twice,
        // which cancels: it holds exactly the uniform batch's term.  The result is ragged.
        std::vector<unsigned char> q0(60, 0), q1(60, 0);
        q0[0] = 1;
        auto raggedOf = [&](const CiphertextBatch &x) { return addPlain(addPlain(x, q0), q1).compact(); };
        std::vector<CiphertextBatch> pr;
        for (unsigned j = 0; j < w; ++j)
            pr.push_back(raggedOf(a0.plane(j)));
        const UIntBatch ar = UIntBatch::fromPlanes(pr);
        const CiphertextBatch mr = raggedOf(m0);
        const std::string tag = " w=" + std::to_string(w);
        expect(!ar.plane(0).uniform() && !mr.uniform(), "compact() gave ragged operands" + tag);
        expect(std::string(addWhereRoute(w, false)) == "loop", "a ragged operand takes the loop" + tag);
        std::vector<uint64_t> fa = d.a, fs = d.s;
        fa[0] ^= maskOf(w);                                  // element 0 of a ragged operand has every bit flipped
        fs[0] ^= 1;
        const uint64_t k = maskOf(w) & 0x15 ? maskOf(w) & 0x15 : 1;
        checkAdd(key, m0, ar, k, &fa, &d.s, " ragged a" + tag);
        checkAdd(key, mr, a0, k, &d.a, &fs, " ragged mask" + tag);
        checkAdd(key, mr, ar, maskOf(w), &fa, &fs, " both ragged" + tag);
    }
    return 0;
}

// A 32-bit decrement of fresh planes is 2^j + 1 terms at plane j; 3-term planes under k = 1 carry 3^(j+1) terms out of
// plane j, past 2^31 words from plane 17 of 32 on.
// The size check comes first, so the calls throw std::invalid_argument at once, before any allocation or launch.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 1000;
    std::vector<uint64_t> x(count);
    for (size_t i = 0; i < count; ++i)
        x[i] = rnd(32);
    const UIntBatch x0 = UIntBatch::encrypt(key, x, 32, 1);
    const CiphertextBatch mask = x0.plane(5);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < 32; ++j)
        planes.push_back((x0.plane(j) + x0.plane(j)) + x0.plane(j));
    const UIntBatch wide = UIntBatch::fromPlanes(planes);
    CiphertextBatch carry = x0.plane(0);
    const auto t0 = std::chrono::steady_clock::now();
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { decrementWhere(mask, x0); });
    thrown += throws<std::invalid_argument>([&] { subWhere(mask, x0, 1); });
    thrown += throws<std::invalid_argument>([&] { addWhere(mask, x0, 0xFFFFFFFFull, &carry); });
    thrown += throws<std::invalid_argument>([&] { incrementWhere(mask, wide, &carry); });
    thrown += throws<std::invalid_argument>([&] { addWhere(mask, wide, 1); });
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(thrown == 5, "oversize throws (" + std::to_string(thrown) + " of 5)");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    expect(carry.size() == count && carry.uniform() && carry.terms() == 1, "a refused call leaves the carry alone");
    // the constant, counts, contexts
    const UIntBatch a4 = UIntBatch::encrypt(key, std::vector<uint64_t>(10, 3), 4, 3);
    Context other(127, 8);
    SecretKey okey(other);
    const UIntBatch o4 = UIntBatch::encrypt(okey, std::vector<uint64_t>(10, 1), 4, 7);
    thrown = 0;
    thrown += throws<std::invalid_argument>([&] { addWhere(a4.plane(0), a4, 16); });                    // k >= 2^w
    thrown += throws<std::invalid_argument>([&] { subWhere(a4.plane(0), a4, 16); });
    thrown += throws<std::invalid_argument>([&] { addWhere(a4.plane(0).slice(0, 9), a4, 1); });         // counts
    thrown += throws<std::invalid_argument>([&] { incrementWhere(o4.plane(0), a4); });                  // contexts
    thrown += throws<std::invalid_argument>([&] { decrementWhere(a4.plane(0), o4); });
    expect(thrown == 5, "a bad constant, counts and contexts throw (" + std::to_string(thrown) + " of 5)");
    // an empty batch: empty planes
    const UIntBatch e4 = a4.slice(0, 0);
    const UIntBatch es = addWhere(e4.plane(0), e4, 5, &carry);
    expect(es.width() == 4 && es.size() == 0 && carry.size() == 0, "an empty batch gives empty planes and an empty carry");
    expect(decrementWhere(e4.plane(0), e4).size() == 0 && addWhere(e4.plane(0), e4, 0).size() == 0, "an empty batch gives empty results");
    return 0;
}

// No device work: the route of the classes for the shapes of words, under the knobs the process was started with.
int forms()
{
    const unsigned widths[] = {1, 8, 16, 17, 32, 33, 40, 64};
    for (unsigned w : widths)
        for (int uniform = 1; uniform >= 0; --uniform)
            printf("w=%u %s -> %s\n", w, uniform ? "uniform" : "ragged", addWhereRoute(w, uniform != 0));
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4735, "uint_add_where_driver",
                    {{"words", words}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
