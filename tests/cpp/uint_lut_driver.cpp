// uint_lut_driver.cpp -- user-style C++ over the public lookup tables of include/certfhe/UInt.h
// (tests/test_uint_lut_cpp.py builds and runs it).
//   uint_lut_driver sbox      the AES S-box over 1000 encrypted bytes: decryptions == the table, words == the
//                             definition composed from CiphertextBatch operators; a second batch reuses the compiled table
//   uint_lut_driver two       two-input lookups (4x4-bit multiply, min, max) by decryption
//   uint_lut_driver ragged    compacted (ragged) planes: elements holding the same terms as the uniform planes give the
//                             same words; every word == the definition; decryptions == the table
//   uint_lut_driver oversize  a lookup past 2^31 words per element throws before anything is allocated; bad tables throw
//   uint_lut_driver forms   "<shape> -> <form>": the form csgn_uint_lut_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

#include <chrono>
#include <stdexcept>

using namespace certFHE;

namespace {

std::vector<uint64_t> aesSbox()
{
    auto gmul = [](unsigned a, unsigned b) {
        unsigned r = 0;
        for (; b; b >>= 1) {
            if (b & 1)
                r ^= a;
            a = (a & 0x80) ? ((a << 1) ^ 0x11B) : a << 1;
        }
        return r;
    };
    std::vector<uint64_t> s(256);
    for (unsigned x = 0; x < 256; ++x) {
        unsigned inv = 0;
        for (unsigned b = 1; x && b < 256; ++b)
            if (gmul(x, b) == 1)
                inv = b;
        unsigned v = inv;
        for (int r = 1; r <= 4; ++r)
            v ^= ((inv << r) | (inv >> (8 - r))) & 0xFF;
        s[x] = v ^ 0x63;
    }
    return s;
}

// the definition of UInt.h, by hand from the batch operators
UIntBatch definition(const UIntBatch &a, const LookupTable &f)
{
    std::vector<CiphertextBatch> out;
    for (unsigned j = 0; j < f.outWidth(); ++j) {
        std::vector<CiphertextBatch> acc;
        for (uint64_t S = 0; S < f.anf().size(); ++S) {
            if (!((f.anf()[S] >> j) & 1u))
                continue;
            std::vector<CiphertextBatch> m;
            for (unsigned i = 0; i < f.inWidth(); ++i)
                if ((S >> i) & 1u) {
                    if (m.empty())
                        m.push_back(a.plane(i));
                    else
                        m[0] = m[0] * a.plane(i);
                }
            if (m.empty())
                m.push_back(constantBatch(a.context(), std::vector<unsigned char>(a.size(), 1)));
            if (acc.empty())
                acc.push_back(m[0]);
            else
                acc[0] = acc[0] + m[0];
        }
        out.push_back(acc.empty() ? constantBatch(a.context(), std::vector<unsigned char>(a.size(), 0)) : acc[0]);
    }
    return UIntBatch::fromPlanes(out);
}

int sbox()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const LookupTable f(aesSbox(), 8, 8);
    for (int round = 0; round < 2; ++round) {
        const size_t count = 1000;
        std::vector<uint64_t> v(count), want(count);
        for (size_t i = 0; i < count; ++i) {
            v[i] = i < 256 ? i : rnd(8);
            want[i] = f.table()[v[i]];
        }
        const UIntBatch a = UIntBatch::encrypt(key, v, 8, 11 + round);
        const UIntBatch r = lookup(a, f);
        expect(r.width() == 8, "sbox width");
        checkValues(r.decrypt(key), want, "sbox round " + std::to_string(round));
        if (round == 0) {
            const UIntBatch small = UIntBatch::encrypt(key, std::vector<uint64_t>(v.begin(), v.begin() + 40), 8, 5);
            expect(sameWords(lookup(small, f), definition(small, f)), "sbox words == definition");
        }
    }
    return 0;
}

int two()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    std::vector<uint64_t> mul(256), mn(256), mx(256);
    for (uint64_t x = 0; x < 256; ++x) {
        const uint64_t a = x & 15, b = x >> 4;
        mul[x] = a * b;
        mn[x] = a < b ? a : b;
        mx[x] = a < b ? b : a;
    }
    const size_t count = 500;
    std::vector<uint64_t> va(count), vb(count);
    for (size_t i = 0; i < count; ++i) {
        va[i] = i < 256 ? i & 15 : rnd(4);
        vb[i] = i < 256 ? i >> 4 : rnd(4);
    }
    const UIntBatch a = UIntBatch::encrypt(key, va, 4, 21), b = UIntBatch::encrypt(key, vb, 4, 22);
    const std::vector<uint64_t> *tables[] = {&mul, &mn, &mx};
    const unsigned outs[] = {8, 4, 4};
    const char *names[] = {"mul", "min", "max"};
    for (int t = 0; t < 3; ++t) {
        const LookupTable f(std::vector<uint64_t>(tables[t]->begin(), tables[t]->end()) , 8, outs[t]);
        std::vector<uint64_t> want(count);
        for (size_t i = 0; i < count; ++i)
            want[i] = (*tables[t])[va[i] + (vb[i] << 4)];
        checkValues(lookup(a, b, f).decrypt(key), want, names[t]);
    }
    bool caught = false;
    try {
        lookup(a, a, LookupTable(std::vector<uint64_t>(1 << 7, 0), 7, 1));
    } catch (const std::invalid_argument &) {
        caught = true;
    }
    expect(caught, "widths that do not add up throw");
    return 0;
}

int ragged()
{
    Context ctx(127, 8);
    SecretKey key(ctx);
    const size_t count = 200;
    for (unsigned w = 1; w <= 5; ++w) {
        std::vector<uint64_t> table(1u << w);
        for (auto &x : table)
            x = rnd(3);
        const LookupTable f(table, w, 3);
        std::vector<uint64_t> v(count);
        for (size_t i = 0; i < count; ++i)
            v[i] = rnd(w);
        const UIntBatch a0 = UIntBatch::encrypt(key, v, w, 40 + w);
        // plane j + x + y, compacted: element 0 keeps [a, ONE, ZERO] (its bit flips), every other element adds ZERO
        // twice, which cancels: it holds exactly the uniform plane's term.  The planes are ragged.
        std::vector<unsigned char> x(count, 0), y(count, 0);
        x[0] = 1;
        std::vector<CiphertextBatch> pr;
        for (unsigned j = 0; j < w; ++j)
            pr.push_back(addPlain(addPlain(a0.plane(j), x), y).compact());
        expect(!pr[0].uniform(), "compact() gave a ragged plane");
        const UIntBatch a = UIntBatch::fromPlanes(pr);
        std::vector<uint64_t> vr = v;
        vr[0] ^= (1ull << w) - 1;
        const UIntBatch u = lookup(a0, f), r = lookup(a, f);
        const std::string tag = " w=" + std::to_string(w);
        for (unsigned j = 0; j < 3; ++j) {
            bool same = true;
            for (uint64_t i = 1; i < count && same; ++i) {
                const Ciphertext ci = u.plane(j).at(i), ri = r.plane(j).at(i);
                same = ci.getLen() == ri.getLen() && memcmp(ci.getValues(), ri.getValues(), ci.getLen() * 8) == 0;
            }
            expect(same, "ragged words == uniform words" + tag);
        }
        expect(sameWords(r, definition(a, f)), "ragged words == definition" + tag);
        std::vector<uint64_t> want(count);
        for (size_t i = 0; i < count; ++i)
            want[i] = table[vr[i]];
        checkValues(r.decrypt(key), want, "ragged" + tag);
    }
    return 0;
}

// 16-bit values of 8 terms a plane at N=1247: x == 0 has every monomial, 9^16 terms per element.  The size check comes
// first, so the call throws std::invalid_argument at once, before any allocation or launch.
int oversize()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 1000;
    std::vector<uint64_t> v(count);
    for (size_t i = 0; i < count; ++i)
        v[i] = rnd(16);
    const UIntBatch a0 = UIntBatch::encrypt(key, v, 16, 1);
    std::vector<CiphertextBatch> planes;
    for (unsigned j = 0; j < 16; ++j) {
        CiphertextBatch p = a0.plane(j);
        for (int d = 0; d < 3; ++d)
            p = p + p;
        planes.push_back(p);
    }
    const UIntBatch a = UIntBatch::fromPlanes(planes);
    std::vector<uint64_t> table(1u << 16, 0);
    table[0] = 1;
    const LookupTable f(table, 16, 1);
    const auto t0 = std::chrono::steady_clock::now();
    bool caught = false;
    try {
        lookup(a, f);
    } catch (const std::invalid_argument &) {
        caught = true;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    expect(caught, "oversize throws");
    expect(s < 1.0, "the size check ran before any launch (" + std::to_string(s) + " s)");
    // bad tables
    const std::vector<uint64_t> three(3, 0), big(16, 16);
    int thrown = 0;
    try {
        LookupTable(three, 2, 1);
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    try {
        LookupTable(big, 4, 4);
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    try {
        LookupTable(std::vector<uint64_t>(1u << 17, 0), 17, 1);
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    try {
        lookup(a0, LookupTable(std::vector<uint64_t>(16, 0), 4, 1));
    } catch (const std::invalid_argument &) {
        ++thrown;
    }
    expect(thrown == 4, "bad tables and widths throw (" + std::to_string(thrown) + " of 4)");
    return 0;
}

// The form csgn_uint_lut_kernel names for the table and shapes of sbox (fresh planes, 1000 and 40 elements), under the
// knob the process was started with.  A compiled table is uploaded when it is made: this mode needs the device.
int forms()
{
    const std::vector<uint64_t> table = aesSbox(), terms(8, 1);
    csgn_uint_lut *lut = nullptr;
    expect(csgn_uint_lut_create(8, 8, table.data(), terms.data(), &lut) == CSGN_OK && lut, "the table compiles");
    if (!lut)
        return 0;
    for (uint64_t count : {(uint64_t)1000, (uint64_t)40}) {
        const char *form = csgn_uint_lut_kernel(1247, lut, count);
        expect(form && *form, "the lookup has a form");
        printf("sbox count=%llu -> %s\n", (unsigned long long)count, form ? form : "");
    }
    csgn_uint_lut_destroy(lut);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 4711, "uint_lut_driver",
                    {{"sbox", sbox}, {"two", two}, {"ragged", ragged}, {"oversize", oversize}, {"forms", forms}});
}
