// uint_decrypt_driver.cpp -- user-style C++ over the two ends of include/certfhe/UInt.h: UIntBatch::encrypt (one block, one
// launch, planes that are views), UIntBatch::decrypt and decryptPacked (one csgn_uint_decrypt), decryptRoute
// (tests/test_uint_decrypt_cpp.py builds and runs it, with CSGN_UINT_DECRYPT_FORM unset, at 0 and at 1).
//   uint_decrypt_driver roundtrip   encrypt (both overloads) then decrypt at widths 1, 8 and 64, counts 1, 2 and 37,
//                                   N=1247 and N=1300; "route -> <decryptRoute>" for every shape
//   uint_decrypt_driver seeded      the seeded planes == CiphertextBatch::encrypt(key, bits_j, seed, j * count), word for word
//   uint_decrypt_driver arith       (a + b).decrypt, a.add(b, &carry) with decryptPacked of the planes and the carry,
//                                   (a + b).compact().decrypt on ragged planes, a ragged plane past the call's bound
//   uint_decrypt_driver lifetime    a plane view outlives its UIntBatch
//   uint_decrypt_driver refusals    decryptPacked refuses 0 planes, 65 planes, planes of different counts or contexts
#include "driver.h"

#include "csgn_hip.h"

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

std::vector<unsigned char> bitsOf(const std::vector<uint64_t> &v, unsigned j)
{
    std::vector<unsigned char> b(v.size());
    for (size_t i = 0; i < v.size(); ++i)
        b[i] = (unsigned char)((v[i] >> j) & 1u);
    return b;
}

// the route the process's knob asks for where nothing else decides
const char *knobRoute()
{
    int form = -1;
    csgn_get_tuning("uint_decrypt_form", &form);
    return form == 0 ? "planes" : "call";
}

const unsigned kWidths[] = {1, 8, 64};
const size_t kCounts[] = {1, 2, 37};

int roundtrip()
{
    const int contexts[2][2] = {{1247, 16}, {1300, 4}};
    for (int c = 0; c < 2; ++c) {
        Context ctx(contexts[c][0], contexts[c][1]);
        SecretKey key(ctx);
        for (unsigned w : kWidths)
            for (size_t count : kCounts) {
                const std::string tag = " N=" + std::to_string(contexts[c][0]) + " w=" + std::to_string(w) + " count=" +
                                        std::to_string(count);
                const std::vector<uint64_t> v = draw(w, count);
                const UIntBatch seeded = UIntBatch::encrypt(key, v, w, 900 + w);
                const UIntBatch fresh = UIntBatch::encrypt(key, v, w);
                expect(seeded.width() == w && seeded.size() == count && fresh.width() == w && fresh.size() == count,
                       "shape" + tag);
                checkValues(seeded.decrypt(key), v, "seeded encrypt then decrypt" + tag);
                checkValues(fresh.decrypt(key), v, "encrypt then decrypt" + tag);
                std::vector<CiphertextBatch> planes;
                for (unsigned j = 0; j < w; ++j)
                    planes.push_back(fresh.plane(j));
                checkValues(decryptPacked(planes, key), v, "decryptPacked of the planes" + tag);
                expect(std::string(decryptRoute(fresh)) == knobRoute(), "fresh planes take the knob's route" + tag);
                printf("N=%d w=%u count=%zu route -> %s\n", contexts[c][0], w, count, decryptRoute(fresh));
            }
        // an empty batch: empty planes, an empty vector
        const UIntBatch none = UIntBatch::encrypt(key, std::vector<uint64_t>(), 5, 3);
        expect(none.width() == 5 && none.size() == 0 && none.decrypt(key).empty(), "an empty batch");
        expect(UIntBatch::encrypt(key, std::vector<uint64_t>(), 5).decrypt(key).empty(), "an empty batch, unseeded");
    }
    return 0;
}

int seeded()
{
    const int contexts[2][2] = {{1247, 16}, {1300, 4}};
    for (int c = 0; c < 2; ++c) {
        Context ctx(contexts[c][0], contexts[c][1]);
        SecretKey key(ctx);
        for (unsigned w : kWidths)
            for (size_t count : kCounts) {
                const std::vector<uint64_t> v = draw(w, count);
                const uint64_t seed = 77 + w + count;
                const UIntBatch a = UIntBatch::encrypt(key, v, w, seed);
                for (unsigned j = 0; j < w; ++j)
                    expect(sameBatchWords(a.plane(j), CiphertextBatch::encrypt(key, bitsOf(v, j), seed, (uint64_t)j * count)),
                           "plane " + std::to_string(j) + " == the per-plane seeded encrypt, N=" +
                               std::to_string(contexts[c][0]) + " w=" + std::to_string(w) + " count=" + std::to_string(count));
                // the same seed gives the same words; the unseeded form does not repeat them
                expect(sameWords(a, UIntBatch::encrypt(key, v, w, seed)), "the seeded form repeats");
                if (w == 8 && count == 37)
                    expect(!sameWords(UIntBatch::encrypt(key, v, w), UIntBatch::encrypt(key, v, w)),
                           "the unseeded form draws fresh randomness for every call");
            }
    }
    return 0;
}

int arith()
{
    const int contexts[2][2] = {{1247, 16}, {127, 8}};
    for (int c = 0; c < 2; ++c) {
        Context ctx(contexts[c][0], contexts[c][1]);
        SecretKey key(ctx);
        for (unsigned w : {1u, 4u, 8u}) {
            const size_t count = 37, same = 11;
            const std::string tag = " N=" + std::to_string(contexts[c][0]) + " w=" + std::to_string(w);
            const std::vector<uint64_t> av = draw(w, count), bv = draw(w, count);
            const uint64_t mask = (1ull << w) - 1;
            std::vector<uint64_t> sum(count), wide(count);
            for (size_t i = 0; i < count; ++i)
                sum[i] = (av[i] + bv[i]) & mask, wide[i] = av[i] + bv[i];
            const UIntBatch a = UIntBatch::encrypt(key, av, w, 30 + w), b = UIntBatch::encrypt(key, bv, w, 40 + w);
            const UIntBatch s = a + b;
            checkValues(s.decrypt(key), sum, "(a + b).decrypt" + tag);
            expect(std::string(decryptRoute(s)) == knobRoute(), "a sum's planes take the knob's route" + tag);
            CiphertextBatch carry = a.plane(0);
            const UIntBatch sc = a.add(b, &carry);
            std::vector<CiphertextBatch> planes;
            for (unsigned j = 0; j < w; ++j)
                planes.push_back(sc.plane(j));
            planes.push_back(carry);
            checkValues(decryptPacked(planes, key), wide, "decryptPacked of the sum's planes and the carry" + tag);
            // ragged planes: where b is a itself the terms of a + b cancel in pairs, elsewhere nothing does
            const UIntBatch mixed = UIntBatch::concat({a.slice(0, same), b.slice(same, count)});
            const UIntBatch r = (a + mixed).compact();
            expect(!r.plane(0).uniform(), "compact() gave ragged planes" + tag);
            std::vector<uint64_t> want(count);
            for (size_t i = 0; i < count; ++i)
                want[i] = (av[i] + (i < same ? av[i] : bv[i])) & mask;
            checkValues(r.decrypt(key), want, "(a + b).compact().decrypt" + tag);
            expect(std::string(decryptRoute(r)) == knobRoute(), "short ragged planes take the knob's route" + tag);
            printf("N=%d w=%u sum route -> %s\n", contexts[c][0], w, decryptRoute(s));
        }
    }
    // a ragged plane with an element of more than 4096 terms: plane by plane whatever the knob says
    Context ctx(127, 8);
    SecretKey key(ctx);
    const size_t big = 4097;
    std::vector<unsigned char> ones(big, 0);
    ones[5] = ones[4000] = ones[4096] = 1;                            // three hits: 1
    const CiphertextBatch longOne = CiphertextBatch::encrypt(key, ones, 5).sumGroups(big);
    const CiphertextBatch shortOne = CiphertextBatch::encrypt(key, std::vector<unsigned char>(1, 0), 6);
    const CiphertextBatch raggedLong = CiphertextBatch::concat({longOne, shortOne, longOne});
    expect(!raggedLong.uniform(), "concat of unlike parts is ragged");
    const UIntBatch u = UIntBatch::fromPlanes({raggedLong, CiphertextBatch::encrypt(key, {1, 1, 0}, 7)});
    expect(std::string(decryptRoute(u)) == "planes", "a ragged plane past 4096 terms takes the planes");
    checkValues(u.decrypt(key), {3, 2, 1}, "a ragged plane past 4096 terms");
    printf("ragged 4097 route -> %s\n", decryptRoute(u));
    return 0;
}

int lifetime()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t count = 37;
    const std::vector<uint64_t> v = draw(8, count);
    CiphertextBatch kept = UIntBatch::encrypt(key, v, 8, 12).plane(3);           // the UIntBatch is gone at the ';'
    // blocks come and go: a freed block of the integer would be handed out again here
    for (int k = 0; k < 4; ++k) {
        std::vector<uint64_t> x = draw(8, count);
        const UIntBatch other = UIntBatch::encrypt(key, x, 8, 100 + k);
        for (size_t i = 0; i < count; ++i)
            x[i] = (2 * x[i]) & 255u;
        checkValues((other + other).decrypt(key), x, "x + x while the view waits");
    }
    const std::vector<unsigned char> want = bitsOf(v, 3), got = kept.decrypt(key);
    expect(got == want, "a plane view outlives its UIntBatch: it still decrypts to its bits");
    expect(sameBatchWords(kept, CiphertextBatch::encrypt(key, want, 12, 3 * count)), "... and still holds its words");
    checkValues(decryptPacked({kept}, key), std::vector<uint64_t>(want.begin(), want.end()), "decryptPacked of one view");
    return 0;
}

int refusals()
{
    Context ctx(1247, 16), other(127, 8);
    SecretKey key(ctx), okey(other);
    const CiphertextBatch p = CiphertextBatch::encrypt(key, randomBits(10), 1);
    int thrown = 0;
    thrown += throws<std::invalid_argument>([&] { decryptPacked(std::vector<CiphertextBatch>(), key); });
    thrown += throws<std::invalid_argument>([&] { decryptPacked(std::vector<CiphertextBatch>(65, p), key); });
    thrown += throws<std::invalid_argument>([&] { decryptPacked({p, p.slice(0, 9)}, key); });
    thrown += throws<std::invalid_argument>([&] { decryptPacked({p, CiphertextBatch::encrypt(okey, randomBits(10), 2)}, key); });
    expect(thrown == 4, "decryptPacked refuses 0 planes, 65 planes, other counts and contexts (" + std::to_string(thrown) + " of 4)");
    const std::vector<uint64_t> all = decryptPacked(std::vector<CiphertextBatch>(64, p), key);
    const std::vector<unsigned char> bit = p.decrypt(key);
    for (size_t i = 0; i < all.size(); ++i)
        expect(all[i] == (bit[i] ? ~0ull : 0ull), "64 planes fill the word");
    expect(decryptPacked({p.slice(0, 0)}, key).empty(), "an empty batch gives an empty vector");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 5150, "uint_decrypt_driver",
                    {{"roundtrip", roundtrip}, {"seeded", seeded}, {"arith", arith}, {"lifetime", lifetime},
                     {"refusals", refusals}});
}
