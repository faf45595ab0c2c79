// dropin_driver.cpp -- exercises the drop-in certFHE:: C++ API (include/certfhe/, libcertFHE.so)
// the way user code of the reference does.  pytest (tests/test_dropin_cpp.py) builds it, runs
// the sub-commands and compares the printed words with the oracle / the golden vectors.
//
//   dropin_driver basic [rounds]          tests/basic_operations.cpp flow, asserted
//   dropin_driver permutations [rounds]   tests/permutations.cpp flow, asserted
//   dropin_driver timings                 tests/timings.cpp flow (sizes asserted, times printed)
//   dropin_driver encrypt N D seed nbits b0 b1 .. key0 key1 ..   deterministic fresh ciphertexts
//   dropin_driver circuit N D seed        deterministic add/mul chain, prints every stage
//   dropin_driver bitlen                  non-canonical Bitlen propagation (left-operand rule)
//   dropin_driver api                     copy/assign/in-place operator semantics, printing
#include <atomic>
#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <algorithm>
#include <sstream>
#include <stdexcept>
#include <streambuf>
#include <vector>

#include "certFHE.h"
#include <thread>
#include "csgn_hip.h"      // wirebench only: csgn_stream_sync

using namespace certFHE;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "EXPECT failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
            exit(2);                                                                  \
        }                                                                             \
    } while (0)

static void dump(const char *label, const Ciphertext &c)
{
    printf("%s len=%llu v=", label, (unsigned long long)c.getLen());
    uint64_t *v = c.getValues();
    for (uint64_t i = 0; i < c.getLen(); ++i)
        printf("%016llx", (unsigned long long)v[i]);
    printf("\n");
}

static int cmd_basic(int rounds)
{
    Library::initializeLibrary();
    for (int r = 0; r < rounds; ++r) {
        Context context(1247, 16);
        SecretKey seckey(context);
        Plaintext p1(1), p0(0);
        Ciphertext c1 = seckey.encrypt(p1);
        Ciphertext c0 = seckey.encrypt(p0);
        Ciphertext added, multiplied;          // default-constructed, then assigned
        added = c1 + c0;
        multiplied = c1 * c0;
        EXPECT(added.getLen() == 40 && multiplied.getLen() == 20);
        Plaintext da = seckey.decrypt(added), dm = seckey.decrypt(multiplied);
        EXPECT(da.getValue() == 1);
        EXPECT(dm.getValue() == 0);
        // the assigned objects stay usable as operands (the reference segfaults here)
        Ciphertext again = added * multiplied;
        EXPECT(again.getLen() == 40);
        EXPECT(seckey.decrypt(again).getValue() == 0);
        Ciphertext one_one = c1 * c1;
        EXPECT(seckey.decrypt(one_one).getValue() == 1);
        Ciphertext xor11 = c1 + c1;
        EXPECT(seckey.decrypt(xor11).getValue() == 0);
    }
    std::cout << "Dec ( Enc (1) + Enc (0) ) = " << Plaintext(1);
    std::cout << "Dec ( Enc (1) * Enc (0) ) = " << Plaintext(0);
    printf("basic ok rounds=%d\n", rounds);
    return 0;
}

static int cmd_permutations(int rounds)
{
    Library::initializeLibrary();
    for (int r = 0; r < rounds; ++r) {
        Context context(1247, 16);
        SecretKey seckey(context);
        for (int bit = 0; bit < 2; ++bit) {
            Plaintext p(bit);
            Ciphertext c = seckey.encrypt(p);
            Permutation permutation(context);
            SecretKey permutedKey = seckey.applyPermutation(permutation);
            Ciphertext permuted = c.applyPermutation(permutation);
            EXPECT(permuted.getLen() == 20);
            EXPECT(permutedKey.decrypt(permuted).getValue() == bit);
            Permutation inverse = permutation.getInverse();
            Permutation identity;
            identity = permutation + inverse;
            EXPECT(identity.getLength() == 1247);
            for (uint64_t i = 0; i < 1247; ++i)
                EXPECT(identity.getPermutation()[i] == i);
            // undoing the permutation brings ciphertext and key back
            Ciphertext back = permuted.applyPermutation(inverse);
            uint64_t *a = back.getValues(), *b = c.getValues();
            for (int i = 0; i < 20; ++i)
                EXPECT(a[i] == b[i]);
            // multi-term input collapses to the permuted first term, as in the reference
            Ciphertext two = c + c;
            Ciphertext two_p = two.applyPermutation(permutation);
            EXPECT(two_p.getLen() == 20);
            uint64_t *x = two_p.getValues(), *y = permuted.getValues();
            for (int i = 0; i < 20; ++i)
                EXPECT(x[i] == y[i]);
            Permutation shorter(10);
            EXPECT((permutation + shorter).getLength() == 0);
        }
    }
    printf("permutations ok rounds=%d\n", rounds);
    return 0;
}

static int cmd_timings()
{
    Library::initializeLibrary();
    Context context(1247, 16);
    std::cout << context;
    Timer t1("Key generation ");
    t1.start();
    SecretKey seckey(context);
    t1.stopAndPrint();
    Plaintext p1(1);
    Timer t2("Encryption ");
    t2.start();
    Ciphertext c1 = seckey.encrypt(p1);
    t2.stopAndPrint();
    Ciphertext added, multiplicated;
    Timer t3("Addition of fresh ciphertexts");
    t3.start();
    added = c1 + c1;
    t3.stopAndPrint();
    Timer t4("Multiplication of fresh ciphertexts");
    t4.start();
    multiplicated = c1 * c1;
    t4.stopAndPrint();
    Timer t5("Permutation generation ");
    t5.start();
    Permutation permutation(context);
    t5.stopAndPrint();
    Timer t6("Permuting the secret key ");
    t6.start();
    SecretKey permutedSecretKey = seckey.applyPermutation(permutation);
    t6.stopAndPrint();
    Timer t7("Permuting the ciphertext ");
    t7.start();
    Ciphertext permutedCiphertext = c1.applyPermutation(permutation);
    t7.stopAndPrint();
    Timer t8("Decryption ");
    t8.start();
    Plaintext decrypted = permutedSecretKey.decrypt(permutedCiphertext);
    t8.stopAndPrint();
    EXPECT(decrypted.getValue() == 1);
    // the sizes the reference prints (tests/timings.cpp:69-72): 144 / 352 / 352 / 672 bytes
    printf("sizes %ld %ld %ld %ld\n", seckey.size(), c1.size(), multiplicated.size(), added.size());
    EXPECT(seckey.size() == 144 && c1.size() == 352 && multiplicated.size() == 352 && added.size() == 672);
    return 0;
}

static int cmd_encrypt(int argc, char **argv)
{
    // encrypt N D seed nbits b.. key..
    if (argc < 6)
        return 64;
    uint64_t n = strtoull(argv[2], 0, 10), d = strtoull(argv[3], 0, 10);
    unsigned seed = (unsigned)strtoul(argv[4], 0, 10);
    int nbits = atoi(argv[5]);
    if (argc != 6 + nbits + (int)d)
        return 64;
    std::vector<uint64_t> key(d);
    for (uint64_t i = 0; i < d; ++i)
        key[i] = strtoull(argv[6 + nbits + i], 0, 10);
    Context ctx(n, d);
    SecretKey sk(ctx);
    sk.setKey(key.data(), d);
    srand(seed);                                   // SURVEY 5.1 determinism recipe
    for (int i = 0; i < nbits; ++i) {
        Plaintext p(atoi(argv[6 + i]));
        Ciphertext c = sk.encrypt(p);
        dump("ct", c);
        printf("dec %d\n", (int)sk.decrypt(c).getValue());
        uint64_t *bl = c.getBitlen();
        printf("bitlen");
        for (uint64_t w = 0; w < c.getLen(); ++w)
            printf(" %llu", (unsigned long long)bl[w]);
        printf("\n");
    }
    return 0;
}

static int cmd_circuit(int argc, char **argv)
{
    if (argc < 5)
        return 64;
    uint64_t n = strtoull(argv[2], 0, 10), d = strtoull(argv[3], 0, 10);
    unsigned seed = (unsigned)strtoul(argv[4], 0, 10);
    Context ctx(n, d);
    SecretKey sk(ctx);
    std::vector<uint64_t> key(d);
    for (uint64_t i = 0; i < d; ++i)
        key[i] = (i * 37 + 11) % n;                 // fixed, distinct for d < n/37
    sk.setKey(key.data(), d);
    srand(seed);
    int bits[12] = {1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1};
    std::vector<Ciphertext> ct;
    for (int i = 0; i < 12; ++i) {
        Plaintext p(bits[i]);
        ct.push_back(sk.encrypt(p));
        dump("fresh", ct.back());
    }
    Ciphertext x = ct[0];
    int xb = bits[0];
    int k = 1;
    for (int level = 1; level <= 6; ++level) {
        if (level % 2) {
            x += ct[k];
            xb ^= bits[k];
            k += 1;
        } else {
            Ciphertext rhs = ct[k] + ct[k + 1];
            x *= rhs;
            xb &= (bits[k] ^ bits[k + 1]);
            k += 2;
        }
        dump("stage", x);
        int got = sk.decrypt(x).getValue();
        printf("stage_dec %d expect %d terms %llu\n", got, xb, (unsigned long long)x.getTerms());
        EXPECT(got == xb);
    }
    return 0;
}

static int cmd_bitlen()
{
    // operands with made-up Bitlen arrays: the product takes the LEFT operand's per-term
    // pattern (src/Ciphertext.cpp:165-176), the sum concatenates (:215-223)
    Context ctx(65, 4);
    const uint64_t dl = 2;
    uint64_t a[3 * dl], b[2 * dl], bla[3 * dl], blb[2 * dl];
    for (uint64_t i = 0; i < 3 * dl; ++i) {
        a[i] = 0xF0F0F0F0F0F0F0F0ull ^ (i * 0x0123456789ABCDEFull);
        bla[i] = 1 + i;
    }
    for (uint64_t i = 0; i < 2 * dl; ++i) {
        b[i] = 0xFFFF0000FFFF0000ull ^ (i * 0x1111111111111111ull);
        blb[i] = 40 + i;
    }
    Ciphertext A(a, bla, 3 * dl, ctx), B(b, blb, 2 * dl, ctx);
    EXPECT(!A.hasCanonicalBitlen());
    Ciphertext P = A * B, S = A + B;
    EXPECT(P.getLen() == 12 && S.getLen() == 10);
    uint64_t *pv = P.getValues(), *pb = P.getBitlen(), *sb = S.getBitlen(), *sv = S.getValues();
    for (uint64_t i = 0; i < 3; ++i)
        for (uint64_t j = 0; j < 2; ++j)
            for (uint64_t k = 0; k < dl; ++k) {
                EXPECT(pv[(i * 2 + j) * dl + k] == (a[i * dl + k] & b[j * dl + k]));
                EXPECT(pb[(i * 2 + j) * dl + k] == bla[i * dl + k]);
            }
    for (uint64_t i = 0; i < 6; ++i)
        EXPECT(sv[i] == a[i] && sb[i] == bla[i]);
    for (uint64_t i = 0; i < 4; ++i)
        EXPECT(sv[6 + i] == b[i] && sb[6 + i] == blb[i]);
    // canonical left operand => canonical product even if the right one is custom
    uint64_t can[2 * dl] = {64, 1, 64, 1};
    Ciphertext C(b, can, 2 * dl, ctx);
    EXPECT(C.hasCanonicalBitlen());
    Ciphertext Q = C * A;
    EXPECT(Q.hasCanonicalBitlen());
    // decrypt / permute of a custom-Bitlen ciphertext: the reference reads (v, bitlen) as a bit
    // stream (src/SecretKey.cpp:110-140, src/Ciphertext.cpp:16-69); checked against that rule
    // evaluated here on the host
    SecretKey sk(ctx);
    {
        uint64_t v[4 * dl], bl[4 * dl];
        for (uint64_t i = 0; i < 4 * dl; ++i) {
            v[i] = 0x9E3779B97F4A7C15ull * (i + 3) ^ 0x5555AAAA5555AAAAull;
            bl[i] = (i % 2) ? 3 : 64;                      // 67 bits per term: every position 65*k + s is inside
        }
        std::vector<unsigned char> stream;
        for (uint64_t i = 0; i < 4 * dl; ++i)
            for (uint64_t k = 0; k < bl[i]; ++k)
                stream.push_back((unsigned char)((v[i] >> (63 - k)) & 1));
        const uint64_t *key = sk.getKey();
        // plant the key into terms 0 and 2 so that the answer is not trivially 0
        for (uint64_t k = 0; k < 4; k += 2)
            for (uint64_t i = 0; i < 4; ++i)
                stream[65 * k + key[i]] = 1;
        // re-pack the stream into v
        uint64_t at = 0;
        for (uint64_t i = 0; i < 4 * dl; ++i) {
            v[i] = 0;
            for (uint64_t k = 0; k < bl[i]; ++k, ++at)
                v[i] |= (uint64_t)stream[at] << (63 - k);
        }
        unsigned want = 0;
        for (uint64_t k = 0; k < 4; ++k) {
            unsigned dec = 1;
            for (uint64_t i = 0; i < 4; ++i)
                dec &= stream[65 * k + key[i]];
            want ^= dec;
        }
        Ciphertext X(v, bl, 4 * dl, ctx);
        EXPECT(!X.hasCanonicalBitlen());
        Plaintext got = sk.decrypt(X);
        EXPECT((unsigned)got.getValue() == want);
        Permutation pi(ctx);
        Ciphertext Y = X.applyPermutation(pi);
        EXPECT(Y.getLen() == dl && Y.hasCanonicalBitlen());
        const uint64_t *pp = pi.getPermutation(), *yv = Y.getValues();
        for (uint64_t j = 0; j < 65; ++j)
            EXPECT(((yv[j / 64] >> (63 - j % 64)) & 1) == stream[pp[j]]);
        EXPECT((yv[1] & ~(1ull << 63)) == 0);
    }
    printf("bitlen ok\n");
    return 0;
}

static int cmd_api()
{
    Context ctx(1247, 16);
    EXPECT(ctx.getN() == 1247 && ctx.getD() == 16 && ctx.getS() == 38 && ctx.getDefaultN() == 20);
    Context c2(ctx);
    c2.setN(4096);
    EXPECT(c2.getDefaultN() == 64 && c2.getS() == 128);
    std::stringstream ss;
    ss << ctx;
    EXPECT(ss.str() == "N= 1247\nD= 16\nS= 38\n");
    ss.str("");
    ss << Plaintext(3) << Plaintext(0);
    EXPECT(ss.str() == "1\n0\n");
    EXPECT(Plaintext(2).getValue() == 0);

    SecretKey sk(ctx);
    EXPECT(sk.getLength() == 16);
    for (int i = 0; i < 16; ++i) {
        EXPECT(sk.getKey()[i] < 1247);
        for (int j = 0; j < i; ++j)
            EXPECT(sk.getKey()[i] != sk.getKey()[j]);
    }
    SecretKey copy(sk), assigned(ctx);
    assigned = sk;
    for (int i = 0; i < 16; ++i)
        EXPECT(copy.getKey()[i] == sk.getKey()[i] && assigned.getKey()[i] == sk.getKey()[i]);
    ss.str("");
    ss << sk;
    EXPECT(!ss.str().empty() && ss.str()[ss.str().size() - 1] == '\n');

    Plaintext one(1), zero(0);
    Ciphertext a = sk.encrypt(one), b = sk.encrypt(zero);
    Ciphertext a_copy(a);
    a += b;                                            // a = a || b
    EXPECT(a.getLen() == 40 && a_copy.getLen() == 20);  // the copy is unaffected
    EXPECT(copy.decrypt(a).getValue() == 1);
    a *= a_copy;                                       // (1^0)&1
    EXPECT(a.getLen() == 40 && assigned.decrypt(a).getValue() == 1);
    // borrowed host mirror: same words as a fresh download, stable until the next mutation
    uint64_t *m1 = a.getValues();
    uint64_t *m2 = a.getValues();
    EXPECT(m1 == m2);
    // setValues / 4-arg ctor round trip (the de-facto wire format)
    Ciphertext wire(a.getValues(), a.getBitlen(), a.getLen(), a.getContext());
    EXPECT(wire.hasCanonicalBitlen() && sk.decrypt(wire).getValue() == 1);
    Ciphertext setter;
    setter.setContext(ctx);
    setter.setValues(b.getValues(), b.getLen());
    setter.setBitlen(b.getBitlen(), b.getLen());
    EXPECT(sk.decrypt(setter).getValue() == 0);
    // operator<< prints N bits per term and a newline
    ss.str("");
    ss << b;
    EXPECT(ss.str().size() == 1247 + 1);
    ss.str("");
    ss << (b + b);
    EXPECT(ss.str().size() == 2 * 1247 + 1);
    // empty ciphertext decrypts to 0; an object without a context refuses arithmetic
    Ciphertext empty;
    EXPECT(sk.decrypt(empty).getValue() == 0);
    bool threw = false;
    try {
        Ciphertext bad = empty * a;
    } catch (const std::logic_error &) {
        threw = true;
    }
    EXPECT(threw);
    EXPECT(Helper::exists(sk.getKey(), 16, sk.getKey()[3]) && !Helper::exists(sk.getKey(), 16, 5000));
    Helper::deletePointer(new uint64_t[4], true);
    printf("api ok device=%d\n", Library::currentDevice());
    return 0;
}

static int cmd_wire(int argc, char **argv)
{
    // wire <path>: deterministic ciphertexts -> product -> save; load back, compare, decrypt
    if (argc < 3)
        return 64;
    Context ctx(1247, 16);
    SecretKey sk(ctx);
    uint64_t key[16];
    for (int i = 0; i < 16; ++i)
        key[i] = (uint64_t)(i * 71 + 5);
    sk.setKey(key, 16);
    srand(2024);
    Plaintext one(1), zero(0);
    Ciphertext a = sk.encrypt(one), b = sk.encrypt(zero), c = sk.encrypt(one);
    Ciphertext prod = (a + b) * (c + a);           // 4 terms, plaintext (1^0)&(1^1) = 0
    {
        std::ofstream f(argv[2], std::ios::binary);
        prod.serialize(f);
        a.serialize(f);                            // two objects back to back in one stream
    }
    std::ifstream f(argv[2], std::ios::binary);
    Ciphertext p2 = Ciphertext::deserialize(f);
    Ciphertext a2 = Ciphertext::deserialize(f);
    EXPECT(p2.getLen() == prod.getLen() && a2.getLen() == 20);
    EXPECT(p2.getContext().getN() == 1247 && p2.getContext().getD() == 16);
    for (uint64_t i = 0; i < prod.getLen(); ++i)
        EXPECT(p2.getValues()[i] == prod.getValues()[i]);
    EXPECT(sk.decrypt(p2).getValue() == 0 && sk.decrypt(a2).getValue() == 1);
    dump("wire_prod", prod);
    dump("wire_a", a);
    // a custom Bitlen survives the round trip; garbage is refused
    uint64_t w[2] = {1, 2}, bl[2] = {7, 9};
    Context small(65, 4);
    Ciphertext odd(w, bl, 2, small);
    std::stringstream ss;
    odd.serialize(ss);
    Ciphertext odd2 = Ciphertext::deserialize(ss);
    EXPECT(!odd2.hasCanonicalBitlen() && odd2.getBitlen()[0] == 7 && odd2.getBitlen()[1] == 9);
    std::stringstream bad("not a ciphertext at all");
    bool threw = false;
    try {
        Ciphertext::deserialize(bad);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    EXPECT(threw);
    // the buffer forms write and read the same bytes as the stream forms
    {
        std::stringstream ref;
        prod.serialize(ref);
        const std::string bytes = ref.str();
        EXPECT(prod.serializedSize() == bytes.size());
        std::vector<unsigned char> buf(bytes.size() + 8, 0xEE);
        EXPECT(prod.serializeTo(buf.data(), buf.size()) == bytes.size());
        EXPECT(memcmp(buf.data(), bytes.data(), bytes.size()) == 0 && buf[bytes.size()] == 0xEE);
        Ciphertext p3 = Ciphertext::deserializeFrom(buf.data(), bytes.size());
        EXPECT(p3.getLen() == prod.getLen() && sk.decrypt(p3).getValue() == 0);
        for (uint64_t i = 0; i < prod.getLen(); ++i)
            EXPECT(p3.getValues()[i] == prod.getValues()[i]);
        std::stringstream oddref;
        odd.serialize(oddref);
        std::vector<unsigned char> ob(odd.serializedSize());
        EXPECT(odd.serializeTo(ob.data(), ob.size()) == oddref.str().size() && memcmp(ob.data(), oddref.str().data(), ob.size()) == 0);
        Ciphertext odd3 = Ciphertext::deserializeFrom(ob.data(), ob.size());
        EXPECT(!odd3.hasCanonicalBitlen() && odd3.getBitlen()[1] == 9 && odd3.getValues()[1] == 2);
        bool small_threw = false, short_threw = false;
        try { prod.serializeTo(buf.data(), bytes.size() - 1); } catch (const std::runtime_error &) { small_threw = true; }
        try { Ciphertext::deserializeFrom(buf.data(), bytes.size() - 1); } catch (const std::runtime_error &) { short_threw = true; }
        EXPECT(small_threw && short_threw);
    }
    printf("wire ok\n");
    return 0;
}

// ---- wirebench: throughput of the wire format and of the host mirror ----
namespace {
// an in-memory sink / source: what the stream write costs is a memcpy, nothing else
struct MemBuf : std::streambuf {
    std::vector<char> store;
    size_t wpos;
    explicit MemBuf(size_t cap) : store(cap), wpos(0) {}
    std::streamsize xsputn(const char *s, std::streamsize n)
    {
        if (wpos + (size_t)n > store.size())
            return 0;
        memcpy(store.data() + wpos, s, (size_t)n);
        wpos += (size_t)n;
        return n;
    }
    int_type overflow(int_type c)
    {
        if (c != traits_type::eof() && wpos < store.size())
            store[wpos++] = (char)c;
        return c;
    }
    void rewindForRead() { setg(store.data(), store.data(), store.data() + wpos); }
    void rewindForWrite() { wpos = 0; }
};
double nowSeconds()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
} // namespace

static int cmd_wirebench()
{
    Library::initializeLibrary();
    Context ctx(1247, 16);
    const uint64_t dl = ctx.getDefaultN();
    // a 1024-term ciphertext of synthetic words, made by deserialising a hand-built stream
    const uint64_t terms = 1024, words = terms * dl;
    MemBuf small(64 + words * 8);
    {
        std::ostream o(&small);
        const char head[8] = {'C', 'S', 'G', 'N', 1, 0, 0, 0};
        o.write(head, 8);
        uint64_t hdr[3] = {1247, 16, words};
        o.write(reinterpret_cast<const char *>(hdr), 24);
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (uint64_t i = 0; i < words; ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const uint64_t w = (i % dl == dl - 1) ? (x & 0xFFFFFFFE00000000ull) : x;
            o.write(reinterpret_cast<const char *>(&w), 8);
        }
    }
    small.rewindForRead();
    std::istream is(&small);
    Ciphertext c1k = Ciphertext::deserialize(is);
    EXPECT(c1k.getLen() == words);
    Ciphertext big = c1k * c1k;                                   // 2^20 terms, 168 MB, never mirrored on the host
    EXPECT(big.getLen() == words * terms);
    const double big_bytes = (double)big.getLen() * 8;
    MemBuf bulk((size_t)big_bytes + 64);
    auto best_of = [&](int reps, const std::function<void()> &fn) {
        double best = 1e30;
        for (int r = 0; r < reps; ++r) {
            const double t0 = nowSeconds();
            fn();
            best = std::min(best, nowSeconds() - t0);
        }
        return best;
    };
    // serialize / deserialize, 168 MB
    double t = best_of(4, [&] { bulk.rewindForWrite(); std::ostream o(&bulk); big.serialize(o); });
    printf("wirebench serialize   2^20 terms %7.1f MB  %8.3f ms  %6.2f GB/s\n", big_bytes / 1e6, t * 1e3, big_bytes / t / 1e9);
    Ciphertext back;
    t = best_of(4, [&] { bulk.rewindForRead(); std::istream i(&bulk); back = Ciphertext::deserialize(i); });
    printf("wirebench deserialize 2^20 terms %7.1f MB  %8.3f ms  %6.2f GB/s\n", big_bytes / 1e6, t * 1e3, big_bytes / t / 1e9);
    EXPECT(back.getLen() == big.getLen());
    // ... and without a stream: straight between HBM and a page-locked buffer of the caller's
    {
        void *pinned = nullptr, *alias = nullptr;
        EXPECT(csgn_host_alloc(&pinned, &alias, (size_t)big_bytes + 64) == 0);
        uint64_t wrote = 0;
        t = best_of(4, [&] { wrote = big.serializeTo(pinned, (uint64_t)big_bytes + 64); });
        printf("wirebench serializeTo     (pinned buffer) 2^20 terms %7.1f MB  %8.3f ms  %6.2f GB/s\n", big_bytes / 1e6, t * 1e3, big_bytes / t / 1e9);
        EXPECT(wrote == 32 + (uint64_t)big_bytes);
        Ciphertext back2;
        t = best_of(4, [&] { back2 = Ciphertext::deserializeFrom(pinned, wrote); });
        printf("wirebench deserializeFrom (pinned buffer) 2^20 terms %7.1f MB  %8.3f ms  %6.2f GB/s\n", big_bytes / 1e6, t * 1e3, big_bytes / t / 1e9);
        EXPECT(back2.getLen() == big.getLen());
        EXPECT(memcmp(static_cast<const char *>(pinned) + 32, bulk.store.data() + 32, 1 << 20) == 0);   // the stream form's bytes
        csgn_host_free(pinned);
    }
    // 160 KB ciphertexts, 200 in a row
    MemBuf sb(64 + words * 8);
    t = best_of(3, [&] { for (int k = 0; k < 200; ++k) { sb.rewindForWrite(); std::ostream o(&sb); c1k.serialize(o); } });
    printf("wirebench serialize   1024 terms  %7.3f MB  %8.3f us  %6.2f GB/s\n", words * 8 / 1e6, t / 200 * 1e6, 200.0 * words * 8 / t / 1e9);
    t = best_of(3, [&] { for (int k = 0; k < 200; ++k) { sb.rewindForRead(); std::istream i(&sb); Ciphertext x = Ciphertext::deserialize(i); } });
    printf("wirebench deserialize 1024 terms  %7.3f MB  %8.3f us  %6.2f GB/s\n", words * 8 / 1e6, t / 200 * 1e6, 200.0 * words * 8 / t / 1e9);
    // the host mirror of a fresh 1024 x 1024 product (getValues: a pinned block out of the runtime's pool; the FIRST
    // call of a size class pins it, later ones reuse it)
    const double tm = best_of(3, [&] { Ciphertext p = c1k * c1k; csgn_stream_sync(nullptr); });
    const double t_first = best_of(1, [&] { Ciphertext p = c1k * c1k; volatile uint64_t sink = p.getValues()[0]; (void)sink; });
    t = best_of(4, [&] { Ciphertext p = c1k * c1k; volatile uint64_t sink = p.getValues()[0]; (void)sink; });
    printf("wirebench getValues   2^20 terms %7.1f MB  %8.3f ms  %6.2f GB/s  (product + mirror %0.3f ms, product alone %0.3f ms; "
           "first call, which pins the block: %0.3f ms = %0.2f GB/s)\n",
           big_bytes / 1e6, (t - tm) * 1e3, big_bytes / (t - tm) / 1e9, t * 1e3, tm * 1e3, (t_first - tm) * 1e3,
           big_bytes / (t_first - tm) / 1e9);
    // words of the round trip equal the product's
    const uint64_t *a = big.getValues(), *b = back.getValues();
    for (uint64_t i = 0; i < big.getLen(); i += 4099)
        EXPECT(a[i] == b[i]);
    printf("wirebench ok\n");
    return 0;
}

static int cmd_batch(int count)
{
    // CiphertextBatch (extension): `count` independent depth-6 circuits in lock step, checked
    // against the circuit evaluated in the clear and against the per-object API.
    Library::initializeLibrary();
    Context ctx(1247, 16);
    SecretKey sk(ctx);
    const int inputs = 10;
    std::vector<std::vector<unsigned char> > bits(inputs, std::vector<unsigned char>(count));
    std::vector<CiphertextBatch> in;
    for (int k = 0; k < inputs; ++k) {
        for (int i = 0; i < count; ++i)
            bits[k][i] = (unsigned char)((i * 2654435761u + k * 40503u) >> 13 & 1);
        in.push_back(CiphertextBatch::encrypt(sk, bits[k], 1000 + k));
        std::vector<unsigned char> back = in.back().decrypt(sk);
        EXPECT(back == bits[k]);
    }
    {
        // default form: generator key from the OS, fresh per call -- decrypts to the bits, never the same words twice
        CiphertextBatch a = CiphertextBatch::encrypt(sk, bits[0]), b = CiphertextBatch::encrypt(sk, bits[0]);
        EXPECT(a.decrypt(sk) == bits[0] && b.decrypt(sk) == bits[0]);
        EXPECT(a.at(0).getLen() == 20);
        bool same = true;
        for (uint64_t w = 0; w < 20; ++w)
            same = same && a.at(0).getValues()[w] == b.at(0).getValues()[w];
        EXPECT(!same);
        // seeded form: a shard of the stream equals the same elements of the whole
        if (count > 3) {
            std::vector<unsigned char> tailbits(bits[1].begin() + 3, bits[1].end());
            CiphertextBatch whole = CiphertextBatch::encrypt(sk, bits[1], 4242);
            CiphertextBatch shard = CiphertextBatch::encrypt(sk, tailbits, 4242, 3);
            Ciphertext w3 = whole.at(3), s0 = shard.at(0);
            for (uint64_t w = 0; w < 20; ++w)
                EXPECT(w3.getValues()[w] == s0.getValues()[w]);
        }
    }
    CiphertextBatch x = in[0];
    std::vector<unsigned char> xb = bits[0];
    int k = 1;
    for (int level = 1; level <= 6; ++level) {
        if (level % 2) {
            x = x + in[k];
            for (int i = 0; i < count; ++i)
                xb[i] ^= bits[k][i];
            k += 1;
        } else {
            CiphertextBatch rhs = in[k] + in[k + 1];
            // the fused form answers Dec(x*rhs) before the product exists
            std::vector<unsigned char> fused = x.decryptProduct(rhs, sk);
            x = x * rhs;
            for (int i = 0; i < count; ++i)
                xb[i] &= (unsigned char)(bits[k][i] ^ bits[k + 1][i]);
            EXPECT(fused == xb);
            k += 2;
        }
        EXPECT(x.decrypt(sk) == xb);
    }
    EXPECT(x.terms() == 22 && x.size() == (uint64_t)count);
    // element 3 through the per-object API gives the same ciphertext words
    Ciphertext e = in[0].at(3);
    int kk = 1;
    for (int level = 1; level <= 6; ++level) {
        if (level % 2) {
            e += in[kk].at(3);
            kk += 1;
        } else {
            e *= (in[kk].at(3) + in[kk + 1].at(3));
            kk += 2;
        }
    }
    Ciphertext b3 = x.at(3);
    EXPECT(b3.getLen() == e.getLen());
    for (uint64_t i = 0; i < e.getLen(); ++i)
        EXPECT(b3.getValues()[i] == e.getValues()[i]);
    // batch-level applyPermutation = the per-object one on every element; the permuted key decrypts it
    {
        Permutation perm(ctx);
        SecretKey psk = sk.applyPermutation(perm);
        CiphertextBatch pb = in[1].applyPermutation(perm);
        EXPECT(pb.terms() == 1 && pb.size() == (uint64_t)count);
        EXPECT(pb.decrypt(psk) == bits[1]);
        CiphertextBatch px = x.applyPermutation(perm);          // multi-term input: ONE term, the permuted first
        EXPECT(px.terms() == 1);
        for (int i = 0; i < count; i += (count > 5 ? count / 5 : 1)) {
            Ciphertext a1 = pb.at(i), b1 = in[1].at(i).applyPermutation(perm);
            Ciphertext a2 = px.at(i), b2 = x.at(i).applyPermutation(perm);
            EXPECT(a1.getLen() == b1.getLen() && a2.getLen() == b2.getLen());
            for (uint64_t w = 0; w < a1.getLen(); ++w)
                EXPECT(a1.getValues()[w] == b1.getValues()[w] && a2.getValues()[w] == b2.getValues()[w]);
        }
    }
    // pack() round trip
    std::vector<Ciphertext> singles;
    for (int i = 0; i < 5; ++i)
        singles.push_back(in[2].at(i));
    CiphertextBatch packed = CiphertextBatch::pack(singles);
    std::vector<unsigned char> pb = packed.decrypt(sk);
    for (int i = 0; i < 5; ++i)
        EXPECT(pb[i] == bits[2][i]);
    // compact() (extension): identical terms cancel in pairs, Dec is unchanged
    {
        CiphertextBatch s2 = in[3] + in[4];                       // 2 terms per element
        CiphertextBatch sq = s2 * s2;                             // a*a + a*b + b*a + b*b
        CiphertextBatch cq = sq.compact();                        // a*b and b*a cancel: 2 terms, uniform again
        EXPECT(sq.terms() == 4 && cq.uniform() && cq.terms() == 2 && cq.totalTerms() == 2 * (uint64_t)count);
        EXPECT(cq.decrypt(sk) == sq.decrypt(sk));
        Ciphertext c0 = cq.at(0), a0 = in[3].at(0), b0 = in[4].at(0);
        for (uint64_t w = 0; w < 20; ++w)                         // a & a = a first, then b & b = b
            EXPECT(c0.getValues()[w] == a0.getValues()[w] && c0.getValues()[20 + w] == b0.getValues()[w]);
        CiphertextBatch zero = (in[3] + in[3]).compact();         // x + x vanishes
        EXPECT(zero.uniform() && zero.terms() == 0 && zero.totalTerms() == 0);
        std::vector<unsigned char> zb = zero.decrypt(sk);
        for (int i = 0; i < count; ++i)
            EXPECT(zb[i] == 0);
        // a ragged result: element i of `mix` is x + x (i even) or x + y (i odd)
        std::vector<Ciphertext> mixed;
        const int m = count < 9 ? count : 9;
        for (int i = 0; i < m; ++i)
            mixed.push_back(in[5].at(i) + (i % 2 ? in[6].at(i) : in[5].at(i)));
        CiphertextBatch mix = CiphertextBatch::pack(mixed).compact();
        if (m > 1) {
            EXPECT(!mix.uniform() && mix.terms() == 0 && mix.size() == (uint64_t)m);
            for (int i = 0; i < m; ++i)
                EXPECT(mix.termsOf(i) == (i % 2 ? 2u : 0u));
            std::vector<unsigned char> mb = mix.decrypt(sk);
            for (int i = 0; i < m; ++i)
                EXPECT(mb[i] == (i % 2 ? (bits[5][i] ^ bits[6][i]) : 0));
            // ragged arithmetic: (mix + y) * z against the clear evaluation; compact() of a ragged batch
            std::vector<Ciphertext> ys, zs;
            for (int i = 0; i < m; ++i) {
                ys.push_back(in[7].at(i));
                zs.push_back(in[8].at(i) + in[9].at(i));
            }
            CiphertextBatch y = CiphertextBatch::pack(ys), z = CiphertextBatch::pack(zs);
            CiphertextBatch r = (mix + y) * z;
            EXPECT(!r.uniform());
            std::vector<unsigned char> rb = r.decrypt(sk), rc = r.compact().decrypt(sk);
            for (int i = 0; i < m; ++i) {
                const unsigned char want = (unsigned char)(((i % 2 ? (bits[5][i] ^ bits[6][i]) : 0) ^ bits[7][i]) &
                                                           (bits[8][i] ^ bits[9][i]));
                EXPECT(r.termsOf(i) == (mix.termsOf(i) + 1) * 2);
                EXPECT(rb[i] == want && rc[i] == want);
                EXPECT(r.at(i).getLen() == r.termsOf(i) * 20);
            }
        }
    }
    printf("batch ok count=%d\n", count);
    return 0;
}

static int cmd_graph(int count)
{
    // BatchCircuit (extension): BASELINE config 5 -- Permutation on every input, depth-16 circuit,
    // decrypt under the permuted key -- captured once into a hipGraph and replayed on three input
    // sets; every replay must equal the circuit in the clear (bits) and, on sampled elements, the
    // same circuit through the per-object API (words).
    Library::initializeLibrary();
    Context ctx(4096, 32);
    SecretKey sk(ctx);
    const int levels = 16, inputs = 1 + levels / 2 + 2 * (levels / 2);
    // a random Permutation applied to every fresh input inside the graph, and to the key (config 5)
    Permutation perm(ctx);
    SecretKey psk = sk.applyPermutation(perm);
    BatchCircuit c(ctx, (uint64_t)count);
    std::vector<unsigned> raw, in;
    for (int i = 0; i < inputs; ++i) {
        raw.push_back(c.input(1));
        in.push_back(c.permute(raw.back(), perm));
    }
    unsigned x = in[0];
    int k = 1;
    for (int level = 1; level <= levels; ++level) {
        if (level % 2) {
            x = c.add(x, in[k]);
            k += 1;
        } else {
            x = c.mul(x, c.add(in[k], in[k + 1]));
            k += 2;
        }
    }
    const unsigned res = c.decrypt(x, psk);
    c.build();
    // the same circuit COMPILED (BatchCircuit::optimize): products written straight into the sums that consume them,
    // the last product fused into the decrypt, buffers reused -- same bits, a fraction of the HBM, and value() only
    // for what was kept
    BatchCircuit cc(ctx, (uint64_t)count);
    std::vector<unsigned> craw;
    unsigned cx = 0, cres = 0;
    {
        std::vector<unsigned> cin;
        for (int i = 0; i < inputs; ++i) {
            craw.push_back(cc.input(1));
            cin.push_back(cc.permute(craw.back(), perm));
        }
        cx = cin[0];
        int ck = 1;
        for (int level = 1; level <= levels; ++level) {
            if (level % 2) {
                cx = cc.add(cx, cin[ck]);
                ck += 1;
            } else {
                cx = cc.mul(cx, cc.add(cin[ck], cin[ck + 1]));
                ck += 2;
            }
        }
        cres = cc.decrypt(cx, psk);
        cc.optimize();
        cc.build();
        EXPECT(cc.blockBytes() * 2 < c.blockBytes());
    }
    for (int round = 0; round < 3; ++round) {
        std::vector<std::vector<unsigned char> > bits(inputs, std::vector<unsigned char>(count));
        std::vector<CiphertextBatch> fresh;
        for (int i = 0; i < inputs; ++i) {
            for (int j = 0; j < count; ++j)
                bits[i][j] = (unsigned char)(((j + 3 * round) * 2654435761u + i * 40503u) >> 11 & 1);
            fresh.push_back(CiphertextBatch::encrypt(sk, bits[i], 7000 + 100 * round + i));
            c.set(raw[i], fresh.back());
            cc.set(craw[i], fresh.back());
        }
        c.run();
        cc.run();
        std::vector<unsigned char> yb = bits[0];
        k = 1;
        for (int level = 1; level <= levels; ++level) {
            if (level % 2) {
                for (int j = 0; j < count; ++j)
                    yb[j] ^= bits[k][j];
                k += 1;
            } else {
                for (int j = 0; j < count; ++j)
                    yb[j] &= (unsigned char)(bits[k][j] ^ bits[k + 1][j]);
                k += 2;
            }
        }
        EXPECT(c.bits(res) == yb);
        EXPECT(cc.bits(cres) == yb);
        {
            bool refused = false;
            try {
                (void)cc.value(cx);
            } catch (const std::invalid_argument &) {
                refused = true;
            }
            EXPECT(refused);                      // not kept: never computed
        }
        CiphertextBatch g = c.value(x);
        EXPECT(g.terms() == 766);
        // sampled elements: the same circuit through the per-object API (applyPermutation, +=, *=)
        for (int j = 0; j < count; j += (count > 3 ? count / 3 : 1)) {
            Ciphertext e = fresh[0].at(j).applyPermutation(perm);
            k = 1;
            for (int level = 1; level <= levels; ++level) {
                if (level % 2) {
                    e += fresh[k].at(j).applyPermutation(perm);
                    k += 1;
                } else {
                    e *= (fresh[k].at(j).applyPermutation(perm) + fresh[k + 1].at(j).applyPermutation(perm));
                    k += 2;
                }
            }
            Ciphertext a = g.at(j);
            EXPECT(a.getLen() == e.getLen());
            for (uint64_t w = 0; w < a.getLen(); ++w)
                EXPECT(a.getValues()[w] == e.getValues()[w]);
            EXPECT(psk.decrypt(e).getValue() == yb[j]);
        }
    }
    {
        // fresh-ciphertext circuit entirely inside one graph (BASELINE configs 2 / 4 end to end):
        // two encrypted inputs, product and sum, both decrypted; new bits and a new keystream per run
        BatchCircuit f(ctx, count);
        unsigned ea = f.encryptInput(sk), eb = f.encryptInput(sk);
        unsigned rm = f.decrypt(f.mul(ea, eb), sk), rs = f.decrypt(f.add(ea, eb), sk);
        f.build();
        std::vector<uint64_t> first_words;
        for (int round = 0; round < 3; ++round) {
            std::vector<unsigned char> ba(count), bb(count), wm(count), ws(count);
            for (int i = 0; i < count; ++i) {
                ba[i] = (unsigned char)((i * 7 + round) & 1);
                bb[i] = (unsigned char)(((i >> 1) + round) & 1);
                wm[i] = ba[i] & bb[i];
                ws[i] = ba[i] ^ bb[i];
            }
            f.setPlain(ea, ba);
            f.setPlain(eb, bb);
            f.run();
            EXPECT(f.bits(rm) == wm);
            EXPECT(f.bits(rs) == ws);
            EXPECT(f.value(ea).decrypt(sk) == ba);
            first_words.push_back(f.value(ea).at(0).getValues()[0]);
        }
        EXPECT(first_words[0] != first_words[1] || first_words[1] != first_words[2]);
    }
    {
        // the same chain as ONE fused node (BatchCircuit::encryptProduct): the product and its decryption
        // come out of a single kernel; the product must decrypt, word by word through the per-object API
        // too, to a[i] & b[i]
        BatchCircuit f(ctx, count);
        unsigned bits_id = 0;
        const unsigned prod = f.encryptProduct(sk, &bits_id);
        f.build();
        std::vector<uint64_t> first_words;
        for (int round = 0; round < 3; ++round) {
            std::vector<unsigned char> ba(count), bb(count), wm(count);
            for (int i = 0; i < count; ++i) {
                ba[i] = (unsigned char)((i * 5 + round) & 1);
                bb[i] = (unsigned char)(((i >> 2) + round) & 1);
                wm[i] = ba[i] & bb[i];
            }
            f.setPlainPair(prod, ba, bb);
            f.run();
            EXPECT(f.bits(bits_id) == wm);
            CiphertextBatch p = f.value(prod);
            EXPECT(p.terms() == 1 && p.decrypt(sk) == wm);
            Ciphertext one = p.at(count - 1);
            EXPECT(sk.decrypt(one).getValue() == wm[count - 1]);
            first_words.push_back(p.at(0).getValues()[0]);
        }
        EXPECT(first_words[0] != first_words[1] || first_words[1] != first_words[2]);
    }
    printf("graph ok count=%d\n", count);
    return 0;
}

static int cmd_deferred(int rounds, uint64_t n, uint64_t d)
{
    // The deferred queue against the immediate path, word for word: random expression DAGs over fresh ciphertexts
    // (products and sums of operands that are themselves queued results, copies, reassigned and destroyed operands, more
    // than one queue-full of operations), evaluated twice -- queued and one launch per operation.  Context(n, d): odd and
    // even word counts put both unit widths of the queue's kernel on the path.
    Library::initializeLibrary();
    Context ctx(n, d);
    SecretKey sk(ctx);
    uint32_t rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (int r = 0; r < rounds; ++r) {
        std::vector<int> bits;
        std::vector<Ciphertext> fresh;
        for (int i = 0; i < 6; ++i) {
            bits.push_back((int)(next() & 1u));
            Plaintext pt(bits.back());
            fresh.push_back(sk.encrypt(pt));
        }
        const uint32_t seed = rng;
        std::vector<std::vector<uint64_t> > words[2];
        std::vector<int> clear[2];
        for (int mode = 0; mode < 2; ++mode) {
            Library::deferSmallOperations(mode == 0);
            rng = seed;
            std::vector<Ciphertext> pool(fresh);
            std::vector<int> pbits(bits);
            const int nops = 40 + (int)(next() % 600u);
            for (int k = 0; k < nops; ++k) {
                const size_t ia = next() % pool.size(), ib = next() % pool.size();
                const bool mul = (next() & 1u) != 0u;
                const uint64_t dl = ctx.getDefaultN(), ta = pool[ia].getLen() / dl, tb = pool[ib].getLen() / dl;
                if ((mul ? ta * tb : ta + tb) > 48)
                    continue;
                Ciphertext res = mul ? pool[ia] * pool[ib] : pool[ia] + pool[ib];
                const int bit = mul ? (pbits[ia] & pbits[ib]) : (pbits[ia] ^ pbits[ib]);
                switch (next() % 4u) {
                case 0: pool.push_back(res); pbits.push_back(bit); break;                 // a new value
                case 1: pool[ia] = res; pbits[ia] = bit; break;                            // the operand is reassigned
                case 2: { Ciphertext copy(res); pool[ib] = copy; pbits[ib] = bit; break; } // through a copy
                default: break;                                                             // the result dies unread
                }
                if (pool.size() > 24) {
                    pool.erase(pool.begin() + 6);
                    pbits.erase(pbits.begin() + 6);
                }
            }
            for (size_t i = 0; i < pool.size(); ++i) {
                const uint64_t *v = pool[i].getValues();
                words[mode].push_back(std::vector<uint64_t>(v, v + pool[i].getLen()));
                clear[mode].push_back(pbits[i]);
                EXPECT(sk.decrypt(pool[i]).getValue() == (unsigned)pbits[i]);
            }
        }
        EXPECT(words[0].size() == words[1].size());
        for (size_t i = 0; i < words[0].size(); ++i)
            EXPECT(words[0][i] == words[1][i]);
        EXPECT(clear[0] == clear[1]);
    }
    Library::deferSmallOperations(true);
    printf("deferred ok rounds=%d n=%llu d=%llu\n", rounds, (unsigned long long)n, (unsigned long long)d);
    return 0;
}

static int cmd_deferred_threads(int rounds)
{
    // The deferred queue across host threads: a ciphertext whose producing operation is still queued in thread A's queue is
    // handed to thread B, which uses it as an operand (B evaluates A's queue under A's lock, on A's device) while A keeps
    // queueing; both threads' results against the same operations done one launch at a time.
    Library::initializeLibrary();
    Context ctx(1247, 16);
    SecretKey sk(ctx);
    for (int r = 0; r < rounds; ++r) {
        Plaintext p1(1), p0(r & 1);
        Ciphertext a = sk.encrypt(p1), b = sk.encrypt(p0), c = sk.encrypt(p1);
        Library::deferSmallOperations(false);
        Ciphertext want_ab = a * b, want_x = (a * b) + c, want_y = ((a * b) + c) * (a * b), want_z = (a + c) * b;
        Library::deferSmallOperations(true);
        Ciphertext ab = a * b;                                    // queued here, in the main thread's queue
        Ciphertext x, y;
        std::thread other([&] {
            x = ab + c;                                           // operand pending in ANOTHER thread's queue
            y = x * ab;
            volatile uint64_t w = y.getValues()[0];               // evaluates this thread's queue
            (void)w;
        });
        Ciphertext z = (a + c) * b;                               // meanwhile the main thread keeps queueing
        other.join();
        auto same = [](const Ciphertext &u, const Ciphertext &v) {
            if (u.getLen() != v.getLen())
                return false;
            const uint64_t *p = u.getValues(), *q = v.getValues();
            for (uint64_t i = 0; i < u.getLen(); ++i)
                if (p[i] != q[i])
                    return false;
            return true;
        };
        EXPECT(same(ab, want_ab));
        EXPECT(same(x, want_x));
        EXPECT(same(y, want_y));
        EXPECT(same(z, want_z));
        EXPECT(sk.decrypt(y).getValue() == (unsigned)((((1 & (r & 1)) ^ 1) & (1 & (r & 1)))));
    }
    printf("deferred threads ok rounds=%d\n", rounds);
    return 0;
}

static int cmd_deferred_exit(int rounds)
{
    // The deferred queue's hand-over between threads, against the same operations done one launch at a time:
    //  - a worker queues 3-20 small operations (the record path, not the one-or-two-operation one), hands the results to
    //    the main thread and ends; its queue is evaluated at its exit and the main thread reads and decrypts the results;
    //  - one const ciphertext whose operations are still queued is read by 4 threads at once (a start barrier), each
    //    through SecretKey::decrypt and serializedSize().
    Library::initializeLibrary();
    Context ctx(1247, 16);
    SecretKey sk(ctx);
    uint32_t rng = 777u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    auto words = [](const Ciphertext &c) {
        const uint64_t *v = c.getValues();
        return std::vector<uint64_t>(v, v + c.getLen());
    };
    for (int r = 0; r < rounds; ++r) {
        std::vector<Ciphertext> fresh;
        std::vector<int> bits;
        for (int i = 0; i < 4; ++i) {
            bits.push_back((int)(next() & 1u));
            Plaintext pt(bits.back());
            fresh.push_back(sk.encrypt(pt));
        }
        const int nops = 3 + (int)(next() % 18u);
        const uint32_t seed = rng;
        // operands of at most 8 terms a side (kDeferMaxTerms): every operation of the worker is queued
        auto program = [&](std::vector<Ciphertext> &pool, std::vector<int> &pbits) {
            rng = seed;
            for (int k = 0; k < nops; ++k) {
                size_t ia, ib;
                do {
                    ia = next() % pool.size();
                    ib = next() % pool.size();
                } while (pool[ia].getTerms() > 8 || pool[ib].getTerms() > 8);
                const bool mul = (next() & 1u) != 0u;
                pool.push_back(mul ? pool[ia] * pool[ib] : pool[ia] + pool[ib]);
                pbits.push_back(mul ? (pbits[ia] & pbits[ib]) : (pbits[ia] ^ pbits[ib]));
            }
        };
        std::vector<Ciphertext> want(fresh), got(fresh);
        std::vector<int> want_bits(bits), got_bits(bits);
        Library::deferSmallOperations(false);
        program(want, want_bits);
        Library::deferSmallOperations(true);
        std::thread worker([&] { program(got, got_bits); });
        worker.join();
        EXPECT(got.size() == want.size() && got_bits == want_bits);
        for (size_t i = 0; i < got.size(); ++i) {
            EXPECT(words(got[i]) == words(want[i]));
            EXPECT(sk.decrypt(got[i]).getValue() == (unsigned)want_bits[i]);
        }

        // four readers of one shared const ciphertext (sk's key mask is made above, so decrypt only reads sk)
        const Ciphertext &a = fresh[0], &b = fresh[1], &c = fresh[2];
        Library::deferSmallOperations(false);
        const Ciphertext x_want = ((a * b) + c) * (a + c);
        Library::deferSmallOperations(true);
        const Ciphertext x = ((a * b) + c) * (a + c);          // queued in the main thread's queue
        const unsigned x_bit = (unsigned)(((bits[0] & bits[1]) ^ bits[2]) & (bits[0] ^ bits[2]));
        std::atomic<int> ready(0);
        unsigned seen_bit[4];
        uint64_t seen_size[4];
        std::vector<std::thread> readers;
        for (int t = 0; t < 4; ++t)
            readers.emplace_back([&, t] {
                ready.fetch_add(1);
                while (ready.load() < 4)
                    std::this_thread::yield();
                // (decrypt takes the reference API's non-const reference; it only reads the ciphertext)
                seen_bit[t] = sk.decrypt(const_cast<Ciphertext &>(x)).getValue();
                seen_size[t] = x.serializedSize();
            });
        for (std::thread &t : readers)
            t.join();
        for (int t = 0; t < 4; ++t)
            EXPECT(seen_bit[t] == x_bit && seen_size[t] == x_want.serializedSize());
        EXPECT(words(x) == words(x_want));
    }
    printf("deferred exit ok rounds=%d\n", rounds);
    return 0;
}

static int cmd_latency(int iters)
{
    // steady-state cost of single operations through the value-semantic class API
    Library::initializeLibrary();
    Context ctx(1247, 16);
    SecretKey sk(ctx);
    Plaintext one(1), zero(0);
    Ciphertext a = sk.encrypt(one), b = sk.encrypt(zero);
    Ciphertext big = a + b, mid = a + b;
    for (int i = 0; i < 6; ++i) {
        big = big * (a + b);                        // 128 terms
        if (i == 4)
            mid = big;                              // 64 terms
    }
    struct Case { const char *name; int kind; } cases[] = {
        {"mul 1x1", 0}, {"add 1+1", 1}, {"decrypt 1 term", 2}, {"encrypt", 3},
        {"mul 128x2", 4}, {"decrypt 128 terms", 5}, {"mul 64x64", 6}};
    // every case twice: operations on small ciphertexts QUEUED (the default: one launch per 256 of them) and issued one
    // by one (Library::deferSmallOperations(false)).  The clock stops after the queue has been evaluated and the GPU has
    // finished: what is timed is work done, not work promised.
    for (int pass = 0; pass < 2; ++pass)
    for (const Case &c : cases) {
        Library::deferSmallOperations(pass == 0);
        Timer t(c.name);
        int acc = 0;
        csgn_stream_sync(nullptr);
        t.start();
        for (int i = 0; i < iters; ++i) {
            switch (c.kind) {
            case 0: { Ciphertext r = a * b; acc += (int)r.getLen(); break; }
            case 1: { Ciphertext r = a + b; acc += (int)r.getLen(); break; }
            case 2: acc += sk.decrypt(a).getValue(); break;
            case 3: { Ciphertext r = sk.encrypt(one); acc += (int)r.getLen(); break; }
            case 4: { Ciphertext r = big * (a + b); acc += (int)r.getLen(); break; }
            case 6: { Ciphertext r = mid * mid; acc += (int)r.getLen(); break; }
            default: acc += sk.decrypt(big).getValue(); break;
            }
        }
        Library::flush();
        csgn_stream_sync(nullptr);
        double ms = t.stop();
        printf("latency %-18s %8.2f us/op (acc %d)%s\n", c.name, ms * 1000.0 / iters, acc, pass == 0 ? "" : "  [one launch per operation]");
    }
    Library::deferSmallOperations(true);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: dropin_driver <basic|permutations|timings|encrypt|circuit|bitlen|api> ...\n");
        return 64;
    }
    try {
        std::string cmd = argv[1];
        if (cmd == "basic")
            return cmd_basic(argc > 2 ? atoi(argv[2]) : 20);
        if (cmd == "permutations")
            return cmd_permutations(argc > 2 ? atoi(argv[2]) : 5);
        if (cmd == "timings")
            return cmd_timings();
        if (cmd == "encrypt")
            return cmd_encrypt(argc, argv);
        if (cmd == "circuit")
            return cmd_circuit(argc, argv);
        if (cmd == "bitlen")
            return cmd_bitlen();
        if (cmd == "api")
            return cmd_api();
        if (cmd == "wire")
            return cmd_wire(argc, argv);
        if (cmd == "wirebench")
            return cmd_wirebench();
        if (cmd == "batch")
            return cmd_batch(argc > 2 ? atoi(argv[2]) : 4096);
        if (cmd == "graph")
            return cmd_graph(argc > 2 ? atoi(argv[2]) : 5);
        if (cmd == "latency")
            return cmd_latency(argc > 2 ? atoi(argv[2]) : 2000);
        if (cmd == "deferred")
            return cmd_deferred(argc > 2 ? atoi(argv[2]) : 20, argc > 4 ? strtoull(argv[3], nullptr, 10) : 1247,
                                argc > 4 ? strtoull(argv[4], nullptr, 10) : 16);
        if (cmd == "deferred_threads")
            return cmd_deferred_threads(argc > 2 ? atoi(argv[2]) : 50);
        if (cmd == "deferred_exit")
            return cmd_deferred_exit(argc > 2 ? atoi(argv[2]) : 20);
        return 64;
    } catch (const std::exception &e) {
        fprintf(stderr, "certFHE error: %s\n", e.what());
        return 3;
    }
}
