// gates_driver.cpp -- user-style C++ over include/certfhe/Gates.h (tests/test_gates_cpp.py builds and runs it).
//   gates_driver single    single-Ciphertext gates: words == the operators' composition, decryptions == the gate
//   gates_driver batch     CiphertextBatch gates, uniform and ragged (compact() output)
//   gates_driver circuit   BatchCircuit: 4-bit equality and 6-bit unsigned less-than over 1000 random pairs
//   gates_driver forms    "<shape> -> <form>": the form csgn_gate_uniform_kernel names under the process's knob
// Prints "<mode> ok" and exits 0, or names the first mismatch and exits 1.
#include "driver.h"

#include "csgn_hip.h"

using namespace certFHE;

namespace {

// the ONE term from its words, not through Gates.cpp
Ciphertext oneByHand(const Context &ctx)
{
    const uint64_t n = ctx.getN(), dl = ctx.getDefaultN();
    std::vector<uint64_t> v(dl, ~0ull), bl(dl, 64);
    if (n % 64) {
        v[dl - 1] = ~0ull << (64 - n % 64);
        bl[dl - 1] = n % 64;
    }
    return Ciphertext(v.data(), bl.data(), dl, ctx);
}

unsigned char dec(SecretKey &key, Ciphertext c) { return key.decrypt(c).getValue(); }

int single()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const Ciphertext one = oneByHand(ctx), zero = constantCiphertext(ctx, 0);
    expect(sameWords(constantCiphertext(ctx, 1), one), "constantCiphertext(1)");
    for (int s = 0; s < 2; ++s)
        for (int x = 0; x < 2; ++x)
            for (int y = 0; y < 2; ++y) {
                Plaintext ps(s), px(x), py(y);
                Ciphertext cs = key.encrypt(ps), a = key.encrypt(px), b = key.encrypt(py);
                const std::string at = " s=" + std::to_string(s) + " a=" + std::to_string(x) + " b=" + std::to_string(y);
                expect(sameWords(logicNot(a), a + one), "NOT words" + at);
                expect(sameWords(logicXnor(a, b), (a + b) + one), "XNOR words" + at);
                expect(sameWords(logicNand(a, b), (a * b) + one), "NAND words" + at);
                expect(sameWords(logicOr(a, b), (a + b) + (a * b)), "OR words" + at);
                expect(sameWords(logicNor(a, b), ((a + b) + (a * b)) + one), "NOR words" + at);
                expect(sameWords(logicMux(cs, a, b), (cs * (a + b)) + b), "MUX words" + at);
                expect(sameWords(addPlain(a, 1), a + one) && sameWords(addPlain(a, 0), a + zero), "addPlain words" + at);
                expect(sameWords(mulPlain(a, 1), a * one) && sameWords(mulPlain(a, 0), a * zero), "mulPlain words" + at);
                expect(dec(key, logicNot(a)) == (1 ^ x), "NOT" + at);
                expect(dec(key, logicXnor(a, b)) == (1 ^ x ^ y), "XNOR" + at);
                expect(dec(key, logicNand(a, b)) == (1 ^ (x & y)), "NAND" + at);
                expect(dec(key, logicOr(a, b)) == (x | y), "OR" + at);
                expect(dec(key, logicNor(a, b)) == (1 ^ (x | y)), "NOR" + at);
                expect(dec(key, logicMux(cs, a, b)) == (s ? x : y), "MUX" + at);
                expect(dec(key, addPlain(a, (unsigned char)s)) == (x ^ s), "addPlain" + at);
                expect(dec(key, mulPlain(a, (unsigned char)s)) == (x & s), "mulPlain" + at);
            }
    return 0;
}

void checkBatch(const CiphertextBatch &r, SecretKey &key, const std::vector<unsigned char> &want, const std::string &what)
{
    const std::vector<unsigned char> got = r.decrypt(key);
    bool ok = got.size() == want.size();
    for (size_t i = 0; ok && i < want.size(); ++i)
        ok = got[i] == want[i];
    expect(ok, what);
}

int batch()
{
    Context ctx(1247, 16);
    SecretKey key(ctx);
    const size_t n = 300;
    const std::vector<unsigned char> bs = randomBits(n), ba = randomBits(n), bb = randomBits(n), p = randomBits(n),
                                     q = randomBits(n);
    CiphertextBatch s = CiphertextBatch::encrypt(key, bs, 1), a = CiphertextBatch::encrypt(key, ba, 2),
                    b = CiphertextBatch::encrypt(key, bb, 3);
    const CiphertextBatch one = constantBatch(ctx, std::vector<unsigned char>(n, 1));
    // ragged: a + C(p) + C(q), compacted -- the two constants cancel where p == q (1 term), stay where not (3 terms)
    const CiphertextBatch x = addPlain(addPlain(a, p), q).compact();
    expect(!x.uniform(), "compact() gave a ragged batch");
    std::vector<unsigned char> vx(n);
    for (size_t i = 0; i < n; ++i)
        vx[i] = ba[i] ^ p[i] ^ q[i];
    for (int pass = 0; pass < 2; ++pass) {
        const CiphertextBatch &u = pass ? x : a;
        const std::vector<unsigned char> &vu = pass ? vx : ba;
        const std::string tag = pass ? " (ragged)" : " (uniform)";
        std::vector<unsigned char> w(n);
        for (size_t i = 0; i < n; ++i) w[i] = 1 ^ vu[i];
        checkBatch(logicNot(u), key, w, "NOT" + tag);
        for (size_t i = 0; i < n; ++i) w[i] = 1 ^ vu[i] ^ bb[i];
        checkBatch(logicXnor(u, b), key, w, "XNOR" + tag);
        for (size_t i = 0; i < n; ++i) w[i] = 1 ^ (vu[i] & bb[i]);
        checkBatch(logicNand(u, b), key, w, "NAND" + tag);
        for (size_t i = 0; i < n; ++i) w[i] = vu[i] | bb[i];
        checkBatch(logicOr(u, b), key, w, "OR" + tag);
        for (size_t i = 0; i < n; ++i) w[i] = 1 ^ (vu[i] | bb[i]);
        checkBatch(logicNor(u, b), key, w, "NOR" + tag);
        for (size_t i = 0; i < n; ++i) w[i] = bs[i] ? vu[i] : bb[i];
        checkBatch(logicMux(s, u, b), key, w, "MUX" + tag);
        for (size_t i = 0; i < n; ++i) w[i] = vu[i] ^ p[i];
        checkBatch(addPlain(u, p), key, w, "addPlain" + tag);
        for (size_t i = 0; i < n; ++i) w[i] = vu[i] & p[i];
        checkBatch(mulPlain(u, p), key, w, "mulPlain" + tag);
        // words: the definition through the batch operators
        expect(sameBatchWords(logicOr(u, b), (u + b) + (u * b)), "OR words" + tag);
        expect(sameBatchWords(logicNor(u, b), ((u + b) + (u * b)) + one), "NOR words" + tag);
        expect(sameBatchWords(logicMux(s, u, b), (s * (u + b)) + b), "MUX words" + tag);
        expect(sameBatchWords(logicNot(u), u + one), "NOT words" + tag);
        expect(sameBatchWords(addPlain(u, p), u + constantBatch(ctx, p)), "addPlain words" + tag);
        expect(sameBatchWords(mulPlain(u, p), u * constantBatch(ctx, p)), "mulPlain words" + tag);
        // NOT(NOT u) compacts back to u's terms
        const CiphertextBatch nn = logicNot(logicNot(u)).compact(), uc = u.compact();
        expect(sameBatchWords(nn, uc), "compact(NOT(NOT u))" + tag);
    }
    return 0;
}

// 4-bit equality (AND over XNORs) and 6-bit unsigned less-than (MUX chain from constant(0), LSB first, compact() after
// every stage) over `count` random pairs, as a tape and optimize()d
int circuit()
{
    Context ctx(127, 8);           // small terms: the less-than chain grows ~3x a stage (values stay under ~100 MB)
    SecretKey key(ctx);
    const uint64_t count = 1000;
    std::vector<std::vector<unsigned char> > abits(6), bbits(6);
    for (int i = 0; i < 6; ++i) {
        abits[i] = randomBits(count);
        bbits[i] = randomBits(count);
    }
    for (uint64_t e = 0; e < count; e += 7)            // some equal pairs, so that equality is not always 0
        for (int i = 0; i < 6; ++i)
            bbits[i][e] = abits[i][e];
    for (int opt = 0; opt < 2; ++opt) {
        BatchCircuit c(ctx, count);
        unsigned a[6], b[6];
        for (int i = 0; i < 6; ++i) {
            a[i] = c.input(1);
            b[i] = c.input(1);
        }
        unsigned eq = c.logicXnor(a[0], b[0]);
        for (int i = 1; i < 4; ++i)
            eq = c.mul(eq, c.logicXnor(a[i], b[i]));
        unsigned lt = c.constant(0);
        for (int i = 0; i < 6; ++i)                     // bits differ at i: a < b iff b_i; else the lower bits decide
            lt = c.compact(c.logicMux(c.add(a[i], b[i]), b[i], lt));
        const unsigned p = c.plainInput();              // a public flip of the equality bit, set after build()
        const unsigned eq_bits = c.decrypt(eq, key), lt_bits = c.decrypt(lt, key);
        const unsigned flip_bits = c.decrypt(c.add(eq, p), key);
        if (opt)
            c.optimize();
        c.build();
        for (int i = 0; i < 6; ++i) {
            c.set(a[i], CiphertextBatch::encrypt(key, abits[i], 10 + i));
            c.set(b[i], CiphertextBatch::encrypt(key, bbits[i], 20 + i));
        }
        const std::vector<unsigned char> flip = randomBits(count);
        c.setPlainBits(p, flip);
        for (int run = 0; run < 2; ++run) {
            c.run();
            const std::vector<unsigned char> ge = c.bits(eq_bits), gl = c.bits(lt_bits), gf = c.bits(flip_bits);
            for (uint64_t e = 0; e < count; ++e) {
                unsigned va = 0, vb = 0;
                for (int i = 0; i < 6; ++i) {
                    va |= (unsigned)abits[i][e] << i;
                    vb |= (unsigned)bbits[i][e] << i;
                }
                const unsigned char want_eq = (va & 15) == (vb & 15), want_lt = va < vb;
                const std::string at = " opt=" + std::to_string(opt) + " run=" + std::to_string(run) + " e=" + std::to_string(e);
                expect(ge[e] == want_eq, "equality" + at);
                expect(gl[e] == want_lt, "less-than" + at);
                expect(gf[e] == (want_eq ^ flip[e]), "plain input" + at);
            }
        }
    }
    return 0;
}

// No device work: the form csgn_gate_uniform_kernel names for the shapes of batch (300 elements at N=1247, fresh
// operands) and for products past the fused / pitched cut, under the knob the process was started with.
int forms()
{
    const char *names[] = {"", "NOT", "XNOR", "NAND", "OR", "NOR", "MUX", "ADD_PLAIN", "MUL_PLAIN"};
    const uint64_t shapes[][3] = {{1, 1, 1}, {1, 3, 3}, {1, 9, 8}, {2, 3, 3}};      // t_sel, t_a, t_b
    for (const auto &t : shapes)
        for (int g = CSGN_GATE_NOT; g <= CSGN_GATE_MUL_PLAIN; ++g) {
            const char *form = csgn_gate_uniform_kernel(1247, g, 300, t[0], t[1], t[2]);
            expect(form && *form, std::string(names[g]) + " has a form");
            printf("%s ts=%llu ta=%llu tb=%llu -> %s\n", names[g], (unsigned long long)t[0], (unsigned long long)t[1],
                   (unsigned long long)t[2], form ? form : "");
        }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    return runModes(argc, argv, 12345, "gates_driver", {{"single", single}, {"batch", batch}, {"circuit", circuit}, {"forms", forms}});
}
