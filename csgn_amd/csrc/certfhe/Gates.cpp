// Gates.cpp -- plaintext constants and the boolean gates (extension, see Gates.h) over the C ABI.
#include "Gates.h"

#include "runtime.h"

#include <cstring>
#include <stdexcept>
#include <string>

namespace certFHE {

using detail::BatchAccess;
using detail::DevicePayload;
using detail::ones;

namespace {

std::shared_ptr<DevicePayload> uploadBits(const std::vector<unsigned char> &bits)
{
    std::vector<uint64_t> stage((bits.size() + 7) / 8, 0);
    if (!bits.empty())
        memcpy(stage.data(), bits.data(), bits.size());
    return detail::uploadWords(stage.data(), stage.size());
}

void requireSame(const CiphertextBatch &a, const CiphertextBatch &b, const char *who)
{
    if (a.context().getN() != b.context().getN() || a.size() != b.size())
        throw std::invalid_argument(std::string("certFHE::") + who + ": operands differ in N or element count");
}

// one csgn_gate_uniform call over uniform operands (sel / b / plain: null when the gate does not read them)
CiphertextBatch uniformGate(int gate, const CiphertextBatch *sel, const CiphertextBatch &a, const CiphertextBatch *b,
                            const DevicePayload *plain)
{
    const uint64_t ts = sel ? sel->terms() : 0, ta = a.terms(), tb = b ? b->terms() : 0;
    const uint64_t terms = csgn_gate_terms(gate, ts, ta, tb);
    if (terms == 0)
        throw std::invalid_argument("certFHE: gate over an empty operand, or its size overflows");
    CiphertextBatch out = BatchAccess::make(a.context(), a.size(), terms);
    if (a.size())
        detail::check(csgn_gate_uniform(a.context().getN(), gate, a.size(), ts, ta, tb, sel ? sel->deviceValues() : nullptr,
                                        a.deviceValues(), b ? b->deviceValues() : nullptr,
                                        plain ? reinterpret_cast<const uint8_t *>(plain->data()) : nullptr,
                                        BatchAccess::words(out), detail::stream()),
                      "csgn_gate_uniform");
    return out;
}

} // namespace

// ------------------------------------------------------------------ batches

CiphertextBatch constantBatch(const Context &context, const std::vector<unsigned char> &bits)
{
    detail::ensureDevice();
    CiphertextBatch out = BatchAccess::make(context, bits.size(), 1);
    if (bits.empty())
        return out;
    std::shared_ptr<DevicePayload> plain = uploadBits(bits);
    detail::check(csgn_const_fill(context.getN(), bits.size(), reinterpret_cast<const uint8_t *>(plain->data()), 0,
                                  BatchAccess::words(out), detail::stream()),
                  "csgn_const_fill");
    return out;
}

// Uniform operands: one fused call.  Ragged ones (compact() output): the definition itself, through the ragged
// operators, with a uniform batch of constants as the 1-term operand.
CiphertextBatch logicNot(const CiphertextBatch &a)
{
    if (a.uniform())
        return uniformGate(CSGN_GATE_NOT, nullptr, a, nullptr, nullptr);
    return a + ones(a);
}

CiphertextBatch logicXnor(const CiphertextBatch &a, const CiphertextBatch &b)
{
    requireSame(a, b, "logicXnor");
    if (a.uniform() && b.uniform())
        return uniformGate(CSGN_GATE_XNOR, nullptr, a, &b, nullptr);
    return (a + b) + ones(a);
}

CiphertextBatch logicNand(const CiphertextBatch &a, const CiphertextBatch &b)
{
    requireSame(a, b, "logicNand");
    if (a.uniform() && b.uniform())
        return uniformGate(CSGN_GATE_NAND, nullptr, a, &b, nullptr);
    return (a * b) + ones(a);
}

CiphertextBatch logicOr(const CiphertextBatch &a, const CiphertextBatch &b)
{
    requireSame(a, b, "logicOr");
    if (a.uniform() && b.uniform())
        return uniformGate(CSGN_GATE_OR, nullptr, a, &b, nullptr);
    return (a + b) + (a * b);
}

CiphertextBatch logicNor(const CiphertextBatch &a, const CiphertextBatch &b)
{
    requireSame(a, b, "logicNor");
    if (a.uniform() && b.uniform())
        return uniformGate(CSGN_GATE_NOR, nullptr, a, &b, nullptr);
    return ((a + b) + (a * b)) + ones(a);
}

CiphertextBatch logicMux(const CiphertextBatch &sel, const CiphertextBatch &a, const CiphertextBatch &b)
{
    requireSame(a, b, "logicMux");
    requireSame(sel, a, "logicMux");
    if (sel.uniform() && a.uniform() && b.uniform())
        return uniformGate(CSGN_GATE_MUX, &sel, a, &b, nullptr);
    return (sel * (a + b)) + b;
}

CiphertextBatch addPlain(const CiphertextBatch &a, const std::vector<unsigned char> &bits)
{
    if (bits.size() != a.size())
        throw std::invalid_argument("certFHE::addPlain: one bit per element expected");
    if (!a.uniform())
        return a + constantBatch(a.context(), bits);
    std::shared_ptr<DevicePayload> plain = uploadBits(bits);
    return uniformGate(CSGN_GATE_ADD_PLAIN, nullptr, a, nullptr, plain.get());
}

CiphertextBatch mulPlain(const CiphertextBatch &a, const std::vector<unsigned char> &bits)
{
    if (bits.size() != a.size())
        throw std::invalid_argument("certFHE::mulPlain: one bit per element expected");
    if (!a.uniform())
        return a * constantBatch(a.context(), bits);
    std::shared_ptr<DevicePayload> plain = uploadBits(bits);
    return uniformGate(CSGN_GATE_MUL_PLAIN, nullptr, a, nullptr, plain.get());
}

// ------------------------------------------------------------------ single ciphertexts

Ciphertext constantCiphertext(const Context &context, unsigned char bit)
{
    const uint64_t n = context.getN(), dl = context.getDefaultN();
    std::vector<uint64_t> v(dl, (bit & 1) ? ~0ull : 0ull), bitlen(dl);
    if ((bit & 1) && n % 64)
        v[dl - 1] = ~0ull << (64 - n % 64);
    detail::check(csgn_bitlen_canonical(n, 1, bitlen.data()), "csgn_bitlen_canonical");
    return Ciphertext(v.data(), bitlen.data(), dl, context);
}

namespace {
Ciphertext one(const Ciphertext &like) { return constantCiphertext(like.getContext(), 1); }
} // namespace

Ciphertext logicNot(const Ciphertext &a) { return a + one(a); }
Ciphertext logicXnor(const Ciphertext &a, const Ciphertext &b) { return (a + b) + one(a); }
Ciphertext logicNand(const Ciphertext &a, const Ciphertext &b) { return (a * b) + one(a); }
Ciphertext logicOr(const Ciphertext &a, const Ciphertext &b) { return (a + b) + (a * b); }
Ciphertext logicNor(const Ciphertext &a, const Ciphertext &b) { return ((a + b) + (a * b)) + one(a); }
Ciphertext logicMux(const Ciphertext &sel, const Ciphertext &a, const Ciphertext &b) { return (sel * (a + b)) + b; }
Ciphertext addPlain(const Ciphertext &a, unsigned char bit) { return a + constantCiphertext(a.getContext(), bit); }
Ciphertext mulPlain(const Ciphertext &a, unsigned char bit) { return a * constantCiphertext(a.getContext(), bit); }

// ------------------------------------------------------------------ BatchCircuit

void BatchCircuit::fillConstant(const ConstInput &c)
{
    uint64_t *dst = csgn_circuit_value(handle, c.id);
    if (!dst)
        throw std::logic_error("certFHE::BatchCircuit: a constant input has no buffer");
    detail::check(csgn_const_fill(ctx.getN(), count_, c.plain ? reinterpret_cast<const uint8_t *>(c.plain->data()) : nullptr,
                                  c.bit, dst, detail::stream()),
                  "csgn_const_fill");
}

unsigned BatchCircuit::constant(unsigned char bit)
{
    ConstInput c;
    c.id = input(1);
    c.bit = bit & 1;
    consts.push_back(c);
    return c.id;
}

unsigned BatchCircuit::plainInput()
{
    ConstInput c;
    c.id = input(1);
    c.bit = 0;
    c.plain = uploadBits(std::vector<unsigned char>(count_, 0));
    consts.push_back(c);
    return c.id;
}

void BatchCircuit::setPlainBits(unsigned plain_input, const std::vector<unsigned char> &bits)
{
    if (bits.size() != count_)
        throw std::invalid_argument("certFHE::BatchCircuit::setPlainBits: one bit per element expected");
    for (size_t i = 0; i < consts.size(); ++i)
        if (consts[i].id == plain_input && consts[i].plain) {
            if (!bits.empty())
                detail::check(csgn_memcpy_h2d(consts[i].plain->data(), bits.data(), bits.size(), detail::stream()),
                              "csgn_memcpy_h2d");
            if (csgn_circuit_value(handle, plain_input))           // built: refill now (stream order: before any later run)
                fillConstant(consts[i]);
            detail::check(csgn_stream_sync(detail::stream()), "csgn_stream_sync");
            return;
        }
    throw std::invalid_argument("certFHE::BatchCircuit::setPlainBits: not a plain input of this circuit");
}

unsigned BatchCircuit::logicNot(unsigned a)
{
    if (one_id == ~0u)
        one_id = constant(1);
    return add(a, one_id);
}

unsigned BatchCircuit::logicXnor(unsigned a, unsigned b) { return logicNot(add(a, b)); }
unsigned BatchCircuit::logicNand(unsigned a, unsigned b) { return logicNot(mul(a, b)); }
unsigned BatchCircuit::logicOr(unsigned a, unsigned b) { return add(add(a, b), mul(a, b)); }
unsigned BatchCircuit::logicNor(unsigned a, unsigned b) { return logicNot(logicOr(a, b)); }
unsigned BatchCircuit::logicMux(unsigned sel, unsigned a, unsigned b) { return add(mul(sel, add(a, b)), b); }

} // namespace certFHE
