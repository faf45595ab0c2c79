// certfhe/Gates.h -- EXTENSION (not in the reference): plaintext constants and the boolean gates they make possible.
//
// `+` (XOR) and `*` (AND) both map 0 to 0, and whoever evaluates a circuit holds no key to encrypt a 1, so with the two
// operators alone no NOT, NAND, NOR, XNOR, equality or less-than can be computed.  A term decrypts to the AND of the
// key's positions in it (src/SecretKey.cpp:82-147): the ALL-ONES term decrypts to 1 under every key and the all-zero
// term to 0.  Adding or multiplying one of these CONSTANTS gives the missing gates.
//
// A constant is a TRIVIAL encryption: its plaintext is public.  An output that is only a constant (or that a gate has
// reduced to one) hides nothing.  Plain bits handed to addPlain / mulPlain / setPlainBits are public as well.
//
// Every gate is defined as a composition of the reference's operator+ / operator*, in this order, and produces exactly
// its words (include/csgn_hip.h, csgn_gate_uniform):
//     logicNot(a)        a + ONE
//     logicXnor(a, b)    (a + b) + ONE
//     logicNand(a, b)    (a * b) + ONE
//     logicOr(a, b)      (a + b) + (a * b)
//     logicNor(a, b)     ((a + b) + (a * b)) + ONE
//     logicMux(s, a, b)  (s * (a + b)) + b          s ? a : b
//     addPlain(a, p)     a + (p ? ONE : ZERO)
//     mulPlain(a, p)     a * (p ? ONE : ZERO)
// Uniform batches run one csgn_gate_uniform call (one fused kernel for fresh operands); ragged batches (what compact()
// may return) are composed from the ragged add / multiply with a constant batch.  Single ciphertexts are composed from
// their operators, so small ones join the deferred small-operation queue.
#ifndef CERTFHE_GATES_H
#define CERTFHE_GATES_H

#include <vector>

#include "Batch.h"
#include "Ciphertext.h"
#include "Context.h"

namespace certFHE {

// element i is ONE if bits[i] & 1, else ZERO (1 term each)
CiphertextBatch constantBatch(const Context &context, const std::vector<unsigned char> &bits);

CiphertextBatch logicNot(const CiphertextBatch &a);
CiphertextBatch logicNand(const CiphertextBatch &a, const CiphertextBatch &b);
CiphertextBatch logicOr(const CiphertextBatch &a, const CiphertextBatch &b);
CiphertextBatch logicNor(const CiphertextBatch &a, const CiphertextBatch &b);
CiphertextBatch logicXnor(const CiphertextBatch &a, const CiphertextBatch &b);
CiphertextBatch logicMux(const CiphertextBatch &sel, const CiphertextBatch &a, const CiphertextBatch &b);
CiphertextBatch addPlain(const CiphertextBatch &a, const std::vector<unsigned char> &bits);   // one bit per element
CiphertextBatch mulPlain(const CiphertextBatch &a, const std::vector<unsigned char> &bits);

// ONE (bit & 1) or ZERO as an ordinary 1-term ciphertext
Ciphertext constantCiphertext(const Context &context, unsigned char bit);

Ciphertext logicNot(const Ciphertext &a);
Ciphertext logicNand(const Ciphertext &a, const Ciphertext &b);
Ciphertext logicOr(const Ciphertext &a, const Ciphertext &b);
Ciphertext logicNor(const Ciphertext &a, const Ciphertext &b);
Ciphertext logicXnor(const Ciphertext &a, const Ciphertext &b);
Ciphertext logicMux(const Ciphertext &sel, const Ciphertext &a, const Ciphertext &b);
Ciphertext addPlain(const Ciphertext &a, unsigned char bit);
Ciphertext mulPlain(const Ciphertext &a, unsigned char bit);

} // namespace certFHE

#endif
