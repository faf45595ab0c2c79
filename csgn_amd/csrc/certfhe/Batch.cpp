// Batch.cpp -- uniform device-resident batches over the C ABI (extension, see Batch.h).
#include "Batch.h"

#include "runtime.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace certFHE {

using detail::DevicePayload;

namespace {
void requireSameShape(const Context &a, const Context &b, uint64_t ca, uint64_t cb)
{
    if (a.getN() != b.getN() || ca != cb)
        throw std::invalid_argument("certFHE::CiphertextBatch: operands differ in N or element count");
}
} // namespace

CiphertextBatch::CiphertextBatch(const Context &c, uint64_t count, uint64_t terms)
    : count_(count), terms_(terms), ctx(c)
{
    payload = detail::allocWords(count * terms * c.getDefaultN());
}

const uint64_t *CiphertextBatch::deviceValues() const { return payload ? payload->data() : nullptr; }

uint64_t CiphertextBatch::termsOf(uint64_t i) const
{
    if (i >= count_)
        throw std::out_of_range("certFHE::CiphertextBatch::termsOf");
    return uniform() ? terms_ : offsets_[i + 1] - offsets_[i];
}

uint64_t CiphertextBatch::maxTerms() const
{
    if (uniform())
        return terms_;
    uint64_t m = 0;
    for (uint64_t i = 0; i < count_; ++i)
        m = std::max(m, offsets_[i + 1] - offsets_[i]);
    return m;
}

const uint64_t *CiphertextBatch::deviceOffsets() const
{
    if (!d_offsets_) {
        if (uniform()) {
            std::vector<uint64_t> off(count_ + 1);
            for (uint64_t i = 0; i <= count_; ++i)
                off[i] = i * terms_;
            d_offsets_ = detail::uploadWords(off.data(), off.size());
        } else {
            d_offsets_ = detail::uploadWords(offsets_.data(), offsets_.size());
        }
    }
    return d_offsets_->data();
}

CiphertextBatch CiphertextBatch::compact() const
{
    const uint64_t total = totalTerms(), n = ctx.getN(), dl = ctx.getDefaultN();
    CiphertextBatch out(ctx, count_, 0);
    out.terms_ = terms_;
    if (count_ == 0 || total == 0) {
        out.offsets_ = offsets_;
        return out;
    }
    out.payload = detail::allocWords(total * dl);                  // room for "nothing cancels"
    std::shared_ptr<DevicePayload> off_out = detail::allocWords(count_ + 1);
    const size_t need = csgn_compact_scratch_bytes(n, count_, total);
    if (need == 0)
        throw std::runtime_error("certFHE::CiphertextBatch::compact: context not supported by csgn_compact_ragged");
    std::shared_ptr<DevicePayload> work = detail::allocBytes(need);
    detail::check(csgn_compact_ragged(n, count_, total, maxTerms(), deviceValues(), deviceOffsets(),
                                      out.payload->data(), off_out->data(), work->ptr, detail::stream()),
                  "csgn_compact_ragged");
    std::vector<uint64_t> off(count_ + 1);
    detail::downloadBytes(off.data(), off_out->data(), (count_ + 1) * 8);      // synchronises
    bool same = true;
    for (uint64_t i = 1; i < count_ && same; ++i)
        same = off[i + 1] - off[i] == off[1] - off[0];
    if (same) {                                                    // dense CSR of equal sizes IS the uniform layout
        out.terms_ = off[1] - off[0];
    } else {
        out.terms_ = 0;
        out.offsets_.swap(off);
        out.d_offsets_ = off_out;
    }
    return out;
}

namespace {
// encrypt `bits` under `key` with the keyed device generator (csgn_encrypt_keyed)
void encryptInto(uint64_t n_bits, uint64_t d, const uint64_t *key_indices, const uint64_t *device_mask,
                 const std::vector<unsigned char> &bits, const csgn_rng &rng, uint64_t first, uint64_t *d_out)
{
    const uint64_t count = bits.size();
    // staging: [key indices (d words)][plaintext bytes]
    std::vector<uint64_t> stage(d + (count + 7) / 8, 0);
    for (uint64_t i = 0; i < d; ++i)
        stage[i] = key_indices[i];
    memcpy(stage.data() + d, bits.data(), count);
    std::shared_ptr<DevicePayload> dstage = detail::uploadWords(stage.data(), stage.size());
    detail::check(csgn_encrypt_keyed(n_bits, d, count, first,
                                     reinterpret_cast<const uint8_t *>(dstage->data() + d), dstage->data(),
                                     device_mask, &rng, d_out, detail::stream()),
                  "csgn_encrypt_keyed");
    // the staging block held the secret indices: wipe it before it returns to the block cache, and
    // the host copy too (~SecretKey zeroises its own copies the same way, src/SecretKey.cpp:354-372)
    detail::check(csgn_memset(dstage->ptr, 0, stage.size() * 8, detail::stream()), "csgn_memset");
    detail::check(csgn_stream_sync(detail::stream()), "csgn_stream_sync");
    volatile uint64_t *wipe = stage.data();
    for (size_t i = 0; i < stage.size(); ++i)
        wipe[i] = 0;
}
} // namespace

CiphertextBatch CiphertextBatch::encrypt(const SecretKey &key, const std::vector<unsigned char> &bits)
{
    if (!key.certFHEContext)
        throw std::logic_error("certFHE::CiphertextBatch::encrypt: key has no Context");
    key.ensureMask();
    CiphertextBatch out(*key.certFHEContext, bits.size(), 1);
    if (bits.empty())
        return out;
    csgn_rng rng;                      // fresh 256-bit generator key + nonce from the OS for every batch
    detail::check(csgn_rng_from_os(&rng, 8), "csgn_rng_from_os");
    encryptInto(key.certFHEContext->getN(), (uint64_t)key.length, key.s, key.device_mask->data(), bits, rng, 0,
                out.payload->data());
    volatile uint32_t *wipe = rng.key;
    for (int i = 0; i < 8; ++i)
        wipe[i] = 0;
    return out;
}

CiphertextBatch CiphertextBatch::encrypt(const SecretKey &key, const std::vector<unsigned char> &bits,
                                         uint64_t seed, uint64_t first_ciphertext)
{
    if (!key.certFHEContext)
        throw std::logic_error("certFHE::CiphertextBatch::encrypt: key has no Context");
    key.ensureMask();
    CiphertextBatch out(*key.certFHEContext, bits.size(), 1);
    if (bits.empty())
        return out;
    csgn_rng rng;
    detail::check(csgn_rng_from_seed(&rng, seed, 8), "csgn_rng_from_seed");
    encryptInto(key.certFHEContext->getN(), (uint64_t)key.length, key.s, key.device_mask->data(), bits, rng,
                first_ciphertext, out.payload->data());
    return out;
}

// The planes of an encrypted integer (UInt.h): ONE block of width * count ciphertexts, one upload, one csgn_encrypt_keyed
// from stream position 0 -- ciphertext j * count + i is element i of plane j, the position the per-plane seeded form
// gives it --, plane j a view at word j * count * dL.  With count * dL odd the views would sit on 8-byte boundaries and
// put every later kernel on its 8-byte path: such a batch (and an empty one) is encrypted plane by plane.
std::vector<CiphertextBatch> CiphertextBatch::encryptPlanes(const SecretKey &key, const std::vector<unsigned char> &bits,
                                                            uint64_t count, unsigned width, const uint64_t *seed)
{
    if (!key.certFHEContext)
        throw std::logic_error("certFHE::UIntBatch::encrypt: key has no Context");
    const Context &c = *key.certFHEContext;
    const uint64_t dl = c.getDefaultN();
    std::vector<CiphertextBatch> planes;
    if (count == 0 || (count * dl) % 2 != 0) {
        for (unsigned j = 0; j < width; ++j) {
            const std::vector<unsigned char> plane(bits.begin() + (size_t)j * count, bits.begin() + (size_t)(j + 1) * count);
            planes.push_back(seed ? encrypt(key, plane, *seed, (uint64_t)j * count) : encrypt(key, plane));
        }
        return planes;
    }
    key.ensureMask();
    std::shared_ptr<DevicePayload> block = detail::allocWords((uint64_t)width * count * dl);
    csgn_rng rng;
    if (seed)
        detail::check(csgn_rng_from_seed(&rng, *seed, 8), "csgn_rng_from_seed");
    else
        detail::check(csgn_rng_from_os(&rng, 8), "csgn_rng_from_os");
    encryptInto(c.getN(), (uint64_t)key.length, key.s, key.device_mask->data(), bits, rng, 0, block->data());
    volatile uint32_t *wipe = rng.key;
    for (int i = 0; i < 8; ++i)
        wipe[i] = 0;
    for (unsigned j = 0; j < width; ++j)
        planes.push_back(detail::BatchAccess::makeView(c, count, 1, block, (uint64_t)j * count * dl));
    return planes;
}

// One csgn_uint_decrypt over all planes, one copy of 8 bytes per element to the host, one synchronisation.
std::vector<uint64_t> CiphertextBatch::decryptPlanes(const std::vector<CiphertextBatch> &planes, const SecretKey &key)
{
    const uint64_t count = planes[0].size(), w = planes.size();
    std::vector<uint64_t> values(count, 0);
    if (count == 0)
        return values;
    key.ensureMask();
    std::vector<const uint64_t *> words(w), offsets(w, nullptr);
    std::vector<uint64_t> terms(w), totals(w, 0), bounds(w, 0);
    for (uint64_t j = 0; j < w; ++j) {
        const CiphertextBatch &p = planes[j];
        words[j] = p.deviceValues();
        terms[j] = p.uniform() ? p.terms_ : 0;
        if (terms[j] == 0) {                       // ragged, or a batch of no terms at all
            offsets[j] = p.deviceOffsets();
            totals[j] = p.totalTerms();
            bounds[j] = p.maxTerms();
        }
    }
    std::shared_ptr<DevicePayload> out = detail::allocWords(count);
    detail::check(csgn_uint_decrypt(planes[0].ctx.getN(), count, w, words.data(), terms.data(), offsets.data(),
                                    totals.data(), bounds.data(), key.device_mask->data(), out->data(), detail::stream()),
                  "csgn_uint_decrypt");
    detail::downloadBytes(values.data(), out->data(), count * 8);      // synchronises
    return values;
}

CiphertextBatch CiphertextBatch::pack(const std::vector<Ciphertext> &items)
{
    if (items.empty())
        throw std::invalid_argument("certFHE::CiphertextBatch::pack: empty list");
    const Context c = items[0].getContext();
    const uint64_t dl = c.getDefaultN(), terms = items[0].getTerms();
    CiphertextBatch out(c, items.size(), terms);
    for (size_t i = 0; i < items.size(); ++i) {
        if (items[i].getTerms() != terms || items[i].getLen() != terms * dl || !items[i].hasCanonicalBitlen())
            throw std::invalid_argument("certFHE::CiphertextBatch::pack: elements must share one shape");
        detail::check(csgn_memcpy_d2d(out.payload->data() + i * terms * dl, items[i].deviceValues(),
                                      (size_t)terms * dl * 8, detail::stream()),
                      "csgn_memcpy_d2d");
    }
    return out;
}

// ---------------------------------------------------------------------------------- data movement (csgn_gather*)

CiphertextBatch CiphertextBatch::gather(const std::vector<uint64_t> &indices) const
{
    for (size_t e = 0; e < indices.size(); ++e)
        if (indices[e] >= count_)
            throw std::out_of_range("certFHE::CiphertextBatch::gather: index " + std::to_string(indices[e]) +
                                    " past a batch of " + std::to_string(count_));
    const uint64_t n = indices.size(), dl = ctx.getDefaultN();
    if (uniform()) {
        CiphertextBatch out(ctx, n, terms_);
        if (n == 0 || terms_ == 0)
            return out;
        std::shared_ptr<DevicePayload> d_idx = detail::uploadWords(indices.data(), n);
        detail::check(csgn_gather(ctx.getN(), count_, deviceValues(), nullptr, terms_, n, d_idx->data(),
                                  out.payload->data(), nullptr, 0, detail::stream()),
                      "csgn_gather");
        return out;
    }
    CiphertextBatch out(ctx, n, 0);
    out.offsets_.assign(n + 1, 0);
    for (uint64_t e = 0; e < n; ++e)
        out.offsets_[e + 1] = out.offsets_[e] + termsOf(indices[e]);
    if (n == 0)
        return out;
    std::shared_ptr<DevicePayload> d_idx = detail::uploadWords(indices.data(), n);
    std::shared_ptr<DevicePayload> off_out = detail::allocWords(n + 1);
    uint64_t plan[2] = {0, 0};
    detail::check(csgn_gather_plan(count_, deviceOffsets(), n, d_idx->data(), off_out->data(), plan, detail::stream()),
                  "csgn_gather_plan");
    if (plan[0] != out.offsets_.back())
        throw std::logic_error("certFHE::CiphertextBatch::gather: device and host offsets disagree");
    out.payload = detail::allocWords(plan[0] * dl);
    out.d_offsets_ = off_out;
    if (plan[0])
        detail::check(csgn_gather(ctx.getN(), count_, deviceValues(), deviceOffsets(), 0, n, d_idx->data(),
                                  out.payload->data(), off_out->data(), plan[0], detail::stream()),
                      "csgn_gather");
    return out;
}

CiphertextBatch CiphertextBatch::slice(uint64_t begin, uint64_t end) const
{
    if (begin > end || end > count_)
        throw std::out_of_range("certFHE::CiphertextBatch::slice: [" + std::to_string(begin) + ", " + std::to_string(end) +
                                ") of a batch of " + std::to_string(count_));
    const uint64_t n = end - begin, dl = ctx.getDefaultN();
    const uint64_t t0 = uniform() ? begin * terms_ : offsets_[begin], t1 = uniform() ? end * terms_ : offsets_[end];
    CiphertextBatch out(ctx, n, uniform() ? terms_ : 0);
    if (!uniform()) {
        out.offsets_.resize(n + 1);
        for (uint64_t i = 0; i <= n; ++i)
            out.offsets_[i] = offsets_[begin + i] - t0;
        out.payload = detail::allocWords((t1 - t0) * dl);
    }
    if (t1 > t0)
        detail::check(csgn_memcpy_d2d(out.payload->data(), deviceValues() + t0 * dl, (size_t)(t1 - t0) * dl * 8,
                                      detail::stream()),
                      "csgn_memcpy_d2d");
    return out;
}

CiphertextBatch CiphertextBatch::broadcast(uint64_t count) const
{
    if (count_ != 1)
        throw std::invalid_argument("certFHE::CiphertextBatch::broadcast: the batch holds " + std::to_string(count_) +
                                    " elements, not 1");
    if (count >= (1ull << 32))
        throw std::invalid_argument("certFHE::CiphertextBatch::broadcast: 2^32 elements or more");
    const uint64_t t = uniform() ? terms_ : offsets_[1];
    if (!uniform()) {                                              // a ragged batch of one element stays ragged
        CiphertextBatch out(ctx, count, 0);
        out.offsets_.resize(count + 1);
        for (uint64_t i = 0; i <= count; ++i)
            out.offsets_[i] = i * t;
        if (count == 0)
            return out;
        std::shared_ptr<DevicePayload> off_out = detail::allocWords(count + 1);
        uint64_t plan[2] = {0, 0};
        detail::check(csgn_gather_plan(1, deviceOffsets(), count, nullptr, off_out->data(), plan, detail::stream()),
                      "csgn_gather_plan");
        out.payload = detail::allocWords(plan[0] * ctx.getDefaultN());
        out.d_offsets_ = off_out;
        if (plan[0])
            detail::check(csgn_gather(ctx.getN(), 1, deviceValues(), deviceOffsets(), 0, count, nullptr,
                                      out.payload->data(), off_out->data(), plan[0], detail::stream()),
                          "csgn_gather");
        return out;
    }
    CiphertextBatch out(ctx, count, t);
    if (count && t)
        detail::check(csgn_gather(ctx.getN(), 1, deviceValues(), nullptr, t, count, nullptr, out.payload->data(),
                                  nullptr, 0, detail::stream()),
                      "csgn_gather");
    return out;
}

CiphertextBatch CiphertextBatch::concat(const std::vector<CiphertextBatch> &parts)
{
    if (parts.empty())
        throw std::invalid_argument("certFHE::CiphertextBatch::concat: no parts");
    const Context &c = parts[0].ctx;
    bool same_terms = true;
    uint64_t count = 0, total = 0;
    for (size_t k = 0; k < parts.size(); ++k) {
        if (parts[k].ctx.getN() != c.getN() || parts[k].ctx.getD() != c.getD())
            throw std::invalid_argument("certFHE::CiphertextBatch::concat: parts differ in context");
        same_terms = same_terms && parts[k].uniform() && parts[k].terms_ == parts[0].terms_;
        count += parts[k].count_;
        total += parts[k].totalTerms();
    }
    const uint64_t dl = c.getDefaultN();
    CiphertextBatch out(c, count, same_terms ? parts[0].terms_ : 0);
    if (!same_terms) {
        out.offsets_.reserve(count + 1);
        out.offsets_.push_back(0);
        for (size_t k = 0; k < parts.size(); ++k)
            for (uint64_t i = 0; i < parts[k].count_; ++i)
                out.offsets_.push_back(out.offsets_.back() + parts[k].termsOf(i));
        out.payload = detail::allocWords(total * dl);
    }
    uint64_t at = 0;
    for (size_t k = 0; k < parts.size(); ++k) {
        const uint64_t words = parts[k].totalTerms() * dl;
        if (words)
            detail::check(csgn_memcpy_d2d(out.payload->data() + at, parts[k].deviceValues(), (size_t)words * 8,
                                          detail::stream()),
                          "csgn_memcpy_d2d");
        at += words;
    }
    return out;
}

CiphertextBatch CiphertextBatch::operator*(const CiphertextBatch &rhs) const
{
    requireSameShape(ctx, rhs.ctx, count_, rhs.count_);
    if (!uniform() || !rhs.uniform()) {                            // CSR kernels: plan, then multiply
        CiphertextBatch out(ctx, count_, 0);
        if (count_ == 0)
            return out;
        std::shared_ptr<DevicePayload> off_out = detail::allocWords(count_ + 1);
        uint64_t plan[4] = {0, 0, 0, 0};
        detail::check(csgn_mul_ragged_plan(count_, deviceOffsets(), rhs.deviceOffsets(), off_out->data(), plan,
                                           detail::stream()),
                      "csgn_mul_ragged_plan");
        out.payload = detail::allocWords(plan[0] * ctx.getDefaultN());
        if (plan[0])
            detail::check(csgn_mul_ragged(ctx.getN(), count_, deviceValues(), deviceOffsets(), rhs.deviceValues(),
                                          rhs.deviceOffsets(), out.payload->data(), off_out->data(), plan[1], plan[2],
                                          plan[0], detail::stream()),
                          "csgn_mul_ragged");
        out.offsets_.resize(count_ + 1);
        for (uint64_t i = 0, run = 0; i <= count_; ++i) {
            out.offsets_[i] = run;
            if (i < count_)
                run += termsOf(i) * rhs.termsOf(i);
        }
        out.d_offsets_ = off_out;
        return out;
    }
    CiphertextBatch out(ctx, count_, terms_ * rhs.terms_);
    detail::check(csgn_mul_uniform(ctx.getN(), count_, terms_, rhs.terms_, deviceValues(),
                                   rhs.deviceValues(), out.payload->data(), 0, detail::stream()),
                  "csgn_mul_uniform");
    return out;
}

CiphertextBatch CiphertextBatch::operator+(const CiphertextBatch &rhs) const
{
    requireSameShape(ctx, rhs.ctx, count_, rhs.count_);
    if (!uniform() || !rhs.uniform()) {
        CiphertextBatch out(ctx, count_, 0);
        if (count_ == 0)
            return out;
        const uint64_t total = totalTerms() + rhs.totalTerms();
        std::shared_ptr<DevicePayload> off_out = detail::allocWords(count_ + 1);
        out.payload = detail::allocWords(total * ctx.getDefaultN());
        detail::check(csgn_add_ragged_bounded(ctx.getN(), count_, maxTerms(), rhs.maxTerms(), deviceValues(), deviceOffsets(),
                                              rhs.deviceValues(), rhs.deviceOffsets(), out.payload->data(), off_out->data(), total,
                                              detail::stream()),
                      "csgn_add_ragged_bounded");
        out.offsets_.resize(count_ + 1);
        for (uint64_t i = 0, run = 0; i <= count_; ++i) {
            out.offsets_[i] = run;
            if (i < count_)
                run += termsOf(i) + rhs.termsOf(i);
        }
        out.d_offsets_ = off_out;
        return out;
    }
    CiphertextBatch out(ctx, count_, terms_ + rhs.terms_);
    detail::check(csgn_add_uniform(ctx.getN(), count_, terms_, rhs.terms_, deviceValues(),
                                   rhs.deviceValues(), out.payload->data(), detail::stream()),
                  "csgn_add_uniform");
    return out;
}

namespace {
// N uint32 permutation entries in HBM (two per uploaded word)
std::shared_ptr<DevicePayload> uploadPermutation(const Permutation &p, uint64_t n, const char *who)
{
    if (p.getLength() < n)
        throw std::invalid_argument(std::string(who) + ": permutation shorter than N");
    std::vector<uint64_t> packed((n + 1) / 2, 0);
    const uint64_t *src = p.getPermutation();
    for (uint64_t i = 0; i < n; ++i)
        packed[i / 2] |= (uint64_t)(uint32_t)src[i] << (32 * (i % 2));
    return detail::uploadWords(packed.data(), packed.size());
}
} // namespace

CiphertextBatch CiphertextBatch::applyPermutation(const Permutation &permutation) const
{
    if (!uniform())
        throw std::logic_error("certFHE::CiphertextBatch::applyPermutation: uniform batches only");
    CiphertextBatch out(ctx, count_, 1);
    if (count_ == 0)
        return out;
    std::shared_ptr<DevicePayload> d = uploadPermutation(permutation, ctx.getN(), "certFHE::CiphertextBatch::applyPermutation");
    detail::check(csgn_permute_uniform(ctx.getN(), count_, terms_, 0, deviceValues(),
                                       reinterpret_cast<const uint32_t *>(d->data()), out.payload->data(),
                                       detail::stream()),
                  "csgn_permute_uniform");
    detail::syncDevice();               // the permutation table is released on return
    return out;
}

std::vector<unsigned char> CiphertextBatch::decrypt(const SecretKey &key) const
{
    std::vector<unsigned char> bits(count_, 0);
    if (count_ == 0)
        return bits;
    key.ensureMask();
    const size_t scratch = (csgn_decrypt_scratch_bytes(count_, totalTerms()) + 255) & ~(size_t)255;
    std::shared_ptr<DevicePayload> work = detail::allocBytes(scratch + count_);
    uint8_t *d_bits = static_cast<uint8_t *>(work->ptr) + scratch;
    if (uniform())
        detail::check(csgn_decrypt_uniform(ctx.getN(), count_, terms_, deviceValues(), key.device_mask->data(),
                                           d_bits, work->ptr, detail::stream()),
                      "csgn_decrypt_uniform");
    else
        detail::check(csgn_decrypt_ragged_bounded(ctx.getN(), count_, totalTerms(), maxTerms(), deviceValues(), deviceOffsets(),
                                                  key.device_mask->data(), d_bits, work->ptr, detail::stream()),
                      "csgn_decrypt_ragged_bounded");
    detail::downloadBytes(bits.data(), d_bits, count_);
    return bits;
}

static std::vector<unsigned char> fusedDecrypt(const CiphertextBatch &a, const CiphertextBatch &b,
                                               const uint64_t *mask, bool product)
{
    std::vector<unsigned char> bits(a.size(), 0);
    if (a.size() == 0)
        return bits;
    const size_t scratch =
        (csgn_decrypt_combined_scratch_bytes(a.size(), a.terms(), b.terms()) + 255) & ~(size_t)255;
    std::shared_ptr<DevicePayload> work = detail::allocBytes(scratch + a.size());
    uint8_t *d_bits = static_cast<uint8_t *>(work->ptr) + scratch;
    const uint64_t n = a.context().getN();
    detail::check(product ? csgn_decrypt_product_uniform(n, a.size(), a.terms(), b.terms(), a.deviceValues(),
                                                         b.deviceValues(), mask, d_bits, work->ptr,
                                                         detail::stream())
                          : csgn_decrypt_sum_uniform(n, a.size(), a.terms(), b.terms(), a.deviceValues(),
                                                     b.deviceValues(), mask, d_bits, work->ptr,
                                                     detail::stream()),
                  "csgn_decrypt_{product,sum}_uniform");
    detail::downloadBytes(bits.data(), d_bits, a.size());
    return bits;
}

std::vector<unsigned char> CiphertextBatch::decryptProduct(const CiphertextBatch &rhs,
                                                           const SecretKey &key) const
{
    requireSameShape(ctx, rhs.ctx, count_, rhs.count_);
    if (!uniform() || !rhs.uniform())
        throw std::logic_error("certFHE::CiphertextBatch::decryptProduct: uniform batches only");
    key.ensureMask();
    return fusedDecrypt(*this, rhs, key.device_mask->data(), true);
}

std::vector<unsigned char> CiphertextBatch::decryptSum(const CiphertextBatch &rhs, const SecretKey &key) const
{
    requireSameShape(ctx, rhs.ctx, count_, rhs.count_);
    if (!uniform() || !rhs.uniform())
        throw std::logic_error("certFHE::CiphertextBatch::decryptSum: uniform batches only");
    key.ensureMask();
    return fusedDecrypt(*this, rhs, key.device_mask->data(), false);
}

Ciphertext CiphertextBatch::at(uint64_t i) const
{
    if (i >= count_)
        throw std::out_of_range("certFHE::CiphertextBatch::at");
    const uint64_t dl = ctx.getDefaultN(), words = termsOf(i) * dl;
    const uint64_t first = (uniform() ? i * terms_ : offsets_[i]) * dl;
    std::shared_ptr<DevicePayload> p = detail::allocWords(words);
    if (words)
        detail::check(csgn_memcpy_d2d(p->data(), deviceValues() + first, (size_t)words * 8, detail::stream()),
                      "csgn_memcpy_d2d");
    Ciphertext c;
    c.certFHEcontext = new Context(ctx);
    c.publish(p, words);
    return c;
}

// ------------------------------------------------------------------ sums over elements, matrix products (csgn_matmul)

CiphertextBatch CiphertextBatch::sumGroups(uint64_t group) const
{
    if (group == 0 || count_ % group != 0)
        throw std::invalid_argument("certFHE::CiphertextBatch::sumGroups: groups of " + std::to_string(group) +
                                    " in a batch of " + std::to_string(count_));
    CiphertextBatch out(ctx, 0, 0);
    out.payload = payload;                                         // a sum is a concatenation: the same words
    out.count_ = count_ / group;
    if (uniform()) {
        out.terms_ = terms_ * group;
        return out;
    }
    out.offsets_.resize(out.count_ + 1);
    for (uint64_t q = 0; q <= out.count_; ++q)
        out.offsets_[q] = offsets_[q * group];
    return out;
}

namespace {
CiphertextBatch matMulAny(const CiphertextBatch &a, const CiphertextBatch &b, uint64_t rows, uint64_t inner,
                          uint64_t cols, bool transposed, const char *who)
{
    const std::string name = std::string("certFHE::") + who;
    const Context &c = a.context();
    if (c.getN() != b.context().getN() || c.getD() != b.context().getD())
        throw std::invalid_argument(name + ": operands differ in context");
    unsigned long long na, nb, nc;
    if (rows == 0 || inner == 0 || cols == 0 || __builtin_mul_overflow((unsigned long long)rows, (unsigned long long)inner, &na) ||
        __builtin_mul_overflow((unsigned long long)inner, (unsigned long long)cols, &nb) ||
        __builtin_mul_overflow((unsigned long long)rows, (unsigned long long)cols, &nc) || a.size() != na || b.size() != nb)
        throw std::invalid_argument(name + ": " + std::to_string(rows) + " x " + std::to_string(inner) + " times " +
                                    std::to_string(inner) + " x " + std::to_string(cols) + " from batches of " +
                                    std::to_string(a.size()) + " and " + std::to_string(b.size()));
    const uint64_t dl = c.getDefaultN();
    if (a.uniform() && b.uniform()) {
        const uint64_t T = csgn_matmul_terms(inner, a.terms(), b.terms());
        if (a.terms() == 0 || b.terms() == 0)
            throw std::invalid_argument(name + ": an operand of no terms");
        if (T == 0 || T > ((1ull << 31) - 1) / dl)
            throw std::invalid_argument(name + ": an output element past 2^31 words");
        CiphertextBatch out = detail::BatchAccess::make(c, nc, T);
        detail::check(csgn_matmul(c.getN(), rows, inner, cols, a.deviceValues(), a.terms(), b.deviceValues(), b.terms(),
                                  transposed ? 1 : 0, detail::BatchAccess::words(out), detail::stream()),
                      "csgn_matmul");
        return out;
    }
    // a ragged operand: the definition itself, from gather, operator* and sumGroups.  The size of every output element
    // first, from the host's term counts.
    if (na >= (1ull << 32) || nb >= (1ull << 32) || nc >= (1ull << 32) / inner)
        throw std::invalid_argument(name + ": ragged operands of 2^32 elements or more");
    for (uint64_t i = 0; i < rows; ++i)
        for (uint64_t k = 0; k < cols; ++k) {
            unsigned long long T = 0;
            for (uint64_t e = 0; e < inner; ++e) {
                unsigned long long p;
                if (__builtin_mul_overflow((unsigned long long)a.termsOf(i * inner + e),
                                           (unsigned long long)b.termsOf(transposed ? k * inner + e : e * cols + k), &p) ||
                    __builtin_add_overflow(T, p, &T))
                    T = ~0ull;
            }
            if (T > ((1ull << 31) - 1) / dl)
                throw std::invalid_argument(name + ": an output element past 2^31 words");
        }
    std::vector<uint64_t> ia(nc * inner), ib(nc * inner);
    for (uint64_t i = 0, p = 0; i < rows; ++i)
        for (uint64_t k = 0; k < cols; ++k)
            for (uint64_t e = 0; e < inner; ++e, ++p) {
                ia[p] = i * inner + e;
                ib[p] = transposed ? k * inner + e : e * cols + k;
            }
    return (a.gather(ia) * b.gather(ib)).sumGroups(inner);
}
} // namespace

CiphertextBatch matMul(const CiphertextBatch &a, const CiphertextBatch &b, uint64_t rows, uint64_t inner, uint64_t cols)
{
    return matMulAny(a, b, rows, inner, cols, false, "matMul");
}

CiphertextBatch matMulTransposed(const CiphertextBatch &a, const CiphertextBatch &bt, uint64_t rows, uint64_t inner,
                                 uint64_t cols)
{
    return matMulAny(a, bt, rows, inner, cols, true, "matMulTransposed");
}

CiphertextBatch dot(const CiphertextBatch &a, const CiphertextBatch &b)
{
    return matMulAny(a, b, 1, a.size(), 1, true, "dot");
}

// ------------------------------------------------------------------ BatchCircuit

BatchCircuit::BatchCircuit(const Context &context, uint64_t count)
    : handle(nullptr), ctx(context), count_(count), next_first(0), one_id(~0u)
{
    detail::ensureDevice();
    detail::check(csgn_circuit_create(ctx.getN(), count, &handle), "csgn_circuit_create");
}

BatchCircuit::~BatchCircuit()
{
    if (handle) {
        detail::syncDevice();           // a launch of the graph may still be running
        csgn_circuit_destroy(handle);
    }
}

unsigned BatchCircuit::input(uint64_t terms)
{
    uint32_t id = 0;
    detail::check(csgn_circuit_input(handle, terms, &id), "csgn_circuit_input");
    return id;
}

unsigned BatchCircuit::encryptInput(const SecretKey &key)
{
    if (!key.certFHEContext || key.certFHEContext->getN() != ctx.getN())
        throw std::invalid_argument("certFHE::BatchCircuit::encryptInput: key and circuit differ in N");
    key.ensureMask();
    masks.push_back(key.device_mask);
    const uint64_t d = (uint64_t)key.length;
    // one block: [key indices (d words)][plaintext bytes, zero until setPlain()]
    std::vector<uint64_t> stage(d + (count_ + 7) / 8, 0);
    for (uint64_t i = 0; i < d; ++i)
        stage[i] = key.s[i];
    std::shared_ptr<DevicePayload> blk = detail::uploadWords(stage.data(), stage.size());
    volatile uint64_t *wipe = stage.data();
    for (uint64_t i = 0; i < d; ++i)
        wipe[i] = 0;
    masks.push_back(blk);
    csgn_rng rng;
    detail::check(csgn_rng_from_os(&rng, 8), "csgn_rng_from_os");
    uint32_t id = 0;
    detail::check(csgn_circuit_encrypt(handle, d, reinterpret_cast<const uint8_t *>(blk->data() + d), blk->data(),
                                       key.device_mask->data(), &rng, next_first, &id),
                  "csgn_circuit_encrypt");
    volatile uint32_t *wk = rng.key;
    for (int i = 0; i < 8; ++i)
        wk[i] = 0;
    next_first += (uint64_t)1 << 40;                // every encrypt input draws from its own range
    plains.push_back(std::make_pair((unsigned)id, blk));
    return id;
}

unsigned BatchCircuit::encryptProduct(const SecretKey &key, unsigned *bits_id)
{
    if (!key.certFHEContext || key.certFHEContext->getN() != ctx.getN())
        throw std::invalid_argument("certFHE::BatchCircuit::encryptProduct: key and circuit differ in N");
    key.ensureMask();
    masks.push_back(key.device_mask);
    const uint64_t d = (uint64_t)key.length, pw = (count_ + 7) / 8;
    // one block: [key indices (d words)][plaintext bytes of a][plaintext bytes of b], zero until setPlainPair()
    std::vector<uint64_t> stage(d + 2 * pw, 0);
    for (uint64_t i = 0; i < d; ++i)
        stage[i] = key.s[i];
    std::shared_ptr<DevicePayload> blk = detail::uploadWords(stage.data(), stage.size());
    volatile uint64_t *wipe = stage.data();
    for (uint64_t i = 0; i < d; ++i)
        wipe[i] = 0;
    masks.push_back(blk);
    csgn_rng ra, rb;                                  // two independent generator keys from the OS
    detail::check(csgn_rng_from_os(&ra, 8), "csgn_rng_from_os");
    detail::check(csgn_rng_from_os(&rb, 8), "csgn_rng_from_os");
    uint32_t id = 0, bid = 0;
    const uint8_t *pa = reinterpret_cast<const uint8_t *>(blk->data() + d);
    detail::check(csgn_circuit_encrypt_mul(handle, d, pa, pa + pw * 8, blk->data(), key.device_mask->data(), &ra, &rb,
                                           next_first, &id, bits_id ? &bid : nullptr),
                  "csgn_circuit_encrypt_mul");
    volatile uint32_t *wa = ra.key, *wb = rb.key;
    for (int i = 0; i < 8; ++i)
        wa[i] = wb[i] = 0;
    next_first += (uint64_t)1 << 40;
    pair_plains.push_back(std::make_pair((unsigned)id, blk));
    if (bits_id)
        *bits_id = bid;
    return id;
}

void BatchCircuit::setPlainPair(unsigned product, const std::vector<unsigned char> &a, const std::vector<unsigned char> &b)
{
    if (a.size() != count_ || b.size() != count_)
        throw std::invalid_argument("certFHE::BatchCircuit::setPlainPair: one bit of each operand per element expected");
    const uint64_t pw = (count_ + 7) / 8;
    for (size_t i = 0; i < pair_plains.size(); ++i)
        if (pair_plains[i].first == product) {
            const uint64_t d_words = pair_plains[i].second->words - 2 * pw;
            detail::check(csgn_memcpy_h2d(pair_plains[i].second->data() + d_words, a.data(), (size_t)count_, detail::stream()),
                          "csgn_memcpy_h2d");
            detail::check(csgn_memcpy_h2d(pair_plains[i].second->data() + d_words + pw, b.data(), (size_t)count_, detail::stream()),
                          "csgn_memcpy_h2d");
            detail::check(csgn_stream_sync(detail::stream()), "csgn_stream_sync");
            return;
        }
    throw std::invalid_argument("certFHE::BatchCircuit::setPlainPair: not a fused product of this circuit");
}

void BatchCircuit::setPlain(unsigned encrypted_input, const std::vector<unsigned char> &bits)
{
    if (bits.size() != count_)
        throw std::invalid_argument("certFHE::BatchCircuit::setPlain: one bit per element expected");
    for (size_t i = 0; i < plains.size(); ++i)
        if (plains[i].first == encrypted_input) {
            // the key indices occupy the first words of the block; the bytes follow
            const uint64_t d_words = plains[i].second->words - (count_ + 7) / 8;
            detail::check(csgn_memcpy_h2d(plains[i].second->data() + d_words, bits.data(), (size_t)count_,
                                          detail::stream()),
                          "csgn_memcpy_h2d");
            detail::check(csgn_stream_sync(detail::stream()), "csgn_stream_sync");
            return;
        }
    throw std::invalid_argument("certFHE::BatchCircuit::setPlain: not an encrypted input of this circuit");
}

unsigned BatchCircuit::add(unsigned a, unsigned b)
{
    uint32_t id = 0;
    detail::check(csgn_circuit_add(handle, a, b, &id), "csgn_circuit_add");
    return id;
}

unsigned BatchCircuit::mul(unsigned a, unsigned b)
{
    uint32_t id = 0;
    detail::check(csgn_circuit_mul(handle, a, b, &id), "csgn_circuit_mul");
    return id;
}

unsigned BatchCircuit::compact(unsigned a)
{
    uint32_t id = 0;
    detail::check(csgn_circuit_compact(handle, a, &id), "csgn_circuit_compact");
    return id;
}

unsigned BatchCircuit::permute(unsigned a, const Permutation &p)
{
    std::shared_ptr<DevicePayload> d = uploadPermutation(p, ctx.getN(), "certFHE::BatchCircuit::permute");
    masks.push_back(d);                 // the graph holds the pointer: keep the block alive
    uint32_t id = 0;
    detail::check(csgn_circuit_permute(handle, a, reinterpret_cast<const uint32_t *>(d->data()), &id),
                  "csgn_circuit_permute");
    return id;
}

unsigned BatchCircuit::decrypt(unsigned a, const SecretKey &key)
{
    key.ensureMask();
    masks.push_back(key.device_mask);   // the graph holds the pointer: keep the block alive
    uint32_t id = 0;
    detail::check(csgn_circuit_decrypt(handle, a, key.device_mask->data(), &id), "csgn_circuit_decrypt");
    return id;
}

void BatchCircuit::optimize(unsigned passes)
{
    detail::check(csgn_circuit_optimize(handle, passes), "csgn_circuit_optimize");
}

void BatchCircuit::keep(unsigned value) { detail::check(csgn_circuit_output(handle, value), "csgn_circuit_output"); }

uint64_t BatchCircuit::blockBytes() const { return csgn_circuit_block_bytes(handle); }

void BatchCircuit::build()
{
    detail::check(csgn_circuit_build(handle), "csgn_circuit_build");
    for (size_t i = 0; i < consts.size(); ++i)
        fillConstant(consts[i]);
}

void BatchCircuit::set(unsigned input, const CiphertextBatch &batch)
{
    const uint64_t terms = csgn_circuit_value_terms(handle, input);
    uint64_t *dst = csgn_circuit_value(handle, input);
    if (!dst || batch.size() != count_ || batch.terms() != terms || batch.context().getN() != ctx.getN())
        throw std::invalid_argument("certFHE::BatchCircuit::set: shape mismatch or circuit not built");
    detail::check(csgn_memcpy_d2d(dst, batch.deviceValues(), (size_t)(count_ * terms * ctx.getDefaultN() * 8),
                                  detail::stream()),
                  "csgn_memcpy_d2d");
}

void BatchCircuit::run() { detail::check(csgn_circuit_run(handle, detail::stream()), "csgn_circuit_run"); }

CiphertextBatch BatchCircuit::value(unsigned id) const
{
    const uint64_t terms = csgn_circuit_value_terms(handle, id);
    const uint64_t *src = csgn_circuit_value(handle, id);
    if (!src)
        throw std::invalid_argument("certFHE::BatchCircuit::value: no such value, circuit not built, or a value a compiled circuit did not keep()");
    const uint64_t *d_off = csgn_circuit_value_offsets(handle, id);
    if (terms == 0 && !d_off)
        throw std::invalid_argument("certFHE::BatchCircuit::value: no such value, circuit not built, or a value a compiled circuit did not keep()");
    if (d_off) {                                    // ragged (static shapes, or data-dependent ones behind compact())
        CiphertextBatch out(ctx, count_, 0);
        out.offsets_.resize(count_ + 1);
        detail::downloadBytes(out.offsets_.data(), d_off, (count_ + 1) * 8);      // synchronises
        const uint64_t words = out.offsets_.back() * ctx.getDefaultN();
        out.payload = detail::allocWords(words);
        if (words)
            detail::check(csgn_memcpy_d2d(out.payload->ptr, src, (size_t)words * 8, detail::stream()), "csgn_memcpy_d2d");
        return out;
    }
    CiphertextBatch out(ctx, count_, terms);
    detail::check(csgn_memcpy_d2d(out.payload->ptr, src, (size_t)(count_ * terms * ctx.getDefaultN() * 8),
                                  detail::stream()),
                  "csgn_memcpy_d2d");
    return out;
}

std::vector<unsigned char> BatchCircuit::bits(unsigned bits_id) const
{
    const uint8_t *src = csgn_circuit_bits(handle, bits_id);
    if (!src)
        throw std::invalid_argument("certFHE::BatchCircuit::bits: no such result or circuit not built");
    std::vector<unsigned char> out(count_, 0);
    detail::downloadBytes(out.data(), src, count_);
    return out;
}

} // namespace certFHE
