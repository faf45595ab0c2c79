// capi_stub_shard.cpp -- the entry points csgn_amd/csrc/certfhe_shard/ShardedBatch.cpp calls that capi_stub.cpp lacks
// (that file is pinned to the 30 of the seven base class sources): ten of include/csgn_hip.h and
// csgn_shard_product_counts of include/csgn_shard.h, whose real form is a kernel.  They compute on host memory through
// oracle/csgn_oracle.c, take the argument rules of csgn_amd/csrc/csgn_capi.hip in that file's order (batch 0 is CSGN_OK
// before any pointer is looked at, and so on), and use capi_stub's pointer / extent / device checks, call log, injected
// failures and stream hook (capi_stub.h).  The knobs are per host thread, as in the library; the names known here are
// the two the tests set.
#include "capi_stub.h"

#include <sys/random.h>

#include <cerrno>
#include <cstring>
#include <map>

#include "csgn_oracle.h"
#include "csgn_shard.h"

using namespace capi_stub;

namespace {

thread_local std::map<std::string, int> t_knobs;

bool known_knob(const char *key) { return !strcmp(key, "mul_flat") || !strcmp(key, "shared_gpu"); }

int refuse(int code, const char *text)
{
    stub_set_error(std::string("stub: ") + text);
    return code;
}

#define REQUIRE(cond, text)                          \
    do {                                             \
        if (!(cond))                                 \
            return refuse(CSGN_ERR_INVALID, text);   \
    } while (0)

#define STREAM(stream)                 \
    if (stub_stream_hook)              \
        stub_stream_hook(stream)

int check_n(uint64_t n_bits)
{
    if (n_bits == 0)
        return refuse(CSGN_ERR_INVALID, "n_bits must be > 0");
    if (((n_bits + 63) / 64) * 8 > 16384)
        return refuse(CSGN_ERR_UNSUPPORTED, "terms above 16384 bytes are not supported");
    return CSGN_OK;
}

bool good_rounds(uint32_t r) { return r == 8 || r == 12 || r == 20; }

std::vector<uint64_t> key_of(const uint64_t *mask, uint64_t n_bits)
{
    std::vector<uint64_t> key;
    for (uint64_t i = 0; i < n_bits; ++i)
        if ((mask[i >> 6] >> (63 - (i & 63))) & 1)
            key.push_back(i);
    return key;
}

int decrypt_combined(const char *entry, bool product, uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                     const uint64_t *d_left, const uint64_t *d_right, const uint64_t *d_mask, uint8_t *d_bits, void *d_scratch,
                     void *stream)
{
    STREAM(stream);
    if (int rc = stub_enter(entry, d_bits, d_left, (size_t)(t1 << 32 | t2), n_bits))
        return rc;
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_mask && d_bits && d_scratch && (d_left || t1 == 0) && (d_right || t2 == 0), "null device pointer");
    const uint64_t dl = csgn_oracle_default_len(n_bits);
    stub_check(entry, d_left, batch * t1 * dl * 8, kDevice);
    stub_check(entry, d_right, batch * t2 * dl * 8, kDevice);
    stub_check(entry, d_mask, dl * 8, kDevice);
    stub_check(entry, d_bits, batch, kDevice);
    stub_check(entry, d_scratch, csgn_decrypt_combined_scratch_bytes(batch, t1, t2), kDevice);
    const std::vector<uint64_t> key = key_of(d_mask, n_bits);
    const uint64_t terms = product ? t1 * t2 : t1 + t2;
    std::vector<uint64_t> tmp(terms * dl + 1);
    for (uint64_t b = 0; b < batch; ++b) {
        if (product)
            csgn_oracle_mul(dl, d_left + b * t1 * dl, t1 * dl, nullptr, d_right + b * t2 * dl, t2 * dl, tmp.data(), nullptr);
        else
            csgn_oracle_add(d_left + b * t1 * dl, t1 * dl, nullptr, d_right + b * t2 * dl, t2 * dl, nullptr, tmp.data(), nullptr);
        d_bits[b] = (uint8_t)csgn_oracle_decrypt_canonical(n_bits, key.size(), key.data(), tmp.data(), terms * dl);
    }
    return CSGN_OK;
}

} // namespace

extern "C" {

int csgn_set_tuning(const char *key, int value)
{
    if (int rc = stub_enter("csgn_set_tuning", key, nullptr, (size_t)value, 0))
        return rc;
    REQUIRE(key, "key is null");
    REQUIRE(known_knob(key), "csgn_set_tuning: no knob of that name");
    t_knobs[key] = value;
    return CSGN_OK;
}

int csgn_get_tuning(const char *key, int *h_value)
{
    if (int rc = stub_enter("csgn_get_tuning", key, nullptr, 0, 0))
        return rc;
    REQUIRE(key && h_value, "null argument");
    REQUIRE(known_knob(key), "csgn_get_tuning: no knob of that name");
    *h_value = t_knobs.count(key) ? t_knobs[key] : 0;
    return CSGN_OK;
}

int csgn_rng_from_seed(csgn_rng *h_rng, uint64_t seed, uint32_t rounds)
{
    if (int rc = stub_enter("csgn_rng_from_seed", h_rng, nullptr, 0, 0))
        return rc;
    REQUIRE(h_rng, "h_rng is null");
    REQUIRE(good_rounds(rounds), "rounds must be 8, 12 or 20");
    csgn_oracle_rng_from_seed(seed, h_rng->key, &h_rng->nonce);
    h_rng->rounds = rounds;
    h_rng->reserved = 0;
    return CSGN_OK;
}

int csgn_rng_from_os(csgn_rng *h_rng, uint32_t rounds)
{
    if (int rc = stub_enter("csgn_rng_from_os", h_rng, nullptr, 0, 0))
        return rc;
    REQUIRE(h_rng, "h_rng is null");
    REQUIRE(good_rounds(rounds), "rounds must be 8, 12 or 20");
    unsigned char buf[40];
    size_t got = 0;
    while (got < sizeof(buf)) {
        const ssize_t r = getrandom(buf + got, sizeof(buf) - got, 0);
        if (r < 0) {
            if (errno == EINTR)
                continue;
            return refuse(CSGN_ERR_INVALID, "getrandom failed");
        }
        got += (size_t)r;
    }
    memcpy(h_rng->key, buf, 32);
    memcpy(&h_rng->nonce, buf + 32, 8);
    h_rng->rounds = rounds;
    h_rng->reserved = 0;
    return CSGN_OK;
}

int csgn_encrypt_keyed(uint64_t n_bits, uint64_t d, uint64_t batch, uint64_t first_ciphertext, const uint8_t *d_plain,
                       const uint64_t *d_key, const uint64_t *d_mask, const csgn_rng *h_rng, uint64_t *d_out, void *stream)
{
    STREAM(stream);
    if (int rc = stub_enter("csgn_encrypt_keyed", d_out, d_plain, (size_t)batch, n_bits))
        return rc;
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_rng, "h_rng is null");
    REQUIRE(good_rounds(h_rng->rounds), "rng rounds must be 8, 12 or 20");
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d >= 1 && d < (1ull << 32), "d must be in [1, 2^32)");
    REQUIRE(d_plain && d_key && d_mask && d_out, "null device pointer");
    REQUIRE(first_ciphertext + batch >= first_ciphertext && first_ciphertext + batch < (1ull << 56), "ciphertext index range too large");
    const uint64_t dl = csgn_oracle_default_len(n_bits);
    stub_check("csgn_encrypt_keyed (the bits)", d_plain, batch, kDevice);
    stub_check("csgn_encrypt_keyed (the key)", d_key, d * 8, kDevice);
    stub_check("csgn_encrypt_keyed (the mask)", d_mask, dl * 8, kDevice);
    stub_check("csgn_encrypt_keyed (out)", d_out, batch * dl * 8, kDevice);
    csgn_oracle_encrypt_keyed(n_bits, d, d_key, batch, first_ciphertext, d_plain, h_rng->key, h_rng->nonce, h_rng->rounds, d_out);
    return CSGN_OK;
}

int csgn_encrypt_mul_keyed(uint64_t n_bits, uint64_t d, uint64_t batch, uint64_t first_ciphertext, const uint8_t *d_plain_a,
                           const uint8_t *d_plain_b, const uint64_t *d_key, const uint64_t *d_mask, const csgn_rng *h_rng_a,
                           const csgn_rng *h_rng_b, uint64_t *d_out, uint8_t *d_bits, void *stream)
{
    STREAM(stream);
    if (int rc = stub_enter("csgn_encrypt_mul_keyed", d_out, d_plain_a, (size_t)batch, n_bits))
        return rc;
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_rng_a && h_rng_b, "h_rng is null");
    REQUIRE(good_rounds(h_rng_a->rounds), "rng rounds must be 8, 12 or 20");
    REQUIRE(h_rng_a->rounds == h_rng_b->rounds, "both generators must use the same number of rounds");
    REQUIRE(memcmp(h_rng_a->key, h_rng_b->key, sizeof(h_rng_a->key)) != 0 || h_rng_a->nonce != h_rng_b->nonce,
            "the two operands must draw from different streams (same key AND nonce given)");
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d >= 1 && d < (1ull << 32), "d must be in [1, 2^32)");
    REQUIRE(d_plain_a && d_plain_b && d_key && d_mask && d_out, "null device pointer");
    REQUIRE(first_ciphertext + batch >= first_ciphertext && first_ciphertext + batch < (1ull << 56), "ciphertext index range too large");
    const uint64_t dl = csgn_oracle_default_len(n_bits);
    stub_check("csgn_encrypt_mul_keyed (the bits of a)", d_plain_a, batch, kDevice);
    stub_check("csgn_encrypt_mul_keyed (the bits of b)", d_plain_b, batch, kDevice);
    stub_check("csgn_encrypt_mul_keyed (the key)", d_key, d * 8, kDevice);
    stub_check("csgn_encrypt_mul_keyed (the mask)", d_mask, dl * 8, kDevice);
    stub_check("csgn_encrypt_mul_keyed (out)", d_out, batch * dl * 8, kDevice);
    if (d_bits)
        stub_check("csgn_encrypt_mul_keyed (the product's bits)", d_bits, batch, kDevice);
    std::vector<uint64_t> a(batch * dl), b(batch * dl);
    csgn_oracle_encrypt_keyed(n_bits, d, d_key, batch, first_ciphertext, d_plain_a, h_rng_a->key, h_rng_a->nonce, h_rng_a->rounds, a.data());
    csgn_oracle_encrypt_keyed(n_bits, d, d_key, batch, first_ciphertext, d_plain_b, h_rng_b->key, h_rng_b->nonce, h_rng_b->rounds, b.data());
    for (uint64_t i = 0; i < batch; ++i) {
        csgn_oracle_mul(dl, a.data() + i * dl, dl, nullptr, b.data() + i * dl, dl, d_out + i * dl, nullptr);
        if (d_bits)
            d_bits[i] = (uint8_t)(d_plain_a[i] & d_plain_b[i] & 1);
    }
    return CSGN_OK;
}

size_t csgn_decrypt_combined_scratch_bytes(uint64_t batch, uint64_t t1, uint64_t t2)
{
    const size_t pad = 256;
    return csgn_decrypt_scratch_bytes(batch, batch * t1) + csgn_decrypt_scratch_bytes(batch, batch * t2) +
           2 * (((size_t)batch + pad - 1) / pad * pad) + 4 * pad;
}

int csgn_decrypt_product_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2, const uint64_t *d_left,
                                 const uint64_t *d_right, const uint64_t *d_mask, uint8_t *d_bits, void *d_scratch, void *stream)
{
    return decrypt_combined("csgn_decrypt_product_uniform", true, n_bits, batch, t1, t2, d_left, d_right, d_mask, d_bits, d_scratch, stream);
}

int csgn_decrypt_sum_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2, const uint64_t *d_left,
                             const uint64_t *d_right, const uint64_t *d_mask, uint8_t *d_bits, void *d_scratch, void *stream)
{
    return decrypt_combined("csgn_decrypt_sum_uniform", false, n_bits, batch, t1, t2, d_left, d_right, d_mask, d_bits, d_scratch, stream);
}

int csgn_digest(const uint64_t *d_words, uint64_t n_words, uint64_t first_index, uint64_t *d_digest, void *stream)
{
    STREAM(stream);
    if (int rc = stub_enter("csgn_digest", d_digest, d_words, (size_t)n_words, first_index))
        return rc;
    REQUIRE(d_digest, "null device pointer");
    if (n_words == 0)
        return CSGN_OK;
    REQUIRE(d_words, "null device pointer");
    stub_check("csgn_digest (the words)", d_words, n_words * 8, kDevice);
    stub_check("csgn_digest (the digest)", d_digest, 8, kDevice);
    *d_digest += csgn_oracle_digest(d_words, n_words, first_index);      // accumulates, as the kernel's atomic add does
    return CSGN_OK;
}

int csgn_shard_product_counts(uint64_t batch, const uint64_t *d_off_left, const uint64_t *d_off_right, uint64_t t1, uint64_t t2,
                              uint64_t *d_counts, void *stream)
{
    if (stream != CSGN_STREAM_OF_COMM)
        STREAM(stream);
    if (int rc = stub_enter("csgn_shard_product_counts", d_counts, d_off_left, (size_t)batch, t1 * t2))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_counts, "d_counts is null");
    REQUIRE((d_off_left == nullptr) == (d_off_right == nullptr), "pass both offset arrays or neither");
    REQUIRE(batch < (1ull << 40), "batch too large");
    REQUIRE((batch + 255) / 256 < (1ull << 24), "batch too large for one launch");
    REQUIRE(stream != CSGN_STREAM_OF_COMM, "csgn_shard_product_counts takes a real stream (no communicator here)");
    stub_check("csgn_shard_product_counts (the counts)", d_counts, batch * 8, kDevice);
    if (d_off_left) {
        stub_check("csgn_shard_product_counts (left offsets)", d_off_left, (batch + 1) * 8, kDevice);
        stub_check("csgn_shard_product_counts (right offsets)", d_off_right, (batch + 1) * 8, kDevice);
    }
    for (uint64_t b = 0; b < batch; ++b)
        d_counts[b] = d_off_left ? (d_off_left[b + 1] - d_off_left[b]) * (d_off_right[b + 1] - d_off_right[b]) : t1 * t2;
    return CSGN_OK;
}

} // extern "C"
