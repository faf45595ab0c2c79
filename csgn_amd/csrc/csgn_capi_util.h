// csgn_capi_util.h -- what the translation units of the extern "C" surface share (csgn_capi.hip, csgn_circuit.hip):
// the thread-local error message, argument checks, the derivation of a circuit encrypt node's key.  Internal.
#pragma once

#include "csgn_hip.h"
#include "csgn_kernels.h"

namespace csgn {
namespace capi {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char *what);
bool product_below(uint64_t a, uint64_t b, uint64_t c, uint64_t limit);   // a*b*c < limit without wrapping
int check_n(uint64_t n_bits);                                              // shape limit shared by every entry point
// An element's largest list, `terms` terms, fits 2^31 words, and `batch` elements of batch_terms terms each fit 2^60
// words; the label (printf-style) names the operation and the list.  CSGN_OK or CSGN_ERR_UNSUPPORTED.
int check_size(uint64_t batch, uint64_t terms, uint64_t batch_terms, uint64_t dl, const char *label, ...)
    __attribute__((format(printf, 5, 6)));
int check_width(uint64_t width, uint64_t k);                               // 1..64 planes, and k fits in them
// a[j] (and b[j], when b is given) non-null for j < n; label: what the message calls element j
int check_planes(const uint64_t *const *a, const uint64_t *const *b, uint64_t n, const char *label);
int check_pair_product(uint64_t t1, uint64_t t2, uint64_t dl);             // one pair's product fits 2^32 words
void node_key_from(const csgn_rng &rng, uint32_t node_key[8]);

inline hipStream_t S(void *stream) { return reinterpret_cast<hipStream_t>(stream); }

} // namespace capi
} // namespace csgn

#define HIP_TRY(expr)                              \
    do {                                           \
        hipError_t e_ = (expr);                    \
        if (e_ != hipSuccess)                      \
            return csgn::capi::hip_fail(e_, #expr); \
    } while (0)

#define REQUIRE(cond, ...)                                           \
    do {                                                             \
        if (!(cond))                                                 \
            return csgn::capi::fail(CSGN_ERR_INVALID, __VA_ARGS__);  \
    } while (0)
