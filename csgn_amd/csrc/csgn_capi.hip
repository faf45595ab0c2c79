// csgn_capi.hip -- the extern "C" surface of libcsgn_hip.so (declared in include/csgn_hip.h).
// Argument validation, error reporting and stream plumbing only; the kernels live in the other translation units, behind
// the launchers of csgn_kernels.h.  There is deliberately no CPU fallback anywhere in this library.
#include "csgn_capi_util.h"
#include "csgn_device.h"
#include "csgn_tuning.h"

#include <sys/random.h>

#include <cerrno>
#include <cstdarg>
#include <vector>
#include <cstdio>
#include <cstring>

namespace csgn {
namespace capi {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
        return fail(CSGN_ERR_NO_DEVICE, "%s: %s (no usable HIP device; this library has no CPU path)",
                    what, hipGetErrorString(e));
    return fail(CSGN_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// a*b*c < limit, evaluated without wrapping (operands may be anything up to 2^64-1)
bool product_below(uint64_t a, uint64_t b, uint64_t c, uint64_t limit)
{
    unsigned long long ab, abc;
    if (__builtin_mul_overflow((unsigned long long)a, (unsigned long long)b, &ab) ||
        __builtin_mul_overflow(ab, (unsigned long long)c, &abc))
        return false;
    return abc < limit;
}

// ChaCha20 block on the host (D. J. Bernstein's function, 64-bit counter / 64-bit nonce layout) with
// caller-chosen constant words: only used to derive a circuit encrypt node's key.
void host_chacha20(const uint32_t sigma[4], const uint32_t key[8], uint64_t nonce, uint64_t counter, uint32_t out[16])
{
    uint32_t in[16], x[16];
    for (int i = 0; i < 4; ++i)
        in[i] = sigma[i];
    for (int i = 0; i < 8; ++i)
        in[4 + i] = key[i];
    in[12] = (uint32_t)counter;
    in[13] = (uint32_t)(counter >> 32);
    in[14] = (uint32_t)nonce;
    in[15] = (uint32_t)(nonce >> 32);
    memcpy(x, in, sizeof(x));
    auto rotl = [](uint32_t v, int n) { return (v << n) | (v >> (32 - n)); };
    auto qr = [&](int a, int b, int c, int d) {
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 16);
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 12);
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 8);
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 7);
    };
    for (int r = 0; r < 20; r += 2) {
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
    }
    for (int i = 0; i < 16; ++i)
        out[i] = x[i] + in[i];
}

// key of a circuit's encrypt node = words 0..7 of ChaCha20(constants "csgn node key v1", key, nonce, counter 0)
void node_key_from(const csgn_rng &rng, uint32_t node_key[8])
{
    static const uint32_t sigma[4] = {0x6e677363u, 0x646f6e20u, 0x656b2065u, 0x31762079u};   // "csgn node key v1"
    uint32_t block[16];
    host_chacha20(sigma, rng.key, rng.nonce, 0, block);
    for (int i = 0; i < 8; ++i)
        node_key[i] = block[i];
    volatile uint32_t *wipe = block;
    for (int i = 0; i < 16; ++i)
        wipe[i] = 0;
}

// Shape limits shared by every compute entry point.
int check_n(uint64_t n_bits)
{
    if (n_bits == 0)
        return fail(CSGN_ERR_INVALID, "n_bits must be > 0");
    if (((n_bits + 63) / 64) * 8 > 16384)
        return fail(CSGN_ERR_UNSUPPORTED, "n_bits=%llu: terms above 16384 bytes are not supported",
                    (unsigned long long)n_bits);
    return CSGN_OK;
}

int check_size(uint64_t batch, uint64_t terms, uint64_t batch_terms, uint64_t dl, const char *label, ...)
{
    const bool element = product_below(terms, dl, 1, 1ull << 31);
    if (element && product_below(batch, batch_terms, dl, 1ull << 60))
        return CSGN_OK;
    char who[128];
    va_list ap;
    va_start(ap, label);
    vsnprintf(who, sizeof(who), label, ap);
    va_end(ap);
    if (!element)
        return fail(CSGN_ERR_UNSUPPORTED, "%s: %llu terms per element exceed 2^31 words", who, (unsigned long long)terms);
    return fail(CSGN_ERR_UNSUPPORTED, "batch of %llu elements: size overflows", (unsigned long long)batch);
}

int check_width(uint64_t width, uint64_t k)
{
    REQUIRE(width >= 1 && width <= 64, "width %llu outside 1..64", (unsigned long long)width);
    REQUIRE(width == 64 || (k >> width) == 0, "constant %llu does not fit in %llu bits", (unsigned long long)k,
            (unsigned long long)width);
    return CSGN_OK;
}

int check_planes(const uint64_t *const *a, const uint64_t *const *b, uint64_t n, const char *label)
{
    for (uint64_t j = 0; j < n; ++j)
        REQUIRE(a[j] && (!b || b[j]), "null device pointer (%s %llu)", label, (unsigned long long)j);
    return CSGN_OK;
}

// What csgn_uint_read and csgn_uint_pick both check of an E stream, `op` ("read" / "pick") leading the text: the index
// width, the width of the table or source and the rows against the index width; and output j of terms * E terms (a
// product that wraps is past every limit).
int check_index(const char *op, uint64_t v, const char *width_name, uint64_t width, uint64_t rows)
{
    REQUIRE(v >= 1 && v <= csgn::kReadMaxIndex, "%s: index width %llu outside 1..16", op, (unsigned long long)v);
    REQUIRE(width >= 1 && width <= 64, "%s: %s %llu outside 1..64", op, width_name, (unsigned long long)width);
    REQUIRE(rows >= 1 && rows <= (1ull << v), "%s: %llu rows outside 1..2^%llu", op, (unsigned long long)rows,
            (unsigned long long)v);
    return CSGN_OK;
}
int check_index_output(const char *op, uint64_t batch, uint64_t terms, uint64_t E, uint64_t dl, uint64_t j)
{
    unsigned long long all;
    if (__builtin_mul_overflow((unsigned long long)terms, (unsigned long long)E, &all))
        all = ~0ull;
    return check_size(batch, all, all, dl, "%s: output %llu", op, (unsigned long long)j);
}

int check_pair_product(uint64_t t1, uint64_t t2, uint64_t dl)
{
    if (t1 >= (1ull << 31) || t2 >= (1ull << 31) || !product_below(t1, t2, dl, 1ull << 32))
        return fail(CSGN_ERR_UNSUPPORTED, "pair product of %llu x %llu terms exceeds 2^32 words",
                    (unsigned long long)t1, (unsigned long long)t2);
    return CSGN_OK;
}

} // namespace capi
} // namespace csgn

using namespace csgn::capi;

extern "C" {

int csgn_abi_version(void) { return CSGN_ABI_VERSION; }

const char *csgn_last_error(void) { return g_err; }

int csgn_device_count(int *h_count)
{
    REQUIRE(h_count, "h_count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *h_count = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    *h_count = n;
    return CSGN_OK;
}

int csgn_device_info(int device, char *h_name, size_t cap, int *h_cu_count, uint64_t *h_hbm_bytes)
{
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (h_name && cap) {
        strncpy(h_name, prop.gcnArchName, cap - 1);
        h_name[cap - 1] = 0;
    }
    if (h_cu_count)
        *h_cu_count = prop.multiProcessorCount;
    if (h_hbm_bytes)
        *h_hbm_bytes = (uint64_t)prop.totalGlobalMem;
    return CSGN_OK;
}

int csgn_init(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(CSGN_ERR_NO_DEVICE,
                    "csgn_init: no HIP device visible (%s); libcsgn_hip has no CPU fallback",
                    e == hipSuccess ? "count is 0" : hipGetErrorString(e));
    REQUIRE(device >= 0 && device < n, "csgn_init: device %d out of range (have %d)", device, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CSGN_ERR_NO_DEVICE, "csgn_init: device %d is %s; the kernels are built for gfx950 only",
                    device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    return CSGN_OK;
}

int csgn_malloc(void **d_ptr, size_t bytes)
{
    REQUIRE(d_ptr, "d_ptr is null");
    *d_ptr = nullptr;
    if (bytes == 0)
        return CSGN_OK;
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return CSGN_OK;
}

int csgn_free(void *d_ptr)
{
    if (d_ptr)
        HIP_TRY(hipFree(d_ptr));
    return CSGN_OK;
}

int csgn_host_alloc(void **h_ptr, void **d_alias, size_t bytes)
{
    REQUIRE(h_ptr && d_alias && bytes, "null pointer or zero size");
    *h_ptr = *d_alias = nullptr;
    HIP_TRY(hipHostMalloc(h_ptr, bytes, hipHostMallocMapped));
    hipError_t e = hipHostGetDevicePointer(d_alias, *h_ptr, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(*h_ptr);
        *h_ptr = *d_alias = nullptr;
        return hip_fail(e, "hipHostGetDevicePointer");
    }
    return CSGN_OK;
}

int csgn_host_free(void *h_ptr)
{
    if (h_ptr)
        HIP_TRY(hipHostFree(h_ptr));
    return CSGN_OK;
}

int csgn_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream)
{
    if (bytes == 0)
        return CSGN_OK;
    REQUIRE(d_dst && h_src, "null pointer");
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, S(stream)));
    return CSGN_OK;
}

int csgn_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream)
{
    if (bytes == 0)
        return CSGN_OK;
    REQUIRE(h_dst && d_src, "null pointer");
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    return CSGN_OK;
}

int csgn_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream)
{
    if (bytes == 0)
        return CSGN_OK;
    REQUIRE(d_dst && d_src, "null pointer");
    HIP_TRY(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, S(stream)));
    return CSGN_OK;
}

int csgn_memset(void *d_dst, int value, size_t bytes, void *stream)
{
    if (bytes == 0)
        return CSGN_OK;
    REQUIRE(d_dst, "null pointer");
    HIP_TRY(hipMemsetAsync(d_dst, value, bytes, S(stream)));
    return CSGN_OK;
}

int csgn_stream_create(void **stream)
{
    REQUIRE(stream, "stream is null");
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return CSGN_OK;
}

int csgn_stream_destroy(void *stream)
{
    if (stream)
        HIP_TRY(hipStreamDestroy(S(stream)));
    return CSGN_OK;
}

int csgn_stream_sync(void *stream)
{
    HIP_TRY(hipStreamSynchronize(S(stream)));
    return CSGN_OK;
}

int csgn_event_create(void **event)
{
    REQUIRE(event, "event is null");
    hipEvent_t ev;
    HIP_TRY(hipEventCreate(&ev));
    *event = ev;
    return CSGN_OK;
}

int csgn_event_destroy(void *event)
{
    if (event)
        HIP_TRY(hipEventDestroy(reinterpret_cast<hipEvent_t>(event)));
    return CSGN_OK;
}

int csgn_event_record(void *event, void *stream)
{
    REQUIRE(event, "event is null");
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(event), S(stream)));
    return CSGN_OK;
}

int csgn_event_sync(void *event)
{
    REQUIRE(event, "event is null");
    HIP_TRY(hipEventSynchronize(reinterpret_cast<hipEvent_t>(event)));
    return CSGN_OK;
}

int csgn_event_elapsed_ms(void *start, void *stop, float *h_ms)
{
    REQUIRE(start && stop && h_ms, "null argument");
    HIP_TRY(hipEventSynchronize(reinterpret_cast<hipEvent_t>(stop)));
    HIP_TRY(hipEventElapsedTime(h_ms, reinterpret_cast<hipEvent_t>(start),
                                reinterpret_cast<hipEvent_t>(stop)));
    return CSGN_OK;
}

/* ------------------------------------------------------------ host-side metadata -- */

uint64_t csgn_default_len(uint64_t n_bits) { return n_bits / 64 + ((n_bits % 64) ? 1 : 0); }

uint64_t csgn_context_s(uint64_t n_bits, uint64_t d) { return d ? n_bits / (2 * d) : 0; }

uint64_t csgn_mul_len(uint64_t n_bits, uint64_t len1, uint64_t len2)
{
    const uint64_t dl = csgn_default_len(n_bits);
    if (dl == 0)
        return 0;
    if (len1 == dl && len1 == len2)
        return len1;
    return ((len1 / dl) * len2) / dl * dl;
}

int csgn_bitlen_canonical(uint64_t n_bits, uint64_t terms, uint64_t *h_bitlen)
{
    REQUIRE(n_bits > 0, "n_bits must be > 0");
    REQUIRE(h_bitlen || terms == 0, "h_bitlen is null");
    const uint64_t dl = csgn_default_len(n_bits), rem = n_bits % 64;
    for (uint64_t t = 0; t < terms; ++t)
        for (uint64_t k = 0; k < dl; ++k)
            h_bitlen[t * dl + k] = (rem && k == dl - 1) ? rem : 64;
    return CSGN_OK;
}

int csgn_key_mask(uint64_t n_bits, const uint64_t *h_key, uint64_t d, uint64_t *h_mask)
{
    REQUIRE(n_bits > 0 && h_key && h_mask && d > 0, "bad argument");
    const uint64_t dl = csgn_default_len(n_bits);
    memset(h_mask, 0, dl * sizeof(uint64_t));
    for (uint64_t i = 0; i < d; ++i) {
        REQUIRE(h_key[i] < n_bits, "key index %llu (slot %llu) is outside [0,%llu)",
                (unsigned long long)h_key[i], (unsigned long long)i, (unsigned long long)n_bits);
        h_mask[h_key[i] / 64] |= 1ull << (63 - (h_key[i] % 64));
    }
    return CSGN_OK;
}

/* ---------------------------------------------------------------------- hot path -- */

int csgn_mul_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                     const uint64_t *d_left, const uint64_t *d_right, uint64_t *d_out,
                     uint64_t out_slots, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0 || t1 == 0 || t2 == 0)
        return CSGN_OK;
    REQUIRE(d_left && d_right && d_out, "null device pointer");
    const uint64_t dl = csgn_default_len(n_bits);
    if (int rc = check_pair_product(t1, t2, dl))
        return rc;
    if (!product_below(batch, t1 + t2, dl, 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "batch of %llu pairs: operand size overflows", (unsigned long long)batch);
    HIP_TRY(csgn::mul_uniform(n_bits, batch, t1, t2, (const u64 *)d_left, (const u64 *)d_right,
                              (u64 *)d_out, out_slots, S(stream)));
    return CSGN_OK;
}

} // extern "C"

namespace {

// the plan step behind csgn_mul_ragged_plan and csgn_mul_plan_ragged; h_head_out (optional): the whole head block
struct PlanScratch {
    u64 *p = nullptr;
    size_t words = 0;
};

// owned: a csgn_mul_plan's own device block (it has to outlive the call: the class lists stay in it);
// nullptr: the calling thread's grow-only block
int plan_ragged(uint64_t batch, const uint64_t *d_off_left, const uint64_t *d_off_right,
                uint64_t *d_off_out, uint64_t h_plan[4], uint64_t *h_head_out, PlanScratch *owned, void *stream)
{
    REQUIRE(d_off_left && d_off_right && d_off_out && h_plan, "null pointer");
    // The call returns host numbers, so it ends with a stream synchronise anyway; its small device
    // scratch is kept per host thread and device (grow-only) because hipMalloc + hipFree around
    // every plan cost more than the plan (hipFree synchronises the whole device).
    static thread_local PlanScratch cache[16];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const size_t need = csgn::mul_ragged_plan_scratch_words(batch);
    PlanScratch local;
    PlanScratch &sc = owned ? *owned : (dev >= 0 && dev < 16) ? cache[dev] : local;
    if (sc.words < need) {
        if (sc.p)
            (void)hipFree(sc.p);
        sc.p = nullptr;
        sc.words = 0;
        const size_t grow = need + need / 2 + 1024;
        HIP_TRY(hipMalloc((void **)&sc.p, grow * sizeof(u64)));
        sc.words = grow;
    }
    hipError_t e = csgn::mul_ragged_plan(batch, (const u64 *)d_off_left, (const u64 *)d_off_right,
                                         (u64 *)d_off_out, sc.p, S(stream));
    // the four plan numbers and, in the same copy, the plan's notes on huge pairs (csgn_mul_ragged
    // gives each of those a uniform launch of its own)
    std::vector<u64> head(csgn::mul_ragged_plan_head_words(), 0);
    if (e == hipSuccess)
        e = hipMemcpyAsync(head.data(), sc.p, head.size() * sizeof(u64), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess)
        e = hipStreamSynchronize(S(stream));
    if (e == hipSuccess) {
        memcpy(h_plan, head.data(), 4 * sizeof(u64));
        if (h_head_out)
            memcpy(h_head_out, head.data(), head.size() * sizeof(u64));
    }
    if (&sc == &local && local.p)
        (void)hipFree(local.p);
    if (e != hipSuccess)
        return hip_fail(e, "csgn_mul_ragged_plan");
    return CSGN_OK;
}

} // namespace

extern "C" {

int csgn_mul_ragged_plan(uint64_t batch, const uint64_t *d_off_left, const uint64_t *d_off_right,
                         uint64_t *d_off_out, uint64_t h_plan[4], void *stream)
{
    return plan_ragged(batch, d_off_left, d_off_right, d_off_out, h_plan, nullptr, nullptr, stream);
}

/* ---- the plan as an object of the caller's ---- */
struct csgn_mul_plan {
    csgn::MulPlanNotes notes;
    bool planned = false;
    bool trust = false;
    u64 *d_sum = nullptr;        // one device word for the checksum check
    int device = -1;
    PlanScratch work;            // the plan kernels' device block: the size-class lists live here
    int work_device = -1;
};

int csgn_mul_plan_create(csgn_mul_plan **plan)
{
    REQUIRE(plan, "plan is null");
    *plan = new csgn_mul_plan();
    return CSGN_OK;
}

void csgn_mul_plan_destroy(csgn_mul_plan *plan)
{
    if (!plan)
        return;
    if (plan->d_sum)
        (void)hipFree(plan->d_sum);
    if (plan->work.p)
        (void)hipFree(plan->work.p);
    delete plan;
}

int csgn_mul_plan_trust(csgn_mul_plan *plan, int trust)
{
    REQUIRE(plan, "plan is null");
    plan->trust = trust != 0;
    return CSGN_OK;
}

int csgn_mul_plan_ragged(csgn_mul_plan *plan, uint64_t batch, const uint64_t *d_off_left,
                         const uint64_t *d_off_right, uint64_t *d_off_out, uint64_t h_plan[4], void *stream)
{
    REQUIRE(plan, "plan is null");
    plan->planned = false;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (plan->work.p && plan->work_device != dev) {          // the object moved to another GPU: start over there
        (void)hipFree(plan->work.p);
        plan->work = PlanScratch();
    }
    plan->work_device = dev;
    std::vector<u64> head(csgn::mul_ragged_plan_head_words(), 0);
    if (int rc = plan_ragged(batch, d_off_left, d_off_right, d_off_out, h_plan, reinterpret_cast<uint64_t *>(head.data()),
                             &plan->work, stream))
        return rc;
    csgn::mul_plan_notes_from_head(plan->notes, (const u64 *)d_off_left, (const u64 *)d_off_right,
                                   (const u64 *)d_off_out, batch, head.data(), plan->work.p);
    plan->planned = true;
    return CSGN_OK;
}

int csgn_mul_plan_validate(csgn_mul_plan *plan, void *stream)
{
    REQUIRE(plan && plan->planned, "no plan: call csgn_mul_plan_ragged first");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (plan->d_sum && plan->device != dev) {
        (void)hipFree(plan->d_sum);
        plan->d_sum = nullptr;
    }
    const u32 slots = csgn::offsets_checksum_words();
    if (!plan->d_sum) {
        HIP_TRY(hipMalloc((void **)&plan->d_sum, slots * 8));
        plan->device = dev;
    }
    const csgn::MulPlanNotes &n = plan->notes;
    HIP_TRY(csgn::offsets_checksum(n.batch, n.offL, n.offR, n.offOut, plan->d_sum, S(stream)));
    std::vector<u64> part(slots, 0);
    HIP_TRY(hipMemcpyAsync(part.data(), plan->d_sum, slots * 8, hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    u64 now = 0;
    for (u64 v : part)
        now += v;
    if (now != n.checksum)
        return fail(CSGN_ERR_INVALID, "the offset arrays changed since csgn_mul_plan_ragged: plan again");
    return CSGN_OK;
}

int csgn_mul_planned(csgn_mul_plan *plan, uint64_t n_bits, const uint64_t *d_left, const uint64_t *d_right,
                     uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(plan && plan->planned, "no plan: call csgn_mul_plan_ragged first");
    const csgn::MulPlanNotes &n = plan->notes;
    if (n.batch == 0 || n.max_t1 == 0 || n.max_t2 == 0 || n.total == 0)
        return CSGN_OK;
    REQUIRE(d_left && d_right && d_out, "null device pointer");
    if (int rc = check_pair_product(n.max_t1, n.max_t2, csgn_default_len(n_bits)))
        return rc;
    // host copies of offsets are only used for huge pairs: that is when stale offsets would give wrong words
    if (n.n != 0 && !plan->trust)
        if (int rc = csgn_mul_plan_validate(plan, stream))
            return rc;
    hipError_t e = csgn::mul_ragged(n_bits, n.batch, (const u64 *)d_left, n.offL, (const u64 *)d_right, n.offR,
                                    (u64 *)d_out, n.offOut, n.max_t1, n.max_t2, n.total, S(stream), &plan->notes);
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "ragged batch too large for one call (2^32 pairs / one pair's tile grid)");
    HIP_TRY(e);
    return CSGN_OK;
}

uint64_t csgn_mul_ragged_async_plan_words(uint64_t batch) { return csgn::mul_ragged_async_plan_words(batch); }

int csgn_mul_ragged_async(uint64_t n_bits, uint64_t batch,
                          const uint64_t *d_left, const uint64_t *d_off_left,
                          const uint64_t *d_right, const uint64_t *d_off_right,
                          uint64_t *d_out, uint64_t *d_off_out, uint64_t out_capacity_terms,
                          uint64_t *d_plan, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_off_left && d_off_right && d_off_out && d_plan, "null pointer");
    REQUIRE(out_capacity_terms == 0 || (d_left && d_right && d_out), "null device pointer");
    if (!product_below(out_capacity_terms, csgn_default_len(n_bits), 1, 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "output capacity overflows");
    hipError_t e = csgn::mul_ragged_async(n_bits, batch, (const u64 *)d_left, (const u64 *)d_off_left,
                                          (const u64 *)d_right, (const u64 *)d_off_right, (u64 *)d_out,
                                          (u64 *)d_off_out, out_capacity_terms, (u64 *)d_plan, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "ragged batch too large for one call (2^32 pairs)");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_mul_ragged_async_result(const uint64_t *d_plan, uint64_t h_result[5], void *stream)
{
    REQUIRE(d_plan && h_result, "null pointer");
    u64 head[12] = {0};                       // [gate: 8 words][plan4]
    HIP_TRY(hipMemcpyAsync(head, d_plan, sizeof(head), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    for (int i = 0; i < 4; ++i)
        h_result[i] = head[8 + i];
    h_result[4] = head[1];
    return CSGN_OK;
}

int csgn_mul_ragged(uint64_t n_bits, uint64_t batch,
                    const uint64_t *d_left, const uint64_t *d_off_left,
                    const uint64_t *d_right, const uint64_t *d_off_right,
                    uint64_t *d_out, const uint64_t *d_off_out,
                    uint64_t max_t1, uint64_t max_t2, uint64_t total_out_terms, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0 || max_t1 == 0 || max_t2 == 0 || total_out_terms == 0)
        return CSGN_OK;
    REQUIRE(d_left && d_right && d_out && d_off_left && d_off_right && d_off_out, "null device pointer");
    if (int rc = check_pair_product(max_t1, max_t2, csgn_default_len(n_bits)))
        return rc;
    hipError_t e = csgn::mul_ragged(n_bits, batch, (const u64 *)d_left, (const u64 *)d_off_left,
                                    (const u64 *)d_right, (const u64 *)d_off_right, (u64 *)d_out,
                                    (const u64 *)d_off_out, max_t1, max_t2, total_out_terms, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "ragged batch too large for one call (2^32 pairs / one pair's tile grid)");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_add_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                     const uint64_t *d_left, const uint64_t *d_right, uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    const uint64_t dl = csgn_default_len(n_bits);
    if (t1 >= (1ull << 31) || t2 >= (1ull << 31) || (t1 + t2) * dl >= (1ull << 31))
        return fail(CSGN_ERR_UNSUPPORTED, "sum of %llu + %llu terms exceeds 2^31 words per pair",
                    (unsigned long long)t1, (unsigned long long)t2);
    if (batch == 0 || t1 + t2 == 0)
        return CSGN_OK;
    REQUIRE(d_out && (d_left || t1 == 0) && (d_right || t2 == 0), "null device pointer");
    if (!product_below(batch, t1 + t2, dl, 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "batch of %llu pairs: size overflows", (unsigned long long)batch);
    HIP_TRY(csgn::add_uniform(n_bits, batch, t1, t2, (const u64 *)d_left, (const u64 *)d_right,
                              (u64 *)d_out, S(stream)));
    return CSGN_OK;
}

int csgn_add_ragged(uint64_t n_bits, uint64_t batch,
                    const uint64_t *d_left, const uint64_t *d_off_left,
                    const uint64_t *d_right, const uint64_t *d_off_right,
                    uint64_t *d_out, uint64_t *d_off_out, uint64_t total_terms_out, void *stream)
{
    return csgn_add_ragged_bounded(n_bits, batch, 0, 0, d_left, d_off_left, d_right, d_off_right, d_out, d_off_out,
                                   total_terms_out, stream);
}

int csgn_add_ragged_bounded(uint64_t n_bits, uint64_t batch, uint64_t max_t1, uint64_t max_t2,
                            const uint64_t *d_left, const uint64_t *d_off_left,
                            const uint64_t *d_right, const uint64_t *d_off_right,
                            uint64_t *d_out, uint64_t *d_off_out, uint64_t total_terms_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(d_off_left && d_off_right && d_off_out, "null offset pointer");
    REQUIRE(total_terms_out == 0 || batch == 0 || (d_left && d_right && d_out), "null device pointer");
    const bool bounded = max_t1 != 0 || max_t2 != 0;
    REQUIRE(!bounded || (max_t1 < (1ull << 31) && max_t2 < (1ull << 31) &&
                         !product_below(batch, max_t1 + max_t2, 1, total_terms_out)),
            "bounds %llu + %llu cannot hold: %llu sums of at most that many terms are fewer than total_terms_out = %llu",
            (unsigned long long)max_t1, (unsigned long long)max_t2, (unsigned long long)batch, (unsigned long long)total_terms_out);
    hipError_t e = csgn::add_ragged(n_bits, batch, (const u64 *)d_left, (const u64 *)d_off_left,
                                    (const u64 *)d_right, (const u64 *)d_off_right, (u64 *)d_out,
                                    (u64 *)d_off_out, total_terms_out, S(stream), false, max_t1, max_t2);
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "ragged batch of 2^32 or more pairs; split it");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_small_ops(uint64_t n_bits, uint64_t count, const csgn_small_op *d_ops, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (count == 0)
        return CSGN_OK;
    REQUIRE(d_ops, "d_ops is null");
    const hipError_t e = csgn::small_ops(n_bits, count, d_ops, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "more than 2^24 - 1 operations in one call; split the list");
    HIP_TRY(e);
    return CSGN_OK;
}

size_t csgn_decrypt_scratch_bytes(uint64_t batch, uint64_t total_terms)
{
    return csgn::decrypt_scratch_bytes(batch, total_terms);
}

int csgn_decrypt_uniform(uint64_t n_bits, uint64_t batch, uint64_t terms,
                         const uint64_t *d_terms, const uint64_t *d_mask,
                         uint8_t *d_bits, void *d_scratch, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_mask && d_bits && d_scratch && (d_terms || terms == 0), "null device pointer");
    if (!product_below(batch, terms, csgn_default_len(n_bits), 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "batch of %llu x %llu terms: size overflows",
                    (unsigned long long)batch, (unsigned long long)terms);
    HIP_TRY(csgn::decrypt(n_bits, batch, terms, batch * terms, (const u64 *)d_terms, nullptr,
                          (const u64 *)d_mask, d_bits, d_scratch, S(stream)));
    return CSGN_OK;
}

int csgn_decrypt_ragged_bounded(uint64_t n_bits, uint64_t batch, uint64_t total_terms, uint64_t max_terms,
                                const uint64_t *d_terms, const uint64_t *d_off, const uint64_t *d_mask,
                                uint8_t *d_bits, void *d_scratch, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_off && d_mask && d_bits && d_scratch && (d_terms || total_terms == 0),
            "null device pointer");
    REQUIRE(max_terms == 0 || !product_below(batch, max_terms, 1, total_terms),
            "max_terms = %llu cannot hold: %llu ciphertexts of at most that many terms are fewer than total_terms = %llu",
            (unsigned long long)max_terms, (unsigned long long)batch, (unsigned long long)total_terms);
    HIP_TRY(csgn::decrypt(n_bits, batch, 0, total_terms, (const u64 *)d_terms, (const u64 *)d_off,
                          (const u64 *)d_mask, d_bits, d_scratch, S(stream), max_terms));
    return CSGN_OK;
}

int csgn_decrypt_ragged(uint64_t n_bits, uint64_t batch, uint64_t total_terms,
                        const uint64_t *d_terms, const uint64_t *d_off, const uint64_t *d_mask,
                        uint8_t *d_bits, void *d_scratch, void *stream)
{
    return csgn_decrypt_ragged_bounded(n_bits, batch, total_terms, 0, d_terms, d_off, d_mask, d_bits, d_scratch, stream);
}

size_t csgn_decrypt_combined_scratch_bytes(uint64_t batch, uint64_t t1, uint64_t t2)
{
    return csgn::decrypt_combined_scratch_bytes(batch, t1, t2);
}

static int decrypt_combined_uniform(bool is_product, uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                                    const uint64_t *d_left, const uint64_t *d_right, const uint64_t *d_mask,
                                    uint8_t *d_bits, void *d_scratch, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_mask && d_bits && d_scratch && (d_left || t1 == 0) && (d_right || t2 == 0),
            "null device pointer");
    if (!product_below(batch, t1, csgn_default_len(n_bits), 1ull << 60) ||
        !product_below(batch, t2, csgn_default_len(n_bits), 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "batch of %llu ciphertexts: size overflows", (unsigned long long)batch);
    HIP_TRY(csgn::decrypt_combined(n_bits, batch, t1, t2, (const u64 *)d_left, (const u64 *)d_right,
                                   (const u64 *)d_mask, is_product, d_bits, d_scratch, S(stream)));
    return CSGN_OK;
}

int csgn_decrypt_product_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                                 const uint64_t *d_left, const uint64_t *d_right,
                                 const uint64_t *d_mask, uint8_t *d_bits, void *d_scratch, void *stream)
{
    return decrypt_combined_uniform(true, n_bits, batch, t1, t2, d_left, d_right, d_mask, d_bits, d_scratch, stream);
}

int csgn_decrypt_sum_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2,
                             const uint64_t *d_left, const uint64_t *d_right,
                             const uint64_t *d_mask, uint8_t *d_bits, void *d_scratch, void *stream)
{
    return decrypt_combined_uniform(false, n_bits, batch, t1, t2, d_left, d_right, d_mask, d_bits, d_scratch, stream);
}

size_t csgn_compact_scratch_bytes(uint64_t n_bits, uint64_t batch, uint64_t total_terms)
{
    if (n_bits == 0 || !csgn::compact_supported(n_bits))
        return 0;
    return csgn::compact_scratch_bytes(n_bits, batch, total_terms);
}

int csgn_compact_ragged(uint64_t n_bits, uint64_t batch, uint64_t total_terms, uint64_t max_terms,
                        const uint64_t *d_terms, const uint64_t *d_off,
                        uint64_t *d_out, uint64_t *d_off_out, void *d_scratch, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_off && d_off_out && d_scratch && ((d_terms && d_out) || total_terms == 0),
            "null device pointer");
    REQUIRE(d_terms != d_out || total_terms == 0, "compaction is not done in place");
    hipError_t e = csgn::compact(n_bits, batch, total_terms, max_terms, (const u64 *)d_terms, (const u64 *)d_off,
                                 (u64 *)d_out, (u64 *)d_off_out, d_scratch, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED,
                    "compaction handles fewer than 2^31 ciphertexts and terms per call");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_encrypt_explicit(uint64_t n_bits, uint64_t d, uint64_t batch,
                          const uint8_t *d_plain, const uint64_t *d_rnd,
                          const uint32_t *d_chosen, const uint8_t *d_last,
                          const uint64_t *d_mask, uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d >= 1, "d must be >= 1");
    REQUIRE(d_plain && d_rnd && d_chosen && d_last && d_mask && d_out, "null device pointer");
    HIP_TRY(csgn::encrypt(n_bits, d, batch, d_plain, (const u64 *)d_rnd, d_chosen, d_last,
                          (const u64 *)d_mask, (u64 *)d_out, S(stream)));
    return CSGN_OK;
}

int csgn_rng_from_os(csgn_rng *h_rng, uint32_t rounds)
{
    REQUIRE(h_rng, "h_rng is null");
    REQUIRE(rounds == 8 || rounds == 12 || rounds == 20, "rounds must be 8, 12 or 20");
    unsigned char buf[40];
    size_t got = 0;
    while (got < sizeof(buf)) {
        const ssize_t r = getrandom(buf + got, sizeof(buf) - got, 0);
        if (r < 0) {
            if (errno == EINTR)
                continue;
            return fail(CSGN_ERR_INVALID, "getrandom failed: %s", strerror(errno));
        }
        got += (size_t)r;
    }
    memcpy(h_rng->key, buf, 32);
    memcpy(&h_rng->nonce, buf + 32, 8);
    h_rng->rounds = rounds;
    h_rng->reserved = 0;
    memset(buf, 0, sizeof(buf));
    return CSGN_OK;
}

int csgn_rng_from_seed(csgn_rng *h_rng, uint64_t seed, uint32_t rounds)
{
    REQUIRE(h_rng, "h_rng is null");
    REQUIRE(rounds == 8 || rounds == 12 || rounds == 20, "rounds must be 8, 12 or 20");
    for (int i = 0; i < 4; ++i) {
        const uint64_t w = csgn_splitmix64(seed + CSGN_GOLDEN * (uint64_t)(i + 1));
        h_rng->key[2 * i] = (uint32_t)w;
        h_rng->key[2 * i + 1] = (uint32_t)(w >> 32);
    }
    h_rng->nonce = csgn_splitmix64(seed ^ 0xD1B54A32D192ED03ull);
    h_rng->rounds = rounds;
    h_rng->reserved = 0;
    return CSGN_OK;
}

int csgn_encrypt_keyed_layout(uint64_t n_bits, uint32_t *h_units, uint32_t *h_passes, uint32_t *h_group)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_units && h_passes && h_group, "null output");
    csgn::encrypt_keyed_layout(n_bits, h_units, h_passes, h_group);
    return CSGN_OK;
}

int csgn_encrypt_keyed(uint64_t n_bits, uint64_t d, uint64_t batch, uint64_t first_ciphertext,
                       const uint8_t *d_plain, const uint64_t *d_key, const uint64_t *d_mask,
                       const csgn_rng *h_rng, uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_rng, "h_rng is null");
    REQUIRE(h_rng->rounds == 8 || h_rng->rounds == 12 || h_rng->rounds == 20, "rng rounds must be 8, 12 or 20");
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d >= 1 && d < (1ull << 32), "d must be in [1, 2^32)");
    REQUIRE(d_plain && d_key && d_mask && d_out, "null device pointer");
    REQUIRE(first_ciphertext + batch >= first_ciphertext && first_ciphertext + batch < (1ull << 56),
            "ciphertext index range too large");
    hipError_t e = csgn::encrypt_keyed(n_bits, d, batch, first_ciphertext, d_plain, (const u64 *)d_key,
                                       (const u64 *)d_mask, h_rng->key, h_rng->nonce, h_rng->rounds, nullptr,
                                       (u64 *)d_out, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "batch too large for one launch");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_encrypt_mul_keyed(uint64_t n_bits, uint64_t d, uint64_t batch, uint64_t first_ciphertext,
                           const uint8_t *d_plain_a, const uint8_t *d_plain_b, const uint64_t *d_key,
                           const uint64_t *d_mask, const csgn_rng *h_rng_a, const csgn_rng *h_rng_b,
                           uint64_t *d_out, uint8_t *d_bits, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_rng_a && h_rng_b, "h_rng is null");
    REQUIRE(h_rng_a->rounds == 8 || h_rng_a->rounds == 12 || h_rng_a->rounds == 20, "rng rounds must be 8, 12 or 20");
    REQUIRE(h_rng_a->rounds == h_rng_b->rounds, "both generators must use the same number of rounds");
    REQUIRE(memcmp(h_rng_a->key, h_rng_b->key, sizeof(h_rng_a->key)) != 0 || h_rng_a->nonce != h_rng_b->nonce,
            "the two operands must draw from different streams (same key AND nonce given)");
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d >= 1 && d < (1ull << 32), "d must be in [1, 2^32)");
    REQUIRE(d_plain_a && d_plain_b && d_key && d_mask && d_out, "null device pointer");
    REQUIRE(first_ciphertext + batch >= first_ciphertext && first_ciphertext + batch < (1ull << 56),
            "ciphertext index range too large");
    hipError_t e = csgn::encrypt_mul_keyed(n_bits, d, batch, first_ciphertext, d_plain_a, d_plain_b, (const u64 *)d_key,
                                           (const u64 *)d_mask, h_rng_a->key, h_rng_a->nonce, h_rng_b->key,
                                           h_rng_b->nonce, h_rng_a->rounds, nullptr, (u64 *)d_out, d_bits, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "batch too large for one launch");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_encrypt_device_rng(uint64_t n_bits, uint64_t d, uint64_t batch,
                            const uint8_t *d_plain, const uint64_t *d_key,
                            const uint64_t *d_mask, uint64_t seed, uint64_t *d_out, void *stream)
{
    csgn_rng rng;
    if (int rc = csgn_rng_from_seed(&rng, seed, 8))
        return rc;
    return csgn_encrypt_keyed(n_bits, d, batch, 0, d_plain, d_key, d_mask, &rng, d_out, stream);
}

int csgn_permute_uniform(uint64_t n_bits, uint64_t batch, uint64_t terms_in, int per_term,
                         const uint64_t *d_terms, const uint32_t *d_perm, uint64_t *d_out,
                         void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_perm && d_out && (d_terms || terms_in == 0), "null device pointer");
    HIP_TRY(csgn::permute(n_bits, batch, terms_in, per_term != 0, (const u64 *)d_terms, d_perm,
                          (u64 *)d_out, S(stream)));
    return CSGN_OK;
}

size_t csgn_bitlen_scratch_bytes(uint64_t len_words) { return csgn::bitlen_scratch_bytes(len_words); }

int csgn_decrypt_bitlen(uint64_t n_bits, uint64_t d, uint64_t len_words, const uint64_t *d_v,
                        const uint64_t *d_bitlen, const uint64_t *d_key, uint8_t *d_bit, void *d_scratch,
                        void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(d >= 1, "d must be >= 1");
    REQUIRE(d_key && d_bit && d_scratch && ((d_v && d_bitlen) || len_words == 0), "null device pointer");
    REQUIRE(len_words < (1ull << 40), "ciphertext too long");
    hipError_t e = csgn::decrypt_bitlen(n_bits, d, len_words, (const u64 *)d_v, (const u64 *)d_bitlen,
                                        (const u64 *)d_key, d_bit, d_scratch, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "ciphertext too long for one launch");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_permute_bitlen(uint64_t n_bits, uint64_t len_words, const uint64_t *d_v, const uint64_t *d_bitlen,
                        const uint32_t *d_perm, uint64_t *d_out, void *d_scratch, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(d_perm && d_out && d_scratch && ((d_v && d_bitlen) || len_words == 0), "null device pointer");
    REQUIRE(len_words < (1ull << 40), "ciphertext too long");
    hipError_t e = csgn::permute_bitlen(n_bits, len_words, (const u64 *)d_v, (const u64 *)d_bitlen, d_perm,
                                        (u64 *)d_out, d_scratch, S(stream));
    if (e == hipErrorInvalidValue)
        return fail(CSGN_ERR_UNSUPPORTED, "ciphertext too long for one launch");
    HIP_TRY(e);
    return CSGN_OK;
}

int csgn_synth_fill(uint64_t seed, uint64_t n_bits, uint64_t first_word, uint64_t n_words,
                    uint64_t *d_out, void *stream)
{
    REQUIRE(n_bits > 0, "n_bits must be > 0");
    if (n_words == 0)
        return CSGN_OK;
    REQUIRE(d_out, "null device pointer");
    HIP_TRY(csgn::synth_fill(seed, n_bits, first_word, n_words, (u64 *)d_out, S(stream)));
    return CSGN_OK;
}

int csgn_digest(const uint64_t *d_words, uint64_t n_words, uint64_t first_index,
                uint64_t *d_digest, void *stream)
{
    REQUIRE(d_digest, "null device pointer");
    if (n_words == 0)
        return CSGN_OK;
    REQUIRE(d_words, "null device pointer");
    HIP_TRY(csgn::digest((const u64 *)d_words, n_words, first_index, (u64 *)d_digest, S(stream)));
    return CSGN_OK;
}

const char *csgn_mul_uniform_kernel(uint64_t n_bits, uint64_t pairs, uint64_t t1, uint64_t t2)
{
    return csgn::mul_uniform_kernel_name(n_bits, pairs, t1, t2);
}

/* ------------------------------------------------------------------- gates ---- */

namespace {
// the gate entry points say NO_DEVICE before anything else when there is no GPU (a launch would report it less plainly)
int require_device(const char *who)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(CSGN_ERR_NO_DEVICE, "%s: no HIP device visible (%s); this library has no CPU fallback", who,
                    e == hipSuccess ? "count is 0" : hipGetErrorString(e));
    return CSGN_OK;
}
} // namespace

uint64_t csgn_gate_terms(int gate, uint64_t t_sel, uint64_t t_a, uint64_t t_b)
{
    return csgn::gate_terms(gate, t_sel, t_a, t_b);
}

const char *csgn_gate_uniform_kernel(uint64_t n_bits, int gate, uint64_t batch, uint64_t t_sel, uint64_t t_a,
                                     uint64_t t_b)
{
    return csgn::gate_kernel_name(n_bits, gate, batch, t_sel, t_a, t_b);
}

int csgn_gate_uniform(uint64_t n_bits, int gate, uint64_t batch, uint64_t t_sel, uint64_t t_a, uint64_t t_b,
                      const uint64_t *d_sel, const uint64_t *d_a, const uint64_t *d_b, const uint8_t *d_plain,
                      uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(gate >= CSGN_GATE_NOT && gate <= CSGN_GATE_MUL_PLAIN, "unknown gate %d", gate);
    const bool uses_sel = gate == CSGN_GATE_MUX;
    const bool uses_b = gate != CSGN_GATE_NOT && gate != CSGN_GATE_ADD_PLAIN && gate != CSGN_GATE_MUL_PLAIN;
    const bool uses_plain = gate == CSGN_GATE_ADD_PLAIN || gate == CSGN_GATE_MUL_PLAIN;
    if (!uses_sel)
        t_sel = 0;
    if (!uses_b)
        t_b = 0;
    const uint64_t terms = csgn::gate_terms(gate, t_sel, t_a, t_b);
    REQUIRE(terms != 0, "gate %d: an operand it reads has no terms, or the term count overflows", gate);
    if (int rc = check_size(batch, terms, terms, csgn_default_len(n_bits), "gate %d", gate))
        return rc;
    if (int rc = require_device("csgn_gate_uniform"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_out && d_a && (d_sel || !uses_sel) && (d_b || !uses_b) && (d_plain || !uses_plain),
            "null device pointer");
    HIP_TRY(csgn::gate_uniform(n_bits, gate, batch, t_sel, t_a, t_b, (const u64 *)(uses_sel ? d_sel : nullptr),
                               (const u64 *)d_a, (const u64 *)(uses_b ? d_b : nullptr), uses_plain ? d_plain : nullptr,
                               (u64 *)d_out, S(stream)));
    return CSGN_OK;
}

int csgn_const_fill(uint64_t n_bits, uint64_t batch, const uint8_t *d_plain, int bit, uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (!product_below(batch, csgn_default_len(n_bits), 1, 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "batch of %llu constants: size overflows", (unsigned long long)batch);
    if (int rc = require_device("csgn_const_fill"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_out, "null device pointer");
    HIP_TRY(csgn::const_fill(n_bits, batch, d_plain, bit, (u64 *)d_out, 0, S(stream)));
    return CSGN_OK;
}

/* ---------------------------------------------------------------- integers ---- */

uint64_t csgn_uint_step_terms(int step, int output, uint64_t t_x, uint64_t t_a, uint64_t t_b)
{
    return csgn::uint_step_terms(step, output, t_x, t_a, t_b);
}

const char *csgn_uint_step_kernel(uint64_t n_bits, int step, uint64_t batch, uint64_t t_x, uint64_t t_a, uint64_t t_b)
{
    return csgn::uint_step_kernel_name(n_bits, step, batch, t_x, t_a, t_b);
}

int csgn_uint_step(uint64_t n_bits, int step, uint64_t batch, const uint64_t *d_x, uint64_t t_x, const uint64_t *d_a,
                   uint64_t t_a, const uint64_t *d_b, uint64_t t_b, uint64_t *d_out0, uint64_t *d_out1, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(step >= CSGN_UINT_ADD_HALF && step <= CSGN_UINT_LT_STEP, "unknown integer step %d", step);
    const bool uses_x = step != CSGN_UINT_ADD_HALF && step != CSGN_UINT_LT_FIRST;
    const bool carry = (step == CSGN_UINT_ADD_HALF || step == CSGN_UINT_ADD_FULL) && d_out1;
    if (!uses_x)
        t_x = 0;
    const uint64_t terms0 = csgn::uint_step_terms(step, 0, t_x, t_a, t_b);
    const uint64_t terms1 = carry ? csgn::uint_step_terms(step, 1, t_x, t_a, t_b) : 0;
    REQUIRE(terms0 != 0 && (terms1 != 0 || !carry),
            "integer step %d: an operand it reads has no terms, or the term count overflows", step);
    if (int rc = check_size(batch, terms0 > terms1 ? terms0 : terms1, terms0 + terms1, csgn_default_len(n_bits),
                            "integer step %d", step))
        return rc;
    if (int rc = require_device("csgn_uint_step"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_out0 && d_a && d_b && (d_x || !uses_x), "null device pointer");
    HIP_TRY(csgn::uint_step(n_bits, step, batch, uses_x ? (const u64 *)d_x : nullptr, t_x, (const u64 *)d_a, t_a,
                            (const u64 *)d_b, t_b, (u64 *)d_out0, carry ? (u64 *)d_out1 : nullptr, S(stream)));
    return CSGN_OK;
}

uint64_t csgn_uint_plain_terms(int cmp, uint64_t width, uint64_t k, const uint64_t *h_terms)
{
    return csgn::uint_plain_terms(cmp, width, k, (const u64 *)h_terms);
}

const char *csgn_uint_plain_kernel(uint64_t n_bits, int cmp, uint64_t batch, uint64_t width, uint64_t k,
                                   const uint64_t *h_terms)
{
    return csgn::uint_plain_kernel_name(n_bits, cmp, batch, width, k, (const u64 *)h_terms);
}

int csgn_uint_plain(uint64_t n_bits, int cmp, uint64_t batch, uint64_t width, uint64_t k,
                    const uint64_t *const *h_planes, const uint64_t *h_terms, uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(cmp >= CSGN_UINT_PLAIN_EQ && cmp <= CSGN_UINT_PLAIN_GE, "unknown comparison %d", cmp);
    if (int rc = check_width(width, k))
        return rc;
    REQUIRE(h_planes && h_terms, "null host pointer");
    const uint64_t terms = csgn::uint_plain_terms(cmp, width, k, (const u64 *)h_terms);
    REQUIRE(terms != 0, "comparison %d: a plane has no terms, or the term count overflows", cmp);
    if (int rc = check_size(batch, terms, terms, csgn_default_len(n_bits), "comparison %d", cmp))
        return rc;
    if (int rc = require_device("csgn_uint_plain"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_out, "null device pointer");
    if (int rc = check_planes(h_planes, nullptr, width, "plane"))
        return rc;
    HIP_TRY(csgn::uint_plain(n_bits, cmp, batch, width, k, (const u64 *const *)h_planes, (const u64 *)h_terms,
                             (u64 *)d_out, S(stream)));
    return CSGN_OK;
}

int csgn_uint_addk_terms(uint64_t width, uint64_t k, const uint64_t *h_terms, uint64_t *h_out_terms)
{
    return csgn::uint_addk_terms(width, k, (const u64 *)h_terms, (u64 *)h_out_terms) ? 1 : 0;
}

const char *csgn_uint_addk_kernel(uint64_t n_bits, uint64_t batch, uint64_t width, uint64_t k, const uint64_t *h_terms,
                                  int with_carry)
{
    return csgn::uint_addk_kernel_name(n_bits, batch, width, k, (const u64 *)h_terms, with_carry != 0);
}

int csgn_uint_addk(uint64_t n_bits, uint64_t batch, uint64_t width, uint64_t k, int negate_out,
                   const uint64_t *const *h_planes, const uint64_t *h_terms, uint64_t *const *h_outs, uint64_t *d_carry,
                   void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (int rc = check_width(width, k))
        return rc;
    REQUIRE(h_planes && h_terms && h_outs, "null host pointer");
    uint64_t T[65];
    REQUIRE(csgn::uint_addk_terms(width, k, (const u64 *)h_terms, (u64 *)T),
            "integer + constant: a plane has no terms, or a term count overflows");
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t j = 0; j < width + (d_carry ? 1 : 0); ++j) {
        const uint64_t terms = T[j] + (negate_out && j < width ? 1 : 0);
        if (int rc = check_size(batch, terms, terms, dl, "integer + constant: plane %llu", (unsigned long long)j))
            return rc;
    }
    if (int rc = require_device("csgn_uint_addk"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    if (int rc = check_planes(h_planes, h_outs, width, "plane"))
        return rc;
    HIP_TRY(csgn::uint_addk(n_bits, batch, width, k, negate_out != 0, (const u64 *const *)h_planes, (const u64 *)h_terms,
                            (u64 *const *)h_outs, (u64 *)d_carry, S(stream)));
    return CSGN_OK;
}

int csgn_uint_lut_anf(uint64_t in_width, uint64_t out_width, const uint64_t *h_table, uint64_t *h_anf)
{
    if (int rc = csgn::uint_lut_anf(in_width, out_width, (const u64 *)h_table, (u64 *)h_anf))
        return fail(rc, "lookup table: in_width %llu (1..16), out_width %llu (1..64), a null pointer or an entry past "
                        "out_width", (unsigned long long)in_width, (unsigned long long)out_width);
    return CSGN_OK;
}

int csgn_uint_lut_terms(uint64_t in_width, uint64_t out_width, const uint64_t *h_table, const uint64_t *h_terms,
                        uint64_t *h_out_terms)
{
    if (int rc = csgn::uint_lut_terms(in_width, out_width, (const u64 *)h_table, (const u64 *)h_terms,
                                      (u64 *)h_out_terms))
        return fail(rc, "lookup table: bad widths, a null pointer, an entry past out_width, a plane of 0 terms or a "
                        "term count of 2^62 or more");
    return CSGN_OK;
}

struct csgn_uint_lut {
    csgn::LutPlan plan;
};

int csgn_uint_lut_create(uint64_t in_width, uint64_t out_width, const uint64_t *h_table, const uint64_t *h_terms,
                         csgn_uint_lut **lut)
{
    REQUIRE(lut, "lut is null");
    *lut = nullptr;
    uint64_t T[csgn::kLutMaxOut];
    if (int rc = csgn_uint_lut_terms(in_width, out_width, h_table, h_terms, T))
        return rc;
    for (uint64_t j = 0; j < out_width; ++j)                 // at any n_bits: a term is one word or more
        if (int rc = check_size(0, T[j], T[j], 1, "lookup table: output %llu", (unsigned long long)j))
            return rc;
    if (int rc = require_device("csgn_uint_lut_create"))
        return rc;
    csgn_uint_lut *l = new csgn_uint_lut();
    hipError_t e = hipSuccess;
    const int rc = csgn::uint_lut_plan_create(in_width, out_width, (const u64 *)h_table, (const u64 *)h_terms, l->plan, e);
    if (rc != CSGN_OK) {
        delete l;
        return rc == CSGN_ERR_HIP ? hip_fail(e, "csgn_uint_lut_create") : fail(rc, "lookup table: invalid");
    }
    *lut = l;
    return CSGN_OK;
}

void csgn_uint_lut_destroy(csgn_uint_lut *lut)
{
    if (!lut)
        return;
    csgn::uint_lut_plan_free(lut->plan);
    delete lut;
}

const char *csgn_uint_lut_kernel(uint64_t n_bits, const csgn_uint_lut *lut, uint64_t batch)
{
    if (!lut || n_bits == 0)
        return "";
    return csgn::uint_lut_kernel_name(lut->plan, n_bits, batch);
}

int csgn_uint_lut_apply(const csgn_uint_lut *lut, uint64_t n_bits, uint64_t batch, const uint64_t *const *h_planes,
                        uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(lut, "lut is null");
    REQUIRE(h_planes && h_out, "null host pointer");
    const csgn::LutPlan &p = lut->plan;
    const uint64_t dl = csgn_default_len(n_bits);
    for (u32 j = 0; j < p.m; ++j)
        if (int rc = check_size(batch, p.T[j], p.T[j], dl, "lookup table: output %u", j))
            return rc;
    if (int rc = require_device("csgn_uint_lut_apply"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    if (int rc = check_planes(h_planes, nullptr, p.w, "plane"))
        return rc;
    if (int rc = check_planes(h_out, nullptr, p.m, "output"))
        return rc;
    HIP_TRY(csgn::uint_lut(p, n_bits, batch, (const u64 *const *)h_planes, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------------ gather / tile / broadcast ---- */

namespace {
// the counts every gather entry point shares; CSGN_OK or the failure (arguments are checked before the device)
int check_gather_counts(uint64_t count_in, uint64_t count_out)
{
    REQUIRE(count_in < (1ull << 32) && count_out < (1ull << 32), "gather: counts %llu -> %llu (both below 2^32)",
            (unsigned long long)count_in, (unsigned long long)count_out);
    REQUIRE(count_in > 0 || count_out == 0, "gather: %llu output elements from an empty source",
            (unsigned long long)count_out);
    return CSGN_OK;
}
} // namespace

const char *csgn_gather_kernel(uint64_t n_bits, uint64_t count_out, int ragged, uint64_t n_planes)
{
    return csgn::gather_kernel_name(n_bits, count_out, ragged != 0, n_planes);
}

int csgn_gather_plan(uint64_t count_in, const uint64_t *d_src_off, uint64_t count_out, const uint64_t *d_index,
                     uint64_t *d_out_off, uint64_t *h_result, void *stream)
{
    REQUIRE(h_result, "h_result is null");
    h_result[0] = h_result[1] = 0;
    if (count_in == 0 && count_out > 0 && d_index && count_out < (1ull << 32)) {
        h_result[1] = count_out;                                   // every index is past an empty source
        return fail(CSGN_ERR_INVALID, "gather plan: %llu indices into an empty source", (unsigned long long)count_out);
    }
    if (int rc = check_gather_counts(count_in, count_out))
        return rc;
    REQUIRE(!d_src_off || d_out_off, "gather plan: a ragged source needs d_out_off");
    if (int rc = require_device("csgn_gather_plan"))
        return rc;
    u64 result[2] = {0, 0};
    hipError_t e = hipSuccess;
    if (csgn::gather_plan(count_in, (const u64 *)d_src_off, count_out, (const u64 *)d_index, (u64 *)d_out_off, result, e,
                          S(stream)))
        return hip_fail(e, "csgn_gather_plan");
    h_result[0] = result[0];
    h_result[1] = result[1];
    if (result[1])
        return fail(CSGN_ERR_INVALID, "gather plan: %llu of %llu indices are >= count_in = %llu",
                    (unsigned long long)result[1], (unsigned long long)count_out, (unsigned long long)count_in);
    return CSGN_OK;
}

int csgn_gather(uint64_t n_bits, uint64_t count_in, const uint64_t *d_src, const uint64_t *d_src_off, uint64_t t_src,
                uint64_t count_out, const uint64_t *d_index, uint64_t *d_dst, const uint64_t *d_dst_off,
                uint64_t total_terms_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (int rc = check_gather_counts(count_in, count_out))
        return rc;
    const uint64_t dl = csgn_default_len(n_bits);
    if (!d_src_off) {
        REQUIRE(!d_dst_off, "gather: a uniform source gives a uniform output (d_dst_off must be NULL)");
        if (int rc = check_size(count_out, t_src, t_src, dl, "gather"))
            return rc;
        REQUIRE(count_out == 0 || t_src == 0 || (d_src && d_dst), "null device pointer");
        if (int rc = require_device("csgn_gather"))
            return rc;
        const u64 *src = (const u64 *)d_src;
        u64 *dst = (u64 *)d_dst;
        HIP_TRY(csgn::gather_planes(n_bits, 1, &src, (const u64 *)&t_src, count_in, count_out, (const u64 *)d_index,
                                    &dst, S(stream)));
        return CSGN_OK;
    }
    REQUIRE(d_dst_off, "gather: a ragged source needs the output offsets of its plan");
    if (!product_below(total_terms_out, dl, 1, 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "gather of %llu terms: size overflows", (unsigned long long)total_terms_out);
    REQUIRE(count_out == 0 || total_terms_out == 0 || (d_src && d_dst), "null device pointer");
    if (int rc = require_device("csgn_gather"))
        return rc;
    HIP_TRY(csgn::gather_ragged(n_bits, count_in, (const u64 *)d_src, (const u64 *)d_src_off, count_out,
                                (const u64 *)d_index, (u64 *)d_dst, (const u64 *)d_dst_off, total_terms_out, S(stream)));
    return CSGN_OK;
}

int csgn_gather_planes(uint64_t n_bits, uint64_t n_planes, const uint64_t *const *h_src, const uint64_t *h_terms,
                       uint64_t count_in, uint64_t count_out, const uint64_t *d_index, uint64_t *const *h_dst,
                       void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(n_planes >= 1 && n_planes <= csgn::kGatherMaxPlanes, "gather: %llu planes (1..64)",
            (unsigned long long)n_planes);
    REQUIRE(h_src && h_terms && h_dst, "null host pointer");
    if (int rc = check_gather_counts(count_in, count_out))
        return rc;
    const uint64_t dl = csgn_default_len(n_bits);
    uint64_t terms = 0;                                       // of the planes so far: all of them fit 2^60 words
    for (uint64_t j = 0; j < n_planes; ++j) {
        terms += h_terms[j];
        if (int rc = check_size(count_out, h_terms[j], terms, dl, "gather: plane %llu", (unsigned long long)j))
            return rc;
        REQUIRE(count_out == 0 || h_terms[j] == 0 || (h_src[j] && h_dst[j]), "null device pointer (plane %llu)",
                (unsigned long long)j);
    }
    if (int rc = require_device("csgn_gather_planes"))
        return rc;
    HIP_TRY(csgn::gather_planes(n_bits, n_planes, (const u64 *const *)h_src, (const u64 *)h_terms, count_in, count_out,
                                (const u64 *)d_index, (u64 *const *)h_dst, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------- encrypted tables at encrypted indices ---- */

uint64_t csgn_uint_read_terms(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows)
{
    return csgn::uint_read_terms(index_width, (const u64 *)h_index_terms, rows);
}

const char *csgn_uint_read_kernel(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                                  uint64_t rows, uint64_t width, const uint64_t *h_table_terms)
{
    return csgn::uint_read_kernel_name(n_bits, batch, index_width, (const u64 *)h_index_terms, rows, width,
                                       (const u64 *)h_table_terms);
}

int csgn_uint_read(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                   const uint64_t *h_index_terms, uint64_t rows, uint64_t width, const uint64_t *const *h_table,
                   const uint64_t *h_table_terms, uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (int rc = check_index("read", index_width, "table width", width, rows))
        return rc;
    REQUIRE(h_index && h_index_terms && h_table && h_table_terms && h_out, "null host pointer");
    const uint64_t E = csgn::uint_read_terms(index_width, (const u64 *)h_index_terms, rows);
    REQUIRE(E != 0, "read: an index plane has no terms, or the term count overflows");
    for (uint64_t j = 0; j < width; ++j) {
        REQUIRE(h_table_terms[j] != 0, "read: table plane %llu has no terms", (unsigned long long)j);
        if (int rc = check_index_output("read", batch, h_table_terms[j], E, csgn_default_len(n_bits), j))
            return rc;
    }
    if (int rc = require_device("csgn_uint_read"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    if (int rc = check_planes(h_index, nullptr, index_width, "index plane"))
        return rc;
    if (int rc = check_planes(h_table, h_out, width, "table plane or output"))
        return rc;
    HIP_TRY(csgn::uint_read(n_bits, batch, index_width, (const u64 *const *)h_index, (const u64 *)h_index_terms, rows,
                            width, (const u64 *const *)h_table, (const u64 *)h_table_terms, (u64 *const *)h_out,
                            S(stream)));
    return CSGN_OK;
}

/* ------------------------------------- shifts, rotates and per-element reads by encrypted amounts ---- */

uint64_t csgn_uint_pick_terms(int op, uint64_t index_width, const uint64_t *h_index_terms, uint64_t width, uint64_t rows,
                              uint64_t j)
{
    return csgn::uint_pick_terms(op, index_width, (const u64 *)h_index_terms, width, rows, j);
}

const char *csgn_uint_pick_kernel(uint64_t n_bits, int op, uint64_t batch, uint64_t index_width,
                                  const uint64_t *h_index_terms, uint64_t width, uint64_t rows, uint64_t terms)
{
    return csgn::uint_pick_kernel_name(n_bits, op, batch, index_width, (const u64 *)h_index_terms, width, rows, terms);
}

int csgn_uint_pick_plan(uint64_t n_bits, int op, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                        uint64_t width, uint64_t rows, uint64_t terms, int wide_units, uint64_t *h_plan)
{
    REQUIRE(h_plan, "null host pointer");
    REQUIRE(csgn::uint_pick_plan(n_bits, op, batch, index_width, (const u64 *)h_index_terms, width, rows, terms,
                                 wide_units != 0, (u64 *)h_plan),
            "pick plan: an invalid shape or an empty batch");
    return CSGN_OK;
}

int csgn_uint_pick(uint64_t n_bits, int op, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                   const uint64_t *h_index_terms, uint64_t width, uint64_t rows, const uint64_t *const *h_a,
                   uint64_t terms, uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(op >= CSGN_UINT_PICK_SHL && op <= CSGN_UINT_PICK_EACH, "pick: unknown op %d", op);
    if (int rc = check_index("pick", index_width, "width", width, op == CSGN_UINT_PICK_EACH ? rows : 1))
        return rc;
    REQUIRE(op == CSGN_UINT_PICK_EACH || rows == 0, "pick: rows must be 0 for a shift or rotate (%llu)",
            (unsigned long long)rows);
    REQUIRE(h_index && h_index_terms && h_a && h_out, "null host pointer");
    REQUIRE(terms != 0 && terms < (1ull << 62), "pick: a source plane of %llu terms", (unsigned long long)terms);
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t j = 0; j < width; ++j) {
        const uint64_t E = csgn::uint_pick_terms(op, index_width, (const u64 *)h_index_terms, width, rows, j);
        REQUIRE(E != 0, "pick: an index plane has no terms, or the term count overflows");
        if (int rc = check_index_output("pick", batch, terms, E, dl, j))
            return rc;
    }
    if (op == CSGN_UINT_PICK_EACH) {
        unsigned long long src_terms;                        // of an element's array in one source plane
        if (__builtin_mul_overflow((unsigned long long)terms, (unsigned long long)rows, &src_terms))
            src_terms = ~0ull;
        if (!product_below(batch, src_terms, dl, 1ull << 60))
            return fail(CSGN_ERR_UNSUPPORTED, "pick: %llu arrays of %llu rows: size overflows",
                        (unsigned long long)batch, (unsigned long long)rows);
    }
    if (int rc = require_device("csgn_uint_pick"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    if (int rc = check_planes(h_index, nullptr, index_width, "index plane"))
        return rc;
    if (int rc = check_planes(h_a, h_out, width, "source plane or output"))
        return rc;
    HIP_TRY(csgn::uint_pick(n_bits, op, batch, index_width, (const u64 *const *)h_index, (const u64 *)h_index_terms,
                            width, rows, (const u64 *const *)h_a, terms, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

int csgn_uint_pick_rows_offsets(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows,
                                const uint64_t *h_row_terms, uint64_t *h_src_off, uint64_t *h_out_off)
{
    REQUIRE(csgn::uint_pick_rows_offsets(index_width, (const u64 *)h_index_terms, rows, (const u64 *)h_row_terms,
                                         (u64 *)h_src_off, (u64 *)h_out_off),
            "pick rows: index width outside 1..16, rows outside 1..2^width, a null pointer, a term count of 0 or a count "
            "of 2^62 or more");
    return CSGN_OK;
}

// Everything csgn_uint_pick_rows decides before it touches a device, and csgn_uint_pick_rows_check's whole body.
static int pick_rows_check(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                           uint64_t rows, uint64_t width, const uint64_t *h_row_terms)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (int rc = check_index("pick rows", index_width, "width", width, rows))
        return rc;
    REQUIRE(h_index_terms && h_row_terms, "null host pointer");
    uint64_t A[csgn::kPickMaxPlanes], Tout[csgn::kPickMaxPlanes];
    REQUIRE(csgn::uint_pick_rows_sizes(index_width, (const u64 *)h_index_terms, rows, width, (const u64 *)h_row_terms,
                                       (u64 *)A, (u64 *)Tout),
            "pick rows: a term count of 0 or a count of 2^62 or more");
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t j = 0; j < width; ++j) {
        if (int rc = check_size(batch, Tout[j], Tout[j], dl, "pick rows: output %llu", (unsigned long long)j))
            return rc;
        if (!product_below(batch, A[j], dl, 1ull << 60))
            return fail(CSGN_ERR_UNSUPPORTED, "pick rows: %llu arrays of %llu terms: size overflows",
                        (unsigned long long)batch, (unsigned long long)A[j]);
    }
    return CSGN_OK;
}

int csgn_uint_pick_rows_check(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                              uint64_t rows, uint64_t width, const uint64_t *h_row_terms)
{
    return pick_rows_check(n_bits, batch, index_width, h_index_terms, rows, width, h_row_terms);
}

const char *csgn_uint_pick_rows_kernel(uint64_t n_bits, uint64_t batch, uint64_t index_width,
                                       const uint64_t *h_index_terms, uint64_t rows, uint64_t width,
                                       const uint64_t *h_row_terms)
{
    if (pick_rows_check(n_bits, batch, index_width, h_index_terms, rows, width, h_row_terms) != CSGN_OK)
        return "";
    return csgn::uint_pick_rows_kernel_name();
}

int csgn_scratch_stats(uint64_t h_out[8])
{
    REQUIRE(h_out, "null host pointer");
    csgn::scratch_stats((u64 *)h_out);
    csgn::uint_pick_rows_stats((u64 *)h_out + 5);
    return CSGN_OK;
}

int csgn_uint_pick_rows_decode(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows,
                               const uint64_t *h_row_terms, uint64_t position, uint64_t *h_out)
{
    const int rc = csgn::uint_pick_rows_decode(index_width, (const u64 *)h_index_terms, rows, (const u64 *)h_row_terms,
                                               position, (u64 *)h_out);
    if (rc == CSGN_ERR_UNSUPPORTED)
        return fail(rc, "pick rows decode: an array or an output element of 2^32 terms or more");
    REQUIRE(rc == CSGN_OK, "pick rows decode: an invalid shape, a null pointer, or position %llu past the output",
            (unsigned long long)position);
    return CSGN_OK;
}

int csgn_uint_pick_rows(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                        const uint64_t *h_index_terms, uint64_t rows, uint64_t width, const uint64_t *const *h_arrays,
                        const uint64_t *h_row_terms, uint64_t *const *h_out, void *stream)
{
    if (int rc = pick_rows_check(n_bits, batch, index_width, h_index_terms, rows, width, h_row_terms))
        return rc;
    REQUIRE(h_index && h_arrays && h_out, "null host pointer");
    if (int rc = require_device("csgn_uint_pick_rows"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    if (int rc = check_planes(h_index, nullptr, index_width, "index plane"))
        return rc;
    if (int rc = check_planes(h_arrays, h_out, width, "array plane or output"))
        return rc;
    HIP_TRY(csgn::uint_pick_rows(n_bits, batch, index_width, (const u64 *const *)h_index, (const u64 *)h_index_terms,
                                 rows, width, (const u64 *const *)h_arrays, (const u64 *)h_row_terms,
                                 (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------- encrypted arrays written at encrypted indices ---- */

uint64_t csgn_uint_write_offset(uint64_t index_width, const uint64_t *h_index_terms, uint64_t rows, uint64_t r,
                                uint64_t t_value, uint64_t t_array)
{
    return csgn::uint_write_offset(index_width, (const u64 *)h_index_terms, rows, r, t_value, t_array);
}

const char *csgn_uint_write_kernel(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                                   uint64_t rows, uint64_t width, const uint64_t *h_value_terms,
                                   const uint64_t *h_array_terms)
{
    return csgn::uint_write_kernel_name(n_bits, batch, index_width, (const u64 *)h_index_terms, rows, width,
                                        (const u64 *)h_value_terms, (const u64 *)h_array_terms);
}

int csgn_uint_write_plan(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *h_index_terms,
                         uint64_t rows, uint64_t width, const uint64_t *h_value_terms, const uint64_t *h_array_terms,
                         int wide_units, uint64_t *h_plan)
{
    REQUIRE(h_plan, "null host pointer");
    REQUIRE(csgn::uint_write_plan(n_bits, batch, index_width, (const u64 *)h_index_terms, rows, width,
                                  (const u64 *)h_value_terms, (const u64 *)h_array_terms, wide_units != 0,
                                  (u64 *)h_plan),
            "write plan: an invalid shape or an empty batch");
    return CSGN_OK;
}

int csgn_uint_write(uint64_t n_bits, uint64_t batch, uint64_t index_width, const uint64_t *const *h_index,
                    const uint64_t *h_index_terms, uint64_t rows, uint64_t width, const uint64_t *const *h_value,
                    const uint64_t *h_value_terms, const uint64_t *const *h_arrays, const uint64_t *h_array_terms,
                    uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    if (int rc = check_index("write", index_width, "width", width, rows))
        return rc;
    REQUIRE(h_index && h_index_terms && h_value && h_value_terms && h_arrays && h_array_terms && h_out,
            "null host pointer");
    const uint64_t E = csgn::uint_read_terms(index_width, (const u64 *)h_index_terms, rows);
    REQUIRE(E != 0, "write: an index plane has no terms, or the term count overflows");
    for (uint64_t j = 0; j < width; ++j) {
        REQUIRE(h_value_terms[j] != 0 && h_value_terms[j] < (1ull << 62), "write: value plane %llu of %llu terms",
                (unsigned long long)j, (unsigned long long)h_value_terms[j]);
        REQUIRE(h_array_terms[j] != 0 && h_array_terms[j] < (1ull << 62), "write: array plane %llu of %llu terms",
                (unsigned long long)j, (unsigned long long)h_array_terms[j]);
        // A_j = E * (tv + td) + rows * td; a sum or product that wraps is past every limit
        unsigned long long prod, tail, all;
        if (__builtin_mul_overflow((unsigned long long)E, (unsigned long long)(h_value_terms[j] + h_array_terms[j]),
                                   &prod) ||
            __builtin_mul_overflow((unsigned long long)rows, (unsigned long long)h_array_terms[j], &tail) ||
            __builtin_add_overflow(prod, tail, &all))
            all = ~0ull;
        if (int rc = check_size(batch, all, all, csgn_default_len(n_bits), "write: output %llu", (unsigned long long)j))
            return rc;
    }
    if (int rc = require_device("csgn_uint_write"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    if (int rc = check_planes(h_index, nullptr, index_width, "index plane"))
        return rc;
    if (int rc = check_planes(h_value, nullptr, width, "value plane"))
        return rc;
    if (int rc = check_planes(h_arrays, h_out, width, "array plane or output"))
        return rc;
    HIP_TRY(csgn::uint_write(n_bits, batch, index_width, (const u64 *const *)h_index, (const u64 *)h_index_terms, rows,
                             width, (const u64 *const *)h_value, (const u64 *)h_value_terms,
                             (const u64 *const *)h_arrays, (const u64 *)h_array_terms, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ encrypted tables by encrypted key ---- */

uint64_t csgn_uint_find_terms(uint64_t key_width, const uint64_t *h_key_terms, const uint64_t *h_query_terms)
{
    return csgn::uint_find_terms(key_width, (const u64 *)h_key_terms, (const u64 *)h_query_terms);
}

const char *csgn_uint_find_kernel(uint64_t n_bits, uint64_t batch, uint64_t key_width, const uint64_t *h_key_terms,
                                  const uint64_t *h_query_terms, uint64_t rows, uint64_t width,
                                  const uint64_t *h_value_terms, int with_member)
{
    return csgn::uint_find_kernel_name(n_bits, batch, key_width, (const u64 *)h_key_terms, (const u64 *)h_query_terms,
                                       rows, width, (const u64 *)h_value_terms, with_member != 0);
}

int csgn_uint_find(uint64_t n_bits, uint64_t batch, uint64_t key_width, const uint64_t *const *h_query,
                   const uint64_t *h_query_terms, uint64_t rows, const uint64_t *const *h_keys,
                   const uint64_t *h_key_terms, uint64_t width, const uint64_t *const *h_values,
                   const uint64_t *h_value_terms, uint64_t *const *h_out, uint64_t *d_member, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(key_width >= 1 && key_width <= csgn::kFindMaxKey, "find: key width %llu outside 1..16",
            (unsigned long long)key_width);
    REQUIRE(width <= csgn::kFindMaxPlanes, "find: value width %llu outside 0..64", (unsigned long long)width);
    REQUIRE(width >= 1 || d_member, "find: no value planes and no member output");
    REQUIRE(rows >= 1, "find: a table of no rows");
    REQUIRE(h_query && h_query_terms && h_keys && h_key_terms, "null host pointer");
    REQUIRE(width == 0 || (h_values && h_value_terms && h_out), "null host pointer");
    const uint64_t P = csgn::uint_find_terms(key_width, (const u64 *)h_key_terms, (const u64 *)h_query_terms);
    REQUIRE(P != 0, "find: a key or query plane has no terms, or the term count overflows");
    for (uint64_t j = 0; j < width; ++j)
        REQUIRE(h_value_terms[j] != 0, "find: value plane %llu has no terms", (unsigned long long)j);
    const uint64_t dl = csgn_default_len(n_bits);
    unsigned long long E;                                    // rows * P; a product that wraps is past every limit
    if (__builtin_mul_overflow((unsigned long long)rows, (unsigned long long)P, &E))
        E = ~0ull;
    for (uint64_t j = 0; j < width + (d_member ? 1 : 0); ++j) {
        unsigned long long terms;                            // of output j; the last is member's
        if (__builtin_mul_overflow(E, (unsigned long long)(j < width ? h_value_terms[j] : 1), &terms))
            terms = ~0ull;
        if (int rc = check_size(batch, terms, terms, dl, j < width ? "find: output %llu" : "find: member",
                                (unsigned long long)j))
            return rc;
    }
    if (int rc = require_device("csgn_uint_find"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    if (int rc = check_planes(h_query, h_keys, key_width, "query or key plane"))
        return rc;
    if (int rc = check_planes(h_values, h_out, width, "value plane or output"))
        return rc;
    HIP_TRY(csgn::uint_find(n_bits, batch, key_width, (const u64 *const *)h_query, (const u64 *)h_query_terms, rows,
                            (const u64 *const *)h_keys, (const u64 *)h_key_terms, width, (const u64 *const *)h_values,
                            (const u64 *)h_value_terms, (u64 *const *)h_out, (u64 *)d_member, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ the first row whose encrypted mask bit is set ---- */

uint64_t csgn_uint_first_terms(uint64_t group, const uint64_t *h_mask_terms, uint64_t row)
{
    return csgn::uint_first_terms(group, (const u64 *)h_mask_terms, row);
}

uint64_t csgn_uint_first_label_terms(uint64_t group, const uint64_t *h_mask_terms, const uint64_t *h_labels, uint64_t bit)
{
    return csgn::uint_first_label_terms(group, (const u64 *)h_mask_terms, (const u64 *)h_labels, bit);
}

int csgn_uint_first(uint64_t n_bits, uint64_t batch, uint64_t group, const uint64_t *const *h_mask, uint64_t n_mask,
                    const uint64_t *h_mask_terms, uint64_t width, const uint64_t *const *h_values,
                    const uint64_t *h_value_terms, uint64_t *const *h_out, uint64_t *d_any, uint64_t n_labels,
                    const uint64_t *h_labels, const uint64_t *h_label_bits, uint64_t *const *h_label_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(group >= 1 && group <= csgn::kFirstMaxGroup, "first: group %llu outside 1..64", (unsigned long long)group);
    REQUIRE(n_mask == 1 || (n_mask == group && group >= 2), "first: %llu mask batches for a group of %llu (1 or the group)",
            (unsigned long long)n_mask, (unsigned long long)group);
    REQUIRE(width <= csgn::kFirstMaxPlanes, "first: value width %llu outside 0..64", (unsigned long long)width);
    REQUIRE(n_labels <= csgn::kFirstMaxLabels, "first: %llu label planes outside 0..64", (unsigned long long)n_labels);
    REQUIRE(width >= 1 || d_any || n_labels >= 1, "first: no value planes, no any output and no label planes");
    REQUIRE(h_mask && h_mask_terms, "null host pointer");
    REQUIRE(width == 0 || (h_values && h_value_terms && h_out), "null host pointer");
    REQUIRE(n_labels == 0 || (h_labels && h_label_bits && h_label_out), "null host pointer");
    REQUIRE(csgn::uint_first_terms(group, (const u64 *)h_mask_terms, 0) != 0, "first: a mask row has no terms, or too many");
    const uint64_t Q = csgn::uint_first_terms(group, (const u64 *)h_mask_terms, group);
    REQUIRE((width == 0 && !d_any) || Q != 0, "first: the term count overflows");
    for (uint64_t j = 0; j < width; ++j)
        REQUIRE(h_value_terms[j] != 0, "first: value plane %llu has no terms", (unsigned long long)j);
    for (uint64_t i = 0; i < n_labels; ++i) {
        REQUIRE(h_label_bits[i] <= 63 && (i == 0 || h_label_bits[i] > h_label_bits[i - 1]),
                "first: label bits must be strictly ascending and below 64 (plane %llu)", (unsigned long long)i);
        REQUIRE(csgn::uint_first_label_terms(group, (const u64 *)h_mask_terms, (const u64 *)h_labels, h_label_bits[i]) != 0,
                "first: no label has bit %llu, or the plane's term count overflows", (unsigned long long)h_label_bits[i]);
    }
    for (uint64_t r = 1; n_mask == 1 && r < group; ++r)
        REQUIRE(h_mask_terms[r] == h_mask_terms[0], "first: the grouped layout takes one term count (row %llu)",
                (unsigned long long)r);
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t j = 0; j < width + (d_any ? 1 : 0); ++j) {
        unsigned long long terms;                            // of output j; the last is any's
        if (__builtin_mul_overflow((unsigned long long)Q, (unsigned long long)(j < width ? h_value_terms[j] : 1), &terms))
            terms = ~0ull;
        if (int rc = check_size(batch, terms, terms, dl, j < width ? "first: output %llu" : "first: any",
                                (unsigned long long)j))
            return rc;
    }
    for (uint64_t i = 0; i < n_labels; ++i) {
        const uint64_t terms =
            csgn::uint_first_label_terms(group, (const u64 *)h_mask_terms, (const u64 *)h_labels, h_label_bits[i]);
        if (int rc = check_size(batch, terms, terms, dl, "first: label plane %llu", (unsigned long long)h_label_bits[i]))
            return rc;
    }
    if (batch != 0) {
        if (int rc = check_planes(h_mask, nullptr, n_mask, "mask"))
            return rc;
        if (int rc = check_planes(h_values, h_out, width, "value plane or output"))
            return rc;
        if (int rc = check_planes(h_label_out, nullptr, n_labels, "label output"))
            return rc;
    }
    if (int rc = require_device("csgn_uint_first"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_first(n_bits, batch, group, (const u64 *const *)h_mask, n_mask, (const u64 *)h_mask_terms, width,
                             (const u64 *const *)h_values, (const u64 *)h_value_terms, (u64 *const *)h_out, (u64 *)d_any,
                             n_labels, (const u64 *)h_labels, (const u64 *)h_label_bits, (u64 *const *)h_label_out,
                             S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ the k-th row whose encrypted mask bit is set ---- */

uint64_t csgn_uint_nth_terms(uint64_t group, uint64_t t_mask, uint64_t slot, uint64_t row)
{
    return csgn::uint_nth_terms(group, t_mask, slot, row);
}

uint64_t csgn_uint_nth_label_terms(uint64_t group, uint64_t t_mask, uint64_t slot, const uint64_t *h_labels, uint64_t bit)
{
    return csgn::uint_nth_label_terms(group, t_mask, slot, (const u64 *)h_labels, bit);
}

int csgn_uint_nth(uint64_t n_bits, uint64_t batch, uint64_t group, uint64_t slot, const uint64_t *const *h_mask,
                  uint64_t n_mask, uint64_t t_mask, uint64_t width, const uint64_t *const *h_values,
                  const uint64_t *h_value_terms, uint64_t *const *h_out, uint64_t *d_valid, uint64_t n_labels,
                  const uint64_t *h_labels, const uint64_t *h_label_bits, uint64_t *const *h_label_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(group >= 1 && group <= csgn::kNthMaxGroup, "nth: group %llu outside 1..64", (unsigned long long)group);
    REQUIRE(slot < group, "nth: slot %llu of a group of %llu", (unsigned long long)slot, (unsigned long long)group);
    REQUIRE(n_mask == 1 || (n_mask == group && group >= 2), "nth: %llu mask batches for a group of %llu (1 or the group)",
            (unsigned long long)n_mask, (unsigned long long)group);
    REQUIRE(width <= csgn::kNthMaxPlanes, "nth: value width %llu outside 0..64", (unsigned long long)width);
    REQUIRE(n_labels <= csgn::kNthMaxLabels, "nth: %llu label planes outside 0..64", (unsigned long long)n_labels);
    REQUIRE(width >= 1 || d_valid || n_labels >= 1, "nth: no value planes, no valid output and no label planes");
    REQUIRE(h_mask, "null host pointer");
    REQUIRE(width == 0 || (h_values && h_value_terms && h_out), "null host pointer");
    REQUIRE(n_labels == 0 || (h_labels && h_label_bits && h_label_out), "null host pointer");
    REQUIRE(t_mask != 0 && t_mask < (1ull << 62), "nth: the mask rows have no terms, or too many");
    const uint64_t Q = csgn::uint_nth_terms(group, t_mask, slot, group);
    REQUIRE(Q != 0, "nth: the term count overflows");
    for (uint64_t j = 0; j < width; ++j)
        REQUIRE(h_value_terms[j] != 0, "nth: value plane %llu has no terms", (unsigned long long)j);
    for (uint64_t i = 0; i < n_labels; ++i) {
        REQUIRE(h_label_bits[i] <= 63 && (i == 0 || h_label_bits[i] > h_label_bits[i - 1]),
                "nth: label bits must be strictly ascending and below 64 (plane %llu)", (unsigned long long)i);
        REQUIRE(csgn::uint_nth_label_terms(group, t_mask, slot, (const u64 *)h_labels, h_label_bits[i]) != 0,
                "nth: no row from the slot on has label bit %llu, or the plane's term count overflows",
                (unsigned long long)h_label_bits[i]);
    }
    const uint64_t dl = csgn_default_len(n_bits);
    /* the stream itself, which the kernel indexes in 32 bits whatever is asked for, then every output */
    if (int rc = check_size(batch, Q, Q, dl, "nth: the selector stream"))
        return rc;
    for (uint64_t j = 0; j < width + (d_valid ? 1 : 0); ++j) {
        unsigned long long terms;                            // of output j; the last is valid's
        if (__builtin_mul_overflow((unsigned long long)Q, (unsigned long long)(j < width ? h_value_terms[j] : 1), &terms))
            terms = ~0ull;
        if (int rc = check_size(batch, terms, terms, dl, j < width ? "nth: output %llu" : "nth: valid",
                                (unsigned long long)j))
            return rc;
    }
    for (uint64_t i = 0; i < n_labels; ++i) {
        const uint64_t terms = csgn::uint_nth_label_terms(group, t_mask, slot, (const u64 *)h_labels, h_label_bits[i]);
        if (int rc = check_size(batch, terms, terms, dl, "nth: label plane %llu", (unsigned long long)h_label_bits[i]))
            return rc;
    }
    if (batch != 0) {
        if (int rc = check_planes(h_mask, nullptr, n_mask, "mask"))
            return rc;
        if (int rc = check_planes(h_values, h_out, width, "value plane or output"))
            return rc;
        if (int rc = check_planes(h_label_out, nullptr, n_labels, "label output"))
            return rc;
    }
    if (int rc = require_device("csgn_uint_nth"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_nth(n_bits, batch, group, slot, (const u64 *const *)h_mask, n_mask, t_mask, width,
                           (const u64 *const *)h_values, (const u64 *)h_value_terms, (u64 *const *)h_out, (u64 *)d_valid,
                           n_labels, (const u64 *)h_labels, (const u64 *)h_label_bits, (u64 *const *)h_label_out,
                           S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ selection by an encrypted comparison ---- */

uint64_t csgn_uint_lt_terms(uint64_t width, const uint64_t *h_a_terms, const uint64_t *h_b_terms)
{
    return csgn::uint_lt_terms(width, (const u64 *)h_a_terms, (const u64 *)h_b_terms);
}

const char *csgn_uint_lt_select_kernel(uint64_t n_bits, uint64_t batch, uint64_t width, const uint64_t *h_a_terms,
                                       const uint64_t *h_b_terms, uint64_t n_out, const uint64_t *h_x_terms,
                                       const uint64_t *h_y_terms, int with_less)
{
    return csgn::uint_lt_select_kernel_name(n_bits, batch, width, (const u64 *)h_a_terms, (const u64 *)h_b_terms, n_out,
                                            (const u64 *)h_x_terms, (const u64 *)h_y_terms, with_less != 0);
}

int csgn_uint_lt_select(uint64_t n_bits, uint64_t batch, uint64_t width, const uint64_t *const *h_a,
                        const uint64_t *h_a_terms, const uint64_t *const *h_b, const uint64_t *h_b_terms, uint64_t n_out,
                        const uint64_t *const *h_x, const uint64_t *h_x_terms, const uint64_t *const *h_y,
                        const uint64_t *h_y_terms, uint64_t *const *h_out, uint64_t *d_less, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(width >= 1 && width <= csgn::kLtSelMaxWidth, "lt_select: width %llu outside 1..16",
            (unsigned long long)width);
    REQUIRE(n_out <= csgn::kLtSelMaxOut, "lt_select: %llu outputs outside 0..64", (unsigned long long)n_out);
    REQUIRE(n_out >= 1 || d_less, "lt_select: no outputs and no comparison output");
    REQUIRE(h_a && h_a_terms && h_b && h_b_terms, "null host pointer");
    REQUIRE(n_out == 0 || (h_x && h_x_terms && h_y && h_y_terms && h_out), "null host pointer");
    const uint64_t L = csgn::uint_lt_terms(width, (const u64 *)h_a_terms, (const u64 *)h_b_terms);
    REQUIRE(L != 0, "lt_select: a plane of a or b has no terms, or the term count overflows");
    for (uint64_t i = 0; i < n_out; ++i)
        REQUIRE(h_x_terms[i] != 0 && h_y_terms[i] != 0 && h_x_terms[i] < (1ull << 62) && h_y_terms[i] < (1ull << 62),
                "lt_select: request %llu has a plane of no terms, or of 2^62 or more", (unsigned long long)i);
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t i = 0; i < n_out + (d_less ? 1 : 0); ++i) {
        unsigned long long terms = L;                        // of output i; the last is the comparison's
        if (i < n_out && (__builtin_mul_overflow((unsigned long long)L, (unsigned long long)(h_x_terms[i] + h_y_terms[i]),
                                                 &terms) ||
                          __builtin_add_overflow(terms, (unsigned long long)h_y_terms[i], &terms)))
            terms = ~0ull;                                   // a count that wraps is past every limit
        if (int rc = check_size(batch, terms, terms, dl, i < n_out ? "lt_select: output %llu" : "lt_select: the comparison",
                                (unsigned long long)i))
            return rc;
    }
    if (int rc = check_planes(h_a, h_b, width, "plane of a or b"))
        return rc;
    if (int rc = check_planes(h_x, h_y, n_out, "plane of a request"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, n_out, "output"))
        return rc;
    if (int rc = require_device("csgn_uint_lt_select"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_lt_select(n_bits, batch, width, (const u64 *const *)h_a, (const u64 *)h_a_terms,
                                 (const u64 *const *)h_b, (const u64 *)h_b_terms, n_out, (const u64 *const *)h_x,
                                 (const u64 *)h_x_terms, (const u64 *const *)h_y, (const u64 *)h_y_terms,
                                 (u64 *const *)h_out, (u64 *)d_less, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ sums, differences and equality of two integers ---- */

uint64_t csgn_uint_arith_terms(int op, uint64_t width, const uint64_t *h_a_terms, const uint64_t *h_b_terms,
                               uint64_t output)
{
    return csgn::uint_arith_terms(op, width, (const u64 *)h_a_terms, (const u64 *)h_b_terms, output);
}

const char *csgn_uint_arith_kernel(uint64_t n_bits, int op, uint64_t batch, uint64_t width, const uint64_t *h_a_terms,
                                   const uint64_t *h_b_terms, int with_carry)
{
    return csgn::uint_arith_kernel_name(n_bits, op, batch, width, (const u64 *)h_a_terms, (const u64 *)h_b_terms,
                                        with_carry != 0);
}

int csgn_uint_arith(uint64_t n_bits, int op, uint64_t batch, uint64_t width, const uint64_t *const *h_a,
                    const uint64_t *h_a_terms, const uint64_t *const *h_b, const uint64_t *h_b_terms,
                    uint64_t *const *h_out, uint64_t *d_carry, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(op >= CSGN_UINT_ARITH_ADD && op <= CSGN_UINT_ARITH_NE, "arith: unknown operation %d", op);
    REQUIRE(width >= 1 && width <= csgn::kArithMaxWidth, "arith: width %llu outside 1..16", (unsigned long long)width);
    REQUIRE(h_a && h_a_terms && h_b && h_b_terms && h_out, "null host pointer");
    const bool sum = op <= CSGN_UINT_ARITH_SUB;
    REQUIRE(sum || !d_carry, "arith: a comparison has no carry output");
    const uint64_t outputs = sum ? width + (d_carry ? 1 : 0) : 1;
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t o = 0; o < outputs; ++o)
        REQUIRE(csgn::uint_arith_terms(op, width, (const u64 *)h_a_terms, (const u64 *)h_b_terms, o) != 0,
                "arith: a plane of a or b has no terms, or the term count of output %llu overflows", (unsigned long long)o);
    for (uint64_t o = 0; o < outputs; ++o) {
        const uint64_t terms = csgn::uint_arith_terms(op, width, (const u64 *)h_a_terms, (const u64 *)h_b_terms, o);
        if (int rc = check_size(batch, terms, terms, dl, sum && o == width ? "arith: the carry" : "arith: output %llu",
                                (unsigned long long)o))
            return rc;
    }
    if (int rc = check_planes(h_a, h_b, width, "plane of a or b"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, sum ? width : 1, "output"))
        return rc;
    if (int rc = require_device("csgn_uint_arith"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_arith(n_bits, op, batch, width, (const u64 *const *)h_a, (const u64 *)h_a_terms,
                             (const u64 *const *)h_b, (const u64 *)h_b_terms, (u64 *const *)h_out, (u64 *)d_carry,
                             S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ a public constant added where an encrypted flag is set ---- */

int csgn_uint_add_where_terms(uint64_t width, uint64_t k, uint64_t t_sel, const uint64_t *h_terms, uint64_t *h_out_terms)
{
    return csgn::uint_add_where_terms(width, k, t_sel, (const u64 *)h_terms, (u64 *)h_out_terms) ? 1 : 0;
}

int csgn_uint_add_where(uint64_t n_bits, uint64_t batch, uint64_t width, uint64_t k, const uint64_t *d_sel,
                        uint64_t t_sel, const uint64_t *const *h_planes, const uint64_t *h_terms,
                        uint64_t *const *h_outs, uint64_t *d_carry, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(width >= 1 && width <= csgn::kAddWhereMaxWidth, "add_where: width %llu outside 1..32",
            (unsigned long long)width);
    REQUIRE((k >> width) == 0, "add_where: k = %llu does not fit in %llu bits", (unsigned long long)k,
            (unsigned long long)width);
    REQUIRE(h_planes && h_terms && h_outs, "null host pointer");
    const uint64_t outputs = width + (d_carry ? 1 : 0);
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t o = 0; o < outputs; ++o)
        REQUIRE(csgn::uint_add_where_output_terms(width, k, t_sel, (const u64 *)h_terms, o) != 0,
                "add_where: the flag or a plane has no terms, or the term count of output %llu overflows",
                (unsigned long long)o);
    for (uint64_t o = 0; o < outputs; ++o) {
        const uint64_t terms = csgn::uint_add_where_output_terms(width, k, t_sel, (const u64 *)h_terms, o);
        if (int rc = check_size(batch, terms, terms, dl, o == width ? "add_where: the carry" : "add_where: output %llu",
                                (unsigned long long)o))
            return rc;
    }
    if (int rc = check_planes(h_planes, nullptr, width, "plane"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_outs, nullptr, width, "output"))
        return rc;
    REQUIRE(k == 0 || d_sel, "add_where: null device pointer (the flag)");
    if (int rc = require_device("csgn_uint_add_where"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_add_where(n_bits, batch, width, k, (const u64 *)d_sel, t_sel, (const u64 *const *)h_planes,
                                 (const u64 *)h_terms, (u64 *const *)h_outs, (u64 *)d_carry, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ the plane-by-plane operators of two integers ---- */

uint64_t csgn_uint_bitwise_terms(int op, uint64_t t_sel, uint64_t t_a, uint64_t t_b)
{
    return csgn::uint_bitwise_terms(op, t_sel, t_a, t_b);
}

const char *csgn_uint_bitwise_kernel(uint64_t n_bits, int op, uint64_t batch, uint64_t width, uint64_t t_sel,
                                     const uint64_t *h_a_terms, const uint64_t *h_b_terms)
{
    return csgn::uint_bitwise_kernel_name(n_bits, op, batch, width, t_sel, (const u64 *)h_a_terms, (const u64 *)h_b_terms);
}

int csgn_uint_bitwise(uint64_t n_bits, int op, uint64_t batch, uint64_t width, const uint64_t *d_sel, uint64_t t_sel,
                      const uint64_t *const *h_a, const uint64_t *h_a_terms, const uint64_t *const *h_b,
                      const uint64_t *h_b_terms, uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(op >= CSGN_UINT_BITWISE_AND && op <= CSGN_UINT_BITWISE_KEEP, "bitwise: unknown operation %d", op);
    REQUIRE(width >= 1 && width <= csgn::kBitwiseMaxPlanes, "bitwise: width %llu outside 1..64", (unsigned long long)width);
    const bool with_b = op != CSGN_UINT_BITWISE_NOT && op != CSGN_UINT_BITWISE_KEEP;
    const bool with_sel = op == CSGN_UINT_BITWISE_SELECT || op == CSGN_UINT_BITWISE_KEEP;
    REQUIRE(h_a && h_a_terms && h_out && (!with_b || (h_b && h_b_terms)), "null host pointer");
    if (int rc = check_planes(h_a, with_b ? h_b : nullptr, width, "plane of a or b"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, width, "output"))
        return rc;
    REQUIRE(!with_sel || d_sel, "null device pointer (selector)");
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t j = 0; j < width; ++j)
        REQUIRE(csgn::uint_bitwise_terms(op, t_sel, h_a_terms[j], with_b ? h_b_terms[j] : 0) != 0,
                "bitwise: an operand of plane %llu has no terms, or the plane's term count overflows",
                (unsigned long long)j);
    for (uint64_t j = 0; j < width; ++j) {
        const uint64_t terms = csgn::uint_bitwise_terms(op, t_sel, h_a_terms[j], with_b ? h_b_terms[j] : 0);
        if (int rc = check_size(batch, terms, terms, dl, "bitwise: plane %llu", (unsigned long long)j))
            return rc;
    }
    if (int rc = require_device("csgn_uint_bitwise"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_bitwise(n_bits, op, batch, width, (const u64 *)d_sel, t_sel, (const u64 *const *)h_a,
                               (const u64 *)h_a_terms, (const u64 *const *)h_b, (const u64 *)h_b_terms,
                               (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ a public matrix over F2 applied to an integer ---- */

uint64_t csgn_uint_linear_terms(uint64_t in_width, const uint64_t *h_terms, uint64_t row, int constant_bit)
{
    return csgn::uint_linear_terms(in_width, (const u64 *)h_terms, row, constant_bit);
}

int csgn_uint_linear_decode(uint64_t in_width, const uint64_t *h_terms, uint64_t row, int constant_bit, uint64_t q,
                            uint64_t *h_plane, uint64_t *h_term)
{
    return csgn::uint_linear_decode(in_width, (const u64 *)h_terms, row, constant_bit, q, (u64 *)h_plane, (u64 *)h_term) ? 1 : 0;
}

namespace {

/* what csgn_uint_linear_plan and csgn_uint_linear check before they look at a device pointer; other_host_arrays: the
 * caller's own host arrays (the plan's table; the call's pointer arrays) are there */
int check_linear(uint64_t n_bits, uint64_t batch, uint64_t in_width, const uint64_t *h_terms, uint64_t out_width,
                 const uint64_t *h_rows, uint64_t constant, bool other_host_arrays)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(in_width >= 1 && in_width <= csgn::kLinearMaxPlanes, "linear: in_width %llu outside 1..64",
            (unsigned long long)in_width);
    if (int rc = check_width(out_width, constant))
        return rc;
    REQUIRE(h_terms && h_rows && other_host_arrays, "null host pointer");
    for (uint64_t j = 0; j < out_width; ++j)
        REQUIRE(in_width == 64 || (h_rows[j] >> in_width) == 0, "linear: row %llu names a plane at or above in_width",
                (unsigned long long)j);
    for (uint64_t i = 0; i < in_width; ++i)
        REQUIRE(h_terms[i] != 0 && h_terms[i] < (1ull << 62), "linear: input plane %llu has no terms or 2^62 or more",
                (unsigned long long)i);
    for (uint64_t j = 0; j < out_width; ++j)
        REQUIRE(csgn::uint_linear_terms(in_width, (const u64 *)h_terms, h_rows[j], (int)((constant >> j) & 1u)) != 0,
                "linear: the term count of row %llu overflows", (unsigned long long)j);
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t i = 0; i < in_width; ++i)
        if (int rc = check_size(batch, h_terms[i], h_terms[i], dl, "linear: input plane %llu", (unsigned long long)i))
            return rc;
    for (uint64_t j = 0; j < out_width; ++j) {
        const uint64_t terms = csgn::uint_linear_terms(in_width, (const u64 *)h_terms, h_rows[j], (int)((constant >> j) & 1u));
        if (int rc = check_size(batch, terms, terms, dl, "linear: output %llu", (unsigned long long)j))
            return rc;
    }
    return CSGN_OK;
}

} // namespace

int csgn_uint_linear_plan(uint64_t n_bits, uint64_t batch, uint64_t in_width, const uint64_t *h_terms, uint64_t out_width,
                          const uint64_t *h_rows, uint64_t constant, uint64_t *h_plan)
{
    if (int rc = check_linear(n_bits, batch, in_width, h_terms, out_width, h_rows, constant, h_plan != nullptr))
        return rc;
    REQUIRE(csgn::uint_linear_plan(n_bits, batch, in_width, (const u64 *)h_terms, out_width, (const u64 *)h_rows, constant,
                                   (u64 *)h_plan),
            "linear: invalid shape");
    return CSGN_OK;
}

int csgn_uint_linear(uint64_t n_bits, uint64_t batch, uint64_t in_width, const uint64_t *const *h_in,
                     const uint64_t *h_terms, uint64_t out_width, const uint64_t *h_rows, uint64_t constant,
                     uint64_t *const *h_out, void *stream)
{
    if (int rc = check_linear(n_bits, batch, in_width, h_terms, out_width, h_rows, constant, h_in && h_out))
        return rc;
    if (int rc = check_planes(h_in, nullptr, in_width, "input plane"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, out_width, "output"))
        return rc;
    if (int rc = require_device("csgn_uint_linear"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_linear(n_bits, batch, in_width, (const u64 *const *)h_in, (const u64 *)h_terms, out_width,
                              (const u64 *)h_rows, constant, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ sums of comparisons against public constants ---- */

uint64_t csgn_uint_plain_sum_terms(uint64_t width, const uint64_t *h_terms, uint64_t n_entries, const int *h_cmp,
                                   const uint64_t *h_k, int constant_bit)
{
    return csgn::uint_plain_sum_terms(width, (const u64 *)h_terms, n_entries, h_cmp, (const u64 *)h_k, constant_bit);
}

int csgn_uint_plain_sum_decode(uint64_t width, const uint64_t *h_terms, uint64_t n_entries, const int *h_cmp,
                               const uint64_t *h_k, int constant_bit, uint64_t q, uint64_t *h_level_plane,
                               uint64_t *h_level_term, uint64_t *h_n_factors)
{
    return csgn::uint_plain_sum_decode(width, (const u64 *)h_terms, n_entries, h_cmp, (const u64 *)h_k, constant_bit, q,
                                       (u64 *)h_level_plane, (u64 *)h_level_term, (u64 *)h_n_factors) ? 1 : 0;
}

namespace {

/* what csgn_uint_plain_sum_plan and csgn_uint_plain_sum_create check before the device, in the documented order */
int check_plain_sum(uint64_t width, const uint64_t *h_terms, uint64_t n_out, const uint64_t *h_first, const int *h_cmp,
                    const uint64_t *h_k, uint64_t constant, bool records, csgn::PlainSumPlan &pl)
{
    REQUIRE(width >= 1 && width <= 64, "plain sum: width %llu outside 1..64", (unsigned long long)width);
    if (int rc = check_width(n_out, constant))
        return rc;
    REQUIRE(h_terms && h_first, "null host pointer");
    REQUIRE(h_first[0] == 0, "plain sum: h_first[0] is %llu, not 0", (unsigned long long)h_first[0]);
    for (uint64_t x = 0; x < n_out; ++x)
        REQUIRE(h_first[x] <= h_first[x + 1], "plain sum: h_first descends at plane %llu", (unsigned long long)x);
    REQUIRE(h_first[n_out] == 0 || (h_cmp && h_k), "null host pointer");
    if (h_first[n_out] > csgn::kPlainSumMaxEntries)
        return fail(CSGN_ERR_UNSUPPORTED, "plain sum: %llu entries (at most 65536 a plan)",
                    (unsigned long long)h_first[n_out]);
    for (uint64_t j = 0; j < width; ++j)
        REQUIRE(h_terms[j] != 0 && h_terms[j] < (1ull << 62), "plain sum: input plane %llu has no terms or 2^62 or more",
                (unsigned long long)j);
    for (uint64_t i = 0; i < h_first[n_out]; ++i) {
        REQUIRE(h_cmp[i] >= CSGN_UINT_PLAIN_EQ && h_cmp[i] <= CSGN_UINT_PLAIN_GE, "plain sum: entry %llu: unknown "
                "comparison %d", (unsigned long long)i, h_cmp[i]);
        REQUIRE(width == 64 || (h_k[i] >> width) == 0, "plain sum: entry %llu: constant %llu does not fit in %llu bits",
                (unsigned long long)i, (unsigned long long)h_k[i], (unsigned long long)width);
    }
    const int rc = csgn::uint_plain_sum_shape(width, (const u64 *)h_terms, n_out, (const u64 *)h_first, h_cmp,
                                              (const u64 *)h_k, constant, records, pl);
    if (rc == CSGN_ERR_INVALID)
        return fail(rc, "plain sum: the term count of an entry or of a plane overflows");
    if (rc != CSGN_OK)
        return fail(rc, "plain sum: a plane of 2^31 terms per element or more");
    return CSGN_OK;
}

/* the sizes of a call: every input and output plane below 2^31 words per element and 2^60 per batch */
int check_plain_sum_sizes(const csgn::PlainSumPlan &p, uint64_t n_bits, uint64_t batch)
{
    const uint64_t dl = csgn_default_len(n_bits);
    for (u32 j = 0; j < p.w; ++j)
        if (int rc = check_size(batch, p.t[j], p.t[j], dl, "plain sum: input plane %u", j))
            return rc;
    for (u32 x = 0; x < p.n_out; ++x)
        if (int rc = check_size(batch, p.T[x], p.T[x], dl, "plain sum: output %u", x))
            return rc;
    return CSGN_OK;
}

} // namespace

struct csgn_uint_plain_sum_plan {
    csgn::PlainSumPlan plan;
};

int csgn_uint_plain_sum_launches(uint64_t n_bits, uint64_t batch, uint64_t width, const uint64_t *h_terms, uint64_t n_out,
                                 const uint64_t *h_first, const int *h_cmp, const uint64_t *h_k, uint64_t constant,
                                 uint64_t *h_plan)
{
    if (int rc = check_n(n_bits))
        return rc;
    csgn::PlainSumPlan pl;
    if (int rc = check_plain_sum(width, h_terms, n_out, h_first, h_cmp, h_k, constant, false, pl))
        return rc;
    REQUIRE(h_plan, "null host pointer");
    if (int rc = check_plain_sum_sizes(pl, n_bits, batch))
        return rc;
    csgn::uint_plain_sum_plan(pl, n_bits, batch, (u64 *)h_plan);
    return CSGN_OK;
}

int csgn_uint_plain_sum_create(uint64_t width, const uint64_t *h_terms, uint64_t n_out, const uint64_t *h_first,
                               const int *h_cmp, const uint64_t *h_k, uint64_t constant, csgn_uint_plain_sum_plan **plan)
{
    REQUIRE(plan, "plan is null");
    *plan = nullptr;
    csgn_uint_plain_sum_plan *p = new csgn_uint_plain_sum_plan();
    int rc = check_plain_sum(width, h_terms, n_out, h_first, h_cmp, h_k, constant, true, p->plan);
    if (rc == CSGN_OK)
        rc = require_device("csgn_uint_plain_sum_create");
    if (rc == CSGN_OK) {
        hipError_t e = hipSuccess;
        if (csgn::uint_plain_sum_create(p->plan, e) != CSGN_OK)
            rc = hip_fail(e, "csgn_uint_plain_sum_create");
    }
    if (rc != CSGN_OK) {
        delete p;
        return rc;
    }
    *plan = p;
    return CSGN_OK;
}

uint64_t csgn_uint_plain_sum_plan_terms(const csgn_uint_plain_sum_plan *plan, uint64_t x)
{
    return plan && x < plan->plan.n_out ? plan->plan.T[x] : 0;
}

void csgn_uint_plain_sum_destroy(csgn_uint_plain_sum_plan *plan)
{
    if (!plan)
        return;
    csgn::uint_plain_sum_free(plan->plan);
    delete plan;
}

int csgn_uint_plain_sum(const csgn_uint_plain_sum_plan *plan, uint64_t n_bits, uint64_t batch,
                        const uint64_t *const *h_planes, uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_planes && h_out, "null host pointer");
    if (!plan) {                      /* no plan exists without a device: say so before calling the pointer null */
        if (int rc = require_device("csgn_uint_plain_sum"))
            return rc;
        return fail(CSGN_ERR_INVALID, "plan is null");
    }
    const csgn::PlainSumPlan &p = plan->plan;
    if (int rc = check_plain_sum_sizes(p, n_bits, batch))
        return rc;
    if (int rc = check_planes(h_planes, nullptr, p.w, "input plane"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, p.n_out, "output"))
        return rc;
    if (int rc = require_device("csgn_uint_plain_sum"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_plain_sum(p, n_bits, batch, (const u64 *const *)h_planes, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ a public bilinear form of two encrypted integers ---- */

uint64_t csgn_uint_bilinear_terms(uint64_t wa, const uint64_t *h_ta, uint64_t wb, const uint64_t *h_tb, uint64_t n_entries,
                                  const uint64_t *h_left, const uint64_t *h_right, int constant_bit)
{
    return csgn::uint_bilinear_terms(wa, (const u64 *)h_ta, wb, (const u64 *)h_tb, n_entries, (const u64 *)h_left,
                                     (const u64 *)h_right, constant_bit);
}

int csgn_uint_bilinear_decode(uint64_t wa, const uint64_t *h_ta, uint64_t wb, const uint64_t *h_tb, uint64_t n_entries,
                              const uint64_t *h_left, const uint64_t *h_right, int constant_bit, uint64_t q,
                              uint64_t *h_entry, uint64_t *h_left_term, uint64_t *h_right_term)
{
    return csgn::uint_bilinear_decode(wa, (const u64 *)h_ta, wb, (const u64 *)h_tb, n_entries, (const u64 *)h_left,
                                      (const u64 *)h_right, constant_bit, q, (u64 *)h_entry, (u64 *)h_left_term,
                                      (u64 *)h_right_term) ? 1 : 0;
}

namespace {

/* what csgn_uint_bilinear_launches and csgn_uint_bilinear_create check before the device, in the documented order */
int check_bilinear(uint64_t wa, const uint64_t *h_ta, uint64_t wb, const uint64_t *h_tb, uint64_t n_out,
                   const uint64_t *h_first, const uint64_t *h_left, const uint64_t *h_right, uint64_t constant,
                   csgn::BilinearPlan &pl)
{
    REQUIRE(wa >= 1 && wa <= 64, "bilinear: wa %llu outside 1..64", (unsigned long long)wa);
    REQUIRE(wb >= 1 && wb <= 64, "bilinear: wb %llu outside 1..64", (unsigned long long)wb);
    if (int rc = check_width(n_out, constant))
        return rc;
    REQUIRE(h_ta && h_tb && h_first, "null host pointer");
    REQUIRE(h_first[0] == 0, "bilinear: h_first[0] is %llu, not 0", (unsigned long long)h_first[0]);
    for (uint64_t x = 0; x < n_out; ++x)
        REQUIRE(h_first[x] <= h_first[x + 1], "bilinear: h_first descends at plane %llu", (unsigned long long)x);
    REQUIRE(h_first[n_out] == 0 || (h_left && h_right), "null host pointer");
    if (h_first[n_out] > csgn::kBilinearMaxEntries)
        return fail(CSGN_ERR_UNSUPPORTED, "bilinear: %llu entries (at most 262144 a plan)",
                    (unsigned long long)h_first[n_out]);
    for (uint64_t i = 0; i < wa; ++i)
        REQUIRE(h_ta[i] != 0 && h_ta[i] < (1ull << 62), "bilinear: plane %llu of a has no terms or 2^62 or more",
                (unsigned long long)i);
    for (uint64_t l = 0; l < wb; ++l)
        REQUIRE(h_tb[l] != 0 && h_tb[l] < (1ull << 62), "bilinear: plane %llu of b has no terms or 2^62 or more",
                (unsigned long long)l);
    for (uint64_t i = 0; i < h_first[n_out]; ++i)
        REQUIRE(h_left[i] < wa && h_right[i] < wb, "bilinear: entry %llu names plane (%llu, %llu) of (%llu, %llu)",
                (unsigned long long)i, (unsigned long long)h_left[i], (unsigned long long)h_right[i],
                (unsigned long long)wa, (unsigned long long)wb);
    const int rc = csgn::uint_bilinear_shape(wa, (const u64 *)h_ta, wb, (const u64 *)h_tb, n_out, (const u64 *)h_first,
                                             (const u64 *)h_left, (const u64 *)h_right, constant, pl);
    if (rc == CSGN_ERR_INVALID)
        return fail(rc, "bilinear: the term count of an entry or of a plane overflows");
    if (rc != CSGN_OK)
        return fail(rc, "bilinear: a plane of 2^31 terms per element or more");
    return CSGN_OK;
}

/* the sizes of a call: every input and output plane below 2^31 words per element and 2^60 per batch */
int check_bilinear_sizes(const csgn::BilinearPlan &p, uint64_t n_bits, uint64_t batch)
{
    const uint64_t dl = csgn_default_len(n_bits);
    for (u32 i = 0; i < p.wa; ++i)
        if (int rc = check_size(batch, p.ta[i], p.ta[i], dl, "bilinear: plane %u of a", i))
            return rc;
    for (u32 l = 0; l < p.wb; ++l)
        if (int rc = check_size(batch, p.tb[l], p.tb[l], dl, "bilinear: plane %u of b", l))
            return rc;
    for (u32 x = 0; x < p.n_out; ++x)
        if (int rc = check_size(batch, p.T[x], p.T[x], dl, "bilinear: output %u", x))
            return rc;
    return CSGN_OK;
}

} // namespace

struct csgn_uint_bilinear_plan {
    csgn::BilinearPlan plan;
};

int csgn_uint_bilinear_launches(uint64_t n_bits, uint64_t batch, uint64_t wa, const uint64_t *h_ta, uint64_t wb,
                                const uint64_t *h_tb, uint64_t n_out, const uint64_t *h_first, const uint64_t *h_left,
                                const uint64_t *h_right, uint64_t constant, uint64_t *h_plan)
{
    if (int rc = check_n(n_bits))
        return rc;
    csgn::BilinearPlan pl;
    if (int rc = check_bilinear(wa, h_ta, wb, h_tb, n_out, h_first, h_left, h_right, constant, pl))
        return rc;
    REQUIRE(h_plan, "null host pointer");
    if (int rc = check_bilinear_sizes(pl, n_bits, batch))
        return rc;
    csgn::uint_bilinear_launches(pl, n_bits, batch, (u64 *)h_plan);
    return CSGN_OK;
}

int csgn_uint_bilinear_create(uint64_t wa, const uint64_t *h_ta, uint64_t wb, const uint64_t *h_tb, uint64_t n_out,
                              const uint64_t *h_first, const uint64_t *h_left, const uint64_t *h_right, uint64_t constant,
                              csgn_uint_bilinear_plan **plan)
{
    REQUIRE(plan, "plan is null");
    *plan = nullptr;
    csgn_uint_bilinear_plan *p = new csgn_uint_bilinear_plan();
    int rc = check_bilinear(wa, h_ta, wb, h_tb, n_out, h_first, h_left, h_right, constant, p->plan);
    if (rc == CSGN_OK)
        rc = require_device("csgn_uint_bilinear_create");
    if (rc == CSGN_OK) {
        hipError_t e = hipSuccess;
        if (csgn::uint_bilinear_create(p->plan, e) != CSGN_OK)
            rc = hip_fail(e, "csgn_uint_bilinear_create");
    }
    if (rc != CSGN_OK) {
        delete p;
        return rc;
    }
    *plan = p;
    return CSGN_OK;
}

uint64_t csgn_uint_bilinear_plan_terms(const csgn_uint_bilinear_plan *plan, uint64_t x)
{
    return plan && x < plan->plan.n_out ? plan->plan.T[x] : 0;
}

void csgn_uint_bilinear_destroy(csgn_uint_bilinear_plan *plan)
{
    if (!plan)
        return;
    csgn::uint_bilinear_free(plan->plan);
    delete plan;
}

int csgn_uint_bilinear(const csgn_uint_bilinear_plan *plan, uint64_t n_bits, uint64_t batch, const uint64_t *const *h_a,
                       const uint64_t *const *h_b, uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_a && h_b && h_out, "null host pointer");
    if (!plan) {                      /* no plan exists without a device: say so before calling the pointer null */
        if (int rc = require_device("csgn_uint_bilinear"))
            return rc;
        return fail(CSGN_ERR_INVALID, "plan is null");
    }
    const csgn::BilinearPlan &p = plan->plan;
    if (int rc = check_bilinear_sizes(p, n_bits, batch))
        return rc;
    if (int rc = check_planes(h_a, nullptr, p.wa, "plane of a"))
        return rc;
    if (int rc = check_planes(h_b, nullptr, p.wb, "plane of b"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, p.n_out, "output"))
        return rc;
    if (int rc = require_device("csgn_uint_bilinear"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_bilinear(p, n_bits, batch, (const u64 *const *)h_a, (const u64 *const *)h_b, (u64 *const *)h_out,
                                S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ a public polynomial over F2 of encrypted planes ---- */

uint64_t csgn_uint_poly_terms(uint64_t n_in, const uint64_t *h_terms, uint64_t n_monomials, const uint64_t *h_mfirst,
                              const uint64_t *h_factor, int constant_bit)
{
    return csgn::uint_poly_terms(n_in, (const u64 *)h_terms, n_monomials, (const u64 *)h_mfirst, (const u64 *)h_factor,
                                 constant_bit);
}

int csgn_uint_poly_decode(uint64_t n_in, const uint64_t *h_terms, uint64_t n_monomials, const uint64_t *h_mfirst,
                          const uint64_t *h_factor, int constant_bit, uint64_t q, uint64_t *h_monomial,
                          uint64_t *h_factor_terms)
{
    return csgn::uint_poly_decode(n_in, (const u64 *)h_terms, n_monomials, (const u64 *)h_mfirst, (const u64 *)h_factor,
                                  constant_bit, q, (u64 *)h_monomial, (u64 *)h_factor_terms) ? 1 : 0;
}

namespace {

/* what csgn_uint_poly_launches and csgn_uint_poly_create check before the device, in the documented order */
int check_poly(uint64_t n_in, const uint64_t *h_terms, uint64_t n_out, const uint64_t *h_first, const uint64_t *h_mfirst,
               const uint64_t *h_factor, uint64_t constant, csgn::PolyPlan &pl)
{
    REQUIRE(n_in >= 1 && n_in <= csgn::kPolyMaxIn, "poly: n_in %llu outside 1..256", (unsigned long long)n_in);
    if (int rc = check_width(n_out, constant))
        return rc;
    REQUIRE(h_terms && h_first, "null host pointer");
    REQUIRE(h_first[0] == 0, "poly: h_first[0] is %llu, not 0", (unsigned long long)h_first[0]);
    for (uint64_t x = 0; x < n_out; ++x)
        REQUIRE(h_first[x] <= h_first[x + 1], "poly: h_first descends at plane %llu", (unsigned long long)x);
    const uint64_t nm = h_first[n_out];
    REQUIRE(nm == 0 || (h_mfirst && h_factor), "null host pointer");
    if (nm > csgn::kPolyMaxMonomials)
        return fail(CSGN_ERR_UNSUPPORTED, "poly: %llu monomials (at most 262144 a plan)", (unsigned long long)nm);
    for (uint64_t i = 0; i < n_in; ++i)
        REQUIRE(h_terms[i] != 0 && h_terms[i] < (1ull << 62), "poly: input plane %llu has no terms or 2^62 or more",
                (unsigned long long)i);
    REQUIRE(nm == 0 || h_mfirst[0] == 0, "poly: h_mfirst[0] is not 0");
    for (uint64_t m = 0; m < nm; ++m) {
        REQUIRE(h_mfirst[m] < h_mfirst[m + 1] && h_mfirst[m + 1] - h_mfirst[m] <= csgn::kPolyMaxDegree,
                "poly: monomial %llu has a degree outside 1..8", (unsigned long long)m);
        for (uint64_t j = h_mfirst[m]; j < h_mfirst[m + 1]; ++j)
            REQUIRE(h_factor[j] < n_in, "poly: monomial %llu names plane %llu of %llu", (unsigned long long)m,
                    (unsigned long long)h_factor[j], (unsigned long long)n_in);
    }
    const int rc = csgn::uint_poly_shape(n_in, (const u64 *)h_terms, n_out, (const u64 *)h_first, (const u64 *)h_mfirst,
                                         (const u64 *)h_factor, constant, pl);
    if (rc == CSGN_ERR_INVALID)
        return fail(rc, "poly: the term count of a monomial or of a plane overflows");
    if (rc != CSGN_OK)
        return fail(rc, "poly: a plane of 2^31 terms per element or more");
    return CSGN_OK;
}

/* the sizes of a call: every input and output plane below 2^31 words per element and 2^60 per batch */
int check_poly_sizes(const csgn::PolyPlan &p, uint64_t n_bits, uint64_t batch)
{
    const uint64_t dl = csgn_default_len(n_bits);
    for (u32 i = 0; i < p.n_in; ++i)
        if (int rc = check_size(batch, p.tin[i], p.tin[i], dl, "poly: input plane %u", i))
            return rc;
    for (u32 x = 0; x < p.n_out; ++x)
        if (int rc = check_size(batch, p.T[x], p.T[x], dl, "poly: output %u", x))
            return rc;
    return CSGN_OK;
}

} // namespace

struct csgn_uint_poly_plan {
    csgn::PolyPlan plan;
};

int csgn_uint_poly_launches(uint64_t n_bits, uint64_t batch, uint64_t n_in, const uint64_t *h_terms, uint64_t n_out,
                            const uint64_t *h_first, const uint64_t *h_mfirst, const uint64_t *h_factor, uint64_t constant,
                            uint64_t *h_plan)
{
    if (int rc = check_n(n_bits))
        return rc;
    csgn::PolyPlan pl;
    if (int rc = check_poly(n_in, h_terms, n_out, h_first, h_mfirst, h_factor, constant, pl))
        return rc;
    REQUIRE(h_plan, "null host pointer");
    if (int rc = check_poly_sizes(pl, n_bits, batch))
        return rc;
    csgn::uint_poly_launches(pl, n_bits, batch, (u64 *)h_plan);
    return CSGN_OK;
}

int csgn_uint_poly_create(uint64_t n_in, const uint64_t *h_terms, uint64_t n_out, const uint64_t *h_first,
                          const uint64_t *h_mfirst, const uint64_t *h_factor, uint64_t constant, csgn_uint_poly_plan **plan)
{
    REQUIRE(plan, "plan is null");
    *plan = nullptr;
    csgn_uint_poly_plan *p = new csgn_uint_poly_plan();
    int rc = check_poly(n_in, h_terms, n_out, h_first, h_mfirst, h_factor, constant, p->plan);
    if (rc == CSGN_OK)
        rc = require_device("csgn_uint_poly_create");
    if (rc == CSGN_OK) {
        hipError_t e = hipSuccess;
        if (csgn::uint_poly_create(p->plan, e) != CSGN_OK)
            rc = hip_fail(e, "csgn_uint_poly_create");
    }
    if (rc != CSGN_OK) {
        delete p;
        return rc;
    }
    *plan = p;
    return CSGN_OK;
}

uint64_t csgn_uint_poly_plan_terms(const csgn_uint_poly_plan *plan, uint64_t x)
{
    return plan && x < plan->plan.n_out ? plan->plan.T[x] : 0;
}

void csgn_uint_poly_destroy(csgn_uint_poly_plan *plan)
{
    if (!plan)
        return;
    csgn::uint_poly_free(plan->plan);
    delete plan;
}

int csgn_uint_poly(const csgn_uint_poly_plan *plan, uint64_t n_bits, uint64_t batch, const uint64_t *const *h_in,
                   uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(h_in && h_out, "null host pointer");
    if (!plan) {                      /* no plan exists without a device: say so before calling the pointer null */
        if (int rc = require_device("csgn_uint_poly"))
            return rc;
        return fail(CSGN_ERR_INVALID, "plan is null");
    }
    const csgn::PolyPlan &p = plan->plan;
    if (int rc = check_poly_sizes(p, n_bits, batch))
        return rc;
    if (int rc = check_planes(h_in, nullptr, p.n_in, "input plane"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, p.n_out, "output"))
        return rc;
    if (int rc = require_device("csgn_uint_poly"))
        return rc;
    if (batch == 0)
        return CSGN_OK;
    HIP_TRY(csgn::uint_poly(p, n_bits, batch, (const u64 *const *)h_in, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ one-bit batches decrypted into one word per element ---- */

const char *csgn_uint_decrypt_kernel(uint64_t n_bits, uint64_t batch, uint64_t n_planes, const uint64_t *h_terms)
{
    return csgn::uint_decrypt_kernel_name(n_bits, batch, n_planes, (const u64 *)h_terms);
}

int csgn_uint_decrypt(uint64_t n_bits, uint64_t batch, uint64_t n_planes, const uint64_t *const *h_planes,
                      const uint64_t *h_terms, const uint64_t *const *h_offsets, const uint64_t *h_total_terms,
                      const uint64_t *h_max_terms, const uint64_t *d_mask, uint64_t *d_values, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(n_planes >= 1 && n_planes <= csgn::kUintDecryptMaxPlanes, "uint_decrypt: %llu planes outside 1..64",
            (unsigned long long)n_planes);
    REQUIRE(batch >= 1, "uint_decrypt: an empty batch");
    REQUIRE(h_planes && h_terms, "null host pointer");
    for (uint64_t j = 0; j < n_planes; ++j) {
        if (h_terms[j] != 0)
            continue;
        REQUIRE(h_offsets && h_total_terms && h_max_terms, "uint_decrypt: plane %llu is ragged: null host pointer",
                (unsigned long long)j);
        REQUIRE(!product_below(batch, h_max_terms[j], 1, h_total_terms[j]),
                "uint_decrypt: plane %llu: max_terms = %llu cannot hold: %llu elements of at most that many terms are "
                "fewer than total_terms = %llu", (unsigned long long)j, (unsigned long long)h_max_terms[j],
                (unsigned long long)batch, (unsigned long long)h_total_terms[j]);
    }
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t j = 0; j < n_planes; ++j) {
        const bool ragged = h_terms[j] == 0;
        if (int rc = check_size(ragged ? 1 : batch, ragged ? h_max_terms[j] : h_terms[j],
                                ragged ? h_total_terms[j] : h_terms[j], dl, "uint_decrypt: plane %llu",
                                (unsigned long long)j))
            return rc;
    }
    for (uint64_t j = 0; j < n_planes; ++j)
        if (h_terms[j] == 0 && h_max_terms[j] > csgn::kLongTerms)
            return fail(CSGN_ERR_UNSUPPORTED, "uint_decrypt: ragged plane %llu has elements of up to %llu terms (more "
                        "than %llu): decrypt it on its own", (unsigned long long)j, (unsigned long long)h_max_terms[j],
                        (unsigned long long)csgn::kLongTerms);
    if (int rc = require_device("csgn_uint_decrypt"))
        return rc;
    for (uint64_t j = 0; j < n_planes; ++j) {
        const bool ragged = h_terms[j] == 0;
        REQUIRE(h_planes[j] || (ragged && h_total_terms[j] == 0), "null device pointer (plane %llu)",
                (unsigned long long)j);
        REQUIRE(!ragged || h_offsets[j], "null device pointer (offsets of plane %llu)", (unsigned long long)j);
    }
    REQUIRE(d_mask && d_values, "null device pointer");
    HIP_TRY(csgn::uint_decrypt(n_bits, batch, n_planes, (const u64 *const *)h_planes, (const u64 *)h_terms,
                               (const u64 *const *)h_offsets, (const u64 *)h_max_terms, (const u64 *)d_mask,
                               (u64 *)d_values, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ encrypted bit matrices over F2 ---- */

uint64_t csgn_matmul_terms(uint64_t inner, uint64_t t_a, uint64_t t_b) { return csgn::matmul_terms(inner, t_a, t_b); }

const char *csgn_matmul_kernel(uint64_t n_bits, uint64_t rows, uint64_t inner, uint64_t cols, uint64_t t_a, uint64_t t_b,
                               int b_transposed)
{
    return csgn::matmul_kernel_name(n_bits, rows, inner, cols, t_a, t_b, b_transposed != 0);
}

int csgn_matmul(uint64_t n_bits, uint64_t rows, uint64_t inner, uint64_t cols, const uint64_t *d_a, uint64_t t_a,
                const uint64_t *d_b, uint64_t t_b, int b_transposed, uint64_t *d_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(rows && inner && cols, "matmul: %llu x %llu x %llu (every dimension at least 1)", (unsigned long long)rows,
            (unsigned long long)inner, (unsigned long long)cols);
    REQUIRE(t_a && t_b && t_a < (1ull << 62) && t_b < (1ull << 62), "matmul: %llu and %llu terms (1 .. 2^62 - 1)",
            (unsigned long long)t_a, (unsigned long long)t_b);
    const uint64_t dl = csgn_default_len(n_bits);
    // the terms of one output element; a product that wraps, or reaches 2^62, is past every limit
    const uint64_t T = csgn::matmul_terms(inner, t_a, t_b);
    if (T == 0 || !product_below(T, dl, 1, 1ull << 31))
        return fail(CSGN_ERR_UNSUPPORTED, "matmul: %llu x %llu x %llu terms per element exceed 2^31 words",
                    (unsigned long long)inner, (unsigned long long)t_a, (unsigned long long)t_b);
    unsigned long long elems;
    if (__builtin_mul_overflow((unsigned long long)rows, (unsigned long long)cols, &elems) ||
        !product_below(elems, T, dl, 1ull << 60))
        return fail(CSGN_ERR_UNSUPPORTED, "matmul of %llu x %llu elements: size overflows", (unsigned long long)rows,
                    (unsigned long long)cols);
    REQUIRE(d_a && d_b && d_out, "null device pointer");
    if (int rc = require_device("csgn_matmul"))
        return rc;
    HIP_TRY(csgn::matmul(n_bits, rows, inner, cols, (const u64 *)d_a, t_a, (const u64 *)d_b, t_b, b_transposed != 0,
                         (u64 *)d_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ encrypted bits counted into integers ---- */

uint64_t csgn_count_terms(uint64_t group, uint64_t t, uint64_t j) { return csgn::count_terms(group, t, j); }

const char *csgn_count_kernel(uint64_t n_bits, uint64_t count, uint64_t group, uint64_t t, uint64_t n_in,
                              uint64_t n_out, const uint64_t *h_js)
{
    return csgn::count_kernel_name(n_bits, count, group, t, n_in, n_out, (const u64 *)h_js);
}

int csgn_count(uint64_t n_bits, uint64_t count, uint64_t group, uint64_t t, const uint64_t *const *h_in, uint64_t n_in,
               uint64_t n_out, const uint64_t *h_js, uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(count && group && t && t < (1ull << 62), "count: %llu elements of %llu inputs of %llu terms (each at least 1, "
            "terms below 2^62)", (unsigned long long)count, (unsigned long long)group, (unsigned long long)t);
    REQUIRE(n_in == 1 || (n_in == group && n_in <= 64), "count: %llu input batches (1, or the group when it is 2..64)",
            (unsigned long long)n_in);
    REQUIRE(n_out >= 1, "count: no planes");
    REQUIRE(h_in && h_js && h_out, "null host pointer");
    REQUIRE(csgn::count_shape_ok(count, group, t, n_in, n_out, (const u64 *)h_js),
            "count: the planes are not strictly ascending with 2^j within the group of %llu", (unsigned long long)group);
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t x = 0; x < n_out; ++x) {
        // the terms of one output element; a count that reaches 2^62 is past every limit
        uint64_t T = csgn::count_terms(group, t, h_js[x]);
        if (T == 0)
            T = ~0ull;
        if (int rc = check_size(count, T, T, dl, "count: plane %llu", (unsigned long long)h_js[x]))
            return rc;
    }
    if (int rc = check_planes(h_in, nullptr, n_in, "input"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, n_out, "output"))
        return rc;
    if (int rc = require_device("csgn_count"))
        return rc;
    HIP_TRY(csgn::count(n_bits, count, group, t, (const u64 *const *)h_in, n_in, n_out, (const u64 *)h_js,
                        (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

uint64_t csgn_count_prefix_offset(uint64_t group, uint64_t t, uint64_t j, uint64_t exclusive, uint64_t r)
{
    return csgn::count_prefix_offset(group, t, j, exclusive, r);
}

int csgn_count_prefix(uint64_t n_bits, uint64_t count, uint64_t group, uint64_t t, uint64_t exclusive,
                      const uint64_t *const *h_in, uint64_t n_in, uint64_t n_out, const uint64_t *h_js,
                      uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(count && group && t && t < (1ull << 62), "count prefix: %llu elements of %llu inputs of %llu terms (each at "
            "least 1, terms below 2^62)", (unsigned long long)count, (unsigned long long)group, (unsigned long long)t);
    REQUIRE(exclusive <= 1, "count prefix: exclusive is %llu (0 or 1)", (unsigned long long)exclusive);
    REQUIRE(n_in == 1 || (n_in == group && n_in <= 64), "count prefix: %llu input batches (1, or the group when it is "
            "2..64)", (unsigned long long)n_in);
    REQUIRE(n_out >= 1, "count prefix: no planes");
    REQUIRE(h_in && h_js && h_out, "null host pointer");
    REQUIRE(csgn::count_prefix_shape_ok(count, group, t, exclusive, n_in, n_out, (const u64 *)h_js),
            "count prefix: the planes are not strictly ascending with 2^j within the %llu inputs of the last row",
            (unsigned long long)(group - exclusive));
    const uint64_t dl = csgn_default_len(n_bits);
    for (uint64_t x = 0; x < n_out; ++x) {
        // the terms of the last row, the longest, and of the rows together; a count that reaches 2^62 is past every limit
        uint64_t T = csgn::count_terms(group - exclusive, t, h_js[x]);
        uint64_t A = csgn::count_prefix_offset(group, t, h_js[x], exclusive, group);
        if (T == 0)
            T = ~0ull;
        if (A == 0)
            A = ~0ull;
        if (int rc = check_size(count, T, A, dl, "count prefix: plane %llu", (unsigned long long)h_js[x]))
            return rc;
    }
    if (int rc = check_planes(h_in, nullptr, n_in, "input"))
        return rc;
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, n_out, "output"))
        return rc;
    if (int rc = require_device("csgn_count_prefix"))
        return rc;
    HIP_TRY(csgn::count_prefix(n_bits, count, group, t, exclusive, (const u64 *const *)h_in, n_in, n_out,
                               (const u64 *)h_js, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------ encrypted integers summed into integers ---- */

uint64_t csgn_wsum_terms(uint64_t n_classes, const uint64_t *h_n, uint64_t t, uint64_t j)
{
    return csgn::wsum_terms(n_classes, (const u64 *)h_n, t, j);
}

struct csgn_wsum_plan {
    csgn::WsumPlan plan;
};

int csgn_wsum_create(uint64_t n_classes, const uint64_t *h_n, uint64_t t, uint64_t n_out, const uint64_t *h_js,
                     csgn_wsum_plan **plan)
{
    REQUIRE(plan, "plan is null");
    *plan = nullptr;
    REQUIRE(n_out >= 1 && n_out <= csgn::kWsumMaxPlanes && h_js, "wsum: %llu planes (1..63), or h_js is null",
            (unsigned long long)n_out);
    uint64_t T[csgn::kWsumMaxPlanes];
    const int checked = csgn::wsum_plan_check(n_classes, (const u64 *)h_n, t, n_out, (const u64 *)h_js, (u64 *)T);
    if (checked == CSGN_ERR_INVALID)
        return fail(checked, "wsum: %llu classes (1..64) of 1..65536 inputs in all, t = %llu (1..2^62 - 1), planes not "
                             "strictly ascending within 0..62, or a plane with no count vector",
                    (unsigned long long)n_classes, (unsigned long long)t);
    if (checked != CSGN_OK)
        return fail(checked, "wsum: a plane of 2^31 terms per element or more");
    if (int rc = require_device("csgn_wsum_create"))
        return rc;
    csgn_wsum_plan *p = new csgn_wsum_plan();
    hipError_t e = hipSuccess;
    const int rc = csgn::wsum_plan_create(n_classes, (const u64 *)h_n, t, n_out, (const u64 *)h_js, p->plan, e);
    if (rc != CSGN_OK) {
        delete p;
        return rc == CSGN_ERR_HIP ? hip_fail(e, "csgn_wsum_create")
                                  : fail(rc, "wsum: more than 65536 count vectors, or a monomial of more than 3072 factors");
    }
    *plan = p;
    return CSGN_OK;
}

uint64_t csgn_wsum_plan_terms(const csgn_wsum_plan *plan, uint64_t x)
{
    return plan && x < plan->plan.n_out ? plan->plan.T[x] : 0;
}

void csgn_wsum_destroy(csgn_wsum_plan *plan)
{
    if (!plan)
        return;
    csgn::wsum_plan_free(plan->plan);
    delete plan;
}

int csgn_wsum(const csgn_wsum_plan *plan, uint64_t n_bits, uint64_t count, const uint64_t *const *h_in,
              uint64_t *const *h_out, void *stream)
{
    if (int rc = check_n(n_bits))
        return rc;
    REQUIRE(plan, "plan is null");
    REQUIRE(count, "wsum: no elements");
    REQUIRE(h_in && h_out, "null host pointer");
    const csgn::WsumPlan &p = plan->plan;
    const uint64_t dl = csgn_default_len(n_bits);
    for (u32 x = 0; x < p.n_out; ++x)
        if (int rc = check_size(count, p.T[x], p.T[x], dl, "wsum: plane %u", p.js[x]))
            return rc;
    for (u32 c = 0; c < p.C; ++c) {
        unsigned long long terms;                               // of class c in one element: below 2^47
        if (__builtin_mul_overflow((unsigned long long)p.n[c], (unsigned long long)p.t, &terms))
            terms = ~0ull;
        if (!product_below(count, terms, dl, 1ull << 60))
            return fail(CSGN_ERR_UNSUPPORTED, "batch of %llu elements: size overflows", (unsigned long long)count);
    }
    for (u32 c = 0; c < p.C; ++c)
        REQUIRE(h_in[c] || p.n[c] == 0, "null device pointer (class %u)", c);
    if (int rc = check_planes((const uint64_t *const *)h_out, nullptr, p.n_out, "output"))
        return rc;
    if (int rc = require_device("csgn_wsum"))
        return rc;
    HIP_TRY(csgn::wsum(p, n_bits, count, (const u64 *const *)h_in, (u64 *const *)h_out, S(stream)));
    return CSGN_OK;
}

/* ------------------------------------------------------------------ tuning ---- */

int csgn_set_tuning(const char *key, int value)
{
    REQUIRE(key, "key is null");
    if (!csgn::tune_set(key, value))
        return fail(CSGN_ERR_INVALID, "csgn_set_tuning: no knob named '%s'", key);
    return CSGN_OK;
}

int csgn_get_tuning(const char *key, int *h_value)
{
    REQUIRE(key && h_value, "null argument");
    if (!csgn::tune_get(key, h_value))
        return fail(CSGN_ERR_INVALID, "csgn_get_tuning: no knob named '%s'", key);
    return CSGN_OK;
}

void csgn_reset_tuning(void) { csgn::tune_reset(); }

const char *csgn_tuning_name(int index) { return csgn::tune_name(index); }

/* debug hook used by the CPU tests to pin the division-by-invariant helper */
uint32_t csgn_debug_fastdiv(uint32_t n, uint32_t d)
{
    return csgn_fastdiv(n, csgn_fastdiv_make(d));
}

/* debug hook used by the CPU tests to pin the workgroup orders of csgn_device.h: xcd_grouped_block, whose group 0 is
 * xcd_contiguous_block */
uint32_t csgn_debug_block_order(uint32_t b, uint32_t nblocks, uint32_t group)
{
    return csgn::xcd_grouped_block(b, nblocks, group);
}

} // extern "C"
