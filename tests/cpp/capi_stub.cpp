// capi_stub.cpp -- the C ABI (include/csgn_hip.h) on a CPU, for the host code of the drop-in classes: the 30 entry
// points that runtime.cpp, Ciphertext.cpp, SecretKey.cpp, Context.cpp, Permutation.cpp, Helpers.cpp and Plaintext.cpp
// of csgn_amd/csrc/certfhe call, and no others -- the link fails when the class layer starts calling something the stub
// does not know.  Compiled with g++ together with those seven files and oracle/csgn_oracle.c; neither libcsgn_hip nor
// the HIP runtime is linked.  See capi_stub.h for what it checks, logs and can be told to refuse, and for what a
// synchronous stub cannot show.
#include "capi_stub.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "csgn_oracle.h"

namespace capi_stub {
namespace {

struct Block {
    size_t bytes, real;
    int kind, device;
    void *ptr;                          // (what is live at the program's end -- the result slots -- stays reachable: no leak report)
};
struct Fail {
    int skip, times, status;
};

std::mutex g_lock;
std::map<uintptr_t, Block> &g_live = *new std::map<uintptr_t, Block>();   // never destroyed: see Block::ptr
std::map<std::string, uint64_t> g_count;
std::map<std::string, Fail> g_fail;
std::vector<Call> g_log;
bool g_thin = false;
thread_local int t_device = -1;
thread_local std::string t_error;

[[noreturn]] void die(const char *entry, const char *what, const void *p, size_t bytes)
{
    printf("STUB %s: %s (pointer %p, %zu bytes, current device %d)\n", entry, what, p, bytes, t_device);
    fflush(stdout);
    _Exit(3);
}

// counts the call; the status to refuse it with, or CSGN_OK.  g_lock held.
int enter(const char *name)
{
    ++g_count[name];
    std::map<std::string, Fail>::iterator f = g_fail.find(name);
    if (f == g_fail.end())
        return CSGN_OK;
    if (f->second.skip > 0) {
        --f->second.skip;
        return CSGN_OK;
    }
    if (f->second.times > 0) {
        --f->second.times;
        t_error = std::string("stub: ") + name + " refused";
        return f->second.status;
    }
    return CSGN_OK;
}

Call &log(const char *name, const void *p0, const void *p1, size_t bytes, uint64_t n_bits, int status)
{
    g_log.push_back(Call{name, p0, p1, bytes, n_bits, t_device, status, std::vector<csgn_small_op>()});
    return g_log.back();
}

// [p, p + bytes) inside one live block of `kind` made on the current device.  g_lock held.
void inside(const char *entry, const void *p, size_t bytes, int kind)
{
    if (bytes == 0)
        return;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::map<uintptr_t, Block>::iterator it = g_live.upper_bound(a);
    if (p == nullptr || it == g_live.begin())
        die(entry, "not in a live allocation", p, bytes);
    --it;
    const Block &b = it->second;
    if (b.kind == kEvent || a - it->first >= b.bytes)
        die(entry, "not in a live allocation", p, bytes);
    if (bytes > b.bytes - (a - it->first))
        die(entry, "runs past the end of its allocation", p, bytes);
    if (b.kind != kind)
        die(entry, kind == kDevice ? "pinned memory where device memory is wanted" : "device memory where pinned memory is wanted", p,
            bytes);
    if (b.device != t_device)
        die(entry, "an allocation of another device than the current one", p, bytes);
    if (a - it->first >= b.real || bytes > b.real - (a - it->first))
        die(entry, "touches a thin allocation past its 16 real bytes", p, bytes);
}

// device memory, or pinned memory through its alias (the record array, the result slot)
void inside_either(const char *entry, const void *p, size_t bytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::map<uintptr_t, Block>::iterator it = g_live.upper_bound(a);
    int kind = kDevice;
    if (it != g_live.begin() && (--it)->second.kind == kPinned && a - it->first < it->second.bytes)
        kind = kPinned;
    inside(entry, p, bytes, kind);
}

// the host side of a copy: unchecked (the sanitizer's business) unless it starts inside a pinned block
void host_side(const char *entry, const void *p, size_t bytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::map<uintptr_t, Block>::iterator it = g_live.upper_bound(a);
    if (bytes == 0 || it == g_live.begin())
        return;
    --it;
    if (it->second.kind != kPinned || a - it->first >= it->second.bytes)
        return;
    if (bytes > it->second.bytes - (a - it->first))
        die(entry, "the host side runs past the end of its pinned block", p, bytes);
    if (bytes > it->second.real)
        die(entry, "touches a thin allocation past its 16 real bytes", p, bytes);
}

int allocate(const char *entry, void **out, size_t bytes, int kind)
{
    std::lock_guard<std::mutex> hold(g_lock);
    int rc = enter(entry);
    if (rc == CSGN_OK && (!out || bytes == 0 || t_device < 0)) {
        t_error = "stub: bad allocation request";
        rc = CSGN_ERR_INVALID;
    }
    void *p = nullptr;
    if (rc == CSGN_OK) {
        const size_t real = g_thin ? 16 : bytes;
        p = malloc(real);
        if (!p)
            die(entry, "the host is out of memory", nullptr, bytes);
        memset(p, 0xA5, real);                               // fresh memory is dirty, as on the device
        g_live[reinterpret_cast<uintptr_t>(p)] = Block{bytes, real, kind, t_device, p};
        *out = p;
    }
    log(entry, p, nullptr, bytes, 0, rc);
    return rc;
}

int release(const char *entry, void *p, int kind)
{
    std::lock_guard<std::mutex> hold(g_lock);
    const int rc = enter(entry);
    log(entry, p, nullptr, 0, 0, rc);
    if (rc != CSGN_OK)
        return rc;
    std::map<uintptr_t, Block>::iterator it = g_live.find(reinterpret_cast<uintptr_t>(p));
    if (it == g_live.end() || it->second.kind != kind)
        die(entry, "FREE of a pointer that is not live", p, 0);
    g_live.erase(it);
    free(p);
    return CSGN_OK;
}

uint64_t dl_of(uint64_t n_bits) { return csgn_oracle_default_len(n_bits); }

// the key indices a dL-word MSB-first mask stands for
std::vector<uint64_t> key_of(const uint64_t *mask, uint64_t n_bits)
{
    std::vector<uint64_t> key;
    for (uint64_t i = 0; i < n_bits; ++i)
        if ((mask[i >> 6] >> (63 - (i & 63))) & 1)
            key.push_back(i);
    return key;
}

void one_op(uint64_t dl, uint32_t kind, const uint64_t *l, uint64_t t1, const uint64_t *r, uint64_t t2, uint64_t *out)
{
    if (kind)
        csgn_oracle_mul(dl, l, t1 * dl, nullptr, r, t2 * dl, out, nullptr);
    else
        csgn_oracle_add(l, t1 * dl, nullptr, r, t2 * dl, nullptr, out, nullptr);
}

} // namespace

void stub_fail(const char *name, int skip, int times, int status)
{
    std::lock_guard<std::mutex> hold(g_lock);
    g_fail[name] = Fail{skip, times, status};
}
void stub_fail_clear()
{
    std::lock_guard<std::mutex> hold(g_lock);
    g_fail.clear();
}
void stub_thin(bool on)
{
    std::lock_guard<std::mutex> hold(g_lock);
    g_thin = on;
}
uint64_t stub_calls(const char *name)
{
    std::lock_guard<std::mutex> hold(g_lock);
    return g_count[name];
}
std::vector<Call> stub_log()
{
    std::lock_guard<std::mutex> hold(g_lock);
    return g_log;
}
size_t stub_log_size()
{
    std::lock_guard<std::mutex> hold(g_lock);
    return g_log.size();
}
std::vector<Alloc> stub_live()
{
    std::lock_guard<std::mutex> hold(g_lock);
    std::vector<Alloc> v;
    for (std::map<uintptr_t, Block>::iterator it = g_live.begin(); it != g_live.end(); ++it)
        v.push_back(Alloc{reinterpret_cast<const void *>(it->first), it->second.bytes, it->second.kind, it->second.device});
    return v;
}
size_t stub_live_count(int kind)
{
    std::lock_guard<std::mutex> hold(g_lock);
    size_t n = 0;
    for (std::map<uintptr_t, Block>::iterator it = g_live.begin(); it != g_live.end(); ++it)
        n += it->second.kind == kind;
    return n;
}
bool stub_is_live(const void *p)
{
    std::lock_guard<std::mutex> hold(g_lock);
    return g_live.count(reinterpret_cast<uintptr_t>(p)) != 0;
}

void (*stub_stream_hook)(void *stream) = nullptr;
int stub_device() { return t_device; }
void stub_set_device(int device) { t_device = device; }
int stub_allocate(const char *entry, void **out, size_t bytes, int kind) { return allocate(entry, out, bytes, kind); }
int stub_release(const char *entry, void *p, int kind) { return release(entry, p, kind); }
int stub_enter(const char *entry, const void *p0, const void *p1, size_t bytes, uint64_t n_bits)
{
    std::lock_guard<std::mutex> hold(g_lock);
    const int rc = enter(entry);
    log(entry, p0, p1, bytes, n_bits, rc);
    return rc;
}
void stub_check(const char *entry, const void *p, size_t bytes, int kind)
{
    std::lock_guard<std::mutex> hold(g_lock);
    inside(entry, p, bytes, kind);
}
void stub_set_error(const std::string &text) { t_error = text; }
void stub_die(const char *entry, const char *what, const void *p, size_t bytes) { die(entry, what, p, bytes); }

} // namespace capi_stub

using namespace capi_stub;

// stream order, where something under the stub models it (capi_stub.h): before the lock, the hook may wait
#define STREAM(stream)                 \
    if (stub_stream_hook)              \
        stub_stream_hook(stream)

// a call that only enters, checks and logs under the lock, then works outside it
#define ENTER(entry, p0, p1, bytes, n_bits, checks)          \
    {                                                        \
        std::lock_guard<std::mutex> hold(g_lock);            \
        const int rc_ = enter(entry);                        \
        log(entry, p0, p1, bytes, n_bits, rc_);              \
        if (rc_ != CSGN_OK)                                  \
            return rc_;                                      \
        checks;                                              \
    }

extern "C" {

const char *csgn_last_error(void) { return t_error.c_str(); }

int csgn_init(int device)
{
    std::lock_guard<std::mutex> hold(g_lock);
    int rc = enter("csgn_init");
    if (rc == CSGN_OK && (device < 0 || device >= 16)) {
        t_error = "stub: no such device";
        rc = CSGN_ERR_NO_DEVICE;
    }
    log("csgn_init", nullptr, nullptr, (size_t)device, 0, rc);
    if (rc == CSGN_OK)
        t_device = device;
    return rc;
}

int csgn_malloc(void **d_ptr, size_t bytes) { return allocate("csgn_malloc", d_ptr, bytes, kDevice); }
int csgn_free(void *d_ptr) { return release("csgn_free", d_ptr, kDevice); }

int csgn_host_alloc(void **h_ptr, void **d_alias, size_t bytes)
{
    const int rc = allocate("csgn_host_alloc", h_ptr, bytes, kPinned);
    if (rc == CSGN_OK && d_alias)
        *d_alias = *h_ptr;
    return rc;
}
int csgn_host_free(void *h_ptr) { return release("csgn_host_free", h_ptr, kPinned); }

int csgn_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream)
{
    STREAM(stream);
    ENTER("csgn_memcpy_h2d", d_dst, h_src, bytes, 0, (inside("csgn_memcpy_h2d", d_dst, bytes, kDevice), host_side("csgn_memcpy_h2d", h_src, bytes)));
    memcpy(d_dst, h_src, bytes);
    return CSGN_OK;
}
int csgn_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream)
{
    STREAM(stream);
    ENTER("csgn_memcpy_d2h", h_dst, d_src, bytes, 0, (inside("csgn_memcpy_d2h", d_src, bytes, kDevice), host_side("csgn_memcpy_d2h", h_dst, bytes)));
    memcpy(h_dst, d_src, bytes);
    return CSGN_OK;
}
int csgn_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream)
{
    STREAM(stream);
    ENTER("csgn_memcpy_d2d", d_dst, d_src, bytes, 0, (inside("csgn_memcpy_d2d", d_dst, bytes, kDevice), inside("csgn_memcpy_d2d", d_src, bytes, kDevice)));
    memmove(d_dst, d_src, bytes);
    return CSGN_OK;
}
int csgn_memset(void *d_dst, int value, size_t bytes, void *stream)
{
    STREAM(stream);
    ENTER("csgn_memset", d_dst, nullptr, bytes, 0, inside("csgn_memset", d_dst, bytes, kDevice));
    memset(d_dst, value, bytes);
    return CSGN_OK;
}

int csgn_stream_sync(void *stream)
{
    STREAM(stream);
    ENTER("csgn_stream_sync", nullptr, nullptr, 0, 0, (void)0);
    return CSGN_OK;
}

int csgn_event_create(void **event)
{
    std::lock_guard<std::mutex> hold(g_lock);
    const int rc = enter("csgn_event_create");
    void *e = nullptr;
    if (rc == CSGN_OK) {
        e = malloc(1);
        g_live[reinterpret_cast<uintptr_t>(e)] = Block{1, 1, kEvent, t_device, e};
        *event = e;
    }
    log("csgn_event_create", e, nullptr, 0, 0, rc);
    return rc;
}
int csgn_event_destroy(void *event) { return release("csgn_event_destroy", event, kEvent); }

static void live_event(const char *entry, void *event)
{
    std::map<uintptr_t, Block>::iterator it = g_live.find(reinterpret_cast<uintptr_t>(event));
    if (it == g_live.end() || it->second.kind != kEvent)
        die(entry, "not a live event", event, 0);
}
int csgn_event_record(void *event, void *stream)
{
    STREAM(stream);
    ENTER("csgn_event_record", event, nullptr, 0, 0, live_event("csgn_event_record", event));
    return CSGN_OK;
}
int csgn_event_sync(void *event)
{
    ENTER("csgn_event_sync", event, nullptr, 0, 0, live_event("csgn_event_sync", event));
    return CSGN_OK;
}

int csgn_synth_fill(uint64_t seed, uint64_t n_bits, uint64_t first_word, uint64_t n_words, uint64_t *d_out, void *stream)
{
    STREAM(stream);
    ENTER("csgn_synth_fill", d_out, nullptr, n_words * 8, n_bits, inside("csgn_synth_fill", d_out, n_words * 8, kDevice));
    csgn_oracle_synth_fill(seed, n_bits, first_word, n_words, d_out);
    return CSGN_OK;
}

uint64_t csgn_default_len(uint64_t n_bits) { return csgn_oracle_default_len(n_bits); }
uint64_t csgn_context_s(uint64_t n_bits, uint64_t d) { return csgn_oracle_context_s(n_bits, d); }
uint64_t csgn_mul_len(uint64_t n_bits, uint64_t len1, uint64_t len2) { return csgn_oracle_mul_len(dl_of(n_bits), len1, len2); }

int csgn_key_mask(uint64_t n_bits, const uint64_t *h_key, uint64_t d, uint64_t *h_mask)
{
    ENTER("csgn_key_mask", h_mask, h_key, d, n_bits, (void)0);
    for (uint64_t i = 0; i < d; ++i)
        if (h_key[i] >= n_bits) {
            t_error = "stub: key index >= N";
            return CSGN_ERR_INVALID;
        }
    csgn_oracle_key_mask(n_bits, h_key, d, h_mask);
    return CSGN_OK;
}

int csgn_mul_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2, const uint64_t *d_left, const uint64_t *d_right,
                     uint64_t *d_out, uint64_t out_slots, void *stream)
{
    STREAM(stream);
    const uint64_t dl = dl_of(n_bits), slots = out_slots ? out_slots : t1 * t2;
    ENTER("csgn_mul_uniform", d_out, nullptr, (size_t)(t1 << 32 | t2), n_bits,
          (inside("csgn_mul_uniform", d_left, batch * t1 * dl * 8, kDevice), inside("csgn_mul_uniform", d_right, batch * t2 * dl * 8, kDevice),
           inside("csgn_mul_uniform", d_out, batch * slots * dl * 8, kDevice)));
    for (uint64_t b = 0; b < batch; ++b)
        one_op(dl, 1, d_left + b * t1 * dl, t1, d_right + b * t2 * dl, t2, d_out + b * slots * dl);
    return CSGN_OK;
}

int csgn_add_uniform(uint64_t n_bits, uint64_t batch, uint64_t t1, uint64_t t2, const uint64_t *d_left, const uint64_t *d_right,
                     uint64_t *d_out, void *stream)
{
    STREAM(stream);
    const uint64_t dl = dl_of(n_bits);
    ENTER("csgn_add_uniform", d_out, nullptr, (size_t)(t1 << 32 | t2), n_bits,
          (inside("csgn_add_uniform", d_left, batch * t1 * dl * 8, kDevice), inside("csgn_add_uniform", d_right, batch * t2 * dl * 8, kDevice),
           inside("csgn_add_uniform", d_out, batch * (t1 + t2) * dl * 8, kDevice)));
    for (uint64_t b = 0; b < batch; ++b)
        one_op(dl, 0, d_left + b * t1 * dl, t1, d_right + b * t2 * dl, t2, d_out + b * (t1 + t2) * dl);
    return CSGN_OK;
}

int csgn_small_ops(uint64_t n_bits, uint64_t count, const csgn_small_op *d_ops, void *stream)
{
    STREAM(stream);
    const uint64_t dl = dl_of(n_bits);
    {
        std::lock_guard<std::mutex> hold(g_lock);
        const int rc = enter("csgn_small_ops");
        Call &c = log("csgn_small_ops", d_ops, nullptr, (size_t)count, n_bits, rc);
        if (rc != CSGN_OK)
            return rc;
        inside("csgn_small_ops (the record array)", d_ops, count * sizeof(csgn_small_op), kPinned);
        c.records.assign(d_ops, d_ops + count);
        for (uint64_t i = 0; i < count; ++i) {
            const csgn_small_op &op = d_ops[i];
            const uint64_t out_terms = op.kind ? (uint64_t)op.t1 * op.t2 : (uint64_t)op.t1 + op.t2;
            if (op.kind > 1 || op.t1 == 0 || op.t2 == 0)
                die("csgn_small_ops", "a record of no known kind or of no terms", &op, 0);
            inside("csgn_small_ops (left)", op.left, (size_t)op.t1 * dl * 8, kDevice);
            inside("csgn_small_ops (right)", op.right, (size_t)op.t2 * dl * 8, kDevice);
            inside("csgn_small_ops (out)", op.out, (size_t)out_terms * dl * 8, kDevice);
        }
    }
    for (uint64_t i = 0; i < count; ++i)
        one_op(dl, d_ops[i].kind, d_ops[i].left, d_ops[i].t1, d_ops[i].right, d_ops[i].t2, d_ops[i].out);
    return CSGN_OK;
}

int csgn_encrypt_explicit(uint64_t n_bits, uint64_t d, uint64_t batch, const uint8_t *d_plain, const uint64_t *d_rnd,
                          const uint32_t *d_chosen, const uint8_t *d_last, const uint64_t *d_mask, uint64_t *d_out, void *stream)
{
    STREAM(stream);
    const uint64_t dl = dl_of(n_bits);
    ENTER("csgn_encrypt_explicit", d_out, nullptr, batch, n_bits,
          (inside("csgn_encrypt_explicit", d_plain, batch, kDevice), inside("csgn_encrypt_explicit", d_rnd, batch * dl * 8, kDevice),
           inside("csgn_encrypt_explicit", d_chosen, batch * 4, kDevice), inside("csgn_encrypt_explicit", d_last, batch, kDevice),
           inside("csgn_encrypt_explicit", d_mask, dl * 8, kDevice), inside("csgn_encrypt_explicit", d_out, batch * dl * 8, kDevice)));
    (void)d;
    for (uint64_t b = 0; b < batch; ++b) {
        uint64_t *out = d_out + b * dl;
        const uint64_t *rnd = d_rnd + b * dl;
        if (d_plain[b] & 1) {                                // bit 1: every secret position is 1
            for (uint64_t k = 0; k < dl; ++k)
                out[k] = rnd[k] | d_mask[k];
        } else {                                             // bit 0: `chosen` is 0 when the other secret positions are all 1, else `last`
            const uint64_t chosen = d_chosen[b], bit = 1ull << (63 - (chosen & 63));
            bool others = false, all_one = true;
            for (uint64_t k = 0; k < dl; ++k) {
                const uint64_t m = d_mask[k] & ~(k == chosen >> 6 ? bit : 0);
                others = others || m != 0;
                all_one = all_one && (rnd[k] & m) == m;
                out[k] = rnd[k];
            }
            out[chosen >> 6] &= ~bit;
            if (!(others && all_one) && (d_last[b] & 1))
                out[chosen >> 6] |= bit;
        }
        if (n_bits % 64)
            out[dl - 1] &= ~0ull << (64 - n_bits % 64);
    }
    return CSGN_OK;
}

size_t csgn_decrypt_scratch_bytes(uint64_t batch, uint64_t total_terms) { return (size_t)((total_terms + 7) / 8 + 8 * batch); }

int csgn_decrypt_uniform(uint64_t n_bits, uint64_t batch, uint64_t terms, const uint64_t *d_terms, const uint64_t *d_mask,
                         uint8_t *d_bits, void *d_scratch, void *stream)
{
    STREAM(stream);
    const uint64_t dl = dl_of(n_bits);
    ENTER("csgn_decrypt_uniform", d_bits, d_terms, (size_t)terms, n_bits,
          (inside("csgn_decrypt_uniform", d_terms, batch * terms * dl * 8, kDevice), inside("csgn_decrypt_uniform", d_mask, dl * 8, kDevice),
           inside_either("csgn_decrypt_uniform (the bits)", d_bits, batch),
           inside("csgn_decrypt_uniform (scratch)", d_scratch, csgn_decrypt_scratch_bytes(batch, batch * terms), kDevice)));
    const std::vector<uint64_t> key = key_of(d_mask, n_bits);
    for (uint64_t b = 0; b < batch; ++b)
        d_bits[b] = (uint8_t)csgn_oracle_decrypt_canonical(n_bits, key.size(), key.data(), d_terms + b * terms * dl, terms * dl);
    return CSGN_OK;
}

size_t csgn_bitlen_scratch_bytes(uint64_t len_words) { return (size_t)(len_words + 1) * 8; }

int csgn_decrypt_bitlen(uint64_t n_bits, uint64_t d, uint64_t len_words, const uint64_t *d_v, const uint64_t *d_bitlen,
                        const uint64_t *d_key, uint8_t *d_bit, void *d_scratch, void *stream)
{
    STREAM(stream);
    ENTER("csgn_decrypt_bitlen", d_bit, d_v, (size_t)len_words, n_bits,
          (inside("csgn_decrypt_bitlen", d_v, len_words * 8, kDevice), inside("csgn_decrypt_bitlen", d_bitlen, len_words * 8, kDevice),
           inside("csgn_decrypt_bitlen", d_key, d * 8, kDevice), inside_either("csgn_decrypt_bitlen (the bit)", d_bit, 1),
           inside("csgn_decrypt_bitlen (scratch)", d_scratch, csgn_bitlen_scratch_bytes(len_words), kDevice)));
    *d_bit = (uint8_t)csgn_oracle_decrypt(n_bits, d, d_key, d_v, len_words, d_bitlen);
    return CSGN_OK;
}

int csgn_permute_bitlen(uint64_t n_bits, uint64_t len_words, const uint64_t *d_v, const uint64_t *d_bitlen, const uint32_t *d_perm,
                        uint64_t *d_out, void *d_scratch, void *stream)
{
    STREAM(stream);
    ENTER("csgn_permute_bitlen", d_out, d_v, (size_t)len_words, n_bits,
          (inside("csgn_permute_bitlen", d_v, len_words * 8, kDevice), inside("csgn_permute_bitlen", d_bitlen, len_words * 8, kDevice),
           inside("csgn_permute_bitlen", d_perm, n_bits * 4, kDevice), inside("csgn_permute_bitlen", d_out, dl_of(n_bits) * 8, kDevice),
           inside("csgn_permute_bitlen (scratch)", d_scratch, csgn_bitlen_scratch_bytes(len_words), kDevice)));
    const std::vector<uint64_t> perm(d_perm, d_perm + n_bits);
    csgn_oracle_permute_ciphertext(n_bits, perm.data(), d_v, len_words, d_bitlen, d_out);
    return CSGN_OK;
}

int csgn_permute_uniform(uint64_t n_bits, uint64_t batch, uint64_t terms_in, int per_term, const uint64_t *d_terms,
                         const uint32_t *d_perm, uint64_t *d_out, void *stream)
{
    STREAM(stream);
    const uint64_t dl = dl_of(n_bits), terms_out = per_term ? terms_in : 1;
    ENTER("csgn_permute_uniform", d_out, d_terms, (size_t)terms_in, n_bits,
          (inside("csgn_permute_uniform", d_terms, batch * terms_in * dl * 8, kDevice), inside("csgn_permute_uniform", d_perm, n_bits * 4, kDevice),
           inside("csgn_permute_uniform", d_out, batch * terms_out * dl * 8, kDevice)));
    const std::vector<uint64_t> perm(d_perm, d_perm + n_bits);
    for (uint64_t b = 0; b < batch; ++b)
        for (uint64_t t = 0; t < terms_out; ++t)
            csgn_oracle_permute_ciphertext(n_bits, perm.data(), d_terms + (b * terms_in + t) * dl, dl, nullptr,
                                           d_out + (b * terms_out + t) * dl);
    return CSGN_OK;
}

} // extern "C"
