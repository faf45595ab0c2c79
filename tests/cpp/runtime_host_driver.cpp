// runtime_host_driver.cpp -- the host code of the drop-in classes (csgn_amd/csrc/certfhe: runtime.cpp, Ciphertext.cpp,
// SecretKey.cpp) on a CPU, against tests/cpp/capi_stub.cpp instead of libcsgn_hip: the per-thread block cache, the
// process-wide pinned pool, the staging buffers, the result slot and the deferred small-operation queue with its ring of
// record slots, its hand-over between host threads and its flush at a thread's end -- with C-ABI calls that FAIL, under
// sanitizers, and with every pointer a call is handed checked against the live allocations.  Expected words come from
// this file's own loops over host copies (Val, vmul, vadd), never from the stub.  Each mode runs in a host thread of its
// own; when it has ended nothing but result slots may still be live.  The stub is synchronous: ordering on a stream is
// asserted only as "the synchronising call is in the log" (capi_stub.h).
// usage: runtime_host_driver words|batch|ring|fail_flush|exit|threads|cache|pinned|staged
// (cache_off is what `cache` runs in a child process with CSGN_NO_BLOCK_CACHE=1)
#include "driver.h"

#include <spawn.h>
#include <sys/wait.h>

#include <atomic>
#include <functional>
#include <map>
#include <set>
#include <sstream>
#include <thread>

#include "capi_stub.h"
#include "runtime.h"

extern char **environ;

using namespace certFHE;
using namespace capi_stub;
using detail::DevicePayload;

namespace {

#define EXPECT(c) expect((c), std::string(#c) + " (line " + std::to_string(__LINE__) + ")")

const size_t kBatch = detail::kDeferBatch;
const size_t kSlotBytes = sizeof(csgn_small_op) * kBatch;
const size_t MiB = (size_t)1 << 20;

// ------------------------------------------------------------------ the model: a term list on the host
struct Val {
    std::vector<uint64_t> w;
    int bit;
};

Val vmul(const Val &a, const Val &b, uint64_t dl)            // every left term AND every right term, left-major
{
    Val r;
    r.bit = a.bit & b.bit;
    for (size_t i = 0; i < a.w.size(); i += dl)
        for (size_t j = 0; j < b.w.size(); j += dl)
            for (uint64_t k = 0; k < dl; ++k)
                r.w.push_back(a.w[i + k] & b.w[j + k]);
    return r;
}

Val vadd(const Val &a, const Val &b)                         // concatenation
{
    Val r = a;
    r.w.insert(r.w.end(), b.w.begin(), b.w.end());
    r.bit = a.bit ^ b.bit;
    return r;
}

struct Setup {
    uint64_t n, d, dl;
    Context ctx;
    SecretKey sk;
    std::vector<uint64_t> key;
    Setup(uint64_t n_, uint64_t d_) : n(n_), d(d_), dl((n_ + 63) / 64), ctx(n_, d_), sk(ctx)
    {
        const uint64_t all[4] = {n - 1, 0, n / 2, n / 3};    // the last position, the first, two inside
        key.assign(all, all + d);
        sk.setKey(key.data(), d);
        srand(1000u + (unsigned)n);                          // (the key's constructor seeds from the clock)
    }
    // XOR over terms of AND over the key's positions
    int decrypt(const Val &v) const
    {
        int bit = 0;
        for (size_t t = 0; t < v.w.size(); t += dl) {
            int all_set = 1;
            for (uint64_t pos : key)
                all_set &= (int)((v.w[t + pos / 64] >> (63 - pos % 64)) & 1);
            bit ^= all_set;
        }
        return bit;
    }
    Ciphertext fresh(int bit, Val *v)
    {
        Plaintext pt(bit);
        Ciphertext c = sk.encrypt(pt);
        const uint64_t *w = c.getValues();
        v->w.assign(w, w + c.getLen());
        v->bit = bit;
        EXPECT(c.getLen() == dl && decrypt(*v) == bit);
        return c;
    }
    void check(const Ciphertext &c, const Val &v, const char *tag)
    {
        Ciphertext copy(c);                                  // (a mirror of our own: `c` may be shared with other threads)
        const bool same = copy.getLen() == v.w.size() && memcmp(copy.getValues(), v.w.data(), v.w.size() * 8) == 0;
        expect(same, std::string(tag) + ": words differ from the driver's own evaluation");
        expect((int)sk.decrypt(copy).getValue() == v.bit && decrypt(v) == v.bit, std::string(tag) + ": decrypts to the wrong bit");
    }
};

struct Lcg {
    uint32_t s;
    uint32_t operator()()
    {
        s = s * 1664525u + 1013904223u;
        return s >> 8;
    }
};

// ------------------------------------------------------------------ the stub's log
std::vector<Call> since(size_t mark)
{
    std::vector<Call> all = stub_log();
    return std::vector<Call>(all.begin() + (long)mark, all.end());
}
size_t count(const std::vector<Call> &log, const char *name, int status = CSGN_OK)
{
    size_t n = 0;
    for (const Call &c : log)
        n += c.name == name && c.status == status;
    return n;
}
std::vector<Call> only(const std::vector<Call> &log, const char *name, int status = CSGN_OK)
{
    std::vector<Call> v;
    for (const Call &c : log)
        if (c.name == name && c.status == status)
            v.push_back(c);
    return v;
}
Call first(const std::vector<Call> &log, const char *name)   // the first good call of that name; none: a call of no name
{
    const std::vector<Call> v = only(log, name);
    return v.empty() ? Call{"", nullptr, nullptr, 0, 0, -1, CSGN_OK, std::vector<csgn_small_op>()} : v[0];
}
size_t arithmetic(const std::vector<Call> &log)
{
    return count(log, "csgn_small_ops") + count(log, "csgn_mul_uniform") + count(log, "csgn_add_uniform");
}

// What must hold of every csgn_small_ops call in `log` (one thread's calls):
//  - at most kDeferBatch records, all inside ONE slot of the queue's ring, and the calls of one flush together too;
//  - no record reads what a record of the same call writes;
//  - a slot is not read by a new flush while an earlier flush's launches on it may be in flight: in between there is a
//    csgn_event_sync on an event recorded behind those launches, or a csgn_stream_sync.
void checkRecordCalls(const std::vector<Call> &log)
{
    struct Ring {
        uintptr_t base;
        int last_slot;
        size_t flush_records;
        size_t launched[8];                                          // log position of the last launch on each slot, 0: clean
    };
    std::map<uintptr_t, Ring> rings;                         // by base address
    std::map<const void *, size_t> recorded;                 // event -> log position of its last record
    for (size_t at = 0; at < log.size(); ++at) {
        const Call &c = log[at];
        if (c.status != CSGN_OK)
            continue;
        if (c.name == "csgn_host_alloc" && c.bytes == kSlotBytes * 8) {
            Ring r = {reinterpret_cast<uintptr_t>(c.p0), -1, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
            rings[r.base] = r;
        } else if (c.name == "csgn_host_free") {
            rings.erase(reinterpret_cast<uintptr_t>(c.p0));
        } else if (c.name == "csgn_event_record") {
            recorded[c.p0] = at + 1;
        } else if (c.name == "csgn_event_sync") {
            for (auto &r : rings)
                for (size_t &l : r.second.launched)
                    if (l && l < recorded[c.p0])
                        l = 0;
        } else if (c.name == "csgn_stream_sync") {
            for (auto &r : rings)
                for (size_t &l : r.second.launched)
                    l = 0;
        } else if (c.name == "csgn_small_ops") {
            const uintptr_t p = reinterpret_cast<uintptr_t>(c.p0);
            auto it = rings.upper_bound(p);
            if (it == rings.begin() || p - (--it)->first >= kSlotBytes * 8) {
                expect(false, "csgn_small_ops: the record array is not in a queue's ring");
                continue;
            }
            Ring &r = it->second;
            const int slot = (int)((p - r.base) / kSlotBytes);
            const size_t first = (p - r.base) % kSlotBytes / sizeof(csgn_small_op);
            EXPECT(c.bytes >= 1 && c.bytes <= kBatch && first + c.bytes <= kBatch);
            if (slot != r.last_slot) {                       // a new flush (every flush moves to the next slot)
                expect(r.launched[slot] == 0, "a record slot is rewritten and read again with no event or stream synchronise "
                                              "behind the launches that read it before");
                r.last_slot = slot;
                r.flush_records = 0;
            }
            r.flush_records += c.bytes;
            EXPECT(r.flush_records <= kBatch);
            r.launched[slot] = at + 1;
            const uint64_t dl = (c.n_bits + 63) / 64;
            for (const csgn_small_op &a : c.records)
                for (const csgn_small_op &b : c.records) {
                    const uint64_t *out_end = b.out + (b.kind ? (uint64_t)b.t1 * b.t2 : (uint64_t)b.t1 + b.t2) * dl;
                    const bool left = a.left < out_end && b.out < a.left + a.t1 * dl;
                    const bool right = a.right < out_end && b.out < a.right + a.t2 * dl;
                    expect(!left && !right, "csgn_small_ops: a record reads a result of its own call");
                }
        }
    }
}

// ------------------------------------------------------------------ a mode in a thread of its own
// a thread_local made FIRST in a thread is destroyed LAST: after the class layer's own (queue, block cache, staging)
struct LateWork {
    std::function<void()> run;
    ~LateWork()
    {
        if (run)
            run();
    }
};
thread_local LateWork t_late;

int inThread(void (*body)())
{
    std::string error;
    std::thread t([&] {
        try {
            body();
        } catch (const std::exception &e) {
            error = e.what();
        }
    });
    t.join();
    if (!error.empty())
        throw std::runtime_error(error);
    stub_fail_clear();
    for (const Alloc &a : stub_live())                      // the result slot stays, as documented (runtime.cpp); nothing else
        expect(a.kind == kPinned && a.bytes == 64, "still live after the mode's thread has ended: " + std::to_string(a.bytes) +
                                                       " bytes of kind " + std::to_string(a.kind));
    return 0;
}

// ------------------------------------------------------------------ words
// the program of dropin_driver's `deferred` mode, next to the model
void wordsProgram(Setup &s, bool defer, uint32_t seed)
{
    Library::deferSmallOperations(defer);
    Lcg next = {seed};
    std::vector<Ciphertext> pool;
    std::vector<Val> val;
    for (int i = 0; i < 6; ++i) {
        Val v;
        pool.push_back(s.fresh((int)(next() & 1u), &v));
        val.push_back(v);
    }
    const int nops = 40 + (int)(next() % 600u);
    for (int k = 0; k < nops; ++k) {
        const size_t ia = next() % pool.size(), ib = next() % pool.size();
        const bool mul = (next() & 1u) != 0u;
        const uint64_t ta = pool[ia].getLen() / s.dl, tb = pool[ib].getLen() / s.dl;
        if ((mul ? ta * tb : ta + tb) > 48)
            continue;
        Ciphertext res = mul ? pool[ia] * pool[ib] : pool[ia] + pool[ib];
        Val rv = mul ? vmul(val[ia], val[ib], s.dl) : vadd(val[ia], val[ib]);
        switch (next() % 4u) {
        case 0: pool.push_back(res); val.push_back(rv); break;                     // a new value
        case 1: pool[ia] = res; val[ia] = rv; break;                               // the operand is reassigned
        case 2: { Ciphertext copy(res); pool[ib] = copy; val[ib] = rv; break; }    // through a copy
        default: break;                                                            // the result dies unread
        }
        if (pool.size() > 24) {
            pool.erase(pool.begin() + 6);
            val.erase(val.begin() + 6);
        }
    }
    for (size_t i = 0; i < pool.size(); ++i)
        s.check(pool[i], val[i], defer ? "words (queued)" : "words (at once)");
}

void wordsEdges(Setup &s)
{
    Library::deferSmallOperations(true);
    Val f, v8, v9;
    Ciphertext cf = s.fresh(1, &f);
    Ciphertext c8 = cf;
    v8 = f;
    for (int i = 1; i < 8; ++i) {
        Val t;
        Ciphertext ct = s.fresh(i & 1, &t);
        c8 = c8 + ct;
        v8 = vadd(v8, t);
    }
    Ciphertext c9 = c8 + cf;
    v9 = vadd(v8, f);
    (void)c8.getValues();                                    // the queue is empty from here
    (void)c9.getValues();
    // 8 terms a side: queued, nothing reaches the C ABI until somebody looks
    size_t mark = stub_log_size();
    Ciphertext q1 = c8 * cf, q2 = cf * c8, q3 = c8 + cf, q4 = c8 * c8;
    EXPECT(arithmetic(since(mark)) == 0);
    s.check(q1, vmul(v8, f, s.dl), "8 x 1");
    s.check(q2, vmul(f, v8, s.dl), "1 x 8");
    s.check(q3, vadd(v8, f), "8 + 1");
    s.check(q4, vmul(v8, v8, s.dl), "8 x 8");
    EXPECT(count(since(mark), "csgn_small_ops") == 1 && first(since(mark), "csgn_small_ops").bytes == 4);
    // 9 terms on either side: computed by the operator itself
    struct Case {
        const Ciphertext *a, *b;
        const Val *va, *vb;
        bool mul;
    } cases[] = {{&c9, &cf, &v9, &f, true}, {&cf, &c9, &f, &v9, true}, {&c9, &cf, &v9, &f, false}, {&cf, &c9, &f, &v9, false}};
    for (const Case &c : cases) {
        mark = stub_log_size();
        Ciphertext r = c.mul ? *c.a * *c.b : *c.a + *c.b;
        const std::vector<Call> log = since(mark);
        EXPECT(count(log, "csgn_small_ops") == 0 && count(log, c.mul ? "csgn_mul_uniform" : "csgn_add_uniform") == 1);
        const Call one = first(log, c.mul ? "csgn_mul_uniform" : "csgn_add_uniform");
        EXPECT(one.bytes == ((size_t)(c.a->getLen() / s.dl) << 32 | (size_t)(c.b->getLen() / s.dl)));
        s.check(r, c.mul ? vmul(*c.va, *c.vb, s.dl) : vadd(*c.va, *c.vb), "9 terms a side");
    }
    // a custom bitlen is never queued, on either side, and follows the left operand under *
    std::vector<uint64_t> bl(s.dl, 64);
    bl[s.dl - 1] = (s.n % 64 ? s.n % 64 : 64) - 1;
    Ciphertext custom(f.w.data(), bl.data(), s.dl, s.ctx);
    EXPECT(!custom.hasCanonicalBitlen());
    for (int side = 0; side < 4; ++side) {
        mark = stub_log_size();
        const bool mul = side < 2;
        Ciphertext r = side % 2 ? (mul ? cf * custom : cf + custom) : (mul ? custom * cf : custom + cf);
        const std::vector<Call> log = since(mark);
        EXPECT(count(log, "csgn_small_ops") == 0 && count(log, mul ? "csgn_mul_uniform" : "csgn_add_uniform") == 1);
        const Val want = mul ? vmul(f, f, s.dl) : vadd(f, f);
        EXPECT(r.getLen() == want.w.size() && memcmp(r.getValues(), want.w.data(), want.w.size() * 8) == 0);
        if (side == 0)
            EXPECT(!r.hasCanonicalBitlen() && r.getBitlen()[s.dl - 1] == bl[s.dl - 1]);
    }
}

void words()
{
    const uint64_t shapes[3][2] = {{63, 2}, {129, 3}, {1247, 4}};
    for (const auto &shape : shapes) {
        Setup s(shape[0], shape[1]);
        for (int round = 0; round < 3; ++round) {
            const size_t mark = stub_log_size();
            wordsProgram(s, true, 12345u + (uint32_t)round * 77u + (uint32_t)s.n);
            EXPECT(count(since(mark), "csgn_small_ops") > 0);
            const size_t off = stub_log_size();
            wordsProgram(s, false, 12345u + (uint32_t)round * 77u + (uint32_t)s.n);
            EXPECT(count(since(off), "csgn_small_ops") == 0);
        }
        wordsEdges(s);
    }
    checkRecordCalls(stub_log());
    Library::deferSmallOperations(true);
}

// ------------------------------------------------------------------ batch
// `k` independent operations queued, then read: the calls the flushes made
void batchOf(Setup &s, size_t k)
{
    Val va, vb;
    Ciphertext a = s.fresh(1, &va), b = s.fresh(0, &vb);
    std::vector<Ciphertext> r;
    const size_t mark = stub_log_size();
    for (size_t i = 0; i < k; ++i)
        r.push_back(i % 3 == 0 ? a * b : i % 3 == 1 ? a + b : b + a);
    Library::flush();
    const std::vector<Call> log = since(mark);
    const size_t rest = k % kBatch, full = k / kBatch;
    const std::vector<Call> calls = only(log, "csgn_small_ops");
    const size_t direct = count(log, "csgn_mul_uniform") + count(log, "csgn_add_uniform");
    EXPECT(calls.size() == full + (rest > 2 ? 1 : 0));       // one level: one call a flush
    EXPECT(direct == (rest <= 2 ? rest : 0));                // one or two pending: the ordinary kernels
    size_t records = 0;
    for (const Call &c : calls)
        records += c.bytes;
    EXPECT(records + direct == k);
    checkRecordCalls(stub_log());
    for (size_t i = 0; i < k; i += (k > 40 ? 37 : 1))
        s.check(r[i], i % 3 == 0 ? vmul(va, vb, s.dl) : i % 3 == 1 ? vadd(va, vb) : vadd(vb, va), "batch");
    s.check(r[k - 1], (k - 1) % 3 == 0 ? vmul(va, vb, s.dl) : (k - 1) % 3 == 1 ? vadd(va, vb) : vadd(vb, va), "batch (last)");
}

void batch()
{
    Library::deferSmallOperations(true);
    Setup s(129, 3);
    const size_t sizes[] = {1, 2, 3, 255, 256, 257, 513};
    for (size_t k : sizes)
        batchOf(s, k);
    Val f[4];
    Ciphertext c[4] = {s.fresh(1, &f[0]), s.fresh(1, &f[1]), s.fresh(0, &f[2]), s.fresh(1, &f[3])};
    {   // depth 2, two operations on the second level
        const size_t mark = stub_log_size();
        Ciphertext p = c[0] * c[1], q = c[2] + c[3], x = p + q, y = p * p;
        Library::flush();
        const std::vector<Call> calls = only(since(mark), "csgn_small_ops");
        EXPECT(calls.size() == 2 && calls[0].bytes == 2 && calls[1].bytes == 2);
        checkRecordCalls(stub_log());
        s.check(x, vadd(vmul(f[0], f[1], s.dl), vadd(f[2], f[3])), "depth 2");
        s.check(y, vmul(vmul(f[0], f[1], s.dl), vmul(f[0], f[1], s.dl), s.dl), "depth 2");
    }
    {   // depth 256: one call a level, each reading the one before
        const size_t mark = stub_log_size();
        Ciphertext x = c[0];
        Val vx = f[0];
        for (size_t i = 0; i < kBatch; ++i) {
            x = x * c[i % 4 == 2 ? 3 : i % 4];               // (c[2] encrypts 0: leave it out so the words stay busy)
            vx = vmul(vx, f[i % 4 == 2 ? 3 : i % 4], s.dl);
        }
        Library::flush();
        const std::vector<Call> calls = only(since(mark), "csgn_small_ops");
        EXPECT(calls.size() == kBatch);
        for (size_t i = 0; i < calls.size(); ++i) {
            EXPECT(calls[i].bytes == 1);
            if (i)
                EXPECT(calls[i].records[0].left == calls[i - 1].records[0].out);
        }
        checkRecordCalls(stub_log());
        s.check(x, vx, "depth 256");
    }
    {   // a change of N in mid-queue: what is pending is evaluated when the first operation of the other size comes
        Setup t(63, 2);
        Val g[2];
        Ciphertext e[2] = {t.fresh(1, &g[0]), t.fresh(1, &g[1])};
        const size_t mark = stub_log_size();
        Ciphertext r1 = c[0] * c[1], r2 = c[0] + c[1], r3 = r1 * r2;
        EXPECT(arithmetic(since(mark)) == 0);
        Ciphertext u1 = e[0] * e[1];
        std::vector<Call> calls = only(since(mark), "csgn_small_ops");
        EXPECT(calls.size() == 2 && calls[0].n_bits == 129 && calls[0].bytes == 2 && calls[1].bytes == 1);
        Ciphertext u2 = e[0] + e[1], u3 = u1 * u2, u4 = u3 + u1;
        Library::flush();
        calls = only(since(mark), "csgn_small_ops");
        EXPECT(calls.size() == 5 && calls[2].n_bits == 63 && calls[2].bytes == 2 && calls[4].n_bits == 63);
        checkRecordCalls(stub_log());
        s.check(r3, vmul(vmul(f[0], f[1], s.dl), vadd(f[0], f[1]), s.dl), "N = 129 before the change");
        const Val vu3 = vmul(vmul(g[0], g[1], t.dl), vadd(g[0], g[1]), t.dl);
        t.check(u4, vadd(vu3, vmul(g[0], g[1], t.dl)), "N = 63 after the change");
    }
}

// ------------------------------------------------------------------ ring
void ring()
{
    Library::deferSmallOperations(true);
    Setup s(129, 3);
    Val f[3];
    Ciphertext c[3] = {s.fresh(1, &f[0]), s.fresh(0, &f[1]), s.fresh(1, &f[2])};
    std::vector<Ciphertext> held;
    std::vector<Val> want;
    std::vector<const void *> event, records;
    for (int flush = 1; flush <= 20; ++flush) {
        const size_t mark = stub_log_size();
        std::vector<Ciphertext> r;
        std::vector<Val> v;
        r.push_back(c[flush % 3] * c[0]);
        v.push_back(vmul(f[flush % 3], f[0], s.dl));
        r.push_back(c[1] + c[flush % 3]);
        v.push_back(vadd(f[1], f[flush % 3]));
        for (int more = 0; more <= flush % 4; ++more) {      // three to six operations, two levels
            r.push_back(r[(size_t)more] * c[2]);
            v.push_back(vmul(v[(size_t)more], f[2], s.dl));
        }
        Library::flush();
        const std::vector<Call> log = since(mark);
        EXPECT(count(log, "csgn_small_ops") == (flush % 4 >= 2 ? 3u : 2u) && count(log, "csgn_event_record") == 1);   // a call a level
        EXPECT(count(log, "csgn_event_create") == (flush <= 8 ? 1u : 0u));
        EXPECT(count(log, "csgn_host_alloc") == (flush == 1 ? 1u : 0u));
        EXPECT(count(log, "csgn_event_sync") == (flush <= 8 ? 0u : 1u));      // never before the ninth flush
        event.push_back(first(log, "csgn_event_record").p0);
        records.push_back(first(log, "csgn_small_ops").p0);
        if (flush > 8) {
            // on the event of the slot about to be rewritten, before its records are read again
            EXPECT(first(log, "csgn_event_sync").p0 == event[(size_t)flush - 9] && event.back() == event[(size_t)flush - 9]);
            EXPECT(records.back() == records[(size_t)flush - 9]);
            EXPECT(log[0].name == "csgn_malloc" ? log[1].name == "csgn_event_sync" : log[0].name == "csgn_event_sync");
        } else if (flush > 1) {
            EXPECT((const char *)records.back() == (const char *)records[(size_t)flush - 2] + kSlotBytes);
        }
        if (flush <= 3 || flush == 9) {                      // results of early flushes, kept to the end
            held.insert(held.end(), r.begin(), r.end());
            want.insert(want.end(), v.begin(), v.end());
        }
    }
    checkRecordCalls(stub_log());
    for (size_t i = 0; i < held.size(); ++i)
        s.check(held[i], want[i], "ring: a result held from an early flush");
}

// ------------------------------------------------------------------ fail_flush
// `flushes` flushes of three operations each
void ringFlushes(Setup &s, const Ciphertext &a, const Ciphertext &b, int flushes)
{
    for (int i = 0; i < flushes; ++i) {
        Ciphertext x = a * b, y = a + b, z = x * y;
        Library::flush();
    }
    (void)s;
}

// a full queue whose flush cannot allocate: the operator throws, nothing is written outside a slot, no later call has
// more than kDeferBatch records, and everything still held has the right words once allocation works again
void failFull()
{
    Library::deferSmallOperations(true);
    Setup s(129, 3);
    Val va, vb;
    Ciphertext a = s.fresh(1, &va), b = s.fresh(1, &vb);
    const size_t begin = stub_log_size();
    ringFlushes(s, a, b, 7);                                 // the ring stands at its last slot
    std::vector<Ciphertext> held;
    std::vector<Val> want;
    auto op = [&](size_t i) {
        // operands: the fresh pair and results still pending
        const size_t n = held.size();
        const Ciphertext &l = n && i % 5 == 1 ? held[n - 1] : a;
        const Val &vl = n && i % 5 == 1 ? want[n - 1] : va;
        const bool mul = i % 2 == 0 || vl.w.size() / s.dl >= 8;
        Ciphertext r = mul ? l * b : l + b;
        held.push_back(r);
        want.push_back(mul ? vmul(vl, vb, s.dl) : vadd(vl, vb));
    };
    for (size_t i = 0; i < kBatch - 1; ++i)
        op(i);
    EXPECT(arithmetic(since(begin)) == 7 * 2);
    Library::releaseDeviceCache();
    { Val t; (void)s.fresh(0, &t); }                         // (something in the cache: take() then drops it and retries once)
    stub_fail("csgn_malloc", 0, 2, CSGN_ERR_HIP);
    int thrown = 0;
    for (size_t i = kBatch - 1; i < kBatch + 1 && !thrown; ++i) {           // the 256th operation, or the one after it
        try {
            op(i);
        } catch (const std::runtime_error &e) {
            ++thrown;
            EXPECT(std::string(e.what()).find("csgn_malloc") != std::string::npos);
        }
    }
    EXPECT(thrown == 1);
    EXPECT(count(since(begin), "csgn_malloc", CSGN_ERR_HIP) == 2);
    stub_fail_clear();
    for (size_t i = 0; i < 40; ++i)
        op(kBatch + 1 + i);
    for (size_t i = 0; i < held.size(); ++i)
        s.check(held[i], want[i], "fail_flush: held across a failed flush of a full queue");
    checkRecordCalls(stub_log());
}

// one flush of three levels fails in the middle (`entry` refused after `skip` good calls); the queue then works
void failOnce(const char *entry, int skip, const char *follows)
{
    Library::deferSmallOperations(true);
    Setup s(63, 2);
    Val va, vb;
    Ciphertext a = s.fresh(1, &va), b = s.fresh(1, &vb);
    for (int round = 0; round < 10; ++round) {              // (past the ring's length: the failed slot comes round again)
        Ciphertext p = a * b, q = p + a, r = q * b, t = a + b;
        const Val vp = vmul(va, vb, s.dl), vq = vadd(vp, va), vr = vmul(vq, vb, s.dl), vt = vadd(va, vb);
        if (round == 1) {
            const size_t mark = stub_log_size();
            stub_fail(entry, skip, 1, CSGN_ERR_HIP);
            bool thrown = false;
            try {
                (void)r.getValues();
            } catch (const std::runtime_error &e) {
                thrown = std::string(e.what()).find(entry) != std::string::npos;
            }
            EXPECT(thrown);
            const std::vector<Call> log = since(mark);
            EXPECT(count(log, entry, CSGN_ERR_HIP) == 1);
            if (follows) {                                   // the launches already issued stay guarded
                size_t at = 0;
                while (at < log.size() && log[at].status == CSGN_OK)
                    ++at;
                bool seen = false;
                for (size_t i = at + 1; i < log.size(); ++i)
                    seen = seen || (log[i].name == follows && log[i].status == CSGN_OK);
                expect(seen, std::string("after a refused ") + entry + " no " + follows + " follows");
            }
            stub_fail_clear();
        }
        s.check(r, vr, "fail_flush: after a failed flush");
        s.check(p, vp, "fail_flush: after a failed flush");
        s.check(q, vq, "fail_flush: after a failed flush");
        s.check(t, vt, "fail_flush: after a failed flush");
    }
    checkRecordCalls(stub_log());
}

// the first flush of a NEW queue cannot make its records or its first event
void failFirst(const char *entry)
{
    Library::deferSmallOperations(true);
    Setup s(1247, 4);
    Val va, vb;
    Ciphertext a = s.fresh(0, &va), b = s.fresh(1, &vb);
    const size_t begin = stub_log_size();
    Ciphertext p = a * b, q = p + a, r = q * b;
    stub_fail(entry, 0, 1, CSGN_ERR_HIP);
    EXPECT(throws<std::runtime_error>([&] { Library::flush(); }));
    EXPECT(count(since(begin), entry, CSGN_ERR_HIP) == 1);
    Ciphertext t = r + p;                                    // the queue takes more
    ringFlushes(s, a, b, 9);
    const Val vp = vmul(va, vb, s.dl), vq = vadd(vp, va), vr = vmul(vq, vb, s.dl);
    s.check(t, vadd(vr, vp), "fail_flush: a queue whose first flush failed");
    s.check(r, vr, "fail_flush: a queue whose first flush failed");
    checkRecordCalls(stub_log());
}

void failFlush()
{
    failFull();
    failOnce("csgn_small_ops", 1, "csgn_event_record");
    failOnce("csgn_event_record", 0, "csgn_stream_sync");
}
void failFirstRecords() { failFirst("csgn_host_alloc"); }
void failFirstEvent() { failFirst("csgn_event_create"); }

// ------------------------------------------------------------------ exit
struct Handed {
    std::vector<Ciphertext> got;
    std::vector<Val> want;
};

// queues 3 + extra operations on a, b; the results go to *out
void queueSome(Setup &s, const Ciphertext &a, const Val &va, const Ciphertext &b, const Val &vb, int extra, Handed *out)
{
    out->got.push_back(a * b);
    out->want.push_back(vmul(va, vb, s.dl));
    out->got.push_back(out->got[0] + a);
    out->want.push_back(vadd(out->want[0], va));
    out->got.push_back(out->got[1] * out->got[0]);
    out->want.push_back(vmul(out->want[1], out->want[0], s.dl));
    for (int i = 0; i < extra; ++i) {
        out->got.push_back(out->got[(size_t)i] + b);
        out->want.push_back(vadd(out->want[(size_t)i], vb));
    }
}

void exitMode()
{
    Library::deferSmallOperations(true);
    Setup s(1247, 4);
    Val va, vb;
    Ciphertext a = s.fresh(1, &va), b = s.fresh(1, &vb);
    for (int extra = 0; extra < 6; extra += 5) {             // a working stub: the worker's exit evaluates its queue
        Handed h;
        const size_t mark = stub_log_size();
        std::thread worker([&] { queueSome(s, a, va, b, vb, extra, &h); });
        worker.join();
        EXPECT(count(since(mark), "csgn_small_ops") == (extra ? 4u : 3u));      // a call a level
        const size_t read = stub_log_size();
        for (size_t i = 0; i < h.got.size(); ++i)
            s.check(h.got[i], h.want[i], "exit: evaluated at the worker's end");
        EXPECT(arithmetic(since(read)) == 0);
    }
    for (int which = 0; which < 2; ++which) {                // a failing stub: the results throw the queue's message
        Handed h;
        const size_t live = stub_live_count(kDevice);
        const char *entry = which ? "csgn_malloc" : "csgn_small_ops";
        std::thread worker([&] {
            queueSome(s, a, va, b, vb, 2, &h);
            if (which)
                Library::releaseDeviceCache();
            stub_fail(entry, which ? 0 : 1, 1000, CSGN_ERR_HIP);            // (the thread's end comes after this)
        });
        worker.join();
        stub_fail_clear();
        for (size_t i = 0; i < h.got.size(); ++i) {
            std::string what;
            try {
                (void)h.got[i].getValues();
            } catch (const std::runtime_error &e) {
                what = e.what();
            }
            EXPECT(what.find("a deferred operation failed when its thread ended") != std::string::npos);
            EXPECT(what.find(entry) != std::string::npos);
            EXPECT(throws<std::runtime_error>([&] { (void)s.sk.decrypt(h.got[i]); }));
            EXPECT(throws<std::runtime_error>([&] { Ciphertext more = h.got[i] * a; (void)more.getValues(); }));
        }
        h.got.clear();                                       // nothing is freed twice (the stub ends the program), and
        Library::releaseDeviceCache();                       // nothing the failed queue held stays live
        EXPECT(stub_live_count(kDevice) <= live);
        EXPECT(stub_live_count(kEvent) == 0);
    }
    {   // an operation started when the thread's queue is gone is computed at once
        Handed h;
        size_t mark = 0;
        std::thread worker([&] {
            t_late.run = [&] {
                mark = stub_log_size();
                try {
                    h.got.push_back(a * b);
                    h.got.push_back(h.got[0] + a);
                } catch (const std::exception &e) {
                    expect(false, std::string("an operation at the thread's end threw: ") + e.what());
                }
            };
            Handed mine;
            queueSome(s, a, va, b, vb, 0, &mine);            // (this thread has a queue, a cache and a device)
        });
        worker.join();
        const std::vector<Call> log = since(mark);
        EXPECT(count(log, "csgn_mul_uniform") == 1 && count(log, "csgn_add_uniform") == 1 && count(log, "csgn_small_ops") == 0);
        const std::vector<Call> blocks = only(log, "csgn_malloc");        // the cache is gone too: the sizes asked, no class sizes
        EXPECT(blocks.size() == 2 && blocks[0].bytes == s.dl * 8 && blocks[1].bytes == 2 * s.dl * 8);
        EXPECT(h.got.size() == 2);
        if (h.got.size() == 2) {
            s.check(h.got[0], vmul(va, vb, s.dl), "exit: computed at once");
            s.check(h.got[1], vadd(vmul(va, vb, s.dl), va), "exit: computed at once");
        }
    }
}

// ------------------------------------------------------------------ threads
void barrier(std::atomic<int> &arrived, int of)
{
    arrived.fetch_add(1);
    while (arrived.load() < of)
        std::this_thread::yield();
}

void threadsChain(Setup &s)
{
    // Shared between threads here, as the classes allow: a ciphertext that nobody changes any more is copied, and the COPY
    // is read (getValues() fills a mirror of the object it is called on, so each thread reads through its own copy);
    // SecretKey::decrypt and serializedSize() only read their arguments once the key's mask exists.
    const int kOps = 40, kReaders = 4;
    Val f[3 + kReaders];
    std::vector<Ciphertext> fresh;
    for (int i = 0; i < 3 + kReaders; ++i)
        fresh.push_back(s.fresh(1, &f[i]));
    std::vector<Val> want(kOps);
    Val v = f[0];
    for (int i = 0; i < kOps; ++i) {
        v = i % 8 == 7 ? vadd(v, f[1]) : vmul(v, f[i % 3], s.dl);           // five sums: at most six terms
        want[(size_t)i] = v;
    }
    std::vector<Ciphertext> chain((size_t)kOps);
    std::atomic<int> made(0);
    int bad[kReaders] = {0, 0, 0, 0};
    std::vector<std::thread> readers;
    std::thread worker([&] {
        Ciphertext x = fresh[0];
        for (int i = 0; i < kOps; ++i) {
            x = i % 8 == 7 ? x + fresh[1] : x * fresh[(size_t)(i % 3)];
            chain[(size_t)i] = x;
            made.store(i + 1, std::memory_order_release);
        }
        while (made.load() >= 0)                             // alive until the readers are through
            std::this_thread::yield();
    });
    for (int t = 0; t < kReaders; ++t)
        readers.emplace_back([&, t] {
            for (int step = 0; step < 12; ++step) {
                int have;
                while ((have = made.load(std::memory_order_acquire)) == 0)
                    std::this_thread::yield();
                const size_t i = (size_t)((step * 7 + t * 3) % have);
                Ciphertext node(chain[i]);
                Ciphertext own = node * fresh[(size_t)(3 + t)], sum = own + node;
                const Val vo = vmul(want[i], f[3 + t], s.dl), vs = vadd(vo, want[i]);
                bad[t] += node.getLen() != want[i].w.size() || memcmp(node.getValues(), want[i].w.data(), node.getLen() * 8) != 0;
                bad[t] += sum.getLen() != vs.w.size() || memcmp(sum.getValues(), vs.w.data(), vs.w.size() * 8) != 0;
                bad[t] += own.getLen() != vo.w.size() || memcmp(own.getValues(), vo.w.data(), vo.w.size() * 8) != 0;
            }
        });
    for (std::thread &t : readers)
        t.join();
    made.store(-1);
    worker.join();
    for (int t = 0; t < kReaders; ++t)
        EXPECT(bad[t] == 0);
    for (int i = 0; i < kOps; i += 13)
        s.check(chain[(size_t)i], want[(size_t)i], "threads: the worker's chain");
}

void threadsConst(Setup &s)
{
    Val va, vb, vc;
    Ciphertext a = s.fresh(1, &va), b = s.fresh(1, &vb), c = s.fresh(0, &vc);
    (void)s.sk.decrypt(a);                                   // the key's mask exists from here: decrypt only reads the key
    const Val vx = vmul(vadd(vmul(va, vb, s.dl), vc), vadd(va, vc), s.dl);
    for (int round = 0; round < 8; ++round) {
        const Ciphertext *x = nullptr;
        std::atomic<int> ready(0);
        unsigned seen_bit[4] = {9, 9, 9, 9};
        uint64_t seen_size[4] = {0, 0, 0, 0};
        std::thread worker([&] {
            x = new Ciphertext(((a * b) + c) * (a + c));     // queued in this thread's queue
            barrier(ready, 5);                               // ... which ends while the readers look
        });
        std::vector<std::thread> readers;
        for (int t = 0; t < 4; ++t)
            readers.emplace_back([&, t] {
                barrier(ready, 5);
                seen_bit[t] = s.sk.decrypt(const_cast<Ciphertext &>(*x)).getValue();
                seen_size[t] = x->serializedSize();
            });
        worker.join();
        for (std::thread &t : readers)
            t.join();
        for (int t = 0; t < 4; ++t)
            EXPECT(seen_bit[t] == (unsigned)vx.bit && seen_size[t] == 32 + vx.w.size() * 8);
        s.check(*x, vx, "threads: one const queued ciphertext");
        delete x;
    }
}

// a queue of device 1 evaluated by a thread on device 0: csgn_init(1), the work and the result block on device 1,
// csgn_init(0) again -- also when the flush throws
void threadsForeign()
{
    std::atomic<int> stage(0);
    Handed h;
    int worker_bad = 0;
    std::thread worker([&] {
        Library::useDevice(1);
        Setup s1(129, 3);
        Val va, vb;
        Ciphertext a = s1.fresh(1, &va), b = s1.fresh(1, &vb);
        queueSome(s1, a, va, b, vb, 3, &h);
        stage.store(1);
        while (stage.load() != 2)
            std::this_thread::yield();
        for (size_t i = 0; i < h.got.size(); ++i) {          // read on the device the words live on
            Ciphertext copy(h.got[i]);
            worker_bad += copy.getLen() != h.want[i].w.size() || memcmp(copy.getValues(), h.want[i].w.data(), copy.getLen() * 8) != 0;
            worker_bad += (int)s1.sk.decrypt(copy).getValue() != h.want[i].bit;
        }
        h.got.clear();
    });
    Setup s0(129, 3);
    Val vc, vd;
    Ciphertext c = s0.fresh(1, &vc), d = s0.fresh(0, &vd);
    EXPECT(Library::currentDevice() == 0);
    while (stage.load() != 1)
        std::this_thread::yield();
    for (int attempt = 0; attempt < 2; ++attempt) {          // the first flush throws
        const size_t mark = stub_log_size();
        if (attempt == 0)
            stub_fail("csgn_small_ops", 1, 1, CSGN_ERR_HIP);
        bool thrown = false;
        try {
            (void)h.got[2].serializedSize();                 // (evaluates the worker's queue; copies nothing)
        } catch (const std::runtime_error &) {
            thrown = true;
        }
        EXPECT(thrown == (attempt == 0));
        const std::vector<Call> log = since(mark);
        EXPECT(log.size() >= 4);
        if (log.size() >= 4) {
            EXPECT(log.front().name == "csgn_init" && log.front().bytes == 1 && log.front().device == 0);
            EXPECT(log.back().name == "csgn_init" && log.back().bytes == 0 && log.back().device == 1);
            for (size_t i = 1; i + 1 < log.size(); ++i)
                EXPECT(log[i].device == 1);
            EXPECT(count(log, "csgn_malloc") == 1 && count(log, "csgn_small_ops") == (attempt == 0 ? 1u : 4u));
        }
        // this thread is on device 0 again: its own work passes the stub's device check
        Ciphertext e = c * d, g = e + c, k = g * g;
        s0.check(k, vmul(vadd(vmul(vc, vd, s0.dl), vc), vadd(vmul(vc, vd, s0.dl), vc), s0.dl), "threads: on device 0 after a foreign flush");
    }
    stage.store(2);
    worker.join();
    EXPECT(worker_bad == 0);
}

void threads()
{
    Library::deferSmallOperations(true);
    Setup s(1247, 4);
    threadsChain(s);
    threadsConst(s);
    threadsForeign();
}

// ------------------------------------------------------------------ cache
size_t classOf(size_t bytes)                                 // the documented size classes (runtime.cpp, BlockCache)
{
    size_t cap = 256;
    while (cap < bytes)
        cap *= 2;
    if (cap <= MiB || bytes <= cap / 2)
        return cap;
    const size_t base = cap / 2, step = base / 4;
    return base + (bytes - base + step - 1) / step * step;
}

void cacheOff()                                              // CSGN_NO_BLOCK_CACHE=1: every payload goes straight back
{
    detail::ensureDevice();
    for (size_t bytes : {(size_t)8, (size_t)4096, MiB}) {
        const size_t mark = stub_log_size();
        std::shared_ptr<DevicePayload> p = detail::allocBytes(bytes);
        const void *ptr = p->ptr;
        p.reset();
        const std::vector<Call> frees = only(since(mark), "csgn_free");
        EXPECT(frees.size() == 1 && frees[0].p0 == ptr && !stub_is_live(ptr));
        p = detail::allocBytes(bytes);
        EXPECT(count(since(mark), "csgn_malloc") == 2);
    }
    Setup s(129, 3);
    wordsProgram(s, true, 99u);
    EXPECT(stub_live_count(kDevice) == 1);                   // the key's mask
}

std::shared_ptr<DevicePayload> g_late_payload;

void cache()
{
    detail::ensureDevice();
    // the capacity asked of csgn_malloc
    stub_thin(true);
    const size_t sizes[] = {1, 256, 257, MiB, MiB + 8, MiB + MiB / 4, MiB + MiB / 4 + 8, 2 * MiB, (size_t)176 * 1000 * 1000};
    const size_t caps[] = {256, 256, 512, MiB, MiB + MiB / 4, MiB + MiB / 4, MiB + MiB / 2, 2 * MiB, (size_t)192 * MiB};
    for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
        Library::releaseDeviceCache();
        size_t mark = stub_log_size();
        std::shared_ptr<DevicePayload> p = sizes[i] % 8 ? detail::allocBytes(sizes[i]) : detail::allocWords(sizes[i] / 8);
        std::vector<Call> m = only(since(mark), "csgn_malloc");
        EXPECT(classOf(sizes[i]) == caps[i]);
        EXPECT(m.size() == 1 && m[0].bytes == caps[i] && m[0].bytes >= sizes[i] && p->capacity == caps[i] && p->ptr == m[0].p0);
        EXPECT(p->words == sizes[i] / 8 && p->device == 0);
        // a freed block is handed out again without a csgn_malloc, to any size of its class
        const void *ptr = p->ptr;
        p.reset();
        EXPECT(stub_is_live(ptr));
        p = detail::allocBytes(caps[i]);
        EXPECT(p->ptr == ptr && count(since(mark), "csgn_malloc") == 1 && count(since(mark), "csgn_free") == 0);
        p.reset();
        p = detail::allocBytes(caps[i] + 1);                 // the next class: another block
        EXPECT(p->ptr != ptr && count(since(mark), "csgn_malloc") == 2 && p->capacity > caps[i]);
    }
    // blocks past 256 MiB go back at once, and so does what would take the cache past 4 GiB
    Library::releaseDeviceCache();
    EXPECT(stub_live_count(kDevice) == 0);
    {
        size_t mark = stub_log_size();
        std::shared_ptr<DevicePayload> edge = detail::allocBytes(256 * MiB), past = detail::allocBytes(256 * MiB + 8);
        const void *p_edge = edge->ptr, *p_past = past->ptr;
        EXPECT(past->capacity == 320 * MiB);
        past.reset();
        EXPECT(!stub_is_live(p_past) && count(since(mark), "csgn_free") == 1);
        edge.reset();
        EXPECT(stub_is_live(p_edge) && count(since(mark), "csgn_free") == 1);
        std::vector<std::shared_ptr<DevicePayload> > many;
        many.push_back(detail::allocBytes(256 * MiB));
        EXPECT(many[0]->ptr == p_edge);
        for (int i = 1; i < 17; ++i)
            many.push_back(detail::allocBytes(256 * MiB));
        mark = stub_log_size();
        for (int i = 0; i < 16; ++i)
            many[(size_t)i].reset();
        EXPECT(count(since(mark), "csgn_free") == 0);       // 16 x 256 MiB: exactly the cap
        const void *last = many[16]->ptr;
        many[16].reset();
        EXPECT(!stub_is_live(last) && count(since(mark), "csgn_free") == 1);
        Library::releaseDeviceCache();
        EXPECT(count(since(mark), "csgn_free") == 17 && stub_live_count(kDevice) == 0);
    }
    stub_thin(false);
    // out of memory: the cache is dropped and the call tried once more; a second refusal throws
    {
        std::vector<const void *> cached;
        for (size_t bytes : {(size_t)256, (size_t)1024, (size_t)4096}) {
            std::shared_ptr<DevicePayload> p = detail::allocBytes(bytes);
            cached.push_back(p->ptr);
        }
        size_t mark = stub_log_size();
        stub_fail("csgn_malloc", 0, 1, CSGN_ERR_HIP);
        std::shared_ptr<DevicePayload> p = detail::allocBytes(8192);
        std::vector<Call> log = since(mark);
        EXPECT(count(log, "csgn_malloc", CSGN_ERR_HIP) == 1 && count(log, "csgn_malloc") == 1 && count(log, "csgn_free") == 3);
        EXPECT(log.front().status == CSGN_ERR_HIP && log.back().name == "csgn_malloc" && log.back().status == CSGN_OK);
        for (const void *c : cached)
            EXPECT(!stub_is_live(c));
        detail::check(csgn_memset(p->ptr, 0, 8192, detail::stream()), "csgn_memset");
        p.reset();                                           // cached: the next refusal has something to drop
        mark = stub_log_size();
        stub_fail("csgn_malloc", 0, 2, CSGN_ERR_HIP);
        EXPECT(throws<std::runtime_error>([&] { (void)detail::allocBytes(16384); }));
        log = since(mark);
        EXPECT(count(log, "csgn_malloc", CSGN_ERR_HIP) == 2 && count(log, "csgn_free") == 1 && stub_live_count(kDevice) == 0);
        mark = stub_log_size();
        p = detail::allocBytes(8192);                        // the cache is empty and usable
        EXPECT(count(since(mark), "csgn_malloc") == 1);
        stub_fail("csgn_malloc", 0, 1, CSGN_ERR_HIP);        // nothing cached: no second try
        mark = stub_log_size();
        EXPECT(throws<std::runtime_error>([&] { (void)detail::allocBytes(16384); }));
        EXPECT(count(since(mark), "csgn_malloc", CSGN_ERR_HIP) == 1 && since(mark).size() == 1);
        stub_fail_clear();
    }
    // a payload dropped on a thread bound to another device is freed, not cached there
    {
        Library::releaseDeviceCache();
        std::shared_ptr<DevicePayload> p = detail::allocBytes(4096);
        const void *ptr = p->ptr;
        size_t mark = 0;
        std::thread other([&] {
            Library::useDevice(1);
            std::shared_ptr<DevicePayload> warm = detail::allocBytes(4096);
            mark = stub_log_size();
            p.reset();
        });
        other.join();
        EXPECT(!p && !stub_is_live(ptr));
        EXPECT(since(mark).size() >= 1 && since(mark)[0].name == "csgn_free" && since(mark)[0].p0 == ptr && since(mark)[0].device == 1);
        EXPECT(stub_live_count(kDevice) == 0);               // and the other thread's own block went with it
    }
    // a thread that moves to another device does not hand out the old device's blocks
    {
        std::thread mover([&] {
            std::shared_ptr<DevicePayload> p = detail::allocBytes(4096);
            p.reset();
            Library::useDevice(1);
            const size_t mark = stub_log_size();
            p = detail::allocBytes(4096);
            EXPECT(p->device == 1 && count(since(mark), "csgn_malloc") == 1);
            detail::check(csgn_memset(p->ptr, 0, 4096, detail::stream()), "csgn_memset");       // (the stub checks the device)
        });
        mover.join();
        EXPECT(stub_live_count(kDevice) == 0);
    }
    // a payload made while the thread's cache is gone has the size asked, no class size: freed when dropped, not cached as
    // the class it would fit in
    {
        Library::releaseDeviceCache();
        std::thread ending([&] {
            t_late.run = [&] { g_late_payload = detail::allocBytes(160); };
            (void)detail::allocBytes(160);
        });
        ending.join();
        EXPECT(g_late_payload && g_late_payload->capacity == 160 && stub_live_count(kDevice) == 1);
        const void *ptr = g_late_payload->ptr;
        const size_t mark = stub_log_size();
        g_late_payload.reset();
        EXPECT(!stub_is_live(ptr) && count(since(mark), "csgn_free") == 1);
        std::shared_ptr<DevicePayload> p = detail::allocBytes(200);
        EXPECT(count(since(mark), "csgn_malloc") == 1 && p->capacity == 256);
        detail::check(csgn_memset(p->ptr, 0, 200, detail::stream()), "csgn_memset");
    }
    // at the thread's end no block stays live: inThread() looks
    std::shared_ptr<DevicePayload> kept = detail::allocBytes(1000);
    kept.reset();
    EXPECT(stub_live_count(kDevice) >= 1);
}

// ------------------------------------------------------------------ pinned
void pinned()
{
    Library::deferSmallOperations(true);
    Setup s(1247, 4);
    const uint64_t big_terms = 6560, big = big_terms * s.dl;               // 1 049 600 bytes of words: a pinned mirror
    std::vector<uint64_t> words(big);
    Lcg next = {5u};
    for (uint64_t &w : words)
        w = ((uint64_t)next() << 40) ^ ((uint64_t)next() << 16) ^ next();
    const size_t cap = classOf(big * 8 + 64);
    EXPECT(cap == MiB + MiB / 4);
    detail::releasePinnedPool();
    const void *block = nullptr;
    {   // a mirror of 1 MiB or more comes from the pool and goes back to it
        Ciphertext c(words.data(), nullptr, big, s.ctx);
        size_t mark = stub_log_size();
        const uint64_t *v = c.getValues();
        std::vector<Call> log = since(mark);
        EXPECT(count(log, "csgn_host_alloc") == 1 && first(log, "csgn_host_alloc").bytes == cap);
        block = first(log, "csgn_host_alloc").p0;
        EXPECT((const char *)v == (const char *)block + 64 && memcmp(v, words.data(), big * 8) == 0);
        EXPECT(c.getValues() == v && since(mark).size() == log.size());    // the mirror stays
        Ciphertext small(words.data(), nullptr, s.dl, s.ctx);              // under 1 MiB: not pinned
        mark = stub_log_size();
        EXPECT(memcmp(small.getValues(), words.data(), s.dl * 8) == 0 && count(since(mark), "csgn_host_alloc") == 0);
    }
    EXPECT(stub_is_live(block));
    {
        Ciphertext c(words.data(), nullptr, big - s.dl, s.ctx);            // the same class
        const size_t mark = stub_log_size();
        const uint64_t *v = c.getValues();
        EXPECT(count(since(mark), "csgn_host_alloc") == 0 && (const char *)v == (const char *)block + 64);
        EXPECT(memcmp(v, words.data(), (big - s.dl) * 8) == 0);
        // a copy that fails leaves no mirror behind: the next call copies again, into the block the failed one gave back
        Ciphertext d(c), e(words.data(), nullptr, 2 * s.dl, s.ctx);
        for (Ciphertext *x : {&d, &e}) {
            stub_fail("csgn_memcpy_d2h", 0, 1, CSGN_ERR_HIP);
            const size_t pinned_before = stub_live_count(kPinned);
            EXPECT(throws<std::runtime_error>([&] { (void)x->getValues(); }));
            EXPECT(stub_live_count(kPinned) == pinned_before + (x == &d ? 1 : 0));
            const uint64_t *again = x->getValues();
            EXPECT(again && memcmp(again, words.data(), x->getLen() * 8) == 0);
            EXPECT(stub_live_count(kPinned) == pinned_before + (x == &d ? 1 : 0));
        }
    }
    // a refused csgn_host_alloc drops the pool and is tried once more; refused again it throws, the pool consistent
    {
        EXPECT(stub_live_count(kPinned) >= 2);
        size_t mark = stub_log_size();
        stub_fail("csgn_host_alloc", 0, 1, CSGN_ERR_HIP);
        size_t capacity = 0;
        void *p = detail::pinnedTake(3 * MiB, &capacity);
        std::vector<Call> log = since(mark);
        EXPECT(capacity == 3 * MiB && count(log, "csgn_host_alloc", CSGN_ERR_HIP) == 1 && count(log, "csgn_host_alloc") == 1);
        EXPECT(count(log, "csgn_host_free") == 2 && !stub_is_live(block));
        detail::pinnedGive(p, capacity);
        mark = stub_log_size();
        stub_fail("csgn_host_alloc", 0, 2, CSGN_ERR_HIP);
        EXPECT(throws<std::runtime_error>([&] { (void)detail::pinnedTake(5 * MiB, &capacity); }));
        log = since(mark);
        EXPECT(count(log, "csgn_host_alloc", CSGN_ERR_HIP) == 2 && count(log, "csgn_host_free") == 1);
        stub_fail_clear();
        mark = stub_log_size();
        p = detail::pinnedTake(3 * MiB, &capacity);          // the pool is empty, not holding freed blocks
        EXPECT(count(since(mark), "csgn_host_alloc") == 1 && stub_is_live(p));
        memset(p, 0, capacity);
        detail::pinnedGive(p, capacity);
        void *q = detail::pinnedTake(3 * MiB - 8, &capacity);
        EXPECT(q == p && count(since(mark), "csgn_host_alloc") == 1);
        detail::pinnedGive(q, capacity);
        detail::releasePinnedPool();
    }
    // at most 2 GiB stay cached
    {
        stub_thin(true);
        size_t capacity = 0;
        std::vector<void *> blocks;
        for (int i = 0; i < 9; ++i)
            blocks.push_back(detail::pinnedTake(256 * MiB, &capacity));
        EXPECT(capacity == 256 * MiB);
        const size_t mark = stub_log_size();
        for (int i = 0; i < 8; ++i)
            detail::pinnedGive(blocks[(size_t)i], capacity);
        EXPECT(count(since(mark), "csgn_host_free") == 0);
        detail::pinnedGive(blocks[8], capacity);
        EXPECT(count(since(mark), "csgn_host_free") == 1 && !stub_is_live(blocks[8]));
        stub_thin(false);
        detail::releasePinnedPool();
        EXPECT(count(since(mark), "csgn_host_free") == 9);
    }
}

// ------------------------------------------------------------------ staged
struct Pieces {
    std::vector<unsigned char> bytes;
    std::vector<size_t> sizes;
    size_t at = 0;
    static void take(void *ctx, const void *piece, size_t n)
    {
        Pieces *p = static_cast<Pieces *>(ctx);
        p->bytes.insert(p->bytes.end(), static_cast<const unsigned char *>(piece), static_cast<const unsigned char *>(piece) + n);
        p->sizes.push_back(n);
    }
    static void fill(void *ctx, void *piece, size_t n)
    {
        Pieces *p = static_cast<Pieces *>(ctx);
        memcpy(piece, p->bytes.data() + p->at, n);
        p->at += n;
        p->sizes.push_back(n);
    }
};

// the copies of `log` (`name`) have the documented sizes, in order, alternate between the two staging buffers, and a
// csgn_stream_sync lies between two uses of one buffer
void checkStagedLog(const std::vector<Call> &log, const char *name, size_t bytes, bool host_is_dst)
{
    std::vector<size_t> want;
    for (size_t done = 0; done < bytes; done += detail::kStageBytes)
        want.push_back(bytes - done < detail::kStageBytes ? bytes - done : detail::kStageBytes);
    std::vector<size_t> got;
    std::map<const void *, size_t> last_use;
    std::vector<const void *> bufs;
    size_t syncs = 0;
    for (const Call &c : log) {
        if (c.name == "csgn_stream_sync")
            ++syncs;
        if (c.name != name)
            continue;
        const void *host = host_is_dst ? c.p0 : c.p1;
        got.push_back(c.bytes);
        if (last_use.count(host))
            expect(syncs > last_use[host], std::string(name) + ": no csgn_stream_sync between two uses of one staging buffer");
        last_use[host] = syncs;
        if (!bufs.empty())
            EXPECT(host != bufs.back());
        bufs.push_back(host);
    }
    EXPECT(got == want && last_use.size() <= 2);
}

void staged()
{
    Library::deferSmallOperations(true);
    const size_t S = detail::kStageBytes;
    EXPECT(S == 8 * MiB);
    const size_t sizes[] = {0, 8, S - 8, S, S + 8, 2 * S, 2 * S + 8};
    Lcg next = {17u};
    for (size_t bytes : sizes) {
        Pieces src, dst;
        src.bytes.resize(bytes);
        for (size_t i = 0; i < bytes; i += 4) {
            const uint32_t r = next();
            memcpy(src.bytes.data() + i, &r, 4);
        }
        std::shared_ptr<DevicePayload> p = detail::allocBytes(bytes ? bytes : 8);
        size_t mark = stub_log_size();
        detail::uploadStaged(p->ptr, bytes, &Pieces::fill, &src);
        checkStagedLog(since(mark), "csgn_memcpy_h2d", bytes, false);
        EXPECT(src.at == bytes);
        if (bytes)
            EXPECT(since(mark).back().name == "csgn_stream_sync" && memcmp(p->ptr, src.bytes.data(), bytes) == 0);
        else
            EXPECT(since(mark).empty());
        mark = stub_log_size();
        detail::downloadStaged(p->ptr, bytes, &Pieces::take, &dst);
        checkStagedLog(since(mark), "csgn_memcpy_d2h", bytes, true);
        EXPECT(dst.bytes == src.bytes && dst.sizes == src.sizes);
    }
    // through the classes: serialize and deserialize of 8 MiB + 8 bytes of one-word terms
    Setup s(63, 2);
    const uint64_t len = (S + 8) / 8;
    std::vector<uint64_t> words(len);
    for (uint64_t &w : words)
        w = ((uint64_t)next() << 40) ^ ((uint64_t)next() << 16) ^ next();
    Ciphertext c(words.data(), nullptr, len, s.ctx);
    std::stringstream wire;
    size_t mark = stub_log_size();
    c.serialize(wire);
    checkStagedLog(since(mark), "csgn_memcpy_d2h", S + 8, true);
    EXPECT(wire.str().size() == 32 + len * 8 && c.serializedSize() == 32 + len * 8);
    EXPECT(memcmp(wire.str().data() + 32, words.data(), len * 8) == 0);
    mark = stub_log_size();
    Ciphertext back = Ciphertext::deserialize(wire);
    checkStagedLog(since(mark), "csgn_memcpy_h2d", S + 8, false);
    EXPECT(back.getLen() == len && memcmp(back.getValues(), words.data(), len * 8) == 0);
    Val f;
    Ciphertext one = s.fresh(1, &f);
    s.check(one, f, "staged");                               // (a decrypt: the result slot exists)
    back = one;                                              // (its pinned mirror goes to the pool, and the pool back)
    detail::releasePinnedPool();
    // inThread() finds both staging buffers freed when this thread has ended, and the result slot still there
}

void stagedEnd()
{
    size_t slots = 0;
    for (const Alloc &a : stub_live())
        slots += a.kind == kPinned && a.bytes == 64;
    EXPECT(slots == 1);
    size_t freed = 0;
    for (const Call &c : stub_log())
        if (c.name == "csgn_host_alloc" && c.bytes == detail::kStageBytes && c.status == CSGN_OK)
            freed += !stub_is_live(c.p0);
    EXPECT(freed == 2);
}

// the `cache` mode's child: this program again, mode cache_off, with CSGN_NO_BLOCK_CACHE=1
int cacheChild(const char *self)
{
    std::vector<std::string> env;
    for (char **e = environ; *e; ++e)
        env.push_back(*e);
    env.push_back("CSGN_NO_BLOCK_CACHE=1");
    std::vector<char *> envp;
    for (std::string &e : env)
        envp.push_back(&e[0]);
    envp.push_back(nullptr);
    char mode[] = "cache_off";
    char *argv[] = {const_cast<char *>(self), mode, nullptr};
    pid_t pid = 0;
    int status = -1;
    fflush(stdout);
    if (posix_spawn(&pid, self, nullptr, nullptr, argv, envp.data()) != 0 || waitpid(pid, &status, 0) != pid)
        return -1;
    return WIFEXITED(status) ? WEXITSTATUS(status) : -1;
}

const char *g_self = "";

} // namespace

int main(int argc, char **argv)
{
    g_self = argv[0];
    return runModes(argc, argv, 1u, "runtime_host_driver",
                    {{"words", [] { return inThread(words); }},
                     {"batch", [] { return inThread(batch); }},
                     {"ring", [] { return inThread(ring); }},
                     {"fail_flush", [] { return inThread(failFlush) + inThread(failFirstRecords) + inThread(failFirstEvent); }},
                     {"exit", [] { return inThread(exitMode); }},
                     {"threads", [] { return inThread(threads); }},
                     {"cache", [] {
                          const int child = cacheChild(g_self);          // (before this process has a second thread)
                          expect(child == 0, "the child with CSGN_NO_BLOCK_CACHE=1 ended with status " + std::to_string(child));
                          return inThread(cache);
                      }},
                     {"cache_off", [] {
                          expect(getenv("CSGN_NO_BLOCK_CACHE") != nullptr, "cache_off runs with CSGN_NO_BLOCK_CACHE set");
                          return inThread(cacheOff);
                      }},
                     {"pinned", [] { return inThread(pinned); }},
                     {"staged", [] {
                          inThread(staged);
                          stagedEnd();
                          return 0;
                      }}});
}
