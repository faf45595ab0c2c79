// scratch_stub.cpp -- csgn_amd/csrc/csgn_scratch.cpp on a CPU: the life cycle of the per-thread temporary blocks against
// stubs of the only HIP calls that file makes.  Compiled with g++ together with csgn_scratch.cpp; the HIP runtime is not
// linked.  hipMalloc hands out a small host allocation whatever size is asked; the stubs record every live pointer, count
// calls, and can be told to fail or to report a capturing stream.  A free of a pointer that is not live ends the program,
// and so does a pointer that is still live once the thread that took it has ended: every mode runs in a thread of its own.
// usage: scratch_stub reuse|grow|evict|owned|capture|pinned|exit
#include "csgn_kernels.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

namespace {

std::mutex g_lock;
std::set<void *> g_live;
std::vector<void *> g_dead;             // freed by the code under test; given back to the host at the end, so no address repeats
int g_mallocs = 0, g_frees = 0, g_queries = 0;
bool g_fail_malloc = false, g_fail_free = false;
int g_capture = 0;                      // 0: not capturing, 1: capturing, 2: the query itself fails
int g_fails = 0;

void expect(bool ok, const char *what, int line)
{
    if (!ok && g_fails++ < 20)
        printf("MISMATCH line %d: %s\n", line, what);
}
#define EXPECT(c) expect((c), #c, __LINE__)

bool live(const void *p)
{
    std::lock_guard<std::mutex> g(g_lock);
    return g_live.count(const_cast<void *>(p)) != 0;
}
size_t live_count()
{
    std::lock_guard<std::mutex> g(g_lock);
    return g_live.size();
}

} // namespace

extern "C" {

hipError_t hipMalloc(void **ptr, size_t size)
{
    std::lock_guard<std::mutex> g(g_lock);
    ++g_mallocs;
    if (g_fail_malloc || size == 0)
        return hipErrorOutOfMemory;
    *ptr = malloc(16);
    g_live.insert(*ptr);
    return hipSuccess;
}

hipError_t hipFree(void *ptr)
{
    std::lock_guard<std::mutex> g(g_lock);
    ++g_frees;
    if (!g_live.erase(ptr)) {
        printf("FREE of a pointer that is not live: %p\n", ptr);
        fflush(stdout);
        _Exit(3);
    }
    g_dead.push_back(ptr);
    return g_fail_free ? hipErrorInvalidValue : hipSuccess;
}

hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *status)
{
    std::lock_guard<std::mutex> g(g_lock);
    ++g_queries;
    if (g_capture == 2)
        return hipErrorInvalidResourceHandle;
    *status = g_capture == 1 ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}

} // extern "C"

namespace {

using namespace csgn;

constexpr size_t kKeep = (size_t)256 << 20;     // kScratchKeep

hipStream_t stream(int i) { return reinterpret_cast<hipStream_t>((uintptr_t)0x1000 + 0x40 * (uintptr_t)i); }

struct Stats {
    u64 blocks, bytes, retired, mallocs, frees;
};
Stats stats()
{
    u64 o[5];
    scratch_stats(o);
    return Stats{o[0], o[1], o[2], o[3], o[4]};
}

// one scratch_take that must succeed with a kept block
u64 *take(ScratchSlot slot, size_t bytes, int s)
{
    bool owned = true;
    hipError_t e = hipSuccess;
    u64 *p = scratch_take(slot, bytes, stream(s), owned, e);
    EXPECT(p != nullptr && e == hipSuccess && !owned);
    EXPECT(live(p));
    return p;
}

// one scratch_take that must be refused with `want`, with no hipMalloc, no hipFree and the lists as they were
void refused(ScratchSlot slot, size_t bytes, int s, hipError_t want, int mallocs)
{
    const Stats before = stats();
    const int m = g_mallocs, f = g_frees;
    const size_t n = live_count();
    bool owned = true;
    hipError_t e = hipSuccess;
    u64 *p = scratch_take(slot, bytes, stream(s), owned, e);
    const Stats after = stats();
    EXPECT(p == nullptr && e == want && !owned);
    EXPECT(g_mallocs == m + mallocs && g_frees == f && live_count() == n);
    EXPECT(after.blocks == before.blocks && after.bytes == before.bytes && after.retired == before.retired);
    EXPECT(after.mallocs == before.mallocs && after.frees == before.frees);
}

void reuse()
{
    u64 *a = take(SCRATCH_UINT_READ, 1000, 0);
    EXPECT(g_mallocs == 1);
    EXPECT(take(SCRATCH_UINT_READ, 1000, 0) == a);
    EXPECT(take(SCRATCH_UINT_READ, 8, 0) == a);
    EXPECT(g_mallocs == 1 && g_frees == 0);
    u64 *b = take(SCRATCH_UINT_PLAIN, 1000, 0);           // another slot, the same stream
    EXPECT(b != a && g_mallocs == 2);
    u64 *c = take(SCRATCH_UINT_READ, 1000, 1);            // another stream, the same slot
    EXPECT(c != a && c != b && g_mallocs == 3);
    for (int slot = 0; slot < SCRATCH_SLOTS; ++slot)      // every slot has a block of its own
        if (slot != SCRATCH_UINT_READ && slot != SCRATCH_UINT_PLAIN)
            EXPECT(live(take((ScratchSlot)slot, 64, 0)));
    EXPECT(g_mallocs == 3 + SCRATCH_SLOTS - 2 && live_count() == (size_t)g_mallocs);
    EXPECT(take(SCRATCH_UINT_READ, 1000, 0) == a && take(SCRATCH_UINT_PLAIN, 1000, 0) == b);
    EXPECT(take(SCRATCH_UINT_READ, 1000, 1) == c);
    const Stats st = stats();
    EXPECT(st.blocks == (u64)g_mallocs && st.bytes == 3000 + 64 * (SCRATCH_SLOTS - 2) && st.retired == 0);
    EXPECT(st.mallocs == (u64)g_mallocs && st.frees == 0 && g_frees == 0);
}

void grow()
{
    u64 *a = take(SCRATCH_UINT_FIND, 1000, 0);
    u64 *other = take(SCRATCH_UINT_FIND, 1000, 1);
    u64 *b = take(SCRATCH_UINT_FIND, 2000, 0);
    EXPECT(b != a && !live(a) && live(other));
    EXPECT(g_mallocs == 3 && g_frees == 1);
    EXPECT(take(SCRATCH_UINT_FIND, 500, 0) == b && take(SCRATCH_UINT_FIND, 2000, 0) == b);
    EXPECT(take(SCRATCH_UINT_FIND, 1000, 1) == other);
    EXPECT(g_mallocs == 3 && g_frees == 1);
    Stats st = stats();
    EXPECT(st.blocks == 2 && st.bytes == 3000 && st.mallocs == 3 && st.frees == 1 && st.retired == 0);
    g_fail_malloc = true;                                  // the old block stays live and usable
    refused(SCRATCH_UINT_FIND, 3000, 0, hipErrorOutOfMemory, 1);
    refused(SCRATCH_UINT_FIND, 3000, 5, hipErrorOutOfMemory, 1);
    g_fail_malloc = false;
    EXPECT(live(b) && take(SCRATCH_UINT_FIND, 2000, 0) == b);
    u64 *c = take(SCRATCH_UINT_FIND, 3000, 0);
    EXPECT(c != b && !live(b) && g_frees == 2);
    st = stats();
    EXPECT(st.blocks == 2 && st.bytes == 4000);
}

void evict()
{
    u64 *kept = take(SCRATCH_UINT_PLAIN, 100, 0);
    u64 *p[10];
    for (int i = 0; i < 8; ++i)
        p[i] = take(SCRATCH_UINT_READ, 100 + i, i);
    EXPECT(g_frees == 0 && g_mallocs == 9 && stats().blocks == 9);    // eight streams fit
    for (int i = 0; i < 8; ++i)
        EXPECT(take(SCRATCH_UINT_READ, 100 + i, i) == p[i]);
    EXPECT(take(SCRATCH_UINT_READ, 100, 0) == p[0]);      // stream 0 is now the most recently used, stream 1 the least
    EXPECT(g_frees == 0 && g_mallocs == 9);
    p[8] = take(SCRATCH_UINT_READ, 108, 8);
    EXPECT(g_frees == 1 && g_mallocs == 10);
    EXPECT(!live(p[1]));                                  // the least recently used left, not the oldest
    for (int i = 0; i < 9; ++i)
        if (i != 1)
            EXPECT(live(p[i]));
    EXPECT(live(kept));
    Stats st = stats();
    EXPECT(st.blocks == 9 && st.frees == 1 && st.retired == 0);
    EXPECT(st.bytes == 100 + (100 + 102 + 103 + 104 + 105 + 106 + 107 + 108));
    EXPECT(take(SCRATCH_UINT_READ, 100, 0) == p[0] && take(SCRATCH_UINT_PLAIN, 100, 0) == kept);
    u64 *again = take(SCRATCH_UINT_READ, 101, 1);         // stream 1 comes back: stream 2 is now the least recently used
    EXPECT(again != p[1] && g_mallocs == 11 && g_frees == 2 && !live(p[2]));
    for (int i = 3; i < 9; ++i)
        EXPECT(live(p[i]));
    EXPECT(live(p[0]) && live(kept) && stats().blocks == 9);
    // a block that grows counts as used: stream 3 grows, then two more streams push out 4 and 5
    u64 *grown = take(SCRATCH_UINT_READ, 1000, 3);
    EXPECT(!live(p[3]) && g_frees == 3);
    take(SCRATCH_UINT_READ, 100, 9);
    take(SCRATCH_UINT_READ, 100, 10);
    EXPECT(!live(p[4]) && !live(p[5]) && live(grown) && live(p[6]) && g_frees == 5);
}

void owned_mode()
{
    u64 *edge = take(SCRATCH_UINT_READ, kKeep, 0);        // exactly the kept size stays with the thread
    const Stats before = stats();
    EXPECT(before.blocks == 1 && before.bytes == kKeep);
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *big = scratch_take(SCRATCH_UINT_READ, kKeep + 8, stream(0), owned, e);
    EXPECT(big && owned && e == hipSuccess && big != edge && live(big) && live(edge));
    EXPECT(g_mallocs == 2 && g_frees == 0);
    Stats st = stats();
    EXPECT(st.blocks == 1 && st.bytes == kKeep && st.mallocs == 2 && st.frees == 0);
    EXPECT(take(SCRATCH_UINT_READ, 100, 0) == edge);
    EXPECT(scratch_done(big, true, hipSuccess) == hipSuccess);
    EXPECT(!live(big) && g_frees == 1 && stats().frees == 1);
    EXPECT(scratch_done(edge, false, hipSuccess) == hipSuccess);     // a kept block is not the call's to free
    EXPECT(scratch_done(edge, false, hipErrorLaunchFailure) == hipErrorLaunchFailure);
    EXPECT(live(edge) && g_frees == 1);
    // a failing e passes through; the free's error shows only where e was success
    big = scratch_take(SCRATCH_UINT_READ, 300u << 20, stream(0), owned, e);
    EXPECT(big && owned && e == hipSuccess);
    EXPECT(scratch_done(big, true, hipErrorLaunchFailure) == hipErrorLaunchFailure);
    EXPECT(!live(big) && g_frees == 2);
    big = scratch_take(SCRATCH_UINT_READ, 300u << 20, stream(1), owned, e);
    EXPECT(big && owned && e == hipSuccess);
    g_fail_free = true;
    EXPECT(scratch_done(big, true, hipSuccess) == hipErrorInvalidValue);
    g_fail_free = false;
    big = scratch_take(SCRATCH_UINT_READ, 300u << 20, stream(1), owned, e);
    g_fail_free = true;
    EXPECT(scratch_done(big, true, hipErrorLaunchFailure) == hipErrorLaunchFailure);
    g_fail_free = false;
    EXPECT(g_frees == 4 && live_count() == 1);
    g_fail_malloc = true;                                  // an owned request that cannot be met
    refused(SCRATCH_UINT_READ, kKeep + 8, 0, hipErrorOutOfMemory, 1);
    g_fail_malloc = false;
    st = stats();
    EXPECT(st.blocks == 1 && st.bytes == kKeep && st.retired == 0 && st.frees == 4);
}

void capture()
{
    for (int how = 1; how <= 2; ++how) {                  // capturing, and the query itself failing
        g_capture = how;
        refused(SCRATCH_UINT_READ, 1000, 0, hipErrorStreamCaptureUnsupported, 0);
        refused(SCRATCH_UINT_READ, kKeep + 8, 0, hipErrorStreamCaptureUnsupported, 0);
    }
    EXPECT(g_mallocs == 0 && g_frees == 0 && stats().blocks == 0);
    g_capture = 0;
    u64 *a = take(SCRATCH_UINT_READ, 1000, 0);
    u64 *b = take(SCRATCH_UINT_READ, 1000, 1);
    for (int how = 1; how <= 2; ++how) {
        g_capture = how;
        EXPECT(take(SCRATCH_UINT_READ, 1000, 0) == a);    // warm: the pointer
        EXPECT(take(SCRATCH_UINT_READ, 10, 0) == a);
        refused(SCRATCH_UINT_READ, 1001, 0, hipErrorStreamCaptureUnsupported, 0);   // would grow
        refused(SCRATCH_UINT_READ, 1000, 2, hipErrorStreamCaptureUnsupported, 0);   // a stream never used
        refused(SCRATCH_UINT_PLAIN, 1000, 0, hipErrorStreamCaptureUnsupported, 0);  // a slot never used
    }
    g_capture = 0;
    EXPECT(live(a) && live(b) && g_mallocs == 2 && g_frees == 0);
    EXPECT(take(SCRATCH_UINT_READ, 1000, 1) == b && take(SCRATCH_UINT_READ, 1000, 0) == a);
    const Stats st = stats();
    EXPECT(st.blocks == 2 && st.bytes == 2000 && st.retired == 0 && st.mallocs == 2 && st.frees == 0);
}

void pinned()
{
    // growth
    u64 *a = take(SCRATCH_UINT_READ, 1000, 0);
    g_capture = 1;
    EXPECT(take(SCRATCH_UINT_READ, 1000, 0) == a);
    g_capture = 0;
    u64 *b = take(SCRATCH_UINT_READ, 2000, 0);
    EXPECT(b != a && live(a) && live(b) && g_frees == 0);
    Stats st = stats();
    EXPECT(st.blocks == 1 && st.bytes == 2000 && st.retired == 1 && st.frees == 0 && st.mallocs == 2);
    u64 *c = take(SCRATCH_UINT_READ, 3000, 0);            // the block that replaced it was never captured: freed
    EXPECT(!live(b) && live(a) && live(c) && g_frees == 1 && stats().retired == 1);
    // eviction: stream 0's block of another slot is captured, then is the least recently used of nine
    u64 *d = take(SCRATCH_UINT_FIND, 100, 0);
    g_capture = 2;                                         // a query that fails marks the block too: the safe side
    EXPECT(take(SCRATCH_UINT_FIND, 100, 0) == d);
    g_capture = 0;
    u64 *q[9];
    for (int i = 1; i <= 8; ++i)
        q[i] = take(SCRATCH_UINT_FIND, 100, i);
    EXPECT(live(d) && g_frees == 1);
    st = stats();
    EXPECT(st.blocks == 9 && st.retired == 2 && st.frees == 1);
    take(SCRATCH_UINT_FIND, 100, 9);                      // the next eviction takes an unmarked block: freed
    EXPECT(!live(q[1]) && live(d) && live(a) && g_frees == 2 && stats().retired == 2);
    // the stream whose block was retired gets a new one, which is not marked
    u64 *d2 = take(SCRATCH_UINT_FIND, 100, 0);
    EXPECT(d2 != d && live(d) && !live(q[2]) && g_frees == 3);
    u64 *d3 = take(SCRATCH_UINT_FIND, 200, 0);
    EXPECT(d3 != d2 && !live(d2) && live(d) && g_frees == 4 && stats().retired == 2);
    // a refusal under capture marks nothing
    g_capture = 1;
    refused(SCRATCH_UINT_FIND, 300, 0, hipErrorStreamCaptureUnsupported, 0);
    g_capture = 0;
    u64 *d4 = take(SCRATCH_UINT_FIND, 300, 0);
    EXPECT(!live(d3) && live(d4) && g_frees == 5 && stats().retired == 2);
    // owned blocks and scratch_done leave the marked ones alone
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *big = scratch_take(SCRATCH_UINT_READ, kKeep + 8, stream(0), owned, e);
    EXPECT(big && owned && scratch_done(big, owned, e) == hipSuccess);
    EXPECT(live(a) && live(d) && g_frees == 6);
}

// what a thread leaves behind: kept blocks in several slots and streams, retired ones, and an owned one it gave back
std::vector<u64 *> g_first;
void exit_first()
{
    for (int s = 0; s < 3; ++s) {
        g_first.push_back(take(SCRATCH_UINT_READ, 1000, s));
        g_first.push_back(take(SCRATCH_MATMUL, 1000, s));
        g_first.push_back(take(SCRATCH_GATHER, 1000, s));
    }
    g_capture = 1;
    EXPECT(take(SCRATCH_UINT_READ, 1000, 0) == g_first[0]);
    EXPECT(take(SCRATCH_MATMUL, 1000, 1) == g_first[4]);
    g_capture = 0;
    g_first.push_back(take(SCRATCH_UINT_READ, 2000, 0));  // retires g_first[0]
    g_first.push_back(take(SCRATCH_MATMUL, 2000, 1));     // retires g_first[4]
    g_first.push_back(take(SCRATCH_GATHER, 2000, 2));     // frees g_first[8]
    bool owned = false;
    hipError_t e = hipSuccess;
    u64 *big = scratch_take(SCRATCH_COUNT, kKeep + 8, stream(0), owned, e);
    EXPECT(big && owned && scratch_done(big, owned, e) == hipSuccess);
    const Stats st = stats();
    EXPECT(st.blocks == 9 && st.retired == 2 && st.mallocs == 13 && st.frees == 2);
    EXPECT(live_count() == 11 && g_mallocs == 13 && g_frees == 2);
}
void exit_second()
{
    const Stats st = stats();                             // nothing of the first thread's
    EXPECT(st.blocks == 0 && st.bytes == 0 && st.retired == 0 && st.mallocs == 0 && st.frees == 0);
    const int m = g_mallocs;
    u64 *p = take(SCRATCH_UINT_READ, 1000, 0);            // the first thread's key: a block of this thread's own
    EXPECT(g_mallocs == m + 1);
    for (u64 *old : g_first)
        EXPECT(p != old);
    EXPECT(stats().blocks == 1 && stats().mallocs == 1);
}

// a mode in a thread of its own; every pointer it left must be gone once the thread has ended
void in_thread(void (*mode)())
{
    std::thread t(mode);
    t.join();
    if (live_count() != 0) {
        printf("LEAK: %zu pointers live after their thread has ended\n", live_count());
        ++g_fails;
    }
}

} // namespace

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    const struct {
        const char *name;
        void (*run)();
    } modes[] = {{"reuse", reuse}, {"grow", grow}, {"evict", evict}, {"owned", owned_mode}, {"capture", capture},
                 {"pinned", pinned}};
    bool found = false;
    for (const auto &m : modes)
        if (mode == m.name) {
            in_thread(m.run);
            found = true;
        }
    if (mode == "exit") {
        found = true;
        in_thread(exit_first);
        EXPECT(g_mallocs == 13 && g_frees == 13);         // every block exactly once: a second free ends the program
        in_thread(exit_second);
        EXPECT(g_mallocs == 14 && g_frees == 14);
    }
    if (!found) {
        fprintf(stderr, "usage: scratch_stub reuse|grow|evict|owned|capture|pinned|exit\n");
        return 2;
    }
    for (void *p : g_dead)
        free(p);
    if (g_fails) {
        printf("%d mismatches\n", g_fails);
        return 1;
    }
    printf("%s ok\n", mode.c_str());
    return 0;
}
