// csgn_scratch.cpp -- the temporaries of the composed forms and of the gather plan (csgn_kernels.h, scratch_take).
// Host code only.
//
// They do NOT come from the stream-ordered pool (hipMallocAsync).  In a process whose payloads come from hipMalloc /
// hipFree -- the classes' block cache -- the tuned launchers' writes into a pool block are not what the next launch
// on the same stream reads back: csgn_uint_plain's composed form, forced in tests/cpp/uint_plain_driver, multiplied
// ZERO words where it had just copied a plane, from its second call on, and the same launches through a hipMalloc
// block gave the right words every time.  Each host thread keeps one plain block per stream it
// has used and per user (ScratchSlot: a composed form that calls another, as csgn_uint_read's calls csgn_uint_plain,
// must not share its block with it), up to kScratchKeep bytes, grown when a call needs more; re-use is ordered by that
// stream, so a steady-state call allocates nothing and stays asynchronous.  A larger temporary is allocated for the
// call and freed behind it, which waits for the device (owned = true).  Growing or allocating under stream capture is
// refused.
//
// A block that is handed out while its stream is capturing goes into a graph, which may be replayed for as long as
// the capturing thread lives.  Such a block is marked, and a marked block is never freed before the thread ends: where
// growth or eviction would free it, it moves to the thread's retired list instead, and the stream gets a new,
// unmarked block.  The price is one hipStreamIsCapturing, a host query, on the warm path.  Where the query itself
// fails on a warm block, the block is marked, which is the safe side.
//
// What this costs now that csgn_gather_plan, a default path of the classes, comes through here; all accepted:
//   - the blocks, kept and retired, are freed by a thread_local destructor, at thread or process exit; at process exit
//     the HIP runtime may already be gone, hipFree then returns an error that is ignored and the memory goes back with
//     the process;
//   - a block is keyed by the stream's handle: a stream destroyed and created again under the same handle inherits the
//     block, which is harmless, since work on the old stream ended with it and re-use is ordered by the new one;
//   - a thread that uses a ninth stream in one slot evicts the block it used least recently (a hit moves a block to
//     the back of its list) with hipFree, a device-wide wait inside an otherwise asynchronous call, as is the hipFree
//     of a block that has to grow;
//   - a thread that keeps capturing and then outgrowing its blocks keeps every one of them until it ends.
//
// scratch_stats reports the calling thread's lists and its counts of hipMalloc and hipFree (csgn_scratch_stats).
#include "csgn_kernels.h"

#include <vector>

namespace csgn {

namespace {

constexpr size_t kScratchKeep = (size_t)256 << 20;
constexpr size_t kScratchStreams = 8;

struct ScratchBlock {
    hipStream_t s;
    void *p;
    size_t bytes;
    bool captured;                      // handed out while s was capturing: a graph may hold p
};
struct ScratchList {
    std::vector<ScratchBlock> v[SCRATCH_SLOTS];
    std::vector<void *> retired;        // marked blocks that growth or eviction replaced
    u64 mallocs = 0, frees = 0;
    void release(const ScratchBlock &b)
    {
        if (b.captured) {
            retired.push_back(b.p);
        } else {
            (void)hipFree(b.p);
            ++frees;
        }
    }
    ~ScratchList()
    {
        for (std::vector<ScratchBlock> &l : v)
            for (ScratchBlock &b : l)
                (void)hipFree(b.p);
        for (void *p : retired)
            (void)hipFree(p);
    }
};
thread_local ScratchList g_scratch;

} // namespace

u64 *scratch_take(ScratchSlot slot, size_t bytes, hipStream_t s, bool &owned, hipError_t &e)
{
    owned = false;
    std::vector<ScratchBlock> &v = g_scratch.v[slot];
    size_t i = 0;
    while (i < v.size() && v[i].s != s)
        ++i;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    if (i < v.size() && v[i].bytes >= bytes) {
        ScratchBlock b = v[i];                            // the most recently used last
        b.captured = b.captured || capturing;
        v.erase(v.begin() + i);
        v.push_back(b);
        return static_cast<u64 *>(b.p);
    }
    if (capturing) {
        e = hipErrorStreamCaptureUnsupported;
        return nullptr;
    }
    void *p = nullptr;
    if ((e = hipMalloc(&p, bytes)) != hipSuccess)
        return nullptr;
    ++g_scratch.mallocs;
    if (bytes > kScratchKeep) {
        owned = true;
        return static_cast<u64 *>(p);
    }
    if (i < v.size()) {                                   // grown: hipFree waits for the work that reads the old block
        g_scratch.release(v[i]);
        v.erase(v.begin() + i);
    } else if (v.size() >= kScratchStreams) {
        g_scratch.release(v.front());
        v.erase(v.begin());
    }
    v.push_back(ScratchBlock{s, p, bytes, false});
    return static_cast<u64 *>(p);
}

hipError_t scratch_done(u64 *block, bool owned, hipError_t e)
{
    if (owned) {                                          // past what the thread keeps: released once the device drains
        const hipError_t f = hipFree(block);
        ++g_scratch.frees;
        if (e == hipSuccess)
            e = f;
    }
    return e;
}

void scratch_stats(u64 out[5])
{
    out[0] = out[1] = 0;
    for (const std::vector<ScratchBlock> &l : g_scratch.v)
        for (const ScratchBlock &b : l) {
            ++out[0];
            out[1] += b.bytes;
        }
    out[2] = g_scratch.retired.size();
    out[3] = g_scratch.mallocs;
    out[4] = g_scratch.frees;
}

} // namespace csgn
