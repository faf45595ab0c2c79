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
// What this costs now that csgn_gather_plan, a default path of the classes, comes through here; all three accepted:
//   - the blocks are freed by a thread_local destructor, at thread or process exit; at process exit the HIP runtime
//     may already be gone, hipFree then returns an error that is ignored and the memory goes back with the process;
//   - a block is keyed by the stream's handle: a stream destroyed and created again under the same handle inherits the
//     block, which is harmless, since work on the old stream ended with it and re-use is ordered by the new one;
//   - a thread that uses a ninth stream evicts its oldest block with hipFree, a device-wide wait inside an otherwise
//     asynchronous call, as is the hipFree of a block that has to grow.
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
};
struct ScratchList {
    std::vector<ScratchBlock> v[SCRATCH_SLOTS];
    ~ScratchList()
    {
        for (std::vector<ScratchBlock> &l : v)
            for (ScratchBlock &b : l)
                (void)hipFree(b.p);
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
    if (i < v.size() && v[i].bytes >= bytes)
        return static_cast<u64 *>(v[i].p);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        e = hipErrorStreamCaptureUnsupported;
        return nullptr;
    }
    void *p = nullptr;
    if ((e = hipMalloc(&p, bytes)) != hipSuccess)
        return nullptr;
    if (bytes > kScratchKeep) {
        owned = true;
        return static_cast<u64 *>(p);
    }
    if (i < v.size()) {                                   // grown: hipFree waits for the work that reads the old block
        (void)hipFree(v[i].p);
        v[i].p = p;
        v[i].bytes = bytes;
    } else {
        if (v.size() >= kScratchStreams) {
            (void)hipFree(v.front().p);
            v.erase(v.begin());
        }
        v.push_back(ScratchBlock{s, p, bytes});
    }
    return static_cast<u64 *>(p);
}

hipError_t scratch_done(u64 *block, bool owned, hipError_t e)
{
    if (owned) {                                          // past what the thread keeps: released once the device drains
        const hipError_t f = hipFree(block);
        if (e == hipSuccess)
            e = f;
    }
    return e;
}

} // namespace csgn
