// fake_hip_rccl.cpp -- see fake_hip_rccl.h.  Plain C++ against the declarations of <hip/hip_runtime_api.h> and
// <rccl/rccl.h>; defines exactly the entry points csgn_amd/csrc/csgn_shard_comm.cpp calls, so a new call there fails
// the link.  One lock and one condition variable for everything: the fake is a model, not a fast one.
#include "fake_hip_rccl.h"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "capi_stub.h"

using capi_stub::kDevice;

// the two handle types the HIP header leaves incomplete
struct ihipStream_t {
    int device;
    uint64_t queued, finished;               // collectives put on this stream / completed or cancelled
};
struct ihipEvent_t {
    ihipStream_t *stream;                    // where it was last recorded (null: never)
    uint64_t ticket;                         // that stream's `queued` at the record
};

namespace {

enum Kind { kAllGather, kBroadcast, kAllReduce };
const char *const kKindName[] = {"allgather", "broadcast", "allreduce"};

struct Op {
    int kind, root, dtype;
    size_t count, esize;
    const void *send;
    void *recv;
    ihipStream_t *stream;
    bool done = false, cancelled = false;
};
typedef std::shared_ptr<Op> OpRef;

struct Group {
    int world;
    std::vector<std::deque<OpRef> > queue;   // per rank, in the order the rank issued them
};

} // namespace

struct ncclComm {
    std::shared_ptr<Group> group;
    int rank, device;
};

namespace {

std::mutex g_m;
std::condition_variable g_cv;
int g_devices = 1;
bool g_block_inside = false;
std::map<int, int> g_delay;                  // rank -> ms
std::set<ncclComm *> g_comms;
std::set<ihipStream_t *> g_streams;
std::set<ihipEvent_t *> g_events;
ihipStream_t g_default[16];                  // the legacy default stream of each device
uint64_t g_completed[3], g_cancelled;

thread_local int t_group_depth = 0;
thread_local std::vector<std::pair<ncclComm *, OpRef> > t_grouped;
thread_local hipError_t t_last_error = hipSuccess;

[[noreturn]] void die(const char *what, const Op &a, const Op *b)
{
    printf("FAKE RCCL: %s: %s count %zu type %d root %d", what, kKindName[a.kind], a.count, a.dtype, a.root);
    if (b)
        printf(" against %s count %zu type %d root %d", kKindName[b->kind], b->count, b->dtype, b->root);
    printf("\n");
    fflush(stdout);
    _Exit(3);
}

size_t size_of(ncclDataType_t t)
{
    switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
    }
}

// g_m held.  nullptr for a handle that is not a live stream (another library's, for all the fake knows)
ihipStream_t *stream_of(void *s)
{
    if (!s) {
        const int d = capi_stub::stub_device();
        return &g_default[d < 0 || d >= 16 ? 0 : d];
    }
    ihipStream_t *p = static_cast<ihipStream_t *>(s);
    return g_streams.count(p) ? p : nullptr;
}

void wait_stream(void *s)                    // capi_stub's stream hook
{
    std::unique_lock<std::mutex> lk(g_m);
    g_cv.wait(lk, [s] {
        ihipStream_t *p = stream_of(s);
        return !p || p->finished >= p->queued;
    });
}

struct Install {
    Install() { capi_stub::stub_stream_hook = wait_stream; }
} g_install;

bool overlap(const void *a, const void *b, size_t na, size_t nb)
{
    const char *x = static_cast<const char *>(a), *y = static_cast<const char *>(b);
    return x < y + nb && y < x + na;
}

// g_m held: run every collective that all ranks of `g` have now registered
void match(Group &g)
{
    for (;;) {
        for (int r = 0; r < g.world; ++r)
            if (g.queue[r].empty())
                return;
        std::vector<OpRef> op(g.world);
        for (int r = 0; r < g.world; ++r) {
            op[r] = g.queue[r].front();
            g.queue[r].pop_front();
            const Op &a = *op[0], &b = *op[r];
            if (a.kind != b.kind || a.count != b.count || a.dtype != b.dtype || a.root != b.root)
                die("the ranks disagree on a collective", a, &b);
        }
        const size_t bytes = op[0]->count * op[0]->esize;
        if (op[0]->kind == kAllGather) {
            for (int k = 0; k < g.world; ++k)
                for (int r = 0; r < g.world; ++r) {
                    char *dst = static_cast<char *>(op[k]->recv) + (size_t)r * bytes;
                    if (dst != op[r]->send)
                        memcpy(dst, op[r]->send, bytes);
                }
        } else if (op[0]->kind == kBroadcast) {
            const int root = op[0]->root;
            std::vector<char> data(static_cast<const char *>(op[root]->send), static_cast<const char *>(op[root]->send) + bytes);
            for (int k = 0; k < g.world; ++k)
                memcpy(op[k]->recv, data.data(), bytes);
        } else {
            std::vector<int32_t> sum(op[0]->count, 0);
            for (int r = 0; r < g.world; ++r)
                for (size_t i = 0; i < op[0]->count; ++i)
                    sum[i] = (int32_t)((uint32_t)sum[i] + (uint32_t)static_cast<const int32_t *>(op[r]->send)[i]);
            for (int k = 0; k < g.world; ++k)
                memcpy(op[k]->recv, sum.data(), bytes);
        }
        for (int r = 0; r < g.world; ++r) {
            op[r]->done = true;
            ++op[r]->stream->finished;
        }
        ++g_completed[op[0]->kind];
        g_cv.notify_all();
    }
}

// puts the calling rank's collectives on their streams; in block-inside mode, waits for them
ncclResult_t submit(const std::vector<std::pair<ncclComm *, OpRef> > &ops)
{
    std::unique_lock<std::mutex> lk(g_m);
    for (size_t i = 0; i < ops.size(); ++i)
        if (!g_comms.count(ops[i].first))
            return ncclInvalidArgument;                      // aborted (freed) between the call and the group's end
    for (size_t i = 0; i < ops.size(); ++i) {
        ncclComm *c = ops[i].first;
        ++ops[i].second->stream->queued;
        c->group->queue[c->rank].push_back(ops[i].second);
    }
    for (size_t i = 0; i < ops.size(); ++i)
        match(*ops[i].first->group);
    if (!g_block_inside)
        return ncclSuccess;
    // from here on the communicator may be freed under this thread's feet (ncclCommAbort): only the operations are touched
    g_cv.wait(lk, [&ops] {
        for (size_t i = 0; i < ops.size(); ++i)
            if (!ops[i].second->done && !ops[i].second->cancelled)
                return false;
        return true;
    });
    for (size_t i = 0; i < ops.size(); ++i)
        if (ops[i].second->cancelled)
            return ncclInternalError;
    return ncclSuccess;
}

ncclResult_t collective(int kind, const void *send, void *recv, size_t count, ncclDataType_t dt, int root, ncclComm_t comm,
                        hipStream_t stream, size_t send_elems, size_t recv_elems)
{
    OpRef op = std::make_shared<Op>();
    int rank = -1, world = 0, device = -1, delay = 0;
    {
        std::lock_guard<std::mutex> g(g_m);
        if (!g_comms.count(comm))
            return ncclInvalidArgument;                      // destroyed or aborted: the handle is dead
        rank = comm->rank;
        world = comm->group->world;
        device = comm->device;
        op->stream = stream_of(stream);
        std::map<int, int>::iterator d = g_delay.find(rank);
        if (d != g_delay.end()) {
            delay = d->second;
            g_delay.erase(d);
        }
    }
    if (delay)
        std::this_thread::sleep_for(std::chrono::milliseconds(delay));
    op->kind = kind;
    op->root = root;
    op->dtype = (int)dt;
    op->count = count;
    op->esize = size_of(dt);
    op->send = send;
    op->recv = recv;
    if (!op->stream || op->esize == 0 || root < 0 || root >= world || (kind == kAllReduce && dt != ncclInt32))
        return ncclInvalidArgument;
    if (count == 0)
        die("a collective of no elements", *op, nullptr);
    if (capi_stub::stub_device() != device)
        capi_stub::stub_die("RCCL collective", "issued from a thread whose current device is not the communicator's", send, 0);
    const size_t sb = send_elems * op->esize, rb = recv_elems * op->esize;
    const bool sends = kind != kBroadcast || rank == root;
    if (sends)
        capi_stub::stub_check("RCCL collective (send)", send, sb, kDevice);
    capi_stub::stub_check("RCCL collective (receive)", recv, rb, kDevice);
    const void *in_place = kind == kAllGather ? static_cast<const char *>(recv) + (size_t)rank * sb : recv;
    if (sends && send != in_place && overlap(send, recv, sb, rb))
        die("the send and the receive range overlap other than in place", *op, nullptr);
    std::pair<ncclComm *, OpRef> item(comm, op);
    if (t_group_depth > 0) {
        t_grouped.push_back(item);
        return ncclSuccess;
    }
    return submit(std::vector<std::pair<ncclComm *, OpRef> >(1, item));
}

// destroy and abort: the rank's pending collectives are cancelled and their streams freed; the handle dies
ncclResult_t retire(ncclComm_t comm)
{
    std::lock_guard<std::mutex> g(g_m);
    if (!g_comms.erase(comm))
        return ncclInvalidArgument;
    std::deque<OpRef> &q = comm->group->queue[comm->rank];
    for (size_t i = 0; i < q.size(); ++i) {
        q[i]->cancelled = true;
        ++g_cancelled;
        ++q[i]->stream->finished;
    }
    q.clear();
    delete comm;
    g_cv.notify_all();
    return ncclSuccess;
}

hipError_t hip(hipError_t e)
{
    if (e != hipSuccess)
        t_last_error = e;
    return e;
}

} // namespace

namespace fake {

void fake_hip_device_count(int count)
{
    std::lock_guard<std::mutex> g(g_m);
    g_devices = count;
}
void fake_rccl_block_inside(bool on)
{
    std::lock_guard<std::mutex> g(g_m);
    g_block_inside = on;
}
void fake_rccl_delay(int rank, int ms)
{
    std::lock_guard<std::mutex> g(g_m);
    g_delay[rank] = ms;
}
size_t fake_live_comms()
{
    std::lock_guard<std::mutex> g(g_m);
    return g_comms.size();
}
size_t fake_live_streams()
{
    std::lock_guard<std::mutex> g(g_m);
    return g_streams.size();
}
size_t fake_live_events()
{
    std::lock_guard<std::mutex> g(g_m);
    return g_events.size();
}
uint64_t fake_completed(const char *kind)
{
    std::lock_guard<std::mutex> g(g_m);
    for (int k = 0; k < 3; ++k)
        if (!strcmp(kind, kKindName[k]))
            return g_completed[k];
    return 0;
}

size_t fake_pending_ranks()
{
    std::lock_guard<std::mutex> g(g_m);
    size_t n = 0;
    for (std::set<ncclComm *>::iterator c = g_comms.begin(); c != g_comms.end(); ++c)
        n += !(*c)->group->queue[(*c)->rank].empty();
    return n;
}
uint64_t fake_cancelled()
{
    std::lock_guard<std::mutex> g(g_m);
    return g_cancelled;
}

} // namespace fake

extern "C" {

// --------------------------------------------------------------------------------------- HIP

hipError_t hipGetDeviceCount(int *count)
{
    std::lock_guard<std::mutex> g(g_m);
    *count = g_devices;
    return hip(g_devices > 0 ? hipSuccess : hipErrorNoDevice);
}

hipError_t hipSetDevice(int device)
{
    {
        std::lock_guard<std::mutex> g(g_m);
        if (device < 0 || device >= g_devices)
            return hip(hipErrorInvalidDevice);
    }
    capi_stub::stub_set_device(device);
    return hipSuccess;
}

hipError_t hipGetDevice(int *device)
{
    const int d = capi_stub::stub_device();
    *device = d < 0 ? 0 : d;                                 // a thread that never chose one is on device 0
    return hipSuccess;
}

hipError_t hipGetLastError(void)
{
    const hipError_t e = t_last_error;
    t_last_error = hipSuccess;
    return e;
}

const char *hipGetErrorString(hipError_t e)
{
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorNotReady: return "device not ready";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    case hipErrorNoDevice: return "no ROCm-capable device is detected";
    case hipErrorInvalidValue: return "invalid argument";
    default: return "invalid resource handle";
    }
}

hipError_t hipMalloc(void **ptr, size_t size)
{
    return hip(capi_stub::stub_allocate("hipMalloc", ptr, size, kDevice) == CSGN_OK ? hipSuccess : hipErrorOutOfMemory);
}

hipError_t hipFree(void *ptr)
{
    if (!ptr)
        return hipSuccess;
    return hip(capi_stub::stub_release("hipFree", ptr, kDevice) == CSGN_OK ? hipSuccess : hipErrorInvalidValue);
}

hipError_t hipMemset(void *dst, int value, size_t bytes)
{
    wait_stream(nullptr);
    if (capi_stub::stub_enter("hipMemset", dst, nullptr, bytes, 0) != CSGN_OK)
        return hip(hipErrorInvalidValue);
    capi_stub::stub_check("hipMemset", dst, bytes, kDevice);
    memset(dst, value, bytes);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int)
{
    ihipStream_t *s = new ihipStream_t();
    s->device = capi_stub::stub_device();
    std::lock_guard<std::mutex> g(g_m);
    g_streams.insert(s);
    *stream = s;
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t stream)
{
    {
        std::lock_guard<std::mutex> g(g_m);
        if (!stream_of(stream))
            return hip(hipErrorInvalidHandle);
    }
    wait_stream(stream);
    return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t stream)
{
    std::lock_guard<std::mutex> g(g_m);
    if (!stream || !g_streams.erase(stream))
        return hip(hipErrorInvalidHandle);
    delete stream;
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned)
{
    ihipEvent_t *e = new ihipEvent_t();
    std::lock_guard<std::mutex> g(g_m);
    g_events.insert(e);
    *event = e;
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t event)
{
    std::lock_guard<std::mutex> g(g_m);
    if (!event || !g_events.erase(event))
        return hip(hipErrorInvalidHandle);
    delete event;
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream)
{
    std::lock_guard<std::mutex> g(g_m);
    ihipStream_t *s = stream_of(stream);
    if (!g_events.count(event) || !s)
        return hip(hipErrorInvalidHandle);
    event->stream = s;
    event->ticket = s->queued;
    return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t event)
{
    std::lock_guard<std::mutex> g(g_m);
    if (!g_events.count(event))
        return hip(hipErrorInvalidHandle);
    if (event->stream && event->stream->finished < event->ticket)
        return hipErrorNotReady;                             // (not an error HIP remembers)
    return hipSuccess;
}

// -------------------------------------------------------------------------------------- RCCL

ncclResult_t ncclGetVersion(int *version)
{
    *version = NCCL_VERSION_CODE;
    return ncclSuccess;
}

const char *ncclGetErrorString(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "unhandled cuda error";
    case ncclSystemError: return "unhandled system error";
    case ncclInternalError: return "internal error";
    case ncclInvalidArgument: return "invalid argument";
    case ncclInvalidUsage: return "invalid usage";
    case ncclInProgress: return "operation in progress";
    default: return "unknown result code";
    }
}

ncclResult_t ncclGetUniqueId(ncclUniqueId *) { return ncclInvalidUsage; }          // the process-per-GPU form: not here
ncclResult_t ncclCommInitRank(ncclComm_t *, int, ncclUniqueId, int) { return ncclInvalidUsage; }

ncclResult_t ncclCommInitAll(ncclComm_t *comms, int ndev, const int *devlist)
{
    std::lock_guard<std::mutex> g(g_m);
    if (!comms || ndev <= 0)
        return ncclInvalidArgument;
    for (int i = 0; i < ndev; ++i) {
        const int d = devlist ? devlist[i] : i;
        if (d < 0 || d >= g_devices)
            return ncclInvalidArgument;
        for (int j = 0; j < i; ++j)
            if ((devlist ? devlist[j] : j) == d)
                return ncclInvalidUsage;                     // two ranks on one device: RCCL refuses
    }
    std::shared_ptr<Group> group = std::make_shared<Group>();
    group->world = ndev;
    group->queue.resize(ndev);
    for (int i = 0; i < ndev; ++i) {
        comms[i] = new ncclComm{group, i, devlist ? devlist[i] : i};
        g_comms.insert(comms[i]);
    }
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) { return retire(comm); }
ncclResult_t ncclCommAbort(ncclComm_t comm) { return retire(comm); }

ncclResult_t ncclCommGetAsyncError(ncclComm_t comm, ncclResult_t *async)
{
    std::lock_guard<std::mutex> g(g_m);
    if (!g_comms.count(comm) || !async)
        return ncclInvalidArgument;
    *async = ncclSuccess;
    return ncclSuccess;
}

ncclResult_t ncclAllGather(const void *send, void *recv, size_t count, ncclDataType_t dt, ncclComm_t comm, hipStream_t stream)
{
    int world = 0;
    {
        std::lock_guard<std::mutex> g(g_m);
        if (!g_comms.count(comm))
            return ncclInvalidArgument;
        world = comm->group->world;
    }
    return collective(kAllGather, send, recv, count, dt, 0, comm, stream, count, count * (size_t)world);
}

ncclResult_t ncclBroadcast(const void *send, void *recv, size_t count, ncclDataType_t dt, int root, ncclComm_t comm,
                           hipStream_t stream)
{
    return collective(kBroadcast, send, recv, count, dt, root, comm, stream, count, count);
}

ncclResult_t ncclAllReduce(const void *send, void *recv, size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm_t comm,
                           hipStream_t stream)
{
    if (op != ncclSum)
        return ncclInvalidArgument;
    return collective(kAllReduce, send, recv, count, dt, 0, comm, stream, count, count);
}

ncclResult_t ncclGroupStart()
{
    ++t_group_depth;
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd()
{
    if (t_group_depth <= 0)
        return ncclInvalidUsage;
    if (--t_group_depth > 0)
        return ncclSuccess;
    std::vector<std::pair<ncclComm *, OpRef> > ops;
    ops.swap(t_grouped);
    return ops.empty() ? ncclSuccess : submit(ops);
}

} // extern "C"
