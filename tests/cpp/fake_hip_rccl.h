// fake_hip_rccl.h -- the switches of tests/cpp/fake_hip_rccl.cpp: the HIP runtime calls and the RCCL calls that
// csgn_amd/csrc/csgn_shard_comm.cpp makes, in process, on a CPU, for any number of "devices".  Test only: linked
// statically into tests/cpp/sharded_host_driver.cpp next to capi_stub.cpp, never preloaded, never installed.
//
// Devices, device memory and the current device are capi_stub's (capi_stub.h): hipSetDevice / hipGetDevice move the
// one current device of the calling thread, hipMalloc / hipFree go through the stub's table of live blocks.
//
// Completion is deferred, as on a GPU.  A collective call checks its buffers (pointer and count x element size lie in
// one live device block of the calling thread's current device, which is the communicator's), registers the rank's
// contribution on its stream and returns.  The data moves when the last rank of the communicator has registered the
// same collective; the ranks must then agree on its kind, count, type and root, or the program ends with status 3, as
// it does for a broadcast whose send and receive ranges overlap other than in place, and for a collective of no
// elements (the code under test promises to issue none: the slice pointer of an empty shard may be one past its block).
// Until then the stream is busy: hipEventQuery of an event recorded behind the collective says hipErrorNotReady,
// hipStreamSynchronize waits, and so does every csgn_* call on that stream (capi_stub's stream hook), which is how a
// digest queued behind a gather reads gathered data.  ncclCommAbort cancels the communicator's pending collectives,
// frees their streams, and frees the communicator: a later call with that handle fails.  A stream's collectives
// finish in the order they were queued (one communicator per stream, which is what the code under test does).
//
// What it is not: RCCL's transports, xGMI, the stream order of real kernels.
#ifndef CSGN_TESTS_FAKE_HIP_RCCL_H
#define CSGN_TESTS_FAKE_HIP_RCCL_H

#include <cstddef>
#include <cstdint>

namespace fake {

void fake_hip_device_count(int count);       // what hipGetDeviceCount says (default 1, at most 16)
// on: a collective call returns only when the collective has completed or its communicator was aborted -- the rank
// whose peer never connects, stuck INSIDE the RCCL call.  off (the default): deferred completion, above.
void fake_rccl_block_inside(bool on);
// the next collective that rank `rank` of any communicator issues sleeps `ms` inside the RCCL call first (once)
void fake_rccl_delay(int rank, int ms);

size_t fake_live_comms();
size_t fake_live_streams();
size_t fake_live_events();
// collectives completed since the program began, by kind: "allgather", "broadcast", "allreduce"
uint64_t fake_completed(const char *kind);
size_t fake_pending_ranks();                 // ranks, of all communicators, with a collective registered and not yet run
uint64_t fake_cancelled();                   // collectives an abort or a destroy cancelled, since the program began

} // namespace fake

#endif
