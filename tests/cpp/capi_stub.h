// capi_stub.h -- the test hooks of tests/cpp/capi_stub.cpp, the host stub of the C ABI (include/csgn_hip.h) that the
// class layer (csgn_amd/csrc/certfhe) is compiled against to run on a CPU.
//
// The stub is plain C++ and SYNCHRONOUS: every call has done its work when it returns, "device" and pinned memory are
// host allocations of exactly the bytes asked for.  It therefore cannot show ORDERING on a stream -- a record slot
// rewritten while a launch still reads it, a block recycled under a kernel in flight compute the right words here --
// and what it offers instead is the call log, from which a driver asserts that the synchronising call was made.  The
// GPU modes of tests/cpp/dropin_driver.cpp (deferred, deferred_threads, deferred_exit) stay the test of ordering.
//
// What the stub checks on every call: each pointer and extent the call reads or writes lies inside ONE live allocation
// of the right kind (device memory, or pinned memory where the C ABI takes its device alias) made on the device that is
// current on the calling thread; the host side of a copy, where it starts inside a pinned block, stays inside it.  A
// violation, or a free of a pointer that is not live, prints a line and ends the program with status 3.
#ifndef CSGN_TESTS_CAPI_STUB_H
#define CSGN_TESTS_CAPI_STUB_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "csgn_hip.h"

namespace capi_stub {

enum Kind { kDevice = 0, kPinned = 1, kEvent = 2 };

// one live allocation: `bytes` is the size asked for (the nominal one in thin mode)
struct Alloc {
    const void *ptr;
    size_t bytes;
    int kind;
    int device;
};

// one logged call, in the order the stub saw them (all threads).  p0 / p1 / bytes by entry point:
//   csgn_malloc, csgn_host_alloc   p0 = the block (null when refused), bytes = the size asked
//   csgn_free, csgn_host_free      p0 = the block
//   csgn_memcpy_*                  p0 = destination, p1 = source, bytes
//   csgn_memset                    p0 = destination, bytes
//   csgn_event_*                   p0 = the event
//   csgn_init                      bytes = the device asked for
//   csgn_small_ops                 p0 = the record array, bytes = count, n_bits, records = a copy of the records
//   csgn_mul_uniform, _add_uniform p0 = out, bytes = t1 << 32 | t2, n_bits
// `device` is the calling thread's current device when the call came (-1: none yet), `status` what it returned.
struct Call {
    std::string name;
    const void *p0, *p1;
    size_t bytes;
    uint64_t n_bits;
    int device, status;
    std::vector<csgn_small_op> records;
};

// Calls number skip+1 ... skip+times of entry point `name`, counted from now, return `status` and do no work.
void stub_fail(const char *name, int skip, int times, int status);
void stub_fail_clear();                     // no entry point fails from now on

void stub_thin(bool on);                    // on: csgn_malloc / csgn_host_alloc hand out 16 real bytes and record the size asked

uint64_t stub_calls(const char *name);      // calls of one entry point since the program began, refused ones included
std::vector<Call> stub_log();               // a copy of the log
size_t stub_log_size();
std::vector<Alloc> stub_live();             // live allocations of every kind
size_t stub_live_count(int kind);
bool stub_is_live(const void *p);

// ---- what capi_stub_shard.cpp (the entries ShardedBatch.cpp adds) and fake_hip_rccl.cpp (HIP and RCCL under the
// communicator code) share with this stub: ONE current device per thread, ONE table of live blocks, one call log.
// Called first, with its stream, by every entry that takes one; null (the default) = nothing.  The fake sets it to "wait
// until this stream is no longer busy", which gives a call behind a collective the gathered data, as stream order does.
extern void (*stub_stream_hook)(void *stream);
int stub_device();                          // the calling thread's current device (-1: none yet)
void stub_set_device(int device);
// csgn_malloc / csgn_free under another name (counted, logged, refusable under `entry`)
int stub_allocate(const char *entry, void **out, size_t bytes, int kind);
int stub_release(const char *entry, void *p, int kind);
// counts and logs a call of `entry`; the status to return at once (an injected failure), or CSGN_OK
int stub_enter(const char *entry, const void *p0, const void *p1, size_t bytes, uint64_t n_bits);
// [p, p + bytes) lies in one live block of `kind` made on the current device, or the program ends with status 3
void stub_check(const char *entry, const void *p, size_t bytes, int kind);
void stub_set_error(const std::string &text);   // what csgn_last_error() says on this thread
[[noreturn]] void stub_die(const char *entry, const char *what, const void *p, size_t bytes);

} // namespace capi_stub

#endif
