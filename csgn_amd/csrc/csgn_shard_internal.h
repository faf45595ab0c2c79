// csgn_shard_internal.h -- what the two translation units of libcsgn_shard.so share: the thread's error text
// (csgn_shard_last_error, kept in csgn_shard_comm.cpp) and the checks that write it.  csgn_shard_comm.cpp is plain
// C++ (partition, communicator, gathers, barrier); csgn_shard.hip holds the one kernel and its launch.
#ifndef CSGN_SHARD_INTERNAL_H
#define CSGN_SHARD_INTERNAL_H

#include "csgn_shard.h"
#include "csgn_hip.h"

#include <hip/hip_runtime_api.h>

namespace csgn_shard_detail {

// writes the calling thread's error text, returns `code`
__attribute__((visibility("hidden"), format(printf, 2, 3))) int fail(int code, const char *fmt, ...);

} // namespace csgn_shard_detail

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return csgn_shard_detail::fail(e_ == hipErrorNoDevice ? CSGN_ERR_NO_DEVICE : CSGN_ERR_HIP, \
                                           "%s: %s", #expr, hipGetErrorString(e_));          \
    } while (0)

#define REQUIRE(cond, ...)                                                  \
    do {                                                                    \
        if (!(cond))                                                        \
            return csgn_shard_detail::fail(CSGN_ERR_INVALID, __VA_ARGS__);  \
    } while (0)

#endif
