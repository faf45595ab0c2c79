// csgn_shard.hip -- the device half of libcsgn_shard.so (include/csgn_shard.h): the per-pair result term counts of a
// multiply, computed where the operands' offsets live.  The partition, the communicator and the RCCL exchange are
// plain C++ in csgn_shard_comm.cpp, which needs no device compiler; the two share csgn_shard_internal.h.
#include "csgn_shard_internal.h"

#include <hip/hip_runtime.h>

namespace {

__global__ void __launch_bounds__(256) k_product_counts(uint64_t batch, const uint64_t *__restrict__ offL,
                                                        const uint64_t *__restrict__ offR, uint64_t uniform,
                                                        uint64_t *__restrict__ counts)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b < batch)
        counts[b] = offL ? (offL[b + 1] - offL[b]) * (offR[b + 1] - offR[b]) : uniform;
}

} // namespace

extern "C" {

int csgn_shard_product_counts(uint64_t batch, const uint64_t *d_off_left, const uint64_t *d_off_right,
                              uint64_t t1, uint64_t t2, uint64_t *d_counts, void *stream)
{
    if (batch == 0)
        return CSGN_OK;
    REQUIRE(d_counts, "d_counts is null");
    REQUIRE((d_off_left == nullptr) == (d_off_right == nullptr), "pass both offset arrays or neither");
    REQUIRE(batch < (1ull << 40), "batch too large");
    const uint64_t blocks = (batch + 255) / 256;
    REQUIRE(blocks < (1ull << 24), "batch too large for one launch");
    REQUIRE(stream != CSGN_STREAM_OF_COMM, "csgn_shard_product_counts takes a real stream (no communicator here)");
    k_product_counts<<<(unsigned)blocks, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        batch, d_off_left, d_off_right, t1 * t2, d_counts);
    HIP_TRY(hipGetLastError());
    return CSGN_OK;
}

} // extern "C"
