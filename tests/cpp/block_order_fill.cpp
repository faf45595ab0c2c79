// The whole image of one launch under csgn_debug_block_order, for tests/test_capi_symbols.py: the exhaustive check of
// the XCD block orders visits sixty million (block, grid, group) triples, too many for one foreign call each.
#include <stdint.h>

#include "csgn_hip.h"

extern "C" void block_order_fill(uint32_t nblocks, uint32_t group, uint32_t *out)
{
    for (uint32_t b = 0; b < nblocks; ++b)
        out[b] = csgn_debug_block_order(b, nblocks, group);
}
