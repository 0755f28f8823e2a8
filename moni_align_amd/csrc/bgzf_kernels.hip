// HIP kernel (gfx950) of the BGZF writer; the per-block code is in bgzf_core.h.
//
// Mapping: one workgroup of 256 lanes per BGZF block, grid-strided over the blocks.  The text is read through L2 (a block's 64 KB are read a
// handful of times, by one CU); LDS holds the 32 KB hash table, the current stretch, the histograms and the code tables: 40 KB, so
// four workgroups (sixteen waves, what 107 VGPRs allow) share a CU.  The tokens of a block go to the workgroup's own region in HBM, the bit stream to the block's zeroed
// staging slot (atomic ORs of whole words); gather_lines_kernel then packs the slots (pos = exclusive scan of the blocks' sizes).
#include "bgzf_core.h"

__global__ void __launch_bounds__(BGZF_T) bgzf_block_kernel(const bgzf_args_t G) {
    __shared__ bgzf_shared_t S;
    uint32_t* tok = G.tok + (uint64_t)blockIdx.x * BGZF_MAX_BLOCK;
    for (uint64_t b = blockIdx.x; b < G.n_blocks; b += gridDim.x) bgzf_block(S, G, b, tok);
}
