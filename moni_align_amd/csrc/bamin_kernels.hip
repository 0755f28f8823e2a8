// HIP kernels (gfx950) of the BAM reader; the per-segment and per-record code is in bamin_core.h.
//
// bamin_sweep_kernel    a workgroup per segment of the group, grid-strided; the segment's table is built in 64 KB of LDS and written out coalesced
// bamin_chain_kernel    one lane: the header where it has not been passed, then one hop per segment of the group
// bamin_list_kernel     a lane per segment of the group: the record starts into the segment's slots, each record checked
// bamin_compact_kernel  a workgroup per segment: the slots to their places behind the scan of the counts
// bamin_select_kernel / bamin_rank_kernel   a lane per record (and one for the scans' sums)
// bamin_summary_kernel  one lane
// bamin_fastq_kernel    a wavefront per record, four to a workgroup, grid-strided
// No workgroup waits for another: the order is the order of the launches on the context's stream.  HBM is written with plain stores; the
// atomics are the minima of a bad record and of the carry.
#include "bamin_core.h"

__global__ void __launch_bounds__(BAMIN_T) bamin_sweep_kernel(const bamin_args_t G) {
    __shared__ uint16_t tbl[BAMIN_S];
    for (uint64_t k = G.k0 + blockIdx.x; k < G.k1; k += gridDim.x) bamin_sweep(G.s, G.n, k, tbl, G.table + (k - G.k0) * BAMIN_S);
}

__global__ void __launch_bounds__(64) bamin_chain_kernel(const bamin_args_t G) {
    if (threadIdx.x || blockIdx.x) return;
    if (G.k0 == 0u && !G.st->header_done) bamin_header(G.s, G.n, G.st);
    bamin_chain(G);
}

__global__ void __launch_bounds__(BAMIN_T) bamin_list_kernel(const bamin_args_t G) {
    const uint64_t k = G.k0 + (uint64_t)blockIdx.x * BAMIN_T + threadIdx.x;
    if (k < G.k1) bamin_list(G, k);
}

__global__ void __launch_bounds__(BAMIN_T) bamin_compact_kernel(const bamin_args_t G) {
    for (uint32_t i = threadIdx.x; i < BAMIN_SLOTS; i += BAMIN_T) bamin_compact(G, blockIdx.x, i);
}

__global__ void __launch_bounds__(BAMIN_T) bamin_select_kernel(const bamin_args_t G) {
    const uint64_t r = (uint64_t)blockIdx.x * BAMIN_T + threadIdx.x;
    if (r <= G.n_rec) bamin_select(G, r);
}

__global__ void __launch_bounds__(BAMIN_T) bamin_rank_kernel(const bamin_args_t G) {
    const uint64_t r = (uint64_t)blockIdx.x * BAMIN_T + threadIdx.x;
    if (r <= G.n_rec) bamin_rank(G, r);
}

__global__ void __launch_bounds__(64) bamin_summary_kernel(const bamin_args_t G) {
    if (threadIdx.x || blockIdx.x) return;
    bamin_summary(G);
}

__global__ void __launch_bounds__(BAMIN_T) bamin_fastq_kernel(const bamin_args_t G) {
    for (uint64_t r = bam_wave_id(); r < G.n_rec; r += bam_n_waves()) bamin_fastq(G, r);
}
