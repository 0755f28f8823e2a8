// HIP kernels (gfx950) of the BAM encoder; the per-line code is in bam_core.h.
//
// Mapping: one wavefront per line (or per tile of BAM_TILE bytes in the two newline passes), four to a workgroup, grid-strided.  The wave's
// index goes through readfirstlane, so a line's bounds, its field boundaries (from ballots) and every branch on them are scalar; the lanes
// differ only where they copy or pack bytes.  No LDS.  HBM is written with plain byte and word stores, each lane its own bytes.
#include "bam_core.h"

typedef struct {
    const uint8_t* text; uint64_t len, n_tiles, n_lines;
    uint64_t* tile_cnt; const uint64_t* tile_pos;          // \n per tile and their exclusive scan
    uint64_t* starts;                                      // n_lines + 1: where every line begins, then len
    uint64_t* size; const uint64_t* off;                   // bytes of every record and their exclusive scan
    unsigned long long* ctr;                               // [0] bad lines, [1] the minimum of (line << 8 | reason) over them
    uint8_t* out;
    bam_dict_t dict;
} bam_args_t;

__device__ __forceinline__ uint64_t bam_wave_id() { return (uint64_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * BAM_T + threadIdx.x) / BAM_W)); }
__device__ __forceinline__ uint64_t bam_n_waves() { return (uint64_t)gridDim.x * (BAM_T / BAM_W); }

__global__ void __launch_bounds__(BAM_T) bam_count_kernel(const bam_args_t G) {
    for (uint64_t tile = bam_wave_id(); tile < G.n_tiles; tile += bam_n_waves()) {
        const uint64_t n = bam_tile_count(G.text, G.len, tile);
        BAM_ONE() G.tile_cnt[tile] = n;
    }
}

__global__ void __launch_bounds__(BAM_T) bam_starts_kernel(const bam_args_t G) {
    for (uint64_t tile = bam_wave_id(); tile < G.n_tiles; tile += bam_n_waves()) bam_tile_starts(G.text, G.len, tile, G.tile_pos[tile], G.starts);
}

__global__ void __launch_bounds__(BAM_T) bam_size_kernel(const bam_args_t G) {
    for (uint64_t i = bam_wave_id(); i < G.n_lines; i += bam_n_waves()) {
        uint32_t why;
        const uint64_t n = bam_line<false>(G.text, G.starts[i], G.starts[i + 1] - 1u, G.dict, nullptr, why);
        BAM_ONE() {
            G.size[i] = n;
            if (why) { atomicAdd(&G.ctr[0], 1ull); atomicMin(&G.ctr[1], (unsigned long long)(i << 8 | why)); }
        }
    }
}

__global__ void __launch_bounds__(BAM_T) bam_write_kernel(const bam_args_t G) {
    for (uint64_t i = bam_wave_id(); i < G.n_lines; i += bam_n_waves()) {
        uint32_t why;
        (void)bam_line<true>(G.text, G.starts[i], G.starts[i + 1] - 1u, G.dict, G.out + G.off[i], why);
    }
}
