// HIP kernel (gfx950) of read screening; the per-lane logic is in screen_core.h.  Included from moni_hip.hip after pml_kernels.hip
// (MS_BLOCK, load_tables, wave_add).
//
// Mapping: 2 * strands neighbouring LANES per read - P0, N0, P1, N1 - so a wavefront walks 16 reads (32 with one strand) as 64 independent chains of
// dependent row fetches, the shape pml_kernel has.  The four lanes of a read take the same steps and close their windows together; the pattern and
// the null lane trade histogram words with a cross-lane move (lane ^ 1), strand 1 hands its figures to strand 0 the same way (lane ^ 2).
// The histogram of a lane's window is a column of LDS: 16 words of two 16-bit bins, word w of lane t at hist[w * MS_BLOCK + t] - lanes that count into
// the same bin (the common case: length 0 in a null lane, the clip in a pattern lane) touch consecutive banks.  16 KB per block beside the 4 KB
// of lds_tables_t: 8 blocks of 256 lanes fit the 160 KB of a CU, which is what 8 waves per SIMD ask for.
// No length and no window score goes to HBM: one 32-byte record per read, written by the lane of P0.
#include "screen_core.h"

#define SCREEN_MINW 8          // waves per SIMD the register allocator must leave room for (DESIGN.md 7.10 has the figures)

struct screen_xchg_t {
    __device__ __forceinline__ uint32_t pair(uint32_t v) const { return (uint32_t)__shfl_xor((int)v, 1); }
    __device__ __forceinline__ uint32_t strand(uint32_t v) const { return (uint32_t)__shfl_xor((int)v, 2); }
};

__global__ void __launch_bounds__(MS_BLOCK, SCREEN_MINW)
screen_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
              const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs,
              const moni_u64x2* __restrict__ blk, uint64_t n_reads, const moni_screen_params_t P, moni_screen_res_t* __restrict__ res,
              unsigned long long* __restrict__ counters) {
    __shared__ lds_tables_t L;
    __shared__ uint32_t hist[SCREEN_WORDS * MS_BLOCK];
#pragma unroll
    for (uint32_t w = 0; w < SCREEN_WORDS; ++w) hist[w * MS_BLOCK + threadIdx.x] = 0;
    load_tables(L, T, K);
    const uint32_t sh = P.strands == 2 ? 2u : 1u;          // lanes per read = 1 << sh
    const uint64_t lane = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    const uint64_t read = lane >> sh;
    unsigned long long n_steps = 0, n_jumps = 0, jumps_p0 = 0;
    if (read < n_reads) {
        screen_xchg_t X;
        screen_task(K, L, rows, frows, cr, recs, pat, offs, blk, read, (uint32_t)lane & ((1u << sh) - 1u), P, hist + threadIdx.x, MS_BLOCK, X, res, n_steps, n_jumps, jumps_p0);
    }
    wave_add(n_steps, &counters[0]);
    wave_add(n_jumps, &counters[1]);
    wave_add(jumps_p0, &counters[2]);
}
