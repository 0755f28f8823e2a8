// HIP kernel (gfx950) of pseudo-matching lengths, the legacy `moni pseudo-ms` (include/ms/spumoni.hpp:356-410; src/spumoni/run_spumoni.cpp:186-193);
// the per-lane logic is in pml_core.h.  Included from moni_hip.hip after seed_kernels.hip (MS_BLOCK, load_tables, wave_add).
//
// Mapping: one LANE per read (forward strand only), as ms_lf_kernel has one per (read, strand): every step is a dependent random access into the
// fast rows, so 64 reads per wavefront keep 64 row fetches in flight.  The state is (run, off), one pattern word, three counters: 8 waves per SIMD.
// Lengths go where they belong in read order, four at a time (16 bytes) where the read covers an aligned group of four, value by value at its
// edges (pml_task); DESIGN.md 7.4 has what was measured on the store side.
#include "pml_core.h"

#define PML_MINW 8          // waves per SIMD the register allocator must leave room for (the kernel takes 56 VGPRs: DESIGN.md 7.4)

__global__ void __launch_bounds__(MS_BLOCK, PML_MINW)
pml_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows, const moni_frow_t* __restrict__ frows,
           const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs, const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs,
           const moni_u64x2* __restrict__ blk, uint64_t n_reads, uint32_t thr, uint32_t* __restrict__ lens, uint32_t* __restrict__ read_max,
           uint32_t* __restrict__ read_hits, unsigned long long* __restrict__ counters) {
    __shared__ lds_tables_t L;
    load_tables(L, T, K);
    const uint64_t read = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_steps = 0, n_jumps = 0;
    if (read < n_reads) pml_task(K, L, rows, frows, cr, recs, pat, offs, blk, read, thr, lens, read_max, read_hits, n_steps, n_jumps);
    wave_add(n_steps, &counters[0]);
    wave_add(n_jumps, &counters[1]);
}
