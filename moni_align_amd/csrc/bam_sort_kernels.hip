// HIP kernels (gfx950) of the coordinate sort of BAM records; the per-record code is in bam_sort_core.h.
//
// bam_reckey_kernel   a lane per record: checks, key, the index entry's fields, the record's index as the sort's value
// bam_place_kernel    a lane per record: the size of the record that lands at place i (the scan of these gives out_off)
// bam_gather_kernel   a wavefront per record, four to a workgroup, grid-strided; the wave's index goes through readfirstlane, so a record's
//                     bounds and the phase of its copy are scalar.  One lane writes the record's index entry.
// No LDS; the only atomics are the two of a bad record.  HBM is written with plain byte and word stores, each lane its own bytes.
#include "bam_sort_core.h"

typedef struct {
    const uint8_t* rec; uint64_t len; const uint64_t* off; uint64_t n; uint32_t n_ref;
    uint64_t* key; uint32_t* idx; bam_pre_t* pre;          // in input order
    const uint32_t* perm;                                  // the sort's values: place i takes record perm[i]
    uint64_t* size; const uint64_t* out_off;               // bytes of the record at place i and their exclusive scan
    unsigned long long* ctr;                               // [0] bad records, [1] the minimum of (record << 8 | reason) over them
    uint8_t* out; moni_bam_ent_t* ents;
} bamsort_args_t;

__global__ void __launch_bounds__(BAMSORT_T) bam_reckey_kernel(const bamsort_args_t G) {
    const uint64_t i = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    if (i >= G.n) return;
    uint64_t key; bam_pre_t pre;
    const uint32_t why = bam_reckey(G.rec, G.len, G.off, i, G.n_ref, key, pre);
    G.key[i] = key; G.idx[i] = (uint32_t)i; G.pre[i] = pre;
    if (why) { atomicAdd(&G.ctr[0], 1ull); atomicMin(&G.ctr[1], (unsigned long long)(i << 8 | why)); }
}

__global__ void __launch_bounds__(BAMSORT_T) bam_place_kernel(const bamsort_args_t G) {
    const uint64_t i = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    if (i > G.n) return;
    const uint32_t r = i < G.n ? G.perm[i] : 0u;
    G.size[i] = i < G.n ? G.off[r + 1u] - G.off[r] : 0u;          // entry n: the scan's sum
}

__global__ void __launch_bounds__(BAMSORT_T) bam_gather_kernel(const bamsort_args_t G) {
    for (uint64_t i = bam_wave_id(); i < G.n; i += bam_n_waves()) {
        const uint32_t r = G.perm[i];
        const uint64_t a = G.off[r], n = G.off[r + 1u] - a, at = G.out_off[i];
        bam_gather(G.rec + a, G.out + at, n);
        BAM_ONE() {
            const bam_pre_t p = G.pre[r];
            moni_bam_ent_t e;
            e.ref_id = p.ref_id; e.pos = p.pos; e.end = p.end; e.bin_flag = p.bin_flag; e.off = at;
            G.ents[i] = e;
        }
    }
}
