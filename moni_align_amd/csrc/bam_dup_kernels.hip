// HIP kernels (gfx950) of duplicate marking; the per-record and per-entry code is in bam_dup_core.h.
//
// bam_dupsig_kernel     a wavefront per record, four to a workgroup, grid-strided: the SEQ and CLIP checks, the score, the end code
// bam_dupinv_kernel     a lane per place: where[perm[i]] = i, the inverse of the sort's permutation
// bam_dupunit_kernel    a lane per unit, twice: the MATE checks and the number of entries (the scan of these places them), then the entries
// bam_dupprep_kernel    a lane per entry of all runs: the idx check, the records' places among all marks, the first keys of both sorts
// bam_dupkey_kernel     a lane per sorted element: the key of the next, more significant pass
// bam_duppair_kernel / bam_dupend_kernel   a lane per sorted element: a duplicate stores 1 over its records' marks
// bam_setdup_kernel     a lane per record: flag |= 0x400 where the record's mark is set
// No LDS.  The atomics are the two of a bad record and the counters of the statistics, one add per wavefront; the marks take plain byte
// stores of 1, and no two kernels that write them differ in what they write.
#include "bam_dup_core.h"

typedef struct {
    const uint8_t* rec; uint64_t len; const uint64_t* off; uint64_t n; uint32_t n_ref, paired;
    bam_dupsig_t* sig; const uint32_t* perm; uint32_t* where;
    uint64_t n_units; uint64_t* cnt; const uint64_t* pos; moni_bam_dup_t* ent;
    unsigned long long* ctr;          // [0] bad records, [1] the minimum of (record << 8 | reason) over them
} bamdup_args_t;

typedef struct {
    const moni_bam_dup_t* ent; uint64_t n_ent; const uint64_t* ent_base; const uint64_t* rec_base; uint64_t n_runs;
    uint32_t* at; uint64_t* pkey; uint64_t* ekey; uint32_t* pidx; uint32_t* eidx;
    const uint32_t* perm; uint64_t* key; uint32_t pass;          // the sorted elements and the key they take next
    uint8_t* marks;
    unsigned long long* ctr;          // [0] bad entries, [1] the first, [2] pairs, [3] duplicate pairs, [4] fragments, [5] duplicate fragments
} bamres_args_t;

__device__ __forceinline__ void bamdup_count(unsigned long long* ctr, bool yes) {
    const uint64_t m = __ballot(yes);
    if (m && (threadIdx.x & (BAM_W - 1u)) == (uint32_t)__builtin_ctzll(m)) atomicAdd(ctr, (unsigned long long)__builtin_popcountll(m));
}

__global__ void __launch_bounds__(BAMSORT_T) bam_dupsig_kernel(const bamdup_args_t G) {
    for (uint64_t i = bam_wave_id(); i < G.n; i += bam_n_waves()) {
        const uint64_t a = G.off[i];
        bam_dupsig_t s;
        const uint32_t why = bam_dupsig(G.rec + a, G.off[i + 1u] - a, G.n_ref, s);
        BAM_ONE() {
            G.sig[i] = s;
            if (why) { atomicAdd(&G.ctr[0], 1ull); atomicMin(&G.ctr[1], (unsigned long long)(i << 8 | why)); }
        }
    }
}

__global__ void __launch_bounds__(BAMSORT_T) bam_dupinv_kernel(const bamdup_args_t G) {
    const uint64_t i = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    if (i < G.n) G.where[G.perm[i]] = (uint32_t)i;
}

template <bool WRITE>
__global__ void __launch_bounds__(BAMSORT_T) bam_dupunit_kernel(const bamdup_args_t G) {
    const uint64_t u = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    if (u > G.n_units) return;
    if (u == G.n_units) { if (!WRITE) G.cnt[u] = 0; return; }          // entry n_units: the scan's sum
    moni_bam_dup_t d0, d1;
    uint32_t has0 = 0, has1 = 0; uint64_t bad = 0;
    const uint32_t why = bam_dupunit(G.rec, G.off, G.sig, G.where, G.n, u, G.paired, has0, d0, has1, d1, bad);
    if (WRITE) {
        if (has0) G.ent[G.pos[u]] = d0;
        if (has1) G.ent[G.pos[u] + has0] = d1;
    } else {
        G.cnt[u] = has0 + has1;
        if (why) { atomicAdd(&G.ctr[0], 1ull); atomicMin(&G.ctr[1], (unsigned long long)(bad << 8 | why)); }
    }
}

__global__ void __launch_bounds__(BAMSORT_T) bam_dupprep_kernel(const bamres_args_t R) {
    const uint64_t j = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    const bool in = j < R.n_ent;
    bool ok = true; uint32_t kind = 0;
    if (in) {
        ok = bam_dupprep(R.ent, R.ent_base, R.rec_base, R.n_runs, j, R.at, R.pkey, R.ekey);
        R.pidx[j] = (uint32_t)j; R.eidx[2u * j] = (uint32_t)(2u * j); R.eidx[2u * j + 1u] = (uint32_t)(2u * j + 1u);
        kind = R.ent[j].kind;
        if (!ok) { atomicAdd(&R.ctr[0], 1ull); atomicMin(&R.ctr[1], (unsigned long long)j); }
    }
    bamdup_count(&R.ctr[2], in && kind != 0);
    bamdup_count(&R.ctr[4], in && kind == 0);
}

// pass 1: k2 of the pairs' order; 2: k1 of it; 3: e of the ends' order
__global__ void __launch_bounds__(BAMSORT_T) bam_dupkey_kernel(const bamres_args_t R) {
    const uint64_t i = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    if (i >= (R.pass == 3u ? 2u * R.n_ent : R.n_ent)) return;
    const uint32_t s = R.perm[i];
    R.key[i] = R.pass == 1u ? R.ent[s].k2 : R.pass == 2u ? R.ent[s].k1 : bam_dup_end(R.ent, s);
}

__global__ void __launch_bounds__(BAMSORT_T) bam_duppair_kernel(const bamres_args_t R) {
    const uint64_t i = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    const bool dup = i < R.n_ent && bam_duppair(R.ent, R.perm, i);
    if (dup) { const uint32_t j = R.perm[i]; R.marks[R.at[2u * j]] = 1; R.marks[R.at[2u * j + 1u]] = 1; }
    bamdup_count(&R.ctr[3], dup);
}

__global__ void __launch_bounds__(BAMSORT_T) bam_dupend_kernel(const bamres_args_t R) {
    const uint64_t i = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    const bool dup = i < 2u * R.n_ent && bam_dupend(R.ent, R.perm, i);
    if (dup) R.marks[R.at[R.perm[i]]] = 1;
    bamdup_count(&R.ctr[5], dup);
}

__global__ void __launch_bounds__(BAMSORT_T) bam_setdup_kernel(uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, const uint8_t* marks) {
    const uint64_t i = (uint64_t)blockIdx.x * BAMSORT_T + threadIdx.x;
    if (i < n) bam_setdup(rec, len, off, i, marks);
}
