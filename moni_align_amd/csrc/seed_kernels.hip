// HIP kernels (gfx950) for the seeding half of the hot path; the per-lane logic is in seed_core.h.
//
// Mapping: one LANE per (read, strand) for the LF / MEM loops and one lane per MEM for the phi walks.
// Every step is a dependent random access into a multi-GB table, so the only parallelism is across
// reads; 64 independent reads per wavefront keep 64 row fetches in flight per wave instruction
// (a wave-per-read mapping keeps one), and the per-step state is a handful of registers so every
// SIMD runs 8 waves.  Tables are laid out so that a step reads one or two adjacent 16-byte rows
// (layout.h).  Byte tables live in LDS.  Integer/indexing work only: no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seed_core.h"
#include "prefilter_core.h"
#include "packfilter_core.h"

#define MS_BLOCK 256
#ifndef MS_CHAINS
#define MS_CHAINS 2          // independent tasks interleaved per lane in ms_lf_kernel (both strands of one read)
#endif
#ifndef OCC_STAGE
#define OCC_STAGE 1          // 0 (profiles/ms_stage): occ_kernel with a store per kept occurrence
#endif

__device__ __forceinline__ void load_tables(lds_tables_t& L, const moni_tables_t* __restrict__ T, const moni_consts_t& K) {
    if (threadIdx.x < MONI_MAX_SIGMA) {
        L.rec_base[threadIdx.x] = K.rec_base[threadIdx.x];
        L.rec_cnt[threadIdx.x] = K.rec_cnt[threadIdx.x];
        L.hot_slot[threadIdx.x] = K.hot_slot[threadIdx.x];
    }
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        L.code[i] = T->code[i];
        L.compl_tab[i] = T->compl_tab[i];
        L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
        L.abs_run[i] = T->abs_run[i];
        L.abs_pos[i] = T->abs_pos[i];
    }
    __syncthreads();
}

__device__ __forceinline__ void wave_add(unsigned long long v, unsigned long long* dst) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

extern "C" __global__ void __launch_bounds__(MS_BLOCK)
pack_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk,
            uint64_t n_tasks, uint64_t* __restrict__ pat, uint8_t* __restrict__ pflag) {
    __shared__ lds_tables_t L;
    load_tables(L, T, K);
    const uint64_t task = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (task < n_tasks) pack_task(L, seq, offs, blk, task, pat, pflag);
}

// NCH independent tasks per lane (see ms_task); MINW = minimum waves per SIMD the register allocator must leave room for.
template <int NCH, int MINW>
__global__ void __launch_bounds__(MS_BLOCK, MINW)
ms_lf_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows,
             const moni_frow_t* __restrict__ frows, const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs,
             const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t n_tasks,
             uint64_t* __restrict__ ptr_out, unsigned long long* __restrict__ counters,
             const uint64_t* __restrict__ live, const uint64_t* __restrict__ n_live) {      // the live list of strand_filter_kernel and its length (null: every task)
    if (live) {
        n_tasks = *n_live;
        if ((uint64_t)blockIdx.x * MS_BLOCK * NCH >= n_tasks) return;          // the grid is the full one: blocks past the live count leave
    }
    __shared__ lds_tables_t L;
    load_tables(L, T, K);
    const uint64_t task0 = ((uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x) * NCH;
    unsigned long long n_steps = 0, n_jumps = 0;
    if (task0 < n_tasks) ms_task<NCH>(K, L, rows, frows, cr, recs, pat, offs, blk, n_tasks, task0, ptr_out, n_steps, n_jumps, live);
    wave_add(n_steps, &counters[0]);
    wave_add(n_jumps, &counters[1]);
}

// The walk of the seeding stage (moni_hip.hip: seed_all): ms_task_events in place of ms_task - the assignments of a walk as a list per task, no dense pointers.
// STAGED (NCH = 1): eight events per lane wait in LDS, [word][lane], 16 KB beside the 4 KB of tables: 20 416 B per block, eight blocks in the 160 KB of a CU.
template <int NCH, int MINW, bool STAGED>
__global__ void __launch_bounds__(MS_BLOCK, MINW)
ms_lf_events_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows,
                    const moni_frow_t* __restrict__ frows, const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs,
                    const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t n_tasks,
                    uint64_t* __restrict__ ev, uint32_t* __restrict__ ev_cnt, unsigned long long* __restrict__ counters,
                    const uint64_t* __restrict__ live, const uint64_t* __restrict__ n_live) {      // as ms_lf_kernel's
    if (live) {
        n_tasks = *n_live;
        if ((uint64_t)blockIdx.x * MS_BLOCK * NCH >= n_tasks) return;
    }
    __shared__ lds_tables_t L;
    __shared__ uint64_t ST[STAGED ? MONI_EV_STAGE_N : 1][STAGED ? MS_BLOCK : 1];      // [event of the group][lane]
    load_tables(L, T, K);
    const uint64_t task0 = ((uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x) * NCH;
    unsigned long long n_steps = 0, n_jumps = 0;
    if (task0 < n_tasks)
        ms_task_events<NCH, STAGED>(K, L, rows, frows, cr, recs, pat, offs, blk, n_tasks, task0, ev, ev_cnt, n_steps, n_jumps, live,
                                    STAGED ? &ST[0][threadIdx.x] : nullptr, MS_BLOCK);
    wave_add(n_steps, &counters[0]);
    wave_add(n_jumps, &counters[1]);
}

// ... with leaps over matched stretches (seed_core.h: ms_task_events_leap): the same lists and counters; leap[0..2] += leaps, steps leapt, comparisons
template <int MINW>
__global__ void __launch_bounds__(MS_BLOCK, MINW)
ms_lf_leap_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const moni_row_t* __restrict__ rows,
                  const moni_frow_t* __restrict__ frows, const uint32_t* __restrict__ cr, const moni_rec_t* __restrict__ recs,
                  const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t n_tasks,
                  uint64_t* __restrict__ ev, uint32_t* __restrict__ ev_cnt, unsigned long long* __restrict__ counters,
                  const uint64_t* __restrict__ live, const uint64_t* __restrict__ n_live, const ms_leap_t Z, const uint8_t* __restrict__ pflag,
                  unsigned long long* __restrict__ leap) {
    if (live) {
        n_tasks = *n_live;
        if ((uint64_t)blockIdx.x * MS_BLOCK >= n_tasks) return;
    }
    __shared__ lds_tables_t L;
    __shared__ uint64_t ST[MONI_EV_STAGE_N][MS_BLOCK];      // [event of the group][lane]
    load_tables(L, T, K);
    const uint64_t slot = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_steps = 0, n_jumps = 0, st[3] = {0, 0, 0};
    ms_task_events_leap(K, L, rows, frows, cr, recs, pat, offs, blk, n_tasks, slot, ev, ev_cnt, n_steps, n_jumps, live, &ST[0][threadIdx.x], MS_BLOCK, Z, pflag, st);
    wave_add(n_steps, &counters[0]);
    wave_add(n_jumps, &counters[1]);
    wave_add(st[0], &leap[0]);
    wave_add(st[1], &leap[1]);
    wave_add(st[2], &leap[2]);
}
// the leap tables, once per index (seed_core.h): the clean bytes, one thread per chunk of text positions; then the sampled ISA, one thread per run
__global__ void __launch_bounds__(256) leap_clean_kernel(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t n, uint64_t chunk, uint32_t sh, uint8_t* __restrict__ clean) {
    const uint64_t c0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * chunk;
    if (c0 < n) leap_clean_chunk(text, n_text, c0, c0 + chunk < n ? c0 + chunk : n, sh, clean);
}
__global__ void __launch_bounds__(256) isa_build_kernel(const moni_row_t* __restrict__ rows, uint64_t r, uint64_t n, const uint64_t* __restrict__ ssa, uint32_t sh,
                                                        uint64_t* __restrict__ isa, uint8_t* __restrict__ clean) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < r) isa_walk_run(rows, r, n, k, ssa[k], sh, isa, clean);
}

// W: 64-bit pattern code words per lane in LDS (reads of up to 32 W bases take the 2-bit comparison; longer ones in the same launch compare bytes)
template <bool EMIT, int W, class SRC>
__device__ __forceinline__ void
mem_body(const moni_consts_t& K, const uint8_t* __restrict__ text, const uint64_t* __restrict__ text2, const uint32_t* __restrict__ exc, uint32_t exc_sh, uint32_t exc_words,
           const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t n_tasks,
           const uint64_t* __restrict__ ptr, uint32_t min_len, uint32_t split_on,
           uint32_t* __restrict__ cnt_m, uint32_t* __restrict__ cnt_s,
           const uint64_t* __restrict__ read_mem_off, moni_mem_t* __restrict__ mems, uint32_t* __restrict__ aux,
           moni_u64x2* __restrict__ slots, unsigned long long* __restrict__ counters,
           const uint64_t* __restrict__ live, const uint64_t* __restrict__ n_live, const SRC& src) {
    if (live) {
        n_tasks = *n_live;
        if ((uint64_t)blockIdx.x * MS_BLOCK >= n_tasks) return;
    }
    __shared__ uint64_t PW[W][MS_BLOCK];                 // [word][lane]: a lane's words lie in its own banks whatever word it reads
    __shared__ uint32_t EX[MONI_EXC_BITS / 32];
    for (uint32_t i = threadIdx.x; i < exc_words && i < MONI_EXC_BITS / 32; i += MS_BLOCK) EX[i] = exc[i];
    __syncthreads();
    mem_fast_t F;
    F.text2 = text2; F.exc = EX; F.exc_sh = exc_sh; F.pw = &PW[0][threadIdx.x]; F.pw_stride = MS_BLOCK; F.pw_words = W;
    const uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_cmp = 0;
    if (g < n_tasks)
        mem_task<EMIT>(K, F, text, pat, offs, blk, live ? live[g] : g, ptr, min_len, split_on, cnt_m, cnt_s, read_mem_off, mems, aux, slots, n_cmp, src);
    if (!EMIT) wave_add(n_cmp, &counters[3]);
}
template <bool EMIT, int W>
__global__ void __launch_bounds__(MS_BLOCK)
mem_kernel(const moni_consts_t K, const uint8_t* __restrict__ text, const uint64_t* __restrict__ text2, const uint32_t* __restrict__ exc, uint32_t exc_sh, uint32_t exc_words,
           const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t n_tasks,
           const uint64_t* __restrict__ ptr, uint32_t min_len, uint32_t split_on,
           uint32_t* __restrict__ cnt_m, uint32_t* __restrict__ cnt_s,
           const uint64_t* __restrict__ read_mem_off, moni_mem_t* __restrict__ mems, uint32_t* __restrict__ aux,
           moni_u64x2* __restrict__ slots, unsigned long long* __restrict__ counters,
           const uint64_t* __restrict__ live, const uint64_t* __restrict__ n_live) {      // as ms_lf_kernel's (the count pass; the emit pass takes every task)
    mem_body<EMIT, W>(K, text, text2, exc, exc_sh, exc_words, pat, offs, blk, n_tasks, ptr, min_len, split_on, cnt_m, cnt_s, read_mem_off, mems, aux, slots, counters, live, n_live,
                      mem_src_dense_t());
}
// ... with the pointers rebuilt from the event lists of ms_lf_events_kernel (both passes: the emit pass walks a task with more than MONI_MEM_SLOTS MEMs again).
// MONI_MEM_EV_SKIP=0 (profiles/ms_events; never in the product build): every read offset takes a turn of the loop, as with the dense workspace
#ifndef MONI_MEM_EV_SKIP
#define MONI_MEM_EV_SKIP 1
#endif
template <bool EMIT, int W>
__global__ void __launch_bounds__(MS_BLOCK)
mem_events_kernel(const moni_consts_t K, const uint8_t* __restrict__ text, const uint64_t* __restrict__ text2, const uint32_t* __restrict__ exc, uint32_t exc_sh, uint32_t exc_words,
                  const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t n_tasks,
                  const uint64_t* __restrict__ ev, const uint32_t* __restrict__ ev_cnt, uint32_t min_len, uint32_t split_on,
                  uint32_t* __restrict__ cnt_m, uint32_t* __restrict__ cnt_s,
                  const uint64_t* __restrict__ read_mem_off, moni_mem_t* __restrict__ mems, uint32_t* __restrict__ aux,
                  moni_u64x2* __restrict__ slots, unsigned long long* __restrict__ counters,
                  const uint64_t* __restrict__ live, const uint64_t* __restrict__ n_live) {
    mem_src_events_t<MONI_MEM_EV_SKIP != 0> src;
    src.ev = ev; src.ev_cnt = ev_cnt;
    mem_body<EMIT, W>(K, text, text2, exc, exc_sh, exc_words, pat, offs, blk, n_tasks, nullptr, min_len, split_on, cnt_m, cnt_s, read_mem_off, mems, aux, slots, counters, live, n_live,
                      src);
}

// the 2-bit text and the bitmap of its blocks that hold a byte outside A / C / G / T (seed_core.h: text2_word), one thread per word; once per index
__global__ void __launch_bounds__(256) text2_build_kernel(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t n_words, uint64_t* __restrict__ text2,
                                                          uint32_t* __restrict__ exc, uint32_t exc_sh) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    bool bad;
    text2[w] = text2_word(text, n_text, w, bad);
    if (bad) { const uint64_t b = (32 * w) >> exc_sh; atomicOr(&exc[b >> 5], 1u << (b & 31u)); }
}

// The k-mer table of the strand prefilter (prefilter_core.h), one thread per 32 text positions; once per index, from the byte text
__global__ void __launch_bounds__(256) kmer_build_kernel(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t n_words, uint32_t k, uint32_t* __restrict__ tab) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w < n_words) pf_build_word(text, n_text, w, k, tab);
}
// ... and the number of k-mers it holds
__global__ void __launch_bounds__(256) kmer_popcount_kernel(const uint32_t* __restrict__ tab, uint64_t n_words, unsigned long long* __restrict__ out) {
    unsigned long long s = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * 256) s += (unsigned)__popc(tab[w]);
    wave_add(s, out);
}

// The strand prefilter, behind pack_kernel: one lane per task decides from the task's 2-bit code words whether it can hold a MEM (pf_task_keep).
// flag[task] = 1 for a task that stays (flag[n_tasks] = 0: the scan's total), and a skipped task's counts are what mem_kernel would have found:
// none.  stats[0] += skipped tasks, stats[1] += table lookups.
__global__ void __launch_bounds__(MS_BLOCK)
strand_filter_kernel(const uint64_t* __restrict__ pat, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, const uint8_t* __restrict__ pflag, uint64_t n_tasks,
                     uint32_t min_len, uint32_t k, const uint32_t* __restrict__ tab, uint64_t* __restrict__ flag, uint32_t* __restrict__ cnt_m, uint32_t* __restrict__ cnt_s,
                     unsigned long long* __restrict__ stats) {
    const uint64_t task = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_lookups = 0, skipped = 0;
    if (task < n_tasks) {
        const uint64_t read = task >> 1;
        const uint32_t m = (uint32_t)(offs[read + 1] - offs[read]);
        const uint64_t cb = ws_pat_base(blk, task) + 64u * ((ws_block_len(blk, task) + 7) / 8);      // the task's code words (pack_task)
        pf_pat_t P;
        pf_pat_init(P, pat + cb, 64u, m);
        const bool keep = pf_task_keep(P, m, min_len, k, pflag[task] != 0, tab, n_lookups);
        flag[task] = keep ? 1u : 0u;
        if (!keep) { cnt_m[task] = 0; cnt_s[task] = 0; skipped = 1; }
    } else if (task == n_tasks) flag[task] = 0;
    wave_add(skipped, &stats[0]);
    wave_add(n_lookups, &stats[1]);
}
// pack_kernel and strand_filter_kernel in one, for the filtered seeding stage (packfilter_core.h): one lane per READ packs both tasks and decides them
// on code words held in its LDS column, and writes byte words only for a task that stays.  W: code words per strand and lane (reads of up to 32 W
// bases take the arithmetic form; longer ones in the same launch take pack_task and the filter as they are).  Same outputs and statistics as the two.
template <int W>
__global__ void __launch_bounds__(MS_BLOCK)
pack_filter_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk,
                   uint64_t n_reads, uint64_t* __restrict__ pat, uint8_t* __restrict__ pflag, uint32_t min_len, uint32_t k, const uint32_t* __restrict__ tab,
                   uint64_t* __restrict__ flag, uint32_t* __restrict__ cnt_m, uint32_t* __restrict__ cnt_s, unsigned long long* __restrict__ stats) {
    __shared__ lds_tables_t L;
    __shared__ uint64_t CW[2 * W][MS_BLOCK];             // [strand * W + word][lane]
    load_tables(L, T, K);
    const uint64_t read = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long n_lookups = 0, skipped = 0;
    if (read < n_reads) {
        pk_args_t A;
        A.min_len = min_len; A.k = k; A.tab = tab; A.cw = &CW[0][threadIdx.x]; A.cw_stride = MS_BLOCK; A.cw_words = W;
        pack_filter_read(L, A, seq, offs, blk, read, pat, pflag, flag, cnt_m, cnt_s, n_lookups, skipped);
    } else if (read == n_reads) flag[2 * n_reads] = 0;
    wave_add(skipped, &stats[0]);
    wave_add(n_lookups, &stats[1]);
}
// the live list in task order: pos = the exclusive scan of flag
__global__ void __launch_bounds__(256) live_list_kernel(const uint64_t* __restrict__ flag, const uint64_t* __restrict__ pos, uint64_t n_tasks, uint64_t* __restrict__ live) {
    const uint64_t task = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (task < n_tasks && flag[task]) live[pos[task]] = task;
}

// per-read final MEM count (orig + 2 * split)
extern "C" __global__ void read_totals_kernel(const uint32_t* __restrict__ cnt_m, const uint32_t* __restrict__ cnt_s,
                                              uint64_t n_reads, uint64_t* __restrict__ tot) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_reads) tot[r] = (uint64_t)cnt_m[2 * r] + cnt_m[2 * r + 1] + 2ull * ((uint64_t)cnt_s[2 * r] + cnt_s[2 * r + 1]);
    if (r == n_reads) tot[r] = 0;
}

extern "C" __global__ void phi_batch_kernel(const moni_consts_t K, phi_tab_t P, const uint64_t* __restrict__ pos, uint64_t n,
                                            uint64_t* __restrict__ out_pos, uint64_t* __restrict__ out_lcp) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) { uint64_t a, b; phi_step(P, K, pos[t], a, b); out_pos[t] = a; out_lcp[t] = b; }
}

// The count pass.  The lists stay where the pass writes them: a seed that keeps at most tmp_cap occurrences points at its own
// tmp_cap entries of tmp, a longer one at overflow space behind the short lists.  The overflow cursor and the list of long seeds are bumped once
// per wavefront (a prefix sum over the lanes' demands), so a repeat-rich index does not put one atomic per seed on one address; the order in
// which wavefronts arrive decides where a long list lies, and nothing reads occ_off as anything but a pointer.
__global__ void __launch_bounds__(MS_BLOCK)
occ_kernel(const moni_consts_t K, occ_args_t A) {
    const uint64_t g = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    unsigned long long phi_steps = 0;
    occ_kept_t kp; kp.n = 0;
#if OCC_STAGE
    __shared__ uint64_t ST[OCC_STAGE_N][MS_BLOCK];           // [entry of the group][lane]
    if (g < A.n_mems) occ_task<false>(K, A, g, phi_steps, &kp, &ST[0][threadIdx.x], MS_BLOCK);
#else
    if (g < A.n_mems) occ_task<false>(K, A, g, phi_steps, &kp);
#endif
    wave_add(phi_steps, &A.counters[2]);
    unsigned long long want = 0, kept = 0;          // overflow entries this lane's long lists need; occurrences its seeds keep
    uint32_t n_long = 0;
#pragma unroll                                       // (both entries by constant index: kp stays in registers)
    for (uint32_t i = 0; i < 2; ++i) {
        if (i >= kp.n) break;
        kept += kp.kept[i];
        if (kp.kept[i] > A.tmp_cap) { want += kp.kept[i]; ++n_long; }
        else A.mems[kp.slot[i]].occ_off = kp.slot[i] * A.tmp_cap;
    }
    wave_add(kept, &A.small->n_occs);
    if (!__any(n_long != 0)) return;
    const int lane = threadIdx.x & 63;
    unsigned long long w_incl = want; uint32_t n_incl = n_long;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long w = __shfl_up(w_incl, o); const uint32_t n = __shfl_up(n_incl, o);
        if (lane >= o) { w_incl += w; n_incl += n; }
    }
    unsigned long long base_w = 0; uint32_t base_n = 0;
    if (lane == 63) { base_w = atomicAdd(&A.small->ovf, w_incl); base_n = atomicAdd(&A.small->n_long, n_incl); }
    base_w = __shfl(base_w, 63); base_n = __shfl(base_n, 63);
    unsigned long long at = base_w + (w_incl - want); uint32_t li = base_n + (n_incl - n_long);
#pragma unroll
    for (uint32_t i = 0; i < 2; ++i)
        if (i < kp.n && kp.kept[i] > A.tmp_cap) {
            A.mems[kp.slot[i]].occ_off = A.n_mems * A.tmp_cap + at;
            A.long_list[li++] = kp.slot[i];               // every slot is appended at most once: the list holds n_mems entries
            at += kp.kept[i];
        }
}

// the seeds the count pass listed as long, walked again into their overflow space; not launched when there is none
__global__ void __launch_bounds__(MS_BLOCK)
occ_long_kernel(const moni_consts_t K, occ_args_t A, uint32_t n_long) {
    const uint32_t t = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t < n_long) occ_long_task(K, A, A.long_list[t]);
}

// Compaction on demand (moni_seed_fetch and the host paths that read the lists as one array): occ_cnt gathered into a u64 array for the scan,
// then every list copied from where it lies to its place in slot order.  The align kernels never run these.
extern "C" __global__ void occ_cnt_gather_kernel(const moni_mem_t* __restrict__ mems, uint64_t n, uint64_t* __restrict__ cnt) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) cnt[g] = mems[g].occ_cnt;
    if (g == n) cnt[g] = 0;
}
extern "C" __global__ void occ_compact_kernel(const moni_mem_t* __restrict__ mems, uint64_t n, const uint64_t* __restrict__ off, const uint64_t* __restrict__ src,
                                              uint64_t* __restrict__ occs, moni_mem_t* __restrict__ mems_out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    moni_mem_t M = mems[g];
    const uint64_t from = M.occ_off, to = off[g];
    const uint32_t cnt = M.occ_cnt;
    M.occ_off = to; mems_out[g] = M;          // the record as a caller sees it: occ_off into the compacted array
    for (uint32_t i = 0; i < cnt; ++i) occs[to + i] = src[from + i];
}


// Matching-statistics lengths of the forward strand (src/matching_statistics.cpp:242-256, src/mems.cpp:241-258: the loop both legacy
// front ends run over ms.query's pointers): lane = read, lens[offs[read] - offs[0] + i] = l at read offset i.
__global__ void __launch_bounds__(MS_BLOCK)
ms_len_kernel(const moni_consts_t K, const moni_tables_t* __restrict__ T, const uint8_t* __restrict__ text, const uint64_t* __restrict__ pat,
              const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk, uint64_t n_reads, const uint64_t* __restrict__ ptr, uint32_t* __restrict__ lens) {
    __shared__ lds_tables_t L;
    load_tables(L, T, K);
    const uint64_t read = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (read >= n_reads) return;
    const uint64_t task = 2 * read;
    const uint64_t pb = ws_pat_base(blk, task), qb = ws_ptr_base(blk, task);
    const uint64_t off = offs[read];
    const uint32_t m = (uint32_t)(offs[read + 1] - off);
    const uint64_t n = K.n_text;
    uint64_t l = 0, prev_pos_plus_one = n + 1;
    pat_cache_t pc; pc.w = 0xFFFFFFFFu; pc.word = 0;
    text_cache_t tc; tc.w = ~0ull; tc.word = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const uint64_t pos = ptr[qb + (uint64_t)(m - 1 - i) * 64u];
        while (pos != prev_pos_plus_one && (i + l) < m && (pos + l) < n) {
            if (pat_byte(pat, pb, m, (uint32_t)(i + l), pc) != text_byte(text, pos + l, tc)) break;
            ++l;
        }
        lens[off - offs[0] + i] = (uint32_t)l;
        l = (l == 0 ? 0 : (l - 1));
        prev_pos_plus_one = pos + 1;
    }
}

// per-seed largest / smallest per-genome occurrence count of slots [g0, g1) (`-c`, genome_task)
__global__ void __launch_bounds__(MS_BLOCK) genome_kernel(const moni_consts_t K, occ_args_t A, uint64_t g0, uint64_t g1, uint32_t* __restrict__ rows, uint64_t* __restrict__ hi_lo) {
    const uint64_t g = g0 + (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (g < g1) genome_task(K, A, g, g0, rows, hi_lo);
}
