// HIP kernels (gfx950) of the depth of coverage; the per-lane code is in cov_core.h.
//
// cov_check_kernel    a lane per record: the record check (unless the records come from the sort) and the record's class; the classes' counts
//                     are summed per wavefront (a ballot and a population count) and added by one lane
// cov_add_kernel      a lane per record: the blocks of a counted record, two device-scope integer atomic adds each, their results unused;
//                     blocks and clipped records summed per wavefront as above
// cov_reduce_kernel   a wavefront per COV_W * COV_STEPS slots of the sealed array: sum / min / max per reference.  A lane flushes by atomics
//                     where the reference changes under it; at the end a wavefront that lies in one reference folds its lanes and flushes once
// cov_tail_kernel     a lane per slot of a call's window: the run-end flags (a byte each), and a zero behind them for the scan's sum
// cov_compact_kernel  a lane per slot: the first `lines` run ends, in order
// cov_len_kernel      a lane per line: its length;  cov_render_kernel: its bytes
// cov_window_kernel   a lane per window below COV_W slots, else a wavefront per window
// No LDS.  HBM is written with plain stores and vector atomics, each lane its own bytes.
#include "cov_core.h"

typedef struct {
    const uint8_t* rec; uint64_t len; const uint64_t* off; uint64_t n; uint32_t n_ref, exclude, min_mapq, trusted;
    const uint64_t* base; int32_t* slots;
    unsigned long long* ctr;          // [0] bad records, [1] the minimum of (record << 8 | reason), [2 + class] records of a class, [6] clipped, [7] blocks
} cov_args_t;

typedef struct {
    const int32_t* depth; const uint64_t* base; uint32_t n_ref; uint64_t S;
    uint64_t x0, w;                   // the call's window: slots x0 .. x0 + w
    uint8_t* flag; const uint32_t* scan;
    uint64_t* pos; uint64_t lines, carry;
    uint64_t* len; const uint64_t* off;
    const uint8_t* names; const uint32_t* name_off; uint8_t* text;
} covtext_args_t;

__device__ __forceinline__ uint32_t cov_wave_sum(uint32_t v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ void __launch_bounds__(COV_T) cov_check_kernel(const cov_args_t G) {
    const uint64_t i = (uint64_t)blockIdx.x * COV_T + threadIdx.x;
    const bool live = i < G.n;
    const uint32_t c = live ? cov_check(G.rec, G.len, G.off, i, G.n_ref, G.exclude, G.min_mapq, G.trusted != 0u) : 0u;
    const uint32_t why = c >> 8;
    if (live && why) { atomicAdd(&G.ctr[0], 1ull); atomicMin(&G.ctr[1], (unsigned long long)(i << 8 | why)); }
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t m = __ballot(live && !why && c == k);
        if (m && (threadIdx.x & (COV_W - 1u)) == 0u) atomicAdd(&G.ctr[2u + k], (unsigned long long)__popcll(m));
    }
}

__global__ void __launch_bounds__(COV_T) cov_add_kernel(const cov_args_t G) {
    const uint64_t i = (uint64_t)blockIdx.x * COV_T + threadIdx.x;
    uint32_t got = 0;
    if (i < G.n) {
        const uint8_t* r = G.rec + G.off[i];
        int32_t* slots = G.slots;
        if (cov_class(r, G.exclude, G.min_mapq) == COV_COUNTED)
            got = cov_blocks(r, G.base, [slots](uint64_t at, int v) { (void)__hip_atomic_fetch_add(slots + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
    }
    const uint64_t clipped = __ballot(got >> 31);
    const uint32_t blocks = cov_wave_sum(got & 0x7FFFFFFFu);
    if ((threadIdx.x & (COV_W - 1u)) == 0u) {
        if (clipped) atomicAdd(&G.ctr[6], (unsigned long long)__popcll(clipped));
        if (blocks) atomicAdd(&G.ctr[7], (unsigned long long)blocks);
    }
}

__device__ __forceinline__ void cov_flush(moni_cov_ref_t* refs, const cov_acc_t& a) {
    if (a.mn > a.mx) return;          // no base seen
    atomicAdd((unsigned long long*)&refs[a.ref].bases, (unsigned long long)a.sum);
    atomicMin(&refs[a.ref].min, a.mn);
    atomicMax(&refs[a.ref].max, a.mx);
}

__global__ void __launch_bounds__(COV_T) cov_reduce_kernel(const int32_t* depth, const uint64_t* base, uint32_t n_ref, uint64_t S, moni_cov_ref_t* refs) {
    const uint64_t wave = ((uint64_t)blockIdx.x * COV_T + threadIdx.x) / COV_W;
    const uint32_t lane = threadIdx.x & (COV_W - 1u);
    const uint64_t w0 = wave * (COV_W * COV_STEPS);
    if (w0 >= S) return;          // the whole wavefront
    cov_acc_t a;
    cov_reduce(depth, base, n_ref, S, w0 + lane, a, [refs](const cov_acc_t& f) { cov_flush(refs, f); });
    const uint32_t first = __shfl(a.ref, 0, 64);
    if (__all(a.ref == first)) {
        for (int d = 32; d; d >>= 1) {
            a.sum += __shfl_xor((unsigned long long)a.sum, d, 64);
            a.mn = min(a.mn, (uint32_t)__shfl_xor(a.mn, d, 64));
            a.mx = max(a.mx, (uint32_t)__shfl_xor(a.mx, d, 64));
        }
        if (lane == 0u) cov_flush(refs, a);
    } else cov_flush(refs, a);
}

// the reference of slot x, from the one that owns the first slot of the lane's wavefront: the same loads for all its lanes, then a loop that
// runs only across a boundary
__device__ __forceinline__ uint32_t cov_lane_ref(const covtext_args_t& T, uint64_t i) {
    const uint64_t first = T.x0 + (i & ~(uint64_t)(COV_W - 1u));
    return cov_ref_from(T.base, cov_ref_of(T.base, T.n_ref, first), T.x0 + i);
}

__global__ void __launch_bounds__(COV_T) cov_tail_kernel(const covtext_args_t T) {
    const uint64_t i = (uint64_t)blockIdx.x * COV_T + threadIdx.x;
    if (i > T.w) return;
    T.flag[i] = i < T.w ? (uint8_t)cov_tail(T.depth, T.base, cov_lane_ref(T, i), T.x0 + i) : (uint8_t)0;
}

__global__ void __launch_bounds__(COV_T) cov_compact_kernel(const covtext_args_t T) {
    const uint64_t i = (uint64_t)blockIdx.x * COV_T + threadIdx.x;
    if (i >= T.w || !T.flag[i]) return;
    const uint64_t k = T.scan[i];
    if (k < T.lines) T.pos[k] = T.x0 + i;
}

__global__ void __launch_bounds__(COV_T) cov_len_kernel(const covtext_args_t T) {
    const uint64_t k = (uint64_t)blockIdx.x * COV_T + threadIdx.x;
    if (k > T.lines) return;
    T.len[k] = k < T.lines ? cov_line_len(cov_line(T.depth, T.base, T.n_ref, T.pos, k, T.carry), T.name_off) : 0u;          // entry `lines`: the scan's sum
}

__global__ void __launch_bounds__(COV_T) cov_render_kernel(const covtext_args_t T) {
    const uint64_t k = (uint64_t)blockIdx.x * COV_T + threadIdx.x;
    if (k >= T.lines) return;
    cov_put_line(T.text + T.off[k], cov_line(T.depth, T.base, T.n_ref, T.pos, k, T.carry), T.names, T.name_off);
}

// depth: the slots of one reference, ln bases; per_lane: a window per lane (window < COV_W), else a window per wavefront
__global__ void __launch_bounds__(COV_T) cov_window_kernel(const int32_t* depth, uint64_t ln, uint32_t window, uint64_t n_win, uint32_t per_lane, uint64_t* sums) {
    const uint64_t t = (uint64_t)blockIdx.x * COV_T + threadIdx.x;
    const uint64_t k = per_lane ? t : t / COV_W;
    if (k >= n_win) return;          // a window per wavefront: the whole wavefront
    const uint64_t lo = k * window, hi = lo + window < ln ? lo + window : ln;
    if (per_lane) { sums[k] = cov_window(depth, lo, hi, 0u, 1u); return; }
    unsigned long long s = cov_window(depth, lo, hi, threadIdx.x & (COV_W - 1u), COV_W);
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & (COV_W - 1u)) == 0u) sums[k] = s;
}
