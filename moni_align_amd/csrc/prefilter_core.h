// The strand prefilter of the seeding stage, written once and compiled twice like seed_core.h: as __device__ code inside seed_kernels.hip
// and as plain host C++ by tests/host_sim/prefilter_sim.cpp.
//
// A MEM of at least min_len bases is a substring of the strand-resolved pattern that occurs verbatim in the text, so every k-mer of it
// (k <= min_len) occurs in the text.  The index keeps one bit per possible k-mer (4^k bits) that says whether the text holds it; a task none
// of whose windows of min_len bases has all of its min_len - k + 1 k-mers in the table can have no MEM, and the LF walk and the text
// comparison of that task are left out (seed_kernels.hip: strand_filter_kernel).  The index holds forward haplotypes only, so of the two
// tasks of a sequenced read one is almost always such a task.
//
// k-mer value: base j of the k-mer in bits 2 j .., with the codes of the 2-bit pattern words (seed_core.h: base2) - the k-mer at pattern
// offset q is 2 k bits cut out of the task's code words.  Only upper-case A / C / G / T have a code: a text k-mer that holds another byte is
// not in the table, and a pattern that holds one is never tested (its pflag is set: pack_task).
#pragma once
#include <stdint.h>

#ifndef MONI_HD
#if defined(__HIPCC__)
#define MONI_HD __host__ __device__ __forceinline__
#else
#define MONI_HD inline
#endif
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define PF_ATOMIC_OR_U32(p, v) atomicOr((p), (v))
#else
#define PF_ATOMIC_OR_U32(p, v) (*(p) |= (v))
#endif

#define PF_K_MAX 16u
#define PF_K_MIN 4u
#define PF_DENSITY_MAX 0.25          // above it a lookup proves too little to pay for itself: the filter stands down for that index

MONI_HD bool pf_acgt(uint32_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }
MONI_HD uint32_t pf_code(uint32_t b) { return (b >> 1) & 3u; }              // = base2: 'A' 0, 'C' 1, 'T' 2, 'G' 3

// k = min(16, ceil(log4(n_text)) + 1): a random text then fills less than a quarter of the table
MONI_HD uint32_t pf_choose_k(uint64_t n_text) {
    uint32_t e = 0;
    while (e < 32 && (1ull << (2 * e)) < n_text) ++e;                      // smallest e with 4^e >= n_text
    const uint32_t k = e + 1;
    return k > PF_K_MAX ? PF_K_MAX : k < PF_K_MIN ? PF_K_MIN : k;
}
MONI_HD uint64_t pf_table_words(uint32_t k) { const uint64_t bits = 1ull << (2 * k); return (bits + 31) / 32; }      // 32-bit words
MONI_HD bool pf_present(const uint32_t* __restrict__ tab, uint64_t v) { return (tab[v >> 5] >> (v & 31u)) & 1u; }

// The k-mers that start in text positions [32 w, 32 w + 32) into the table (one thread per w).  The bit is tested with a plain load first: a
// text of one repeated k-mer would otherwise send every position's atomic to one word.
MONI_HD void pf_build_word(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t w, uint32_t k, uint32_t* __restrict__ tab) {
    const uint64_t p0 = 32 * w;
    if (p0 + k > n_text) return;
    uint64_t end = p0 + 31 + k;                                            // one past the last byte of the last k-mer that starts in this word
    if (end > n_text) end = n_text;
    const uint64_t mask = (1ull << (2 * k)) - 1;
    uint64_t v = 0;
    uint32_t run = 0;                                                      // A / C / G / T bytes in a row up to here
    for (uint64_t p = p0; p < end; ++p) {
        const uint32_t b = text[p];
        if (!pf_acgt(b)) { run = 0; v = 0; continue; }
        v = (v >> 2) | ((uint64_t)pf_code(b) << (2 * (k - 1)));
        if (++run >= k) {
            const uint64_t x = v & mask;
            if (!pf_present(tab, x)) PF_ATOMIC_OR_U32(&tab[x >> 5], 1u << (x & 31u));
        }
    }
}

// A task's 2-bit code words (pack_task: base qi in word qi >> 5, bits 2 (qi & 31) ..), word w at codes[w * stride], through a register copy
// of the two words a k-mer can lie in.
struct pf_pat_t {
    const uint64_t* codes; uint64_t stride; uint32_t n_words;
    uint32_t w; uint64_t lo, hi;
};
MONI_HD void pf_pat_init(pf_pat_t& P, const uint64_t* codes, uint64_t stride, uint32_t m) {
    P.codes = codes; P.stride = stride; P.n_words = (m + 31u) >> 5; P.w = 0xFFFFFFFFu; P.lo = P.hi = 0;
}
// the k-mer at pattern offset q (q + k <= m); one that straddles two words takes its upper bases from the next word
MONI_HD uint64_t pf_kmer(pf_pat_t& P, uint32_t q, uint32_t k) {
    const uint32_t w = q >> 5, sh = 2 * (q & 31u);
    if (w != P.w) {
        P.lo = w == P.w + 1 && P.w != 0xFFFFFFFFu ? P.hi : P.codes[(uint64_t)w * P.stride];
        P.hi = w + 1 < P.n_words ? P.codes[(uint64_t)(w + 1) * P.stride] : 0;
        P.w = w;
    }
    const uint64_t v = sh ? (P.lo >> sh) | (P.hi << (64u - sh)) : P.lo;
    return v & ((1ull << (2 * k)) - 1);
}

// Can the task hold a MEM of min_len bases?  (The caller has dealt with pflag, min_len < k and m < min_len.)  W = min_len - k + 1 k-mers make
// a window; the task is live when W k-mers in a row are present.  Every such row holds a k-mer at an offset that is a multiple of W, so those
// are looked up first, and only around one that is present its neighbours: to the left while present (at most W - 1), then to the right for
// what is still missing.  Leaves at the first complete window.
MONI_HD bool pf_task_live(pf_pat_t& P, uint32_t m, uint32_t min_len, uint32_t k, const uint32_t* __restrict__ tab, unsigned long long& n_lookups) {
    const uint32_t W = min_len - k + 1, nk = m - k + 1;
    for (uint32_t p = 0; p < nk; p += W) {
        ++n_lookups;
        if (!pf_present(tab, pf_kmer(P, p, k))) continue;
        uint32_t have = 1;
        for (uint32_t q = p; q > 0 && have < W; ) {
            --q; ++n_lookups;
            if (!pf_present(tab, pf_kmer(P, q, k))) break;
            ++have;
        }
        for (uint32_t q = p + 1; q < nk && have < W; ++q) {
            ++n_lookups;
            if (!pf_present(tab, pf_kmer(P, q, k))) break;
            ++have;
        }
        if (have >= W) return true;
    }
    return false;
}

// the decision for one task; pflag: the pattern holds a byte outside A / C / G / T.  Returns true when the task must be worked on.
MONI_HD bool pf_task_keep(pf_pat_t& P, uint32_t m, uint32_t min_len, uint32_t k, bool pflag, const uint32_t* __restrict__ tab, unsigned long long& n_lookups) {
    if (pflag || min_len < k || tab == nullptr) return true;
    if (m < min_len) return false;
    return pf_task_live(P, m, min_len, k, tab, n_lookups);
}
