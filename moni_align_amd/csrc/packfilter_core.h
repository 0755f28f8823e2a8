// The fused front end of the filtered seeding stage, written once and compiled twice like seed_core.h and prefilter_core.h: as __device__ code
// inside seed_kernels.hip (pack_filter_kernel) and as plain host C++ by tests/host_sim/packfilter_sim.cpp.
//
// One lane per READ does what pack_task (both tasks of the read) and pf_task_keep (both tasks) do, and leaves out what their results do not need:
//   - the read's bytes are loaded once, as aligned 8-byte words;
//   - a read that holds only upper-case A / C / G / T (and fits the lane's window of code words) needs no table: the code of a byte is
//     (b >> 1) & 3 (seed_core.h: base2), the complement of a code is code ^ 2, so strand 1's code words are strand 0's with the bases in reverse
//     order, shifted for m % 32 and XORed with 0xAAAA..., and the bytes of a pattern are spelled from the codes of the other strand;
//   - both tasks are decided by pf_task_keep on code words that lie in the lane's own column (LDS in the kernel): no read-back from the workspace;
//   - the byte words of a task that is skipped are not written (8 of the 10 words a 150-base task has).  Only the LF walk and the byte
//     comparison of mem_task read them, and both work on live tasks.
// Any other read - a byte outside A / C / G / T, or more bases than the window holds - takes pack_task itself for both tasks and the filter over
// the code words pack_task wrote, so results are those of pack_kernel + strand_filter_kernel in every case.
//
// The arithmetic form relies on compl_tab mapping A / C / G / T to T / G / C / A (pk_compl_ok, checked once per index by the caller).
#pragma once
#include <stdint.h>

#include "seed_core.h"
#include "prefilter_core.h"

MONI_HD bool pk_compl_ok(const uint8_t* compl_tab) { return compl_tab['A'] == 'T' && compl_tab['C'] == 'G' && compl_tab['G'] == 'C' && compl_tab['T'] == 'A'; }

#define PK_B01 0x0101010101010101ull
// the bytes A / C / G / T of eight 2-bit codes, code j in bits 0..1 of byte j:  A 0x41, C 0x43 (^ 0x02), T 0x54 (^ 0x15), G 0x47 (^ 0x02 ^ 0x15 ^ 0x11)
MONI_HD uint64_t pk_spell8(uint64_t c) {
    const uint64_t c0 = c & PK_B01, c1 = (c >> 1) & PK_B01;
    return (0x41 * PK_B01) ^ (c0 * 0x02) ^ (c1 * 0x15) ^ ((c0 & c1) * 0x11);
}
// bit 7 of byte j: byte j of v is not one of A / C / G / T
MONI_HD uint64_t pk_bad8(uint64_t v) {
    const uint64_t e = v ^ pk_spell8((v >> 1) & (3 * PK_B01));
    return (((e & (0x7F * PK_B01)) + (0x7F * PK_B01)) | e) & (0x80 * PK_B01);
}
// bits 0..1 of the eight bytes of c into 16 bits, and back
MONI_HD uint32_t pk_squeeze8(uint64_t c) {
    c = (c | (c >> 6)) & 0x000F000F000F000Full;
    c = (c | (c >> 12)) & 0x000000FF000000FFull;
    return (uint32_t)(c | (c >> 24)) & 0xFFFFu;
}
MONI_HD uint64_t pk_spread8(uint32_t c16) {
    uint64_t c = c16;
    c = (c | (c << 24)) & 0x000000FF000000FFull;
    c = (c | (c << 12)) & 0x000F000F000F000Full;
    return (c | (c << 6)) & (3 * PK_B01);
}
// the 32 bases of a code word in reverse order
MONI_HD uint64_t pk_rev32(uint64_t x) {
    x = bswap64_(x);
    x = ((x & 0x0F0F0F0F0F0F0F0Full) << 4) | ((x >> 4) & 0x0F0F0F0F0F0F0F0Full);
    return ((x & 0x3333333333333333ull) << 2) | ((x >> 2) & 0x3333333333333333ull);
}
// the code bits of bases [32 w, 32 w + 32) that lie inside a pattern of m bases
MONI_HD uint64_t pk_valid_bits(uint32_t m, uint32_t w) { const uint32_t left = m - 32 * w; return left >= 32 ? ~0ull : (1ull << (2 * left)) - 1; }

// what the filter is run with (as strand_filter_kernel's arguments), and the lane's column of code words
struct pk_args_t {
    uint32_t min_len, k;
    const uint32_t* tab;
    uint64_t* cw;                     // code words of strand 0 at cw[w * cw_stride], of strand 1 at cw[(cw_words + w) * cw_stride]
    uint32_t cw_stride, cw_words;     // reads of up to 32 * cw_words bases take the arithmetic form
};

// Both tasks of one read.  Always written: code words, mask words, pflag, flag, and zeroed cnt_m / cnt_s of a skipped task; the byte words of
// a task that is kept (the general form writes them for both).  n_lookups / skipped: as strand_filter_kernel counts them.
MONI_HD void pack_filter_read(const lds_tables_t& L, const pk_args_t& A, const uint8_t* __restrict__ seq, const uint64_t* __restrict__ offs, const moni_u64x2* __restrict__ blk,
                              uint64_t read, uint64_t* __restrict__ pat, uint8_t* __restrict__ pflag, uint64_t* __restrict__ flag, uint32_t* __restrict__ cnt_m,
                              uint32_t* __restrict__ cnt_s, unsigned long long& n_lookups, unsigned long long& skipped) {
    const uint64_t task0 = 2 * read;
    const uint64_t off = offs[read];
    const uint32_t m = (uint32_t)(offs[read + 1] - off);
    const uint64_t pb = ws_pat_base(blk, task0), lb = ws_block_len(blk, task0);       // (task0 is even: both tasks lie in one block, strand 1 one word on)
    const uint64_t cb = pb + 64u * ((lb + 7) / 8), mb = cb + 64u * ((lb + 31) / 32);
    const uint32_t n8 = (m + 7u) >> 3, n2 = (m + 31u) >> 5;
    bool plain = m <= 32u * A.cw_words;
    if (plain) {                                          // the forward code words from the bytes; any byte outside A / C / G / T ends the arithmetic form
        const uint64_t a0 = off & ~7ull;
        const uint32_t sh = (uint32_t)(off & 7u) * 8u;
        uint64_t lo = n8 ? *reinterpret_cast<const uint64_t*>(seq + a0) : 0, word = 0, bad = 0;
        for (uint32_t g = 0; g < n8; ++g) {
            uint64_t v = lo;
            if (sh) { lo = *reinterpret_cast<const uint64_t*>(seq + a0 + 8ull * (g + 1)); v = (v >> sh) | (lo << (64u - sh)); }      // (the buffer is padded by 16 bytes)
            else if (g + 1 < n8) lo = *reinterpret_cast<const uint64_t*>(seq + a0 + 8ull * (g + 1));
            const uint32_t nv = m - 8 * g;
            if (nv < 8) { const uint64_t in = (1ull << (8 * nv)) - 1; bad |= pk_bad8(v) & in; v &= in; }
            else bad |= pk_bad8(v);
            word |= (uint64_t)pk_squeeze8((v >> 1) & (3 * PK_B01)) << (16 * (g & 3u));
            if ((g & 3u) == 3u || g + 1 == n8) { A.cw[(g >> 2) * A.cw_stride] = word; word = 0; }
        }
        plain = bad == 0;
    }
    bool keep[2];
    if (plain) {
        // strand 1: pattern[qi] = complement of read[m - 1 - qi].  R = the read's 32 n2 bases reversed (word w of R = word n2 - 1 - w reversed) starts
        // with the d = 32 n2 - m empty places of the last word: strand 1 is R from base d on.
        const uint32_t d2 = 2 * (32 * n2 - m);
        uint64_t r0 = n2 ? pk_rev32(A.cw[(n2 - 1) * A.cw_stride]) : 0;
        for (uint32_t w = 0; w < n2; ++w) {
            const uint64_t c0 = A.cw[w * A.cw_stride];
            const uint64_t r1 = w + 1 < n2 ? pk_rev32(A.cw[(n2 - 2 - w) * A.cw_stride]) : 0;
            const uint64_t c1 = ((d2 ? (r0 >> d2) | (r1 << (64u - d2)) : r0) ^ 0xAAAAAAAAAAAAAAAAull) & pk_valid_bits(m, w);
            r0 = r1;
            A.cw[(A.cw_words + w) * A.cw_stride] = c1;
            moni_u64x2 cc; cc.x = c0; cc.y = c1;
            *reinterpret_cast<moni_u64x2*>(pat + cb + (uint64_t)w * 64u) = cc;          // (16-byte aligned: a block's words start at a multiple of 64)
            moni_u64x2 zz; zz.x = 0; zz.y = 0;
            *reinterpret_cast<moni_u64x2*>(pat + mb + (uint64_t)w * 64u) = zz;
        }
        pflag[task0] = 0; pflag[task0 + 1] = 0;
        for (uint32_t s = 0; s < 2; ++s) {
            pf_pat_t P;
            pf_pat_init(P, A.cw + (uint64_t)s * A.cw_words * A.cw_stride, A.cw_stride, m);
            keep[s] = pf_task_keep(P, m, A.min_len, A.k, false, A.tab, n_lookups);
        }
        // byte word w of a task holds pattern[m - 1 - 8 w - j] in byte j: the complement of the OTHER strand's bases 8 w + j
        for (uint32_t s = 0; s < 2; ++s) {
            if (!keep[s]) continue;
            const uint64_t* oc = A.cw + (uint64_t)(1 - s) * A.cw_words * A.cw_stride;
            uint64_t word = 0;
            for (uint32_t w = 0; w < n8; ++w) {
                if ((w & 3u) == 0) word = oc[(w >> 2) * A.cw_stride];
                uint64_t v = pk_spell8(pk_spread8((uint32_t)word & 0xFFFFu) ^ (2 * PK_B01));
                word >>= 16;
                const uint32_t nv = m - 8 * w;
                if (nv < 8) v &= (1ull << (8 * nv)) - 1;
                pat[pb + s + (uint64_t)w * 64u] = v;
            }
        }
    } else {
        for (uint32_t s = 0; s < 2; ++s) {
            pack_task(L, seq, offs, blk, task0 + s, pat, pflag);
            pf_pat_t P;
            pf_pat_init(P, pat + cb + s, 64u, m);
            keep[s] = pf_task_keep(P, m, A.min_len, A.k, pflag[task0 + s] != 0, A.tab, n_lookups);
        }
    }
    for (uint32_t s = 0; s < 2; ++s) {
        flag[task0 + s] = keep[s] ? 1u : 0u;
        if (!keep[s]) { cnt_m[task0 + s] = 0; cnt_s[task0 + s] = 0; ++skipped; }
    }
}
