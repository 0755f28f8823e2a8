// Per-block code of the BGZF writer: one BGZF block = one gzip member with one raw DEFLATE block, made by one workgroup of
// BGZF_T lanes.  The file compiles for the host with the lanes as loops (tests/host_sim/bgzf_sim.cpp): a phase is a BGZF_LANES loop, BGZF_SYNC
// stands between two phases, and whatever one phase hands the next lives in bgzf_shared_t (LDS on the device).  What lanes share inside a phase
// is order-independent - a maximum (hash table), sums (histograms, counters), an XOR (the CRC), ORs into zeroed words (the bit stream) - so the
// bytes are a function of (text, block_size, level) alone and the host replay equals the kernel byte for byte.
//
// Phases of a block of n bytes:
//   crc      lane l takes the l-th piece of ceil(n / T) bytes with a table in LDS, multiplies by x^(8 * bytes behind the piece), XORs into S.crc
//   match    per stretch of T positions: lane l looks position base + l up in the hash table (3-byte hash, the latest earlier position of
//            every hash value BEFORE the stretch) and at distance 1 (runs), measures both, keeps the longer; then all lanes enter their
//            positions (maximum) while lane 0 walks the stretch from S.next and writes one token per literal or match to the token region
//   hist     tokens -> the counts of the 286 + 30 symbols
//   lengths  rank sort of the used symbols (all lanes), then one lane per alphabet: Huffman depths in place (Moffat / Katajainen), depth
//            limit by moving codes down one level at a time with the Kraft sum kept at 1, canonical codes bit-reversed for LSB-first packing
//   header   the code-length code (limit 7) over the lengths 0..15 as they are - symbols 16/17/18 are not used -, the size of the
//            dynamic block; stored where that is not smaller
//   emit     lane l takes the l-th run of ceil(ntok / T) tokens: bit sums, an exclusive scan, then every lane ORs its codes in
//   frame    BGZF header, CRC-32 and ISIZE, the block's size
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/moni_hip.h"

#ifndef MONI_HD
#if defined(__HIPCC__)
#define MONI_HD __host__ __device__ __forceinline__
#else
#define MONI_HD inline
#endif
#endif

#define BGZF_T 256u                 // lanes of a block's workgroup
#define BGZF_MAX_BLOCK 65280u       // uncompressed bytes of a block at most
#define BGZF_FRAME 31u              // bytes a stored block adds to its text: 18 of header, 5 of the stored block's, CRC-32 and ISIZE
#define BGZF_MIN_DYNAMIC 30u        // up to here a block is stored without a look: a dynamic block spends 3 + 14 + 12 bits and a length
                                    // for each of 257 literal/length and one distance symbol, over 35 bytes, before its first code
#define BGZF_HASH_BITS 13
#define BGZF_MIN_MATCH 3u
#define BGZF_MAX_MATCH 258u
#define BGZF_MAX_DIST 32768u
#define BGZF_NLIT 286u
#define BGZF_NDIST 30u
#define BGZF_NCL 19u
#define BGZF_CRC_POLY 0xEDB88320u

#if defined(__HIP_DEVICE_COMPILE__)
#define BGZF_LANES(l) for (uint32_t l = threadIdx.x, once_ = 1; once_; once_ = 0)
#define BGZF_SYNC() __syncthreads()
#else
#define BGZF_LANES(l) for (uint32_t l = 0; l < BGZF_T; ++l)
#define BGZF_SYNC() ((void)0)
#endif
#if defined(__HIPCC__)
#define BGZF_FN __device__ __forceinline__
#define BGZF_TABLE static __device__ const
#else
#define BGZF_FN inline
#define BGZF_TABLE static const
#endif

// the order in which a dynamic block sends the lengths of the code-length code (RFC 1951, 3.2.7)
BGZF_TABLE uint8_t bgzf_cl_order[BGZF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- shared updates: each commutes with itself, so the order of the lanes does not show ----
BGZF_FN void bgzf_amax(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (*p < v) *p = v;
#endif
}
BGZF_FN void bgzf_aadd(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
BGZF_FN void bgzf_axor(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicXor(p, v);
#else
    *p ^= v;
#endif
}
BGZF_FN void bgzf_aor(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
BGZF_FN void bgzf_aadd64(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// ---- symbols -------------------------------------------------------------------------------------------------------------------------
MONI_HD uint32_t bgzf_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
// length 3..258 -> its code 257..285, the number of extra bits and their value
MONI_HD void bgzf_len_sym(uint32_t len, uint32_t& code, uint32_t& eb, uint32_t& ev) {
    const uint32_t ll = len - 3u;
    if (ll < 8u) { code = 257u + ll; eb = 0; ev = 0; return; }
    if (len == 258u) { code = 285u; eb = 0; ev = 0; return; }
    eb = bgzf_log2(ll) - 2u;
    code = 261u + 4u * eb + ((ll >> eb) & 3u);
    ev = ll & ((1u << eb) - 1u);
}
// distance 1..32768 -> its code 0..29
MONI_HD void bgzf_dist_sym(uint32_t dist, uint32_t& code, uint32_t& eb, uint32_t& ev) {
    const uint32_t dd = dist - 1u;
    if (dd < 4u) { code = dd; eb = 0; ev = 0; return; }
    const uint32_t nb = bgzf_log2(dd);
    eb = nb - 1u;
    code = 2u * nb + ((dd >> eb) & 1u);
    ev = dd & ((1u << eb) - 1u);
}
MONI_HD uint32_t bgzf_len_extra(uint32_t code) { return code < 265u || code == 285u ? 0u : (code - 261u) >> 2; }
MONI_HD uint32_t bgzf_dist_extra(uint32_t code) { return code < 4u ? 0u : (code >> 1) - 1u; }

// a token: the byte at its position | length << 8 | (distance - 1) << 17; length 0: the literal
MONI_HD uint32_t bgzf_tok_len(uint32_t e) { return (e >> 8) & 0x1FFu; }
MONI_HD uint32_t bgzf_tok_dist(uint32_t e) { return (e >> 17) + 1u; }

// ---- bytes ---------------------------------------------------------------------------------------------------------------------------
MONI_HD uint64_t bgzf_ld64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
MONI_HD uint32_t bgzf_hash3(const uint8_t* p) {
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return (v * 0x9E3779B1u) >> (32 - BGZF_HASH_BITS);
}
// common prefix of a and b, at most maxlen; no byte at or past a + maxlen / b + maxlen is read
// (every step is a round trip through L2 that the next one waits for: 32 bytes a step while they last, and the last bytes with one load that ends at maxlen)
MONI_HD uint32_t bgzf_match_len(const uint8_t* a, const uint8_t* b, uint32_t maxlen) {
    uint32_t k = 0;
    while (k + 32u <= maxlen) {
        const uint64_t x0 = bgzf_ld64(a + k) ^ bgzf_ld64(b + k), x1 = bgzf_ld64(a + k + 8) ^ bgzf_ld64(b + k + 8);
        const uint64_t x2 = bgzf_ld64(a + k + 16) ^ bgzf_ld64(b + k + 16), x3 = bgzf_ld64(a + k + 24) ^ bgzf_ld64(b + k + 24);
        if (x0) return k + ((uint32_t)__builtin_ctzll(x0) >> 3);
        if (x1) return k + 8u + ((uint32_t)__builtin_ctzll(x1) >> 3);
        if (x2) return k + 16u + ((uint32_t)__builtin_ctzll(x2) >> 3);
        if (x3) return k + 24u + ((uint32_t)__builtin_ctzll(x3) >> 3);
        k += 32u;
    }
    while (k + 8u <= maxlen) {
        const uint64_t x = bgzf_ld64(a + k) ^ bgzf_ld64(b + k);
        if (x) return k + ((uint32_t)__builtin_ctzll(x) >> 3);
        k += 8u;
    }
    if (k < maxlen && maxlen >= 8u) {          // the 8 bytes that end at maxlen: those before k are known to be equal
        const uint64_t x = bgzf_ld64(a + maxlen - 8u) ^ bgzf_ld64(b + maxlen - 8u);
        return x ? maxlen - 8u + ((uint32_t)__builtin_ctzll(x) >> 3) : maxlen;
    }
    while (k < maxlen && a[k] == b[k]) ++k;
    return k;
}

// ---- CRC-32 (IEEE, reflected): polynomials mod P with bit 31 = x^0 --------------------------------------------------------------------
MONI_HD uint32_t bgzf_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ BGZF_CRC_POLY : b >> 1;
    }
    return p;
}
// the CRC of a piece followed by `behind` zero-effect bytes: crc * x^(8 * behind); crc(A B) = shift(crc(A), |B|) ^ crc(B)
MONI_HD uint32_t bgzf_crc_shift(uint32_t crc, uint32_t behind) {
    uint32_t sq = 0x00800000u, p = 0x80000000u;          // x^8, x^0
    for (; behind; behind >>= 1) {
        if (behind & 1u) p = bgzf_gf_mul(sq, p);
        sq = bgzf_gf_mul(sq, sq);
    }
    return bgzf_gf_mul(p, crc);
}

// ---- code lengths ---------------------------------------------------------------------------------------------------------------------
// Workspace of one alphabet of at most N symbols.
template <int N>
struct bgzf_hl_t {
    uint32_t A[N];            // the used symbols' counts in increasing order; then their depths
    uint16_t sym[N];          // the used symbols in that order (ties: the smaller symbol first)
    uint32_t cnt[16], nxt[16];
    uint32_t nu;
};

// All lanes: zero the lengths, put the used symbols in order by counting, per symbol, the used symbols that go before it.
BGZF_FN void bgzf_hl_rank(const uint32_t* freq, uint32_t n, uint8_t* len, uint32_t* A, uint16_t* sym, uint32_t* nu, uint32_t lane) {
    for (uint32_t s = lane; s < n; s += BGZF_T) {
        len[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t g = freq[j];
            r += (g && (g < f || (g == f && j < s))) ? 1u : 0u;
        }
        A[r] = f;
        sym[r] = (uint16_t)s;
    }
    if (lane == 0) {
        uint32_t u = 0;
        for (uint32_t j = 0; j < n; ++j) u += freq[j] ? 1u : 0u;
        *nu = u;
    }
}

// One lane, after bgzf_hl_rank: lengths of at most `limit` bits with Kraft sum 1, then the canonical codes, bit-reversed.
// One used symbol: length 1 (RFC 1951: one distance code); with `complete` a second symbol takes the other code of length 1, since
// the code-length code has to be complete.  No used symbol: every length 0.
BGZF_FN void bgzf_hl_finish(uint32_t n, uint32_t limit, bool complete, uint8_t* len, uint16_t* code, uint32_t* A, const uint16_t* sym,
                            uint32_t nu, uint32_t* cnt, uint32_t* nxt) {
    if (nu == 1) {
        len[sym[0]] = 1;
        if (complete) len[sym[0] == 0 ? 1 : 0] = 1;
    } else if (nu >= 2) {
        // depths in place (Moffat & Katajainen, "In-place calculation of minimum-redundancy codes"): A sorted increasing
        const int m = (int)nu;
        A[0] += A[1];
        int root = 0, leaf = 2, next;
        for (next = 1; next < m - 1; ++next) {
            if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = m - 2; next = m - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
            while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
        // codes per length, the deeper ones taken up to the limit; then codes move down a level until the Kraft sum is 1 again
        for (uint32_t i = 0; i < 16; ++i) cnt[i] = 0;
        for (uint32_t i = 0; i < nu; ++i) { const uint32_t d = A[i]; cnt[d > limit ? limit : d] += 1; }
        uint32_t total = 0;
        for (uint32_t i = limit; i >= 1; --i) total += cnt[i] << (limit - i);
        while (total != (1u << limit)) {
            cnt[limit] -= 1;
            for (uint32_t i = limit - 1; i >= 1; --i)
                if (cnt[i]) { cnt[i] -= 1; cnt[i + 1] += 2; break; }
            total -= 1;
        }
        // the most frequent symbols take the shortest codes
        uint32_t j = nu;
        for (uint32_t i = 1; i <= limit; ++i)
            for (uint32_t k = cnt[i]; k; --k) len[sym[--j]] = (uint8_t)i;
    }
    for (uint32_t i = 0; i < 16; ++i) cnt[i] = 0;
    for (uint32_t s = 0; s < n; ++s) cnt[len[s]] += 1;
    uint32_t c = 0;
    cnt[0] = 0; nxt[0] = 0;
    for (uint32_t i = 1; i < 16; ++i) { c = (c + cnt[i - 1]) << 1; nxt[i] = c; }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s];
        uint32_t v = 0;
        if (l) {
            uint32_t x = nxt[l]++;
            for (uint32_t i = 0; i < l; ++i) { v = (v << 1) | (x & 1u); x >>= 1; }
        }
        code[s] = (uint16_t)v;
    }
}

// ---- the bit stream of a block: 32-bit words of the zeroed staging slot, LSB first ----------------------------------------------------
struct bgzf_bits_t {
    uint32_t* w;
    uint64_t acc;
    uint32_t nb, word;
};
BGZF_FN void bgzf_bits_at(bgzf_bits_t& B, uint32_t* slot, uint32_t bitpos) { B.w = slot; B.acc = 0; B.nb = bitpos & 31u; B.word = bitpos >> 5; }
BGZF_FN void bgzf_put(bgzf_bits_t& B, uint32_t v, uint32_t n) {          // n <= 32, v < 2^n
    B.acc |= (uint64_t)v << B.nb;
    B.nb += n;
    if (B.nb >= 32u) {
        if ((uint32_t)B.acc) bgzf_aor(B.w + B.word, (uint32_t)B.acc);
        ++B.word; B.acc >>= 32; B.nb -= 32u;
    }
}
BGZF_FN void bgzf_flush(bgzf_bits_t& B) { if ((uint32_t)B.acc) bgzf_aor(B.w + B.word, (uint32_t)B.acc); B.acc = 0; }

// ---- a block ------------------------------------------------------------------------------------------------------------------------
struct bgzf_shared_t {
    uint32_t table[1u << BGZF_HASH_BITS];      // hash -> position + 1 of its latest occurrence before the current stretch, 0: none
    uint32_t chunk[BGZF_T];                    // the current stretch: a token per position (what the walk would emit there)
    uint16_t hh[BGZF_T];                       // ... and its hash (0xFFFF: less than 3 bytes left)
    uint32_t crc_tab[256];
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    bgzf_hl_t<288> lw;
    bgzf_hl_t<32> dw;                          // distances, then the code-length code
    uint16_t lcode[288], dcode[32], ccode[20];
    uint8_t llen[288], dlen[32], clen[20];
    uint32_t lane_bits[BGZF_T + 1];
    uint32_t crc, next, ntok, nmatch, nlit, ndist, ncl, hdr_bits, dyn_bits, use_dyn;
};

// staging bytes of a block: the largest it can become (stored), in whole 8-byte words
MONI_HD uint32_t bgzf_slot_bytes(uint32_t block_size) { return (block_size + BGZF_FRAME + 7u) & ~7u; }

struct bgzf_args_t {
    const uint8_t* text; uint64_t len;         // the whole input
    uint32_t block_size, level;
    uint64_t n_blocks;
    uint32_t* staging;                         // n_blocks slots of bgzf_slot_bytes(block_size) bytes, zero
    uint32_t* tok;                             // BGZF_MAX_BLOCK tokens per workgroup
    uint64_t* out_len; uint64_t* out_off;      // per block: its bytes, its slot in 8-byte words (what the gather takes)
    unsigned long long* counters;              // [0] matches [1] literals [2] stored blocks [3] blocks whose emitted bits missed the computed size (0)
};

BGZF_FN void bgzf_put_gz_header(bgzf_bits_t& B, uint32_t total) {
    bgzf_put(B, 0x04088B1Fu, 32); bgzf_put(B, 0, 32); bgzf_put(B, 0xFF00u, 16); bgzf_put(B, 0x0006u, 16);
    bgzf_put(B, 0x00024342u, 32); bgzf_put(B, total - 1u, 16);
}

// Block b of the input, by the BGZF_T lanes of one workgroup; tok: this workgroup's token region.
BGZF_FN void bgzf_block(bgzf_shared_t& S, const bgzf_args_t& G, uint64_t b, uint32_t* tok) {
    const uint64_t at = b * G.block_size;
    const uint8_t* t = G.text + at;
    const uint32_t n = (uint32_t)(G.len - at < G.block_size ? G.len - at : G.block_size);
    uint32_t* slot = G.staging + b * (bgzf_slot_bytes(G.block_size) / 4u);

    BGZF_LANES(l) {
        for (uint32_t i = l; i < (1u << BGZF_HASH_BITS); i += BGZF_T) S.table[i] = 0;
        for (uint32_t i = l; i < 288u; i += BGZF_T) S.lfreq[i] = 0;
        if (l < 32u) S.dfreq[l] = 0;
        if (l < 20u) S.cfreq[l] = 0;
        uint32_t c = l;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ BGZF_CRC_POLY : c >> 1;
        S.crc_tab[l] = c;
        if (l == 0) { S.crc = 0; S.next = 0; S.ntok = 0; S.nmatch = 0; S.use_dyn = 0; }
    }
    BGZF_SYNC();

    // crc
    BGZF_LANES(l) {
        const uint32_t piece = (n + BGZF_T - 1u) / BGZF_T;
        const uint32_t lo = l * piece < n ? l * piece : n, hi = lo + piece < n ? lo + piece : n;
        if (hi > lo) {
            uint32_t c = 0xFFFFFFFFu;
            for (uint32_t i = lo; i < hi; ++i) c = S.crc_tab[(c ^ t[i]) & 0xFFu] ^ (c >> 8);
            bgzf_axor(&S.crc, bgzf_crc_shift(~c, n - hi));
        }
    }

    if (G.level && n > BGZF_MIN_DYNAMIC) {
        // match
        for (uint32_t base = 0; base < n; base += BGZF_T) {
            BGZF_LANES(l) {
                const uint32_t p = base + l;
                uint32_t e = 0, h = 0xFFFFu;
                if (p < n) {
                    const uint32_t maxlen = n - p < BGZF_MAX_MATCH ? n - p : BGZF_MAX_MATCH;
                    uint32_t len = 0, dist = 0;
                    e = t[p];
                    if (maxlen >= BGZF_MIN_MATCH) {
                        h = bgzf_hash3(t + p);
                        const uint32_t c = S.table[h];
                        if (c && p - (c - 1u) <= BGZF_MAX_DIST) { len = bgzf_match_len(t + p, t + (c - 1u), maxlen); dist = p - (c - 1u); }
                        if (p && t[p - 1] == e && len < maxlen) {
                            const uint32_t rl = bgzf_match_len(t + p, t + p - 1, maxlen);
                            if (rl >= len) { len = rl; dist = 1; }
                        }
                        if (len >= BGZF_MIN_MATCH) e |= (len << 8) | ((dist - 1u) << 17);
                    }
                }
                S.chunk[l] = e;
                S.hh[l] = (uint16_t)h;
            }
            BGZF_SYNC();
            BGZF_LANES(l) {
                const uint32_t h = S.hh[l];
                if (h != 0xFFFFu) bgzf_amax(&S.table[h], base + l + 1u);
                if (l == 0) {
                    const uint32_t end = base + BGZF_T < n ? base + BGZF_T : n;
                    uint32_t next = S.next, ntok = S.ntok;
                    while (next < end) {
                        const uint32_t e = S.chunk[next - base];
                        const uint32_t len = bgzf_tok_len(e);
                        tok[ntok++] = e;
                        next += len ? len : 1u;
                    }
                    S.next = next; S.ntok = ntok;
                }
            }
            BGZF_SYNC();
        }

        // hist
        BGZF_LANES(l) {
            const uint32_t ntok = S.ntok;
            uint32_t nm = 0;
            for (uint32_t i = l; i < ntok; i += BGZF_T) {
                const uint32_t e = tok[i], len = bgzf_tok_len(e);
                if (len) {
                    uint32_t c, eb, ev;
                    bgzf_len_sym(len, c, eb, ev); bgzf_aadd(&S.lfreq[c], 1);
                    bgzf_dist_sym(bgzf_tok_dist(e), c, eb, ev); bgzf_aadd(&S.dfreq[c], 1);
                    ++nm;
                } else bgzf_aadd(&S.lfreq[e & 0xFFu], 1);
            }
            if (nm) bgzf_aadd(&S.nmatch, nm);
            if (l == 0) bgzf_aadd(&S.lfreq[256], 1);
        }
        BGZF_SYNC();

        // lengths
        BGZF_LANES(l) {
            bgzf_hl_rank(S.lfreq, BGZF_NLIT, S.llen, S.lw.A, S.lw.sym, &S.lw.nu, l);
            bgzf_hl_rank(S.dfreq, BGZF_NDIST, S.dlen, S.dw.A, S.dw.sym, &S.dw.nu, l);
        }
        BGZF_SYNC();
        BGZF_LANES(l) {
            if (l == 0) bgzf_hl_finish(BGZF_NLIT, 15, false, S.llen, S.lcode, S.lw.A, S.lw.sym, S.lw.nu, S.lw.cnt, S.lw.nxt);
            if (l == 64) bgzf_hl_finish(BGZF_NDIST, 15, false, S.dlen, S.dcode, S.dw.A, S.dw.sym, S.dw.nu, S.dw.cnt, S.dw.nxt);
        }
        BGZF_SYNC();

        // header: how many lengths are sent, how often each length occurs among them
        BGZF_LANES(l) {
            if (l == 0) {
                uint32_t nlit = BGZF_NLIT, ndist = BGZF_NDIST;
                while (nlit > 257u && !S.llen[nlit - 1]) --nlit;
                while (ndist > 1u && !S.dlen[ndist - 1]) --ndist;
                S.nlit = nlit; S.ndist = ndist;
                for (uint32_t i = 0; i < nlit; ++i) S.cfreq[S.llen[i]] += 1;
                for (uint32_t i = 0; i < ndist; ++i) S.cfreq[S.dlen[i]] += 1;
            }
        }
        BGZF_SYNC();
        BGZF_LANES(l) { bgzf_hl_rank(S.cfreq, BGZF_NCL, S.clen, S.dw.A, S.dw.sym, &S.dw.nu, l); }
        BGZF_SYNC();
        BGZF_LANES(l) {
            if (l == 0) {
                bgzf_hl_finish(BGZF_NCL, 7, true, S.clen, S.ccode, S.dw.A, S.dw.sym, S.dw.nu, S.dw.cnt, S.dw.nxt);
                uint32_t ncl = BGZF_NCL;
                while (ncl > 4u && !S.clen[bgzf_cl_order[ncl - 1]]) --ncl;
                uint32_t bits = 17u + 3u * ncl;
                for (uint32_t i = 0; i < BGZF_NCL; ++i) bits += S.cfreq[i] * S.clen[i];
                S.ncl = ncl; S.hdr_bits = bits;
                for (uint32_t i = 0; i < BGZF_NLIT; ++i) bits += S.lfreq[i] * (S.llen[i] + (i > 256u ? bgzf_len_extra(i) : 0u));
                for (uint32_t i = 0; i < BGZF_NDIST; ++i) bits += S.dfreq[i] * (S.dlen[i] + bgzf_dist_extra(i));
                S.dyn_bits = bits;
                S.use_dyn = (bits + 7u) / 8u < n + 5u ? 1u : 0u;
            }
        }
        BGZF_SYNC();
    } else {
        BGZF_SYNC();
    }

    if (S.use_dyn) {
        // emit: the bits of every lane's run of tokens, where each run starts, then the codes
        BGZF_LANES(l) {
            const uint32_t ntok = S.ntok, per = (ntok + BGZF_T - 1u) / BGZF_T;
            const uint32_t lo = l * per < ntok ? l * per : ntok, hi = lo + per < ntok ? lo + per : ntok;
            uint32_t bits = 0;
            for (uint32_t i = lo; i < hi; ++i) {
                const uint32_t e = tok[i], len = bgzf_tok_len(e);
                if (len) {
                    uint32_t c, eb, ev;
                    bgzf_len_sym(len, c, eb, ev); bits += S.llen[c] + eb;
                    bgzf_dist_sym(bgzf_tok_dist(e), c, eb, ev); bits += S.dlen[c] + eb;
                } else bits += S.llen[e & 0xFFu];
            }
            S.lane_bits[l] = bits;
        }
        BGZF_SYNC();
        BGZF_LANES(l) {
            if (l == 0) {
                uint32_t at_bit = 144u + S.hdr_bits;
                for (uint32_t i = 0; i < BGZF_T; ++i) { const uint32_t v = S.lane_bits[i]; S.lane_bits[i] = at_bit; at_bit += v; }
                S.lane_bits[BGZF_T] = at_bit;
            }
        }
        BGZF_SYNC();
        BGZF_LANES(l) {
            const uint32_t ntok = S.ntok, per = (ntok + BGZF_T - 1u) / BGZF_T;
            const uint32_t lo = l * per < ntok ? l * per : ntok, hi = lo + per < ntok ? lo + per : ntok;
            bgzf_bits_t B;
            if (hi > lo) {
                bgzf_bits_at(B, slot, S.lane_bits[l]);
                for (uint32_t i = lo; i < hi; ++i) {
                    const uint32_t e = tok[i], len = bgzf_tok_len(e);
                    if (len) {
                        uint32_t c, eb, ev;
                        bgzf_len_sym(len, c, eb, ev);
                        bgzf_put(B, S.lcode[c], S.llen[c]);
                        if (eb) bgzf_put(B, ev, eb);
                        bgzf_dist_sym(bgzf_tok_dist(e), c, eb, ev);
                        bgzf_put(B, S.dcode[c], S.dlen[c]);
                        if (eb) bgzf_put(B, ev, eb);
                    } else bgzf_put(B, S.lcode[e & 0xFFu], S.llen[e & 0xFFu]);
                }
                bgzf_flush(B);
            }
            if (l == 0) {
                // frame: the gzip member's header, the block's header, the end-of-block code, CRC-32 and ISIZE
                const uint32_t dbytes = (S.dyn_bits + 7u) / 8u, total = 18u + dbytes + 8u;
                bgzf_bits_at(B, slot, 0);
                bgzf_put_gz_header(B, total);
                bgzf_put(B, 1, 1); bgzf_put(B, 2, 2);
                bgzf_put(B, S.nlit - 257u, 5); bgzf_put(B, S.ndist - 1u, 5); bgzf_put(B, S.ncl - 4u, 4);
                for (uint32_t i = 0; i < S.ncl; ++i) bgzf_put(B, S.clen[bgzf_cl_order[i]], 3);
                for (uint32_t i = 0; i < S.nlit; ++i) bgzf_put(B, S.ccode[S.llen[i]], S.clen[S.llen[i]]);
                for (uint32_t i = 0; i < S.ndist; ++i) bgzf_put(B, S.ccode[S.dlen[i]], S.clen[S.dlen[i]]);
                bgzf_flush(B);
                const uint32_t eob = S.lane_bits[BGZF_T];
                bgzf_bits_at(B, slot, eob);
                bgzf_put(B, S.lcode[256], S.llen[256]);
                bgzf_flush(B);
                bgzf_bits_at(B, slot, 8u * (18u + dbytes));
                bgzf_put(B, S.crc, 32); bgzf_put(B, n, 32);
                bgzf_flush(B);
                G.out_len[b] = total; G.out_off[b] = b * (bgzf_slot_bytes(G.block_size) / 8u);
                bgzf_aadd64(&G.counters[0], S.nmatch);
                bgzf_aadd64(&G.counters[1], S.ntok - S.nmatch);
                if (eob + S.llen[256] != 144u + S.dyn_bits) bgzf_aadd64(&G.counters[3], 1);
            }
        }
    } else {
        // stored: bytes only, no word of the slot is shared
        uint8_t* s8 = reinterpret_cast<uint8_t*>(slot);
        BGZF_LANES(l) {
            for (uint32_t i = l; i < n; i += BGZF_T) s8[23u + i] = t[i];
            if (l == 0) {
                const uint32_t total = 18u + 5u + n + 8u;
                const uint8_t hd[16] = {0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0, 0xFF, 0x06, 0, 0x42, 0x43, 0x02, 0};
                for (uint32_t i = 0; i < 16; ++i) s8[i] = hd[i];
                s8[16] = (uint8_t)((total - 1u) & 0xFFu); s8[17] = (uint8_t)((total - 1u) >> 8);
                s8[18] = 1;
                s8[19] = (uint8_t)(n & 0xFFu); s8[20] = (uint8_t)(n >> 8); s8[21] = (uint8_t)(~n & 0xFFu); s8[22] = (uint8_t)((~n >> 8) & 0xFFu);
                const uint32_t crc = S.crc;
                for (uint32_t i = 0; i < 4; ++i) { s8[23u + n + i] = (uint8_t)(crc >> (8u * i)); s8[27u + n + i] = (uint8_t)(n >> (8u * i)); }
                G.out_len[b] = total; G.out_off[b] = b * (bgzf_slot_bytes(G.block_size) / 8u);
                bgzf_aadd64(&G.counters[2], 1);
            }
        }
    }
    BGZF_SYNC();
}

// block_size 1..65280, level 0 or 1, reserved 0 (eof: any non-zero value asks for the end-of-file block)
MONI_HD bool bgzf_params_ok(const moni_bgzf_params_t& p) {
    return p.block_size >= 1 && p.block_size <= BGZF_MAX_BLOCK && p.level <= 1 && !p.reserved;
}
