// Host-only halves of the sorted BAM output: the plan that cuts the merged order of sorted runs into chunks, and the builder of
// the .bai index.  Plain C++ over include/moni_hip.h: no HIP, no context (bam_sort_api.inc wraps them; tests/host_sim/bamsort_sim.cpp builds
// them for the sanitizer run).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../include/moni_hip.h"

// ---- the merge plan ---------------------------------------------------------------------------------------------------------------------
// The merged order is that of (key, run, index).  A boundary is a vector of positions, one per run, that some point of that order gives:
// everything before the point lies below the positions.  From the boundary P the next one is found by rank:
//   1. the largest key K such that all records up to K (upper_bound per run, never below P) fit - a binary search over the key space with a
//      binary search per run;
//   2. the next key's tie group does not fit whole: it is taken run by run, whole while it fits, then up to the index that still fits;
//   3. a chunk that would be empty (one record above chunk_bytes) takes that one record.
inline int bam_merge_plan(const uint64_t* const* keys, const uint64_t* n, const uint64_t* const* offs, uint64_t R, uint64_t chunk_bytes,
                          std::vector<uint64_t>& cuts) {
    cuts.assign(R, 0);
    if (chunk_bytes > (1ull << 62)) chunk_bytes = 1ull << 62;          // sums of offsets stay inside 64 bits
    for (uint64_t r = 0; r < R; ++r) {
        if (n[r] && (!keys[r] || !offs[r])) return MONI_EINVAL;
        for (uint64_t i = 0; i < n[r]; ++i)
            if (offs[r][i] >= offs[r][i + 1] || (i && keys[r][i - 1] > keys[r][i])) return MONI_EINVAL;
    }
    std::vector<uint64_t> P(R, 0), Q(R);
    auto upper = [&](uint64_t r, uint64_t K) { return (uint64_t)(std::upper_bound(keys[r], keys[r] + n[r], K) - keys[r]); };
    auto bytes_to = [&](const std::vector<uint64_t>& T) {
        uint64_t b = 0;
        for (uint64_t r = 0; r < R; ++r)
            if (T[r] > P[r]) b += offs[r][T[r]] - offs[r][P[r]];
        return b;
    };
    auto up_to = [&](uint64_t K, std::vector<uint64_t>& T) {
        for (uint64_t r = 0; r < R; ++r) T[r] = std::max(P[r], upper(r, K));
    };
    for (;;) {
        bool left = false;
        for (uint64_t r = 0; r < R; ++r) left = left || P[r] < n[r];
        if (!left) break;
        // 1. the largest K whose records all fit; `none` when not even those of the smallest key do
        bool none = true;
        uint64_t lo = 0, hi = ~0ull;          // invariant: every K < lo fits
        up_to(hi, Q);
        if (bytes_to(Q) <= chunk_bytes) { none = false; lo = hi; }
        else {
            up_to(0, Q);
            if (bytes_to(Q) <= chunk_bytes) {
                none = false;
                hi = ~0ull;          // hi does not fit, lo = 0 does
                while (hi - lo > 1) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    up_to(mid, Q);
                    if (bytes_to(Q) <= chunk_bytes) lo = mid; else hi = mid;
                }
            }
        }
        if (none) Q = P; else up_to(lo, Q);
        // 2. the tie group of the next key, run by run
        uint64_t room = chunk_bytes - bytes_to(Q);
        bool have = false;
        uint64_t K = 0;
        for (uint64_t r = 0; r < R; ++r)
            if (Q[r] < n[r] && (!have || keys[r][Q[r]] < K)) { K = keys[r][Q[r]]; have = true; }
        if (have) {
            for (uint64_t r = 0; r < R; ++r) {
                if (Q[r] >= n[r] || keys[r][Q[r]] != K) continue;
                const uint64_t tie_end = upper(r, K), base = offs[r][Q[r]];
                // the most records of [Q[r], tie_end) whose bytes stay within room
                const uint64_t take = (uint64_t)(std::upper_bound(offs[r] + Q[r], offs[r] + tie_end + 1, base + room) - (offs[r] + Q[r])) - 1u;
                room -= offs[r][Q[r] + take] - base;
                Q[r] += take;
                if (Q[r] < tie_end) break;          // the cut: runs behind this one stay at their lower bound
            }
        }
        // 3. one record larger than a chunk: the first of the order, alone
        if (Q == P) {
            for (uint64_t r = 0; r < R; ++r)
                if (P[r] < n[r] && keys[r][P[r]] == K) { ++Q[r]; break; }
        }
        P = Q;
        cuts.insert(cuts.end(), P.begin(), P.end());
    }
    return MONI_OK;
}

// ---- the .bai builder -------------------------------------------------------------------------------------------------------------------
struct moni_bai {
    struct Ref {
        std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
        std::vector<uint64_t> lin;          // ~0: no record overlaps the window
        uint64_t first = 0, last = 0, n_mapped = 0, n_unmapped = 0;
        bool any = false;
    };
    std::vector<Ref> refs;
    uint64_t n_no_coor = 0, next_off = 0;
    bool started = false, bad = false;
    // the chunk that is open: consecutive records of one reference and one bin
    int32_t cur_ref = -1; uint32_t cur_bin = 0; uint64_t cur_beg = 0, cur_end = 0; bool open = false;
    // the order
    int64_t last_tid = -1; int32_t last_pos = -1;
    std::vector<uint8_t> bytes;

    void close_chunk() {
        if (open) refs[(size_t)cur_ref].bins[cur_bin].emplace_back(cur_beg, cur_end);
        open = false;
    }
};

inline int bai_add(moni_bai* b, const moni_bam_ent_t* ents, uint64_t n, uint64_t chunk_len, uint32_t block_size, const uint32_t* csizes,
                   uint64_t n_blocks, uint64_t file_off) {
    if (!b || b->bad || (!ents && n) || (!csizes && n_blocks) || !block_size || block_size > 65536u) return MONI_EINVAL;
    if (n_blocks != (chunk_len + block_size - 1) / block_size || (b->started && file_off != b->next_off)) return b->bad = true, MONI_EINVAL;
    std::vector<uint64_t> coff(n_blocks + 1, file_off);
    for (uint64_t k = 0; k < n_blocks; ++k) coff[k + 1] = coff[k] + csizes[k];
    if (coff[n_blocks] >= (1ull << 48)) return b->bad = true, MONI_EINVAL;
    auto voff = [&](uint64_t x) { return x == chunk_len ? coff[n_blocks] << 16 : coff[x / block_size] << 16 | x % block_size; };          // chunk_len: the block behind the chunk
    for (uint64_t i = 0; i < n; ++i) {
        const moni_bam_ent_t& e = ents[i];
        const uint64_t end_x = i + 1 < n ? ents[i + 1].off : chunk_len;
        const int64_t tid = e.ref_id < 0 ? (int64_t)b->refs.size() : e.ref_id;
        if (e.ref_id < -1 || tid > (int64_t)b->refs.size() || (e.ref_id >= 0 && (size_t)e.ref_id >= b->refs.size()) || e.pos < -1 || e.end <= e.pos ||
            e.off >= end_x || end_x > chunk_len || tid < b->last_tid || (tid == b->last_tid && e.pos < b->last_pos))
            return b->bad = true, MONI_EINVAL;
        b->last_tid = tid; b->last_pos = e.pos;
        if (e.ref_id < 0) { b->close_chunk(); ++b->n_no_coor; continue; }
        const uint64_t v0 = voff(e.off), v1 = voff(end_x);
        const uint32_t bin = e.bin_flag >> 16;
        if (b->open && b->cur_ref == e.ref_id && b->cur_bin == bin) b->cur_end = v1;
        else { b->close_chunk(); b->open = true; b->cur_ref = e.ref_id; b->cur_bin = bin; b->cur_beg = v0; b->cur_end = v1; }
        moni_bai::Ref& R = b->refs[(size_t)e.ref_id];
        if (!R.any) { R.any = true; R.first = v0; }
        R.last = v1;
        if (e.bin_flag & 4u) ++R.n_unmapped; else ++R.n_mapped;
        // the windows of 16 384 bases the record overlaps; a position of -1 counts as 0
        const uint64_t w0 = (uint64_t)std::max<int32_t>(e.pos, 0) >> 14, w1 = (uint64_t)std::max<int32_t>(e.end - 1, 0) >> 14;
        if (R.lin.size() <= w1) R.lin.resize(w1 + 1, ~0ull);
        for (uint64_t w = w0; w <= w1; ++w) R.lin[w] = std::min(R.lin[w], v0);
    }
    b->started = true;
    b->next_off = coff[n_blocks];
    return MONI_OK;
}

inline int bai_finish(moni_bai* b, uint64_t eof_off, const uint8_t** bytes, uint64_t* len) {
    if (!b || b->bad || !bytes || !len || (b->started && eof_off != b->next_off)) return MONI_EINVAL;
    b->close_chunk();
    std::vector<uint8_t>& o = b->bytes;
    o.clear();
    auto p32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); };
    auto p64 = [&](uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); };
    o.insert(o.end(), {'B', 'A', 'I', 1});
    p32((uint32_t)b->refs.size());
    for (moni_bai::Ref& R : b->refs) {
        p32((uint32_t)R.bins.size() + (R.any ? 1u : 0u));
        for (const auto& kv : R.bins) {
            p32(kv.first); p32((uint32_t)kv.second.size());
            for (const auto& c : kv.second) { p64(c.first); p64(c.second); }
        }
        if (R.any) { p32(37450u); p32(2u); p64(R.first); p64(R.last); p64(R.n_mapped); p64(R.n_unmapped); }
        p32((uint32_t)R.lin.size());
        uint64_t above = 0;
        std::vector<uint64_t> lin(R.lin);
        for (size_t w = lin.size(); w-- > 0;) { if (lin[w] == ~0ull) lin[w] = above; else above = lin[w]; }
        for (uint64_t v : lin) p64(v);
    }
    p64(b->n_no_coor);
    *bytes = o.data(); *len = o.size();
    return MONI_OK;
}
