// bam_sort_core.h (what the kernels of the coordinate sort run per record) replayed on the host: the lanes of a wavefront as loops, the passes in
// launch order - keys and checks, the sort of (key, record index) over the key's live bits, the placement and its scan, the gather with the
// index entries.  The records go through the key pass and the gather LAST TO FIRST, so a later bad record is met before an earlier one: the
// first index is a minimum, as on the device.  The records and the output are sized exactly, so a sanitizer build sees any byte read or
// written past them.
// As a library (tests/test_host_bamsort.py) and, with BAMSORT_SIM_MAIN, as a stand-alone program for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DBAMSORT_SIM_MAIN -o bamsort_sim_asan bamsort_sim.cpp && ./bamsort_sim_asan
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "../../moni_align_amd/csrc/bam_sort_core.h"
#include "../../moni_align_amd/csrc/bam_index.hpp"

extern "C" {

// rec[0, len) with off[0, n] -> out (room for len bytes), keys[n], out_off[n + 1], ents[n], all in sorted order.
// stats: bad records, the first bad record, its reason.  MONI_OK or MONI_EINVAL (a bad record: nothing is written).
int bamsortsim_sort(uint32_t n_ref, const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t* keys, uint64_t* out_off,
                    moni_bam_ent_t* ents, uint64_t* stats) {
    if (!stats || (!rec && len) || !off) return MONI_EINVAL;
    stats[0] = stats[1] = stats[2] = 0;
    std::unique_ptr<uint8_t[]> r(new uint8_t[len ? len : 1]);          // exactly len bytes, at a multiple of 16 as the device's buffers are
    if (len) memcpy(r.get(), rec, len);
    std::vector<uint64_t> key(n);
    std::vector<bam_pre_t> pre(n);
    uint64_t bad = 0, first = ~0ull;
    for (uint64_t i = n; i-- > 0;) {
        const uint32_t why = bam_reckey(r.get(), len, off, i, n_ref, key[i], pre[i]);
        if (why) { ++bad; first = std::min(first, i << 8 | why); }
    }
    if (bad) { stats[0] = bad; stats[1] = first >> 8; stats[2] = first & 0xFFu; return MONI_EINVAL; }
    const uint32_t bits = bam_key_bits(n_ref);
    const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1u;
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return (key[a] & mask) < (key[b] & mask); });
    std::vector<uint64_t> place(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) place[i + 1] = place[i] + (off[perm[i] + 1u] - off[perm[i]]);
    const uint64_t total = place[n];
    std::unique_ptr<uint8_t[]> o(new uint8_t[total ? total : 1]);
    memset(o.get(), 0xAA, total);
    for (uint64_t i = n; i-- > 0;) {
        const uint32_t p = perm[i];
        bam_gather(r.get() + off[p], o.get() + place[i], off[p + 1u] - off[p]);
        moni_bam_ent_t e;
        e.ref_id = pre[p].ref_id; e.pos = pre[p].pos; e.end = pre[p].end; e.bin_flag = pre[p].bin_flag; e.off = place[i];
        ents[i] = e;
        keys[i] = key[p];
    }
    memcpy(out, o.get(), total);
    memcpy(out_off, place.data(), (n + 1) * sizeof(uint64_t));
    return MONI_OK;
}

// n bytes from src + sphase to dst + dphase, both buffers sized exactly; returns 0 when the bytes arrived and nothing around them changed
int bamsortsim_gather(const uint8_t* bytes, uint64_t n, uint32_t sphase, uint32_t dphase) {
    std::unique_ptr<uint8_t[]> s(new uint8_t[sphase + n]), d(new uint8_t[dphase + n]);
    memset(s.get(), 0x55, sphase);
    memcpy(s.get() + sphase, bytes, n);
    memset(d.get(), 0xAA, dphase + n);
    bam_gather(s.get() + sphase, d.get() + dphase, n);
    for (uint32_t k = 0; k < dphase; ++k)
        if (d[k] != 0xAA) return 1;
    return memcmp(d.get() + dphase, bytes, n) ? 2 : 0;
}

uint32_t bamsortsim_key_bits(uint32_t n_ref) { return bam_key_bits(n_ref); }

}  // extern "C"

#ifdef BAMSORT_SIM_MAIN
// a record of `size` bytes (at least 36 + l_name + 4 * ops): fixed fields, a name, CIGAR ops of 3M, filler
static std::vector<uint8_t> record(int32_t ref, int32_t pos, uint32_t flag, uint32_t l_name, uint32_t n_ops, uint32_t size, uint32_t seed) {
    std::vector<uint8_t> r(size);
    n_ops = std::min(n_ops, (size - 36u - l_name) / 4u);          // the smallest record has room for a name alone
    for (uint32_t k = 0; k < size; ++k) r[k] = (uint8_t)(seed * 131u + k * 7u);
    bam_put32(r.data(), size - 4u); bam_put32(r.data() + 4, (uint32_t)ref); bam_put32(r.data() + 8, (uint32_t)pos);
    r[12] = (uint8_t)l_name; r[13] = 0;
    bam_put16(r.data() + 14, bam_reg2bin(pos, (int64_t)pos + (n_ops ? 3 * n_ops : 1)) & 0xFFFFu);
    bam_put16(r.data() + 16, n_ops); bam_put16(r.data() + 18, flag);
    for (uint32_t k = 0; k < n_ops; ++k) bam_put32(r.data() + 36 + l_name + 4 * k, 3u << 4 | 0u);
    return r;
}

struct Batch { std::vector<uint8_t> rec; std::vector<uint64_t> off{0}; void add(const std::vector<uint8_t>& r) { rec.insert(rec.end(), r.begin(), r.end()); off.push_back(rec.size()); } };

// the replay against a sort written without it: keys from the fields, std::stable_sort, memcpy
static int run_case(const char* what, uint32_t n_ref, const Batch& b, uint32_t want_reason, uint64_t want_first) {
    const uint64_t n = b.off.size() - 1, len = b.rec.size();
    std::vector<uint8_t> out(len ? len : 1);          // exactly the size
    std::vector<uint64_t> keys(n + 1), oo(n + 1), st(3);
    std::vector<moni_bam_ent_t> ents(n + 1);
    const int rc = bamsortsim_sort(n_ref, b.rec.data(), len, b.off.data(), n, out.data(), keys.data(), oo.data(), ents.data(), st.data());
    bool ok;
    if (want_reason) ok = rc == MONI_EINVAL && st[2] == want_reason && st[1] == want_first;
    else {
        std::vector<uint32_t> p(n);
        std::iota(p.begin(), p.end(), 0u);
        auto key = [&](uint32_t i) {
            const uint8_t* r = b.rec.data() + b.off[i];
            int32_t ref, pos; uint16_t flag;
            memcpy(&ref, r + 4, 4); memcpy(&pos, r + 8, 4); memcpy(&flag, r + 18, 2);
            return (uint64_t)(ref < 0 ? n_ref : (uint32_t)ref) << 33 | (uint64_t)(uint32_t)(pos + 1) << 1 | (flag >> 4 & 1u);
        };
        std::stable_sort(p.begin(), p.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
        std::vector<uint8_t> want;
        for (uint32_t i : p) want.insert(want.end(), b.rec.begin() + b.off[i], b.rec.begin() + b.off[i + 1]);
        ok = rc == MONI_OK && oo[n] == len && (!len || !memcmp(want.data(), out.data(), len));
        for (uint64_t i = 0; ok && i < n; ++i) ok = keys[i] == key(p[i]) && ents[i].off == oo[i];
    }
    printf("%-34s %6llu records %8llu bytes -> rc %d, %llu bad (first %llu, reason %llu)  %s\n", what, (unsigned long long)n, (unsigned long long)len, rc,
           (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    const uint32_t sizes[] = {40, 63, 64, 65, 127, 129, 1140};
    for (uint64_t n : {0, 1, 2, 63, 64, 65, 257}) {
        Batch b;
        for (uint64_t i = 0; i < n; ++i) b.add(record((int32_t)(i % 3) - 1, (int32_t)((i * 7919u) % 1000u) - 1, (i & 1) ? 16u : 0u, 2, 1, sizes[i % 7], (uint32_t)i));
        bad += run_case("record counts", 2, b, 0, 0);
    }
    {   // every phase of source and destination, every size class
        std::vector<uint8_t> bytes(1140);
        for (size_t k = 0; k < bytes.size(); ++k) bytes[k] = (uint8_t)(k * 13u + 1u);
        int g = 0;
        for (uint32_t sz : sizes)
            for (uint32_t sp = 0; sp < 16; ++sp)
                for (uint32_t dp = 0; dp < 16; ++dp) g += bamsortsim_gather(bytes.data(), sz, sp, dp) != 0;
        for (uint32_t sz = 0; sz < 40; ++sz)
            for (uint32_t ph = 0; ph < 16; ++ph) g += bamsortsim_gather(bytes.data(), sz, ph, 15u - ph) != 0;
        printf("%-34s %d failed\n", "gather phases", g);
        bad += g;
    }
    {   // keys: all equal; both strands at one position; pos -1 placed; pos 2^31 - 2; unplaced between placed; 300 references; sorted and reversed
        Batch eq, strands, edge, many, fwd, rev;
        for (uint32_t i = 0; i < 70; ++i) eq.add(record(0, 5, 0, 3, 0, 40 + i, i));
        for (uint32_t i = 0; i < 70; ++i) strands.add(record(0, 5, (i % 3) ? 16u : 0u, 3, 2, 60 + i, i));
        const int32_t pos[] = {-1, 2147483646, 0, 16383, -1, 7};
        for (uint32_t i = 0; i < 60; ++i) edge.add(record((i % 4 == 1) ? -1 : 0, pos[i % 6], 0, 1, (i % 6 == 1) ? 0 : 70, 360 + i, i));
        for (uint32_t i = 0; i < 600; ++i) many.add(record((int32_t)((i * 131u) % 300u), (int32_t)(i % 5u), 0, 2, 1, 50 + i % 40, i));
        for (uint32_t i = 0; i < 130; ++i) { fwd.add(record(0, (int32_t)i, 0, 2, 1, 48 + i % 9, i)); rev.add(record(0, 129 - (int32_t)i, 0, 2, 1, 48 + i % 9, i)); }
        bad += run_case("all keys equal", 1, eq, 0, 0) + run_case("both strands", 1, strands, 0, 0) + run_case("edge positions, unplaced", 1, edge, 0, 0) +
               run_case("300 references", 300, many, 0, 0) + run_case("sorted", 1, fwd, 0, 0) + run_case("reversed", 1, rev, 0, 0);
    }
    {   // bad records: every class at record 3 of 8, and a later one that is met first
        for (uint32_t why = MONI_BAMSORT_OFFSET; why <= MONI_BAMSORT_POS; ++why) {
            Batch b;
            for (uint32_t i = 0; i < 8; ++i) b.add(record(0, (int32_t)i, 0, 2, 1, 48, i));
            for (uint64_t at : {(uint64_t)3, (uint64_t)6}) {
                uint8_t* r = b.rec.data() + b.off[at];
                switch (why) {
                    case MONI_BAMSORT_OFFSET: b.off[at + 1] = b.off[at]; break;
                    case MONI_BAMSORT_SHORT: bam_put16(r + 16, 9); break;
                    case MONI_BAMSORT_SIZE: bam_put32(r, 45); break;
                    case MONI_BAMSORT_NAME: r[12] = 0; break;
                    case MONI_BAMSORT_REF: bam_put32(r + 4, 1); break;
                    default: bam_put32(r + 8, 0x7FFFFFFFu); break;
                }
            }
            // an offset that does not increase spoils the record behind it too (its size no longer fits): the first is still record 3
            bad += run_case("bad record", 1, b, why, 3);
        }
    }
    {   // the plan and the index on the replay's own entries
        Batch b;
        for (uint32_t i = 0; i < 500; ++i) b.add(record((int32_t)(i % 3) - 1, (int32_t)((i * 7919u) % 70000u), 0, 2, 1, 300 + i % 100, i));
        const uint64_t n = 500, len = b.rec.size();
        std::vector<uint8_t> out(len);
        std::vector<uint64_t> keys(n), oo(n + 1), st(3);
        std::vector<moni_bam_ent_t> ents(n);
        int rc = bamsortsim_sort(2, b.rec.data(), len, b.off.data(), n, out.data(), keys.data(), oo.data(), ents.data(), st.data());
        const uint64_t* kp[2] = {keys.data(), keys.data()};
        const uint64_t* op[2] = {oo.data(), oo.data()};
        const uint64_t nn[2] = {n, n};
        std::vector<uint64_t> cuts;
        rc = rc ? rc : bam_merge_plan(kp, nn, op, 2, 4096, cuts);
        bool ok = rc == MONI_OK && cuts.size() % 2 == 0 && cuts[cuts.size() - 1] == n && cuts[cuts.size() - 2] == n;
        moni_bai B;
        B.refs.resize(2);
        std::vector<uint32_t> cs((len + 999) / 1000, 100u);
        const uint8_t* bytes; uint64_t bl;
        ok = ok && bai_add(&B, ents.data(), n, len, 1000, cs.data(), cs.size(), 50) == MONI_OK && bai_finish(&B, 50 + 100 * cs.size(), &bytes, &bl) == MONI_OK && bl > 16;
        printf("%-34s %zu chunks, %llu bytes of index  %s\n", "plan and index", cuts.size() / 2 - 1, (unsigned long long)bl, ok ? "ok" : "FAILED");
        bad += !ok;
    }
    printf("%d case(s) failed\n", bad);
    return bad ? 1 : 0;
}
#endif
