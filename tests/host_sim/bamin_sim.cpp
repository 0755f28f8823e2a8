// bamin_core.h (what the kernels of the BAM reader run per segment and per record) replayed on the host: the lanes of a workgroup as loops,
// the kernels in launch order, rocPRIM's scans as loops; around it what moni_bam_in_feed does with the carry and the verdict.  The replay
// takes the INFLATED bytes of a call (the inflater has its own replay, inflate_sim.cpp).  The stream, the tables and the texts are sized
// exactly, so a sanitizer build sees any byte touched past them.  As a library (tests/test_host_bamin.py) and, with BAMIN_SIM_MAIN, as a
// stand-alone program for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DBAMIN_SIM_MAIN -o bamin_sim_asan bamin_sim.cpp && ./bamin_sim_asan CASE...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../moni_align_amd/csrc/bamin_core.h"

namespace {

struct Sim {
    uint32_t paired = 0;
    uint64_t group = BAMIN_GROUP;          // segments per sweep launch (the tests take small ones to cross a group's edge)
    std::vector<uint8_t> carry;
    uint64_t rec_base = 0;
    bool header_done = false;
    std::vector<uint8_t> text1, text2;
};

void scan(const std::vector<uint64_t>& in, std::vector<uint64_t>& out) {
    uint64_t s = 0;
    for (size_t i = 0; i < in.size(); ++i) { out[i] = s; s += in[i]; }
}

}  // namespace

extern "C" {

void* baminsim_create(uint32_t paired, uint64_t group) {
    Sim* s = new Sim;
    s->paired = paired;
    if (group) s->group = group;
    return s;
}
void baminsim_destroy(void* h) { delete static_cast<Sim*>(h); }
void baminsim_reset(void* h) { Sim* s = static_cast<Sim*>(h); s->carry.clear(); s->rec_base = 0; s->header_done = false; }
uint32_t baminsim_segment(void) { return BAMIN_S; }

// stats: records, reads, skipped_secondary, skipped_empty, carried_bytes, bad_records, first_bad_record, bad_record_reason, header_done.
// MONI_OK / MONI_EINVAL as moni_bam_in_feed gives them; the texts stay valid until the next call on this replay.
int baminsim_feed(void* h, const uint8_t* data, uint64_t len, int last, const uint8_t** text1, uint64_t* len1, const uint8_t** text2, uint64_t* len2,
                  uint64_t* n_reads, uint64_t* stats) {
    if (!h || !text1 || !len1 || !text2 || !len2 || !n_reads || !stats || last < 0 || last > 1 || (!data && len)) return MONI_EINVAL;
    Sim& S = *static_cast<Sim*>(h);
    for (int i = 0; i < 9; ++i) stats[i] = 0;
    stats[4] = S.carry.size(); stats[8] = S.header_done ? 1 : 0;
    *text1 = *text2 = nullptr; *len1 = *len2 = *n_reads = 0;
    if (!len && !last) return MONI_OK;
    const uint64_t N = S.carry.size() + len;
    std::unique_ptr<uint8_t[]> stream(new uint8_t[N ? N : 1]);          // exactly N bytes, at an address that is a multiple of 4
    if (!S.carry.empty()) memcpy(stream.get(), S.carry.data(), S.carry.size());
    if (len) memcpy(stream.get() + S.carry.size(), data, len);

    bamin_state_t H;
    memset(&H, 0, sizeof H);
    H.pending = S.header_done ? 0ull : BAMIN_END; H.carry_off = N; H.bad = ~0ull; H.rec_base = S.rec_base; H.lone_rec = ~0ull; H.header_done = S.header_done ? 1u : 0u;
    bamin_args_t G;
    memset(&G, 0, sizeof G);
    uint64_t n_rec = 0;
    std::vector<uint32_t> entry, slots, seg_bad, rec_off, kept_off;
    std::vector<uint64_t> cnt, pos, cls, cls_x, l1, l2, l1_x, l2_x;
    if (N) {
        const uint64_t n_seg = (N + BAMIN_S - 1u) / BAMIN_S, group = n_seg < S.group ? n_seg : S.group;
        std::vector<uint16_t> table(group * BAMIN_S);
        std::unique_ptr<uint16_t[]> lds(new uint16_t[BAMIN_S]);
        entry.assign(n_seg, 0xDEADBEEFu); slots.resize(n_seg * BAMIN_SLOTS); seg_bad.resize(n_seg); cnt.resize(n_seg + 1); pos.resize(n_seg + 1);
        rec_off.resize(N / BAM_FIXED + 2);
        G.s = stream.get(); G.n = N; G.st = &H; G.table = table.data(); G.entry = entry.data(); G.n_seg = n_seg; G.slots = slots.data(); G.cnt = cnt.data();
        G.seg_bad = seg_bad.data(); G.pos = pos.data(); G.rec_off = rec_off.data(); G.paired = S.paired;
        for (uint64_t k0 = 0; k0 < n_seg; k0 += S.group) {
            G.k0 = k0; G.k1 = n_seg < k0 + S.group ? n_seg : k0 + S.group;
            for (uint64_t k = G.k0; k < G.k1; ++k) bamin_sweep(G.s, G.n, k, lds.get(), G.table + (k - G.k0) * BAMIN_S);
            if (G.k0 == 0u && !H.header_done) bamin_header(G.s, G.n, &H);
            bamin_chain(G);
            for (uint64_t k = G.k0; k < G.k1; ++k) bamin_list(G, k);
        }
        scan(cnt, pos);
        for (uint64_t k = 0; k < n_seg; ++k)
            for (uint32_t i = 0; i < BAMIN_SLOTS; ++i) bamin_compact(G, k, i);
        n_rec = pos[n_seg];
    }
    if (n_rec) {
        cls.resize(n_rec + 1); cls_x.resize(n_rec + 1); l1.resize(n_rec + 1); l1_x.resize(n_rec + 1);
        if (S.paired) { l2.resize(n_rec + 1); l2_x.resize(n_rec + 1); kept_off.resize(n_rec + 1); }
        G.n_rec = n_rec; G.cls = cls.data(); G.cls_x = cls_x.data(); G.len1 = l1.data(); G.len2 = l2.data(); G.len1_x = l1_x.data(); G.len2_x = l2_x.data();
        G.kept_off = kept_off.data();
        for (uint64_t r = 0; r <= n_rec; ++r) bamin_select(G, r);
        scan(cls, cls_x);
        if (S.paired)
            for (uint64_t r = 0; r <= n_rec; ++r) bamin_rank(G, r);
        scan(l1, l1_x);
        if (S.paired) scan(l2, l2_x);
        bamin_summary(G);
        S.text1.assign(H.len1, 0xEE); S.text2.assign(H.len2, 0xEE);
        S.text1.shrink_to_fit(); S.text2.shrink_to_fit();
        G.text1 = S.text1.data(); G.text2 = S.text2.data();
        if (H.len1 + H.len2)
            for (uint64_t r = 0; r < n_rec; ++r) bamin_fastq(G, r);
    } else { S.text1.clear(); S.text2.clear(); }
    const uint64_t left = N - H.carry_off;
    if (H.bad == ~0ull && last && left) H.bad = (S.rec_base + H.seen) << 8 | MONI_BAMIN_TRUNCATED;
    if (H.bad != ~0ull) { stats[5] = 1; stats[6] = H.bad >> 8; stats[7] = H.bad & 255u; return MONI_EINVAL; }
    S.carry.assign(stream.get() + H.carry_off, stream.get() + N);
    S.rec_base += H.seen; S.header_done = H.header_done != 0u;
    stats[0] = H.seen; stats[1] = H.kept; stats[2] = H.skipped_sec; stats[3] = H.skipped_empty; stats[4] = left; stats[8] = H.header_done;
    *text1 = S.text1.data(); *len1 = H.len1; *n_reads = S.paired ? H.kept / 2u : H.kept;
    if (S.paired) { *text2 = S.text2.data(); *len2 = H.len2; }
    return MONI_OK;
}

}  // extern "C"

#ifdef BAMIN_SIM_MAIN
typedef std::vector<uint8_t> bytes_t;

static bool slurp(const std::string& path, bytes_t& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

// CASE: the inflated stream; CASE.meta: "paired chunk group rc index reason" - the stream is fed `chunk` bytes a call (0: all at once), the
// last call with last set; rc 0: CASE.t1 / CASE.t2 hold the texts of all calls; rc -22: the call that fails names record `index`, `reason`.
int main(int argc, char** argv) {
    int bad = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string name = argv[i];
        bytes_t raw, w1, w2, t1, t2;
        unsigned paired = 0;
        unsigned long long chunk = 0, group = 0, index = 0;
        int rc_want = 0;
        unsigned reason = 0;
        FILE* m = fopen((name + ".meta").c_str(), "r");
        if (!slurp(name, raw) || !m || fscanf(m, "%u %llu %llu %d %llu %u", &paired, &chunk, &group, &rc_want, &index, &reason) != 6) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        fclose(m);
        slurp(name + ".t1", w1); slurp(name + ".t2", w2);
        void* h = baminsim_create(paired, group);
        if (!chunk) chunk = raw.size() ? raw.size() : 1;
        int rc = 0;
        uint64_t st[9] = {0};
        for (uint64_t at = 0; rc == 0 && (at < raw.size() || at == 0); at += chunk) {
            const uint64_t n = raw.size() - at < chunk ? raw.size() - at : chunk;
            const bytes_t piece(raw.begin() + at, raw.begin() + at + n);          // exactly n bytes
            const uint8_t *p1, *p2;
            uint64_t n1, n2, nr;
            rc = baminsim_feed(h, piece.data(), n, at + n >= raw.size(), &p1, &n1, &p2, &n2, &nr, st);
            if (rc == 0) { t1.insert(t1.end(), p1, p1 + n1); t2.insert(t2.end(), p2, p2 + n2); }
        }
        baminsim_destroy(h);
        const bool ok = rc == rc_want && (rc ? st[6] == index && st[7] == reason : t1 == w1 && t2 == w2);
        if (!ok) { ++bad; printf("%s: rc %d (want %d), record %llu reason %llu (want %llu, %u), %zu + %zu bytes (want %zu + %zu)  FAILED\n", argv[i], rc, rc_want, (unsigned long long)st[6], (unsigned long long)st[7], index, reason, t1.size(), t2.size(), w1.size(), w2.size()); }
    }
    printf("%d case(s), %d failed\n", argc - 1, bad);
    return bad ? 1 : 0;
}
#endif
