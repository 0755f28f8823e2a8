// bam_dup_core.h (what the kernels of duplicate marking run per record, unit and entry) replayed on the host: the lanes of a wavefront as loops,
// the passes in launch order - for a run the key pass and the sort of bam_sort_core.h, the signatures, the inverse of the permutation, the
// units' counts, their scan, the entries; for the resolve the preparation, the stable sorts least significant key first, the two flag passes.
// Every pass takes its elements LAST TO FIRST, so a later bad record is met before an earlier one: the first index is a minimum, as on the
// device.  The records are sized exactly, so a sanitizer build sees any byte read or written past them.
// As a library (tests/test_host_markdup.py) and, with MARKDUP_SIM_MAIN, as a stand-alone program for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DMARKDUP_SIM_MAIN -o markdup_sim_asan markdup_sim.cpp && ./markdup_sim_asan
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <set>
#include <tuple>
#include <vector>

#include "../../moni_align_amd/csrc/bam_dup_core.h"

static void stable_by(std::vector<uint32_t>& perm, const std::vector<uint64_t>& key, uint32_t bits) {
    const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1u;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return (key[a] & mask) < (key[b] & mask); });
}

extern "C" {

// One run: rec[0, len) with off[0, n] -> ents (room for n), *n_ent.  stats: bad records, the first bad record, its reason.
// MONI_OK or MONI_EINVAL (a bad record of the sort's checks or of SEQ, CLIP, MATE: nothing is written).
int markdupsim_run(uint32_t n_ref, const uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, uint32_t paired, moni_bam_dup_t* ents, uint64_t* n_ent,
                   uint64_t* stats) {
    if (!stats || !n_ent || (!rec && len) || !off || paired > 1u) return MONI_EINVAL;
    stats[0] = stats[1] = stats[2] = 0; *n_ent = 0;
    std::unique_ptr<uint8_t[]> r(new uint8_t[len ? len : 1]);          // exactly len bytes
    if (len) memcpy(r.get(), rec, len);
    std::vector<uint64_t> key(n);
    uint64_t bad = 0, first = ~0ull;
    for (uint64_t i = n; i-- > 0;) {
        bam_pre_t pre;
        const uint32_t why = bam_reckey(r.get(), len, off, i, n_ref, key[i], pre);
        if (why) { ++bad; first = std::min(first, i << 8 | why); }
    }
    if (bad) { stats[0] = bad; stats[1] = first >> 8; stats[2] = first & 0xFFu; return MONI_EINVAL; }
    std::vector<uint32_t> perm(n), where(n);
    std::iota(perm.begin(), perm.end(), 0u);
    stable_by(perm, key, bam_key_bits(n_ref));
    std::vector<bam_dupsig_t> sig(n);
    for (uint64_t i = n; i-- > 0;) {
        const uint32_t why = bam_dupsig(r.get() + off[i], off[i + 1] - off[i], n_ref, sig[i]);
        if (why) { ++bad; first = std::min(first, i << 8 | why); }
    }
    for (uint64_t i = n; i-- > 0;) where[perm[i]] = (uint32_t)i;
    const uint64_t n_units = paired ? (n + 1) / 2 : n;
    std::vector<uint64_t> cnt(n_units + 1, 0), pos(n_units + 1, 0);
    for (uint64_t u = n_units; u-- > 0;) {
        moni_bam_dup_t d0, d1; uint32_t has0 = 0, has1 = 0; uint64_t at = 0;
        const uint32_t why = bam_dupunit(r.get(), off, sig.data(), where.data(), n, u, paired, has0, d0, has1, d1, at);
        cnt[u] = has0 + has1;
        if (why) { ++bad; first = std::min(first, at << 8 | why); }
    }
    if (bad) { stats[0] = bad; stats[1] = first >> 8; stats[2] = first & 0xFFu; return MONI_EINVAL; }
    for (uint64_t u = 0; u < n_units; ++u) pos[u + 1] = pos[u] + cnt[u];
    std::vector<moni_bam_dup_t> out(pos[n_units]);          // exactly the entries
    for (uint64_t u = n_units; u-- > 0;) {
        moni_bam_dup_t d0, d1; uint32_t has0 = 0, has1 = 0; uint64_t at = 0;
        bam_dupunit(r.get(), off, sig.data(), where.data(), n, u, paired, has0, d0, has1, d1, at);
        if (has0) out[pos[u]] = d0;
        if (has1) out[pos[u] + has0] = d1;
    }
    if (!out.empty()) memcpy(ents, out.data(), out.size() * sizeof(moni_bam_dup_t));
    *n_ent = out.size();
    return MONI_OK;
}

// All entries of all runs, one behind the other (n_dups[r] of run r, which has n_records[r] records) -> marks, the runs' one behind the other.
// stats: bad entries, the first, pairs, duplicate pairs, fragments, duplicate fragments.  MONI_EINVAL: an idx outside its run, nothing written.
int markdupsim_resolve(uint32_t n_ref, const moni_bam_dup_t* all, const uint64_t* n_dups, const uint64_t* n_records, uint64_t n_runs, uint8_t* marks, uint64_t* stats) {
    if (!stats || (n_runs && (!n_dups || !n_records))) return MONI_EINVAL;
    for (int k = 0; k < 6; ++k) stats[k] = 0;
    std::vector<uint64_t> eb(n_runs + 1, 0), rb(n_runs + 1, 0);
    for (uint64_t r = 0; r < n_runs; ++r) { eb[r + 1] = eb[r] + n_dups[r]; rb[r + 1] = rb[r] + n_records[r]; }
    const uint64_t N = eb[n_runs], M = rb[n_runs];
    std::vector<moni_bam_dup_t> ent(all, all + N);          // exactly N entries
    std::vector<uint32_t> at(2 * N);
    std::vector<uint64_t> pkey(N), ekey(2 * N), key(2 * N);
    uint64_t bad = 0, first = ~0ull;
    for (uint64_t j = N; j-- > 0;) {
        if (!bam_dupprep(ent.data(), eb.data(), rb.data(), n_runs, j, at.data(), pkey.data(), ekey.data())) { ++bad; first = std::min(first, j); }
        ++stats[ent[j].kind ? 2 : 4];
    }
    if (bad) { stats[0] = bad; stats[1] = first; return MONI_EINVAL; }
    std::vector<uint8_t> m(M, 0);          // exactly M marks
    const uint32_t ebits = bam_dup_bits(n_ref);
    std::vector<uint32_t> perm(N);
    std::iota(perm.begin(), perm.end(), 0u);
    stable_by(perm, pkey, 34);
    for (uint64_t j = 0; j < N; ++j) key[j] = ent[j].k2;
    stable_by(perm, key, ebits);
    for (uint64_t j = 0; j < N; ++j) key[j] = ent[j].k1;
    stable_by(perm, key, ebits);
    for (uint64_t i = N; i-- > 0;)
        if (bam_duppair(ent.data(), perm.data(), i)) { m[at[2 * perm[i]]] = 1; m[at[2 * perm[i] + 1]] = 1; ++stats[3]; }
    perm.resize(2 * N);
    std::iota(perm.begin(), perm.end(), 0u);
    stable_by(perm, ekey, 34);
    for (uint64_t s = 0; s < 2 * N; ++s) key[s] = bam_dup_end(ent.data(), (uint32_t)s);
    stable_by(perm, key, ebits);
    for (uint64_t i = 2 * N; i-- > 0;)
        if (bam_dupend(ent.data(), perm.data(), i)) { m[at[perm[i]]] = 1; ++stats[5]; }
    if (M) memcpy(marks, m.data(), M);
    return MONI_OK;
}

// the flag pass of moni_bam_sort_marked on rec[0, len), in place (the caller's buffer is exactly len bytes)
void markdupsim_setdup(uint8_t* rec, uint64_t len, const uint64_t* off, uint64_t n, const uint8_t* marks) {
    for (uint64_t i = n; i-- > 0;) bam_setdup(rec, len, off, i, marks);
}

uint32_t markdupsim_bits(uint32_t n_ref) { return bam_dup_bits(n_ref); }

}  // extern "C"

#ifdef MARKDUP_SIM_MAIN
// a record: fixed fields, a name, the CIGAR, SEQ, QUAL of one value (or 14 and 15 alternating with q = 1), and `extra` bytes of tags
static std::vector<uint8_t> record(int32_t ref, int32_t pos, uint32_t flag, const char* name, const std::vector<uint32_t>& ops, uint32_t l_seq, uint8_t q, uint32_t extra = 0) {
    const uint32_t l_name = (uint32_t)strlen(name) + 1u;
    const uint32_t size = 36u + l_name + 4u * (uint32_t)ops.size() + (l_seq + 1u) / 2u + l_seq + extra;
    std::vector<uint8_t> r(size, 0x11);
    uint64_t reflen = 0;
    for (uint32_t v : ops) if ((0x18Du >> (v & 15u)) & 1u) reflen += v >> 4;
    bam_put32(r.data(), size - 4u); bam_put32(r.data() + 4, (uint32_t)ref); bam_put32(r.data() + 8, (uint32_t)pos);
    r[12] = (uint8_t)l_name; r[13] = 30;
    bam_put16(r.data() + 14, bam_reg2bin(pos, (int64_t)pos + (int64_t)(reflen ? reflen : 1)) & 0xFFFFu);
    bam_put16(r.data() + 16, (uint32_t)ops.size()); bam_put16(r.data() + 18, flag); bam_put32(r.data() + 20, l_seq);
    memcpy(r.data() + 36, name, l_name);
    for (size_t k = 0; k < ops.size(); ++k) bam_put32(r.data() + 36 + l_name + 4 * k, ops[k]);
    uint8_t* qual = r.data() + 36 + l_name + 4 * ops.size() + (l_seq + 1u) / 2u;
    for (uint32_t j = 0; j < l_seq; ++j) qual[j] = q == 1 ? (uint8_t)(14 + (j & 1u)) : q;
    return r;
}
static uint32_t op(uint32_t n, char c) { return n << 4 | bam_cigar_op((uint8_t)c); }

struct Batch { std::vector<uint8_t> rec; std::vector<uint64_t> off{0}; void add(const std::vector<uint8_t>& r) { rec.insert(rec.end(), r.begin(), r.end()); off.push_back(rec.size()); } };

// the rule once more, with maps in place of sorts: the duplicates among `runs` (entries as the replay made them)
static std::vector<std::vector<uint8_t>> brute(const std::vector<std::vector<moni_bam_dup_t>>& runs, const std::vector<uint64_t>& n_rec) {
    std::vector<std::vector<uint8_t>> m;
    for (uint64_t n : n_rec) m.emplace_back(n, 0);
    typedef std::tuple<uint64_t, uint64_t, uint32_t> PK;
    std::map<PK, std::vector<std::tuple<int64_t, size_t, size_t>>> pairs;
    std::map<uint64_t, std::vector<std::tuple<int64_t, size_t, size_t>>> frags;
    std::set<uint64_t> pe;
    for (size_t r = 0; r < runs.size(); ++r)
        for (size_t k = 0; k < runs[r].size(); ++k) {
            const moni_bam_dup_t& d = runs[r][k];
            if (d.kind) { pairs[PK(d.k1, d.k2, d.kind)].emplace_back(-(int64_t)d.score, r, k); pe.insert(d.k1); pe.insert(d.k2); }
            else frags[d.k1].emplace_back(-(int64_t)d.score, r, k);
        }
    for (auto& g : pairs) {
        std::sort(g.second.begin(), g.second.end());
        for (size_t x = 1; x < g.second.size(); ++x) { const moni_bam_dup_t& d = runs[std::get<1>(g.second[x])][std::get<2>(g.second[x])]; m[std::get<1>(g.second[x])][d.idx[0]] = 1; m[std::get<1>(g.second[x])][d.idx[1]] = 1; }
    }
    for (auto& g : frags) {
        std::sort(g.second.begin(), g.second.end());
        for (size_t x = pe.count(g.first) ? 0 : 1; x < g.second.size(); ++x) m[std::get<1>(g.second[x])][runs[std::get<1>(g.second[x])][std::get<2>(g.second[x])].idx[0]] = 1;
    }
    return m;
}

static int run_case(const char* what, const std::vector<Batch>& runs, uint32_t paired, uint32_t want_reason, uint64_t want_first, int64_t want_marked) {
    std::vector<std::vector<moni_bam_dup_t>> ents;
    std::vector<uint64_t> n_rec, n_dups;
    std::vector<moni_bam_dup_t> all;
    bool ok = true;
    uint64_t st[6] = {0, 0, 0, 0, 0, 0};
    int rc = MONI_OK;
    for (const Batch& b : runs) {
        const uint64_t n = b.off.size() - 1;
        std::vector<moni_bam_dup_t> e(n + 1);
        uint64_t k = 0;
        rc = markdupsim_run(1, b.rec.data(), b.rec.size(), b.off.data(), n, paired, e.data(), &k, st);
        if (want_reason) { ok = rc == MONI_EINVAL && st[2] == want_reason && st[1] == want_first; st[2] = st[3] = st[4] = st[5] = 0; break; }
        ok = ok && rc == MONI_OK;
        e.resize(k);
        ents.push_back(e); n_rec.push_back(n); n_dups.push_back(k);
        all.insert(all.end(), e.begin(), e.end());
    }
    uint64_t marked = 0;
    if (!want_reason && ok) {
        uint64_t M = 0;
        for (uint64_t n : n_rec) M += n;
        std::vector<uint8_t> marks(M ? M : 1, 0xEE);          // exactly the marks
        rc = markdupsim_resolve(1, all.data(), n_dups.data(), n_rec.data(), runs.size(), marks.data(), st);
        const auto want = brute(ents, n_rec);
        ok = rc == MONI_OK;
        uint64_t at = 0;
        for (size_t r = 0; ok && r < runs.size(); ++r) { ok = !n_rec[r] || !memcmp(want[r].data(), marks.data() + at, n_rec[r]); at += n_rec[r]; }
        for (uint64_t i = 0; i < M; ++i) marked += marks[i] == 1;
        ok = ok && marked == 2 * st[3] + st[5] && (want_marked < 0 || (uint64_t)want_marked == marked);
    }
    printf("%-40s %zu run(s) -> rc %d, %llu pairs (%llu dup), %llu fragments (%llu dup), %llu marked  %s\n", what, runs.size(), rc, (unsigned long long)st[2],
           (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[5], (unsigned long long)marked, ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    const std::vector<uint32_t> M50 = {op(50, 'M')};
    for (uint64_t n : {0, 1, 2, 63, 64, 65, 257}) {          // units, single and paired; positions from a few so that groups form
        Batch se, pe;
        for (uint64_t i = 0; i < n; ++i) {
            const int32_t pos = (int32_t)((i * 7919u) % 5u) * 10;
            se.add(record(0, pos, (i % 3) ? 0u : 16u, "r", M50, (uint32_t)(i % 70), (uint8_t)(20 + i % 7)));
            const uint32_t f1 = (i % 4 == 3) ? 0x49u : 0x63u, f2 = (i % 4 == 3) ? 0x85u : 0x93u;          // every fourth pair: the second mate unmapped
            pe.add(record(0, pos, f1, "p", M50, 50, 30)); pe.add(record(0, pos + 100, f2, "p", M50, (uint32_t)(i % 66), 30));
        }
        bad += run_case("single units", {se}, 0, 0, 0, -1) + run_case("paired units", {pe}, 1, 0, 0, -1);
    }
    {   // clips on both strands: 5S45M at 105 and 50M at 100 share u5 = 100 forward; 45M5H at 100 and 50M at 100 share 149 reverse
        Batch b;
        b.add(record(0, 105, 0, "a", {op(5, 'S'), op(45, 'M')}, 50, 30)); b.add(record(0, 100, 0, "b", M50, 50, 40));
        b.add(record(0, 100, 16, "c", {op(45, 'M'), op(5, 'H')}, 45, 30)); b.add(record(0, 100, 16, "d", {op(2, 'H'), op(50, 'M')}, 50, 20));
        b.add(record(0, 3, 0, "e", {op(10, 'S'), op(40, 'M')}, 50, 30));          // u5 = -7
        b.add(record(0, 0, 0, "f", {op(4, 'S'), op(3, 'H')}, 4, 30)); b.add(record(0, 0, 0, "g", {}, 0, 30));          // clips only; no ops
        b.add(record(0, 5, 0, "h", M50, 64, 1)); b.add(record(0, 5, 0, "i", M50, 64, 0xFF)); b.add(record(0, 5, 0, "j", M50, 1, 15));
        b.add(record(-1, -1, 4, "u", {}, 300, 30)); b.add(record(0, 5, 0x100, "s", M50, 10, 30)); b.add(record(0, 5, 0x800, "t", M50, 10, 30));
        // duplicates: a (30 * 50 < 40 * 50), d (u5 149, 20 * 50 < 30 * 45), f (u5 0 - 7 = -7 as e, 4 * 30 < 50 * 30), i (0) and j (15) behind h (32 * 15);
        // g (u5 0) stands alone, u, s and t take no part
        bad += run_case("clips, qualities, flags", {b}, 0, 0, 0, 5);
    }
    {   // pairs: FR against RF at the same ends; FF with lo read 1 against read 2; equal scores; a fragment at a pair's end; across runs
        Batch x, y, z;
        auto pair = [&](Batch& b, int32_t p1, uint32_t s1, int32_t p2, uint32_t s2, uint8_t q, const char* nm) {
            b.add(record(0, p1, 0x41u | s1 | (s2 << 1), nm, M50, 50, q)); b.add(record(0, p2, 0x81u | s2 | (s1 << 1), nm, M50, 50, q));
        };
        pair(x, 100, 0, 300, 16, 30, "p0"); pair(x, 100, 0, 300, 16, 30, "p1");          // equal scores: the first stays
        pair(x, 51, 16, 349, 0, 30, "p2");          // RF at the ends of FR: read 1 reverse ending at 100, read 2 forward from 349 - other codes, no duplicate
        pair(x, 100, 0, 400, 0, 30, "p3"); pair(x, 400, 0, 100, 0, 30, "p4");          // FF, lo read 1 against lo read 2: not duplicates
        pair(y, 100, 0, 300, 16, 35, "p5");         // a better copy in the next run: p0 and p1 are the duplicates
        y.add(record(0, 100, 0x49, "p6", M50, 50, 40)); y.add(record(0, 100, 0x85, "p6", {}, 50, 40));          // a fragment at a pair's end
        pair(z, 100, 0, 100, 0, 30, "p7"); pair(z, 100, 0, 100, 0, 31, "p8");          // e1 == e2
        bad += run_case("pairs over three runs", {x, y, Batch(), z}, 1, 0, 0, 7);
        bad += run_case("all runs empty", {Batch(), Batch()}, 1, 0, 0, 0) + run_case("no runs", {}, 1, 0, 0, 0);
    }
    {   // bad records: at record 4 and again at 8 (met first)
        for (int why = 0; why < 5; ++why) {
            Batch b;
            for (uint32_t i = 0; i < 10; ++i) b.add(record(0, (int32_t)i, (i & 1) ? 0x83u : 0x43u, i / 2 % 2 ? "n1" : "n0", M50, 50, 30));
            uint32_t want = 0;
            for (uint64_t at : {(uint64_t)4, (uint64_t)8}) {
                uint8_t* r = b.rec.data() + b.off[at];
                switch (why) {
                    case 0: bam_put32(r + 20, 200); want = MONI_BAMSORT_SEQ; break;
                    case 1: break;          // built below
                    case 2: bam_put16(r + 18, 0x83); want = MONI_BAMSORT_MATE; break;
                    case 3: r[36] = 'x'; want = MONI_BAMSORT_MATE; break;
                    default: want = MONI_BAMSORT_MATE; break;
                }
            }
            if (why == 1) {          // forty H ops of 2^28 - 1 in front of the first M: u5 below -2^31
                Batch c;
                std::vector<uint32_t> ops(40, op((1u << 28) - 1u, 'H'));
                ops.push_back(op(5, 'M'));
                for (uint32_t i = 0; i < 10; ++i) c.add(record(0, 0, (i & 1) ? 0x83u : 0x43u, "n", (i == 4 || i == 8) ? ops : M50, 5, 30));
                bad += run_case("bad record: CLIP", {c}, 1, MONI_BAMSORT_CLIP, 4, 0);
                continue;
            }
            if (why == 4) { b.rec.resize(b.off[9]); b.off.pop_back(); bad += run_case("bad record: odd n", {b}, 1, want, 8, 0); continue; }
            bad += run_case("bad record", {b}, 1, want, 4, 0);
        }
    }
    {   // an idx outside its run
        moni_bam_dup_t d[3] = {{5, 0, 1, 0, {0, BAMDUP_NONE}}, {5, 9, 1, 1, {1, 2}}, {5, 0, 1, 0, {1, 0}}};
        const uint64_t nd[1] = {3}, nr[1] = {2};
        uint8_t marks[2] = {0xEE, 0xEE};
        uint64_t st[6];
        const int rc = markdupsim_resolve(1, d, nd, nr, 1, marks, st);
        const bool ok = rc == MONI_EINVAL && st[0] == 2 && st[1] == 1 && marks[0] == 0xEE && marks[1] == 0xEE;
        printf("%-40s rc %d, %llu bad, first %llu  %s\n", "idx out of range", rc, (unsigned long long)st[0], (unsigned long long)st[1], ok ? "ok" : "FAILED");
        bad += !ok;
    }
    {   // 2000 random units from 50 end codes, in 7 runs
        std::vector<Batch> runs(7);
        uint32_t x = 12345;
        auto rnd = [&](uint32_t m) { x = x * 1664525u + 1013904223u; return (x >> 8) % m; };
        for (uint32_t i = 0; i < 2000; ++i) {
            Batch& b = runs[i * 7 / 2000];
            const int32_t p1 = (int32_t)rnd(7) * 20, p2 = (int32_t)rnd(7) * 20;
            const uint32_t s1 = rnd(2) * 16, s2 = rnd(2) * 16, un = rnd(6) == 0;
            b.add(record(0, p1, 0x41u | s1 | (un ? 8u : s2 << 1), "q", M50, 50, (uint8_t)(20 + rnd(4))));
            b.add(record(0, p2, 0x81u | (un ? 4u : s2) | (s1 << 1), "q", M50, 50, (uint8_t)(20 + rnd(4))));
        }
        bad += run_case("2000 random pairs", runs, 1, 0, 0, -1);
    }
    printf("%d case(s) failed\n", bad);
    return bad ? 1 : 0;
}
#endif
