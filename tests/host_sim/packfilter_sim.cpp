// TEST HARNESS ONLY - not part of the product.  A stand-alone program over moni_align_amd/csrc/packfilter_core.h (the code pack_filter_kernel runs,
// compiled for the host): pack_filter_read, read by read, against pack_task + pf_task_keep of the same tree, task by task, as pack_kernel and
// strand_filter_kernel run them.  Compared: every workspace word that is defined behind the fused kernel (code and mask words of every task, byte
// words of a task that is kept), pflag, flag, cnt_m / cnt_s and the lookup count of every read; and that no word outside a task's own words is touched.
// Built plain and with the address and undefined-behaviour sanitizers by tests/test_host_packfilter.py.  Prints "OK ..." and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../moni_align_amd/csrc/packfilter_core.h"

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }
static const char ACGT[] = "ACGT";

#define FAIL(...) do { fprintf(stderr, "packfilter_sim: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static const uint64_t STALE = 0xDEADBEEFCAFEF00Dull;          // what an earlier batch left in the workspace
static const uint32_t LENS[] = {0, 1, 7, 8, 9, 24, 25, 26, 31, 32, 33, 63, 64, 65, 150, 159, 160, 161, 250, 256, 257};
static const uint32_t N_LENS = sizeof(LENS) / sizeof(LENS[0]);
// kinds of read: 0 A/C/G/T only; N at 1: 0, 2: m-1, 3: 7, 4: 8, 5: 31, 6: 32; 7 a lower-case base; 8 a byte >= 0x80; 9 several of them
static const uint32_t N_KINDS = 10;

static std::vector<uint8_t> make_read(uint32_t m, uint32_t kind) {
    std::vector<uint8_t> r(m);
    for (uint32_t i = 0; i < m; ++i) r[i] = (uint8_t)ACGT[rnd_below(4)];
    auto put = [&](uint32_t at, uint8_t b) { if (at < m) r[at] = b; };
    switch (kind) {
        case 1: put(0, 'N'); break;
        case 2: if (m) put(m - 1, 'N'); break;
        case 3: put(7, 'N'); break;
        case 4: put(8, 'N'); break;
        case 5: put(31, 'N'); break;
        case 6: put(32, 'N'); break;
        case 7: if (m) { const uint32_t at = rnd_below(m); r[at] = (uint8_t)(r[at] | 0x20); } break;
        case 8: if (m) put(rnd_below(m), (uint8_t)(0x80 + rnd_below(128))); break;
        case 9: for (uint32_t j = 0; j < 3 && m; ++j) put(rnd_below(m), j == 0 ? 'N' : j == 1 ? 'g' : (uint8_t)0xC1); break;
        default: break;
    }
    return r;
}

struct Totals { uint64_t reads = 0, tasks = 0, kept = 0, skipped = 0, flagged = 0, plain_long = 0, lookups = 0, words = 0; };

// one batch against one table and one pair (min_len, k), with cw_words code words per strand and lane
static int run_batch(const std::vector<std::vector<uint8_t>>& reads, const lds_tables_t& L, const std::vector<uint32_t>& tab, uint32_t min_len, uint32_t k, uint32_t cw_words, Totals& T) {
    std::vector<uint8_t> seq; std::vector<uint64_t> offs(1, 0);
    for (const auto& r : reads) { seq.insert(seq.end(), r.begin(), r.end()); offs.push_back(seq.size()); }
    const uint64_t n_reads = reads.size(), n_tasks = 2 * n_reads, n_blk = (n_reads + 31) / 32;
    std::vector<moni_u64x2> blk(n_blk + 1);          // the workspace layout of reads_upload
    {
        uint64_t pw = 0, qw = 0;
        for (uint64_t b = 0; b < n_blk; ++b) {
            uint64_t lb = 0;
            for (uint64_t i = 32 * b; i < n_reads && i < 32 * b + 32; ++i) if (offs[i + 1] - offs[i] > lb) lb = offs[i + 1] - offs[i];
            blk[b].x = qw; blk[b].y = pw;
            qw += 64 * lb; pw += 64 * ws_pat_words(lb);
        }
        blk[n_blk].x = qw; blk[n_blk].y = pw;
    }
    std::vector<uint64_t> seq_pad((seq.size() + 16 + 7) / 8 + 1, 0);          // 8-byte aligned, padded by 16 bytes: as the context's buffer
    if (!seq.empty()) memcpy(seq_pad.data(), seq.data(), seq.size());
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    const uint64_t n_pat = blk[n_blk].y;
    // the two kernels
    std::vector<uint64_t> pat_a(n_pat + 1, STALE), flag_a(n_tasks + 1, 9);
    std::vector<uint8_t> pflag_a(n_tasks + 8, 9);
    std::vector<uint32_t> cm_a(n_tasks + 2, 7), cs_a(n_tasks + 2, 7);
    std::vector<unsigned long long> look_a(n_tasks, 0);
    for (uint64_t t = 0; t < n_tasks; ++t) pack_task(L, sq, offs.data(), blk.data(), t, pat_a.data(), pflag_a.data());
    for (uint64_t t = 0; t < n_tasks; ++t) {
        const uint32_t m = (uint32_t)(offs[(t >> 1) + 1] - offs[t >> 1]);
        const uint64_t cb = ws_pat_base(blk.data(), t) + 64u * ((ws_block_len(blk.data(), t) + 7) / 8);
        pf_pat_t P;
        pf_pat_init(P, pat_a.data() + cb, 64u, m);
        const bool keep = pf_task_keep(P, m, min_len, k, pflag_a[t] != 0, tab.data(), look_a[t]);
        flag_a[t] = keep ? 1u : 0u;
        if (!keep) { cm_a[t] = 0; cs_a[t] = 0; }
    }
    // the fused one, a block of 256 lanes at a time over one array of code words, [strand * cw_words + word][lane] as in the kernel
    std::vector<uint64_t> pat_b(n_pat + 1, STALE), flag_b(n_tasks + 1, 9);
    std::vector<uint8_t> pflag_b(n_tasks + 8, 9);
    std::vector<uint32_t> cm_b(n_tasks + 2, 7), cs_b(n_tasks + 2, 7);
    std::vector<uint64_t> cw((size_t)2 * cw_words * 256, STALE);
    for (uint64_t r = 0; r < n_reads; ++r) {
        pk_args_t A;
        A.min_len = min_len; A.k = k; A.tab = tab.data(); A.cw = cw.data() + (r & 255u); A.cw_stride = 256; A.cw_words = cw_words;
        unsigned long long lookups = 0, skipped = 0;
        pack_filter_read(L, A, sq, offs.data(), blk.data(), r, pat_b.data(), pflag_b.data(), flag_b.data(), cm_b.data(), cs_b.data(), lookups, skipped);
        const uint32_t m = (uint32_t)(offs[r + 1] - offs[r]);
        if (lookups != look_a[2 * r] + look_a[2 * r + 1]) FAIL("read %llu (m %u): %llu lookups, the two kernels make %llu + %llu", (unsigned long long)r, m, lookups, look_a[2 * r], look_a[2 * r + 1]);
        if (skipped != (flag_a[2 * r] ? 0u : 1u) + (flag_a[2 * r + 1] ? 0u : 1u)) FAIL("read %llu (m %u): %llu tasks counted as skipped", (unsigned long long)r, m, skipped);
        T.lookups += lookups;
        if (m > 32 * cw_words && !pflag_a[2 * r]) T.plain_long++;
    }
    // every word of the workspace: a task's own, or nobody's
    std::vector<uint8_t> owned(n_pat + 1, 0);
    for (uint64_t t = 0; t < n_tasks; ++t) {
        const uint32_t m = (uint32_t)(offs[(t >> 1) + 1] - offs[t >> 1]);
        const uint64_t pb = ws_pat_base(blk.data(), t), lb = ws_block_len(blk.data(), t);
        const uint64_t cb = pb + 64u * ((lb + 7) / 8), mb = cb + 64u * ((lb + 31) / 32);
        if (pflag_b[t] != pflag_a[t]) FAIL("task %llu (m %u): pflag %u, pack_task gives %u", (unsigned long long)t, m, pflag_b[t], pflag_a[t]);
        if (flag_b[t] != flag_a[t]) FAIL("task %llu (m %u, min_len %u, k %u): flag %llu, pf_task_keep gives %llu", (unsigned long long)t, m, min_len, k, (unsigned long long)flag_b[t], (unsigned long long)flag_a[t]);
        if (cm_b[t] != cm_a[t] || cs_b[t] != cs_a[t]) FAIL("task %llu: cnt_m / cnt_s %u / %u, expected %u / %u", (unsigned long long)t, cm_b[t], cs_b[t], cm_a[t], cs_a[t]);
        for (uint32_t w = 0; w < (m + 31) / 32; ++w) {
            owned[cb + 64ull * w] = owned[mb + 64ull * w] = 1;
            if (pat_b[cb + 64ull * w] != pat_a[cb + 64ull * w]) FAIL("task %llu (m %u): code word %u is %016llx, pack_task gives %016llx", (unsigned long long)t, m, w, (unsigned long long)pat_b[cb + 64ull * w], (unsigned long long)pat_a[cb + 64ull * w]);
            if (pat_b[mb + 64ull * w] != pat_a[mb + 64ull * w]) FAIL("task %llu (m %u): mask word %u is %016llx, pack_task gives %016llx", (unsigned long long)t, m, w, (unsigned long long)pat_b[mb + 64ull * w], (unsigned long long)pat_a[mb + 64ull * w]);
            T.words += 2;
        }
        for (uint32_t w = 0; w < (m + 7) / 8; ++w) {
            owned[pb + 64ull * w] = 1;
            if (!flag_a[t]) continue;                          // a skipped task's byte words are not defined
            if (pat_b[pb + 64ull * w] != pat_a[pb + 64ull * w]) FAIL("task %llu (m %u): byte word %u is %016llx, pack_task gives %016llx", (unsigned long long)t, m, w, (unsigned long long)pat_b[pb + 64ull * w], (unsigned long long)pat_a[pb + 64ull * w]);
            T.words++;
        }
        T.tasks++; if (flag_a[t]) T.kept++; else T.skipped++; if (pflag_a[t]) T.flagged++;
    }
    for (uint64_t i = 0; i <= n_pat; ++i)
        if (!owned[i] && pat_b[i] != STALE) FAIL("workspace word %llu of %llu belongs to no task and was written", (unsigned long long)i, (unsigned long long)n_pat);
    for (uint64_t t = n_tasks; t < n_tasks + 8; ++t) if (pflag_b[t] != 9) FAIL("pflag written behind the last task");
    if (flag_b[n_tasks] != 9 || cm_b[n_tasks] != 7 || cs_b[n_tasks] != 7) FAIL("flag / cnt written behind the last task");
    T.reads += n_reads;
    return 0;
}

int main() {
    lds_tables_t L;
    memset(&L, 0, sizeof L);
    for (int b = 0; b < 256; ++b) L.compl_tab[b] = (uint8_t)b;                  // the index's table (image.hpp)
    L.compl_tab['A'] = 'T'; L.compl_tab['C'] = 'G'; L.compl_tab['G'] = 'C'; L.compl_tab['T'] = 'A';
    L.compl_tab['a'] = 'T'; L.compl_tab['c'] = 'G'; L.compl_tab['g'] = 'C'; L.compl_tab['t'] = 'A';
    for (int i = 0; i < 256; ++i) L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    if (!pk_compl_ok(L.compl_tab)) FAIL("pk_compl_ok rejects the index's complement table");
    { uint8_t id[256]; for (int b = 0; b < 256; ++b) id[b] = (uint8_t)b; if (pk_compl_ok(id)) FAIL("pk_compl_ok accepts the identity"); }
    // the byte arithmetic against the definitions, for every byte value in every place of a word
    for (uint32_t b = 0; b < 256; ++b)
        for (uint32_t j = 0; j < 8; ++j) {
            const uint64_t v = (0x41ull * PK_B01 & ~(0xFFull << (8 * j))) | ((uint64_t)b << (8 * j));
            if (pk_bad8(v) != (base_acgt(b) ? 0ull : 0x80ull << (8 * j))) FAIL("pk_bad8: byte %02x in place %u", b, j);
        }
    for (uint32_t c = 0; c < 65536; c += 7) {
        const uint64_t s = pk_spread8(c);
        if (pk_squeeze8(s) != c) FAIL("pk_squeeze8(pk_spread8(%04x))", c);
        const uint64_t sp = pk_spell8(s);
        for (uint32_t j = 0; j < 8; ++j) { const uint32_t by = (uint32_t)(sp >> (8 * j)) & 0xFFu; if (!base_acgt(by) || base2(by) != ((c >> (2 * j)) & 3u)) FAIL("pk_spell8: code word %04x, place %u", c, j); }
    }
    // the reads: every length in every kind
    std::vector<std::vector<uint8_t>> pool;
    for (uint32_t kind = 0; kind < N_KINDS; ++kind) for (uint32_t li = 0; li < N_LENS; ++li) pool.push_back(make_read(LENS[li], kind));
    // tables for k = 8 (64 K bits) and k = 5: all present, empty, random at density 0.2
    Totals T;
    const uint32_t ks[] = {8, 5};
    for (uint32_t k : ks) {
        const uint64_t tw = pf_table_words(k);
        std::vector<uint32_t> full(tw, 0xFFFFFFFFu), empty(tw, 0), sparse(tw, 0);
        for (uint64_t v = 0; v < (1ull << (2 * k)); ++v) if (rnd_below(5) == 0) sparse[v >> 5] |= 1u << (v & 31u);
        const std::vector<uint32_t>* tabs[] = {&full, &empty, &sparse};
        const uint32_t min_lens[] = {25, k, k + 2, k - 1};                      // W = 26 - k, W = 1, W = 3, the filter stands down; the short reads have m < min_len
        for (const auto* tab : tabs)
            for (uint32_t min_len : min_lens)
                for (uint32_t cw_words : {5u, 8u}) {
                    if (run_batch(pool, L, *tab, min_len, k, cw_words, T)) return 1;          // all of them: blocks whose longest read is not the lane's
                    for (uint32_t nb : {1u, 31u, 32u, 33u, 65u}) {                             // 64-task blocks that are partial, full, and spilling by one
                        std::vector<std::vector<uint8_t>> batch;
                        for (uint32_t i = 0; i < nb; ++i) batch.push_back(pool[rnd_below((uint32_t)pool.size())]);
                        if (run_batch(batch, L, *tab, min_len, k, cw_words, T)) return 1;
                    }
                    std::vector<std::vector<uint8_t>> same(33, make_read(150, 0));              // equal lengths, as the benchmark's
                    if (run_batch(same, L, *tab, min_len, k, cw_words, T)) return 1;
                }
    }
    if (!T.kept || !T.skipped || !T.flagged || !T.plain_long || !T.lookups)
        FAIL("the cases do not cover what they should: %llu kept, %llu skipped, %llu flagged, %llu long reads of A/C/G/T, %llu lookups", (unsigned long long)T.kept, (unsigned long long)T.skipped,
             (unsigned long long)T.flagged, (unsigned long long)T.plain_long, (unsigned long long)T.lookups);
    printf("OK %llu reads, %llu tasks (%llu kept, %llu skipped, %llu with a byte outside A/C/G/T), %llu workspace words compared, %llu lookups\n", (unsigned long long)T.reads,
           (unsigned long long)T.tasks, (unsigned long long)T.kept, (unsigned long long)T.skipped, (unsigned long long)T.flagged, (unsigned long long)T.words, (unsigned long long)T.lookups);
    return 0;
}
