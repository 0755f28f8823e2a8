// TEST HARNESS ONLY - not part of the product.  A stand-alone program over moni_align_amd/csrc/prefilter_core.h (the code strand_filter_kernel and
// kmer_build_kernel run, compiled for the host) and pack_task of seed_core.h, which writes the code words the filter reads: the k-mer table against
// a brute-force k-mer set, and the filter's decisions against an exact bytewise search for a common substring of min_len bytes.  Built plain
// and with the address and undefined-behaviour sanitizers by tests/test_host_prefilter.py.  Prints "OK ..." and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../moni_align_amd/csrc/seed_core.h"
#include "../../moni_align_amd/csrc/prefilter_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }
static const char ACGT[] = "ACGT";

#define FAIL(...) do { fprintf(stderr, "prefilter_sim: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

struct Totals { uint64_t tasks = 0, skipped = 0, none_acgt = 0, none_acgt_skipped = 0, with_mem = 0, flagged = 0, sparse_none = 0, sparse_none_skipped = 0, lookups = 0; int sparse_cases = 0; };

// one text, one k, one min_len
// kmers_only: no table (4^16 bits are 512 MB), only the k-mers cut out of the code words against the pattern's bytes
static int run_case(uint32_t n_text, uint32_t k, uint32_t min_len, Totals& T, bool kmers_only = false) {
    // the text: random A / C / G / T with separators, runs of N and lower-case stretches
    std::vector<uint8_t> text(n_text + 16, 0);
    for (uint32_t i = 0; i < n_text; ++i) text[i] = (uint8_t)ACGT[rnd_below(4)];
    for (uint32_t j = 0; j < 1 + n_text / 5000; ++j) text[rnd_below(n_text)] = '$';
    for (uint32_t j = 0; j < 1 + n_text / 8000; ++j) { const uint32_t at = rnd_below(n_text), ln = 1 + rnd_below(40); for (uint32_t i = at; i < at + ln && i < n_text; ++i) text[i] = 'N'; }
    for (uint32_t j = 0; j < 1 + n_text / 8000; ++j) { const uint32_t at = rnd_below(n_text), ln = 1 + rnd_below(60); for (uint32_t i = at; i < at + ln && i < n_text; ++i) text[i] = (uint8_t)(text[i] | 0x20); }
    // the table as the kernel builds it, against the k-mers found position by position
    const uint64_t tw = kmers_only ? 1 : pf_table_words(k);
    std::vector<uint32_t> tab(tw, 0), want(tw, 0);
    if (!kmers_only) for (uint64_t w = 0; w < (uint64_t)n_text / 32 + 1; ++w) pf_build_word(text.data(), n_text, w, k, tab.data());
    uint64_t pop = 0;
    for (uint32_t p = 0; !kmers_only && p + k <= n_text; ++p) {
        uint64_t v = 0; bool ok = true;
        for (uint32_t j = 0; j < k && ok; ++j) { const uint8_t b = text[p + j]; ok = b == 'A' || b == 'C' || b == 'G' || b == 'T'; v |= (uint64_t)(b == 'A' ? 0 : b == 'C' ? 1 : b == 'T' ? 2 : 3) << (2 * j); }
        if (ok) want[v >> 5] |= 1u << (v & 31);
    }
    for (uint64_t w = 0; w < tw; ++w) { if (tab[w] != want[w]) FAIL("n_text %u k %u: table word %llu is %08x, the k-mer set gives %08x", n_text, k, (unsigned long long)w, tab[w], want[w]); pop += (unsigned)__builtin_popcount(tab[w]); }
    const double density = (double)pop / (double)(1ull << (2 * k));
    // every substring of min_len bytes of the text (exact: the strings themselves)
    std::set<std::string> grams;
    if (min_len && n_text >= min_len) for (uint32_t p = 0; p + min_len <= n_text; ++p) grams.insert(std::string((const char*)text.data() + p, min_len));
    // the reads: cut from the text with substitutions, the reverse complements of such, random ones; every length of the list
    const uint32_t lens[] = {0, k - 1, k, min_len ? min_len - 1 : 0, min_len, 31, 32, 33, 63, 64, 65, 150, 250};
    uint8_t compl_tab[256];
    for (int b = 0; b < 256; ++b) compl_tab[b] = (uint8_t)b;
    compl_tab['A'] = 'T'; compl_tab['C'] = 'G'; compl_tab['G'] = 'C'; compl_tab['T'] = 'A'; compl_tab['a'] = 'T'; compl_tab['c'] = 'G'; compl_tab['g'] = 'C'; compl_tab['t'] = 'A';
    std::vector<uint8_t> seq; std::vector<uint64_t> offs(1, 0);
    for (uint32_t rep = 0; rep < 3; ++rep)
        for (uint32_t li = 0; li < sizeof(lens) / sizeof(lens[0]); ++li)
            for (uint32_t kind = 0; kind < 3; ++kind) {
                const uint32_t m = lens[li] < n_text ? lens[li] : n_text;
                std::vector<uint8_t> r(m);
                if (kind == 2) for (uint32_t i = 0; i < m; ++i) r[i] = (uint8_t)ACGT[rnd_below(4)];
                else {
                    const uint32_t at = rnd_below(n_text - m + 1);
                    for (uint32_t i = 0; i < m; ++i) r[i] = text[at + i];
                    for (uint32_t i = 0; i < m; ++i) if (rnd_below(100) < (rep == 2 ? 8u : 1u)) r[i] = (uint8_t)ACGT[rnd_below(4)];       // 1 % substitutions; a third of the reads 8 %
                    if (kind == 1) { std::vector<uint8_t> q(m); for (uint32_t i = 0; i < m; ++i) q[i] = compl_tab[r[m - 1 - i]]; r.swap(q); }
                }
                seq.insert(seq.end(), r.begin(), r.end());
                offs.push_back(seq.size());
            }
    const uint64_t n_reads = offs.size() - 1, n_tasks = 2 * n_reads;
    // the workspace layout of reads_upload and the packed patterns, as the product makes them
    const uint64_t n_blk = (n_reads + 31) / 32;
    std::vector<moni_u64x2> blk(n_blk + 1);
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
    lds_tables_t L;
    memset(&L, 0, sizeof L);
    memcpy(L.compl_tab, compl_tab, 256);
    for (int i = 0; i < 256; ++i) L.c2[i] = base_acgt((uint32_t)i) ? (uint8_t)base2((uint32_t)i) : (uint8_t)4;
    std::vector<uint64_t> seq_pad((seq.size() + 16 + 7) / 8 + 1, 0);
    if (!seq.empty()) memcpy(seq_pad.data(), seq.data(), seq.size());
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(seq_pad.data());
    std::vector<uint64_t> pat(blk[n_blk].y + 1, 0);
    std::vector<uint8_t> pflag(n_tasks + 1, 0);
    for (uint64_t t = 0; t < n_tasks; ++t) pack_task(L, sq, offs.data(), blk.data(), t, pat.data(), pflag.data());
    for (uint64_t t = 0; t < n_tasks; ++t) {
        const uint64_t rd = t >> 1;
        const uint32_t m = (uint32_t)(offs[rd + 1] - offs[rd]);
        std::string p(m, ' ');                                             // the strand-resolved pattern, byte by byte
        for (uint32_t i = 0; i < m; ++i) p[i] = (t & 1) ? (char)compl_tab[seq[offs[rd] + m - 1 - i]] : (char)seq[offs[rd] + i];
        bool only_acgt = true;
        for (uint32_t i = 0; i < m; ++i) only_acgt = only_acgt && (p[i] == 'A' || p[i] == 'C' || p[i] == 'G' || p[i] == 'T');
        if (only_acgt == (pflag[t] != 0)) FAIL("task %llu: pflag %u for a pattern that %s", (unsigned long long)t, pflag[t], only_acgt ? "holds only A/C/G/T" : "holds another byte");
        bool has = false;
        if (min_len == 0) has = true;
        else for (uint32_t i = 0; i + min_len <= m && !has; ++i) has = grams.count(p.substr(i, min_len)) != 0;
        const uint64_t cb = ws_pat_base(blk.data(), t) + 64u * ((ws_block_len(blk.data(), t) + 7) / 8);
        pf_pat_t P;
        pf_pat_init(P, pat.data() + cb, 64u, m);
        for (uint32_t q = 0; only_acgt && q + k <= m; ++q) {                // k-mers that straddle a word boundary included
            uint64_t v = 0;
            for (uint32_t j = 0; j < k; ++j) v |= (uint64_t)(p[q + j] == 'A' ? 0 : p[q + j] == 'C' ? 1 : p[q + j] == 'T' ? 2 : 3) << (2 * j);
            const uint32_t qq = (q * 7u) % (m - k + 1);                      // (not in increasing order: the two-word copy is reloaded both ways)
            uint64_t vv = 0;
            for (uint32_t j = 0; j < k; ++j) vv |= (uint64_t)(p[qq + j] == 'A' ? 0 : p[qq + j] == 'C' ? 1 : p[qq + j] == 'T' ? 2 : 3) << (2 * j);
            if (pf_kmer(P, q, k) != v || pf_kmer(P, qq, k) != vv) FAIL("k %u: the k-mer at offset %u or %u of task %llu (m %u) is not the pattern's", k, q, qq, (unsigned long long)t, m);
        }
        if (kmers_only) continue;
        unsigned long long lookups = 0;
        const bool keep = pf_task_keep(P, m, min_len, k, pflag[t] != 0, tab.data(), lookups);
        T.tasks++; T.lookups += lookups;
        if (!keep) {
            T.skipped++;
            if (has) FAIL("n_text %u k %u min_len %u: task %llu (m %u) was skipped and shares %u bytes with the text: %s", n_text, k, min_len, (unsigned long long)t, m, min_len, p.c_str());
            if (min_len < k) FAIL("min_len %u < k %u: task %llu was skipped", min_len, k, (unsigned long long)t);
            if (!only_acgt) FAIL("task %llu holds a byte outside A/C/G/T and was skipped", (unsigned long long)t);
        }
        if (has) T.with_mem++;
        if (!only_acgt) T.flagged++;
        if (!has && only_acgt && min_len >= k) {
            T.none_acgt++; if (!keep) T.none_acgt_skipped++;
            if (density <= 0.02) { T.sparse_none++; if (!keep) T.sparse_none_skipped++; }
        }
    }
    if (density <= 0.02 && min_len >= k) T.sparse_cases++;
    printf("n_text %6u k %2u min_len %2u: density %.4f, %llu tasks\n", n_text, k, min_len, density, (unsigned long long)n_tasks);
    return 0;
}

int main() {
    Totals T;
    // the k of the formula and a larger one (a sparse table, as a pangenome's is: haplotypes share their k-mers) for texts of 2 k to 50 k bases
    const uint32_t sizes[] = {2000, 7001, 50000};
    for (uint32_t n : sizes) {
        const uint32_t k0 = pf_choose_k(n);
        if (run_case(n, k0, 25, T)) return 1;
        if (run_case(n, k0 + 3 > 12 ? 12 : k0 + 3, 25, T)) return 1;
    }
    if (run_case(20000, 12, 25, T)) return 1;
    if (run_case(20000, 12, 12, T)) return 1;                  // min_len == k: a window is one k-mer
    if (run_case(20000, 12, 11, T)) return 1;                  // min_len < k: nothing may be skipped
    if (run_case(3000, 14, 19, T)) return 1;
    if (run_case(3000, 16, 25, T, true)) return 1;             // k-mers of a whole half word
    if (pf_choose_k(61420004ull * 12) != 16 || pf_choose_k(1ull << 20) != 11 || pf_choose_k((1ull << 20) + 1) != 12 || pf_choose_k(1) != PF_K_MIN || pf_choose_k(~0ull) != 16)
        FAIL("pf_choose_k: %u %u %u %u", pf_choose_k(61420004ull * 12), pf_choose_k(1ull << 20), pf_choose_k((1ull << 20) + 1), pf_choose_k(1));
    if (T.sparse_cases < 3 || T.sparse_none == 0) FAIL("no case with a table density of at most 2 %%");
    if (2 * T.sparse_none_skipped < T.sparse_none) FAIL("tables of density <= 2 %%: %llu of %llu tasks without a common substring were skipped, less than half",
                                                        (unsigned long long)T.sparse_none_skipped, (unsigned long long)T.sparse_none);
    if (T.with_mem == 0 || T.flagged == 0 || T.skipped == 0) FAIL("the cases do not cover what they should: %llu with a common substring, %llu flagged, %llu skipped",
                                                                  (unsigned long long)T.with_mem, (unsigned long long)T.flagged, (unsigned long long)T.skipped);
    printf("OK %llu tasks, %llu skipped, %llu with a common substring, %llu with a byte outside A/C/G/T; without a common substring and A/C/G/T only: %llu of %llu skipped "
           "(density <= 2 %%: %llu of %llu); %.2f lookups per task\n", (unsigned long long)T.tasks, (unsigned long long)T.skipped, (unsigned long long)T.with_mem, (unsigned long long)T.flagged,
           (unsigned long long)T.none_acgt_skipped, (unsigned long long)T.none_acgt, (unsigned long long)T.sparse_none_skipped, (unsigned long long)T.sparse_none, (double)T.lookups / (double)T.tasks);
    return 0;
}
