// moni-hip-align: the `align_full_ksw2` command line (src/align/align_full_ksw2.cpp:101-431) over libmoni_hip.so.
//
//   moni-hip-align <prefix> -p reads.fq [-o out.sam] [-t T] [-b B] [-l len] [-L ext] [-A a] [-B b] [-O o1[,o2]] [-E e1[,e2]]
//                  [-s] [-f] [-a] [-S n] [-F f] [-w iter] [-v pred] [-x dx] [-y dy] [-k mem] [-j score] [--gpus N] [--gpu-batch R]
//
// Same getopt string, flag meanings, struct defaults and default output name as the reference, so the `moni align` wrapper
// (pipeline/moni.in:494-546) can call it unchanged.  Index: <prefix>.mfi (the flat arrays moni_align_amd/index_build.py
// writes) or, when that file is absent, the reference's own files <prefix>.thrbv.full.lcp.ms + <prefix>.ldx as `moni build` leaves them
// (moni_index_load_reference: the .plain.slp grammar is not read, the text is rebuilt from the BWT on the GPU; a <prefix>.txt with the
// text as plain bytes is used when present).  The .thrbv.full.lcp.ms reader follows the sdsl / r-index layouts from recall: no file
// written by the reference was available to check it against.  Reads are streamed in large batches (the
// reference's -b is a per-thread batch of 512; a GPU wants ~10^6).  Plain FASTQ / FASTA files (the streaming path, fast_align below):
// the file is mapped and cut into record-aligned byte ranges of about --gpu-batch reads; three workers per GPU, each with its own
// context, take ranges in order: parse (two passes over the range with a few helper threads: count, then fill the batch arrays in
// place), moni_align_stream (upload, kernels, the lines in read order in the context's pinned buffer), then pwrite of the block at its
// place in the output file, again in parallel slices.  A block's place is known as soon as the earlier ranges have reported their
// lengths, so parsing, GPU work and file writes of different ranges overlap and nothing is copied twice.  gzip input, -m and the legacy
// modes take the older path: a reader thread parses ahead into a bounded queue, two workers per GPU, a writer thread with a bounded
// in-order window.  BGZF input (blocked gzip: bgzip, this program's own --bgzf) of single-end and paired alignment is inflated on the GPU
// (BgzfInput below: a thread per input file with a context of its own inflates --inflate-blocks members at a time, in file order, and hands
// record-aligned text to the same workers, which parse it as if it were a range of a mapped plain file); --host-inflate, plain gzip, -m, -c,
// --extend, the legacy and pattern-query modes and FASTA with wrapped lines stay on the older path.  -m writes the report-MEMs records (aligner_ksw2.hpp:346-373);
// --ms / --mems write the legacy `moni ms` / `moni mems` text outputs (src/matching_statistics.cpp:520-610, src/mems.cpp:520-600).
// Output: the three pipelines that write SAM - pairs (run_paired), single-end streaming, single-end queue - write through one Sink (below, behind parse): it
// opens the file, writes the header in the flavour's form (text, --bgzf blocks, --bam, --bam --sort [--mark-dup]) and sets the BAM dictionary on the contexts,
// turns a batch's text into the bytes that go into the file (or into a run of the sort), and ends the file (the sort's merge and index, the end-of-file
// block, the close).  Its Placer puts blocks that come in any order at the in-order prefix sum of their lengths with pwrite in parallel slices; both streaming
// pipelines use it, paired -c a second one for <sam>.csv, and the queue pipeline's writer thread appends.  The pattern modes write their own <out><suffix> files.
// --ms / --mems --split [--seg-len N] [--overlap N] take patterns of genome length (a chromosome, an assembly) through moni_ms_long_batch: every pattern
// is cut into segments of N bases that are walked side by side, and batches are sized by bases, not by reads.  .lengths and the (offset,length) pairs
// of .mems are byte-identical to the run without --split; .pointers may differ where a pattern was cut - every pointer is a position of a maximal
// match, but not necessarily the one the reference reports.
// --extend writes the SAM file of the legacy `moni extend` (extender_ksw2.hpp, extend_reads_dispatcher.hpp:435-486; moni_extend_batch) - single-end
// reads, the same path as -m; its @HD line has the tabs of moni_sam_header where the reference's extender writes blanks.
// --pseudo-ms writes <out>.pseudo_lengths, the text of the legacy `moni pseudo-ms` (src/spumoni/run_spumoni.cpp:466-501; moni_pml_batch): per read a
// line ">" + the read's running number in the input, then its pseudo-matching lengths, each followed by a blank.  Single-end reads, the same path as -m.
// --screen [--window N] [--min-win N] [--ks NUM/DEN] [--one-strand] writes <out>.screen (moni_screen_batch: every read called present or absent from its
// pseudo-matching lengths on both strands against those of the read reversed): per read, in input order, one line
// `name length P|A|S +|-|. n_win n_pos0 n_pos1 d_max0 d_max1 max_pml0 max_pml1`, tab-separated - P present, A absent, S too short for a scored window; the strand
// column is . unless the read is present.  Single-end reads, the same path as -m.
// --seq-count [--both-strands] [--max-walk N] writes <out>.seqcount (moni_seqcount_batch: per pattern and strand, the occurrences that start in each
// sequence of the index): name <+|-> count matched n_seqs seqname:count,... - the sequences with a count, in index order; * for none, ? where the
// pattern has more than --max-walk occurrences and was not enumerated.
// --loci [--both-strands] [--max-walk N] [--no-lift] writes <out>.loci (moni_loci_batch: per pattern and strand, the distinct reference positions its
// occurrences lift to): name <+|-> count matched n_loci seqname:pos:support,... - tab-separated, pos 1-based, the loci in reference order, support the
// occurrences that land on each; * for none, ? where the pattern has more than --max-walk occurrences and was not enumerated.  --no-lift keeps text
// positions: every occurrence, in text order, each with support 1.
// --approx K [--max-hits N] [--max-occ N] [--both-strands] [--max-steps N] writes <out>.approx (moni_approx_batch: every string within K <= 3
// substitutions of the pattern that occurs in the index): per pattern and strand one line `name <+|-> complete cnt0,..,cntK n_hits hits`, tab-separated -
// complete is 0 where --max-steps stopped a part of the search (the figures are lower bounds then), cnt the text positions at each distance, n_hits the
// distinct matching strings; the hits kept (--max-hits, default 16) as n_mis:count:seqname:pos,seqname:pos,... (1-based, --max-occ of them, default 0: `*`),
// separated by `;`, sorted by distance; `*` when there are none.
// --locate [--max-occ N] [--both-strands] writes <out>.locate (moni_locate_batch: exact-match count and locate, what r_index::count / locate_all give):
// per pattern and strand one line `name <+|-> count matched occurrences`, tab-separated, the occurrences as seqname:pos (1-based), comma-separated, in
// the library's order, `*` when there are none.  Single-end input (FASTA or FASTQ), the same path as -m.
// -n loads <prefix>.thrbv.full.ms (no LCP samples); -q is accepted (the text comes from the BWT, not from either grammar).
// -c writes <sam>.csv (per-read MEM statistics, csv.hpp:55-67; through the host pipeline - for pairs one line per pair, moni_pe_align_csv_batch).  -Z (secondary chains,
// chain.hpp:442-727) acts on paired input and is ignored for single-end input, as in the reference (aligner_ksw2.hpp:1190-1191 is the only call site).
#include <fcntl.h>
#include <getopt.h>
#include <libgen.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/moni_hip.h"

static void die(const std::string& msg) { fprintf(stderr, "[ERROR] %s\n", msg.c_str()); exit(1); }   // common.hpp:108-117
// output that did not reach the file (a full disk) is an error, not a shorter SAM file with exit code 0
static void put(const void* p, size_t n, FILE* f) { if (n && fwrite(p, 1, n, f) != n) die("short write to the output file"); }
static void close_out(FILE* f) { if (f && fclose(f) != 0) die("closing the output file failed (output incomplete)"); }
static void info(const std::string& msg) { printf("[INFO] Message: %s\n", msg.c_str()); fflush(stdout); }
// every byte of [p, p + n) at `at` in fd
static void pwrite_all(int fd, const char* p, size_t n, uint64_t at) {
    while (n) {
        const ssize_t w = pwrite(fd, p, n, (off_t)at);
        if (w < 0) { if (errno == EINTR) continue; die("write to the output file failed"); }
        p += w; n -= (size_t)w; at += (uint64_t)w;
    }
}

// ---- --bam --sort: coordinate-sorted, indexed BAM -----------------------------------------------------------------------
// Phase 1: every batch's SAM text becomes a sorted run (moni_bam_sorted_run on the context that aligned it); the run's records go to a temporary
// file beside the output - unlinked as soon as it is open -, its keys and offsets stay in memory, 16 bytes a read.  Phase 2, behind the last
// batch: moni_bam_merge_plan cuts the merged order into chunks, one contiguous slice of every run each; the contexts take the chunks in turn -
// pread the slices, moni_bam_sort, the blocks at their place in the file - and moni_bai_add sees them in chunk order.
// --coverage: the files beside <out>.bam from a sealed object - the summary, the per-base text in BGZF blocks and, with a window, the regions
struct CoverageOut { bool on = false; uint32_t window = 0, min_mapq = 0; uint64_t max_bases = 64ull << 20, max_lines = 4ull << 20; };      // the two limits of a moni_cov_next call stand as proposed: neither has been measured
static void write_coverage(moni_ctx_t* c, moni_cov_t* cov, const CoverageOut& co, const std::string& bam_path, const std::string& header, uint64_t counted, uint64_t records);

struct SortedBam {
    struct Run { uint64_t at = 0; std::vector<uint64_t> keys, offs{0}; std::vector<moni_bam_dup_t> dups; std::vector<uint8_t> marks; };
    bool mark = false;              // --mark-dup: the runs keep their entries, 32 bytes a pair or fragment; the marks, a byte a record, come between the phases
    uint32_t paired = 0;            // the records of a run are mates two by two
    uint64_t mark_max_entries = 1ull << 29;          // about 80 GB of the device's memory at 150 bytes an entry; the library's own limit is 2^31 - 1
    int tmp_fd = -1;
    uint64_t chunk_bytes = 0;
    uint32_t n_ref = 0;
    CoverageOut cover;              // --coverage: every chunk's records are added to one object while they are still on the device
    std::string out_path, sam_header;
    std::string bai_path;
    std::atomic<uint64_t> tmp_len{0};
    std::mutex mu;
    std::map<size_t, Run> runs;

    void open(const std::string& out_path, uint64_t chunk, const std::string& header) {
        chunk_bytes = chunk; bai_path = out_path + ".bai"; this->out_path = out_path; sam_header = header;
        for (size_t at = 0; at < header.size(); at = header.find('\n', at) == std::string::npos ? header.size() : header.find('\n', at) + 1)
            if (!header.compare(at, 4, "@SQ\t")) ++n_ref;
        std::string t = out_path + ".sort.XXXXXX";
        tmp_fd = mkstemp(&t[0]);
        if (tmp_fd < 0) die("cannot create a temporary file beside " + out_path);
        unlink(t.c_str());          // a crash leaves nothing behind
    }
    // run `id` (the batch's number in the input): the SAM lines through moni_bam_sorted_run on context c
    void add_run(moni_ctx_t* c, size_t id, const char* sam, uint64_t len) {
        const uint8_t* rec; const uint64_t* keys; const uint64_t* offs; uint64_t rl, n, nd = 0;
        const moni_bam_dup_t* dups = nullptr;
        moni_bam_run_dup_stats_t ds;
        memset(&ds, 0, sizeof ds);
        const int rc = mark ? moni_bam_sorted_run_dup(c, sam, len, paired, &rec, &rl, &keys, &offs, &n, &dups, &nd, &ds) : moni_bam_sorted_run(c, sam, len, &rec, &rl, &keys, &offs, &n, &ds.run);
        const moni_bam_sort_stats_t& st = ds.run;
        if (rc == MONI_EINVAL && st.bad_records && ds.bad_is_record)
            die("moni_bam_sorted_run_dup: " + std::to_string(st.bad_records) + " record(s) of a batch cannot be marked; the first is its record " +
                std::to_string(st.first_bad_record) + " (reason " + std::to_string(st.bad_reason) + " of MONI_BAMSORT_*)");
        if (rc == MONI_EINVAL && st.bad_records)
            die("moni_bam_sorted_run: " + std::to_string(st.bad_records) + " line(s) of a batch cannot be written as BAM records; the first is its line " +
                std::to_string(st.first_bad_record) + " (reason " + std::to_string(st.bad_reason) + " of MONI_BAM_*)");
        if (rc) die("moni_bam_sorted_run failed (" + std::to_string(rc) + ")");
        Run r;
        r.at = tmp_len.fetch_add(rl);
        r.keys.assign(keys, keys + n); r.offs.assign(offs, offs + n + 1);
        if (nd) r.dups.assign(dups, dups + nd);
        for (uint64_t done = 0; done < rl;) {
            const ssize_t w = pwrite(tmp_fd, rec + done, rl - done, (off_t)(r.at + done));
            if (w <= 0) die("short write to the sort's temporary file");
            done += (uint64_t)w;
        }
        std::lock_guard<std::mutex> lk(mu);
        runs[id] = std::move(r);
    }
    // --mark-dup, between the phases: one context resolves the entries of all runs; every run gets its marks, a byte a record in sorted order.
    // On the device the resolve holds 124 bytes an entry (the entries, the keys and elements of its sorts before and behind a pass - of twice as
    // many ends as entries -, the records' places), a byte a record and the radix sort's own space: about 150 bytes an entry.  More than
    // mark_max_entries is refused here; a device that has less free memory makes moni_bam_dup_resolve return MONI_ENOMEM.
    void resolve(moni_ctx_t* c, const std::vector<Run*>& run) {
        const size_t R = run.size();
        std::vector<const moni_bam_dup_t*> dp(R); std::vector<uint8_t*> mp(R); std::vector<uint64_t> nd(R), nr(R);
        uint64_t entries = 0, records = 0;
        for (size_t r = 0; r < R; ++r) {
            run[r]->marks.assign(run[r]->keys.size(), 0);
            dp[r] = run[r]->dups.data(); mp[r] = run[r]->marks.data(); nd[r] = run[r]->dups.size(); nr[r] = run[r]->keys.size();
            entries += nd[r]; records += nr[r];
        }
        if (entries > mark_max_entries || records >= 0xFFFFFFFFull)
            die("--mark-dup: " + std::to_string(entries) + " pairs and fragments in " + std::to_string(records) + " records are more than one GPU resolves (" +
                std::to_string(mark_max_entries) + " entries, 2^32 - 2 records); split the input");
        moni_bam_dup_stats_t st;
        const int rc = moni_bam_dup_resolve(c, dp.data(), nd.data(), nr.data(), R, mp.data(), &st);
        if (rc) die("moni_bam_dup_resolve failed (" + std::to_string(rc) + ")");
        for (size_t r = 0; r < R; ++r) std::vector<moni_bam_dup_t>().swap(run[r]->dups);
        info("Duplicates: " + std::to_string(st.dup_pairs) + " of " + std::to_string(st.pairs) + " pairs, " + std::to_string(st.dup_fragments) + " of " + std::to_string(st.fragments) +
             " fragments, " + std::to_string(st.marked_records) + " records marked");
    }
    // the chunks behind `at` in fd, then the index; returns where the end-of-file block goes
    uint64_t finish(const std::vector<moni_ctx_t*>& cs, int fd, uint64_t at) {
        const auto t0 = std::chrono::steady_clock::now();
        const size_t R = runs.empty() ? 0 : runs.rbegin()->first + 1;
        std::vector<Run*> run(R, nullptr);
        Run none;
        for (size_t r = 0; r < R; ++r) run[r] = runs.count(r) ? &runs[r] : &none;          // a number no batch took: an empty run
        std::vector<const uint64_t*> kp(R), op(R);
        std::vector<uint64_t> nn(R);
        for (size_t r = 0; r < R; ++r) { kp[r] = run[r]->keys.data(); op[r] = run[r]->offs.data(); nn[r] = run[r]->keys.size(); }
        if (mark) resolve(cs[0], run);
        moni_bam_plan_t* plan = nullptr;
        if (moni_bam_merge_plan(kp.data(), nn.data(), op.data(), R, chunk_bytes, &plan)) die("moni_bam_merge_plan failed");
        moni_bai_t* bai = moni_bai_create(n_ref);
        if (!bai) die("out of memory");
        moni_bam_params_t bp; moni_bam_params_default(&bp);
        moni_cov_t* cov = nullptr;
        std::atomic<uint64_t> cov_counted{0}, cov_records{0};
        if (cover.on) {
            moni_cov_params_t cp; moni_cov_params_default(&cp);
            cp.min_mapq = cover.min_mapq;
            const int rc = moni_cov_create(cs[0], &cp, &cov);
            if (rc) die("moni_cov_create failed (" + std::to_string(rc) + (rc == MONI_ENOMEM ? "): --coverage takes 4 bytes of the device's memory per reference base" : ")"));
        }
        std::atomic<uint64_t> next{0};
        std::mutex mo; std::condition_variable cv;
        uint64_t upto = 0, off_upto = at;
        auto worker = [&](moni_ctx_t* c) {
            std::vector<uint8_t> buf, mk; std::vector<uint64_t> offs; std::vector<uint32_t> cs_;
            for (uint64_t k; (k = next.fetch_add(1)) < plan->n_chunks;) {
                const uint64_t* lo = plan->cuts + k * R; const uint64_t* hi = lo + R;
                uint64_t bytes = 0, n = 0;
                for (size_t r = 0; r < R; ++r) { bytes += run[r]->offs[hi[r]] - run[r]->offs[lo[r]]; n += hi[r] - lo[r]; }
                buf.resize(bytes); offs.assign(1, 0); mk.clear();
                for (size_t r = 0; r < R; ++r) {
                    const uint64_t a0 = run[r]->offs[lo[r]], a1 = run[r]->offs[hi[r]], base = offs.back();
                    for (uint64_t done = 0; done < a1 - a0;) {
                        const ssize_t g = pread(tmp_fd, buf.data() + base + done, a1 - a0 - done, (off_t)(run[r]->at + a0 + done));
                        if (g <= 0) die("short read from the sort's temporary file");
                        done += (uint64_t)g;
                    }
                    for (uint64_t i = lo[r]; i < hi[r]; ++i) offs.push_back(base + run[r]->offs[i + 1] - a0);
                    if (mark) mk.insert(mk.end(), run[r]->marks.begin() + (ptrdiff_t)lo[r], run[r]->marks.begin() + (ptrdiff_t)hi[r]);
                }
                const uint8_t* z; uint64_t zl; const moni_bam_ent_t* ents; moni_bam_sort_stats_t st;
                const int rc = moni_bam_sort_marked(c, buf.data(), bytes, offs.data(), n, mark ? mk.data() : nullptr, &bp, &z, &zl, &ents, &st);
                if (rc) die("moni_bam_sort failed (" + std::to_string(rc) + ")");
                if (cov) {          // z and ents stay valid: the adds have buffers of their own
                    moni_cov_stats_t vs;
                    const int vrc = moni_cov_add_sorted(c, cov, &vs);
                    if (vrc) die("moni_cov_add_sorted failed (" + std::to_string(vrc) + (vrc == MONI_ERANGE ? "): --coverage counts fewer than 2^31 records" : ")"));
                    cov_counted += vs.counted; cov_records += vs.records;
                }
                cs_.clear();
                for (uint64_t p = 0; p < zl;) { const uint32_t b = (uint32_t)z[p + 16] + ((uint32_t)z[p + 17] << 8) + 1u; cs_.push_back(b); p += b; }
                uint64_t mine;
                {
                    std::unique_lock<std::mutex> lk(mo);
                    cv.wait(lk, [&] { return upto == k; });
                    mine = off_upto;
                    if (moni_bai_add(bai, ents, n, bytes, bp.block_size, cs_.data(), cs_.size(), mine)) die("moni_bai_add failed: the chunks are not in coordinate order");
                    off_upto += zl; ++upto;
                    cv.notify_all();
                }
                for (uint64_t done = 0; done < zl;) {
                    const ssize_t w = pwrite(fd, z + done, zl - done, (off_t)(mine + done));
                    if (w <= 0) die("short write to the output file");
                    done += (uint64_t)w;
                }
            }
        };
        std::vector<std::thread> th;
        for (size_t w = 1; w < cs.size(); ++w) th.emplace_back(worker, cs[w]);
        worker(cs[0]);
        for (auto& t : th) t.join();
        if (cov) {
            write_coverage(cs[0], cov, cover, out_path, sam_header, cov_counted.load(), cov_records.load());
            moni_cov_destroy(cov);
        }
        const uint8_t* ib; uint64_t il;
        if (moni_bai_finish(bai, off_upto, &ib, &il)) die("moni_bai_finish failed");
        FILE* f = fopen(bai_path.c_str(), "w");
        if (!f) die("open() file " + bai_path + " failed");
        put(ib, il, f);
        close_out(f);
        moni_bai_destroy(bai);
        const uint64_t n_chunks = plan->n_chunks;
        moni_bam_plan_free(plan);
        ::close(tmp_fd); tmp_fd = -1;
        uint64_t n_rec = 0;
        for (size_t r = 0; r < R; ++r) n_rec += nn[r];
        info("Sorted output: " + std::to_string(n_rec) + " records in " + std::to_string(R) + " runs (" + std::to_string(tmp_len.load()) + " bytes) merged as " + std::to_string(n_chunks) +
             " chunks over " + std::to_string(cs.size()) + " contexts in " + std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()) + " s; index: " + bai_path);
        return off_upto;
    }
};

struct Batch {
    std::vector<uint8_t> seq, qual, names;
    std::vector<uint64_t> off{0}, name_off{0};
    bool has_qual = true;
    size_t n() const { return off.size() - 1; }
};

// kseq.h semantics: name = first word of the header, sequence/quality may span lines, '>' or '@' records
struct Reader {
    gzFile fp;
    std::string line;
    bool have_line = false, eof = false;
    explicit Reader(const std::string& path) { fp = gzopen(path.c_str(), "r"); if (!fp) die("open() file " + path + " failed"); }
    ~Reader() { if (fp) gzclose(fp); }
    bool getline() {
        if (have_line) { have_line = false; return true; }
        line.clear();
        char buf[65536];
        bool any = false;
        while (gzgets(fp, buf, sizeof buf)) {
            any = true;
            size_t l = strlen(buf);
            if (l && buf[l - 1] == '\n') { buf[--l] = 0; if (l && buf[l - 1] == '\r') buf[--l] = 0; line.append(buf, l); return true; }
            line.append(buf, l);
        }
        if (!any) eof = true;
        return any;
    }
    // appends one record; false at end of file
    bool next(Batch& b) {
        while (getline()) if (!line.empty() && (line[0] == '>' || line[0] == '@')) break;
        if (eof && line.empty()) return false;
        if (line.empty() || (line[0] != '>' && line[0] != '@')) return false;
        const bool fq = line[0] == '@';
        size_t e = 1;
        while (e < line.size() && !isspace((unsigned char)line[e])) ++e;
        b.names.insert(b.names.end(), line.begin() + 1, line.begin() + e);
        b.name_off.push_back(b.names.size());
        size_t slen = 0;
        while (getline()) {
            if (!line.empty() && (line[0] == '+' || line[0] == '>' || (line[0] == '@' && !fq))) break;
            if (!line.empty() && line[0] == '@' && fq) break;
            for (char c : line) if (!isspace((unsigned char)c)) { b.seq.push_back((uint8_t)c); ++slen; }
        }
        b.off.push_back(b.seq.size());
        if (!eof && !line.empty() && line[0] == '+') {
            size_t qlen = 0;
            while (qlen < slen && getline()) { for (char c : line) { b.qual.push_back((uint8_t)c); ++qlen; } }
            if (qlen != slen) die("truncated quality string");
        } else {
            if (!eof) have_line = true;            // header of the next record
            b.has_qual = false;
            b.qual.resize(b.seq.size(), (uint8_t)'*');
        }
        return true;
    }
};

// Plain (uncompressed) four-line FASTQ / two-line FASTA mapped into memory: records are split with memchr.  Anything else (gzip, wrapped
// sequences) takes the kseq-style Reader above.
struct MappedReader {
    const char* p = nullptr; size_t n = 0, at = 0; int fd = -1;
    bool open(const std::string& path) {
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size < 4) { ::close(fd); fd = -1; return false; }
        n = (size_t)st.st_size;
        void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { ::close(fd); fd = -1; return false; }
        madvise(m, n, MADV_SEQUENTIAL);
        p = (const char*)m;
        if ((unsigned char)p[0] == 0x1f && (unsigned char)p[1] == 0x8b) { close(); return false; }     // gzip
        // the fast path needs one-line sequences: check the first record
        const char* l1 = (const char*)memchr(p, '\n', n);
        if (!l1 || (p[0] != '@' && p[0] != '>')) { close(); return false; }
        const char* l2 = (const char*)memchr(l1 + 1, '\n', n - (size_t)(l1 + 1 - p));
        if (!l2) { close(); return false; }
        if (p[0] == '@' && (l2 + 1 >= p + n || l2[1] != '+')) { close(); return false; }
        return true;
    }
    void close() { if (p) munmap((void*)p, n); p = nullptr; if (fd >= 0) ::close(fd); fd = -1; }
    ~MappedReader() { close(); }
    static const char* eol(const char* s, const char* end) { const char* e = (const char*)memchr(s, '\n', (size_t)(end - s)); return e ? e : end; }
    bool next(Batch& b) {
        const char* end = p + n;
        const char* s = p + at;
        while (s < end && (*s == '\n' || *s == '\r')) ++s;
        if (s >= end) return false;
        const bool fq = *s == '@';
        if (!fq && *s != '>') die("malformed record in the reads file");
        const char* e1 = eol(s, end);
        const char* w = s + 1;
        while (w < e1 && !isspace((unsigned char)*w)) ++w;
        b.names.insert(b.names.end(), (const uint8_t*)s + 1, (const uint8_t*)w);
        b.name_off.push_back(b.names.size());
        const char* q = e1 < end ? e1 + 1 : end;
        const char* e2 = eol(q, end);
        size_t slen = (size_t)(e2 - q);
        if (slen && q[slen - 1] == '\r') --slen;
        b.seq.insert(b.seq.end(), (const uint8_t*)q, (const uint8_t*)q + slen);
        b.off.push_back(b.seq.size());
        const char* nx = e2 < end ? e2 + 1 : end;
        if (fq) {
            const char* e3 = eol(nx, end);                     // '+' line
            const char* ql = e3 < end ? e3 + 1 : end;
            const char* e4 = eol(ql, end);
            size_t qlen = (size_t)(e4 - ql);
            if (qlen && ql[qlen - 1] == '\r') --qlen;
            if (qlen != slen) die("truncated quality string");
            b.qual.insert(b.qual.end(), (const uint8_t*)ql, (const uint8_t*)ql + qlen);
            nx = e4 < end ? e4 + 1 : end;
        } else {
            b.has_qual = false;
            b.qual.resize(b.seq.size(), (uint8_t)'*');
        }
        at = (size_t)(nx - p);
        return true;
    }
};

struct Args {
    std::string filename, patterns, mate1, mate2, output;
    size_t b = 512, th = 1;
    moni_align_params_t P;
    bool report_mems = false, csv = false, no_lcp = false, shaped_slp = false, secondary = false;
    bool legacy_ms = false, legacy_mems = false;      // --ms / --mems
    bool split = false; uint32_t seg_len = 0, overlap = 0; bool seg_len_set = false, overlap_set = false;      // --ms / --mems --split [--seg-len N] [--overlap N]: long patterns, moni_ms_long_batch
    bool extend = false;                              // --extend: the legacy `moni extend` (longest MEM of each strand, extended to both sides)
    bool pseudo_ms = false;                           // --pseudo-ms: the legacy `moni pseudo-ms` (pseudo-matching lengths of every read)
    bool screen = false, one_strand = false, screen_opt = false; moni_screen_params_t SP;      // --screen [--window N] [--min-win N] [--ks NUM/DEN] [--one-strand]: present / absent calls (screen_opt: one of its options was given)
    bool locate = false, both_strands = false;        // --locate [--both-strands]: exact-match count and locate of every pattern
    uint32_t max_occ = 0;                             // --max-occ: positions listed per pattern and strand (0: counts alone)
    bool seq_count = false;                           // --seq-count [--both-strands] [--max-walk N]: per-sequence occurrence counts of every pattern
    bool loci = false, no_lift = false;               // --loci [--both-strands] [--max-walk N] [--no-lift]: the reference loci of every pattern
    uint64_t max_walk = 1ull << 20; bool max_walk_set = false;      // --max-walk: patterns with more occurrences are counted, not enumerated (0: no limit)
    bool approx = false; uint32_t approx_k = 0;      // --approx K [--max-hits N] [--max-occ N] [--both-strands] [--max-steps N]: count and locate within K substitutions
    uint32_t max_hits = 16; bool max_hits_set = false;      // --max-hits: matching strings listed per pattern and strand
    uint64_t max_steps = MONI_APPROX_MAX_STEPS_DEFAULT; bool max_steps_set = false;      // --max-steps: backward-search steps per piece of a search tree (0: no limit)
    int gpus = 1;
    size_t gpu_batch = 1048576;
    int ctx_per_gpu = 3;               // streaming path: contexts (ranges in flight) per GPU
    bool host_inflate = false;         // --host-inflate: BGZF input through zlib on the host (the record-by-record Reader), as plain gzip goes
    size_t inflate_blocks = 4096;      // --inflate-blocks: BGZF members per moni_bgzf_inflate call (4096: about 256 MB of text)
    std::string interleaved;           // --interleaved FILE.bam: pairs from one name-grouped BAM (unaligned BAM, samtools collate): first mate, second mate
    bool dry_run = false;
    bool dry_write = false;     // --dry-run-write: no GPU, but the single-end front end's batching runs - ranges, workers of all (absent) GPUs, blocks placed in input order - with placeholder records
    moni_pe_params_t PE;               // -d, -D (paired-end)
    bool find_orphan = true;           // -u switches orphan recovery off
    bool bam = false;                  // --bam: the SAM lines as BAM records in BGZF blocks in <out>.bam, encoded and deflated on the GPU by the context that aligned them (moni_bam_records)
    bool sort = false;                 // --sort (with --bam): the records in coordinate order, with <out>.bam.bai beside them
    uint64_t sort_chunk = 256ull << 20; bool sort_chunk_set = false;      // --sort-chunk: uncompressed bytes of a chunk of the merge
    bool mark_dup = false;             // --mark-dup (with --sort): duplicates flagged 0x400 on the GPU between the two phases of the sort
    bool coverage = false;             // --coverage (with --sort): depth of coverage of the sorted records, added on the GPU as the chunks are merged
    uint32_t cov_window = 0, cov_mapq = 0; bool cov_window_set = false, cov_mapq_set = false; bool cov_window_bad = false, cov_mapq_bad = false;      // --cov-window N, --cov-mapq Q
    bool bgzf = false;                 // --bgzf: the SAM text as BGZF blocks in <out>.gz, deflated on the GPU by the context that aligned it (moni_bgzf_compress)
};

static void parse(int argc, char** argv, Args& a) {
    moni_align_params_default(&a.P);
    moni_pe_params_default(&a.PE);
    moni_screen_params_default(&a.SP);
    a.P.n_seeds_thr = 5000; a.P.freq_thr = 0.30;          // struct defaults of align_full_ksw2.cpp:70,73 (the wrapper always passes -S/-F)
    std::vector<char*> av;
    for (int i = 0; i < argc; ++i) {
        if (!strcmp(argv[i], "--gpus") && i + 1 < argc) { a.gpus = atoi(argv[++i]); continue; }
        if (!strcmp(argv[i], "--gpu-batch") && i + 1 < argc) { a.gpu_batch = strtoull(argv[++i], nullptr, 10); continue; }
        if (!strcmp(argv[i], "--dry-run")) { a.dry_run = true; continue; }
        if (!strcmp(argv[i], "--dry-run-write")) { a.dry_run = true; a.dry_write = true; continue; }
        if (!strcmp(argv[i], "--ctx-per-gpu") && i + 1 < argc) { a.ctx_per_gpu = std::max(1, atoi(argv[++i])); continue; }
        if (!strcmp(argv[i], "--bgzf")) { a.bgzf = true; continue; }
        if (!strcmp(argv[i], "--host-inflate")) { a.host_inflate = true; continue; }
        if (!strcmp(argv[i], "--interleaved") && i + 1 < argc) { a.interleaved = argv[++i]; continue; }
        if (!strcmp(argv[i], "--inflate-blocks") && i + 1 < argc) { a.inflate_blocks = std::max<size_t>(1, strtoull(argv[++i], nullptr, 10)); continue; }
        if (!strcmp(argv[i], "--bam")) { a.bam = true; continue; }
        if (!strcmp(argv[i], "--sort")) { a.sort = true; continue; }
        if (!strcmp(argv[i], "--mark-dup")) { a.mark_dup = true; continue; }
        if (!strcmp(argv[i], "--coverage")) { a.coverage = true; continue; }
        if (!strcmp(argv[i], "--cov-window") && i + 1 < argc) { const unsigned long long v = strtoull(argv[++i], nullptr, 10); a.cov_window = (uint32_t)v; a.cov_window_set = true; a.cov_window_bad = v < 1 || v >= (1ull << 31); continue; }
        if (!strcmp(argv[i], "--cov-mapq") && i + 1 < argc) { const unsigned long long v = strtoull(argv[++i], nullptr, 10); a.cov_mapq = (uint32_t)v; a.cov_mapq_set = true; a.cov_mapq_bad = v > 255; continue; }
        if (!strcmp(argv[i], "--sort-chunk") && i + 1 < argc) { a.sort_chunk = strtoull(argv[++i], nullptr, 10); a.sort_chunk_set = true; continue; }
        if (!strcmp(argv[i], "--ms")) { a.legacy_ms = true; continue; }
        if (!strcmp(argv[i], "--mems")) { a.legacy_mems = true; continue; }
        if (!strcmp(argv[i], "--split")) { a.split = true; continue; }
        if (!strcmp(argv[i], "--seg-len") && i + 1 < argc) { a.seg_len = (uint32_t)strtoul(argv[++i], nullptr, 10); a.seg_len_set = true; continue; }
        if (!strcmp(argv[i], "--overlap") && i + 1 < argc) { a.overlap = (uint32_t)strtoul(argv[++i], nullptr, 10); a.overlap_set = true; continue; }
        if (!strcmp(argv[i], "--extend")) { a.extend = true; continue; }
        if (!strcmp(argv[i], "--pseudo-ms")) { a.pseudo_ms = true; continue; }
        if (!strcmp(argv[i], "--screen")) { a.screen = true; continue; }
        if (!strcmp(argv[i], "--window") && i + 1 < argc) { a.SP.window = (uint32_t)strtoul(argv[++i], nullptr, 10); a.screen_opt = true; continue; }
        if (!strcmp(argv[i], "--min-win") && i + 1 < argc) { a.SP.min_win = (uint32_t)strtoul(argv[++i], nullptr, 10); a.screen_opt = true; continue; }
        if (!strcmp(argv[i], "--ks") && i + 1 < argc) {          // NUM/DEN
            char* e = nullptr;
            a.SP.ks_num = (uint32_t)strtoul(argv[++i], &e, 10);
            a.SP.ks_den = *e == '/' ? (uint32_t)strtoul(e + 1, nullptr, 10) : 0;
            a.screen_opt = true; continue;
        }
        if (!strcmp(argv[i], "--one-strand")) { a.one_strand = true; a.screen_opt = true; continue; }
        if (!strcmp(argv[i], "--locate")) { a.locate = true; continue; }
        if (!strcmp(argv[i], "--seq-count")) { a.seq_count = true; continue; }
        if (!strcmp(argv[i], "--loci")) { a.loci = true; continue; }
        if (!strcmp(argv[i], "--no-lift")) { a.no_lift = true; continue; }
        if (!strcmp(argv[i], "--max-walk") && i + 1 < argc) { a.max_walk = strtoull(argv[++i], nullptr, 10); a.max_walk_set = true; continue; }
        if (!strcmp(argv[i], "--approx") && i + 1 < argc) { a.approx = true; a.approx_k = (uint32_t)strtoul(argv[++i], nullptr, 10); continue; }
        if (!strcmp(argv[i], "--max-hits") && i + 1 < argc) { a.max_hits = (uint32_t)strtoul(argv[++i], nullptr, 10); a.max_hits_set = true; continue; }
        if (!strcmp(argv[i], "--max-steps") && i + 1 < argc) { a.max_steps = strtoull(argv[++i], nullptr, 10); a.max_steps_set = true; continue; }
        if (!strcmp(argv[i], "--both-strands")) { a.both_strands = true; continue; }
        if (!strcmp(argv[i], "--max-occ") && i + 1 < argc) { a.max_occ = (uint32_t)strtoul(argv[++i], nullptr, 10); continue; }
        av.push_back(argv[i]);
    }
    const std::string usage = "usage: " + std::string(argv[0]) + " infile [-p patterns] [-o output] [-t threads] [-b batch] [-l len] [-L ext_l] [-A smatch] "
                              "[-B smismatch] [-O gapo] [-E gape] [-s seeds_dis] [-f freq_dis] [-S seeds_thr] [-F freq_thr] [-w max_iter] [-v max_pred] "
                              "[-x max_dist_x] [-y max_dist_y] [-k min_chain_mem] [-j min_chain_score] [-a chain_dis] [--gpus N] [--gpu-batch reads] [--bgzf] [--bam] [--sort [--sort-chunk BYTES]] [--mark-dup] [--coverage [--cov-window N] [--cov-mapq Q]] [--host-inflate] [--inflate-blocks N] [--interleaved FILE.bam] [--ms | --mems [--split [--seg-len N] [--overlap N]] | --extend | --pseudo-ms | --screen [--window N] [--min-win N] [--ks NUM/DEN] [--one-strand] | --locate [--max-occ N] [--both-strands] | --seq-count [--max-walk N] [--both-strands] | --loci [--max-walk N] [--both-strands] [--no-lift] | --approx K [--max-hits N] [--max-occ N] [--both-strands] [--max-steps N]]\n"
                              "  --split: patterns of genome length, cut into segments of --seg-len bases walked side by side; .lengths / .mems are identical to the run without it, .pointers may name other positions of the same matches\n"
                              "  --bgzf: the SAM output (single end, -1 / -2, -m, --extend) as blocked gzip in <output>.gz, compressed on the GPU; samtools, htslib and bgzip -d read it as SAM\n"
                              "  --host-inflate: BGZF (blocked gzip) input of single-end and -1 / -2 alignment is inflated on the GPU; this option sends it through zlib on the host, as plain gzip, -m, -c, --extend, the legacy and pattern-query modes and FASTA with wrapped lines always go\n"
                              "  --inflate-blocks N: BGZF members inflated per call (4096, about 256 MB of text)\n"
                              "  -p / -1 / -2 FILE.bam: BAM input, unaligned or aligned: the records are found and turned into reads on the GPU; every primary record with bases is a read (as sequenced: reverse-strand records are turned back), secondary and supplementary records are skipped, tags are dropped\n"
                              "  --interleaved FILE.bam: pairs from one BAM grouped by name (unaligned BAM, samtools collate): first mate, then second mate; in place of -1 / -2\n"
                              "  --bam: the SAM output (the same four modes) as BAM in <output>.bam (a trailing .sam becomes .bam): header and records encoded and compressed on the GPU, unsorted, no index\n"
                              "  --sort: with --bam, the records in coordinate order (samtools sort's: reference, position, forward strand first; ties keep input order) under @HD SO:coordinate, and the index in <output>.bam.bai; sorted on the GPU, merged through a temporary file beside the output\n"
                              "  --sort-chunk BYTES: uncompressed bytes of the records sorted and compressed per call in the merge (268435456; at least 65536)\n"
                              "  --mark-dup: with --sort (single end and -1 / -2), duplicates get flag 0x400 (Picard's rule on unclipped 5' ends, strands and the sum of base qualities of 15 and more; no optical duplicates, no UMIs): signatures on the GPU while a batch's records are still there, one resolve over all batches between the two phases of the sort, the flags set as the chunks are merged\n"
                              "  --coverage: with --sort, the depth of coverage of the sorted records (mosdepth --fast-mode with deletions counted: no mate-overlap correction; records with flag & 1796 are skipped, so --mark-dup's duplicates do not count): added on the GPU while a chunk of the merge is still there; <output>.bam.mosdepth.summary.txt and <output>.bam.per-base.bed.gz, and with --cov-window N the windows' mean depth in <output>.bam.regions.bed.gz; 4 bytes of the GPU's memory per reference base, one GPU\n"
                              "  --cov-window N: with --coverage, windows of N bases (1 to 2147483647)\n"
                              "  --cov-mapq Q: with --coverage, records with a mapping quality below Q are skipped (0 to 255; 0)\n";
    int c;
    char* s;
    optind = 1;
    while ((c = getopt((int)av.size(), av.data(), "ql:hp:o:t:1:2:b:A:B:O:E:L:dsfnD:S:F:w:v:x:y:k:j:Zaumc")) != -1) {
        switch (c) {
            case 'p': a.patterns = optarg; break;
            case 'o': a.output = optarg; break;
            case '1': a.mate1 = optarg; break;
            case '2': a.mate2 = optarg; break;
            case 'l': a.P.min_len = (uint32_t)std::stoi(optarg); break;
            case 'b': a.b = (size_t)std::stoi(optarg); break;
            case 't': a.th = (size_t)std::stoi(optarg); break;
            case 'L': a.P.ext_len = (uint32_t)std::stoi(optarg); break;
            case 'A': a.P.smatch = (int8_t)std::stoi(optarg); break;
            case 'B': a.P.smismatch = (int8_t)std::stoi(optarg); break;
            case 'd': a.PE.filter_dir = 0; break;              // filter_dir off (align_full_ksw2.cpp:189-191)
            case 's': a.P.filter_seeds = 0; break;
            case 'f': a.P.filter_freq = 0; break;
            case 'n': a.no_lcp = true; break;
            case 'D': a.PE.dir_thr = std::stoi(optarg); break;  // dir_thr (parsed with stoi, align_full_ksw2.cpp:195-198)
            case 'S': a.P.n_seeds_thr = (uint32_t)std::stoi(optarg); break;
            case 'F': a.P.freq_thr = std::stod(optarg); break;
            case 'O': a.P.gapo = a.P.gapo2 = (int8_t)strtol(optarg, &s, 10); if (*s == ',') a.P.gapo2 = (int8_t)strtol(s + 1, &s, 10); break;
            case 'E': a.P.gape = a.P.gape2 = (int8_t)strtol(optarg, &s, 10); if (*s == ',') a.P.gape2 = (int8_t)strtol(s + 1, &s, 10); break;
            case 'q': a.shaped_slp = true; break;
            case 'w': a.P.max_iter = std::stoi(optarg); break;
            case 'v': a.P.max_pred = std::stoi(optarg); break;
            case 'x': a.P.max_dist_x = std::stoi(optarg); break;
            case 'y': a.P.max_dist_y = std::stoi(optarg); break;
            case 'k': a.P.min_chain_length = std::stoi(optarg); break;
            case 'j': a.P.min_chain_score = std::stoi(optarg); break;
            case 'Z': a.secondary = true; break;
            case 'a': a.P.left_mem_check = 0; break;
            case 'u': a.find_orphan = false; break;
            case 'm': a.report_mems = true; break;
            case 'c': a.csv = true; break;
            case 'h': die(usage);
            default: die("Unknown option.\n" + usage);
        }
    }
    if ((int)av.size() == optind + 1) a.filename = av[optind];
    else die("Invalid number of arguments\n" + usage);
    if (a.th > 1) a.P.host_threads = (uint32_t)a.th;
}

// what --dry-run says of the output's kind
static const char* output_word(const Args& a) {
    return a.bgzf ? " bgzf=1" : !a.bam ? "" : !a.sort ? " bam=1" : a.mark_dup ? (a.coverage ? " bam=1 sort=1 markdup=1 coverage=1" : " bam=1 sort=1 markdup=1") : a.coverage ? " bam=1 sort=1 coverage=1" : " bam=1 sort=1";
}

// ---- the output of a run that writes SAM ------------------------------------------------------------------------------------------------
// Placer: blocks that come in any order land in one file in the order of their ids, each at the prefix sum of the lengths before it.
struct Placer {
    int fd = -1;
    uint64_t end = 0;               // behind everything appended or placed so far
    std::mutex mu; std::condition_variable cv;
    std::vector<uint64_t> slot;     // of an id: ~0, then the length it reported, then - once all ids before it have reported - its place
    size_t upto = 0;                // the ids below have their place
    void open(const std::string& path) {
        fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) die("open() file " + path + " failed");
    }
    // a block behind the rest: for the one thread that writes before the placing starts, after it has ended, or instead of it
    void append(const void* p, uint64_t n) { pwrite_all(fd, (const char*)p, n, end); end += n; }
    // block `id` has `len` bytes: waits until every earlier id has reported and returns where the block goes.  The ids count from 0; how many come need not be known.
    uint64_t place(size_t id, uint64_t len) {
        std::unique_lock<std::mutex> lk(mu);
        if (slot.size() <= id) slot.resize(id + 1, ~0ull);
        slot[id] = len;
        for (; upto < slot.size() && slot[upto] != ~0ull; ++upto) { const uint64_t l = slot[upto]; slot[upto] = end; end += l; }
        cv.notify_all();
        cv.wait(lk, [&] { return upto > id; });
        return slot[id];
    }
    // the block at its place, in P slices side by side
    void write(const char* p, uint64_t len, uint64_t at, int P) const {
        if (!len) return;
        std::vector<std::thread> th;
        const size_t sl = (len + P - 1) / P;
        for (int i = 1; i < P; ++i) { const size_t lo = std::min<size_t>(len, sl * i), hi = std::min<size_t>(len, sl * (i + 1)); if (hi > lo) th.emplace_back(pwrite_all, fd, p + lo, hi - lo, at + lo); }
        pwrite_all(fd, p, std::min<size_t>(len, sl), at);
        for (auto& t : th) t.join();
    }
    void close(const char* msg) { if (::close(fd) != 0) die(msg); fd = -1; }
};

// Sink: the file of a SAM-writing run in the flavour the flags ask for - the text, the text as BGZF blocks (--bgzf), BAM (--bam), or coordinate-sorted BAM with
// its index (--sort, with duplicates marked under --mark-dup).  All three pipelines (pairs, single-end streaming, single-end queue) write through it: begin,
// encode per batch, the block placed (Placer) or appended, finish.  A new flavour is added here and nowhere else.
struct Block { const char* p; uint64_t n; };
struct Sink : Placer {
    bool bgzf = false, bam = false, sort = false;
    uint64_t sort_chunk = 0;
    std::string path, header;       // header: the SAM header whose @SQ lines are the BAM dictionary (under --sort with SO:coordinate)
    SortedBam sorted;               // --sort: a batch is a run; nothing but the header reaches the file before finish

    // `len` bytes of text as BGZF blocks, in the context's pinned buffer until its next call; eof: the end-of-file block behind them
    static Block bgzf_blocks(moni_ctx_t* c, const char* text, uint64_t len, bool eof) {
        moni_bgzf_params_t bp; moni_bgzf_params_default(&bp);
        bp.eof = eof ? 1 : 0;
        const uint8_t* o = nullptr; uint64_t zl = 0;
        const int rc = moni_bgzf_compress(c, text, len, &bp, &o, &zl, nullptr);
        if (rc) die("moni_bgzf_compress failed (" + std::to_string(rc) + ")");
        return {(const char*)o, zl};
    }
    // `len` bytes of SAM lines as BAM records in BGZF blocks (moni_bam_records, against the dictionary set on this context), in the context's pinned buffer until its next call
    static Block bam_blocks(moni_ctx_t* c, const char* text, uint64_t len) {
        moni_bam_params_t bp; moni_bam_params_default(&bp);
        const uint8_t* o = nullptr; uint64_t zl = 0;
        moni_bam_stats_t st;
        const int rc = moni_bam_records(c, text, len, &bp, &o, &zl, &st);
        if (rc == MONI_EINVAL && st.bad_lines)
            die("moni_bam_records: " + std::to_string(st.bad_lines) + " line(s) of a batch cannot be written as BAM records; the first is its line " + std::to_string(st.first_bad_line) +
                " (reason " + std::to_string(st.bad_reason) + " of MONI_BAM_*)");
        if (rc) die("moni_bam_records failed (" + std::to_string(rc) + ")");
        return {(const char*)o, zl};
    }

    void open(const std::string& file, const Args& a, bool paired) {
        path = file; bgzf = a.bgzf; bam = a.bam; sort = a.sort; sort_chunk = a.sort_chunk;
        sorted.mark = a.mark_dup; sorted.paired = paired ? 1 : 0;
        sorted.cover.on = a.coverage; sorted.cover.window = a.cov_window; sorted.cover.min_mapq = a.cov_mapq;
        Placer::open(file);
    }
    // --bam: the header becomes the dictionary of every context that will encode records; returns the BAM header, in cs[0]'s buffer.  begin calls it; a pipeline
    // that makes further contexts behind begin calls it for those.
    Block set_dictionary(const std::vector<moni_ctx_t*>& cs) const {
        const uint8_t* bh = nullptr; uint64_t bhl = 0;
        for (size_t k = cs.size(); bam && k-- > 0;)
            if (moni_bam_set_header(cs[k], header.data(), header.size(), &bh, &bhl)) die("moni_bam_set_header failed: the SAM header's @SQ lines do not make a BAM dictionary");
        return {(const char*)bh, bhl};
    }
    // the header at the start of the file, in the flavour's form (blocks of its own, made on cs[0] before the workers take the contexts); `end` is where the body starts
    void begin(moni_index_t* idx0, const std::vector<moni_ctx_t*>& cs) {
        char* h; uint64_t hl; if (moni_sam_header(idx0, &h, &hl)) die("header");
        Block z{h, hl};
        if (bgzf) z = bgzf_blocks(cs[0], h, hl, false);
        if (bam) {
            header.assign(h, hl);
            const size_t at = sort ? header.find("SO:unknown") : std::string::npos;
            if (at != std::string::npos && header.compare(0, 3, "@HD") == 0 && at < header.find('\n')) header.replace(at, 10, "SO:coordinate");
            z = set_dictionary(cs);
            z = bgzf_blocks(cs[0], z.p, z.n, false);
        }
        append(z.p, z.n);
        moni_free(h);
        if (sort) sorted.open(path, sort_chunk, header);
    }
    // what goes into the file for a batch's text: the text itself, its blocks in c's pinned buffer (valid until c's next library call), or nothing - the batch
    // became run `run_id` of the sort
    Block encode(moni_ctx_t* c, size_t run_id, const char* text, uint64_t len) {
        if (sort) { sorted.add_run(c, run_id, text, len); return {nullptr, 0}; }
        if (bam) return bam_blocks(c, text, len);
        if (bgzf) return bgzf_blocks(c, text, len, false);
        return {text, len};
    }
    // behind the last batch: the merged chunks and the index of the sort over all contexts, the end-of-file block of the block flavours, the close
    void finish(const std::vector<moni_ctx_t*>& cs) {
        if (sort) end = sorted.finish(cs, fd, end);
        if (bgzf || bam) { const Block z = bgzf_blocks(cs[0], nullptr, 0, true); append(z.p, z.n); }
        close("closing the output file failed (output incomplete)");
    }
};


// The files of --coverage.  The per-base text comes in pieces from moni_cov_next and goes through the blocks of --bgzf; the regions are formatted
// here from the windows' sums, a reference at a time.
static void write_coverage(moni_ctx_t* c, moni_cov_t* cov, const CoverageOut& co, const std::string& bam_path, const std::string& header, uint64_t counted, uint64_t records) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::string> names;          // the first SN: of every @SQ line, as the dictionary takes it
    for (size_t at = 0; at < header.size();) {
        const size_t e = std::min(header.find('\n', at), header.size());
        for (size_t f = at + 4; !header.compare(at, 4, "@SQ\t") && f < e;) {
            const size_t g = std::min(header.find('\t', f), e);
            if (!header.compare(f, 3, "SN:")) { names.push_back(header.substr(f + 3, g - f - 3)); break; }
            f = g + 1;
        }
        at = e + 1;
    }
    const moni_cov_ref_t* refs = nullptr; uint32_t n_ref = 0;
    int rc = moni_cov_seal(c, cov, &refs, &n_ref);
    if (rc) die("moni_cov_seal failed (" + std::to_string(rc) + ")");
    if (names.size() != n_ref) die("--coverage: the header's @SQ lines and the dictionary disagree");
    auto open_out = [](const std::string& p) { FILE* f = fopen(p.c_str(), "w"); if (!f) die("open() file " + p + " failed"); return f; };
    char line[512];
    // the summary
    uint64_t t_len = 0, t_bases = 0; uint32_t t_min = n_ref ? 0xFFFFFFFFu : 0u, t_max = 0;
    {
        FILE* f = open_out(bam_path + ".mosdepth.summary.txt");
        std::string out = "chrom\tlength\tbases\tmean\tmin\tmax\n";
        for (uint32_t r = 0; r < n_ref; ++r) {
            snprintf(line, sizeof line, "\t%llu\t%llu\t%.2f\t%u\t%u\n", (unsigned long long)refs[r].length, (unsigned long long)refs[r].bases, (double)refs[r].bases / (double)refs[r].length, refs[r].min, refs[r].max);
            out += names[r] + line;
            t_len += refs[r].length; t_bases += refs[r].bases; t_min = std::min(t_min, refs[r].min); t_max = std::max(t_max, refs[r].max);
        }
        snprintf(line, sizeof line, "total\t%llu\t%llu\t%.2f\t%u\t%u\n", (unsigned long long)t_len, (unsigned long long)t_bases, t_len ? (double)t_bases / (double)t_len : 0.0, t_min, t_max);
        out += line;
        put(out.data(), out.size(), f);
        close_out(f);
    }
    // the per-base text
    uint64_t n_lines = 0;
    {
        FILE* f = open_out(bam_path + ".per-base.bed.gz");
        for (int done = 0; !done;) {
            const char* t = nullptr; uint64_t tl = 0;
            rc = moni_cov_next(c, cov, co.max_bases, co.max_lines, &t, &tl, &done);
            if (rc) die("moni_cov_next failed (" + std::to_string(rc) + ")");
            n_lines += (uint64_t)std::count(t, t + tl, '\n');
            const Block z = Sink::bgzf_blocks(c, t, tl, false);
            put(z.p, z.n, f);
        }
        const Block z = Sink::bgzf_blocks(c, nullptr, 0, true);
        put(z.p, z.n, f);
        close_out(f);
    }
    // the regions
    if (co.window) {
        FILE* f = open_out(bam_path + ".regions.bed.gz");
        std::string out;
        auto flush = [&](bool eof) { const Block z = Sink::bgzf_blocks(c, out.data(), out.size(), eof); put(z.p, z.n, f); out.clear(); };
        for (uint32_t r = 0; r < n_ref; ++r) {
            const uint64_t* sums = nullptr; uint64_t nw = 0;
            rc = moni_cov_windows(c, cov, r, co.window, &sums, &nw);
            if (rc) die("moni_cov_windows failed (" + std::to_string(rc) + ")");
            for (uint64_t k = 0; k < nw; ++k) {
                const uint64_t a = k * co.window, b = std::min<uint64_t>(a + co.window, refs[r].length);
                snprintf(line, sizeof line, "\t%llu\t%llu\t%.2f\n", (unsigned long long)a, (unsigned long long)b, (double)sums[k] / (double)(b - a));
                out += names[r]; out += line;
                if (out.size() >= (32u << 20)) flush(false);
            }
        }
        flush(true);
        close_out(f);
    }
    snprintf(line, sizeof line, "%.2f", t_len ? (double)t_bases / (double)t_len : 0.0);
    info("Coverage: " + std::to_string(counted) + " counted of " + std::to_string(records) + " records, mean depth " + line + " over " + std::to_string(t_len) + " bases of " +
         std::to_string(n_ref) + " references; " + std::to_string(n_lines) + " per-base lines in " + std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()) + " s: " + bam_path + ".per-base.bed.gz");
}

// ---- streaming path for plain files ---------------------------------------------------------------------------------------------------
namespace fastpath {

static inline const char* next_line(const char* s, const char* end) { const char* e = (const char*)memchr(s, '\n', (size_t)(end - s)); return e ? e + 1 : end; }

// the first record that starts at or after s.  Four-line FASTQ: a line that starts with '@' whose second-next line starts with '+'
// (a quality line may start with '@', but then the second-next line is a sequence); FASTA: a line that starts with '>'.
static const char* align_record(const char* s, const char* base, const char* end, bool fq) {
    if (s <= base) return base;
    if (s >= end) return end;
    s = next_line(s - 1, end);
    while (s < end) {
        if (fq) {
            if (*s == '@') { const char* l3 = next_line(next_line(s, end), end); if (l3 < end && *l3 == '+') return s; }
        } else if (*s == '>') return s;
        s = next_line(s, end);
    }
    return end;
}

struct Count { size_t n = 0, seq = 0, name = 0; };
struct Raw {          // uninitialised grow-only bytes (a vector would zero 300 MB per batch)
    uint8_t* p = nullptr; size_t cap = 0;
    void ensure(size_t n) { if (n > cap) { free(p); cap = n + n / 8 + 64; p = (uint8_t*)malloc(cap); if (!p) die("out of memory"); } }
    ~Raw() { free(p); }
};

// one pass over the records of [a, b): FILL = false counts, FILL = true writes them at the given cursors
template <bool FILL>
static Count walk(const char* a, const char* b, bool fq, uint8_t* seq, uint8_t* qual, uint8_t* names, uint64_t* off, uint64_t* name_off,
                  uint64_t seq_at, uint64_t name_at) {
    Count c;
    const char* s = a;
    while (s < b) {
        while (s < b && (*s == '\n' || *s == '\r')) ++s;
        if (s >= b) break;
        if (*s != (fq ? '@' : '>')) die("malformed record in the reads file");
        const char* e1 = (const char*)memchr(s, '\n', (size_t)(b - s)); if (!e1) e1 = b;
        const char* w = s + 1;
        while (w < e1 && !isspace((unsigned char)*w)) ++w;
        const size_t nl = (size_t)(w - (s + 1));
        const char* q = e1 < b ? e1 + 1 : b;
        const char* e2 = (const char*)memchr(q, '\n', (size_t)(b - q)); if (!e2) e2 = b;
        size_t sl = (size_t)(e2 - q);
        if (sl && q[sl - 1] == '\r') --sl;
        const char* nx = e2 < b ? e2 + 1 : b;
        const char* ql = nullptr;
        if (fq) {
            const char* e3 = (const char*)memchr(nx, '\n', (size_t)(b - nx)); if (!e3) e3 = b;
            ql = e3 < b ? e3 + 1 : b;
            const char* e4 = (const char*)memchr(ql, '\n', (size_t)(b - ql)); if (!e4) e4 = b;
            size_t qn = (size_t)(e4 - ql);
            if (qn && ql[qn - 1] == '\r') --qn;
            if (qn != sl) die("truncated quality string");
            nx = e4 < b ? e4 + 1 : b;
        }
        if (FILL) {
            memcpy(names + name_at + c.name, s + 1, nl);
            memcpy(seq + seq_at + c.seq, q, sl);
            if (fq) memcpy(qual + seq_at + c.seq, ql, sl); else memset(qual + seq_at + c.seq, '*', sl);
            off[c.n + 1] = seq_at + c.seq + sl; name_off[c.n + 1] = name_at + c.name + nl;
        }
        c.n++; c.seq += sl; c.name += nl;
        s = nx;
    }
    return c;
}

struct ParsedBatch {
    Raw seq, qual, names;
    std::vector<uint64_t> off, name_off;
    size_t n = 0;
};

static void parse_range(const char* a, const char* b, const char* base, const char* end, bool fq, int P, ParsedBatch& B) {
    std::vector<const char*> cut(P + 1);
    cut[0] = a; cut[P] = b;
    for (int i = 1; i < P; ++i) { cut[i] = align_record(a + (size_t)(b - a) / P * i, base, end, fq); if (cut[i] > b) cut[i] = b; if (cut[i] < cut[i - 1]) cut[i] = cut[i - 1]; }
    std::vector<Count> cnt(P);
    auto run = [&](auto&& fn) {
        std::vector<std::thread> th;
        for (int i = 1; i < P; ++i) th.emplace_back(fn, i);
        fn(0);
        for (auto& t : th) t.join();
    };
    run([&](int i) { cnt[i] = walk<false>(cut[i], cut[i + 1], fq, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0); });
    std::vector<size_t> n_at(P + 1, 0), s_at(P + 1, 0), m_at(P + 1, 0);
    for (int i = 0; i < P; ++i) { n_at[i + 1] = n_at[i] + cnt[i].n; s_at[i + 1] = s_at[i] + cnt[i].seq; m_at[i + 1] = m_at[i] + cnt[i].name; }
    B.n = n_at[P];
    B.seq.ensure(s_at[P] + 16); B.qual.ensure(s_at[P] + 16); B.names.ensure(m_at[P] + 16);
    if (B.off.size() < B.n + 1) { B.off.resize(B.n + 1 + B.n / 8); B.name_off.resize(B.n + 1 + B.n / 8); }
    B.off[0] = 0; B.name_off[0] = 0;
    run([&](int i) { walk<true>(cut[i], cut[i + 1], fq, B.seq.p, B.qual.p, B.names.p, B.off.data() + n_at[i], B.name_off.data() + n_at[i], s_at[i], m_at[i]); });
}

// the end of the n_rec-th record from s in a mapped four-line FASTQ file (or the end of the file; got = the records before it): the newlines of a
// window are counted by P threads side by side, the slice in which the count is reached is scanned
static const char* skip_records(const char* s, const char* end, size_t n_rec, int P, size_t& got) {
    size_t need = 4 * n_rec, lines = 0;
    const char* cur = s;
    while (need > 0 && cur < end) {
        const size_t win = std::min<size_t>((size_t)(end - cur), std::max<size_t>((size_t)1 << 20, need * 48));
        std::vector<size_t> cnt(P, 0);
        auto count = [&](int i) {
            const char* a = cur + win / P * i; const char* b = i + 1 == P ? cur + win : cur + win / P * (i + 1);
            size_t c = 0;
            while (a < b) { const char* e = (const char*)memchr(a, '\n', (size_t)(b - a)); if (!e) break; ++c; a = e + 1; }
            cnt[i] = c;
        };
        { std::vector<std::thread> th; for (int i = 1; i < P; ++i) th.emplace_back(count, i); count(0); for (auto& t : th) t.join(); }
        size_t total = 0;
        for (int i = 0; i < P; ++i) total += cnt[i];
        if (total < need) { need -= total; lines += total; cur += win; continue; }
        int i = 0;
        while (cnt[i] < need) { need -= cnt[i]; lines += cnt[i]; ++i; }
        const char* a = cur + win / P * i;
        while (need > 0) { const char* e = (const char*)memchr(a, '\n', (size_t)(end - a)); a = e + 1; --need; ++lines; }
        cur = a;
    }
    if (cur >= end && end > s && end[-1] != '\n') ++lines;          // a last line without its newline
    got = lines / 4;
    return cur;
}

// n_pairs pairs from the cursors of two mapped four-line FASTQ files: both ranges parsed in two passes by P threads each (parse_range), then
// interleaved (mates 2p, 2p + 1) into uninitialised buffers
struct PairBatch { Raw seq, qual, names; std::vector<uint64_t> off, name_off; size_t n_reads = 0; };
static size_t read_pairs_fast(const char* base[2], const char* end[2], size_t at[2], size_t n_pairs, int P, ParsedBatch pb[2], PairBatch& B) {
    size_t got[2] = {0, 0};
    const char* lim[2];
    auto one = [&](int k) {
        lim[k] = skip_records(base[k] + at[k], end[k], n_pairs, P, got[k]);
        if (got[k]) parse_range(base[k] + at[k], lim[k], base[k], end[k], true, P, pb[k]); else pb[k].n = 0;
    };
    { std::thread t(one, 1); one(0); t.join(); }
    if (got[0] != got[1]) die("the mate files have different numbers of records");
    if (pb[0].n != got[0] || pb[1].n != got[1]) die("the mate files are not four-line FASTQ throughout (blank or wrapped lines): compress them or use FASTA to take the record-by-record reader");
    at[0] = (size_t)(lim[0] - base[0]); at[1] = (size_t)(lim[1] - base[1]);
    const size_t n = got[0];
    if (!n) return 0;
    B.n_reads = 2 * n;
    if (B.off.size() < 2 * n + 1) { B.off.resize(2 * n + 1); B.name_off.resize(2 * n + 1); }
    const ParsedBatch& b1 = pb[0]; const ParsedBatch& b2 = pb[1];
    B.seq.ensure(b1.off[n] + b2.off[n] + 16); B.qual.ensure(b1.off[n] + b2.off[n] + 16); B.names.ensure(b1.name_off[n] + b2.name_off[n] + 16);
    auto part = [&](size_t lo, size_t hi) {
        for (size_t p = lo; p < hi; ++p) {
            const uint64_t o1 = b1.off[p] + b2.off[p], o2 = b1.off[p + 1] + b2.off[p], m1 = b1.name_off[p] + b2.name_off[p], m2 = b1.name_off[p + 1] + b2.name_off[p];
            B.off[2 * p] = o1; B.off[2 * p + 1] = o2; B.name_off[2 * p] = m1; B.name_off[2 * p + 1] = m2;
            const size_t l1 = (size_t)(b1.off[p + 1] - b1.off[p]), l2 = (size_t)(b2.off[p + 1] - b2.off[p]);
            memcpy(B.seq.p + o1, b1.seq.p + b1.off[p], l1); memcpy(B.seq.p + o2, b2.seq.p + b2.off[p], l2);
            memcpy(B.qual.p + o1, b1.qual.p + b1.off[p], l1); memcpy(B.qual.p + o2, b2.qual.p + b2.off[p], l2);
            memcpy(B.names.p + m1, b1.names.p + b1.name_off[p], (size_t)(b1.name_off[p + 1] - b1.name_off[p]));
            memcpy(B.names.p + m2, b2.names.p + b2.name_off[p], (size_t)(b2.name_off[p + 1] - b2.name_off[p]));
        }
    };
    { std::vector<std::thread> th; for (int t = 1; t < P; ++t) th.emplace_back(part, n * t / P, n * (t + 1) / P); part(0, n / P); for (auto& t : th) t.join(); }
    B.off[2 * n] = b1.off[n] + b2.off[n]; B.name_off[2 * n] = b1.name_off[n] + b2.name_off[n];
    return n;
}

}  // namespace fastpath

// ---- BGZF input: inflated on the GPU -----------------------------------------------------------------------------------------------------
// A file of BGZF members throughout (moni_bgzf_scan takes all of it) whose text starts with a one-line FASTQ / FASTA record - the condition
// MappedReader::open applies, on the leading members inflated with zlib.  A thread with a context of its own (it never aligns, so it never makes the
// large first-call allocations) inflates `blocks` members per call in file order, puts the unfinished record of the chunk before in front, cuts
// behind the last whole record - it counts newlines; it knows the line phase because it works in order - and queues the record-aligned text.
// A file whose text starts with BAM\1 is BAM (unaligned or aligned): the same thread feeds the members to moni_bam_in_feed, which finds the records
// and writes the primary ones as FASTQ on the GPU; its text is record-aligned already, so nothing is counted or cut.  `pairs`: a name-grouped
// BAM (--interleaved) - every call gives the first mates' text and the second mates', with equal numbers of reads, in the two queues.
struct TextChunk { size_t id = 0; char* p = nullptr; size_t n = 0, cap = 0; };          // p: malloc'ed; the taker gives it back with recycle()
struct BgzfInput {
    std::string path;
    const uint8_t* z = nullptr; size_t zn = 0; int fd = -1;
    bool fq = false, bam = false, pairs = false;
    std::vector<uint64_t> cut;          // where the chunks start in the file, and its end
    moni_ctx_t* ctx = nullptr;
    std::thread th; std::mutex mu; std::condition_variable cv_put, cv_get; std::deque<TextChunk> q, q2; bool done = false;          // q2: the second mates' chunks of a BAM with pairs
    std::vector<TextChunk> pool;          // buffers that came back: a fresh 256 MB block costs its page faults, about twice the copy into it
    double t_inflate = 0, t_cut = 0, t_full = 0;          // seconds in moni_bgzf_inflate, in copying + cutting, waiting for room in the queue

    static size_t member_bytes(const uint8_t* h) {          // of a member the scan has accepted
        const uint32_t xlen = (uint32_t)h[10] | ((uint32_t)h[11] << 8);
        for (uint32_t x = 0; x + 4 <= xlen;) {
            const uint32_t slen = (uint32_t)h[12 + x + 2] | ((uint32_t)h[12 + x + 3] << 8);
            if (h[12 + x] == 'B' && h[12 + x + 1] == 'C' && slen == 2) return (size_t)((uint32_t)h[12 + x + 4] | ((uint32_t)h[12 + x + 5] << 8)) + 1;
            x += 4 + slen;
        }
        return 0;
    }
    void close() { if (z) munmap((void*)z, zn); z = nullptr; if (fd >= 0) ::close(fd); fd = -1; }
    bool open(const std::string& file) {
        path = file;
        fd = ::open(file.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size < 28) { close(); return false; }
        zn = (size_t)st.st_size;
        void* m = mmap(nullptr, zn, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { z = nullptr; close(); return false; }
        z = (const uint8_t*)m;
        uint64_t nb = 0, used = 0, text = 0;
        if (z[0] != 0x1f || z[1] != 0x8b || moni_bgzf_scan(z, zn, &nb, &used, &text) != MONI_OK || used != zn || !nb || !text) { close(); return false; }
        // the first record, from the leading members (at most 64 KB of text), through zlib
        std::vector<char> head(65536);
        size_t hn = 0, at = 0;
        auto first_record = [&]() -> int {          // 1: a one-line record, 0: not one, -1: not yet whole
            const char* p = head.data();
            if (!hn) return -1;
            if (p[0] == 'B') { if (hn < 4 && at < zn) return -1; bam = hn >= 4 && !memcmp(p, "BAM\1", 4); return bam ? 1 : 0; }
            if (p[0] != '@' && p[0] != '>') return 0;
            const char* l1 = (const char*)memchr(p, '\n', hn);
            if (!l1) return -1;
            const char* l2 = (const char*)memchr(l1 + 1, '\n', hn - (size_t)(l1 + 1 - p));
            if (!l2) return -1;
            if (l2 + 1 >= p + hn) return p[0] == '>' && at >= zn ? 1 : -1;          // (a FASTA file of one record)
            return l2[1] == (p[0] == '@' ? '+' : '>') ? 1 : 0;          // FASTA: a third line that is no header is a wrapped sequence
        };
        int ok = -1;
        while (ok < 0 && at < zn && hn < head.size()) {
            const size_t mb = member_bytes(z + at);
            z_stream zs; memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, 15 + 16) != Z_OK) break;
            zs.next_in = const_cast<Bytef*>(z + at); zs.avail_in = (uInt)mb;
            zs.next_out = (Bytef*)head.data() + hn; zs.avail_out = (uInt)(head.size() - hn);
            const int rc = inflate(&zs, Z_FINISH);
            hn += zs.total_out;
            inflateEnd(&zs);
            if (rc != Z_STREAM_END && rc != Z_BUF_ERROR && rc != Z_OK) break;
            at += mb;
            ok = first_record();
        }
        if (ok < 0 && at >= zn) ok = first_record();          // the text ends here
        if (ok != 1) { close(); return false; }
        fq = bam || head[0] == '@';
        return true;
    }
    size_t n_chunks() const { return cut.size() - 1; }
    // the chunks of `blocks` members; the thread starts
    void start(moni_index_t* idx, size_t blocks) {
        cut.assign(1, 0);
        size_t k = 0;
        for (uint64_t at = 0; at < zn;) { at += member_bytes(z + at); if (++k == blocks || at >= zn) { cut.push_back(at); k = 0; } }
        if (moni_ctx_create(idx, &ctx)) die("cannot create the inflater's context");
        th = std::thread([this] { run(); });
    }
    // the end of the last whole record of text[0, n), which holds `lines` newlines: behind the last one whose number is a multiple of `per`
    static size_t record_end(const char* text, size_t n, size_t lines, size_t per) {
        size_t skip = lines % per;
        const char* e = text + n;
        while (true) {
            const char* nl = (const char*)memrchr(text, '\n', (size_t)(e - text));
            if (!nl) return 0;
            if (!skip) return (size_t)(nl + 1 - text);
            --skip; e = nl;
        }
    }
    // a buffer of at least `need` bytes: one that came back, or a new one
    TextChunk buffer(size_t need) {
        TextChunk c;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < pool.size(); ++i) if (pool[i].cap >= need) { c = pool[i]; pool.erase(pool.begin() + i); return c; }
            if (!pool.empty()) { free(pool.back().p); pool.pop_back(); }
        }
        c.cap = need + need / 8 + 64;
        c.p = (char*)malloc(c.cap);
        if (!c.p) die("out of memory");
        return c;
    }
    void recycle(TextChunk& c) {
        if (!c.p) return;
        std::lock_guard<std::mutex> lk(mu);
        if (pool.size() < 4) pool.push_back(c); else free(c.p);
        c = TextChunk();
    }
    // out[0, n) into dst by a few threads side by side; with `lines`, the newlines of each part are counted
    static size_t copy_out(char* dst, const uint8_t* out, size_t n, bool lines) {
        const int T = 8;
        size_t cnt[T];
        auto part = [&](int i) {
            const size_t lo = n / T * i, hi = i + 1 == T ? n : n / T * (i + 1);
            if (hi > lo) memcpy(dst + lo, out + lo, hi - lo);
            cnt[i] = lines ? (size_t)std::count(dst + lo, dst + hi, '\n') : 0;
        };
        { std::vector<std::thread> t; for (int i = 1; i < T; ++i) t.emplace_back(part, i); part(0); for (auto& x : t) x.join(); }
        size_t sum = 0;
        for (int i = 0; i < T; ++i) sum += cnt[i];
        return sum;
    }
    void run_bam() {
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        static const char* const why[] = {"", "it does not start with BAM\\1", "a bad header", "a block_size outside [32, 2^28]", "fields that do not fit their record",
                                          "the primary records do not come as first mate, second mate under one name (a coordinate-sorted file? samtools collate groups it by name)", "the file ends inside a header, a record or a pair"};
        moni_bamin_params_t bp; moni_bamin_params_default(&bp);
        bp.paired = pairs ? 1 : 0;
        for (size_t id = 0; id + 1 < cut.size(); ++id) {
            const uint8_t *o1 = nullptr, *o2 = nullptr; uint64_t n1 = 0, n2 = 0, nr = 0;
            moni_bamin_stats_t st;
            const double x0 = now();
            const int rc = moni_bam_in_feed(ctx, z + cut[id], cut[id + 1] - cut[id], &bp, id + 2 == cut.size(), &o1, &n1, &o2, &n2, &nr, &st);
            if (rc == MONI_EINVAL && st.inflate.bad_blocks) die(path + ": BGZF member " + std::to_string(st.inflate.first_bad_block) + " of chunk " + std::to_string(id) + " is damaged (reason " + std::to_string(st.inflate.bad_reason) + ")");
            if (rc == MONI_EINVAL && st.bad_records) die(path + ": BAM record " + std::to_string(st.first_bad_record) + " is refused (reason " + std::to_string(st.bad_record_reason) + ": " + why[st.bad_record_reason < 7 ? st.bad_record_reason : 0] + ")");
            if (rc) die("moni_bam_in_feed failed (" + std::to_string(rc) + ")");
            const double x1 = now();
            TextChunk c = buffer((size_t)n1 + 1), c2;
            c.id = id; c.n = (size_t)n1;
            copy_out(c.p, o1, (size_t)n1, false);
            if (pairs) { c2 = buffer((size_t)n2 + 1); c2.id = id; c2.n = (size_t)n2; copy_out(c2.p, o2, (size_t)n2, false); }
            const double x2 = now();
            std::unique_lock<std::mutex> lk(mu);
            cv_put.wait(lk, [&] { return q.size() < 2 && q2.size() < 2; });
            q.push_back(c);
            if (pairs) q2.push_back(c2);
            cv_get.notify_all();
            t_inflate += x1 - x0; t_cut += x2 - x1; t_full += now() - x2;
        }
        std::lock_guard<std::mutex> lk(mu);
        done = true;
        cv_get.notify_all();
    }
    void run() {
        if (bam) return run_bam();
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        moni_inflate_params_t ip; moni_inflate_params_default(&ip);
        std::vector<char> carry;
        for (size_t id = 0; id + 1 < cut.size(); ++id) {
            const uint8_t* out = nullptr; uint64_t ol = 0;
            moni_inflate_stats_t st;
            const double x0 = now();
            const int rc = moni_bgzf_inflate(ctx, z + cut[id], cut[id + 1] - cut[id], &ip, &out, &ol, &st);
            if (rc == MONI_EINVAL && st.bad_blocks) die(path + ": BGZF member " + std::to_string(st.first_bad_block) + " of chunk " + std::to_string(id) + " is damaged (reason " + std::to_string(st.bad_reason) + ")");
            if (rc) die("moni_bgzf_inflate failed (" + std::to_string(rc) + ")");
            const double x1 = now();
            const size_t total = carry.size() + (size_t)ol;
            TextChunk c = buffer(total + 1);
            c.id = id;
            if (!carry.empty()) memcpy(c.p, carry.data(), carry.size());
            // the text out of the pinned buffer and its newlines
            const size_t lines = (size_t)std::count(carry.begin(), carry.end(), '\n') + copy_out(c.p + carry.size(), out, (size_t)ol, true);
            c.n = id + 2 == cut.size() ? total : record_end(c.p, total, lines, fq ? 4 : 2);
            carry.assign(c.p + c.n, c.p + total);
            const double x2 = now();
            std::unique_lock<std::mutex> lk(mu);
            cv_put.wait(lk, [&] { return q.size() < 2; });
            q.push_back(c);
            cv_get.notify_one();
            t_inflate += x1 - x0; t_cut += x2 - x1; t_full += now() - x2;
        }
        std::lock_guard<std::mutex> lk(mu);
        done = true;
        cv_get.notify_all();
    }
    // the next chunk, in file order (side 1: of the second mates); false behind the last
    bool next(TextChunk& c, int side = 0) {
        std::deque<TextChunk>& Q = side ? q2 : q;
        std::unique_lock<std::mutex> lk(mu);
        cv_get.wait(lk, [&] { return !Q.empty() || done; });
        if (Q.empty()) return false;
        c = Q.front(); Q.pop_front();
        cv_put.notify_one();
        return true;
    }
    // the thread has delivered its last chunk: its context goes (before the index does), its times are said
    void finish() {
        if (th.joinable()) th.join();
        if (ctx) moni_ctx_destroy(ctx);
        ctx = nullptr;
        fprintf(stderr, "[INFO] %s input %s: %zu chunks; inflater thread seconds: %s %.3f, copy%s %.3f, waiting for room in the queue %.3f\n", bam ? "BAM" : "BGZF", path.c_str(), n_chunks(),
                bam ? "moni_bam_in_feed" : "moni_bgzf_inflate", t_inflate, bam ? "" : " + cut", t_cut, t_full);
    }
    ~BgzfInput() {
        if (th.joinable()) th.join();
        for (TextChunk& c : q) free(c.p);
        for (TextChunk& c : q2) free(c.p);
        for (TextChunk& c : pool) free(c.p);
        if (ctx) moni_ctx_destroy(ctx);
        close();
    }
};

// The text of `path` starts with BAM\1 (through zlib, which reads BGZF as the gzip it is): what the modes without a BAM reader refuse by name.
static bool looks_like_bam(const std::string& path) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return false;
    char h[4];
    const bool bam = gzdirect(f) == 0 && gzread(f, h, 4) == 4 && !memcmp(h, "BAM\1", 4);
    gzclose(f);
    return bam;
}
// looks_like_bam goes through zlib, which also reads what the GPU reader does not take: BAM in plain gzip, a file cut inside a member, trailing bytes.
// Such a file is refused by name here, before anything parses it as text.
static void require_bgzf_bam(const std::string& path) {
    BgzfInput probe;
    if (!probe.open(path) || !probe.bam) die(path + ": BAM input must be whole BGZF members from the first byte to the last; plain-gzip BAM is not read, and this file may be cut off inside a member");
}
// --dry-run of BAM input, on the host: the records that would become reads are counted by hopping over block_size, nothing else of them is looked at
struct BamCount { size_t reads = 0, bases = 0; std::string first, second; };
static BamCount bam_dry_count(const std::string& path) {
    BamCount c;
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) die("cannot read " + path);
    auto get = [&](void* p, unsigned n) { return gzread(f, p, n) == (int)n; };
    auto skip = [&](int64_t n) { return n >= 0 && gzseek(f, (z_off_t)n, SEEK_CUR) >= 0; };
    char magic[4]; int32_t l_text = 0, n_ref = 0;
    bool ok = get(magic, 4) && !memcmp(magic, "BAM\1", 4) && get(&l_text, 4) && skip(l_text) && get(&n_ref, 4);
    for (int32_t r = 0; ok && r < n_ref; ++r) { int32_t l = 0; ok = get(&l, 4) && skip((int64_t)l + 4); }
    if (!ok) die(path + ": not a whole BAM header");
    uint8_t h[36];
    while (get(h, 36)) {
        uint32_t bs, l_seq; uint16_t flag;
        memcpy(&bs, h, 4); memcpy(&flag, h + 18, 2); memcpy(&l_seq, h + 20, 4);
        const uint32_t l_name = h[12];
        if (bs < 32u + l_name) die(path + ": a record's fields do not fit its block_size");
        std::string name(l_name, 0);
        if (l_name && !get(&name[0], l_name)) break;
        if (!skip((int64_t)bs - 32 - l_name)) break;
        if ((flag & 0x900) || !l_seq) continue;
        if (c.reads < 2) (c.reads ? c.second : c.first) = name.c_str();
        c.reads += 1; c.bases += l_seq;
    }
    gzclose(f);
    return c;
}

// ---- paired-end (-1 / -2): st_align's paired loop (align_reads_dispatcher.hpp:356-389) over the C ABI ----------------------------------
// Learn the insert-size model on batches of -b pairs until it is complete (or the input ends), align those batches, then the rest (in
// larger batches: with the model fixed every pair is independent).  -u switches orphan recovery off.
struct AnyReader {
    MappedReader m; Reader* z = nullptr; bool mapped = false;
    BgzfInput* bz = nullptr; TextChunk cur;          // BGZF input inflated on the GPU: m is a view of the current chunk
    int side = 0;                                    // 1: the second mates of `first`'s BAM with pairs (bz is first's)
    explicit AnyReader(const std::string& path, bool gpu_inflate = false) {
        if (gpu_inflate) { bz = new BgzfInput(); if (!bz->open(path)) { delete bz; bz = nullptr; } }
        if (!bz) { mapped = m.open(path); if (!mapped) z = new Reader(path); }
    }
    explicit AnyReader(AnyReader& first) : bz(first.bz), side(1) {}
    ~AnyReader() { if (bz) { m.p = nullptr; free(cur.p); if (!side) delete bz; } delete z; }          // (free: the pool may be gone with bz's thread)
    bool fastq_view() const { return bz ? bz->fq : mapped && m.p[m.at < m.n ? m.at : 0] == '@'; }
    // the next chunk becomes the view; false behind the last
    bool refill() {
        bz->recycle(cur); m.p = nullptr; m.n = m.at = 0;
        if (!bz->next(cur, side)) return false;
        m.p = cur.p; m.n = cur.n;
        return true;
    }
    // the view stands on a record (chunks are record-aligned); false at the end of the input
    bool more() {
        while (true) {
            while (m.p && m.at < m.n && (m.p[m.at] == '\n' || m.p[m.at] == '\r')) ++m.at;
            if (m.p && m.at < m.n) return true;
            if (!bz || !refill()) return false;
        }
    }
    bool next(Batch& b) {
        if (bz) return more() && m.next(b);
        return mapped ? m.next(b) : z->next(b);
    }
};
static size_t read_pairs(AnyReader& r1, AnyReader& r2, size_t n_pairs, Batch& b) {
    size_t n = 0;
    while (n < n_pairs) {
        const bool g1 = r1.next(b);
        if (!g1) { Batch t; if (r2.next(t)) die("the mate files have different numbers of records"); break; }
        if (!r2.next(b)) die("the mate files have different numbers of records");
        ++n;
    }
    return n;
}
// the same with the two files parsed side by side (one thread each) and interleaved afterwards (mates 2p, 2p + 1), by T threads
static size_t read_pairs_par(AnyReader& r1, AnyReader& r2, size_t n_pairs, Batch& b, int T) {
    Batch b1, b2;
    size_t n2 = 0;
    std::thread t2([&] { while (n2 < n_pairs && r2.next(b2)) ++n2; });
    size_t n1 = 0;
    while (n1 < n_pairs && r1.next(b1)) ++n1;
    t2.join();
    if (n1 != n2) die("the mate files have different numbers of records");
    if (n1 < n_pairs) { Batch t; if (r1.next(t) || r2.next(t)) die("the mate files have different numbers of records"); }
    const size_t n = n1;
    if (!n) return 0;
    b.has_qual = b1.has_qual && b2.has_qual;
    b.off.resize(2 * n + 1); b.name_off.resize(2 * n + 1);
    for (size_t p = 0; p < n; ++p) {
        b.off[2 * p] = b1.off[p] + b2.off[p]; b.off[2 * p + 1] = b1.off[p + 1] + b2.off[p];
        b.name_off[2 * p] = b1.name_off[p] + b2.name_off[p]; b.name_off[2 * p + 1] = b1.name_off[p + 1] + b2.name_off[p];
    }
    b.off[2 * n] = b1.off[n] + b2.off[n]; b.name_off[2 * n] = b1.name_off[n] + b2.name_off[n];
    b.seq.resize(b.off[2 * n]); b.names.resize(b.name_off[2 * n]);
    if (b.has_qual) b.qual.resize(b.off[2 * n]);
    auto part = [&](size_t lo, size_t hi) {
        for (size_t p = lo; p < hi; ++p) {
            const size_t l1 = (size_t)(b1.off[p + 1] - b1.off[p]), l2 = (size_t)(b2.off[p + 1] - b2.off[p]);
            memcpy(b.seq.data() + b.off[2 * p], b1.seq.data() + b1.off[p], l1); memcpy(b.seq.data() + b.off[2 * p + 1], b2.seq.data() + b2.off[p], l2);
            if (b.has_qual) { memcpy(b.qual.data() + b.off[2 * p], b1.qual.data() + b1.off[p], l1); memcpy(b.qual.data() + b.off[2 * p + 1], b2.qual.data() + b2.off[p], l2); }
            memcpy(b.names.data() + b.name_off[2 * p], b1.names.data() + b1.name_off[p], (size_t)(b1.name_off[p + 1] - b1.name_off[p]));
            memcpy(b.names.data() + b.name_off[2 * p + 1], b2.names.data() + b2.name_off[p], (size_t)(b2.name_off[p + 1] - b2.name_off[p]));
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(part, n * t / T, n * (t + 1) / T);
    part(0, n / T);
    for (auto& t : th) t.join();
    return n;
}
// the index on GPU g: <prefix>.mfi, or the reference's own files when that one is absent
static moni_index_t* load_index(const Args& a, int g) {
    const std::string idx_path = a.filename + ".mfi";
    const bool have_mfi = !a.no_lcp && access(idx_path.c_str(), R_OK) == 0;          // (the flat file always carries the LCP samples)
    const std::string ms_path = a.filename + (a.no_lcp ? ".thrbv.full.ms" : ".thrbv.full.lcp.ms"), ldx_path = a.filename + ".ldx", txt_path = a.filename + ".txt";
    const bool have_txt = access(txt_path.c_str(), R_OK) == 0;          // optional: without it the text is rebuilt from the BWT on the GPU
    moni_index_t* idx = nullptr;
    if (have_mfi) { if (moni_index_load(idx_path.c_str(), g, &idx)) die("cannot load " + idx_path + " on GPU " + std::to_string(g) + " (moni-hip has no CPU path)"); }
    else if (moni_index_load_reference(ms_path.c_str(), ldx_path.c_str(), have_txt ? txt_path.c_str() : nullptr, g, &idx))
        die("cannot load " + idx_path + " nor " + ms_path + " + " + ldx_path + " (reader of the reference's files: layout unverified against a real `moni build` output) on GPU " + std::to_string(g) + " (moni-hip has no CPU path)");
    return idx;
}
// a batch of interleaved mates as the library takes it: the slow reader's Batch, or the fast reader's PairBatch (both mate files four-line FASTQ)
struct PairView {
    const uint8_t* seq; const uint64_t* off; const uint8_t* names; const uint64_t* name_off; const uint8_t* qual; size_t n;
    PairView(const Batch& b) : seq(b.seq.data()), off(b.off.data()), names(b.names.data()), name_off(b.name_off.data()), qual(b.has_qual ? b.qual.data() : nullptr), n(b.n()) {}
    PairView(const fastpath::PairBatch& f) : seq(f.seq.p), off(f.off.data()), names(f.names.p), name_off(f.name_off.data()), qual(f.qual.p), n(f.n_reads) {}
};
// The paired library call the flags choose: -m the MEM records instead of the pairs' (the fragment model plays no part in them), -c the records and <sam>.csv's
// lines, else the records alone - with `pinned` in C's pinned buffer, to be written out before C's next call, not freed.  owned: sam is moni_free's; csv always is.
struct PairOut { char* sam = nullptr; uint64_t len = 0; char* csv = nullptr; uint64_t csv_len = 0; size_t aligned = 0; bool owned = true; };
static PairOut pe_call(moni_ctx_t* C, const PairView& v, const Args& a, const moni_pe_model_t& model, bool pinned) {
    const moni_read_batch_t rb{v.seq, v.off, v.n};
    PairOut o;
    moni_align_stats_t st;
    if (a.report_mems) {
        const int rm = moni_pe_report_mems_batch(C, &rb, v.names, v.name_off, v.qual, &a.P, &a.PE, &o.sam, &o.len);
        if (rm) die("moni_pe_report_mems_batch failed (" + std::to_string(rm) + ")");
        return o;
    }
    if (a.csv) {
        const int rc = moni_pe_align_csv_batch(C, &rb, v.names, v.name_off, v.qual, &a.P, &a.PE, &model, &o.sam, &o.len, &o.csv, &o.csv_len, &st);
        if (rc) die("moni_pe_align_csv_batch failed (" + std::to_string(rc) + ")");
    } else {
        const int rc = (pinned ? moni_pe_align_stream : moni_pe_align_batch)(C, &rb, v.names, v.name_off, v.qual, &a.P, &a.PE, &model, &o.sam, &o.len, &st);
        if (rc) die(std::string(pinned ? "moni_pe_align_stream" : "moni_pe_align_batch") + " failed (" + std::to_string(rc) + (rc == MONI_ERANGE ? ": a pair exceeds the paired path's capacities)" : ")"));
        o.owned = !pinned;
    }
    o.aligned = st.aligned;
    return o;
}
static int run_paired(Args& a, const std::string& sam_filename) {
    a.PE.find_orphan = a.find_orphan ? 1 : 0;            // -u switches orphan recovery off (align_full_ksw2.cpp:248-250)
    a.PE.secondary_chains = a.secondary ? 1 : 0;         // -Z: find_chains_secondary (the second track of the chaining, on the staged paired kernels)
    info("Output file: " + sam_filename);
    const bool one_file = !a.interleaved.empty();
    if (one_file) a.mate1 = a.mate2 = a.interleaved;
    const bool bam_in = looks_like_bam(a.mate1) || looks_like_bam(a.mate2);
    if (one_file && !bam_in) die("--interleaved takes a BAM file");
    if (bam_in && !(looks_like_bam(a.mate1) && looks_like_bam(a.mate2))) die("-1 and -2: one mate file is BAM, the other is not");
    if (bam_in && a.host_inflate) die("--host-inflate cannot be combined with BAM input: there is no host BAM parser, the records are read on the GPU");
    if (bam_in && (a.report_mems || a.csv)) die(std::string(a.report_mems ? "-m" : "-c") + " does not take BAM input");
    if (bam_in) { require_bgzf_bam(a.mate1); if (!one_file) require_bgzf_bam(a.mate2); }
    if (bam_in && a.dry_run) {
        const BamCount c1 = bam_dry_count(a.mate1), c2 = one_file ? c1 : bam_dry_count(a.mate2);
        if (one_file ? (c1.reads & 1) != 0 : c1.reads != c2.reads) die(one_file ? "--interleaved: an odd number of primary records" : "the mate files have different numbers of records");
        const std::string& second = one_file ? c1.second : c2.first;
        printf("dry-run: pairs=%zu bases=%zu min_len=%u filter_dir=%u dir_thr=%.1f find_orphan=%u b=%zu threads=%zu gpus=%d out=%s first=%s second=%s%s input=bam\n", one_file ? c1.reads / 2 : c1.reads,
               one_file ? c1.bases : c1.bases + c2.bases, a.P.min_len, a.PE.filter_dir, a.PE.dir_thr, a.PE.find_orphan, a.b, a.th, a.gpus, sam_filename.c_str(), c1.first.c_str(), second.c_str(), output_word(a));
        return 0;
    }
    const bool gpu_inflate = !a.host_inflate && !a.report_mems && !a.csv && !a.dry_run;
    AnyReader r1(a.mate1, gpu_inflate);
    if (one_file) r1.bz->pairs = true;
    const std::unique_ptr<AnyReader> second(one_file ? new AnyReader(r1) : new AnyReader(a.mate2, gpu_inflate));          // (it goes before r1 does)
    AnyReader& r2 = *second;
    if (a.dry_run) {
        bool bz_in = false;          // counting stays on the host; the word says what the run would do
        if (!a.host_inflate && !a.report_mems && !a.csv) { BgzfInput p1, p2; bz_in = p1.open(a.mate1) || p2.open(a.mate2); }
        Batch b;
        const size_t n = read_pairs(r1, r2, (size_t)-1, b);
        printf("dry-run: pairs=%zu bases=%zu min_len=%u filter_dir=%u dir_thr=%.1f find_orphan=%u b=%zu threads=%zu gpus=%d out=%s first=%.*s second=%.*s%s%s\n", n, b.seq.size(),
               a.P.min_len, a.PE.filter_dir, a.PE.dir_thr, a.PE.find_orphan, a.b, a.th, a.gpus, sam_filename.c_str(), n ? (int)b.name_off[1] : 0,
               n ? (const char*)b.names.data() : "", n ? (int)(b.name_off[2] - b.name_off[1]) : 0, n ? (const char*)b.names.data() + b.name_off[1] : "", output_word(a), bz_in ? " input=bgzf" : "");
        return 0;
    }
    std::vector<moni_index_t*> idx(a.gpus, nullptr);
    std::vector<moni_ctx_t*> ctx(a.gpus, nullptr);
    for (int g = 0; g < a.gpus; ++g) {
        idx[g] = load_index(a, g);
        if (moni_ctx_create(idx[g], &ctx[g])) die("cannot create a context on GPU " + std::to_string(g));
    }
    if (r1.bz) r1.bz->start(idx[0], a.inflate_blocks);
    if (r2.bz && !one_file) r2.bz->start(idx[0], a.inflate_blocks);
    const auto t0 = std::chrono::steady_clock::now();
    Sink sink;          // --sort: the learning batches are run 0, the workers' batches follow
    sink.open(sam_filename, a, true);
    sink.begin(idx[0], ctx);
    // -c: <sam>.csv, one line per pair (aligner_ksw2.hpp:911-914; header of aligner::to_csv, :3230-3234); the lines of a batch are placed behind those of the batches before it, as its records are
    Placer csv;
    if (a.csv) {
        csv.open(sam_filename + ".csv");
        static const char hdr[] = "Read,Unique,Total,Max_Freq,Min_Freq,Highest_Occ,Lowest_Occ,Filtered,Chains_Skipped\n";
        csv.append(hdr, sizeof hdr - 1);
    }
    moni_pe_model_t model;
    memset(&model, 0, sizeof model);
    size_t processed = 0, aligned = 0;
    std::vector<Batch*> learnt;
    while (!model.complete && !a.report_mems) {
        Batch* b = new Batch();
        if (!read_pairs(r1, r2, a.b, *b)) { delete b; break; }
        moni_read_batch_t rb{b->seq.data(), b->off.data(), b->n()};
        const int rc = moni_pe_learn_batch(ctx[0], &rb, &a.P, &a.PE, &model);
        if (rc) die("moni_pe_learn_batch failed (" + std::to_string(rc) + ")");
        learnt.push_back(b);
    }
    info("Insert size model: count " + std::to_string(model.count) + ", mean " + std::to_string(model.mean) + ", std dev " + std::to_string(model.std_dev) +
         (model.complete ? "" : " (input ended before " + std::to_string(a.PE.ins_learning_n) + " pairs)"));
    {   // the learning batches as one batch
        Batch all;
        for (Batch* b : learnt) {
            const uint64_t s0 = all.seq.size(), n0 = all.names.size();
            all.seq.insert(all.seq.end(), b->seq.begin(), b->seq.end()); all.qual.insert(all.qual.end(), b->qual.begin(), b->qual.end());
            all.names.insert(all.names.end(), b->names.begin(), b->names.end());
            for (size_t i = 1; i < b->off.size(); ++i) { all.off.push_back(s0 + b->off[i]); all.name_off.push_back(n0 + b->name_off[i]); }
            all.has_qual = all.has_qual && b->has_qual;
            delete b;
        }
        if (all.n()) {
            const PairOut o = pe_call(ctx[0], all, a, model, false);
            const Block z = sink.encode(ctx[0], 0, o.sam, o.len);
            sink.append(z.p, z.n);
            moni_free(o.sam);
            if (a.csv) csv.append(o.csv, o.csv_len);
            moni_free(o.csv);
            processed += all.n() / 2; aligned += o.aligned;
        }
    }
    // ---- the rest: reader thread (the two files parsed side by side) -> bounded queue -> a few workers per GPU, each with its own context (one's upload and
    // seeding run beside the others' paired kernels) -> every block written at its place in the file (the in-order prefix sum of the blocks' lengths) ----
    const size_t pairs_per_batch = std::max<size_t>(a.gpu_batch / 2, 1024);          // as many mates per batch as the single-end path has reads
    const int per_gpu = a.report_mems ? 1 : std::max(1, a.ctx_per_gpu), P = 4;          // contexts per GPU (--ctx-per-gpu, 3): one's upload, seeding and file write beside the others' paired kernels
    std::vector<moni_ctx_t*> wctx((size_t)a.gpus * per_gpu, nullptr);
    for (int g = 0; g < a.gpus; ++g) for (int k = 0; k < per_gpu; ++k) {
        if (k == 0) wctx[(size_t)g * per_gpu] = ctx[g];
        else if (moni_ctx_create(idx[g], &wctx[(size_t)g * per_gpu + k])) die("cannot create a context on GPU " + std::to_string(g));
    }
    sink.set_dictionary(wctx);          // the dictionary alone: the header is in the file
    // a batch for the workers: the slow reader's Batch, or the fast reader's PairBatch (both mate files mapped four-line FASTQ)
    struct Item { size_t id; Batch* b; fastpath::PairBatch* f; };
    const bool fast_reader = r1.fastq_view() && r2.fastq_view() && getenv("MONI_CLI_SLOW_READER") == nullptr;
    const bool chunked = r1.bz || r2.bz;          // a view is a chunk of inflated text, not the whole file: a batch ends where a chunk does
    std::mutex mu_q;
    std::condition_variable cv_put, cv_get;
    std::deque<Item> queue;
    bool reader_done = false;
    const size_t q_cap = wctx.size() + 1;
    std::atomic<size_t> n_proc{0}, n_al_all{0};
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_read = 0; std::vector<double> t_lib(wctx.size(), 0), t_wait(wctx.size(), 0), t_write(wctx.size(), 0);
    const bool verbose_batches = getenv("MONI_CLI_VERBOSE") != nullptr;
    std::thread reader([&] {
        size_t id = 0;
        const char* fbase[2] = {r1.m.p, r2.m.p}; const char* fend[2] = {r1.m.p + r1.m.n, r2.m.p + r2.m.n}; size_t fat[2] = {r1.m.at, r2.m.at};
        fastpath::ParsedBatch pb[2];
        while (true) {
            Batch* b = nullptr; fastpath::PairBatch* f = nullptr;
            const double r0 = now();
            size_t want = pairs_per_batch;
            if (fast_reader && chunked) {
                const bool m1 = r1.more(), m2 = r2.more();
                if (m1 != m2) die("the mate files have different numbers of records");
                if (!m1) break;
                fbase[0] = r1.m.p; fbase[1] = r2.m.p; fend[0] = r1.m.p + r1.m.n; fend[1] = r2.m.p + r2.m.n; fat[0] = r1.m.at; fat[1] = r2.m.at;
                for (int k = 0; k < 2; ++k) { size_t got = 0; fastpath::skip_records(fbase[k] + fat[k], fend[k], want, 2 * P, got); want = std::min(want, got); }
                if (!want) die("the mate files are not four-line FASTQ throughout (blank or wrapped lines): use --host-inflate to take the record-by-record reader");
            }
            if (fast_reader) {
                f = new fastpath::PairBatch();
                if (!fastpath::read_pairs_fast(fbase, fend, fat, want, 2 * P, pb, *f)) { delete f; break; }
                if (chunked) { r1.m.at = fat[0]; r2.m.at = fat[1]; }
            }
            else { b = new Batch(); if (!read_pairs_par(r1, r2, pairs_per_batch, *b, P)) { delete b; break; } }
            t_read += now() - r0;
            std::unique_lock<std::mutex> lk(mu_q);
            cv_put.wait(lk, [&] { return queue.size() < q_cap; });
            queue.push_back(Item{id++, b, f});
            cv_get.notify_one();
        }
        std::lock_guard<std::mutex> lk(mu_q);
        reader_done = true;
        cv_get.notify_all();
    });
    auto worker = [&](int w) {
        moni_ctx_t* C = wctx[w];
        while (true) {
            Item it;
            {
                std::unique_lock<std::mutex> lk(mu_q);
                cv_get.wait(lk, [&] { return !queue.empty() || reader_done; });
                if (queue.empty()) return;
                it = queue.front(); queue.pop_front();
                cv_put.notify_one();
            }
            const PairView v = it.f ? PairView(*it.f) : PairView(*it.b);
            const double x1 = now();
            const PairOut o = pe_call(C, v, a, model, true);          // the text in the context's pinned buffer (-m, -c: malloc'ed): written out before the context's next call
            const Block z = sink.encode(C, it.id + 1, o.sam, o.len);
            const double x2 = now();
            const uint64_t at = sink.place(it.id, z.n);
            const double x3 = now();
            sink.write(z.p, z.n, at, P);
            const double x4 = now();
            t_lib[w] += x2 - x1; t_wait[w] += x3 - x2; t_write[w] += x4 - x3;
            if (verbose_batches) fprintf(stderr, "batch %zu (worker %d, %zu pairs): library %.0f ms, wait %.0f ms, write %.0f ms, done at %.3f s\n", it.id, w, v.n / 2, (x2 - x1) * 1e3, (x3 - x2) * 1e3, (x4 - x3) * 1e3,
                                        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
            if (a.csv) csv.write(o.csv, o.csv_len, csv.place(it.id, o.csv_len), 1);
            if (o.owned) moni_free(o.sam);
            moni_free(o.csv);
            n_proc += v.n / 2; n_al_all += o.aligned;
            delete it.b; delete it.f;
        }
    };
    {
        std::vector<std::thread> th;
        for (size_t w = 0; w < wctx.size(); ++w) th.emplace_back(worker, (int)w);
        for (auto& t : th) t.join();
    }
    reader.join();
    if (a.csv) csv.close("short write to the csv file");
    processed += n_proc.load(); aligned += n_al_all.load();
    {
        double sl = 0, sw = 0, sr = 0;
        for (size_t w = 0; w < wctx.size(); ++w) { sl += t_lib[w]; sw += t_wait[w]; sr += t_write[w]; }
        info("Stage seconds: reading + interleaving the mate files " + std::to_string(t_read) + " (one reader thread, two parsers); summed over " + std::to_string(wctx.size()) + " workers: library calls " +
             std::to_string(sl) + ", waiting for the block's place " + std::to_string(sw) + ", file writes " + std::to_string(sr));
    }
    if (r1.bz) r1.bz->finish();
    if (r2.bz && !one_file) r2.bz->finish();
    sink.finish(wctx);
    for (int g = 0; g < a.gpus; ++g) for (int k = 1; k < per_gpu; ++k) moni_ctx_destroy(wctx[(size_t)g * per_gpu + k]);
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    info("Number of aligned pairs: " + std::to_string(aligned) + "/" + std::to_string(processed));
    info("Elapsed time (s): " + std::to_string(el));
    info("Pairs per second: " + std::to_string(processed / (el > 0 ? el : 1)));
    for (int g = 0; g < a.gpus; ++g) { moni_ctx_destroy(ctx[g]); moni_index_destroy(idx[g]); }
    return 0;
}

// ---- the single-end modes of the queue path -------------------------------------------------------------------------------------------
struct Done { char* a = nullptr; uint64_t la = 0; std::string b; };      // a batch's output - a: a malloc'ed block (the library's, or give()'s); b: a second stream (.lengths, .csv)
typedef std::vector<std::string> Names;
// A mode's worker: the library call on batch b (rb: as the library takes it; its first read is number `first` of the input) and the text of its results into d; returns the batch's count for the summary line.
typedef size_t RunFn(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t first, Args& a, const Names& seq_names, Done& d);

static void give(Done& d, const std::string& s) { d.a = (char*)malloc(s.size() + 1); if (!d.a) die("out of memory"); memcpy(d.a, s.data(), s.size()); d.la = s.size(); }
static void put_name(std::string& sa, const Batch& b, size_t r) { sa.append((const char*)b.names.data() + b.name_off[r], (size_t)(b.name_off[r + 1] - b.name_off[r])); }

// One line per pattern lo .. hi - 1 and strand: name, strand, what line(task) writes (tasks count from lo); returns the patterns for which it said "occurs" on a strand.
template <class F>
static size_t task_lines(std::string& sa, const Batch& b, size_t lo, size_t hi, uint32_t strands, F line) {
    size_t n = 0;
    for (size_t r = lo; r < hi; ++r) {
        bool occurs = false;
        for (uint32_t s = 0; s < strands; ++s) {
            put_name(sa, b, r);
            sa += s ? "\t-\t" : "\t+\t";
            if (line((r - lo) * strands + s)) occurs = true;
            sa.push_back('\n');
        }
        if (occurs) ++n;
    }
    return n;
}

// seq:pos[,seq:pos...] of entries off .. off + n - 1 of the lists a call returned (`total` entries; su: each followed by :support)
static void put_positions(std::string& sa, const Names& seq_names, const uint32_t* sq, const uint64_t* so, const uint64_t* su, uint64_t off, uint64_t n, uint64_t total, const char* call) {
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t o = off + k;
        if (o >= total || sq[o] >= seq_names.size()) die(std::string(call) + " returned a position outside the index");
        if (k) sa.push_back(',');
        sa += seq_names[sq[o]]; sa.push_back(':'); sa += std::to_string(so[o] + 1);
        if (su) { sa.push_back(':'); sa += std::to_string(su[o]); }
    }
}

static size_t run_ms(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names&, Done& d) {          // --ms / --mems
    std::vector<uint64_t> ptr(b.seq.size() + 1), len(b.seq.size() + 1);
    if (a.split) {
        moni_mslong_params_t sp; moni_mslong_params_default(&sp);
        if (a.seg_len_set) sp.seg_len = a.seg_len;
        if (a.overlap_set) sp.overlap = a.overlap;
        const int sr = moni_ms_long_batch(C, &rb, &sp, ptr.data(), len.data(), nullptr);
        if (sr) die("moni_ms_long_batch failed (" + std::to_string(sr) + ")");
    } else if (moni_ms_lengths_batch(C, &rb, ptr.data(), len.data())) die("moni_ms_lengths_batch failed");
    std::string sa, sb;
    for (size_t r = 0; r < b.n(); ++r) {
        const std::string hdr = ">" + std::string((const char*)b.names.data() + b.name_off[r], (size_t)(b.name_off[r + 1] - b.name_off[r])) + "\n";
        sa += hdr;
        const size_t o = b.off[r], m = b.off[r + 1] - o;
        if (a.legacy_ms) {          // matching_statistics.cpp:565-600: values followed by a blank, one line per read
            sb += hdr;
            for (size_t k = 0; k < m; ++k) { sa += std::to_string(ptr[o + k]); sa.push_back(' '); sb += std::to_string(len[o + k]); sb.push_back(' '); }
            sb.push_back('\n');
        } else {                    // mems.cpp:241-262, 585-590: (offset,length) of every position whose length does not drop
            for (size_t k = 0; k < m; ++k) if (k == 0 || len[o + k] >= len[o + k - 1]) { sa += "(" + std::to_string(k) + "," + std::to_string(len[o + k]) + ") "; }
        }
        sa.push_back('\n');
    }
    give(d, sa); d.b = std::move(sb);
    return 0;
}

static size_t run_pseudo_ms(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t first, Args& a, const Names&, Done& d) {       // run_spumoni.cpp:495-498: ">" + the read's running number, then the lengths, each followed by a blank
    std::vector<uint32_t> len(b.seq.size() + 1), hits(b.n() + 1);
    const int pr = moni_pml_batch(C, &rb, a.P.min_len, len.data(), nullptr, hits.data());
    if (pr) die("moni_pml_batch failed (" + std::to_string(pr) + ")");
    std::string sa;
    sa.reserve(b.seq.size() * 3 + b.n() * 12);
    char num[24];
    size_t n_al = 0;
    for (size_t r = 0; r < b.n(); ++r) {
        sa.push_back('>'); sa += std::to_string(first + r); sa.push_back('\n');
        const size_t o = b.off[r], m = b.off[r + 1] - o;
        for (size_t k = 0; k < m; ++k) { const int nc = snprintf(num, sizeof num, "%u ", len[o + k]); sa.append(num, (size_t)nc); }
        sa.push_back('\n');
        if (hits[r]) ++n_al;          // reads with a length >= -l somewhere
    }
    give(d, sa);
    return n_al;
}

static size_t run_screen(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names&, Done& d) {          // one line per read: name, length, call, strand, scored windows, then per strand positive windows, largest D, largest length
    std::vector<moni_screen_res_t> res(b.n() + 1);
    const int sr = moni_screen_batch(C, &rb, &a.SP, res.data());
    if (sr) die("moni_screen_batch failed (" + std::to_string(sr) + ")");
    std::string sa;
    sa.reserve(b.n() * 64 + b.names.size());
    char num[128];
    size_t n_al = 0;
    for (size_t r = 0; r < b.n(); ++r) {
        const moni_screen_res_t& R = res[r];
        const bool present = (R.flags & MONI_SCREEN_PRESENT) != 0;
        put_name(sa, b, r);
        const int nc = snprintf(num, sizeof num, "\t%llu\t%c\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", (unsigned long long)(b.off[r + 1] - b.off[r]),
                                (R.flags & MONI_SCREEN_SHORT) ? 'S' : present ? 'P' : 'A', !present ? '.' : (R.flags & MONI_SCREEN_STRAND1) ? '-' : '+', R.n_win, R.n_pos[0],
                                R.n_pos[1], R.d_max[0], R.d_max[1], R.max_pml[0], R.max_pml[1]);
        sa.append(num, (size_t)nc);
        if (present) ++n_al;
    }
    give(d, sa);
    return n_al;
}

static size_t run_locate(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names& seq_names, Done& d) {          // per pattern and strand: count, bytes matched, the occurrences kept
    moni_locate_params_t lp; moni_locate_params_default(&lp);
    lp.strands = a.both_strands ? 2 : 1; lp.max_occ = a.max_occ;
    std::vector<moni_locate_res_t> res(b.n() * lp.strands + 1);
    uint32_t* sq = nullptr; uint64_t* so = nullptr; uint64_t n_occ = 0;
    const int lr = moni_locate_batch(C, &rb, &lp, res.data(), nullptr, &sq, &so, &n_occ);
    if (lr) die("moni_locate_batch failed (" + std::to_string(lr) + ")");
    std::string sa;
    const size_t n_al = task_lines(sa, b, 0, b.n(), lp.strands, [&](size_t t) {
        const moni_locate_res_t& R = res[t];
        sa += std::to_string(R.count); sa.push_back('\t'); sa += std::to_string(R.matched); sa.push_back('\t');
        if (!R.n_occ) sa.push_back('*');
        put_positions(sa, seq_names, sq, so, nullptr, R.occ_off, R.n_occ, n_occ, "moni_locate_batch");
        return R.count != 0;
    });
    moni_free(sq); moni_free(so);
    give(d, sa);
    return n_al;
}

static size_t run_seq_count(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names& seq_names, Done& d) {       // per pattern and strand: count, bytes matched, sequences that hold it, their counts
    moni_seqcount_params_t sp; moni_seqcount_params_default(&sp);
    sp.strands = a.both_strands ? 2 : 1; sp.max_walk = a.max_walk;
    const size_t n_seq = seq_names.size(), n_tasks = b.n() * sp.strands;
    std::vector<moni_seqcount_res_t> res(n_tasks + 1);
    std::vector<uint64_t> counts(n_tasks * n_seq + 1);
    const int sr = moni_seqcount_batch(C, &rb, &sp, res.data(), counts.data());
    if (sr) die("moni_seqcount_batch failed (" + std::to_string(sr) + ")");
    std::string sa;
    const size_t n_al = task_lines(sa, b, 0, b.n(), sp.strands, [&](size_t t) {
        const moni_seqcount_res_t& R = res[t];
        sa += std::to_string(R.count); sa.push_back('\t'); sa += std::to_string(R.matched); sa.push_back('\t'); sa += std::to_string(R.n_seqs); sa.push_back('\t');
        if (!R.walked) sa.push_back('?');
        else if (!R.n_seqs) sa.push_back('*');
        else {
            bool first = true;
            for (size_t q = 0; q < n_seq; ++q) {
                const uint64_t v = counts[t * n_seq + q];
                if (!v) continue;
                if (!first) sa.push_back(',');
                first = false;
                sa += seq_names[q]; sa.push_back(':'); sa += std::to_string(v);
            }
        }
        return R.count != 0;
    });
    give(d, sa);
    return n_al;
}

static size_t run_loci(moni_ctx_t* C, Batch& b, const moni_read_batch_t&, size_t, Args& a, const Names& seq_names, Done& d) {          // per pattern and strand: count, bytes matched, loci, each locus with its support
    moni_loci_params_t lp; moni_loci_params_default(&lp);
    lp.strands = a.both_strands ? 2 : 1; lp.max_walk = a.max_walk; lp.lift = a.no_lift ? 0 : 1;
    std::string sa;
    std::vector<moni_loci_res_t> res;
    size_t n_al = 0;
    // a batch whose occurrences do not fit the library's bound (MONI_ENOMEM) is run in halves, in order
    std::function<void(size_t, size_t)> part = [&](size_t lo, size_t hi) {
        const size_t n = hi - lo;
        moni_read_batch_t sub{b.seq.data(), b.off.data() + lo, n};
        res.assign(n * lp.strands + 1, moni_loci_res_t());
        uint32_t* sq = nullptr; uint64_t* so = nullptr; uint64_t* su = nullptr; uint64_t n_loci = 0;
        const int lr = moni_loci_batch(C, &sub, &lp, res.data(), nullptr, &sq, &so, &su, &n_loci);
        if (lr == MONI_ENOMEM && n > 1) { part(lo, lo + n / 2); part(lo + n / 2, hi); return; }
        if (lr == MONI_ENOMEM) die("--loci: the occurrences of one pattern do not fit in memory; lower --max-walk");
        if (lr) die("moni_loci_batch failed (" + std::to_string(lr) + ")");
        n_al += task_lines(sa, b, lo, hi, lp.strands, [&](size_t t) {
            const moni_loci_res_t& R = res[t];
            sa += std::to_string(R.count); sa.push_back('\t'); sa += std::to_string(R.matched); sa.push_back('\t'); sa += std::to_string(R.n_loci); sa.push_back('\t');
            if (!R.walked) sa.push_back('?');
            else if (!R.n_loci) sa.push_back('*');
            put_positions(sa, seq_names, sq, so, su, R.loci_off, R.n_loci, n_loci, "moni_loci_batch");
            return R.count != 0;
        });
        moni_free(sq); moni_free(so); moni_free(su);
    };
    if (b.n()) part(0, b.n());
    give(d, sa);
    return n_al;
}

static size_t run_approx(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names& seq_names, Done& d) {          // per pattern and strand: complete, the counts per distance, the matching strings, those kept
    moni_approx_params_t ap; moni_approx_params_default(&ap);
    ap.strands = a.both_strands ? 2 : 1; ap.k = a.approx_k; ap.max_hits = a.max_hits; ap.max_occ = a.max_occ; ap.max_steps = a.max_steps;
    std::vector<moni_approx_res_t> res(b.n() * ap.strands + 1);
    moni_approx_hit_t* hits = nullptr; uint32_t* sq = nullptr; uint64_t* so = nullptr; uint64_t n_hits = 0, n_occ = 0;
    const int ar = moni_approx_batch(C, &rb, &ap, res.data(), &hits, nullptr, &sq, &so, &n_hits, &n_occ);
    if (ar) die("moni_approx_batch failed (" + std::to_string(ar) + ")");
    std::string sa;
    const size_t n_al = task_lines(sa, b, 0, b.n(), ap.strands, [&](size_t t) {
        const moni_approx_res_t& R = res[t];
        sa += std::to_string(R.complete); sa.push_back('\t');
        for (uint32_t e = 0; e <= ap.k; ++e) { if (e) sa.push_back(','); sa += std::to_string(R.cnt[e]); }
        sa.push_back('\t'); sa += std::to_string(R.n_hits); sa.push_back('\t');
        if (!R.n_kept) sa.push_back('*');
        for (uint32_t j = 0; j < R.n_kept; ++j) {
            if (R.hit_off + j >= n_hits) die("moni_approx_batch returned a hit outside its list");
            const moni_approx_hit_t& H = hits[R.hit_off + j];
            if (j) sa.push_back(';');
            sa += std::to_string(H.n_mis); sa.push_back(':'); sa += std::to_string(H.count); sa.push_back(':');
            if (!H.n_occ) sa.push_back('*');
            put_positions(sa, seq_names, sq, so, nullptr, H.occ_off, H.n_occ, n_occ, "moni_approx_batch");
        }
        return R.n_hits != 0;
    });
    moni_free(hits); moni_free(sq); moni_free(so);
    give(d, sa);
    return n_al;
}

static size_t run_extend(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names&, Done& d) {          // extender::config_t from the flags it shares with the aligner (-l -L -A -B -O -E)
    moni_extend_params_t xp; moni_extend_params_default(&xp);
    xp.min_len = a.P.min_len; xp.ext_len = a.P.ext_len; xp.smatch = a.P.smatch; xp.smismatch = a.P.smismatch; xp.gapo = a.P.gapo; xp.gape = a.P.gape;
    moni_extend_stats_t st;
    const int xr = moni_extend_batch(C, &rb, b.names.data(), b.name_off.data(), b.has_qual ? b.qual.data() : nullptr, &xp, &d.a, &d.la, &st);
    if (xr) die("moni_extend_batch failed (" + std::to_string(xr) + ")");
    return st.extended;
}

static size_t run_report_mems(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names&, Done& d) {          // -m
    if (moni_report_mems_batch(C, &rb, b.names.data(), b.name_off.data(), b.has_qual ? b.qual.data() : nullptr, &a.P, &d.a, &d.la)) die("moni_report_mems_batch failed");
    return b.n();
}

static size_t run_csv(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names&, Done& d) {          // -c
    moni_align_stats_t st; char* cs = nullptr; uint64_t cl = 0;
    if (moni_align_csv_batch(C, &rb, b.names.data(), b.name_off.data(), b.has_qual ? b.qual.data() : nullptr, &a.P, &d.a, &d.la, &cs, &cl, &st)) die("moni_align_csv_batch failed");
    d.b.assign(cs, cl); moni_free(cs);
    return st.aligned;
}

static size_t run_align(moni_ctx_t* C, Batch& b, const moni_read_batch_t& rb, size_t, Args& a, const Names&, Done& d) {          // plain alignment: no entry of the table
    moni_align_stats_t st;
    if (moni_align_batch(C, &rb, b.names.data(), b.name_off.data(), b.has_qual ? b.qual.data() : nullptr, &a.P, &d.a, &d.la, &st)) die("moni_align_batch failed");
    return st.aligned;
}

// The table.  At most one of the modes past --mems is set (main refuses the rest), and the first set entry is the mode that runs.
// id: the flag's bit in `older`, the flags a mode refuses to be combined with; they are named in the bits' order, which is the order the flags came to be.
enum : unsigned { O_M = 1, O_C = 2, O_MS = 4, O_MEMS = 8, O_EXTEND = 16, O_PSEUDO_MS = 32, O_LOCATE = 64, O_SEQ_COUNT = 128, O_LOCI = 256, O_APPROX = 512, O_SCREEN = 1024 };
enum Strands { S_NONE, S_BOTH, S_ONE };          // what --dry-run says of the strands: nothing, 2 with --both-strands, 1 with --one-strand
struct Mode {
    const char* flag;          // as spelled in messages
    unsigned id, older;
    bool Args::*set;
    const char* suffix; const char* suffix2;          // of the output file(s); with one, the output is named <patterns>_<index> by default; without, the mode writes SAM
    const char* dry; Strands strands;                 // --dry-run: mode=...
    bool seq_names;                                   // its lines name the index's sequences
    const char* label;                                // of the summary line
    RunFn* run;
};
static const char L_ALIGNED[] = "Number of aligned reads: ", L_OCCUR[] = "Number of patterns that occur: ";
static const Mode MODES[] = {
    {"--ms", O_MS, 0, &Args::legacy_ms, ".pointers", ".lengths", nullptr, S_NONE, false, L_ALIGNED, run_ms},
    {"--mems", O_MEMS, 0, &Args::legacy_mems, ".mems", nullptr, nullptr, S_NONE, false, L_ALIGNED, run_ms},
    {"--pseudo-ms", O_PSEUDO_MS, O_PSEUDO_MS - 1, &Args::pseudo_ms, ".pseudo_lengths", nullptr, "pseudo-ms", S_NONE, false, "Number of reads with a pseudo-matching length >= -l: ", run_pseudo_ms},
    {"--screen", O_SCREEN, O_SCREEN - 1, &Args::screen, ".screen", nullptr, "screen", S_ONE, false, "Number of reads called present: ", run_screen},
    {"--locate", O_LOCATE, O_LOCATE - 1, &Args::locate, ".locate", nullptr, "locate", S_BOTH, true, L_OCCUR, run_locate},
    {"--seq-count", O_SEQ_COUNT, O_SEQ_COUNT - 1, &Args::seq_count, ".seqcount", nullptr, "seq-count", S_BOTH, true, L_OCCUR, run_seq_count},
    {"--loci", O_LOCI, (O_LOCI - 1) | O_APPROX, &Args::loci, ".loci", nullptr, "loci", S_BOTH, true, L_OCCUR, run_loci},
    {"--approx", O_APPROX, O_LOCI - 1, &Args::approx, ".approx", nullptr, "approx", S_BOTH, true, L_OCCUR, run_approx},          // (it does not name --loci: --loci names it)
    {"--extend", O_EXTEND, O_EXTEND - 1, &Args::extend, nullptr, nullptr, "extend", S_NONE, false, "Number of extended reads: ", run_extend},          // (extend_reads_dispatcher.hpp:478)
    {"-m", O_M, 0, &Args::report_mems, nullptr, nullptr, nullptr, S_NONE, false, L_ALIGNED, run_report_mems},
    {"-c", O_C, 0, &Args::csv, nullptr, nullptr, nullptr, S_NONE, false, L_ALIGNED, run_csv},
};

// Mode `id`, if set: single-end input, and none of the older flags it refuses beside it (the first of them in their order is the one named).
static bool mode_alone(const Args& a, unsigned id, bool paired) {
    const Mode* M = nullptr;
    for (const Mode& m : MODES) if (m.id == id) M = &m;
    if (!(a.*M->set)) return false;
    if (paired) die(std::string(M->flag) + " takes single-end input (-p), not -1 / -2");
    for (unsigned bit = 1; bit < O_SCREEN; bit <<= 1)
        for (const Mode& o : MODES) if ((M->older & bit) && o.id == bit && a.*o.set) die(std::string(M->flag) + " cannot be combined with " + o.flag);
    return true;
}

// The output flags in the order that decides which message a wrong combination gets.  A set flag wants `needs` beside it, then refuses its `extras` in their
// order, then - where it is a form of the SAM output (`sam`) - every mode that writes files of its own, in the table's order; `after` has the last word.
struct Beside { bool Args::*set; const char* flag; };
struct OutputFlag { Beside self, needs; Beside extras[3]; bool sam; void (*after)(const Args&); };
static const Beside B_BGZF = {&Args::bgzf, "--bgzf"}, B_C = {&Args::csv, "-c"}, B_DRY_WRITE = {&Args::dry_write, "--dry-run-write"};
static const OutputFlag OUTPUT_FLAGS[] = {
    {{&Args::bgzf, "--bgzf"}, {}, {B_C, B_DRY_WRITE}, true, nullptr},
    {{&Args::sort, "--sort"}, {&Args::bam, "--bam"}, {B_BGZF, B_C, B_DRY_WRITE}, true, [](const Args& a) {
        if (a.sort ? a.sort_chunk < 65536 : a.sort_chunk_set) die(a.sort ? "--sort-chunk takes at least 65536 bytes" : "--sort-chunk belongs to --sort");
    }},
    // duplicate marking: a decision over the whole input, so it lives between the two phases of the sort; one record per read
    {{&Args::mark_dup, "--mark-dup"}, {&Args::sort, "--sort"}, {{&Args::extend, "--extend"}, {&Args::report_mems, "-m"}}, false, nullptr},
    // depth of coverage: added where the sorted records lie, so it lives in the second phase of the sort
    {{&Args::coverage, "--coverage"}, {&Args::sort, "--sort"}, {{&Args::extend, "--extend"}, {&Args::report_mems, "-m"}}, false, [](const Args& a) {
        if (a.cov_window_set && (!a.coverage || a.cov_window_bad)) die(a.coverage ? "--cov-window takes 1 to 2147483647 bases" : "--cov-window belongs to --coverage");
        if (a.cov_mapq_set && (!a.coverage || a.cov_mapq_bad)) die(a.coverage ? "--cov-mapq takes 0 to 255" : "--cov-mapq belongs to --coverage");
        if (a.coverage && a.gpus > 1) die("--coverage takes one GPU (--gpus 1)");
    }},
    {{&Args::bam, "--bam"}, {}, {B_BGZF, B_C, B_DRY_WRITE}, true, nullptr},          // one container
};
static void check_output_flags(const Args& a) {
    for (const OutputFlag& f : OUTPUT_FLAGS) {
        if (a.*f.self.set) {
            const std::string clash = std::string(f.self.flag) + " cannot be combined with ";
            if (f.needs.set && !(a.*f.needs.set)) die(std::string(f.self.flag) + " belongs to " + f.needs.flag);
            for (const Beside& e : f.extras) if (e.set && a.*e.set) die(clash + e.flag);
            for (const Mode& m : MODES) if (f.sam && m.suffix && a.*m.set) die(clash + m.flag);
        }
        if (f.after) f.after(a);
    }
}

int main(int argc, char** argv) {
    // HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues; every context runs its launches on several streams (the paired
    // path on ~11), and streams that share a queue run one after the other
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    Args a;
    parse(argc, argv, a);
    // several contexts per GPU keep it busy by themselves: the library's sub-batches can be larger then (fewer, longer launches; bench.py --inflight, profiles/r04o)
    if (a.ctx_per_gpu >= 2) setenv("MONI_ALIGN_SUB", "500000", 0);
    // -Z (secondary chains) acts in the paired path only, as in the reference (aligner_ksw2.hpp:1190-1191): run_paired passes it on; single-end input ignores it
    // -n: <prefix>.thrbv.full.ms (ms_pointers<>: no LCP samples; the occurrence walks measure the LCP on the text, seed_finder.hpp:346-370).
    // -q: the reference would take the text from <prefix>.slp (SelfShapedSlp) instead of <prefix>.plain.slp; both grammars spell the same
    //     text and neither is read here - the text is rebuilt from the BWT - so the flag changes nothing (align_full_ksw2.cpp:414-426)
    if (!a.interleaved.empty() && (!a.patterns.empty() || !a.mate1.empty() || !a.mate2.empty())) die("--interleaved cannot be combined with -p, -1 or -2: it names the one file of both mates");
    const bool paired = !a.mate1.empty() || !a.mate2.empty() || !a.interleaved.empty();
    if (paired && a.interleaved.empty() && (a.mate1.empty() || a.mate2.empty())) die("paired-end alignment needs both -1 and -2");
    if (paired && (a.legacy_ms || a.legacy_mems)) die("--ms / --mems take single-end input (-p)");
    if (a.split && !(a.legacy_ms || a.legacy_mems)) die("--split belongs to --ms / --mems");
    if ((a.seg_len_set || a.overlap_set) && !a.split) die("--seg-len / --overlap belong to --split");
    if (a.seg_len_set && a.seg_len < 8) die("--seg-len must be at least 8");
    // one mode at a time: the modes' checks in the order that decides which message a wrong combination gets; between them, the options that belong to one mode
    mode_alone(a, O_PSEUDO_MS, paired);
    if (mode_alone(a, O_SCREEN, paired)) {
        a.SP.strands = a.one_strand ? 1 : 2;
        if (a.SP.window < 8 || a.SP.window > 65535) die("--window takes 8 to 65535");
        if (a.SP.min_win < 1 || a.SP.min_win > a.SP.window) die("--min-win takes 1 to --window");
        if (a.SP.ks_num < 1 || a.SP.ks_num > a.SP.ks_den || a.SP.ks_den > 65535) die("--ks takes NUM/DEN with 1 <= NUM <= DEN <= 65535");
    } else if (a.screen_opt) die("--window / --min-win / --ks / --one-strand belong to --screen");
    if (!mode_alone(a, O_LOCATE, paired) && !a.approx && ((a.both_strands && !a.seq_count && !a.loci) || a.max_occ)) die("--max-occ / --both-strands belong to --locate");
    if (!mode_alone(a, O_SEQ_COUNT, paired) && a.max_walk_set && !a.loci) die("--max-walk belongs to --seq-count / --loci");
    if (!mode_alone(a, O_LOCI, paired) && a.no_lift) die("--no-lift belongs to --loci");
    if (a.approx && a.approx_k > MONI_APPROX_MAX_K) die("--approx takes 0 to " + std::to_string(MONI_APPROX_MAX_K) + " mismatches");
    if (mode_alone(a, O_APPROX, paired)) {
        if (a.max_occ && !a.max_hits) die("--approx: --max-occ needs --max-hits above 0");
    } else if (a.max_hits_set || a.max_steps_set) die("--max-hits / --max-steps belong to --approx");
    mode_alone(a, O_EXTEND, paired);
    check_output_flags(a);
    if (!paired && a.patterns.empty()) die("no reads given (-p)");
    std::string fn = a.filename;
    std::vector<char> tmp(fn.begin(), fn.end()); tmp.push_back(0);
    const std::string base_name = basename(tmp.data());
    std::string sam_filename = (!a.interleaved.empty() ? a.interleaved : paired ? a.mate1 : a.patterns) + "_" + base_name + "_" + std::to_string(a.P.min_len) + ".sam";   // align_full_ksw2.cpp:347-353
    if (!a.output.empty()) sam_filename = a.output;
    if (a.bgzf) sam_filename += ".gz";
    if (a.bam) {             // a trailing .sam becomes .bam
        if (sam_filename.size() >= 4 && !sam_filename.compare(sam_filename.size() - 4, 4, ".sam")) sam_filename.resize(sam_filename.size() - 4);
        sam_filename += ".bam";
    }
    if (paired) return run_paired(a, sam_filename);
    const bool legacy = a.legacy_ms || a.legacy_mems;
    const Mode* M = nullptr;          // the mode that runs; none: plain alignment
    for (const Mode& m : MODES) if (a.*m.set) { M = &m; break; }
    if (M && M->suffix && a.output.empty()) sam_filename = a.patterns + "_" + base_name;       // mems.cpp / matching_statistics.cpp / run_spumoni.cpp: <patterns>_<index> + .mems / .pointers / .lengths / .pseudo_lengths (and .locate / .seqcount)
    info("Output file: " + sam_filename);
    if (looks_like_bam(a.patterns)) {          // BAM is read on the GPU, by the streaming path of plain alignment alone
        if (M) die(std::string(M->flag) + " does not take BAM input");
        if (a.host_inflate) die("--host-inflate cannot be combined with BAM input: there is no host BAM parser, the records are read on the GPU");
        if (getenv("MONI_CLI_QUEUE_PATH")) die("the queue path does not take BAM input");
        require_bgzf_bam(a.patterns);
        if (a.dry_run) {
            const BamCount c = bam_dry_count(a.patterns);
            printf("dry-run: reads=%zu bases=%zu min_len=%u ext_len=%u S=%u F=%.2f O=%d,%d E=%d,%d threads=%zu gpus=%d out=%s first=%s%s input=bam\n", c.reads, c.bases, a.P.min_len,
                   a.P.ext_len, a.P.n_seeds_thr, a.P.freq_thr, a.P.gapo, a.P.gapo2, a.P.gape, a.P.gape2, a.th, a.gpus, sam_filename.c_str(), c.first.c_str(), output_word(a));
            return 0;
        }
    }
    BgzfInput bzin;          // BGZF input of plain alignment: inflated on the GPU; counting (--dry-run) stays with the Reader
    const bool bz = !a.host_inflate && !M && getenv("MONI_CLI_QUEUE_PATH") == nullptr && bzin.open(a.patterns);
    MappedReader mrd;
    const bool mapped = mrd.open(a.patterns);
    Reader* zrd = mapped ? nullptr : new Reader(a.patterns);
    auto next_record = [&](Batch& b) { return mapped ? mrd.next(b) : zrd->next(b); };
    if (a.dry_run) {
        Batch b; size_t n = 0, bases = 0;
        while (next_record(b)) { ++n; }
        bases = b.seq.size();
        std::string mode;
        if (M && M->dry) {
            mode = std::string(" mode=") + M->dry;
            if (M->id == O_APPROX) mode += " k=" + std::to_string(a.approx_k);
            if (M->strands) mode += (M->strands == S_ONE ? !a.one_strand : a.both_strands) ? " strands=2" : " strands=1";
        }
        printf("dry-run: reads=%zu bases=%zu min_len=%u ext_len=%u S=%u F=%.2f O=%d,%d E=%d,%d threads=%zu gpus=%d out=%s first=%.*s%s%s%s\n", n, bases, a.P.min_len,
               a.P.ext_len, a.P.n_seeds_thr, a.P.freq_thr, a.P.gapo, a.P.gapo2, a.P.gape, a.P.gape2, a.th, a.gpus, sam_filename.c_str(),
               n ? (int)b.name_off[1] : 0, n ? (const char*)b.names.data() : "", mode.c_str(), output_word(a), bz ? " input=bgzf" : "");
        if (!a.dry_write || !mapped) return 0;
    }
    const bool fast = (mapped || bz) && !M && getenv("MONI_CLI_QUEUE_PATH") == nullptr;
    const int per_gpu = legacy ? 1 : (fast ? a.ctx_per_gpu : 2);                      // contexts (batches in flight) per GPU
    std::vector<moni_index_t*> idx(a.gpus, nullptr);
    std::vector<moni_ctx_t*> ctx((size_t)a.gpus * per_gpu, nullptr);
    for (int g = 0; g < a.gpus && !a.dry_write; ++g) {
        idx[g] = load_index(a, g);
        for (int k = 0; k < per_gpu; ++k) if (moni_ctx_create(idx[g], &ctx[(size_t)g * per_gpu + k])) die("cannot create a context on GPU " + std::to_string(g));
    }
    Sink sink;          // the output of the modes that write SAM; --sort: a range or batch is a run
    if (fast) {
        using namespace fastpath;
        const auto t0 = std::chrono::steady_clock::now();
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const char* base = mrd.p; const char* end = mrd.p + mrd.n;
        const bool fq = bz ? bzin.fq : base[0] == '@';
        // record-aligned ranges of about gpu_batch reads (the first record's size is the estimate); BGZF input: a range is a chunk of the inflater's
        const char* r1 = base; for (int k = 0; k < (fq ? 4 : 2) && !bz; ++k) r1 = next_line(r1, end);
        const size_t rec_bytes = std::max<size_t>((size_t)(r1 - base), 8), chunk_bytes = std::max<size_t>(rec_bytes * a.gpu_batch, 1 << 16);
        std::vector<const char*> cuts(1, base);
        if (bz) bzin.start(idx[0], a.inflate_blocks);
        while (!bz && cuts.back() < end) { const char* nx = (size_t)(end - cuts.back()) <= chunk_bytes + chunk_bytes / 4 ? end : align_record(cuts.back() + chunk_bytes, base, end, fq); if (nx <= cuts.back()) nx = end; cuts.push_back(nx); }
        const size_t n_chunks = bz ? bzin.n_chunks() : cuts.size() - 1;
        sink.open(sam_filename, a, false);
        if (!a.dry_write) sink.begin(idx[0], ctx);
        std::atomic<size_t> next_chunk{0};
        std::atomic<size_t> processed{0}, aligned{0};
        const int P = (int)std::max<size_t>(1, std::min<size_t>(8, a.th / std::max<size_t>(1, ctx.size() / (size_t)a.gpus)));      // helper threads of one worker
        std::vector<double> t_parse(ctx.size(), 0), t_lib(ctx.size(), 0), t_wait(ctx.size(), 0), t_write(ctx.size(), 0);
        const bool verbose_ranges = getenv("MONI_CLI_VERBOSE") != nullptr;
        auto worker = [&](int w) {
            ParsedBatch B;
            while (true) {
                size_t id;
                TextChunk tc;
                double x0 = now();
                if (bz) {
                    if (!bzin.next(tc)) return;
                    id = tc.id;
                    x0 = now();
                    parse_range(tc.p, tc.p + tc.n, tc.p, tc.p + tc.n, fq, P, B);
                    bzin.recycle(tc);
                } else {
                    id = next_chunk.fetch_add(1);
                    if (id >= n_chunks) return;
                    parse_range(cuts[id], cuts[id + 1], base, end, fq, P, B);
                }
                double x1 = now(); t_parse[w] += x1 - x0;
                Block z{nullptr, 0};          // the range's bytes for the file
                moni_align_stats_t st; memset(&st, 0, sizeof st);
                std::string placeholder;
                if (a.dry_write) {          // one unaligned record per read (what the library returns for a read without seeds), worker id in a tag
                    for (size_t r = 0; r < B.n; ++r) {
                        placeholder.append((const char*)B.names.p + B.name_off[r], (size_t)(B.name_off[r + 1] - B.name_off[r]));
                        placeholder += "\t4\t*\t0\t255\t*\t*\t0\t0\t";
                        placeholder.append((const char*)B.seq.p + B.off[r], (size_t)(B.off[r + 1] - B.off[r]));
                        placeholder += "\t";
                        if (fq) placeholder.append((const char*)B.qual.p + B.off[r], (size_t)(B.off[r + 1] - B.off[r])); else placeholder += "*";
                        placeholder += "\tXW:i:" + std::to_string(w) + "\n";
                    }
                    z = {placeholder.data(), placeholder.size()};
                    std::this_thread::sleep_for(std::chrono::milliseconds(3));          // (a library call takes longer than that: the other workers get their ranges)
                } else if (B.n) {
                    moni_read_batch_t rb{B.seq.p, B.off.data(), (uint64_t)B.n};
                    char* sam = nullptr; uint64_t len = 0;
                    if (moni_align_stream(ctx[w], &rb, B.names.p, B.name_off.data(), fq ? B.qual.p : nullptr, &a.P, &sam, &len, &st)) die("moni_align_stream failed");
                    z = sink.encode(ctx[w], id, sam, len);          // the text in the context's pinned buffer, and so are its blocks
                }
                double x2 = now(); t_lib[w] += x2 - x1;
                const uint64_t at = sink.place(id, z.n);
                double x3 = now(); t_wait[w] += x3 - x2;
                sink.write(z.p, z.n, at, P);
                const double x4 = now();
                t_write[w] += x4 - x3;
                if (verbose_ranges) fprintf(stderr, "range %zu (worker %d, %zu reads): parse %.0f ms, library %.0f ms (seed %.0f, align kernels %.0f), wait %.0f ms, write %.0f ms, done at %.3f s\n", id, w, B.n,
                                            (x1 - x0) * 1e3, (x2 - x1) * 1e3, st.t_seed * 1e3, st.t_dp_kernel * 1e3, (x3 - x2) * 1e3, (x4 - x3) * 1e3,
                                            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
                processed += B.n; aligned += st.aligned;
            }
        };
        std::vector<std::thread> th;
        for (size_t w = 0; w < ctx.size(); ++w) th.emplace_back(worker, (int)w);
        for (auto& t : th) t.join();
        if (bz) bzin.finish();
        sink.finish(ctx);
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        info("Number of aligned reads: " + std::to_string(aligned.load()) + "/" + std::to_string(processed.load()));
        info("Elapsed time (s): " + std::to_string(el));
        info("Reads per second: " + std::to_string(processed.load() / (el > 0 ? el : 1)));
        double sp = 0, sl2 = 0, sw = 0, sr = 0;
        for (size_t w = 0; w < ctx.size(); ++w) { sp += t_parse[w]; sl2 += t_lib[w]; sw += t_wait[w]; sr += t_write[w]; }
        info("Stage seconds summed over " + std::to_string(ctx.size()) + " workers (" + std::to_string(n_chunks) + " ranges, " + std::to_string(P) + " helper threads each): parse " + std::to_string(sp) +
             ", library calls " + std::to_string(sl2) + ", waiting for the block's place " + std::to_string(sw) + ", file writes " + std::to_string(sr));
        for (size_t w = 0; w < ctx.size(); ++w) if (ctx[w]) moni_ctx_destroy(ctx[w]);
        for (int g = 0; g < a.gpus; ++g) if (idx[g]) moni_index_destroy(idx[g]);
        return 0;
    }
    if (a.dry_write) return 0;
    FILE* out = nullptr; FILE* out2 = nullptr;          // the files of a pattern mode; out2 also <sam>.csv
    const bool sam_out = !(M && M->suffix);
    if (M && M->suffix) {
        out = fopen((sam_filename + M->suffix).c_str(), "w");
        if (M->suffix2) out2 = fopen((sam_filename + M->suffix2).c_str(), "w");
        if (!out || (M->suffix2 && !out2)) die("open() file " + sam_filename + M->suffix + (M->suffix2 ? std::string("/") + M->suffix2 : "") + " failed");
    } else {
        sink.open(sam_filename, a, false);
        sink.begin(idx[0], ctx);
        if (a.csv) {          // -c: <sam>.csv (align_reads_dispatcher.hpp:302,334-339), header of aligner::to_csv (aligner_ksw2.hpp:3230-3234)
            out2 = fopen((sam_filename + ".csv").c_str(), "w");
            if (!out2) die("open() file " + sam_filename + ".csv failed");
            static const char hdr[] = "Read,Unique,Total,Max_Freq,Min_Freq,Highest_Occ,Lowest_Occ,Filtered,Chains_Skipped\n";
            put(hdr, sizeof hdr - 1, out2);
        }
    }
    Names seq_names;          // the sequences' names, from the header's @SQ lines (one per sequence of the concatenation, in order)
    if (M && M->seq_names) {
        char* h; uint64_t hl; if (moni_sam_header(idx[0], &h, &hl)) die("header");
        const std::string hs(h, hl); moni_free(h);
        for (size_t at = 0; (at = hs.find("@SQ\tSN:", at)) != std::string::npos;) { at += 7; seq_names.push_back(hs.substr(at, hs.find('\t', at) - at)); }
    }
    size_t batch_cap = a.gpu_batch;          // reads per GPU batch; --seq-count keeps the dense table (tasks x sequences x 8 bytes) below 1 GiB
    if (a.seq_count) batch_cap = std::min(batch_cap, std::max<size_t>(1, (((size_t)1 << 27) - 1) / (std::max<size_t>(1, seq_names.size()) * (a.both_strands ? 2 : 1))));
    // --approx keeps the hit region (tasks x --max-hits records of 40 bytes) below 1 GiB
    if (a.approx) batch_cap = std::min(batch_cap, std::max<size_t>(1, ((size_t)1 << 30) / (sizeof(moni_approx_hit_t) * std::max<size_t>(1, a.max_hits) * (a.both_strands ? 2 : 1))));
    auto t0 = std::chrono::steady_clock::now();
    // ---- reader thread -> bounded queue of parsed batches -> workers -> bounded in-order window -> writer thread ----
    struct Item { size_t id; Batch* b; size_t first; };      // first: the running number of the batch's first read in the input
    std::mutex mu_q, mu_out;
    std::condition_variable cv_q_put, cv_q_get, cv_out, cv_window;
    std::deque<Item> queue;
    bool reader_done = false;
    const size_t q_cap = (size_t)a.gpus * per_gpu + 2, window = 2 * (size_t)a.gpus * per_gpu + 2;
    size_t next_out = 0, n_batches = 0, processed = 0, aligned = 0;
    double t_reader = 0, t_writer = 0, t_align = 0, t_wait_window = 0;      // busy seconds of the stages (t_align summed over the workers)
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    bool workers_done = false;
    std::map<size_t, Done> done;
    std::thread reader([&]() {
        size_t id = 0, n_read = 0;
        while (true) {
            const double r0 = now();
            Batch* b = new Batch();
            b->seq.reserve(a.gpu_batch * 160); b->qual.reserve(a.gpu_batch * 160); b->names.reserve(a.gpu_batch * 24);
            // the matching-statistics workspace of a batch is strided by its longest read (2 x reads x longest x 8 bytes): the legacy modes,
            // which take long patterns, close a batch when that product passes 2^28 entries (4 GB)
            size_t longest = 0;
            while (b->n() < batch_cap && next_record(*b)) {
                if (a.split) { if (b->seq.size() >= ((size_t)1 << 28)) break; continue; }      // --split: a batch is closed by its bases (12 bytes each on the device), not by its reads
                if (!legacy) continue;
                longest = std::max(longest, (size_t)(b->off[b->n()] - b->off[b->n() - 1]));
                if (b->n() * longest > ((size_t)1 << 28)) break;
            }
            t_reader += now() - r0;
            if (b->n() == 0) { delete b; break; }
            std::unique_lock<std::mutex> lk(mu_q);
            cv_q_put.wait(lk, [&] { return queue.size() < q_cap; });
            const size_t first = n_read;
            n_read += b->n();
            queue.push_back(Item{id++, b, first});
            cv_q_get.notify_one();
        }
        std::lock_guard<std::mutex> lk(mu_q);
        reader_done = true; n_batches = id;
        cv_q_get.notify_all();
    });
    std::thread writer([&]() {
        while (true) {
            Done d;
            {
                std::unique_lock<std::mutex> lk(mu_out);
                cv_out.wait(lk, [&] { return (!done.empty() && done.begin()->first == next_out) || workers_done; });
                if (done.empty() || done.begin()->first != next_out) { if (workers_done && done.empty()) return; if (workers_done) die("a batch is missing from the output"); continue; }
                d = std::move(done.begin()->second);
                done.erase(done.begin());
                ++next_out;
                cv_window.notify_all();
            }
            const double w0 = now();
            if (sam_out) sink.append(d.a, d.la); else put(d.a, d.la, out);
            if (d.a) moni_free(d.a);
            if (out2 && !d.b.empty()) put(d.b.data(), d.b.size(), out2);
            t_writer += now() - w0;
        }
    });
    auto worker = [&](int w) {
        moni_ctx_t* C = ctx[w];
        while (true) {
            Item it;
            {
                std::unique_lock<std::mutex> lk(mu_q);
                cv_q_get.wait(lk, [&] { return !queue.empty() || reader_done; });
                if (queue.empty()) return;
                it = queue.front(); queue.pop_front();
                cv_q_put.notify_one();
            }
            Batch& b = *it.b;
            const moni_read_batch_t rb{b.seq.data(), b.off.data(), b.n()};
            Done d;
            const double a0 = now();
            const size_t n_al = (M ? M->run : run_align)(C, b, rb, it.first, a, seq_names, d);
            if (sam_out) {
                const Block z = sink.encode(C, it.id, d.a, d.la);
                if (z.p != d.a) {          // blocks in this worker's context's pinned buffer, which is the context's next call's: a copy of them waits for the writer
                    moni_free(d.a);
                    d.a = nullptr; d.la = z.n;
                    if (z.n) { d.a = (char*)malloc(z.n); if (!d.a) die("out of memory"); memcpy(d.a, z.p, z.n); }
                }
            }
            const size_t n_reads = b.n();
            delete it.b;
            const double a1 = now();
            std::unique_lock<std::mutex> lk(mu_out);
            cv_window.wait(lk, [&] { return it.id < next_out + window; });
            t_align += a1 - a0; t_wait_window += now() - a1;      // bounded: a slow writer holds the workers back instead of the heap growing
            done[it.id] = std::move(d);
            processed += n_reads; aligned += n_al;
            cv_out.notify_one();
        }
    };
    std::vector<std::thread> th;
    for (size_t w = 0; w < ctx.size(); ++w) th.emplace_back(worker, (int)w);
    reader.join();
    for (auto& t : th) t.join();
    { std::lock_guard<std::mutex> lk(mu_out); workers_done = true; cv_out.notify_all(); }
    writer.join();
    if (sam_out) sink.finish(ctx);
    close_out(out);
    close_out(out2);
    delete zrd;
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    info(std::string(M ? M->label : L_ALIGNED) + std::to_string(aligned) + "/" + std::to_string(processed));
    info("Elapsed time (s): " + std::to_string(el));
    info("Reads per second: " + std::to_string(processed / (el > 0 ? el : 1)));
    info("Stage busy seconds: reader (parse) " + std::to_string(t_reader) + ", library calls summed over " + std::to_string(ctx.size()) + " workers " + std::to_string(t_align) +
         ", writer " + std::to_string(t_writer) + ", workers held back by the writer " + std::to_string(t_wait_window));
    for (size_t w = 0; w < ctx.size(); ++w) moni_ctx_destroy(ctx[w]);
    for (int g = 0; g < a.gpus; ++g) moni_index_destroy(idx[g]);
    return 0;
}
