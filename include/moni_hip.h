/*
 * moni_hip.h — C ABI of libmoni_hip.so, the MI355X (gfx950) implementation of the moni-align
 * per-read hot path.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * The reference has no FFI layer of its own: its seams are C++ template
 * concepts and one C function from ksw2.  Each entry point below names the reference interface
 * it stands in for (paths relative to the reference checkout).
 *
 * Conventions: opaque handles; every function returns 0 on success and a negative MONI_E* code
 * on failure and never calls exit(); the caller owns every input buffer; the library owns all
 * device memory; one moni_ctx_t per host thread / HIP stream (not thread-safe per ctx, thread-safe
 * across ctxs — mirrors include/aligner/align_reads_dispatcher.hpp:226-235: shared const index,
 * per-thread everything else).
 *
 * What runs where: every kernel-side stage of the path runs on the GPU only - without a HIP device moni_index_create returns
 * MONI_ENODEV, and nothing under oracle/ is linked or called.  The library does contain host code that is part of the product,
 * not a fallback for a missing GPU: (1) the "host pipeline" (align_host.hpp, pe_host.hpp, pe_big.cpp) redoes, with DP batches on
 * the GPU, the few reads or pairs whose seeds / anchors / chains / CIGAR exceed even the general kernel's capacities (0 reads per
 * 1 M in the benchmark; the statistics report them as handed_back), and (2) moni_align_csv_batch (`-c`) sends EVERY read through
 * that host pipeline by design, because the per-read MEM statistics are taken inside its chaining loop.
 */
#ifndef MONI_HIP_H
#define MONI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MONI_OK 0
#define MONI_EINVAL (-22)
#define MONI_ENOMEM (-12)
#define MONI_EIO (-5)
#define MONI_ENODEV (-19)   /* no HIP device / kernel launch failed */
#define MONI_ERANGE (-34)   /* index violates an invariant the device layout relies on */

typedef struct moni_index moni_index_t;   /* device-resident index image (one per GPU) */
typedef struct moni_ctx moni_ctx_t;       /* stream + workspaces + resident read batch */

/* Semantic content of <prefix>.thrbv.full.lcp.ms + .plain.slp + .ldx as flat host arrays
 * (field order of include/aligner/moni_lcp.hpp:208-225; values as built by
 * include/ms/moni.hpp:148-251, include/ms/ms_rle_string.hpp:245-303,
 * include/ms/thresholds_ds.hpp:393-430, include/common/seqidx.hpp:215-238). */
typedef struct {
    uint64_t n;              /* bwt.size() = text length + 1 */
    uint64_t r;              /* number of BWT runs */
    uint64_t w;              /* separator width */
    uint64_t n_seq;          /* number of sequences */
    const uint64_t *F;       /* [256] */
    const uint8_t *heads;    /* [r]   run heads (bytes <= 1 stored as 1) */
    const uint64_t *starts;  /* [r+1] run start positions, starts[r] = n */
    const uint64_t *ssa;     /* [r]   samples_start */
    const uint64_t *esa;     /* [r]   samples_last */
    const uint64_t *thr;     /* [r]   threshold position of each run, 0 = first run of its letter */
    const uint64_t *slcp;    /* [r]   LCP at each run start */
    const uint8_t *text;     /* [n-1] */
    const uint64_t *seq_starts; /* [n_seq+1] onsets in text coordinates */
    const char *seq_names;   /* n_seq NUL-terminated names back to back (seqidx names), or NULL */
    /* liftidx::lifts (include/aligner/liftidx.hpp:131-143), one lift::Lift per sequence, or all NULL for a FASTA-built
     * index (null lifts, liftidx.hpp:150-157): lift_second[i] = start of the target contig in the concatenation,
     * lift_len[i] = alignment columns, sorted positions of the ones of the levioSAM ins / del bit-vectors (ragged). */
    const uint64_t *lift_second;  /* [n_seq] */
    const uint64_t *lift_len;     /* [n_seq] */
    const uint64_t *lift_ins_off; /* [n_seq+1] */
    const uint64_t *lift_ins;
    const uint64_t *lift_del_off; /* [n_seq+1] */
    const uint64_t *lift_del;
} moni_flat_index_t;

/* Ragged batch of reads: read i is seq[offsets[i] .. offsets[i+1]).  Replaces the kseq_t batches of
 * include/common/kpbseq.h:315-326 (kbseq_read). */
typedef struct {
    const uint8_t *seq;
    const uint64_t *offsets; /* [n_reads+1] */
    uint64_t n_reads;
} moni_read_batch_t;

/* One MEM / seed, fields of include/aligner/mems.hpp:31-60 (count_dict is internal). */
typedef struct {
    uint64_t pos;          /* position in the text */
    uint32_t len;
    uint32_t idx;          /* position in the read */
    uint32_t rpos;
    uint32_t mate;         /* MATE_1|MATE_F = 0, MATE_1|MATE_RC = 2 */
    uint32_t total_occ;
    uint32_t num_filtered;
    uint64_t occ_off;      /* into the occs array */
    uint32_t occ_cnt;
    uint32_t read;         /* read index in the batch */
} moni_mem_t;

/* Seeding parameters: seed_finder ctor (include/aligner/seed_finder.hpp:64-68). */
typedef struct {
    uint32_t min_len;      /* -l, default 25 */
    uint32_t filter_seeds; /* -f off, default on */
    uint32_t n_seeds_thr;  /* -S, wrapper default 1000 */
    uint32_t report_mems;  /* populate_seeds(mems, report_mems) */
} moni_seed_params_t;

/* ksw_extz_t result fields (lh3/ksw2 ksw2.h) of one DP problem. */
typedef struct {
    int32_t max, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, zdropped;
    uint32_t n_cigar;
    uint32_t cigar_off;    /* into the cigar pool */
} moni_dp_result_t;

/* One ksw_extz2_sse call: query = qseq[q_off .. q_off+qlen), target = tseq[t_off .. t_off+tlen), nt4 codes. */
typedef struct {
    uint64_t q_off, t_off;
    int32_t qlen, tlen;
    int32_t flag;          /* KSW_EZ_* */
    int32_t reserved;
} moni_dp_task_t;

typedef struct {
    int8_t m;              /* 5 */
    int8_t mat[25];        /* ksw_gen_simple_mat, include/aligner/aligner_ksw2.hpp:3199-3211 */
    int8_t q, e;           /* gapo 4, gape 2 */
    int32_t w, zdrop, end_bonus; /* -1, -1, 400 (aligner_ksw2.hpp:110-113) */
} moni_dp_params_t;

/* ---- index ------------------------------------------------------------------------------- */
/* Replaces seed_finder's loading of .thrbv.full.lcp.ms/.plain.slp/.ldx (seed_finder.hpp:64-124):
 * converts the semantic arrays to the device layout and uploads it to `device`.  flat->text may be NULL: the text is redundant with
 * the r-index and is then rebuilt on the device by inverting the BWT (LF walks from the 2 r sampled positions, each down to the next
 * smaller sample), and checked against the BWT's symbol counts. */
int moni_index_create(const moni_flat_index_t *flat, int device, moni_index_t **out);
/* Same, from a MONIFLT2 file written by moni_align_amd/index_build.py. */
int moni_index_load(const char *path, int device, moni_index_t **out);
void moni_index_destroy(moni_index_t *idx);
uint64_t moni_index_n(const moni_index_t *idx);
uint64_t moni_index_r(const moni_index_t *idx);
uint64_t moni_index_device_bytes(const moni_index_t *idx);
/* The text the index was built over (n - 1 bytes: what PlainSlp::expandSubstr(0, n - 1) returns, seed_finder.hpp:88-99), whether it was
 * handed over or rebuilt from the BWT. */
int moni_index_text(const moni_index_t *idx, uint8_t *out, uint64_t cap);

/* ---- context / resident batch ------------------------------------------------------------ */
int moni_ctx_create(moni_index_t *idx, moni_ctx_t **out);
void moni_ctx_destroy(moni_ctx_t *ctx);
/* Copy a read batch to HBM (replaces rc_copy_kseq_t + kseq storage; the reverse-complement strand is
 * derived on the device with the table of include/common/kpbseq.h:120-137). */
int moni_reads_upload(moni_ctx_t *ctx, const moni_read_batch_t *batch);
/* Exchange the resident batch with the one parked in `slot` (0..255; an unused slot holds an empty batch): a caller that cycles
 * through several batches (one rank's shard of a read set, align_reads_dispatcher.hpp:300-345 reads them one after the other) uploads
 * each once, parks it, and swaps it in before moni_align_run.  Pointer exchange only; no copy, no kernel. */
int moni_reads_swap(moni_ctx_t *ctx, uint32_t slot);

/* ---- matching statistics: ms_t::query (include/ms/moni.hpp:292-295, 568-624) -------------- */
/* Device-only run over the resident batch, both strands (aligner_ksw2.hpp:333-334). */
int moni_ms_run(moni_ctx_t *ctx);
/* Host-buffer form: pointers[2*offsets[i] + s*len_i + k] = pointer k of strand s (0 fwd, 1 rc) of read i. */
int moni_ms_query_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, uint64_t *pointers);

/* Legacy `moni ms` / `moni mems` (src/matching_statistics.cpp:236-278, src/mems.cpp:236-280): pointers and matching-statistics
 * lengths of every read as given (forward strand), pointers[offsets[i] - offsets[0] + k] / lengths[...] for read offset k. */
int moni_ms_lengths_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, uint64_t *pointers, uint64_t *lengths);

/* The same for patterns of genome length (a chromosome, an assembly): every pattern is cut into segments that are walked side by side, each
 * from `overlap` bases to the right of its end, the match lengths measured at the pointers tell which segments the cut cannot have touched,
 * and the others are walked once more, a run of neighbours by one lane, from the state of the accepted segment behind them (csrc/mslong_core.h,
 * DESIGN.md 7.7).  Output layout of moni_ms_lengths_batch; either output pointer may be NULL, not both.
 *   lengths  - the matching statistics: identical to moni_ms_lengths_batch's and to the reference's.
 *   pointers - valid (the text at pointers[k] agrees with the pattern over lengths[k] bases) but, where a pattern was cut, not necessarily the
 *              positions moni_ms_lengths_batch reports: any position with a maximal match qualifies.  With seg_len >= the longest pattern nothing
 *              is cut and they are identical too.
 * Device memory: the bytes, 8 bytes of pointer and 4 of length per base, 48 bytes per segment.  A pattern may have up to 2^32 - 1 bases
 * (MONI_ERANGE beyond); batch totals are 64-bit.  MONI_EINVAL: seg_len < 8, a non-zero reserved word, a NULL ctx / batch / params, both outputs
 * NULL.  An empty batch and empty patterns give MONI_OK.  The call replaces the resident batch by one no other entry point can run on
 * (moni_reads_upload again first).  seg_len is taken down to a multiple of 8 and a pattern's first segment shortened so that the later ones begin
 * at a multiple of 8 of the output index; a pattern of at most seg_len bases is one segment.  moni_last_kernel_ms(ctx, 0, ..) then gives the
 * speculative walk's time, (ctx, 1, ..) the length pass's, (ctx, 2, ..) the chain round's. */
typedef struct { uint32_t seg_len;   /* bases per segment, >= 8; default 4096 */
                 uint32_t overlap;   /* bases walked beyond a segment's end before it, >= 0; default 256 */
                 uint32_t reserved[2]; } moni_mslong_params_t;
typedef struct { uint64_t patterns, bases, segments, flagged, chain_runs;
                 uint64_t steps_spec, steps_chain, jumps;      /* LF steps of rounds 1 and 3, threshold jumps of both */
                 double t_walk, t_len, t_chain, t_total;       /* seconds, HIP events, transfers excluded except in t_total */
               } moni_mslong_stats_t;
void moni_mslong_params_default(moni_mslong_params_t *p);
int  moni_ms_long_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_mslong_params_t *prm,
                        uint64_t *pointers, uint64_t *lengths, moni_mslong_stats_t *stats);

/* ---- seeds: seed_finder::find_mems + populate_seeds (seed_finder.hpp:126-166, 258-318) ----- */
/* Device-only run (ms + mems + occurrences) over the resident batch. */
int moni_seed_run(moni_ctx_t *ctx, const moni_seed_params_t *prm);
/* Sizes of the last moni_seed_run. */
int moni_seed_counts(moni_ctx_t *ctx, uint64_t *n_mems, uint64_t *n_occs);
/* Copy the last result to host: mems in the order of the reference's per-read `mems` vector
 * (forward MEMs, reverse-complement MEMs, then for every MEM in that order its two halves),
 * read_mem_off[n_reads+1] delimits reads. */
int moni_seed_fetch(moni_ctx_t *ctx, moni_mem_t *mems, uint64_t *occs, uint64_t *read_mem_off);
/* Host-buffer form of the three calls above; *mems / *occs / *read_mem_off are malloc'ed, free with moni_free. */
int moni_seed_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_seed_params_t *prm,
                    moni_mem_t **mems, uint64_t *n_mems, uint64_t **occs, uint64_t *n_occs, uint64_t **read_mem_off);
void moni_free(void *p);

/* ---- phi: moni_lcp::Phi_lcp / Phi_inv_lcp (include/aligner/moni_lcp.hpp:230-272) ---------- */
int moni_phi_lcp_batch(moni_ctx_t *ctx, const uint64_t *pos, uint64_t n, int inverse, uint64_t *out_pos, uint64_t *out_lcp);

/* ---- seed extension: ksw_extz2_sse (thirdparty/ksw2; call sites aligner_ksw2.hpp:2812-3015) */
int moni_extz_batch(moni_ctx_t *ctx, const moni_dp_params_t *prm, const uint8_t *qseq, uint64_t qseq_len,
                    const uint8_t *tseq, uint64_t tseq_len, const moni_dp_task_t *tasks, uint64_t n_tasks,
                    moni_dp_result_t *results, uint32_t *cigar_pool, uint64_t cigar_pool_cap, uint64_t *cigar_pool_used);

/* ---- the whole single-end path: aligner::align (include/aligner/aligner_ksw2.hpp:314-521) over a batch --- */
/* aligner::config_t (aligner_ksw2.hpp:84-130) with the `moni align` wrapper defaults (pipeline/moni.in:748-768). */
typedef struct {
    uint32_t min_len, ext_len, check_k, region_dist;      /* 25, 100, 5, 10 */
    uint32_t filter_seeds, n_seeds_thr, filter_freq, left_mem_check; /* 1, 1000, 1, 1 */
    double freq_thr;                                      /* 0.5 */
    int8_t smatch, smismatch, gapo, gapo2, gape, gape2;   /* 2, 4, 4, 13, 2, 1 */
    int32_t end_bonus, w, zdrop;                          /* 400, -1, -1 */
    int64_t max_dist_x, max_dist_y, max_iter, max_pred, min_chain_score, min_chain_length; /* 500,100,10,5,40,1 */
    uint32_t host_threads;                                /* threads for the host stages (chaining, stitching, SAM) */
    uint32_t reserved;
} moni_align_params_t;

typedef struct {
    uint64_t reads, aligned, dp_tasks, dp_cells, dp_rounds;
    double t_seed, t_chain, t_dp, t_host;                 /* seconds: seeding incl. fetch, chaining, DP batches incl. transfers, other host work */
    double t_dp_kernel;                                   /* seconds inside the align / extz kernels (HIP events) */
    uint64_t handed_back;                                 /* reads that exceeded the align kernel's capacities and went through the host pipeline */
    uint64_t dp_reused, dp_cells_reused;                  /* DP problems (and their cells) answered from the per-read memo of identical problems; not in dp_tasks/dp_cells */
    uint64_t kernel_fallback;                             /* reads outside the staged kernels' common case, taken by the general align kernel */
    uint64_t dp_ref_bytes;                                /* text bytes of the DP targets (the R of SURVEY.md 8(d)) */
    double t_k_chain, t_k_dp, t_k_select, t_k_finish;     /* HIP-event seconds of the staged kernels by group, summed over the sub-batches (launches of two
                                                             streams overlap: the sum exceeds the span t_dp_kernel) */
    uint64_t handover_why[12];                            /* why reads left the staged kernels (their sum can exceed kernel_fallback + handed_back: a read is counted once per
                                                             reason met): 0 read of 512 bases or more, 1 seeds / anchors beyond the largest LDS instance, 2 chains, 3 chains to
                                                             score, 4 anchors of the chains to score, 5 a DP problem beyond the register tile, 6 (unused), 7 wildcard base or
                                                             direction-bit budget, 8 selection loop depends on a score, 9 extension short of the query end, 10 a queue or pool
                                                             full, 11 CIGAR / MD / line beyond the staging (host pipeline) */
    uint64_t dp_cells_cut;                                /* staged DP kernels: cells of the problems after an extension's target rows that cannot hold its result are
                                                             cut (dp_cells counts the problems as the reference poses them: qlen x tlen of every ksw_extz2_sse call) */
    uint64_t dp_slots;                                    /* ... and the cell slots those kernels ran (128 problems x the chunk's longest query x the target rows of its passes) */
    uint64_t runs_routed;                                 /* reads whose runs of anchors were chained with one lane per run (chain_runs_kernel), not in chain_plan_kernel */
} moni_align_stats_t;

void moni_align_params_default(moni_align_params_t *p);
/* Replaces the per-read loop of st_align/mt_align (include/aligner/align_reads_dispatcher.hpp:346-357): SAM records of
 * the batch in input order, no header.  names: ragged bytes with name_off[n_reads+1]; quals: same offsets as the reads
 * or NULL.  *sam is malloc'ed (moni_free). */
int moni_align_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                     const uint8_t *quals, const moni_align_params_t *prm, char **sam, uint64_t *sam_len,
                     moni_align_stats_t *stats);
/* The same over the batch that moni_reads_upload made resident (reads already in HBM when the call starts).  *sam points
 * into a buffer the context owns: valid until the next moni_align_run / moni_ctx_destroy on this context, NOT to be freed
 * (a streaming caller writes it out and calls again; the pages stay mapped between batches). */
int moni_align_run(moni_ctx_t *ctx, const uint8_t *names, const uint64_t *name_off, const uint8_t *quals,
                   const moni_align_params_t *prm, char **sam, uint64_t *sam_len, moni_align_stats_t *stats);
/* moni_align_batch for a streaming caller: reads in host memory (uploaded by the call, no host copy kept), *sam in the context-owned
 * pinned buffer of moni_align_run (valid until the next moni_align_run / moni_align_stream / moni_ctx_destroy on this context, NOT to
 * be freed): the lines arrive in read order by one DMA per sub-batch, no host thread touches the text. */
int moni_align_stream(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                      const uint8_t *quals, const moni_align_params_t *prm, char **sam, uint64_t *sam_len,
                      moni_align_stats_t *stats);
/* aligner::align with csv (-c; aligner_ksw2.hpp:340-343, 417, include/common/csv.hpp:26-67): the SAM records and, per read, one line
 * `name,unique MEMs,total occurrences,max frequency,min frequency,highest / lowest count on one genome,filtered,chains skipped` (no header:
 * aligner::to_csv, aligner_ksw2.hpp:3230-3234).  A diagnostics mode: every read takes the host pipeline over the GPU's seeds and DP batches
 * (the selection loop counts the chains it skips); both texts are malloc'ed (moni_free). */
int moni_align_csv_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                         const uint8_t *quals, const moni_align_params_t *prm, char **sam, uint64_t *sam_len,
                         char **csv, uint64_t *csv_len, moni_align_stats_t *stats);
/* aligner::align with report_mems (-m; aligner_ksw2.hpp:346-373): one secondary record per MEM occurrence.  *sam is malloc'ed. */
int moni_report_mems_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                           const uint8_t *quals, const moni_align_params_t *prm, char **sam, uint64_t *sam_len);
/* ---- the paired-end path: aligner::align(kpbseq_t*) (aligner_ksw2.hpp:888-918, 1000-1326, 1536-1640) -------------------------------- */
/* The batch holds the pairs interleaved: reads 2p and 2p+1 are mate 1 and mate 2 of pair p (kpbseq_t's two kbseq_t,
 * include/common/kpbseq.h:300-326).  find_orphan: orphan recovery (aligner_ksw2.hpp:1536-1640, 2329-2720) for the pairs that chain but fail
 * jointly; its local alignment is klib's ksw_align (an absent submodule) restated as plain DP with its tie rules. */
typedef struct {
    uint32_t filter_dir, find_orphan;                     /* 1, 1: aligner::config_t::filter_dir, find_orphan (aligner_ksw2.hpp:113,128) */
    double dir_thr;                                       /* 50.0 */
    uint64_t ins_learning_n;                              /* 1000 */
    uint64_t ins_learning_score_gap_threshold;            /* 0 */
    uint32_t secondary_chains, reserved;                  /* 0: -Z, find_chains_secondary instead of find_chains (include/aligner/chain.hpp:442-727, aligner_ksw2.hpp:1190-1191);
                                                           * the staged paired kernels keep the second track of the chaining in LDS (pe_plan_kernel's SEC instances) */
} moni_pe_params_t;
/* The insert-size model (aligner_ksw2.hpp:3252-3262): zero-initialise, feed batches to moni_pe_learn_batch until complete != 0 (or
 * the input ends), then align - the order of st_align's paired loop (align_reads_dispatcher.hpp:356-389). */
typedef struct {
    double mean, std_dev, variance, sample_variance, m2;
    uint64_t count;
    uint32_t complete, reserved;
} moni_pe_model_t;
void moni_pe_params_default(moni_pe_params_t *p);
/* aligner::learn_fragment_model (aligner_ksw2.hpp:816-885) over one batch: updates *model.  MONI_ERANGE: a pair exceeded the
 * kernel's capacities and those of the host pipeline for pairs behind it (32 k anchors, mates of 32 k bases). */
int moni_pe_learn_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_align_params_t *prm,
                        const moni_pe_params_t *pe, moni_pe_model_t *model);
/* The two SAM records of every pair, in input order, no header.  names / name_off / quals as in moni_align_batch (2N reads).
 * *sam is malloc'ed (moni_free). */
int moni_pe_align_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                        const uint8_t *quals, const moni_align_params_t *prm, const moni_pe_params_t *pe,
                        const moni_pe_model_t *model, char **sam, uint64_t *sam_len, moni_align_stats_t *stats);
/* The same for a streaming caller: *sam points into the pinned text buffer the context owns (moni_align_run's: valid until the next
 * moni_pe_align_stream / moni_pe_align_batch / moni_align_run / moni_align_stream / moni_ctx_destroy on this context, NOT to be freed).  The
 * two lines of every pair are written by the GPU and arrive in input order by one transfer per chunk of pairs; moni_pe_align_batch is this
 * call plus a copy into a malloc'ed block. */
int moni_pe_align_stream(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                        const uint8_t *quals, const moni_align_params_t *prm, const moni_pe_params_t *pe,
                        const moni_pe_model_t *model, char **sam, uint64_t *sam_len, moni_align_stats_t *stats);
/* The same over the interleaved pairs that moni_reads_upload made resident (reads already in HBM when the call starts; names and qualities
 * are host buffers as in moni_align_run); *sam in the context's buffer as for moni_pe_align_stream. */
int moni_pe_align_run(moni_ctx_t *ctx, const uint8_t *names, const uint64_t *name_off, const uint8_t *quals, const moni_align_params_t *prm,
                      const moni_pe_params_t *pe, const moni_pe_model_t *model, char **sam, uint64_t *sam_len, moni_align_stats_t *stats);
/* aligner::align(kpbseq_t*, out, csv_out) with csv (-c for pairs; aligner_ksw2.hpp:888-918, 1030-1031, 1066-1075, 1115-1118, 1354-1358;
 * include/common/csv.hpp:26-67): the SAM records of moni_pe_align_batch and one line of MEM statistics per PAIR under mate 1's name (the MEMs of a
 * pair are kept together: alignment.record_csv writes csv_m1 alone, aligner_ksw2.hpp:787-791).  A diagnostics mode like moni_align_csv_batch: the
 * counts of filtered MEMs and skipped chains exist only in the selection loop, so every pair takes the host's state machine (pe_big.cpp) over the GPU's
 * seeds and DP batches.  *sam and *csv are malloc'ed (moni_free). */
int moni_pe_align_csv_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                            const uint8_t *quals, const moni_align_params_t *prm, const moni_pe_params_t *pe,
                            const moni_pe_model_t *model, char **sam, uint64_t *sam_len, char **csv, uint64_t *csv_len,
                            moni_align_stats_t *stats);
/* aligner::align(paired_alignment_t&) with report_mems (-m for pairs; aligner_ksw2.hpp:1118-1180): one secondary record per occurrence of every MEM
 * the direction and frequency filters leave, under its mate's name.  *sam is malloc'ed. */
int moni_pe_report_mems_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off,
                              const uint8_t *quals, const moni_align_params_t *prm, const moni_pe_params_t *pe, char **sam, uint64_t *sam_len);
/* ---- extend mode: the legacy `moni extend` (include/extender/extender_ksw2.hpp, include/extender/extend_reads_dispatcher.hpp:435-486) ---- */
/* extender::config_t (extender_ksw2.hpp:82-102) with its defaults.  w and zdrop must stay negative (the full matrix, no z-drop: what the reference
 * passes); ext_len <= 512 and reads of at most 2048 bases (MONI_ERANGE beyond, as for a line or a CIGAR that exceeds the kernels' staging). */
typedef struct {
    uint32_t min_len, ext_len;                            /* 25, 100 */
    int8_t smatch, smismatch, gapo, gape;                 /* 2, 4, 4, 2 */
    int32_t end_bonus, w, zdrop;                          /* 400, -1, -1 */
    uint32_t reserved;
} moni_extend_params_t;
typedef struct {
    uint64_t reads, extended, records;                    /* extended: reads with a record on either strand (extend_reads_dispatcher.hpp:468-469) */
    uint64_t dp_tasks, dp_cells;                          /* ksw_extz2_sse calls and their qlen x tlen */
    double t_kernel;                                      /* seconds inside the kernels (HIP events; the chunks' transfers are not in it) */
} moni_extend_stats_t;
void moni_extend_params_default(moni_extend_params_t *p);
/* Replaces the per-read loop of st_extend (extend_reads_dispatcher.hpp:452-476): for every read, strand 0 then strand 1 (complement() of
 * common.hpp:556-571, reversed), extender::extend (extender_ksw2.hpp:192-244): find_longest_mem (261-296), one extension per side (306-399), the
 * stitched CIGAR, MD / NM and the record (401-511, 526-576, 595-675).  At most one record per strand, none for a strand that does not pass
 * score > min_score; no header, input order.  names / name_off / quals as in moni_align_batch.  *sam is malloc'ed (moni_free); an empty batch gives
 * MONI_OK and zero bytes.  Where this differs from the reference on purpose: a MEM at mem_pos <= ext_len takes text [0, mem_pos) reversed as its left
 * target (the reference reads ext_len - mem_pos bytes from position 0, extender_ksw2.hpp:343-346). */
int moni_extend_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const uint8_t *names, const uint64_t *name_off, const uint8_t *quals,
                      const moni_extend_params_t *prm, char **sam, uint64_t *sam_len, moni_extend_stats_t *stats);
/* The same over the batch that moni_reads_upload made resident; *sam points into the context's text buffer (moni_align_run's: valid until the next
 * *_run / *_stream / moni_extend_batch / moni_ctx_destroy on this context, NOT to be freed; NULL when there is no text). */
int moni_extend_run(moni_ctx_t *ctx, const uint8_t *names, const uint64_t *name_off, const uint8_t *quals, const moni_extend_params_t *prm,
                    char **sam, uint64_t *sam_len, moni_extend_stats_t *stats);
/* aligner::to_sam (aligner_ksw2.hpp:3213-3219): "@HD", one "@SQ" per sequence, "@PG".  Also extend mode's header (extender::to_sam,
 * extender_ksw2.hpp:739-745, whose "@HD" line is written with blanks - not valid SAM; this one has the tabs): every sequence of the concatenation
 * is listed, with or without lifts. */
int moni_sam_header(const moni_index_t *idx, char **sam, uint64_t *sam_len);

/* ---- pseudo-matching lengths: the legacy `moni pseudo-ms` (include/ms/spumoni.hpp:356-410; src/spumoni/run_spumoni.cpp:186-193) ---- */
/* SPUMONI's pseudo-matching lengths (PML) of every read, forward strand, bytes as they are: the walk of ms_t::query over the run-length BWT
 * and the thresholds, with one counter per read in place of the suffix-array sample - length + 1 on a BWT match, 0 on a threshold jump or on
 * a byte whose letter the BWT does not hold.  lengths[offsets[i] - offsets[0] + k] is the PML of read i at read offset k; read_max[i] the
 * read's largest PML (0 for an empty read); read_hits[i] the number of its offsets with PML >= thr.  Any of the three may be NULL, not all.
 * An empty batch gives MONI_OK and writes nothing. */
int moni_pml_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, uint32_t thr,
                   uint32_t *lengths, uint32_t *read_max, uint32_t *read_hits);
/* The same over the batch that moni_reads_upload made resident, device only: the results stay in HBM.  moni_last_kernel_ms(ctx, 0, ..) then
 * gives pml_kernel's time, (ctx, 6, ..) the whole run's (pack_kernel included); moni_last_counters the steps and the threshold jumps. */
int moni_pml_run(moni_ctx_t *ctx, uint32_t thr);
/* The results of the last moni_pml_run on this context (any pointer may be NULL); MONI_EINVAL before any run, and after another batch was
 * made resident (moni_reads_upload, moni_reads_swap, any *_batch call).  The call takes no capacities: it writes as many values as the batch
 * that was resident at moni_pml_run has - moni_pml_sizes gives the two figures - so `lengths` must hold *total_len and the other two
 * *n_reads values. */
int moni_pml_fetch(moni_ctx_t *ctx, uint32_t *lengths, uint32_t *read_max, uint32_t *read_hits);
/* What moni_pml_fetch would write: the reads and the bases of the batch of the last moni_pml_run (either pointer may be NULL);
 * MONI_EINVAL where moni_pml_fetch gives it. */
int moni_pml_sizes(moni_ctx_t *ctx, uint64_t *n_reads, uint64_t *total_len);

/* ---- read screening: present / absent calls from pseudo-matching lengths against the read's own null ---- */
/* Every read is walked as four strings: P0 its bytes as they are (the string of moni_pml_batch), P1 its reverse complement by the index's
 * complement table, and the reverse - not complemented - of each, N0 and N1: the same composition, no homology.  Offsets are cut into windows of
 * `window`; a window is scored if it holds at least min_win offsets.  The score of a window is the one-sided Kolmogorov-Smirnov numerator
 * D = max over v in 0 .. MONI_SCREEN_BINS - 2 of #{null lengths <= v} - #{pattern lengths <= v}, lengths clipped to MONI_SCREEN_BINS - 1; a scored
 * window of len offsets is positive when D * ks_den >= ks_num * len.  All arithmetic is integer. */
#define MONI_SCREEN_BINS 32
#define MONI_SCREEN_PRESENT 1u      /* 2 * n_pos[s] > n_win on either strand */
#define MONI_SCREEN_STRAND1 2u      /* n_pos[1] > n_pos[0] */
#define MONI_SCREEN_SHORT 4u        /* n_win == 0: never present */
typedef struct { uint32_t window;    /* 8 .. 65535 */
                 uint32_t min_win;   /* 1 .. window */
                 uint32_t ks_num, ks_den;   /* 1 <= ks_num <= ks_den <= 65535 */
                 uint32_t strands;   /* 1: P0 / N0 alone (the fields of strand 1 are 0), 2: both */
                 uint32_t reserved[3]; } moni_screen_params_t;
/* n_win: scored windows (the same on both strands); per strand s: n_pos[s] positive windows, d_max[s] the largest D of a scored window,
 * max_pml[s] the largest unclipped pseudo-matching length of Ps. */
typedef struct { uint32_t n_win, n_pos[2], d_max[2], max_pml[2], flags; } moni_screen_res_t;
void moni_screen_params_default(moni_screen_params_t *p);            /* window 50, min_win 25, ks 1/4, strands 2 */
/* Device-only run over the batch that moni_reads_upload made resident; one record per read stays in HBM, nothing per base or per window is
 * written.  MONI_EINVAL: a parameter outside its range, a non-zero reserved word, no resident batch.  moni_last_kernel_ms(ctx, 0, ..) then gives
 * screen_kernel's time, (ctx, 6, ..) the whole run's (pack_kernel included); moni_last_counters: [0] steps = 2 * strands * bases, [1] threshold
 * jumps of all strings, [2] those of the P0 strings alone. */
int moni_screen_run(moni_ctx_t *ctx, const moni_screen_params_t *prm);
/* What moni_screen_fetch would write: the reads of the batch of the last moni_screen_run (the pointer may be NULL); MONI_EINVAL before any run,
 * and after another batch was made resident (moni_reads_upload, moni_reads_swap, any *_batch call). */
int moni_screen_sizes(moni_ctx_t *ctx, uint64_t *n_reads);
/* The records of the last moni_screen_run on this context: res holds *n_reads of them. */
int moni_screen_fetch(moni_ctx_t *ctx, moni_screen_res_t *res);
/* Host-buffer form: upload, run, fetch.  res: batch->n_reads records (the caller's).  An empty batch gives MONI_OK and writes nothing. */
int moni_screen_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_screen_params_t *prm, moni_screen_res_t *res);

/* ---- exact-match count and locate: what ri::r_index::count / locate_all give the users of ms_pointers (include/ms/moni.hpp: ms_pointers derives
 * from ri::r_index) ---- */
/* A backward search of every pattern of the batch over the BWT the matching-statistics walk reads.  Strand 0 takes the pattern's bytes as they are
 * (no case folding; N matches only an N of the text), strand 1 its reverse complement by the aligner's table (kpbseq.h:120-137).  A byte the BWT does
 * not hold never matches, nor does a byte <= 1 (terminator, separator).  Task t of pattern i on strand s is i * strands + s. */
typedef struct { uint32_t strands;   /* 1: forward only, 2: forward and reverse complement */
                 uint32_t max_occ;   /* positions kept per (pattern, strand); 0 = count only */
                 uint32_t reserved[2]; } moni_locate_params_t;
/* count: occurrences in the concatenation, exact and uncapped (0: none; an empty pattern has none).  sa_lo: the first BWT position of the
 * pattern's interval, defined where count > 0.  matched: pattern bytes consumed while the interval held a position = the length of the longest
 * suffix of the (strand's) pattern that occurs; the pattern's length where it occurs.  n_occ = min(count, max_occ) positions lie at occ_off (defined
 * where n_occ > 0) of pos / seq / seq_off: the text position of the occurrence's first byte (0-based, in the concatenation; no lift-over), the
 * sequence it lies in and the 0-based offset inside it (seqidx::index, seqidx.hpp:149-154) - the suffixes of the n_occ highest ranks of the interval,
 * in decreasing rank order (the order in which phi yields them from the toehold at the interval's upper end). */
typedef struct { uint64_t count, sa_lo, occ_off; uint32_t n_occ, matched; } moni_locate_res_t;
void moni_locate_params_default(moni_locate_params_t *p);            /* strands 1, max_occ 0 */
/* Device-only run over the batch that moni_reads_upload made resident; the results stay in HBM.  MONI_EINVAL: strands outside {1, 2}, a non-zero
 * reserved word, no resident batch.  moni_last_kernel_ms(ctx, 0, ..) then gives count_kernel's time, (ctx, 3, ..) locate_walk_kernel's (with the
 * buffer growth in front of it), (ctx, 6, ..) the whole run's; moni_last_counters: [0] search steps, [1] fast rows fetched, [2] phi steps, [3] steps
 * that took the general path.  Works on an index without LCP samples. */
int  moni_locate_run(moni_ctx_t *ctx, const moni_locate_params_t *prm);
/* What moni_locate_fetch would write: the tasks (patterns x strands) and the positions of the last moni_locate_run (either pointer may be NULL);
 * MONI_EINVAL before any run, and after another batch was made resident (moni_reads_upload, moni_reads_swap, any *_batch call). */
int  moni_locate_sizes(moni_ctx_t *ctx, uint64_t *n_tasks, uint64_t *n_occ);
/* The results of the last moni_locate_run on this context: res holds *n_tasks records, pos / seq / seq_off *n_occ values each (any pointer may be NULL). */
int  moni_locate_fetch(moni_ctx_t *ctx, moni_locate_res_t *res, uint64_t *pos, uint32_t *seq, uint64_t *seq_off);
/* Host-buffer form: upload, run, fetch.  res: batch->n_reads * strands records (the caller's); *pos / *seq / *seq_off are malloc'ed (moni_free; NULL
 * when there is no position), any of the three pointers may be NULL; *n_occ (may be NULL) their length.  An empty batch gives MONI_OK. */
int  moni_locate_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_locate_params_t *prm,
                       moni_locate_res_t *res, uint64_t **pos, uint32_t **seq, uint64_t **seq_off, uint64_t *n_occ);

/* ---- sequence counts: in which sequences of the index a pattern occurs, and how often in each ---- */
/* The search is moni_locate's (strand 0 the bytes as they are, strand 1 the reverse complement, task t = pattern * strands + strand).  Every
 * occurrence is attributed to the sequence its first byte lies in - the seq of moni_locate_res_t's lists, no lift-over - and counted into a dense
 * table of n_tasks rows of n_seq 64-bit counts.  The whole interval is enumerated, in pieces that run in parallel (one per BWT run the interval
 * touches), so the cost does not depend on a cap per pattern; max_walk bounds it instead. */
typedef struct { uint32_t strands;    /* 1: forward only, 2: forward and reverse complement */
                 uint32_t reserved;   /* 0 */
                 uint64_t max_walk;   /* a task with count > max_walk is not enumerated; 0 = no limit */
               } moni_seqcount_params_t;
/* count, sa_lo, matched: as in moni_locate_res_t, exact whether or not the task was walked.  walked: 1 where the interval was enumerated
 * (count <= max_walk, or no limit) - then the task's row sums to count and n_seqs is the number of its non-zero entries; 0 where it was not - then
 * the row is all zero and n_seqs is 0.  n_segs: the pieces the interval was cut into, 0 for a task that was not walked or has no occurrence. */
typedef struct { uint64_t count, sa_lo; uint32_t matched, n_seqs, walked, n_segs; } moni_seqcount_res_t;
void moni_seqcount_params_default(moni_seqcount_params_t *p);        /* strands 1, max_walk 1 << 20 */
/* Device-only run over the batch that moni_reads_upload made resident; the results stay in HBM.  MONI_EINVAL: strands outside {1, 2}, a non-zero
 * reserved, no resident batch; MONI_ENOMEM: the table of n_tasks * n_seq * 8 bytes cannot be had.  moni_last_kernel_ms(ctx, 0, ..) then gives
 * count_kernel's time, (ctx, 3, ..) the walk's with its planning and scan, (ctx, 6, ..) the whole run's; moni_last_counters: [0] search steps,
 * [1] fast rows fetched, [2] phi steps = the sum of count - n_segs over the walked tasks, [3] steps that took the general path.  Works on an index
 * without LCP samples. */
int  moni_seqcount_run(moni_ctx_t *ctx, const moni_seqcount_params_t *prm);
/* The shape of what moni_seqcount_fetch would write (either pointer may be NULL); MONI_EINVAL before any run, and after another batch was made
 * resident (moni_reads_upload, moni_reads_swap, any *_batch call). */
int  moni_seqcount_sizes(moni_ctx_t *ctx, uint64_t *n_tasks, uint32_t *n_seq);
/* The results of the last moni_seqcount_run on this context: res holds n_tasks records, counts n_tasks * n_seq values, one row per task (either
 * pointer may be NULL). */
int  moni_seqcount_fetch(moni_ctx_t *ctx, moni_seqcount_res_t *res, uint64_t *counts);
/* Host-buffer form: upload, run, fetch into the caller's buffers (batch->n_reads * strands records and rows; counts may be NULL).  An empty batch
 * gives MONI_OK. */
int  moni_seqcount_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_seqcount_params_t *prm,
                         moni_seqcount_res_t *res, uint64_t *counts);

/* ---- reference loci: where on the reference a pattern lies, and how many of its occurrences land there ---- */
/* The search is moni_locate's (strand 0 the bytes as they are, strand 1 the reverse complement, task t = pattern * strands + strand).  The whole
 * interval is enumerated, in the pieces the sequence counts use: one per BWT run the interval touches, max_walk bounds a task.  Every occurrence - the text
 * position p of the pattern's first byte - gets a key: with lift = 1 liftidx::lift(p) (liftidx.hpp:89-95), the position on the contig the sequence
 * of p was built from, the value the aligner's records carry; with lift = 0 p itself.  On an index with null lifts (FASTA-built) both are p.  A locus
 * is a distinct key of a task, its support the number of the task's occurrences with that key.  Support can exceed the number of sequences: the
 * bases of an insertion all lift to the reference base the insertion precedes. */
typedef struct { uint32_t strands;      /* 1: forward only, 2: forward and reverse complement */
                 uint32_t lift;         /* 1: keys are lifted positions; 0: text positions (the full locate, in text order) */
                 uint64_t max_walk;     /* a task with count > max_walk is not enumerated; 0 = no limit */
                 uint64_t max_total;    /* bound of the sum of count over the walked tasks of one run; 0 = no limit */
                 uint64_t reserved[2];  /* 0 */
               } moni_loci_params_t;
/* count, sa_lo, matched: as in moni_locate_res_t, exact whether or not the task was walked.  walked, n_segs: as in moni_seqcount_res_t.  A walked
 * task's n_loci loci lie at loci_off of lpos / lseq / lseq_off / support, in ascending lpos order (tasks in task order), and their supports sum to
 * count; a task that was not walked has n_loci = 0. */
typedef struct { uint64_t count, sa_lo, loci_off, n_loci; uint32_t matched, walked, n_segs, reserved; } moni_loci_res_t;
void moni_loci_params_default(moni_loci_params_t *p);                /* strands 1, lift 1, max_walk 1 << 20, max_total 1 << 28 */
/* Device-only run over the batch that moni_reads_upload made resident; the results stay in HBM, in buffers of their own (a locate, seqcount or
 * approx result of the context stays fetchable).  MONI_EINVAL: strands outside {1, 2}, lift > 1, a non-zero reserved word, no resident batch;
 * MONI_ERANGE: more than 2^24 tasks (the task index is sorted beside a 40-bit position in one 64-bit key); MONI_ENOMEM: the walked total exceeds
 * max_total, or the buffers cannot be had - returned before anything is written, the context stays usable (and has no loci result).
 * moni_last_kernel_ms(ctx, 0, ..) then gives count_kernel's time, (ctx, 3, ..) the walk's with its planning and scans, (ctx, 4, ..) the sort's and
 * the fold's, (ctx, 6, ..) the whole run's; moni_last_counters: [0] search steps, [1] fast rows fetched, [2] phi steps = the sum of count - n_segs
 * over the walked tasks, [3] steps that took the general path.  Works on an index without LCP samples. */
int  moni_loci_run(moni_ctx_t *ctx, const moni_loci_params_t *prm);
/* What moni_loci_fetch would write: the tasks and the loci of the last moni_loci_run (either pointer may be NULL); MONI_EINVAL before any run, after
 * a run that failed, and after another batch was made resident (moni_reads_upload, moni_reads_swap, any *_batch call). */
int  moni_loci_sizes(moni_ctx_t *ctx, uint64_t *n_tasks, uint64_t *n_loci);
/* The results of the last moni_loci_run on this context: res holds *n_tasks records, lpos / lseq / lseq_off / support *n_loci values each (any
 * pointer may be NULL).  lseq is the sequence lpos lies in and lseq_off the 0-based offset inside it (seqidx::index). */
int  moni_loci_fetch(moni_ctx_t *ctx, moni_loci_res_t *res, uint64_t *lpos, uint32_t *lseq, uint64_t *lseq_off, uint64_t *support);
/* Host-buffer form: upload, run, fetch.  res: batch->n_reads * strands records (the caller's); *lpos / *lseq / *lseq_off / *support are malloc'ed
 * (moni_free; NULL when there is no locus), any of the four pointers may be NULL; *n_loci (may be NULL) their length.  An empty batch gives MONI_OK. */
int  moni_loci_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_loci_params_t *prm, moni_loci_res_t *res,
                     uint64_t **lpos, uint32_t **lseq, uint64_t **lseq_off, uint64_t **support, uint64_t *n_loci);

/* ---- k-mismatch count and locate: every string within Hamming distance k of a pattern that occurs in the index ---- */
/* Tasks, strands and bytes are moni_locate's (task t = pattern * strands + strand; strand 1 is the reverse complement by the aligner's table).  Only
 * substitutions are searched.  A text window of the pattern's length occurs at distance e where it differs from the pattern at exactly e <= k
 * places and the TEXT byte at every such place is one of upper-case A, C, G, T.  So the pattern's own byte matches itself as in a moni_locate_batch search (N against
 * N; a byte <= 1 or one the BWT does not hold never does, but its place can be paid for as a mismatch), and a window that holds a separator, the
 * terminator or an N where the pattern holds another byte does not occur.  Distinct matching strings have disjoint suffix-array intervals: the
 * counts are counts of text positions, and with k = 0 cnt[0] is moni_locate's count.
 * The search tree of a task is cut into pieces of chunk_len pattern places that run in parallel; max_steps bounds the backward-search steps of ONE
 * piece, so that no batch turns into minutes of kernel time: a task one of whose pieces stopped there has complete = 0 and lower bounds. */
#define MONI_APPROX_MAX_K 3
#define MONI_APPROX_MAX_STEPS_DEFAULT (1ull << 20)
#define MONI_APPROX_CHUNK_LEN_DEFAULT (1u << 30)   /* one piece per task: what the measurement favours */
typedef struct { uint32_t strands;    /* 1: forward only, 2: forward and reverse complement */
                 uint32_t k;          /* mismatches allowed, 0 .. MONI_APPROX_MAX_K */
                 uint32_t max_hits;   /* matching strings (intervals) kept per task; 0 = counts only */
                 uint32_t max_occ;    /* positions kept per kept hit; 0 = none (needs max_hits > 0 otherwise) */
                 uint32_t chunk_len;  /* pattern places per piece, >= 1; >= the pattern's length: one piece per task */
                 uint32_t reserved;   /* 0 */
                 uint64_t max_steps;  /* backward-search steps of one piece; 0 = no limit */
               } moni_approx_params_t;
/* cnt[e]: text positions at distance exactly e (entries above k are 0).  n_hits: distinct matching strings, exact and uncapped; n_kept =
 * min(n_hits, max_hits) of them lie at hit_off of the hit list.  complete: 0 where max_steps stopped a piece of the task - cnt and n_hits are then
 * lower bounds.  matched: as in moni_locate_res_t, the length of the longest suffix of the pattern that occurs exactly. */
typedef struct { uint64_t cnt[4], n_hits, hit_off; uint32_t n_kept, complete, matched, reserved; } moni_approx_res_t;
/* One matching string of a task: its distance, its interval [sa_lo, sa_lo + count - 1], and n_occ = min(count, max_occ) positions at occ_off of
 * pos / seq / seq_off - as moni_locate lists them: the n_occ highest ranks of the interval in decreasing rank order, no lift-over.  The list is
 * grouped by task and sorted by (n_mis, sa_lo) inside a task.  Where n_hits > max_hits, which hits are kept is not specified; each is a true one. */
typedef struct { uint64_t task; uint32_t n_mis, n_occ; uint64_t sa_lo, count, occ_off; } moni_approx_hit_t;
void moni_approx_params_default(moni_approx_params_t *p);   /* strands 1, k 1, max_hits 0, max_occ 0, chunk_len MONI_APPROX_CHUNK_LEN_DEFAULT, max_steps MONI_APPROX_MAX_STEPS_DEFAULT */
/* Device-only run over the batch that moni_reads_upload made resident; the results stay in HBM, in buffers of their own (a locate or seqcount
 * result of the context stays fetchable).  MONI_EINVAL: strands outside {1, 2}, k > 3, chunk_len 0, max_occ > 0 with max_hits 0, a non-zero
 * reserved, no resident batch; MONI_ENOMEM: the hit region of n_tasks * max_hits records cannot be had (nothing is written then).
 * moni_last_kernel_ms(ctx, 0, ..) then gives the exact pass's time, (ctx, 3, ..) the tree pass's with the scans and the compaction of the hits,
 * (ctx, 4, ..) the position walk's, (ctx, 6, ..) the whole run's; moni_last_counters: [0] the steps of the search tree - every attempted
 * (node, letter) step once -, [1] fast rows fetched, [2] phi steps = the sum of n_occ - 1 over the kept hits, [3] steps that took the general
 * path.  Works on an index without LCP samples. */
int  moni_approx_run(moni_ctx_t *ctx, const moni_approx_params_t *prm);
/* What moni_approx_fetch would write (any pointer may be NULL); MONI_EINVAL before any run, and after another batch was made resident. */
int  moni_approx_sizes(moni_ctx_t *ctx, uint64_t *n_tasks, uint64_t *n_hits_kept, uint64_t *n_occ);
/* The results of the last moni_approx_run on this context: res holds *n_tasks records, hits *n_hits_kept, pos / seq / seq_off *n_occ values each
 * (any pointer may be NULL; the three position arrays are taken together, with hits). */
int  moni_approx_fetch(moni_ctx_t *ctx, moni_approx_res_t *res, moni_approx_hit_t *hits, uint64_t *pos, uint32_t *seq, uint64_t *seq_off);
/* Host-buffer form: upload, run, fetch.  res: batch->n_reads * strands records (the caller's); *hits / *pos / *seq / *seq_off are malloc'ed
 * (moni_free; NULL where empty), *n_hits_kept / *n_occ (may be NULL) their lengths.  An empty batch gives MONI_OK. */
int  moni_approx_batch(moni_ctx_t *ctx, const moni_read_batch_t *batch, const moni_approx_params_t *prm, moni_approx_res_t *res,
                       moni_approx_hit_t **hits, uint64_t **pos, uint32_t **seq, uint64_t **seq_off, uint64_t *n_hits_kept, uint64_t *n_occ);

/* ---- BGZF output: the SAM text deflated on the GPU ------------------------------------ */
/* The output is a concatenation of BGZF blocks (SAM specification 4.1): each one gzip member with the `BC` extra subfield and exactly one raw
 * DEFLATE block (BFINAL = 1) of at most block_size bytes of the text - dynamic Huffman over an LZ77 parse that never leaves the block, or
 * stored where that is not smaller (and always at level 0).  The bytes are a function of (text, block_size, level) alone: not of the context,
 * the device, or how the text is cut into calls at multiples of block_size. */
typedef struct { uint32_t block_size;  /* uncompressed bytes per block, 1 .. 65280; default 65280 */
                 uint32_t level;       /* 0 stored blocks, 1 LZ77 + dynamic Huffman; default 1 */
                 uint32_t eof;         /* append the 28-byte end-of-file block; default 0 */
                 uint32_t reserved; } moni_bgzf_params_t;
typedef struct { uint64_t in_bytes, out_bytes, blocks, stored_blocks, matches, literals;
                 double t_kernel, t_total; } moni_bgzf_stats_t;      /* HIP-event seconds of the kernels; host seconds with the transfers */
void moni_bgzf_params_default(moni_bgzf_params_t *p);
/* text: len bytes of host memory (the context's pinned SAM buffer, as moni_align_stream / moni_pe_align_stream / moni_extend_run return it, is
 * the intended caller).  *out points into a pinned buffer of the context: valid until the next moni_bgzf_compress or moni_ctx_destroy on this
 * context, not to be freed.  blocks / out_bytes count the end-of-file block too.  The resident read batch and every result a later *_fetch may
 * want stay as they are.  stats may be NULL.  MONI_EINVAL: a NULL ctx, prm, out or out_len, block_size 0 or above 65280, level above 1, a
 * non-zero reserved, text NULL with len > 0.  len 0 gives MONI_OK and no byte (28 with eof).  MONI_ENOMEM is returned before anything is written. */
int  moni_bgzf_compress(moni_ctx_t *ctx, const void *text, uint64_t len, const moni_bgzf_params_t *prm,
                        const uint8_t **out, uint64_t *out_len, moni_bgzf_stats_t *stats);

/* ---- BAM output: SAM lines encoded as BAM records and deflated on the GPU -------------- */
/* The records of SAM specification 4.2 with the bins of 5.3, made from SAM text (records only: every line ends in \n, has 11 or more
 * tab-separated fields, no @ line) against the dictionary of the header that moni_bam_set_header was given.  The bytes are a function of
 * (header text, record text, block_size, level) alone.  Integer tags take the smallest type (C S I for values from 0, c s i below); tag
 * types other than A, i and Z are not produced by this library and make a bad line. */
typedef struct { uint32_t block_size, level, eof;   /* as in moni_bgzf_params_t: the BAM stream goes through the same blocks */
                 uint32_t raw;                      /* 1: the BAM bytes themselves, no BGZF (block_size, level and eof are still checked; eof is not applied) */
                 uint32_t reserved[2]; } moni_bam_params_t;
typedef struct { uint64_t in_bytes, lines, bam_bytes, out_bytes, blocks, bad_lines, first_bad_line; uint32_t bad_reason, pad;
                 double t_encode, t_deflate, t_total; } moni_bam_stats_t;      /* HIP-event seconds of the encoder's and the deflater's kernels; host seconds of the call */
/* why a line is a bad line (moni_bam_stats_t::bad_reason: the reason of line first_bad_line, the lowest bad index) */
enum { MONI_BAM_OK = 0,
       MONI_BAM_NEWLINE = 1,   /* the text does not end in \n (first_bad_line: the unterminated line; the other lines are not looked at: bad_lines = 1) */
       MONI_BAM_AT = 2,        /* a line that begins with @ */
       MONI_BAM_FIELDS = 3,    /* fewer than 11 fields */
       MONI_BAM_QNAME = 4,     /* an empty QNAME or one of more than 254 bytes */
       MONI_BAM_INT = 5,       /* FLAG, POS, MAPQ, PNEXT or TLEN is not -?[0-9]+ or leaves its range (uint16, [0, 2^31), uint8, [0, 2^31), (-2^31, 2^31)) */
       MONI_BAM_RNAME = 6,     /* RNAME or RNEXT is neither * (= for RNEXT) nor a name of the dictionary */
       MONI_BAM_CIGAR = 7,     /* not * or ([0-9]+[MIDNSHP=X])+, an op length of 2^28 or more, more than 65535 ops */
       MONI_BAM_SEQ = 8,       /* an empty SEQ */
       MONI_BAM_QUAL = 9,      /* QUAL is neither * nor as long as SEQ */
       MONI_BAM_TAG = 10,      /* a tag that is not XX:T:value, or an A tag whose value is not one byte */
       MONI_BAM_TAGINT = 11,   /* an i tag whose value is not -?[0-9]+ within [-2^31, 2^32) */
       MONI_BAM_TAGTYPE = 12,  /* a tag type other than A, i, Z */
       MONI_BAM_LENGTH = 13 }; /* a line of 2^28 bytes or more */
void moni_bam_params_default(moni_bam_params_t *p);
/* Parses the @SQ lines of a SAM header (SN: and LN: of each, in order), keeps the dictionary in the context - on the device too - and returns
 * the uncompressed BAM header (magic, l_text, the text as given, n_ref, the references) in a buffer of the context: valid until the next
 * moni_bam_set_header or moni_ctx_destroy on it.  The caller sends it through moni_bgzf_compress as blocks of its own.  A header may be set
 * again.  MONI_EINVAL: a NULL argument, an @SQ line without SN: or with an LN: outside [1, 2^31), a name of more than 254 bytes, len of 2^31 or more. */
int  moni_bam_set_header(moni_ctx_t *ctx, const char *sam_header, uint64_t len, const uint8_t **bam_header, uint64_t *bam_header_len);
/* sam_lines: len bytes of host memory (the context's pinned SAM buffer is the intended caller).  The records stay on the device between the
 * encoder and the deflater.  *out points into a pinned buffer of the context: valid until the next moni_bam_records, moni_bgzf_compress or
 * moni_ctx_destroy on this context, not to be freed.  Records may straddle blocks.  As with moni_bgzf_compress, the resident read batch,
 * moni_last_kernel_ms, moni_last_counters and every result a later *_fetch may want stay as they are.  stats may be NULL.
 * MONI_EINVAL: a NULL ctx, prm, out or out_len; parameters moni_bgzf_compress refuses, eof or raw above 1, a non-zero reserved; sam_lines NULL
 * with len > 0; no header set on this context; a bad line - then nothing is written (*out_len = 0) and stats, where given, carry bad_lines,
 * first_bad_line (0-based, the minimum over all bad lines) and bad_reason.  len 0 gives MONI_OK and no byte (28 with eof and without raw). */
int  moni_bam_records(moni_ctx_t *ctx, const void *sam_lines, uint64_t len, const moni_bam_params_t *prm,
                      const uint8_t **out, uint64_t *out_len, moni_bam_stats_t *stats);

/* ---- coordinate-sorted, indexed BAM: records sorted on the GPU -------------------------- */
/* The order is samtools sort's: by reference (unplaced records last), by position, forward strand before reverse; ties keep input order.
 * As one key, with n_ref of the header set on the context:
 *     key = (refID < 0 ? n_ref : refID) << 33 | (uint64)(pos + 1) << 1 | (flag >> 4 & 1) */
typedef struct { int32_t ref_id, pos, end;       /* end: pos + the M/D/N/=/X lengths, at least pos + 1 (the reflen rule of the record's bin) */
                 uint32_t bin_flag;              /* bin << 16 | flag, as in the record */
                 uint64_t off; } moni_bam_ent_t; /* where the record begins in the sorted, uncompressed stream of its call */
typedef struct { uint64_t in_bytes, records, bam_bytes, out_bytes, blocks, bad_records, first_bad_record; uint32_t bad_reason, pad;
                 double t_encode,                /* moni_bam_sorted_run: the encoder's kernels (HIP-event seconds, as the next four) */
                        t_key, t_sort, t_gather, t_deflate, t_total; } moni_bam_sort_stats_t;      /* t_total: host seconds of the call */
/* why a record is a bad record (moni_bam_sort_stats_t::bad_reason: of record first_bad_record, the lowest bad index).  The checks run in the order
 * OFFSET, fewer than 36 bytes (SHORT), SIZE, SHORT, NAME, REF, POS, and the first that fails is the record's reason */
enum { MONI_BAMSORT_OK = 0,
       MONI_BAMSORT_OFFSET = 1,  /* offs[i] >= offs[i + 1], or offs[i + 1] > len */
       MONI_BAMSORT_SHORT = 2,   /* fewer bytes than 36 + l_read_name + 4 * n_cigar_op */
       MONI_BAMSORT_SIZE = 3,    /* 4 + block_size is not offs[i + 1] - offs[i] */
       MONI_BAMSORT_NAME = 4,    /* l_read_name 0 */
       MONI_BAMSORT_REF = 5,     /* refID outside [-1, n_ref) */
       MONI_BAMSORT_POS = 6,     /* pos outside [-1, 2^31 - 1) */
       MONI_BAMSORT_LENGTH = 7,  /* offs[n] is not len (first_bad_record: n; the records are not looked at) */
       /* moni_bam_sorted_run_dup alone, on records that passed the checks above (SEQ before CLIP; MATE: of the pair's first record) */
       MONI_BAMSORT_SEQ = 8,     /* fewer bytes than 36 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq */
       MONI_BAMSORT_CLIP = 9,    /* the unclipped 5' end of a mapped, primary record outside [-2^31, 3 * 2^31) */
       MONI_BAMSORT_MATE = 10 }; /* paired: records 2p, 2p + 1 do not carry one name, or one with flag & 1 does not carry 0x40 (2p) / 0x80 (2p + 1) alone,
                                  * or n is odd (then record n - 1).  A record without flag & 1 is not asked for its read's bit. */
/* moni_bam_records with raw = 1, then the records - still on the device - in coordinate order.  *records (*records_len bytes), *keys (n,
 * ascending) and *offs (n + 1: where every record begins, then *records_len) point into pinned buffers of the context that belong to
 * moni_bam_sorted_run and moni_bam_sort alone: valid until the next of those two or moni_ctx_destroy on this context.  Everything else is as
 * for moni_bam_records: the bad-line rules (stats->bad_records, first_bad_record and bad_reason then carry the line's MONI_BAM_* figures),
 * the header, and what stays undisturbed.  len 0 gives *n 0.  stats may be NULL. */
int  moni_bam_sorted_run(moni_ctx_t *ctx, const void *sam_lines, uint64_t len, const uint8_t **records, uint64_t *records_len,
                         const uint64_t **keys, const uint64_t **offs, uint64_t *n, moni_bam_sort_stats_t *stats);
/* records: len bytes of host memory, n raw BAM records in any order, record i at offs[i] .. offs[i + 1] (offs: n + 1 entries).  They are
 * sorted stably by key on the device and leave through the BGZF blocks of prm (*out as for moni_bam_records) or, with raw, as they are
 * (*out then is the pinned buffer of moni_bam_sorted_run's records).  *ents: n entries in sorted order, pinned, valid as *records above.
 * MONI_EINVAL: a NULL argument but stats (records and offs may be NULL with n 0 and len 0), parameters moni_bam_records refuses, no header
 * set, offs[n] != len, n of 2^32 or more, a bad record - then nothing is written (*out_len = 0) and stats, where given, carry bad_records,
 * first_bad_record and bad_reason. */
int  moni_bam_sort(moni_ctx_t *ctx, const void *records, uint64_t len, const uint64_t *offs, uint64_t n, const moni_bam_params_t *prm,
                   const uint8_t **out, uint64_t *out_len, const moni_bam_ent_t **ents, moni_bam_sort_stats_t *stats);

/* ---- duplicate marking of the sorted output ---------------------------------------------- */
/* Picard's rule without optical duplicates or UMIs.  A record takes part if flag & 0x904 == 0.  Its unclipped 5' end u5 is pos minus the
 * leading S/H lengths (forward) or pos + reflen - 1 plus the trailing S/H lengths (reverse); its end code is
 *     e = (refID < 0 ? n_ref : refID) << 34 | (uint64)(u5 + 2^31) << 1 | (flag >> 4 & 1)
 * and its score the sum of its base qualities of 15 and more (a byte of 0xFF counts 0; the sum saturates at 2^31 - 1).
 * An entry is a pair (both mates take part and carry flag & 1: k1 <= k2 their end codes; kind 1, or 3 when the strands are equal and the
 * mate with the smaller code - at a tie read 1 - is read 2; score: the sum of the two) or a fragment (k1 = e, k2 = 0, kind 0).
 * idx: the records' places in the sorted run, idx[1] = 0xFFFFFFFF for a fragment. */
typedef struct { uint64_t k1, k2; uint32_t score, kind; uint32_t idx[2]; } moni_bam_dup_t;
typedef struct { moni_bam_sort_stats_t run;      /* as moni_bam_sorted_run fills it; the bad-record fields also carry SEQ, CLIP and MATE */
                 uint64_t entries, pairs, fragments;
                 uint32_t bad_is_record, pad;    /* 1: run's bad_* fields speak of a record (MONI_BAMSORT_*, input order), not of a line (MONI_BAM_*) */
                 double t_sig, t_entry; } moni_bam_run_dup_stats_t;    /* HIP-event seconds: the signature kernel; the unit, scan and entry passes */
typedef struct { uint64_t entries, pairs, dup_pairs, fragments, dup_fragments, marked_records, bad_entries, first_bad_entry;
                 double t_sort, t_flag, t_total; } moni_bam_dup_stats_t;   /* the sort passes, the other kernels (HIP-event seconds); host seconds */
/* moni_bam_sorted_run, byte for byte, and the run's entries in input order: with paired = 1 records 2p and 2p + 1 of the lines are the two
 * mates of a pair, with paired = 0 every record stands alone.  *dups (*n_dups entries) is a pinned buffer of the context, valid as *records.
 * MONI_EINVAL in addition: a NULL dups, n_dups; paired above 1; a bad record by MONI_BAMSORT_SEQ, CLIP or MATE - then nothing is written
 * (*n = *n_dups = 0) and stats->run carries bad_records, first_bad_record (in input order) and bad_reason. */
int  moni_bam_sorted_run_dup(moni_ctx_t *ctx, const void *sam_lines, uint64_t len, uint32_t paired, const uint8_t **records, uint64_t *records_len,
                             const uint64_t **keys, const uint64_t **offs, uint64_t *n, const moni_bam_dup_t **dups, uint64_t *n_dups,
                             moni_bam_run_dup_stats_t *stats);
/* The entries of all runs, in run order (that is input order): dups[r][0, n_dups[r]) of a run of n_records[r] records.  Pairs with equal
 * (k1, k2, kind): the highest score stays, at a tie the earliest; the records of the others are duplicates.  Fragments whose e is an end of a
 * pair are duplicates; among the fragments of an e without one the best stays.  marks[r][0, n_records[r]) - the caller's - is written whole:
 * 1 for a duplicate, else 0, by the record's place in its sorted run.  The entries must be of the header set on this context.
 * MONI_EINVAL: a NULL argument but stats (the arrays may be NULL with n_runs 0), no header set, an idx at or above n_records[r] (but a
 * fragment's idx[1]), a kind other than 0, 1, 3 - then no mark is written and stats carry bad_entries and first_bad_entry (counted over all
 * runs).  MONI_ERANGE: 2^31 entries or 2^32 - 1 records and more. */
int  moni_bam_dup_resolve(moni_ctx_t *ctx, const moni_bam_dup_t *const *dups, const uint64_t *n_dups, const uint64_t *n_records, uint64_t n_runs,
                          uint8_t *const *marks, moni_bam_dup_stats_t *stats);
/* moni_bam_sort with marks[n] beside the input records: record i with marks[i] != 0 gets flag |= 0x400 on the device, before its key and
 * its entry are made.  marks NULL: moni_bam_sort. */
int  moni_bam_sort_marked(moni_ctx_t *ctx, const void *records, uint64_t len, const uint64_t *offs, uint64_t n, const uint8_t *marks,
                          const moni_bam_params_t *prm, const uint8_t **out, uint64_t *out_len, const moni_bam_ent_t **ents, moni_bam_sort_stats_t *stats);

/* Host only, no context, no GPU.  Runs r = 0 .. n_runs - 1, each sorted by key: keys[r][0, n[r]) ascending, offs[r][0, n[r]] the records'
 * offsets in the run.  The merged order - by (key, run, index) - is cut into chunks of at most chunk_bytes (a record larger than that is a
 * chunk of its own); a chunk is one contiguous slice of every run, and its slices, concatenated in run order and sorted stably by key, are
 * that part of the merged order.  Chunk k takes records cuts[k * n_runs + r] .. cuts[(k + 1) * n_runs + r] of run r. */
typedef struct { uint64_t n_chunks, n_runs; uint64_t *cuts; /* (n_chunks + 1) * n_runs */ } moni_bam_plan_t;
int  moni_bam_merge_plan(const uint64_t *const *keys, const uint64_t *n, const uint64_t *const *offs, uint64_t n_runs, uint64_t chunk_bytes,
                         moni_bam_plan_t **plan);
void moni_bam_plan_free(moni_bam_plan_t *plan);
/* Host only: the .bai index (SAM specification 5.2) of a coordinate-sorted BAM written as chunks of BGZF blocks.  moni_bai_add takes the
 * chunks in file order: ents[n] as moni_bam_sort gave them, the chunk's uncompressed bytes, the block_size it was deflated with, the
 * compressed size of each of its n_blocks blocks and the file offset of the first.  The chunks follow one another in the file; eof_off
 * (where the end-of-file block begins) must be where the last one ended.  *bytes: the index, in the builder until moni_bai_destroy.
 * MONI_EINVAL: records out of order, a ref_id outside [-1, n_ref), offsets or blocks that do not fit chunk_len, a gap between chunks. */
typedef struct moni_bai moni_bai_t;
moni_bai_t *moni_bai_create(uint32_t n_ref);
int  moni_bai_add(moni_bai_t *b, const moni_bam_ent_t *ents, uint64_t n, uint64_t chunk_len, uint32_t block_size, const uint32_t *csizes,
                  uint64_t n_blocks, uint64_t file_off);
int  moni_bai_finish(moni_bai_t *b, uint64_t eof_off, const uint8_t **bytes, uint64_t *len);
void moni_bai_destroy(moni_bai_t *b);

/* ---- depth of coverage of the sorted output ---------------------------------------------- */
/* The references r = 0 .. n_ref - 1 of the header set on the context, of lengths LN_r.  Reference r owns LN_r + 1 slots of one int32 array,
 * from base_r = sum over q < r of (LN_q + 1); the last slot of a reference takes the -1 of a block that ends at LN_r and is never a base.
 * A record counts iff refID >= 0, pos >= 0, n_cigar_op > 0, flag & exclude_flags == 0 and mapq >= min_mapq; one that fails several of
 * these is counted once, as unplaced (the first three) before skipped_flag before skipped_mapq.  The CIGAR is walked from p = pos: M = X D
 * cover [p, p + len) and advance p, N advances p, I S H P do nothing; adjacent covering operations are one block.  A block [b, e) is
 * clipped to e = min(e, LN_r) and dropped if b >= LN_r (the record then counts in `clipped`, once); it adds +1 at slot base_r + b and -1 at
 * base_r + e, and counts in `blocks`.  The depth at base x of r is the sum of the slots base_r .. base_r + x.  No mate-overlap correction:
 * mosdepth's --fast-mode with deletions counted.  The depth is an int32 because an object counts fewer than 2^31 records in all. */
typedef struct moni_cov moni_cov_t;
typedef struct { uint32_t exclude_flags, min_mapq, reserved[2]; } moni_cov_params_t;      /* defaults: 0x704 (mosdepth's 1796), 0 */
typedef struct { uint64_t records, counted, skipped_flag, skipped_mapq, unplaced, clipped, blocks,
                 bad_records, first_bad_record; uint32_t bad_reason, pad;      /* as moni_bam_sort_stats_t has them (MONI_BAMSORT_OFFSET .. LENGTH) */
                 double t_add, t_total; } moni_cov_stats_t;      /* the call's kernels (HIP-event seconds); host seconds of the call */
typedef struct { uint64_t length, bases; uint32_t min, max; } moni_cov_ref_t;      /* bases: the sum of the depth over [0, length) */
void moni_cov_params_default(moni_cov_params_t *p);
/* An object for the dictionary of the header set on ctx, its slots zeroed on ctx's device and owned by the object (4 bytes a slot).  It may be
 * added to from any context of that device whose header has the same dictionary, from several host threads at once: the adds are
 * device-scope integer atomics, so the result is exact and independent of their order.  Seal, next, windows and destroy are for one thread,
 * after the adds have returned.  MONI_EINVAL: a NULL argument, no header set, a non-zero reserved word. */
int  moni_cov_create(moni_ctx_t *ctx, const moni_cov_params_t *prm, moni_cov_t **cov);
void moni_cov_destroy(moni_cov_t *cov);
/* records, len, offs, n: raw BAM records in host memory as moni_bam_sort takes them, with its checks and reasons; a bad record adds nothing
 * of the call (MONI_EINVAL, stats carry bad_records, first_bad_record, bad_reason).  MONI_ERANGE, with nothing added, once the object's
 * counted records would reach 2^31.  MONI_EINVAL too: a sealed object, a context of another device or of another number of references.
 * Both adds leave undisturbed what moni_bam_records leaves undisturbed, and the results of the sort calls.  stats may be NULL. */
int  moni_cov_add(moni_ctx_t *ctx, moni_cov_t *cov, const void *records, uint64_t len, const uint64_t *offs, uint64_t n, moni_cov_stats_t *stats);
/* The records that the context's last successful moni_bam_sort, moni_bam_sort_marked, moni_bam_sorted_run or moni_bam_sorted_run_dup left on
 * the device, in coordinate order and with the 0x400 bits of moni_bam_sort_marked set: no second upload.  The result is that of moni_cov_add on
 * the raw bytes those calls return.  MONI_EINVAL if no such call has succeeded on ctx. */
int  moni_cov_add_sorted(moni_ctx_t *ctx, moni_cov_t *cov, moni_cov_stats_t *stats);
/* The slots become depths (one scan in place; every reference's slots sum to zero, so the scan needs no restart), and *refs (*n_ref entries,
 * valid until moni_cov_destroy) the figures of every reference.  After a seal the adds return MONI_EINVAL; a second seal gives the same refs. */
int  moni_cov_seal(moni_ctx_t *ctx, moni_cov_t *cov, const moni_cov_ref_t **refs, uint32_t *n_ref);
/* An iterator over the per-base text in genome order: for every reference the maximal runs of equal depth over [0, LN_r), zero included, one
 * line `name\tstart\tend\tdepth\n` a run (0-based, half-open; mosdepth's per-base.bed).  A call looks at no more than max_bases slots and
 * writes no more than max_lines lines (both at least 1); lines are whole, and a run that reaches past what a call looked at is written by the
 * call that sees its end.  *text (*len bytes, possibly 0) is a pinned buffer of ctx, valid until ctx's next moni_cov_next or its destroy;
 * *done = 1 with the last piece.  The pieces of all calls, one behind the other, are the same bytes for every max_bases and max_lines.
 * MONI_EINVAL: a NULL argument, an object that is not sealed, max_bases or max_lines 0. */
int  moni_cov_next(moni_ctx_t *ctx, moni_cov_t *cov, uint64_t max_bases, uint64_t max_lines, const char **text, uint64_t *len, int *done);
/* *sums (*n = ceil(LN_r / window) entries, a pinned buffer of ctx valid until ctx's next moni_cov_windows or its destroy): the sum of the
 * depth over [k * window, min((k + 1) * window, LN_r)).  MONI_EINVAL: not sealed, ref_id >= n_ref, window outside [1, 2^31). */
int  moni_cov_windows(moni_ctx_t *ctx, moni_cov_t *cov, uint32_t ref_id, uint32_t window, const uint64_t **sums, uint64_t *n);
/* For the tests alone: the object's count of counted records becomes `counted`, so that the 2^31 bound is reached without 2^31 records. */
void moni_cov_test_set_counted(moni_cov_t *cov, uint64_t counted);

/* ---- BGZF input: blocked gzip inflated on the GPU --------------------------------------- */
/* Input is a concatenation of BGZF members (SAM specification 4.1: what bgzip, unaligned BAM and moni_bgzf_compress write): gzip members
 * with the `BC` extra subfield - anywhere in the extra field -, each at most 64 KB and inflating to at most 64 KB, with any number of
 * DEFLATE blocks of any BTYPE (RFC 1951 whole).  Members are independent; one wavefront inflates one. */
typedef struct { uint32_t check_crc;          /* verify CRC-32 of every member; default 1 */
                 uint32_t reserved[3]; } moni_inflate_params_t;
typedef struct { uint64_t in_bytes, out_bytes, blocks, bad_blocks, first_bad_block;
                 uint32_t bad_reason, pad;
                 uint64_t stored, fixed, dynamic;      /* DEFLATE blocks seen, by BTYPE */
                 double t_kernel, t_total; } moni_inflate_stats_t;      /* HIP-event seconds of the kernel; host seconds with the transfers */
/* why a member is bad (moni_inflate_stats_t::bad_reason: of member first_bad_block, the lowest bad index): the first failure in the order
 * a sequential reader of that member meets them */
enum { MONI_INF_OK = 0,
       MONI_INF_HEADER,        /* not a BGZF member: ID1 ID2 CM FLG, no BC subfield, a BSIZE that leaves no room for header and trailer */
       MONI_INF_BTYPE,         /* BTYPE 11 */
       MONI_INF_STORED_LEN,    /* LEN and NLEN of a stored block disagree */
       MONI_INF_CODE_LENGTHS,  /* more than 286 / 30 codes, an over-subscribed or incomplete set of lengths (but no distance code at all, or one code
                                  of length 1), a repeat with nothing before it or past the last length, no end-of-block code */
       MONI_INF_BAD_SYMBOL,    /* bits that are no code, literal/length symbol 286 / 287, distance symbol 30 / 31 */
       MONI_INF_DISTANCE,      /* a match reaches before the member's first byte */
       MONI_INF_OVERRUN,       /* more output than ISIZE (or than 65536 bytes) */
       MONI_INF_TRUNCATED,     /* the payload ends inside a block; as a header reason: len ends inside a member */
       MONI_INF_TRAILING,      /* whole bytes between the last block and the trailer */
       MONI_INF_ISIZE,         /* fewer bytes than ISIZE */
       MONI_INF_CRC };
void moni_inflate_params_default(moni_inflate_params_t *p);
/* Host only: hops over the members of data[0, len) by BSIZE.  *n_blocks members lie wholly within len and take *used bytes (what is left
 * is the start of a member: carry it over to the next chunk); *out_bytes is the sum of their ISIZE.  Any of the three may be NULL.
 * MONI_EINVAL: data NULL with len > 0, or a member that is not BGZF - the three then describe the members before it. */
int  moni_bgzf_scan(const void *data, uint64_t len, uint64_t *n_blocks, uint64_t *used, uint64_t *out_bytes);
/* blocks: len bytes of host memory, whole members only (len = *used of moni_bgzf_scan).  *out points into a pinned buffer of the context
 * that belongs to this call alone: valid until the next moni_bgzf_inflate or moni_ctx_destroy on this context, not to be freed; a pointer
 * moni_bgzf_compress or moni_bam_records returned stays valid.  The resident read batch, moni_last_kernel_ms, moni_last_counters and
 * every result a later *_fetch may want stay as they are.  ISIZE may be 0 (the end-of-file block) and up to 65536.  stats may be NULL.
 * MONI_EINVAL: a NULL ctx, prm, out or out_len; check_crc above 1, a non-zero reserved; blocks NULL with len > 0; a bad member - then
 * *out_len = 0 and stats, where given, carry bad_blocks, first_bad_block (0-based, the lowest) and bad_reason.  len 0 gives MONI_OK, no
 * byte, and launches nothing. */
int  moni_bgzf_inflate(moni_ctx_t *ctx, const void *blocks, uint64_t len, const moni_inflate_params_t *prm,
                       const uint8_t **out, uint64_t *out_len, moni_inflate_stats_t *stats);

/* ---- BAM input: the reads of unaligned or aligned BAM as FASTQ text, made on the GPU ---- */
/* A BAM file is BGZF members whose text is the header (`BAM\1`, l_text, the text, n_ref, the references) and then records, each behind
 * its own block_size, aligned to nothing.  A context holds one stream: the header's state and the bytes that no call has used yet (the
 * carry: a header, a record or a pair that is not whole).  moni_bam_in_feed inflates the members it is given behind the carry, finds
 * every record start on the device, and writes the primary records that have bases as four-line FASTQ: @name, the bases (= as N), +,
 * the qualities + 33 (`"` for every base where they are absent: a first byte of 0xFF).  A record with 0x10 is given as sequenced: the
 * bases reversed and complemented, the qualities reversed.  CIGAR and tags are dropped.  Records with 0x100 or 0x800 and records
 * without bases are skipped and counted.  paired: the records kept come as a first mate (0x1 | 0x40) followed by its second
 * (0x1 | 0x80) under the same name - what unaligned BAM and `samtools collate` give; the first mates go to text1, the second to text2. */
typedef struct { uint32_t paired;             /* default 0 */
                 uint32_t check_crc;          /* verify CRC-32 of every member; default 1 */
                 uint32_t reserved[2]; } moni_bamin_params_t;
typedef struct { moni_inflate_stats_t inflate;          /* of the members of this call, as moni_bgzf_inflate gives them (its bad_blocks, first_bad_block, bad_reason) */
                 uint64_t records, reads;               /* records seen by this call (those carried on are not); reads written (paired: both mates) */
                 uint64_t skipped_secondary, skipped_empty;
                 uint64_t carried_bytes;                /* of the stream, left for the next call */
                 uint64_t bad_records;                  /* 1 where a record (or the header) was refused: what lies behind it is not looked at */
                 uint64_t first_bad_record;             /* its index among the records since the last reset, the lowest */
                 uint32_t bad_record_reason, header_done;
                 double t_kernel[4];                    /* HIP-event seconds: inflation; sweep, chain and list; selection and scans; text */
                 double t_total; } moni_bamin_stats_t;
enum { MONI_BAMIN_OK = 0,
       MONI_BAMIN_MAGIC,       /* the stream does not start with BAM\1 */
       MONI_BAMIN_HEADER,      /* a negative l_text or n_ref, a reference name of length 0 or less */
       MONI_BAMIN_BLOCK_SIZE,  /* outside [32, 2^28] */
       MONI_BAMIN_FIELDS,      /* l_read_name 0, a name that does not end in NUL, a negative l_seq, fields that do not fit block_size */
       MONI_BAMIN_PAIRING,     /* paired: a kept record without 0x1, not the mate (0x40 / 0x80) its turn asks for, or a second mate under another name */
       MONI_BAMIN_TRUNCATED }; /* last was set and bytes are left over: a header or a record that is not whole, a lone first mate */
void moni_bamin_params_default(moni_bamin_params_t *p);
/* Forgets the header's state, the carry and the record count: the next feed starts a file. */
int  moni_bam_in_reset(moni_ctx_t *ctx);
/* blocks: len bytes of host memory, whole BGZF members only (as for moni_bgzf_inflate); last: nothing follows.  *text1 / *len1 (and,
 * paired, *text2 / *len2 - else NULL and 0) point into pinned buffers of the context that belong to this call alone: valid until the
 * next moni_bam_in_feed, moni_bam_in_reset or moni_ctx_destroy on this context.  *n_reads: records in text1 (paired: pairs).  A header
 * may span any number of calls.  len 0 with last 0 launches nothing.  What the other calls of the context hold - the resident batch,
 * moni_last_kernel_ms, moni_last_counters, pending *_fetch results, the pointers moni_bgzf_compress, moni_bam_records, moni_bgzf_inflate
 * and the sort calls returned - stays as it is.  stats may be NULL.
 * MONI_EINVAL: a NULL argument but stats (blocks may be NULL with len 0); paired, check_crc or last above 1, a non-zero reserved; a bad
 * member (stats->inflate says which); a bad record (stats->first_bad_record, bad_record_reason).  Then nothing is written, both lengths
 * are 0, and the stream is left as it was before the call.  MONI_ERANGE: carry and text together reach 2^32 bytes. */
int  moni_bam_in_feed(moni_ctx_t *ctx, const void *blocks, uint64_t len, const moni_bamin_params_t *prm, int last,
                      const uint8_t **text1, uint64_t *len1, const uint8_t **text2, uint64_t *len2, uint64_t *n_reads, moni_bamin_stats_t *stats);

/* ---- the reference's on-disk liftidx (<prefix>.ldx: include/aligner/liftidx.hpp:117-143 over include/common/seqidx.hpp:197-238) ---- */
/* Both layouts load: the current one (u64 w after u) and the older one the reference's fixture data/Chr21.10.ldx has. */
int moni_ldx_info(const char *path, uint64_t *n_seq, uint64_t *u, uint64_t *w, int *has_w);
/* Load and write again (with_w: current layout).  Writing is sdsl-exact: the fixture round-trips byte for byte. */
int moni_ldx_rewrite(const char *in_path, const char *out_path, int with_w);
/* liftidx::serialize of a flat index's sequences and lifts (null lifts, liftidx.hpp:150-157, when idx carries none). */
int moni_ldx_write(const moni_flat_index_t *idx, const char *path, int with_w);
/* liftidx::lift (liftidx.hpp:89-95) of n text positions with the lifts of an .ldx file, on the GPU (lift_core.h tables). */
int moni_ldx_lift_batch(const char *path, int device, const uint64_t *pos, uint64_t n, uint64_t *out);

/* ---- the reference's on-disk r-index (<prefix>.thrbv.full.lcp.ms: moni_lcp::serialize / load, include/aligner/moni_lcp.hpp:178-225) ---- */
/* Layout of the absent r-index / sdsl pieces restated from recall (UNPINNED: the reference tree holds no such file); the reader takes a
 * file only if it parses to its last byte AND every redundancy in it agrees (moni_align_amd/csrc/ms_index_io.hpp).  Host-only calls. */
int moni_ms_file_info(const char *path, uint64_t *n, uint64_t *r);
/* Arrays for r runs (from moni_ms_file_info): F[256], heads[r], starts[r+1], ssa[r], esa[r], thr[r] (0 = none), slcp[r].  On
 * MONI_EIO err (if given) says which part of the file disagreed. */
int moni_ms_file_read(const char *path, uint64_t r, uint64_t *F, uint8_t *heads, uint64_t *starts, uint64_t *ssa, uint64_t *esa,
                      uint64_t *thr, uint64_t *slcp, char *err, uint64_t err_cap);
/* moni_lcp::serialize of a flat index (only n, r, F, heads, starts, ssa, esa, thr, slcp are read). */
int moni_ms_file_write(const moni_flat_index_t *idx, const char *path);
/* What aligner's constructor loads (seed_finder.hpp:66-124): <prefix>.thrbv.full.lcp.ms + <prefix>.ldx + the text.  text_path: plain
 * bytes (n - 1 of them, what PlainSlp::expandSubstr would return), or NULL - the output of `moni build` as it is: the .plain.slp grammar
 * (ShapedSlp, an absent submodule) is not read, the text is rebuilt from the BWT on the GPU instead (see moni_index_create). */
int moni_index_load_reference(const char *ms_path, const char *ldx_path, const char *text_path, int device, moni_index_t **out);

/* ---- measurement -------------------------------------------------------------------------- */
/* HIP-event time (ms) of the kernels of the last *_run on this ctx's stream.
 * which: 0 ms_lf, 1 mem_count, 2 mem_emit, 3 phi_count, 4 phi_emit, 5 extz, 6 whole run. */
int moni_last_kernel_ms(moni_ctx_t *ctx, int which, float *ms);
/* Work counters of the last moni_seed_run: out[0] LF steps, [1] threshold jumps, [2] phi steps,
 * [3] text bytes compared (the S, J, P, C of SURVEY.md §8(d)). */
int moni_last_counters(moni_ctx_t *ctx, uint64_t out[4]);
/* The occurrence stage of the last moni_seed_run: out[0] seeds whose list is longer than the in-place cap (16) and lies in the overflow
 * region, [1] overflow entries they take, [2] entries the region holds, [3] count passes run (more than one: the counter pool or the
 * overflow region was grown and the pass repeated), [4] launches of the long-seed kernel (0: skipped, there was no long seed),
 * [5] compactions done for moni_seed_fetch since that run (the align paths do none). */
int moni_seed_occ_stats(moni_ctx_t *ctx, uint64_t out[6]);
/* The strand prefilter of the seeding stage (csrc/prefilter_core.h): a task - one strand of one read - none of whose windows of min_len bases
 * has all of its k-mers in the index's k-mer table can hold no MEM, and its LF walk and text comparison are left out.  mode 0: off;
 * 1 (default): on in the align, paired, report-MEMs and csv entry points, off in moni_seed_run / moni_seed_batch; 2: on everywhere.
 * MONI_SEED_PREFILTER=0|1|2 sets the mode of a new context.  The seeds are the same in every mode.  Where the filter runs, moni_last_counters
 * counts the work done: [0] the steps walked, [1] the jumps taken and [3] the bytes compared, of the tasks that were not skipped.  The filter stands
 * down by itself for a task whose pattern holds a byte outside A / C / G / T, when min_len is below the table's k, and for an index whose
 * table is more than a quarter full.  The matching-statistics entry points and extend mode never filter: their pointers are complete. */
int moni_seed_prefilter(moni_ctx_t *ctx, int mode);
/* The filter in the last seeding run: out[0] tasks, [1] tasks skipped, [2] table lookups, [3] the table's density x 1e6. */
int moni_seed_prefilter_stats(moni_ctx_t *ctx, uint64_t out[4]);
/* The leaping walk of the seeding stage (csrc/seed_core.h: ms_task_events_leap): behind 8 matched steps in a row the walk compares the read with
 * the text and crosses the rest of the matched stretch in one move, re-entering through a sampled inverse suffix array that every index
 * carries (one entry per `stride` text positions, built on the device when the index is created; MONI_MS_LEAP_STRIDE=8|16|32).  The seeds and
 * moni_last_counters are the same with and without it: [0] there counts the reference walk's steps, not the rows fetched.  MONI_MS_LEAP=0 at
 * index creation leaves the tables out, in a new context it leaves them unused.  Of the last seeding run: out[0] leaps, [1] steps leapt,
 * [2] comparisons started, [3] the table's stride (0: the index has no table). */
int moni_ms_leap_stats(moni_ctx_t *ctx, uint64_t out[4]);
/* The table itself (tests): *n_entries entries, isa[i] = run | off << 32 of ISA[i * stride] and clean[i] = the number of text bytes from
 * i * stride on that are A / C / G / T, at most 255; *build_ms the time its build took on the device.  Any pointer may be NULL; cap: the
 * entries isa and clean have room for (MONI_EINVAL if fewer than *n_entries). */
int moni_index_leap_table(const moni_index_t *index, uint64_t *isa, uint8_t *clean, uint64_t cap, uint64_t *n_entries, uint32_t *stride, float *build_ms);
const char *moni_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MONI_HIP_H */
