// Paired-end entry points (inside extern "C" of moni_hip.hip).  The batch holds the pairs interleaved: reads 2p and 2p + 1 are the
// mates of pair p (what kpbseq_t's two kbseq_t hold side by side, include/common/kpbseq.h:300-326).
//   moni_pe_learn_batch          aligner::learn_fragment_model (aligner_ksw2.hpp:816-885) over one batch
//   moni_pe_align_batch / _stream / _run   aligner::align(kpbseq_t*, ...) (aligner_ksw2.hpp:888-918), orphan recovery included
//   moni_pe_report_mems_batch    the same call with report_mems (-m)
// All run the seeding kernels over the 2 N reads, then the paired kernels (pe_fast.hip, pe_kernel.hip, pe_lines.hip).

#define PE_PEN_TAB 8192u
#define PE_K1_DIRS 65536u        // direction bytes per wave of the orphan scoring pass (gap fills between anchors: up to ~180 x 180)
struct PeChunk { uint64_t lo = 0, n = 0; std::vector<pe_rec_t> recs; std::vector<uint32_t> cig; std::vector<moni_alt_t> alt; };

// Upload, seed, then the paired kernels over chunks of pairs.  The staged kernels of ALL chunks are queued up front on the context's stream (one
// set of their large buffers: they run one after the other); every chunk owns its records, pools, counters and hand-over list, and its hand-over
// launches (pe_orphan_kernel: park, score the chains in parts, replay), its lines (pe_lines_kernel) and their gather follow on one of PE_NSTREAM
// streams, beside the staged kernels of the later chunks.  The host takes the chunks in order: a summary in pinned memory, then one queued
// transfer of the chunk's block into the pinned text buffer; `consume` - the host finishing - only for a chunk the kernels could not finish.
// moni_pe_align_*: the two lines of every pair are written on the GPU (pe_lines.hip), put in input order there and arrive by one transfer per chunk in
// the context's pinned text buffer; the host finishes a chunk itself (consume) only when one of its pairs does not fit the kernel's staging
struct PeText {
    const uint8_t* names; const uint64_t* name_off; const uint8_t* quals;
    std::function<char*(size_t)> room;      // the text buffer with room for that many bytes in all (what is in it stays)
    size_t* used;                           // bytes of text so far
    uint64_t aligned = 0, chunks_gpu = 0, chunks_host = 0, pairs_upto = 0;      // pairs_upto: the pairs the text holds once the current request is filled
};

// pe_orphan_kernel's replay trusts a chain's record by its tag: one counter for the whole process (contexts recycle each other's device memory), and the record
// array is cleared whenever it is (re)allocated
static std::atomic<uint32_t> pe_launch_tag{0};

// `-c` for pairs: the two numbers of a pair's line that only the state machine knows (pe_core.h: PE_CSV_COUNT), per pair of the batch.  Asking for them sends
// every pair through the host's state machine (pe_big.cpp), as `-c` does with the reads of the single-end path: a diagnostics mode.
struct PeCsvCounts { std::vector<uint64_t> filter, skipped; };

static int pe_run(moni_ctx* c, const moni_read_batch_t* b, const moni_align_params_t* prm, const moni_pe_params_t* pe, bool finalize, double mean, double std_dev,
                  const std::function<int(const PeChunk&)>& consume, moni_align_stats_t* stats, PeText* txt = nullptr, bool resident = false, PeCsvCounts* csvq = nullptr) {
    moni_index* I = c->idx;
    HIPCHK(hipSetDevice(I->device));
    if (prm->w >= 0 || prm->zdrop >= 0) return MONI_EINVAL;
    if (b->n_reads & 1) return MONI_EINVAL;
    const uint64_t NP = b->n_reads / 2;
    if (!NP) return MONI_OK;
    int rc;
    const double t0 = mh::now_s();
    moni_seed_params_t sp;
    sp.min_len = prm->min_len; sp.filter_seeds = prm->filter_seeds; sp.n_seeds_thr = prm->n_seeds_thr; sp.report_mems = 0;
    if (txt && getenv("MONI_PE_HOST_FORMAT")) txt = nullptr;          // (the host finishing for every chunk: what the kernel's lines are checked against)
    uint64_t force_big = 0;            // test hook: every n-th pair is treated as beyond the kernel's capacities
    if (const char* v = getenv("MONI_PE_FORCE_BIG")) { const long long x = atoll(v); if (x > 0) force_big = (uint64_t)x; }
    if (csvq) { force_big = 1; csvq->filter.assign(NP, 0); csvq->skipped.assign(NP, 0); }
    if (force_big) txt = nullptr;      // (the hook acts on the records the host fetches; decided before the uploader thread is started: `txt` does not change after this line)
    // read names and qualities go to the device while the seeding runs
    std::thread uploader;
    int rc_up = MONI_OK;
    if (txt) {
        const uint64_t NR = b->n_reads;
        const uint64_t nb_names = txt->name_off[NR] - txt->name_off[0], nb_q = txt->quals ? b->offsets[NR] - b->offsets[0] : 0;
        if ((rc = c->ak_rnames.ensure(nb_names + 16)) || (rc = c->ak_rname_off.ensure(NR + 1)) || (rc = c->ak_quals.ensure(nb_q + 16))) return rc;
        if (!c->copy_stream) HIPCHK(hipStreamCreateWithFlags(&c->copy_stream.h, hipStreamNonBlocking));
        const PeText* const txt_up = txt;          // (by value: the thread never reads the caller's variable)
        uploader = std::thread([&, NR, nb_names, nb_q, txt_up]() {
            const PeText* const txt = txt_up;
            if (hipSetDevice(I->device) != hipSuccess) { rc_up = MONI_ENODEV; return; }
            std::vector<uint64_t> rel(NR + 1);
            for (uint64_t r = 0; r <= NR; ++r) rel[r] = txt->name_off[r] - txt->name_off[0];
            if (hipMemcpyAsync(c->ak_rnames.p, txt->names + txt->name_off[0], nb_names, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess ||
                hipMemcpyAsync(c->ak_rname_off.p, rel.data(), (NR + 1) * 8, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess ||
                (nb_q && hipMemcpyAsync(c->ak_quals.p, txt->quals + b->offsets[0], nb_q, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess) ||
                hipStreamSynchronize(c->copy_stream) != hipSuccess) rc_up = MONI_ENODEV;
        });
    }
    struct JoinGuard { std::thread& t; ~JoinGuard() { if (t.joinable()) t.join(); } } join_guard{uploader};
    if ((!resident && (rc = reads_upload(c, b, false))) || (rc = seed_run_align(c, &sp))) return rc;
    // (the names and qualities are the lines kernel's: their upload is waited for after the staged kernels have been queued)
    const double t1 = mh::now_s();
    std::vector<int32_t> msc(c->max_len + 2);
    for (uint64_t l = 0; l <= c->max_len + 1; ++l) msc[l] = l ? (int32_t)(20 + 8 * log((double)l)) : INT32_MIN;      // aligner_ksw2.hpp:752-753
    int n_cu = 256, per_cu = 4;
    n_cu = ctx_n_cu(c);
    if (!c->pe_occ_cached) c->pe_occ_cached = (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pe_align_kernel, 64, 0) != hipSuccess || per_cu < 1) ? 4 : per_cu;
    per_cu = c->pe_occ_cached;
    const uint64_t waves_max = std::min<uint64_t>((uint64_t)n_cu * (uint64_t)per_cu, 4096);        // persistent waves: every block must be resident (91 KB of HBM per pair in flight)
    uint64_t NL = 16;                                                                              // pairs per wave (measured: profiles/r02z)
    if (const char* v = getenv("MONI_PE_NL")) { const long long x = atoll(v); if (x >= 1 && x <= 64) NL = (uint64_t)x; }
    // behind the staged kernels pe_align_kernel sees a few hundred pairs per chunk, the expensive ones (orphan recovery: a local alignment per chain):
    // one pair per wave - a wave solves its pairs' problems one after the other, and 16 of those pairs on one wave took 300 ms where a pair takes ~20
    // The staged kernels (pe_fast.hip) take the common case; pe_align_kernel takes the pairs they hand over (MONI_PE_V1=1: every pair)
    const bool staged = getenv("MONI_PE_V1") == nullptr && !(pe->secondary_chains && getenv("MONI_PE_Z_V1"));          // (MONI_PE_Z_V1: -Z through pe_align_kernel for every pair, the round-3 arrangement)
    if (staged && getenv("MONI_PE_NL") == nullptr) NL = 1;
    const int NS = staged ? PE_NSET : 1;                                                           // sets of the staged kernels' buffers
    // 262144 pairs: a chunk's DP kernels see ~2700 groups of 128 problems for their 1024-3072 wave slots (at 65536 pairs most slots stay empty and a
    // launch takes as long as one group: 194 -> 153 ms per 1 M pairs, profiles/r03p)
    uint64_t CH = staged ? 262144 : waves_max * NL;                                                // pairs per chunk (pe_align_kernel alone: one per lane slot)
    if (const char* v = getenv("MONI_PE_CHUNK")) { const long long x = atoll(v); if (x > 0) CH = (uint64_t)x; }
    if (CH > NP) CH = NP;
    // chunk starts.  (What follows a batch's last staged kernel is not hidden by anything: that chunk's hand-over kernel, ~30 ms whatever its size, then
    // its lines, gather and transfer.  A small last chunk was measured and does not shorten it: 140.6 against 139.1 ms per 1 M pairs, profiles/r03r.)
    std::vector<uint64_t> clo;
    for (uint64_t at = 0; at < NP; at += CH) clo.push_back(at);
    clo.push_back(NP);
    const uint64_t n_chunks = clo.size() - 1;
    uint64_t n_waves = waves_max;
    if (n_waves * NL > CH) n_waves = (CH + NL - 1) / NL;
    if (staged) n_waves = std::min<uint64_t>(n_waves, 1024);                                       // the hand-over list is short: fewer 159 KB slots
    const uint64_t cig_cap = 32 * CH + 4096, alt_cap = 48 * CH + 4096;
    // buffers of the staged kernels (one set per chunk in flight: the chunks alternate)
    const uint32_t pf_slot_cap = (uint32_t)std::min<uint64_t>((uint64_t)AF_MAX_TASKS_READ * CH + 4 * CH + 4096, 0xFFFFFFF0ull);
    const uint32_t pf_task_cap = (uint32_t)std::min<uint64_t>(24 * CH + 4096, (1ull << AF_POS_BITS) - 1), pf_tb_cap = (uint32_t)std::min<uint64_t>((8 + c->max_len / 25) * CH + 1024, 0x7FFFFFFFull);
    const uint32_t pf_chunk_cap = pf_task_cap / 64 + 2 * AF_NBIN;
    uint64_t pf_dirs_per = 32768;
    { const double f = (double)c->max_len / 150.0; if (f > 1.0) pf_dirs_per = (uint64_t)(32768.0 * f * f); }
    pf_dirs_per = std::min<uint64_t>(pf_dirs_per * c->dirs_scale, 1ull << 21);
    uint64_t pf_dirs_cap = pf_dirs_per * CH + (16ull << 20);
    // 17 GB at 2 x 150 bp, 48 GB at 2 x 250 bp, doubled after a batch that overflowed it - per context, and a front end runs several: never more than 2 / 5 of what
    // the device has free when the buffer has to grow (a chunk whose direction bits do not fit hands its pairs to pe_align_kernel: slower, same results)
    if (staged && c->af_pe[0].dirs.cap < pf_dirs_cap) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            const uint64_t lim = std::max<uint64_t>(((uint64_t)fr + c->af_pe[0].dirs.cap) / 5 * 2, 1ull << 30);
            if (pf_dirs_cap + pf_dirs_cap / 8 > lim) pf_dirs_cap = std::max<uint64_t>(lim - lim / 8, c->af_pe[0].dirs.cap);
        }
    } else if (staged) pf_dirs_cap = std::min<uint64_t>(pf_dirs_cap, c->af_pe[0].dirs.cap);
    const unsigned pf_dp_grid = (unsigned)n_cu * 12;
    if (staged) for (int x = 0; x < (int)std::min<uint64_t>(n_chunks, NS); ++x) {
        moni_ctx::AfSet& S = c->af_pe[x];
        if ((rc = S.plans.ensure(CH + 1)) || (rc = S.tasks.ensure(pf_slot_cap)) || (rc = S.res.ensure(pf_slot_cap)) || (rc = S.ntasks.ensure(CH + 8)) || (rc = S.bin_q.ensure((size_t)(AF_NBIN + 1) * pf_task_cap)) ||
            (rc = S.task_pos.ensure(pf_slot_cap)) || (rc = S.tb_task.ensure(pf_tb_cap)) || (rc = S.tb.ensure(pf_tb_cap)) || (rc = S.big_list.ensure(3 * (CH + 1))) ||
            (rc = S.ctr.ensure(AF_NCTR)) || (rc = S.bnd.ensure((size_t)pf_dp_grid * AF_QCAP * 64)) || (rc = S.chunks.ensure(pf_chunk_cap)) || (rc = S.dirs.ensure(pf_dirs_cap)) ||
            (rc = c->pe.sel[x].ensure(CH + 1)))
            return rc;
    }
    if ((rc = c->af_ctr_host.ensure((size_t)n_chunks * AF_NCTR)) || (staged && (rc = c->pe.fb[0].ensure(n_chunks * (CH + 16))))) return rc;
    if ((rc = c->pe_hcur.ensure(10 * n_chunks + 10))) return rc;
    // the hand-over list in three launches (pe_orphan_kernel): the chains of a pair that needs orphan recovery scored by `nsplit` waves at once
    uint32_t o_nsplit = 3;          // measured 2 .. 16 (profiles/r03ae/sweep.txt): with the memo a wave answers most of a block's requests from the chain before, few large blocks do best
    if (const char* v = getenv("MONI_PE_NSPLIT")) { const long long x = atoll(v); if (x >= 0 && x <= 64) o_nsplit = (uint32_t)x; }
    // (more parts for the batch's last chunk only - the tail nothing runs beside - were measured: 8, 12, 24 parts all slower than 3, profiles/r03ag/sweep.txt)
    const bool o_split = staged && finalize && pe->find_orphan && o_nsplit >= 2 && NL == 1 && !(getenv("MONI_PE_SW_WAVE") && atoi(getenv("MONI_PE_SW_WAVE")) == 0);      // (the one-lane local alignment is pe_align_kernel's)
    uint64_t k1_waves = std::min<uint64_t>((uint64_t)n_cu * 16, 4096);                                 // waves of the scoring pass: all that can be resident (92 KB of state each)
    if (const char* v = getenv("MONI_PE_K1_WAVES")) { const long long x = atoll(v); if (x >= 64 && x <= 8192) k1_waves = (uint64_t)x; }
    uint32_t o_cap = 2048;                                                                   // parked pairs per chunk (beyond: one wave does the whole pair, as before)
    if (const char* v = getenv("MONI_PE_OCAP")) { const long long x = atoll(v); if (x >= 1 && x <= 65536) o_cap = (uint32_t)x; }      // (tests: few parked pairs, the rest by one wave each)
    const int NST = staged ? PE_NSTREAM : 1;                                                       // hand-over kernels in flight, each with its slots
    bool pf_dirs_ovf = false;
    if (o_split && ((rc = c->pe.park.ensure((size_t)NST * o_cap)) || (rc = c->pe.k1_slots.ensure((size_t)NST * k1_waves)) || (rc = c->pe.k1_dirs.ensure((size_t)NST * k1_waves * PE_K1_DIRS)) || (rc = c->pe.parked.ensure((size_t)NST * o_cap)))) return rc;
    if (o_split && c->pe.orec.cap < (size_t)NST * o_cap * AC_MAX_CHAINS) { if ((rc = c->pe.orec.ensure((size_t)NST * o_cap * AC_MAX_CHAINS))) return rc; HIPCHK(hipMemset(c->pe.orec.p, 0, c->pe.orec.cap * sizeof(pe_orec_t))); }
    if ((rc = c->pe.slots.ensure(NST * n_waves * NL)) || (rc = c->pe.waves.ensure(NST * n_waves)) || (rc = c->pe.recs.ensure(n_chunks * (CH + 1))) || (rc = c->pe.cig.ensure(n_chunks * cig_cap)) ||
        (rc = c->pe.alt.ensure(n_chunks * alt_cap)) || (rc = c->pe.cur.ensure(8 * n_chunks)) || (rc = c->pe.minscore.ensure(msc.size()))) return rc;
    if (!c->copy_stream) HIPCHK(hipStreamCreateWithFlags(&c->copy_stream.h, hipStreamNonBlocking));
    const uint64_t ln_per = 2 * CH + 8;                          // lines of a chunk (two per pair)
    size_t scan_bytes = 0;
    if (txt) {
        const uint32_t TAB = 8192, SUBN = 1024;
        if ((rc = c->pe.txt_pool.ensure((size_t)NST * CH * PEL_PAIR_WORDS + 8)) || (rc = c->pe.block.ensure(n_chunks * CH * PEL_PAIR_WORDS + 8)) || (rc = c->pe.dev_len.ensure(n_chunks * ln_per)) ||
            (rc = c->pe.dev_off.ensure(n_chunks * ln_per)) || (rc = c->pe.dev_pos.ensure(n_chunks * ln_per)) || (rc = c->ak_dev_sum.ensure(160 * n_chunks + 8)) || (rc = c->h_sum.ensure(4 * n_chunks + 4)) ||
            (rc = c->ak_mapq_tab.ensure(TAB)) || (rc = c->pe.subn_tab.ensure(SUBN))) return rc;
        if (rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(2 * CH), rocprim::plus<uint64_t>(), c->stream) != hipSuccess) return MONI_ENODEV;
        for (int x = 0; x < NST; ++x) if ((rc = c->pe.scan_tmp[x].ensure(scan_bytes + 16))) return rc;
        if (!c->mapq_tab_ready) {
            std::vector<double> tab(TAB, 1.);
            const int32_t coeff_fac = (int32_t)log(50.0f);                                 // aligner_ksw2.hpp:3250-3251
            for (int32_t l = 2; l < (int32_t)TAB; ++l) tab[l] = coeff_fac / log(l);         // the expression of mapq.hpp:170, libm on the host
            HIPCHK(hipMemcpy(c->ak_mapq_tab.p, tab.data(), TAB * sizeof(double), hipMemcpyHostToDevice));
            c->mapq_tab_ready = true;
        }
        if (!c->pe.subn_ready) {
            std::vector<int32_t> tab(SUBN, 0);
            for (int32_t n = 1; n < (int32_t)SUBN; ++n) tab[n] = (int)(4.343 * log(n + 1) + .499);      // mapq.hpp:176, 208 (libm on the host)
            HIPCHK(hipMemcpy(c->pe.subn_tab.p, tab.data(), SUBN * sizeof(int32_t), hipMemcpyHostToDevice));
            c->pe.subn_ready = true;
        }
        HIPCHK(hipMemsetAsync(c->ak_dev_sum.p, 0, (160 * n_chunks + 8) * sizeof(unsigned long long), c->stream));
        memset(c->h_sum.p, 0, (4 * n_chunks + 4) * sizeof(unsigned long long));
    }
    std::vector<Event> ev(n_chunks), ev_staged(n_chunks);
    for (uint64_t i = 0; i < n_chunks; ++i) { HIPCHK(hipEventCreateWithFlags(&ev[i].h, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&ev_staged[i].h, hipEventDisableTiming)); }
    HIPCHK(hipMemcpyAsync(c->pe.minscore.p, msc.data(), msc.size() * 4, hipMemcpyHostToDevice, c->stream));
    pe_args_t A;
    memset(&A, 0, sizeof A);
    ac_params_t& P = A.PP.P;
    P.min_len = prm->min_len; P.ext_len = prm->ext_len; P.check_k = prm->check_k; P.region_dist = prm->region_dist;
    P.filter_freq = prm->filter_freq; P.left_mem_check = prm->left_mem_check; P.freq_thr = prm->freq_thr;
    P.smatch = prm->smatch; P.gapo = prm->gapo; P.gapo2 = prm->gapo2; P.gape = prm->gape; P.gape2 = prm->gape2;
    P.max_dist_x = prm->max_dist_x; P.max_dist_y = prm->max_dist_y; P.max_iter = prm->max_iter; P.max_pred = prm->max_pred;
    P.min_chain_score = prm->min_chain_score; P.min_chain_length = prm->min_chain_length;
    P.n_text = I->K.n_text; P.n_seq = I->K.n_seq; P.seq_starts = I->d_seq_starts.p;
    P.lift_seqs = I->d_lift_seqs.p; P.lift_runs = I->d_lift_runs.p; P.pdir = I->d_pdir.p;
    A.PP.smismatch = prm->smismatch; A.PP.max_penalty = (int32_t)(int8_t)std::max(prm->smatch + prm->smismatch, prm->gapo + prm->gape);
    A.PP.filter_dir = pe->filter_dir; A.PP.finalize = finalize ? 1u : 0u; A.PP.dir_thr = pe->dir_thr; A.PP.mean = (float)mean; A.PP.std_dev = (float)std_dev;
    A.PP.secondary_chains = pe->secondary_chains ? 1u : 0u;
    A.PP.find_orphan = (finalize && pe->find_orphan) ? 1u : 0u; A.PP.w = (uint32_t)I->hix.w; A.PP.ins_mean = mean; A.PP.ins_std_dev = std_dev;
    // the pairing term's penalty per dist, from the host's libm (pe_core.h: pe_pair_pen); the host pipeline reads the same table in host memory
    std::vector<double> pen_tab(PE_PEN_TAB);
    A.PP.pen_tab = nullptr; A.PP.pen_tab_n = 0;
    for (uint32_t d = 0; d < PE_PEN_TAB; ++d) pen_tab[d] = pe_pair_pen(A.PP, (long long)d);
    if ((rc = c->pe.pen_tab.ensure(PE_PEN_TAB))) return rc;
    HIPCHK(hipMemcpyAsync(c->pe.pen_tab.p, pen_tab.data(), PE_PEN_TAB * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    A.PP.pen_tab = c->pe.pen_tab.p; A.PP.pen_tab_n = PE_PEN_TAB;
    A.D.sc_mch = prm->smatch; A.D.sc_mis = -prm->smismatch; A.D.sc_N = -prm->gape; A.D.wild = 4; A.D.qo = prm->gapo; A.D.e = prm->gape;
    A.D.end_bonus = prm->end_bonus; A.D.reads = c->seq.p; A.D.text = I->d_text.p; A.D.n_text = I->K.n_text;
    A.D.reads_limit = (c->total_len + 8) & ~7ull; A.D.text_limit = (I->K.n_text + 8) & ~7ull;
    A.mems = c->mems.p; A.occs = c->tmp.p; A.read_mem_off = c->read_mem_off.p; A.aux = c->aux.p; A.offs = c->offs.p;
    A.min_score_of_len = c->pe.minscore.p; A.max_len = (uint32_t)c->max_len + 1;
    A.sw_wave = 1;                     // MONI_PE_SW_WAVE=0: the orphan search by the pair's own lane (the first, slower form; same results)
    if (const char* v = getenv("MONI_PE_SW_WAVE")) A.sw_wave = atoi(v) ? 1u : 0u;
    A.nl = (uint32_t)NL; A.cig_cap = cig_cap; A.alt_cap = alt_cap;
    std::vector<uint32_t> one_level_n(n_chunks);
    for (uint64_t k = 0; k < n_chunks; ++k) one_level_n[k] = (uint32_t)(clo[k + 1] - clo[k]);
    // phase 0: the chunk's staged kernels on the context's stream; phase 1: what follows them on the chunk's own stream (hand-over launches, lines, gather)
    auto launch = [&](uint64_t k, int phase) -> int {
        const int set = (int)(k % (uint64_t)NS), st = (int)(k % (uint64_t)NST);
        A.slots = c->pe.slots.p + (size_t)st * n_waves * NL; A.waves = c->pe.waves.p + (size_t)st * n_waves;
        A.pair_lo = clo[k]; A.n_pairs = clo[k + 1] - clo[k];
        A.recs = c->pe.recs.p + (size_t)k * (CH + 1); A.cig_pool = c->pe.cig.p + (size_t)k * cig_cap; A.alt_pool = c->pe.alt.p + (size_t)k * alt_cap;
        A.cursors = c->pe.cur.p + 8 * k;
        if (phase == 0) HIPCHK(hipMemsetAsync(A.cursors, 0, 8 * sizeof(unsigned long long), c->stream));
        A.pair_list = nullptr; A.n_list = nullptr;
        if (staged && phase == 1) { uint32_t* const fbk = c->pe.fb[0].p + (size_t)k * (CH + 16); A.pair_list = fbk + 16; A.n_list = fbk; }
        if (staged && phase == 0) {
            moni_ctx::AfSet& S = c->af_pe[set];
            pef_args_t X;
            memset(&X, 0, sizeof X);
            af_args_t& G = X.G;
            G.A.P = A.PP.P; G.A.D = A.D; G.A.mems = A.mems; G.A.occs = A.occs; G.A.read_mem_off = A.read_mem_off; G.A.offs = A.offs;
            G.A.min_score_of_len = A.min_score_of_len; G.A.max_len = A.max_len; G.A.read_lo = A.pair_lo; G.A.n_reads = A.n_pairs;
            G.pe = 1; G.pe_sel = c->pe.sel[set].p; G.chain_narrow = cc_narrow_ok(G.A.P) ? 1u : 0u;
            G.plans = S.plans.p; G.tasks = S.tasks.p; G.task_cap = pf_slot_cap; G.ntasks = S.ntasks.p; G.res = S.res.p; G.bin_q = S.bin_q.p; G.bin_cap = pf_task_cap; G.task_pos = S.task_pos.p;
            G.chunks = S.chunks.p; G.chunk_cap = pf_chunk_cap; G.dirs = S.dirs.p; G.dirs_cap = pf_dirs_cap; G.tb_task = S.tb_task.p; G.tb = S.tb.p; G.tb_cap = pf_tb_cap;
            uint32_t* const fbk = c->pe.fb[0].p + (size_t)k * (CH + 16);
            G.fb_n = fbk; G.fb_list = fbk + 16; G.big_list = S.big_list.p; G.huge_list = S.big_list.p + (CH + 1); G.list0 = S.big_list.p + 2 * (CH + 1);
            G.ctr = S.ctr.p; G.bnd = S.bnd.p;
            G.pat = c->pat.p; G.blk = c->blk.p; G.text2 = I->d_text2.p; G.exc = I->d_exc.p; G.exc_sh = I->exc_sh; G.pflag = c->pflag.p; G.wave_max = af_wave_max();
            X.PP = A.PP; X.aux = A.aux; X.recs = A.recs; X.cig_pool = A.cig_pool; X.cig_cap = A.cig_cap; X.alt_pool = A.alt_pool; X.alt_cap = A.alt_cap; X.cursors = A.cursors;
            HIPCHK(hipMemsetAsync(S.ctr.p, 0, AF_NCTR * sizeof(uint32_t), c->stream));
            HIPCHK(hipMemsetAsync(fbk, 0, 16 * sizeof(uint32_t), c->stream));
            const uint64_t np = A.n_pairs;
            hipStream_t sx = c->stream;
            static const bool one_level = getenv("MONI_PE_ONE_LEVEL") != nullptr;      // (every pair on the large instance: the arrangement before the small one existed)
            if (one_level) {
                HIPCHK(hipMemcpyAsync(S.ctr.p + AFC_BIG, &one_level_n[k], 4, hipMemcpyHostToDevice, sx));
                hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, sx, S.big_list.p, (uint32_t)np);
            } else if (pe->secondary_chains) hipLaunchKernelGGL((pe_plan_kernel<pef_wave_small_z_t, 3, PEF_RAW_SMALL, 0>), dim3((unsigned)std::min<uint64_t>(np, (uint64_t)n_cu * 13)), dim3(64), 0, sx, X);
            else hipLaunchKernelGGL((pe_plan_kernel<pef_wave_small_t, 4, PEF_RAW_SMALL, 0>), dim3((unsigned)std::min<uint64_t>(np, (uint64_t)n_cu * 17)), dim3(64), 0, sx, X);
            // (-Z: the instances with the second track of find_chains_secondary, chain.hpp:442-727)
            if (pe->secondary_chains) {
                hipLaunchKernelGGL((pe_plan_kernel<pef_wave_z_t, 2, PEF_RAW, 1, 0>), dim3((unsigned)std::min<uint64_t>(np, (uint64_t)n_cu * 8)), dim3(64), 0, sx, X);
                hipLaunchKernelGGL((pe_plan_kernel<pef_wave_zz_t, 1, PEF_RAW, 2, 1>), dim3((unsigned)std::min<uint64_t>(np, (uint64_t)n_cu * 4)), dim3(64), 0, sx, X);
            }
            else hipLaunchKernelGGL((pe_plan_kernel<pef_wave_t, 2, PEF_RAW, 1>), dim3((unsigned)std::min<uint64_t>(np, (uint64_t)n_cu * 9)), dim3(64), 0, sx, X);
            hipLaunchKernelGGL(bin_tasks_kernel, dim3((unsigned)((np + AF_BT_READS - 1) / AF_BT_READS)), dim3(256), 0, sx, G);
            af_launch_dp(G, sx, pf_dp_grid, (unsigned)n_cu, np);
            hipLaunchKernelGGL(pe_select_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, sx, X);
            hipLaunchKernelGGL(traceback_kernel, dim3((unsigned)((pf_tb_cap + 255) / 256)), dim3(256), 0, sx, G);
            hipLaunchKernelGGL(pe_finish_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, sx, X);
            HIPCHK(hipMemcpyAsync(c->af_ctr_host.p + AF_NCTR * k, S.ctr.p, AF_NCTR * sizeof(uint32_t), hipMemcpyDeviceToHost, sx));
            HIPCHK(hipEventRecord(ev_staged[k], c->stream));
            HIPCHK(hipGetLastError());
        }
        if (phase == 0) return MONI_OK;
        // the hand-over pairs run on their own stream beside the next chunk's staged kernels (its other buffer set); the host takes this chunk when they are through
        hipStream_t sf = c->stream;
        if (staged) {
            if (!c->pe_stream[st]) HIPCHK(hipStreamCreateWithFlags(&c->pe_stream[st].h, hipStreamNonBlocking));
            sf = c->pe_stream[st];
            HIPCHK(hipStreamWaitEvent(sf, ev_staged[k], 0));
        }
        if (o_split) {
            pe_oargs_t O;
            O.park = c->pe.park.p + (size_t)st * o_cap; O.parked = c->pe.parked.p + (size_t)st * o_cap; O.cap = o_cap;
            O.orec = c->pe.orec.p + (size_t)st * o_cap * AC_MAX_CHAINS; O.nsplit = o_nsplit; O.tag = ++pe_launch_tag; O.k1_slots = c->pe.k1_slots.p + (size_t)st * k1_waves; O.k1_dirs = c->pe.k1_dirs.p + (size_t)st * k1_waves * PE_K1_DIRS; O.k1_dirs_cap = PE_K1_DIRS;
            if (O.tag == 0) O.tag = ++c->pe.tag;
            hipLaunchKernelGGL((pe_orphan_kernel<3>), dim3((unsigned)n_waves), dim3(64), 0, sf, A, O);
            hipLaunchKernelGGL((pe_orphan_kernel<1>), dim3((unsigned)k1_waves), dim3(64), 0, sf, A, O);
            hipLaunchKernelGGL((pe_orphan_kernel<2>), dim3((unsigned)n_waves), dim3(64), 0, sf, A, O);
        } else
        hipLaunchKernelGGL(pe_align_kernel, dim3((unsigned)std::min<uint64_t>(n_waves, (A.n_pairs + NL - 1) / NL)), dim3(64), 0, sf, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->pe_hcur.p + 10 * k, A.cursors, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, sf));
        if (staged) HIPCHK(hipMemcpyAsync(c->pe_hcur.p + 10 * k + 8, c->pe.fb[0].p + (size_t)k * (CH + 16), sizeof(uint32_t), hipMemcpyDeviceToHost, sf));
        if (txt) {          // the pair's two lines, then the chunk's lines in input order: scan of the lengths, gather, summary for the host
            pel_args_t Y;
            memset(&Y, 0, sizeof Y);
            Y.P = A.PP.P; Y.D = A.D; Y.offs = A.offs;
            Y.F.rnames = c->ak_rnames.p; Y.F.rname_off = c->ak_rname_off.p; Y.F.quals = txt->quals ? c->ak_quals.p : nullptr;
            Y.F.snames = I->d_snames.p; Y.F.sname_off = I->d_sname_off.p; Y.F.mapq_tab = c->ak_mapq_tab.p; Y.F.mapq_tab_n = 8192;
            Y.F.min_len = (int32_t)prm->min_len; Y.F.smatch = prm->smatch; Y.F.smismatch = prm->smismatch;
            Y.recs = A.recs; Y.cig_pool = A.cig_pool; Y.alt_pool = A.alt_pool; Y.pair_lo = A.pair_lo; Y.n_pairs = A.n_pairs;
            Y.subn_tab = c->pe.subn_tab.p; Y.subn_tab_n = 1024; Y.min_score_of_len = A.min_score_of_len; Y.max_len = (uint32_t)c->max_len;
            Y.txt_pool = c->pe.txt_pool.p + (size_t)st * CH * PEL_PAIR_WORDS;
            Y.dev_len = c->pe.dev_len.p + k * ln_per; Y.dev_off = c->pe.dev_off.p + k * ln_per; Y.dev_sum = c->ak_dev_sum.p + 160 * k;
            uint64_t* pos = c->pe.dev_pos.p + k * ln_per;
            const uint64_t np = A.n_pairs, nl2 = 2 * np;
            hipLaunchKernelGGL(pe_lines_kernel, dim3((unsigned)std::min<uint64_t>(np, (uint64_t)n_cu * 32)), dim3(64), 0, sf, Y);
            size_t tmp_bytes = 0;
            if (rocprim::exclusive_scan(nullptr, tmp_bytes, Y.dev_len, pos, (uint64_t)0, (size_t)nl2, rocprim::plus<uint64_t>(), sf) != hipSuccess || tmp_bytes > scan_bytes + 16) return MONI_ENODEV;
            if (rocprim::exclusive_scan(c->pe.scan_tmp[st].p, tmp_bytes, Y.dev_len, pos, (uint64_t)0, (size_t)nl2, rocprim::plus<uint64_t>(), sf) != hipSuccess) return MONI_ENODEV;
            hipLaunchKernelGGL(gather_lines_kernel, dim3((unsigned)std::min<uint64_t>((nl2 + 3) / 4, (uint64_t)n_cu * 8)), dim3(256), 0, sf, (const uint64_t*)Y.txt_pool,
                               (const uint64_t*)Y.dev_len, (const uint64_t*)Y.dev_off, (const uint64_t*)pos, nl2, reinterpret_cast<uint8_t*>(c->pe.block.p + k * CH * PEL_PAIR_WORDS));
            hipLaunchKernelGGL(gather_summary_kernel, dim3(1), dim3(64), 0, sf, (const uint64_t*)Y.dev_len, (const uint64_t*)pos, nl2, (const unsigned long long*)Y.dev_sum, Y.dev_sum + 150);
            HIPCHK(hipMemcpyAsync(c->h_sum.p + 4 * k, Y.dev_sum + 150, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, sf));
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ev[k], sf));
        return MONI_OK;
    };
    PeChunk ch;
    double t_host = 0;
    std::vector<PeBigPair> big;
    std::vector<moni_mem_t> h_mems; std::vector<uint64_t> h_occs, h_rmo, h_offs; std::vector<uint32_t> h_aux;
    auto take = [&](uint64_t k) -> int {
        HIPCHK(hipEventSynchronize(ev[k]));
        ch.lo = clo[k]; ch.n = clo[k + 1] - clo[k];
        if (txt) {
            const unsigned long long* sm = c->h_sum.p + 4 * k;
            if (sm[1] == 0 && sm[0] <= CH * PEL_PAIR_WORDS * 8) {          // every line of the chunk was written by the kernels: the block goes straight into the text buffer
                const double h0 = mh::now_s();
                txt->pairs_upto = ch.lo + ch.n;
                if (*txt->used + (size_t)sm[0] + 1 > c->out_buf.cap) HIPCHK(hipStreamSynchronize(c->copy_stream));      // the buffer is about to move
                char* dst = txt->room(*txt->used + (size_t)sm[0] + 1);
                if (!dst) return MONI_ENOMEM;
                // (no wait here: the transfers queue up on the copy stream behind one another while the host goes on to the next chunk; pe_run waits for
                // them at its end.  room() may move the buffer only while nothing is in flight)
                if (sm[0]) HIPCHK(hipMemcpyAsync(dst + *txt->used, c->pe.block.p + k * CH * PEL_PAIR_WORDS, (size_t)sm[0], hipMemcpyDeviceToHost, c->copy_stream));
                *txt->used += (size_t)sm[0]; txt->aligned += sm[2]; ++txt->chunks_gpu;
                if (stats) {
                    const unsigned long long* cur2 = c->pe_hcur.p + 10 * k;
                    stats->dp_tasks += cur2[2]; stats->dp_cells += cur2[3]; stats->dp_rounds += 1;
                    if (staged) {
                        const uint32_t* fc = c->af_ctr_host.p + AF_NCTR * k;
                        unsigned long long cells; memcpy(&cells, fc + AFC_CELLS, 8); if (stats) { unsigned long long cutc, slots; memcpy(&cutc, fc + AFC_CUTCELLS, 8); memcpy(&slots, fc + AFC_SLOTS, 8); stats->dp_cells_cut += cutc; stats->dp_slots += slots; }
                        const uint32_t nfb = (uint32_t)(cur2[8] & 0xFFFFFFFFull);
                        stats->dp_tasks += fc[AFC_NT]; stats->dp_cells += cells; stats->kernel_fallback += nfb; for (int x = 0; x < 12; ++x) stats->handover_why[x] += fc[AFC_WHY + x];
                    }
                }
                if (staged) pf_dirs_ovf = pf_dirs_ovf || c->af_ctr_host.p[AF_NCTR * k + AFC_DIRS_OVF] != 0;
                t_host += mh::now_s() - h0;
                return MONI_OK;
            }
            ++txt->chunks_host;
        }
        unsigned long long cur[8];
        ch.recs.resize(ch.n);
        HIPCHK(hipMemcpyAsync(cur, c->pe.cur.p + 8 * k, sizeof cur, hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(hipMemcpyAsync(ch.recs.data(), c->pe.recs.p + (size_t)k * (CH + 1), ch.n * sizeof(pe_rec_t), hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(hipStreamSynchronize(c->copy_stream));
        const uint64_t nc = std::min<uint64_t>(cur[0], cig_cap), na = std::min<uint64_t>(cur[1], alt_cap);
        ch.cig.resize(nc + 1); ch.alt.resize(na + 1);
        if (nc) HIPCHK(hipMemcpyAsync(ch.cig.data(), c->pe.cig.p + (size_t)k * cig_cap, nc * 4, hipMemcpyDeviceToHost, c->copy_stream));
        if (na) HIPCHK(hipMemcpyAsync(ch.alt.data(), c->pe.alt.p + (size_t)k * alt_cap, na * sizeof(moni_alt_t), hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(hipStreamSynchronize(c->copy_stream));
        if (stats) { stats->dp_tasks += cur[2]; stats->dp_cells += cur[3]; stats->dp_rounds += 1; }
        if (staged) {          // the staged kernels' own counters (copied on the launch stream before the event)
            const uint32_t* fc = c->af_ctr_host.p + AF_NCTR * k;
            unsigned long long cells; memcpy(&cells, fc + AFC_CELLS, 8); if (stats) { unsigned long long cutc, slots; memcpy(&cutc, fc + AFC_CUTCELLS, 8); memcpy(&slots, fc + AFC_SLOTS, 8); stats->dp_cells_cut += cutc; stats->dp_slots += slots; }
            uint32_t nfb = 0;
            HIPCHK(hipMemcpy(&nfb, c->pe.fb[0].p + (size_t)k * (CH + 16), 4, hipMemcpyDeviceToHost));
            if (stats) { stats->dp_tasks += fc[AFC_NT]; stats->dp_cells += cells; stats->kernel_fallback += nfb; for (int x = 0; x < 12; ++x) stats->handover_why[x] += fc[AFC_WHY + x]; }
            pf_dirs_ovf = pf_dirs_ovf || fc[AFC_DIRS_OVF] != 0;
            if (getenv("MONI_AK_PROFILE")) fprintf(stderr, "  staged paired kernels, chunk %llu: %u DP tasks, %llu cells, %u traced, %u pairs to pe_align_kernel%s; %u pairs beyond the small instance of pe_plan_kernel, %u beyond the large one\n", (unsigned long long)k, fc[AFC_NT], cells,
                                                   fc[AFC_TRACED], nfb, fc[AFC_DIRS_OVF] ? " (direction bits overflowed)" : "", fc[AFC_BIG], fc[AFC_HUGE]);
        }
        // pairs beyond the kernel's capacities: the same state machine with large capacities on the host, DP on the GPU (pe_big.h)
        if (force_big) for (uint64_t i = 0; i < ch.n; ++i) if ((ch.lo + i) % force_big == 0) ch.recs[i].status = 2;
        big.clear();
        for (uint64_t i = 0; i < ch.n; ++i) if (ch.recs[i].status == 2) { PeBigPair bp; bp.pair = ch.lo + i; big.push_back(std::move(bp)); }
        if (!big.empty()) {
            if (h_mems.empty()) {          // the batch's seeds, once
                h_mems.resize(c->n_mems + 1); h_occs.resize(c->n_occs + 1); h_rmo.resize(c->n_reads + 1); h_aux.resize(c->n_mems + 1); h_offs.resize(c->n_reads + 1);
                if ((rc = moni_seed_fetch(c, h_mems.data(), h_occs.data(), h_rmo.data()))) return rc;          // the host reads the lists as one array: compacted here, on demand
                if (c->n_mems) HIPCHK(hipMemcpyAsync(h_aux.data(), c->aux.p, c->n_mems * 4, hipMemcpyDeviceToHost, c->copy_stream));
                HIPCHK(hipMemcpyAsync(h_offs.data(), c->offs.p, (c->n_reads + 1) * 8, hipMemcpyDeviceToHost, c->copy_stream));
                HIPCHK(hipStreamSynchronize(c->copy_stream));
            }
            pe_params_t HP = A.PP;
            HP.pen_tab = pen_tab.data();
            HP.P.seq_starts = I->hix.seq_starts.data(); HP.P.lift_seqs = I->hix.lift_seqs.data(); HP.P.lift_runs = I->hix.lift_runs.data(); HP.P.pdir = nullptr;
            moni_dp_params_t dpp;
            memset(&dpp, 0, sizeof dpp);
            dpp.m = 5;
            for (int x = 0; x < 4; ++x) for (int y = 0; y < 4; ++y) dpp.mat[x * 5 + y] = x == y ? prm->smatch : (int8_t)-prm->smismatch;
            dpp.q = prm->gapo; dpp.e = prm->gape; dpp.w = -1; dpp.zdrop = -1; dpp.end_bonus = prm->end_bonus;
            const int rb = pe_big_run(&HP, sizeof HP, h_mems.data(), h_rmo.data(), h_aux.data(), h_occs.data(), h_offs.data(), big,
                                      [&](const std::vector<moni_dp_task_t>& t, std::vector<moni_dp_result_t>& r, std::vector<uint32_t>& cg) -> int {
                                          r.resize(t.size());
                                          if (stats) { stats->dp_tasks += t.size(); }
                                          // the local-alignment requests of orphan recovery go to pe_sw_kernel (one lane each), the rest to the DP kernels
                                          std::vector<moni_dp_task_t> lt, ot; std::vector<size_t> li, oi;
                                          for (size_t x = 0; x < t.size(); ++x) { if (t[x].flag & DP_EZ_LOCAL) { lt.push_back(t[x]); li.push_back(x); } else { ot.push_back(t[x]); oi.push_back(x); } }
                                          // a mate beyond the rows pe_sw_kernel keeps per request: no silent zero result - the batch fails with MONI_ERANGE, as the header documents
                                          for (const moni_dp_task_t& x : lt) if (x.qlen > PE_SW_QMAX) { fprintf(stderr, "moni_hip: orphan recovery of a mate of %d bases (more than %d)\n", x.qlen, PE_SW_QMAX); return MONI_ERANGE; }
                                          cg.clear();
                                          if (!ot.empty()) {
                                              std::vector<moni_dp_result_t> orr(ot.size());
                                              const int rd = dp_run(c, &dpp, nullptr, 0, nullptr, 0, ot.data(), ot.size(), orr.data(), cg, true);
                                              if (rd) return rd;
                                              for (size_t x = 0; x < ot.size(); ++x) r[oi[x]] = orr[x];
                                          }
                                          if (!lt.empty()) {
                                              DBuf<moni_dp_task_t> dt; DBuf<pe_sw_ws_t> dw; DBuf<moni_dp_result_t> dr;
                                              int rl;
                                              if ((rl = dt.ensure(lt.size())) || (rl = dw.ensure(lt.size())) || (rl = dr.ensure(lt.size()))) return rl;
                                              std::vector<moni_dp_result_t> lr(lt.size());
                                              bool ok = hipMemcpy(dt.p, lt.data(), lt.size() * sizeof(moni_dp_task_t), hipMemcpyHostToDevice) == hipSuccess;
                                              if (ok) { hipLaunchKernelGGL(pe_sw_kernel, dim3((unsigned)((lt.size() + 63) / 64)), dim3(64), 0, c->copy_stream, A.D, (const moni_dp_task_t*)dt.p, (uint32_t)lt.size(), dw.p, dr.p);
                                                        ok = hipStreamSynchronize(c->copy_stream) == hipSuccess && hipMemcpy(lr.data(), dr.p, lt.size() * sizeof(moni_dp_result_t), hipMemcpyDeviceToHost) == hipSuccess; }
                                              if (!ok) return MONI_ENODEV;
                                              for (size_t x = 0; x < lt.size(); ++x) r[li[x]] = lr[x];
                                          }
                                          return MONI_OK;
                                      });
            if (rb) return rb;
            for (const PeBigPair& bp : big) {
                if (csvq) { csvq->filter[bp.pair] = bp.csv_filter; csvq->skipped[bp.pair] = bp.csv_skipped; }
                pe_rec_t& R = ch.recs[bp.pair - ch.lo];
                R.status = bp.status; R.strand = bp.strand; R.tot = bp.tot; R.score2 = bp.score2; R.sub_n = bp.sub_n; R.dist = bp.dist;
                for (int k = 0; k < 2; ++k) {
                    R.score2_m[k] = bp.score2_m[k]; R.mate_score[k] = bp.mate_score[k]; R.filled[k] = bp.filled[k]; R.orphan[k] = bp.orphan[k]; R.ref_pos[k] = bp.ref_pos[k]; R.as[k] = bp.as[k];
                    R.n_cigar[k] = (uint32_t)bp.cig[k].size(); R.cigar_off[k] = ch.cig.size(); ch.cig.insert(ch.cig.end(), bp.cig[k].begin(), bp.cig[k].end());
                    R.n_alt[k] = (uint32_t)bp.alt_pos[k].size(); R.alt_off[k] = ch.alt.size();
                    for (size_t x = 0; x < bp.alt_pos[k].size(); ++x) { moni_alt_t al; al.pos = bp.alt_pos[k][x]; al.score = bp.alt_score[k][x]; al.pad = 0; ch.alt.push_back(al); }
                }
            }
            if (stats) stats->handed_back += big.size();
            ch.cig.push_back(0); { moni_alt_t z; z.pos = 0; z.score = 0; z.pad = 0; ch.alt.push_back(z); }      // (an empty list may point one past the end)
        }
        const double h0 = mh::now_s();
        const int r = consume(ch);
        t_host += mh::now_s() - h0;
        return r;
    };
    rc = MONI_OK;
    const double t_prep = mh::now_s();
    for (uint64_t k = 0; k < n_chunks && !rc; ++k) rc = launch(k, 0);
    if (uploader.joinable()) uploader.join();
    if (!rc && rc_up) rc = rc_up;
    for (uint64_t k = 0; k < n_chunks && !rc; ++k) rc = launch(k, 1);
    if (getenv("MONI_AK_PROFILE")) fprintf(stderr, "  paired path: %.2f ms between the seeds and the first launch, %.2f ms to queue %llu chunks\n", (t_prep - t1) * 1e3, (mh::now_s() - t_prep) * 1e3, (unsigned long long)n_chunks);
    for (uint64_t k = 0; k < n_chunks && !rc; ++k) rc = take(k);
    (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream && hipStreamSynchronize(c->copy_stream) != hipSuccess && !rc) rc = MONI_ENODEV;
    for (int x = 0; x < PE_NSTREAM; ++x) if (c->pe_stream[x]) (void)hipStreamSynchronize(c->pe_stream[x]);
    if (pf_dirs_ovf && c->dirs_scale < 32) c->dirs_scale *= 2;
    if (stats) { stats->reads = b->n_reads; stats->t_seed += t1 - t0; stats->t_dp += mh::now_s() - t1 - t_host; stats->t_host += t_host; }
    return rc;
}

void moni_pe_params_default(moni_pe_params_t* p) {
    if (!p) return;
    p->filter_dir = 1; p->find_orphan = 1; p->dir_thr = 50.0; p->ins_learning_n = 1000; p->ins_learning_score_gap_threshold = 0; p->secondary_chains = 0; p->reserved = 0;
}

int moni_pe_learn_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_align_params_t* prm, const moni_pe_params_t* pe, moni_pe_model_t* model) {
    if (!c || !b || !prm || !pe || !model) return MONI_EINVAL;
    const uint64_t NP = b->n_reads / 2;
    std::vector<uint8_t> al(NP); std::vector<int32_t> tot(NP), s2(NP), ms(NP); std::vector<long long> dist(NP);
    int rc = pe_run(c, b, prm, pe, false, 0.0, 0.0, [&](const PeChunk& ch) -> int {
        for (uint64_t i = 0; i < ch.n; ++i) {
            const uint64_t p = ch.lo + i;
            const pe_rec_t& R = ch.recs[i];
            if (R.status == 2) return MONI_ERANGE;            // beyond the host pipeline's capacities too
            al[p] = R.status == 1; tot[p] = R.tot; s2[p] = R.score2; dist[p] = R.dist;
            const uint64_t l1 = b->offsets[2 * p + 1] - b->offsets[2 * p], l2 = b->offsets[2 * p + 2] - b->offsets[2 * p + 1];
            ms[p] = (int32_t)(20 + 8 * log((double)l1)) + (int32_t)(20 + 8 * log((double)l2));
        }
        return MONI_OK;
    }, nullptr);
    if (rc) return rc;
    mh::PeModel M;
    M.mean = model->mean; M.std_dev = model->std_dev; M.variance = model->variance; M.sample_variance = model->sample_variance; M.m2 = model->m2;
    M.count = model->count; M.complete = model->complete != 0;
    mh::pe_learn_update(M, al.data(), tot.data(), s2.data(), ms.data(), dist.data(), NP, pe->ins_learning_n, pe->ins_learning_score_gap_threshold);
    model->mean = M.mean; model->std_dev = M.std_dev; model->variance = M.variance; model->sample_variance = M.sample_variance; model->m2 = M.m2;
    model->count = M.count; model->complete = M.complete ? 1u : 0u;
    return MONI_OK;
}

// The text is assembled in the context's pinned buffer (kept across calls: the chunks' blocks land in it by DMA, a chunk the host finishes is written
// into it by the host threads); own_buf: the caller gets that buffer (moni_pe_align_stream) instead of a malloc'ed copy
static int pe_align_text(moni_ctx_t* c, const moni_read_batch_t* b, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals,
                         const moni_align_params_t* prm, const moni_pe_params_t* pe, const moni_pe_model_t* model, char** sam, uint64_t* sam_len,
                         moni_align_stats_t* stats, bool own_buf, bool resident = false, std::string* csv_out = nullptr) {
    if (!c || !b || !prm || !pe || !model || !sam || !sam_len || (b->n_reads && (!names || !name_off))) return MONI_EINVAL;
    PeCsvCounts csvq;
    try {
        const double w0 = mh::now_s();
        if (stats) memset(stats, 0, sizeof *stats);
        if (hipSetDevice(c->idx->device) != hipSuccess) return MONI_ENODEV;
        const uint8_t* base = b->seq + b->offsets[0];
        const uint8_t* qbase = quals ? quals + b->offsets[0] : nullptr;
        mh::Aligner AL(c->idx->hix, *prm, base, b->offsets);
        const int T = prm->host_threads > 0 ? (int)prm->host_threads : 1;
        mh::Pool pool(T);
        std::vector<std::string> piece(T);
        std::vector<uint64_t> aligned(T, 0);
        size_t used = 0;
        const uint64_t NP_all = b->n_reads / 2;
        PeText txt;
        auto room = [&](size_t need) -> char* {          // grows the pinned buffer (sized from the bytes per pair so far), keeps the first `used` bytes
            if (need <= c->out_buf.cap) return c->out_buf.p;
            size_t want = need + need / 8 + 65536;
            if (txt.pairs_upto) want = std::max<size_t>(want, (size_t)((double)need / (double)txt.pairs_upto * 1.06 * (double)NP_all) + 65536);
            return c->out_buf.ensure_keep(want, used) ? nullptr : c->out_buf.p;
        };
        std::vector<size_t> at(T + 1, 0);
        txt.names = names; txt.name_off = name_off; txt.quals = quals; txt.room = room; txt.used = &used;
        bool over = false;
        uint64_t chunk_pairs = 0;
        int rc = pe_run(c, b, prm, pe, true, model->mean, model->std_dev, [&](const PeChunk& ch) -> int {
            for (uint64_t i = 0; i < ch.n; ++i) if (ch.recs[i].status == 2) { over = true; return MONI_ERANGE; }
            pool.run([&](int t) {
                std::string& dst = piece[t];
                dst.clear();
                const uint64_t lo = ch.n * t / T, hi = ch.n * (t + 1) / T;
                std::vector<uint64_t> ap; std::vector<int32_t> as;
                for (uint64_t i = lo; i < hi; ++i) {
                    const uint64_t p = ch.lo + i;
                    const pe_rec_t& R = ch.recs[i];
                    mh::PePairOut O;
                    O.finalized = R.status == 1; O.strand = R.strand; O.tot = R.tot; O.score2 = R.score2; O.sub_n = R.sub_n;
                    ap.clear(); as.clear();
                    for (int k = 0; k < 2; ++k) for (uint32_t x = 0; x < R.n_alt[k]; ++x) { ap.push_back(ch.alt[R.alt_off[k] + x].pos); as.push_back(ch.alt[R.alt_off[k] + x].score); }
                    for (int k = 0; k < 2; ++k) {
                        O.score2_m[k] = R.score2_m[k];
                        mh::PeMateOut& M = O.mate[k];
                        M.off = b->offsets[2 * p + k] - b->offsets[0]; M.m = (uint32_t)(b->offsets[2 * p + k + 1] - b->offsets[2 * p + k]);
                        M.score = R.mate_score[k]; M.filled = O.finalized && R.filled[k]; M.orphan = R.orphan[k] != 0;
                        M.ref_pos = R.ref_pos[k]; M.as = R.as[k]; M.cig = ch.cig.data() + R.cigar_off[k]; M.n_cig = R.n_cigar[k];
                        const size_t a0 = k ? R.n_alt[0] : 0;
                        M.alt_pos = ap.data() + a0; M.alt_score = as.data() + a0; M.n_alt = R.n_alt[k];
                    }
                    if (O.finalized && R.tot >= (int32_t)(20 + 8 * log((double)O.mate[0].m)) + (int32_t)(20 + 8 * log((double)O.mate[1].m))) ++aligned[t];      // al.aligned: tot >= min_score
                    mh::pe_emit_fast(AL, *prm, O, (const char*)names + name_off[2 * p], (size_t)(name_off[2 * p + 1] - name_off[2 * p]), (const char*)names + name_off[2 * p + 1],
                                     (size_t)(name_off[2 * p + 2] - name_off[2 * p + 1]), base, qbase, dst);
                }
            });
            for (int t = 0; t < T; ++t) at[t + 1] = at[t] + piece[t].size();      // in order: chunk by chunk, thread share by thread share
            txt.pairs_upto = ch.lo + ch.n;
            char* dst = room(used + at[T] + 1);
            if (!dst) return MONI_ENOMEM;
            dst += used;
            pool.run([&](int t) { memcpy(dst + at[t], piece[t].data(), piece[t].size()); });
            used += at[T];
            chunk_pairs += ch.n;
            return MONI_OK;
        }, stats, &txt, resident, csv_out ? &csvq : nullptr);
        if (rc) return rc;
        if (csv_out) {
            // calculate_MEM_stats over the pair's MEMs (aligner_ksw2.hpp:1030-1031, 1115-1116, 1868-1902): the four find_mems calls and populate_seeds' halves are
            // the seeds of the two mates as the seeding kernels left them; the per-genome counts of a seed come from genome_kernel; the sums, the largest and the
            // smallest do not depend on the order of the list.  Then the line (include/common/csv.hpp:55-67) under mate 1's name as remove_slash_mate leaves it.
            std::vector<moni_mem_t> gm(c->n_mems + 1); std::vector<uint64_t> go(c->n_occs + 1), rmo(c->n_reads + 1), hl;
            if ((rc = moni_seed_fetch(c, gm.data(), go.data(), rmo.data())) || (rc = genome_hi_lo(c, *prm, hl))) return rc;
            csv_out->clear();
            char buf[256];
            for (uint64_t p = 0; p < NP_all; ++p) {
                size_t num_uniq_mems = 0, total_mem_occ = 0, high_occ_mem = 0, low_occ_mem = 0, num_mems_filter = 0;
                double max_mem_freq = 0, min_mem_freq = 1;
                const uint64_t a = rmo[2 * p], e = rmo[2 * p + 2];
                num_uniq_mems = (size_t)(e - a);
                for (uint64_t k = a; k < e; ++k) { total_mem_occ += gm[k].total_occ; num_mems_filter += gm[k].num_filtered; }
                for (uint64_t k = a; k < e; ++k) {
                    const double mem_freq = (gm[k].occ_cnt / (static_cast<double>(total_mem_occ)));
                    max_mem_freq = (max_mem_freq > mem_freq ? max_mem_freq : mem_freq);
                    min_mem_freq = (min_mem_freq > mem_freq ? mem_freq : min_mem_freq);
                    const size_t hi = (size_t)(hl[k] & 0xFFFFFFFFull), lo = (size_t)(hl[k] >> 32);
                    if (hi) {
                        if (high_occ_mem == 0 && low_occ_mem == 0) { high_occ_mem = hi; low_occ_mem = lo; }
                        else { high_occ_mem = (high_occ_mem > hi ? high_occ_mem : hi); low_occ_mem = (low_occ_mem > lo ? lo : low_occ_mem); }
                    }
                }
                num_mems_filter += (size_t)csvq.filter[p];
                size_t nl = (size_t)(name_off[2 * p + 1] - name_off[2 * p]);
                const char* nm = (const char*)names + name_off[2 * p];
                if (nl >= 2 && nm[nl - 2] == '/' && (nm[nl - 1] == '1' || nm[nl - 1] == '2')) nl -= 2;      // remove_slash_mate
                csv_out->append(nm, nl);
                snprintf(buf, sizeof buf, ",%zu,%zu,%f,%f,%zu,%zu,%zu,%zu\n", num_uniq_mems, total_mem_occ, max_mem_freq, min_mem_freq, high_occ_mem, low_occ_mem, num_mems_filter, (size_t)csvq.skipped[p]);
                *csv_out += buf;
            }
        }
        char* out = room(used + 1);
        if (!out) return MONI_ENOMEM;
        out[used] = 0;
        if (own_buf) { *sam = out; *sam_len = used; }
        else {
            char* cp = (char*)malloc(used + 1);
            if (!cp) return MONI_ENOMEM;
            const size_t per = (used + (size_t)T) / (size_t)T;
            pool.run([&](int t) { const size_t lo = std::min(used, per * (size_t)t), hi = std::min(used, lo + per); memcpy(cp + lo, out + lo, hi - lo); });
            cp[used] = 0;
            *sam = cp; *sam_len = used;
        }
        if (stats) { for (int t = 0; t < T; ++t) stats->aligned += aligned[t]; stats->aligned += txt.aligned; }
        if (getenv("MONI_AK_PROFILE")) fprintf(stderr, "  paired batch: %.1f ms in all (seeding %.1f, waiting for kernels and copies %.1f, host finishing %.1f); lines of %llu chunks written by the kernels, of %llu by the host\n",
                                               (mh::now_s() - w0) * 1e3, stats ? stats->t_seed * 1e3 : 0.0, stats ? stats->t_dp * 1e3 : 0.0, stats ? stats->t_host * 1e3 : 0.0,
                                               (unsigned long long)txt.chunks_gpu, (unsigned long long)txt.chunks_host);
        (void)over; (void)chunk_pairs;
        return MONI_OK;
    } catch (const std::bad_alloc&) { return MONI_ENOMEM; }
}

int moni_pe_align_batch(moni_ctx_t* c, const moni_read_batch_t* b, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals,
                        const moni_align_params_t* prm, const moni_pe_params_t* pe, const moni_pe_model_t* model, char** sam, uint64_t* sam_len,
                        moni_align_stats_t* stats) {
    return pe_align_text(c, b, names, name_off, quals, prm, pe, model, sam, sam_len, stats, false);
}
int moni_pe_align_stream(moni_ctx_t* c, const moni_read_batch_t* b, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals,
                         const moni_align_params_t* prm, const moni_pe_params_t* pe, const moni_pe_model_t* model, char** sam, uint64_t* sam_len,
                         moni_align_stats_t* stats) {
    return pe_align_text(c, b, names, name_off, quals, prm, pe, model, sam, sam_len, stats, true);
}

// aligner::align(kpbseq_t*, out, csv_out) with csv (-c for pairs; aligner_ksw2.hpp:888-918, 1030-1031, 1066-1075, 1115-1118, 1354-1358; include/common/csv.hpp:26-67)
int moni_pe_align_csv_batch(moni_ctx_t* c, const moni_read_batch_t* b, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals,
                            const moni_align_params_t* prm, const moni_pe_params_t* pe, const moni_pe_model_t* model, char** sam, uint64_t* sam_len,
                            char** csv, uint64_t* csv_len, moni_align_stats_t* stats) {
    if (!csv || !csv_len) return MONI_EINVAL;
    try {
        std::string lines;
        const int rc = pe_align_text(c, b, names, name_off, quals, prm, pe, model, sam, sam_len, stats, false, false, &lines);
        if (rc) return rc;
        char* d = (char*)malloc(lines.size() + 1);
        if (!d) { free(*sam); *sam = nullptr; return MONI_ENOMEM; }
        memcpy(d, lines.data(), lines.size()); d[lines.size()] = 0;
        *csv = d; *csv_len = lines.size();
        return MONI_OK;
    } catch (const std::bad_alloc&) { return MONI_ENOMEM; }
}

int moni_pe_align_run(moni_ctx_t* c, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals, const moni_align_params_t* prm, const moni_pe_params_t* pe,
                      const moni_pe_model_t* model, char** sam, uint64_t* sam_len, moni_align_stats_t* stats) {
    if (!c || (c->n_reads & 1)) return MONI_EINVAL;
    if (c->h_offs.size() != c->n_reads + 1) return MONI_EINVAL;          // no batch resident (moni_reads_upload first)
    const moni_read_batch_t view{c->h_seq.data(), c->h_offs.data(), c->n_reads};      // the host copy moni_reads_upload keeps: what a chunk the host finishes is formatted from
    return pe_align_text(c, &view, names, name_off, quals, prm, pe, model, sam, sam_len, stats, true, true);
}

// aligner::align(paired_alignment_t&) with report_mems (-m for pairs; aligner_ksw2.hpp:1118-1180): after the four find_mems calls, populate_seeds
// without the halves, the direction filter and the frequency filter, one secondary record per occurrence of every MEM that is left, under its mate's name
// (remove_slash_mate), SEQ / QUAL = the MEM's part of the mate (of its reverse complement for the other strand).  The fragment model plays no part.
int moni_pe_report_mems_batch(moni_ctx_t* c, const moni_read_batch_t* b, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals,
                              const moni_align_params_t* prm, const moni_pe_params_t* pe, char** sam, uint64_t* sam_len) {
    if (!c || !b || !prm || !pe || !sam || !sam_len || (b->n_reads & 1) || (b->n_reads && (!names || !name_off))) return MONI_EINVAL;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    moni_seed_params_t sp;
    sp.min_len = prm->min_len; sp.filter_seeds = prm->filter_seeds; sp.n_seeds_thr = prm->n_seeds_thr; sp.report_mems = 1;
    if ((rc = seed_run_align(c, &sp))) return rc;
    try {
        std::vector<moni_mem_t> mems(c->n_mems); std::vector<uint64_t> occs(c->n_occs), rmo(c->n_reads + 1);
        if ((rc = moni_seed_fetch(c, mems.data(), occs.data(), rmo.data()))) return rc;
        const mh::HostIndex& ix = c->idx->hix;
        std::string out;
        char num[32];
        std::vector<const moni_mem_t*> list;
        for (uint64_t p = 0; p < c->n_reads / 2; ++p) {
            const uint64_t r[2] = {2 * p, 2 * p + 1};
            // the calls in the reference's order (aligner_ksw2.hpp:1012-1040, 1104-1109): (mate, strand bit of the seeds)
            const int c_read[4] = {0, pe->filter_dir ? 1 : 0, 1, pe->filter_dir ? 0 : 1};
            const uint32_t c_rc[4] = {0u, 2u, 0u, 2u};
            list.clear();
            size_t n_dir1 = 0, n_dir2 = 0;
            for (int k = 0; k < 4; ++k)
                for (uint64_t g = rmo[r[c_read[k]]]; g < rmo[r[c_read[k]] + 1]; ++g) if (mems[g].mate == c_rc[k]) { list.push_back(&mems[g]); if (k < 2) ++n_dir1; else ++n_dir2; }
            size_t lo = 0, hi = list.size();
            if (pe->filter_dir) {                                    // aligner_ksw2.hpp:1042-1100: the two plain averages decide
                double a1 = 0.0, a2 = 0.0;
                for (size_t i = 0; i < n_dir1; ++i) a1 += (double)list[i]->len;
                for (size_t i = n_dir1; i < list.size(); ++i) a2 += (double)list[i]->len;
                if (n_dir1 > 0) a1 = a1 / (double)n_dir1;
                if (n_dir2 > 0) a2 = a2 / (double)n_dir2;
                if (a1 > a2 && (a1 - a2) > pe->dir_thr) hi = n_dir1;
                if (a2 > a1 && (a2 - a1) > pe->dir_thr) lo = n_dir1;
            }
            size_t total = 0;
            for (size_t i = lo; i < hi; ++i) total += list[i]->occ_cnt;
            for (size_t i = lo; i < hi; ++i) {
                const moni_mem_t& M = *list[i];
                if (prm->filter_freq) { const double fr = static_cast<double>(M.occ_cnt) / total; if (fr > prm->freq_thr) continue; }      // seed_freq_filter
                const uint64_t rd = M.read;                          // the mate the seeding kernels found it in
                const uint64_t off = b->offsets[rd], m = b->offsets[rd + 1] - off;
                const bool rc_strand = (M.mate & 2) != 0;
                size_t nl = (size_t)(name_off[rd + 1] - name_off[rd]);
                const char* nm = (const char*)names + name_off[rd];
                if (nl >= 2 && nm[nl - 2] == '/' && (nm[nl - 1] == '1' || nm[nl - 1] == '2')) nl -= 2;      // remove_slash_mate
                std::string seq(M.len, 'N'), ql;
                for (uint32_t x = 0; x < M.len; ++x) seq[x] = rc_strand ? (char)mh::compl_of(b->seq[off + m - 1 - (M.idx + x)]) : (char)b->seq[off + M.idx + x];
                if (quals) { ql.resize(M.len); for (uint32_t x = 0; x < M.len; ++x) ql[x] = rc_strand ? (char)quals[off + m - 1 - (M.idx + x)] : (char)quals[off + M.idx + x]; }
                for (uint32_t j = 0; j < M.occ_cnt; ++j) {
                    const auto ref = ix.index(occs[M.occ_off + j]);
                    out.append(nm, nl);
                    out += rc_strand ? "\t272\t" : "\t256\t";
                    out += ix.names[ref.first]; out.push_back('\t');
                    snprintf(num, sizeof num, "%d", (int)(ref.second + 1)); out += num;
                    out += "\t255\t"; snprintf(num, sizeof num, "%d", (int)M.len); out += num; out += "M\t*\t0\t0\t";
                    out += seq; out.push_back('\t');
                    if (quals) out += ql; else out.push_back('*');
                    out += "\tAS:i:0\tNM:i:0\tMD:Z:\tOA:Z:*,0,"; out += rc_strand ? "-" : "+"; out += ",*,255,0;\tAA:Z:\n";
                }
            }
        }
        char* dst = (char*)malloc(out.size() + 1);
        if (!dst) return MONI_ENOMEM;
        memcpy(dst, out.data(), out.size()); dst[out.size()] = 0;
        *sam = dst; *sam_len = out.size();
        return MONI_OK;
    } catch (const std::bad_alloc&) { return MONI_ENOMEM; }
}
