// Host side of extend mode (included inside extern "C" of moni_hip.hip): the kernels are in extend_kernels.hip.
// The resident batch is taken in chunks of reads; per chunk: extend_plan_kernel, extend_dp_kernel over the device-resident task list,
// extend_finish_kernel, a scan of the line lengths, gather_lines_kernel, one transfer of the chunk's block into the context's text buffer.

void moni_extend_params_default(moni_extend_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_len = 25; p->ext_len = 100;
    p->smatch = 2; p->smismatch = 4; p->gapo = 4; p->gape = 2;
    p->end_bonus = 400; p->w = -1; p->zdrop = -1;
}

// DP over a task list that a kernel wrote (the device-list entry beside dp_run): tasks, their direction / CIGAR offsets and their count stay
// in HBM, operands are named by position (DP_Q_READS over `reads`, DP_T_TEXT over the index text).  t_max: the longest target of the list.
static int dp_run_device(moni_ctx* c, const moni_extend_params_t* prm, const uint8_t* reads, const moni_dp_task_t* tasks, const uint64_t* dir_off,
                         const uint64_t* cig_off, const unsigned long long* n_tasks, uint64_t task_cap, uint32_t t_max, uint8_t* dirs, uint32_t* cig,
                         moni_dp_result_t* results) {
    if (t_max > EXT_MAX_TLEN) return MONI_ERANGE;
    dp_launch_t P;
    memset(&P, 0, sizeof P);
    P.tasks = tasks; P.dir_off = dir_off; P.cig_off = cig_off; P.dirs = dirs; P.cig_tmp = cig; P.results = results;
    // ksw_gen_simple_mat(5, mat, smatch, -smismatch) (extender_ksw2.hpp:174, 579-592): a wildcard on either side scores 0, which extz_wave takes as -gape
    P.sc_mch = prm->smatch < 0 ? -prm->smatch : prm->smatch; P.sc_mis = prm->smismatch > 0 ? -prm->smismatch : prm->smismatch; P.sc_N = -prm->gape;
    P.wild = 4; P.qo = prm->gapo; P.e = prm->gape; P.end_bonus = prm->end_bonus;
    P.reads = reads; P.text = c->idx->d_text.p; P.n_text = c->idx->K.n_text;
    const unsigned grid = (unsigned)std::min<uint64_t>(task_cap, (uint64_t)ctx_n_cu(c) * 32);
    if (!grid) return MONI_OK;
    if (t_max <= 64) hipLaunchKernelGGL(extend_dp_kernel<1>, dim3(grid), dim3(64), 0, c->stream, P, n_tasks, task_cap);
    else if (t_max <= 128) hipLaunchKernelGGL(extend_dp_kernel<2>, dim3(grid), dim3(64), 0, c->stream, P, n_tasks, task_cap);
    else if (t_max <= 256) hipLaunchKernelGGL(extend_dp_kernel<4>, dim3(grid), dim3(64), 0, c->stream, P, n_tasks, task_cap);
    else hipLaunchKernelGGL(extend_dp_kernel<8>, dim3(grid), dim3(64), 0, c->stream, P, n_tasks, task_cap);
    return MONI_OK;
}

static int ex_out_reserve(moni_ctx* c, size_t used, size_t need) {          // the context's pinned text buffer, its first `used` bytes kept
    return need <= c->out_buf.cap ? MONI_OK : c->out_buf.ensure_keep(need + need / 2 + 4096, used);
}

static int extend_core(moni_ctx* c, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals, const moni_extend_params_t* prm,
                       uint64_t* sam_len, moni_extend_stats_t* stats) {
    moni_index* I = c->idx;
    const uint64_t nr = c->n_reads, total = c->total_len;
    *sam_len = 0;
    if (stats) { memset(stats, 0, sizeof *stats); stats->reads = nr; }
    if (prm->ext_len == 0 || prm->ext_len > EXT_MAX_TLEN) return MONI_ERANGE;
    if (prm->zdrop >= 0 || prm->w >= 0) return MONI_EINVAL;          // the reference's extender passes w = -1, zdrop = -1 (extender_ksw2.hpp:97-98); only that is implemented
    if (prm->gapo < 0 || prm->gape < 0) return MONI_EINVAL;
    {   // ksw2 returns with ez just reset when the mismatch penalty exceeds 2 (q + e): no traceback to stitch
        const int mis = prm->smismatch < 0 ? -prm->smismatch : prm->smismatch;
        if (mis > 2 * (prm->gapo + prm->gape)) return MONI_EINVAL;
    }
    if (!nr) return MONI_OK;
    if (!name_off || (name_off[nr] > name_off[0] && !names)) return MONI_EINVAL;
    if (c->max_len > EXT_MAX_READ) return MONI_ERANGE;
    if (c->h_offs.size() != nr + 1) return MONI_EINVAL;          // (a batch made resident by moni_reads_upload keeps its offsets on the host)
    HIPCHK(hipSetDevice(I->device));
    auto& B = c->ex;
    int rc;
    if (!B.tables.p) {          // the index tables with extend's complement (ext_complement) for pack_kernel
        DBuf<moni_tables_t> t;
        if ((rc = t.alloc_exact(1))) return rc;
        uint8_t tab[256];
        for (int b = 0; b < 256; ++b) tab[b] = ext_complement((uint8_t)b);
        if (hipMemcpy(t.p, I->d_tables.p, sizeof(moni_tables_t), hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy(reinterpret_cast<uint8_t*>(t.p) + offsetof(moni_tables_t, compl_tab), tab, 256, hipMemcpyHostToDevice) != hipSuccess) return MONI_ENODEV;
        B.tables = std::move(t);
    }
    HIPCHK(hipMemsetAsync(c->d_counters.p, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = ms_launch(c, B.tables.p))) return rc;
    // both strands' sequences in one buffer: DP queries and SEQ are read from it by position
    if ((rc = B.seq2.ensure(2 * total + 32))) return rc;
    HIPCHK(hipMemcpyAsync(B.seq2.p, c->seq.p, total, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemsetAsync(B.seq2.p + 2 * total, 0, 32, c->stream));
    hipLaunchKernelGGL(extend_rc_kernel, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, c->stream, c->seq.p, c->offs.p, nr, B.seq2.p + total);
    // names, qualities, the threshold per read length
    const uint64_t name_bytes = name_off[nr] - name_off[0];
    uint64_t name_max = 0;
    std::vector<uint64_t> noff(nr + 1);
    for (uint64_t i = 0; i <= nr; ++i) {
        if (i && name_off[i] < name_off[i - 1]) return MONI_EINVAL;
        noff[i] = name_off[i] - name_off[0];
        if (i) name_max = std::max(name_max, name_off[i] - name_off[i - 1]);
    }
    std::vector<int32_t> msc(c->max_len + 1, 0);
    for (uint64_t L = 1; L <= c->max_len; ++L) msc[L] = (int32_t)(20 + 8 * log((double)L));          // extender_ksw2.hpp:222
    if ((rc = B.rnames.ensure(name_bytes + 8)) || (rc = B.rname_off.ensure(nr + 1)) || (rc = B.minscore.ensure(msc.size())) || (quals && (rc = B.quals.ensure(total + 8))) ||
        (rc = B.cur.ensure(EXC_N)) || (rc = B.hcur.ensure(EXC_N)))
        return rc;
    if (name_bytes) HIPCHK(hipMemcpyAsync(B.rnames.p, names + name_off[0], name_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(B.rname_off.p, noff.data(), (nr + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(B.minscore.p, msc.data(), msc.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (quals && total) HIPCHK(hipMemcpyAsync(B.quals.p, quals, total, hipMemcpyHostToDevice, c->stream));
    // chunks of reads: MONI_EXTEND_CHUNK reads at most, fewer where long reads would need more than DIR_CAP direction bytes.  Per (read, strand) the
    // two queries have at most L bases together and each target at most E: direction bytes <= (L + 2 E) E, CIGAR slots <= L + 2 E + 4.
    uint64_t chunk = 16384;
    if (const char* v = getenv("MONI_EXTEND_CHUNK")) { const uint64_t x = strtoull(v, nullptr, 10); if (x) chunk = x; }
    const uint64_t E = prm->ext_len, DIR_CAP = 2ull << 30;
    const std::vector<uint64_t>& ho = c->h_offs;
    std::vector<uint64_t> cuts(1, 0);
    uint64_t dir_cap = 0, cig_cap = 0, chunk_max = 0;
    {
        uint64_t d = 0, g = 0;
        for (uint64_t r = 0; r < nr; ++r) {
            const uint64_t L = ho[r + 1] - ho[r], dr = 2 * (L + 2 * E) * E, gr = 2 * (L + 2 * E + 4);
            if (r > cuts.back() && (r - cuts.back() == chunk || d + dr > DIR_CAP)) { cuts.push_back(r); d = g = 0; }
            d += dr; g += gr;
            dir_cap = std::max(dir_cap, d); cig_cap = std::max(cig_cap, g); chunk_max = std::max(chunk_max, r + 1 - cuts.back());
        }
        cuts.push_back(nr);
    }
    const uint64_t task_cap = 4 * chunk_max, n_rec = 2 * chunk_max;
    const uint64_t slot = (name_max + EXT_HEAD + 2 * c->max_len + 2 + EXT_TAIL + 7) & ~7ull;
    if ((rc = B.plans.ensure(n_rec)) || (rc = B.tasks.ensure(task_cap)) || (rc = B.dir_off.ensure(task_cap)) || (rc = B.cig_off.ensure(task_cap)) || (rc = B.res.ensure(task_cap)) ||
        (rc = B.dirs.ensure(dir_cap + 16)) || (rc = B.cig.ensure(cig_cap + 16)) || (rc = B.lines.ensure(n_rec * slot + 8)) || (rc = B.block.ensure(n_rec * slot + 8)) ||
        (rc = B.len.ensure(n_rec + 1)) || (rc = B.off.ensure(n_rec + 1)) || (rc = B.pos.ensure(n_rec + 1)))
        return rc;
    ext_args_t X;
    memset(&X, 0, sizeof X);
    X.K = I->K; X.text = I->d_text.p; X.pat = c->pat.p; X.offs = c->offs.p; X.blk = c->blk.p; X.ptr = c->ptr.p;
    X.seq2 = B.seq2.p; X.total_len = total;
    X.min_len = prm->min_len; X.ext_len = prm->ext_len; X.smatch = prm->smatch < 0 ? -prm->smatch : prm->smatch;
    X.plans = B.plans.p; X.tasks = B.tasks.p; X.dir_off = B.dir_off.p; X.cig_off = B.cig_off.p; X.cur = B.cur.p;
    X.task_cap = task_cap; X.dir_cap = dir_cap; X.cig_cap = cig_cap;
    X.res = B.res.p; X.cig = B.cig.p; X.min_score_of_len = B.minscore.p;
    X.seq_starts = I->d_seq_starts.p; X.snames = I->d_snames.p; X.sname_off = I->d_sname_off.p; X.n_seq = I->K.n_seq;
    X.rnames = B.rnames.p; X.rname_off = B.rname_off.p; X.quals = quals ? B.quals.p : nullptr;
    X.lines = B.lines.p; X.slot = slot; X.len = B.len.p; X.off = B.off.p;
    const int n_cu = ctx_n_cu(c);
    uint64_t used = 0;
    double k_ms = 0;
    bool first = true;
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const uint64_t r0 = cuts[k], nc = cuts[k + 1] - r0;
        if (!nc) continue;
        X.read_lo = r0; X.n_reads = nc;
        HIPCHK(hipMemsetAsync(B.cur.p, 0, EXC_N * sizeof(unsigned long long), c->stream));
        rec(c, EV_DP0);
        hipLaunchKernelGGL(extend_plan_kernel, dim3((unsigned)((2 * nc + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, X);
        if ((rc = dp_run_device(c, prm, B.seq2.p, B.tasks.p, B.dir_off.p, B.cig_off.p, B.cur.p + EXC_TASKS, 4 * nc, prm->ext_len, B.dirs.p, B.cig.p, B.res.p))) return rc;
        hipLaunchKernelGGL(extend_finish_kernel, dim3((unsigned)std::min<uint64_t>(nc, (uint64_t)n_cu * 16)), dim3(64), 0, c->stream, X);
        if ((rc = exclusive_scan_u64(c, B.len.p, B.pos.p, 2 * nc))) return rc;
        hipLaunchKernelGGL(gather_lines_kernel, dim3((unsigned)std::min<uint64_t>((2 * nc + 3) / 4, (uint64_t)n_cu * 8)), dim3(256), 0, c->stream, (const uint64_t*)B.lines.p,
                           (const uint64_t*)B.len.p, (const uint64_t*)B.off.p, (const uint64_t*)B.pos.p, 2 * nc, B.block.p);
        rec(c, EV_DP1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(B.hcur.p, B.cur.p, EXC_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        { float ms = 0; if (hipEventElapsedTime(&ms, c->ev[EV_DP0], c->ev[EV_DP1]) == hipSuccess) k_ms += ms; }
        if (first) { float ms = 0; if (hipEventElapsedTime(&ms, c->ev[EV_MS0], c->ev[EV_MS1]) == hipSuccess) k_ms += ms; first = false; }
        const unsigned long long* h = B.hcur.p;
        if (h[EXC_ERR]) return MONI_ERANGE;          // a line or a CIGAR beyond the staging, or a list beyond its capacity: nothing was written out of bounds
        const uint64_t bytes = h[EXC_BYTES];
        if ((rc = ex_out_reserve(c, used, used + bytes + 1))) return rc;
        if (bytes) HIPCHK(hipMemcpy(c->out_buf.p + used, B.block.p, bytes, hipMemcpyDeviceToHost));
        used += bytes;
        if (stats) { stats->records += h[EXC_RECORDS]; stats->extended += h[EXC_EXTENDED]; stats->dp_tasks += h[EXC_TASKS]; stats->dp_cells += h[EXC_CELLS]; }
    }
    if ((rc = ex_out_reserve(c, used, used + 1))) return rc;
    c->out_buf.p[used] = 0;
    if (stats) stats->t_kernel = k_ms * 1e-3;
    *sam_len = used;
    return MONI_OK;
}

int moni_extend_run(moni_ctx_t* c, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals, const moni_extend_params_t* prm,
                    char** sam, uint64_t* sam_len, moni_extend_stats_t* stats) {
    if (!c || !prm || !sam || !sam_len) return MONI_EINVAL;
    *sam = nullptr;
    try {
        const int rc = extend_core(c, names, name_off, quals, prm, sam_len, stats);
        if (rc) { *sam_len = 0; return rc; }
    } catch (const std::bad_alloc&) { *sam_len = 0; return MONI_ENOMEM; }
    *sam = c->out_buf.p;
    return MONI_OK;
}

int moni_extend_batch(moni_ctx_t* c, const moni_read_batch_t* b, const uint8_t* names, const uint64_t* name_off, const uint8_t* quals,
                      const moni_extend_params_t* prm, char** sam, uint64_t* sam_len, moni_extend_stats_t* stats) {
    if (!c || !b || !prm || !sam || !sam_len) return MONI_EINVAL;
    *sam = nullptr; *sam_len = 0;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    char* txt = nullptr; uint64_t len = 0;
    if ((rc = moni_extend_run(c, names, name_off, quals ? quals + b->offsets[0] : nullptr, prm, &txt, &len, stats))) return rc;
    char* out = (char*)malloc(len + 1);
    if (!out) return MONI_ENOMEM;
    if (len) memcpy(out, txt, len);
    out[len] = 0;
    *sam = out; *sam_len = len;
    return MONI_OK;
}
