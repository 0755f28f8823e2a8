// Host side of matching statistics of long patterns (included inside extern "C" of moni_hip.hip): the kernels are in mslong_kernels.hip, the
// method in mslong_core.h.  One call = upload of the bytes and offsets (no step-major workspace is laid out: the call takes patterns
// moni_reads_upload refuses), segment table, speculative walk, length pass, and - where segments were flagged - the list of runs, the chain
// re-walk and its length pass.  The host reads back the number of segments, the number of runs and the counters.

void moni_mslong_params_default(moni_mslong_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->seg_len = 4096;          // placeholders until the table of DESIGN.md 7.7 (profiles/mslong_rate.py) is measured
    p->overlap = 256;
}

int moni_ms_long_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_mslong_params_t* prm, uint64_t* pointers, uint64_t* lengths, moni_mslong_stats_t* stats) {
    if (!c || !b || !prm || (!pointers && !lengths)) return MONI_EINVAL;
    if (prm->seg_len < 8 || prm->reserved[0] || prm->reserved[1]) return MONI_EINVAL;
    if (!b->offsets || (b->n_reads && !b->seq)) return MONI_EINVAL;
    const uint64_t nr = b->n_reads;
    if (nr >= 0xFFFFFFFFull) return MONI_ERANGE;
    for (uint64_t i = 0; i < nr; ++i) {
        if (b->offsets[i + 1] < b->offsets[i]) return MONI_EINVAL;
        if (b->offsets[i + 1] - b->offsets[i] > 0xFFFFFFFFull) return MONI_ERANGE;          // positions inside a pattern are 32-bit
    }
    moni_index* I = c->idx;
    if (I->K.n > (1ull << 39)) return MONI_ERANGE;          // mslong_core.h: a pointer waits for its group of 8 in 40 bits with a sign
    HIPCHK(hipSetDevice(I->device));
    const auto h0 = std::chrono::steady_clock::now();
    const uint64_t total = nr ? b->offsets[nr] - b->offsets[0] : 0;
    moni_mslong_stats_t st;
    memset(&st, 0, sizeof(st));
    st.patterns = nr; st.bases = total;
    // the resident batch is replaced by bytes and offsets alone: nothing of the other entry points can run on it
    c->n_reads = 0; c->total_len = 0; c->max_len = 0; c->h_blk.clear(); c->h_seq.clear(); c->h_offs.clear();
    c->n_mems = c->n_occs = 0; c->occs_valid = false; c->pml.valid = false; c->loc.valid = false; c->sc.valid = false; c->loci.valid = false;
    for (int e = 0; e < EV_N; ++e) c->ev_valid[e] = false;
    if (!total) { if (stats) *stats = st; return MONI_OK; }
    auto& B = c->msl;
    int rc;
    if ((rc = c->seq.ensure(total + 16)) || (rc = c->offs.ensure(nr + 1)) || (rc = B.ptr.ensure(total + 8)) || (rc = B.lens.ensure(total + 8)) || (rc = B.cnt.ensure(nr + 2)) ||
        (rc = B.seg_off.ensure(nr + 2)) || (rc = B.counters.ensure(8)))
        return rc;
    try {
        std::vector<uint64_t> rel(nr + 1);
        for (uint64_t i = 0; i <= nr; ++i) rel[i] = b->offsets[i] - b->offsets[0];
        HIPCHK(hipMemcpyAsync(c->seq.p, b->seq + b->offsets[0], total, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->offs.p, rel.data(), (nr + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    } catch (const std::bad_alloc&) { return MONI_ENOMEM; }
    HIPCHK(hipMemsetAsync(B.counters.p, 0, 8 * sizeof(unsigned long long), c->stream));
    rec(c, EV_ALL0);
    // segment table: a count per pattern, its exclusive scan, one lane per segment
    hipLaunchKernelGGL(mslong_count_kernel, dim3((unsigned)((nr + 1 + 255) / 256)), dim3(256), 0, c->stream, c->offs.p, nr, prm->seg_len, B.cnt.p);
    if ((rc = exclusive_scan_u64(c, B.cnt.p, B.seg_off.p, nr + 1))) return rc;
    uint64_t n_segs = 0;
    HIPCHK(hipMemcpyAsync(&n_segs, B.seg_off.p + nr, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_segs >= 0xFFFFFFFFull) return MONI_ERANGE;
    if ((rc = B.segs.ensure(n_segs + 1)) || (rc = B.flags.ensure(n_segs + 1)) || (rc = B.states.ensure(n_segs + 1)) || (rc = B.head.ensure(n_segs + 2)) || (rc = B.run_idx.ensure(n_segs + 2)))
        return rc;
    const unsigned g256 = (unsigned)((n_segs + 1 + 255) / 256), gseg = (unsigned)((n_segs + MS_BLOCK - 1) / MS_BLOCK);
    hipLaunchKernelGGL(mslong_table_kernel, dim3(g256), dim3(256), 0, c->stream, c->offs.p, B.seg_off.p, nr, n_segs, prm->seg_len, prm->overlap, B.segs.p, B.flags.p);
    rec(c, EV_MS0);
    hipLaunchKernelGGL(mslong_walk_kernel, dim3(gseg), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, I->d_rows.p, I->d_frows.p, I->d_cr.p, I->d_recs.p, c->seq.p, c->offs.p, B.segs.p, n_segs,
                       B.ptr.p, B.states.p, B.counters.p);
    rec(c, EV_MS1);
    rec(c, EV_MC0);
    hipLaunchKernelGGL(mslong_len_kernel, dim3(gseg), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_text.p, c->seq.p, c->offs.p, B.segs.p, n_segs, B.ptr.p, B.lens.p, B.flags.p, B.counters.p);
    rec(c, EV_MC1);
    // runs of flagged segments: heads, their exclusive scan, one entry per run
    hipLaunchKernelGGL(mslong_head_kernel, dim3(g256), dim3(256), 0, c->stream, B.flags.p, n_segs, B.head.p);
    if ((rc = exclusive_scan_u64(c, B.head.p, B.run_idx.p, n_segs + 1))) return rc;
    uint64_t n_runs = 0;
    HIPCHK(hipMemcpyAsync(&n_runs, B.run_idx.p + n_segs, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    rec(c, EV_ME0);
    if (n_runs) {
        if ((rc = B.runs.ensure(n_runs + 1))) return rc;
        const unsigned grun = (unsigned)((n_runs + MS_BLOCK - 1) / MS_BLOCK);
        hipLaunchKernelGGL(mslong_runs_kernel, dim3(g256), dim3(256), 0, c->stream, B.flags.p, n_segs, B.run_idx.p, B.runs.p);
        hipLaunchKernelGGL(mslong_chain_kernel, dim3(grun), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, I->d_rows.p, I->d_frows.p, I->d_cr.p, I->d_recs.p, c->seq.p, c->offs.p, B.segs.p, n_segs,
                           B.runs.p, n_runs, B.ptr.p, B.states.p, B.counters.p);
        hipLaunchKernelGGL(mslong_relen_kernel, dim3(grun), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_text.p, c->seq.p, c->offs.p, B.segs.p, B.runs.p, n_runs, B.ptr.p, B.lens.p);
    }
    rec(c, EV_ME1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    unsigned long long hc[8];
    HIPCHK(hipMemcpyAsync(hc, B.counters.p, sizeof(hc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (pointers) HIPCHK(hipMemcpy(pointers, B.ptr.p, total * 8, hipMemcpyDeviceToHost));
    if (lengths) {
        try {
            std::vector<uint32_t> hl(total);
            HIPCHK(hipMemcpy(hl.data(), B.lens.p, total * 4, hipMemcpyDeviceToHost));
            for (uint64_t k = 0; k < total; ++k) lengths[k] = hl[k];
        } catch (const std::bad_alloc&) { return MONI_ENOMEM; }
    }
    st.segments = n_segs; st.flagged = hc[3]; st.chain_runs = n_runs;
    st.steps_spec = hc[0]; st.steps_chain = hc[2]; st.jumps = hc[1];
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[EV_MS0], c->ev[EV_MS1]) == hipSuccess) st.t_walk = ms * 1e-3;
    if (hipEventElapsedTime(&ms, c->ev[EV_MC0], c->ev[EV_MC1]) == hipSuccess) st.t_len = ms * 1e-3;
    if (hipEventElapsedTime(&ms, c->ev[EV_ME0], c->ev[EV_ME1]) == hipSuccess) st.t_chain = ms * 1e-3;
    st.t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - h0).count();
    if (stats) *stats = st;
    return MONI_OK;
}
