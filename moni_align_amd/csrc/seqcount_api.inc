// Host side of the sequence-count query (included inside extern "C" of moni_hip.hip): the kernels are in seqcount_kernels.hip.
// One run = pack_kernel + count_kernel (max_occ 0: the search alone), then seqcount_plan_kernel, the rocPRIM exclusive scan of the segment counts,
// one 8-byte copy of their total, the memset of the table, seqcount_walk_kernel (where there is a segment) and seqcount_finish_kernel; the results
// stay on the device until fetched.  The walk finds a segment's task by a binary search over the scan, so the segments themselves are never stored.

void moni_seqcount_params_default(moni_seqcount_params_t* p) {
    if (!p) return;
    p->strands = 1; p->reserved = 0; p->max_walk = 1ull << 20;
}

static int seqcount_params_ok(const moni_seqcount_params_t* p) { return p && (p->strands == 1 || p->strands == 2) && !p->reserved; }

#define SC_MAX_GRID (1u << 20)          // blocks of the walk's grid; it strides over the segments beyond

static int seqcount_run_resident(moni_ctx* c, const moni_seqcount_params_t* prm) {
    moni_index* I = c->idx;
    SearchDims D; int rc;
    if ((rc = search_dims(c, prm->strands, D))) return rc;
    auto& B = c->sc;
    B.valid = false;
    const uint64_t nr = D.nr, n_tasks = D.n_tasks, n_seq = I->K.n_seq;
    const unsigned task_grid = D.task_grid;
    if (n_seq && n_tasks > (~0ull >> 4) / n_seq) return MONI_ENOMEM;          // the table's size in bytes does not fit 60 bits
    const uint64_t n_cells = n_tasks * n_seq;
    if ((rc = B.s.ensure(n_tasks)) || (rc = B.res.ensure(n_tasks + 1)) || (rc = B.k_lo.ensure(n_tasks + 1)) || (rc = B.counts.ensure(n_cells + 1))) return refused(rc);
    if ((rc = search_pack(c, D)) || (rc = search_count(c, D, prm->strands, 0u, B.s))) return rc;
    rec(c, EV_PC0);
    uint64_t total = 0;
    if (nr) {
        hipLaunchKernelGGL(seqcount_plan_kernel, dim3(task_grid), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_rows.p, n_tasks, prm->max_walk, B.s.res.p, B.res.p, B.k_lo.p, B.s.cnt.p);
        HIPCHK(hipGetLastError());
        if ((rc = exclusive_scan_u64(c, B.s.cnt.p, B.s.off.p, n_tasks + 1))) return rc;
        HIPCHK(hipMemcpyAsync(&total, B.s.off.p + n_tasks, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (n_cells) HIPCHK(hipMemsetAsync(B.counts.p, 0, n_cells * sizeof(uint64_t), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (total) {          // no segment: no walk launch, and every n_seqs stays 0
        phi_tab_t P; P.recs = I->d_phi.p; P.dir = I->d_phi_dir.p;
        const uint64_t blocks = (total + MS_BLOCK - 1) / MS_BLOCK;
        hipLaunchKernelGGL(seqcount_walk_kernel, dim3((unsigned)std::min<uint64_t>(blocks, SC_MAX_GRID)), dim3(MS_BLOCK), 0, c->stream, I->K, P, I->d_rows.p, I->d_cr.p, I->d_recs.p,
                           I->d_seq_starts.p, n_tasks, total, B.res.p, B.s.toe.p, B.k_lo.p, B.s.off.p, (unsigned long long*)B.counts.p, c->d_counters.p);
        hipLaunchKernelGGL(seqcount_finish_kernel, dim3((unsigned)((n_tasks + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, (uint32_t)n_seq, n_tasks,
                           (const unsigned long long*)B.counts.p, B.res.p);
    }
    rec(c, EV_PC1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    B.n_tasks = n_tasks; B.n_seq = (uint32_t)n_seq; B.n_segs = total; B.valid = true;
    return MONI_OK;
}

int moni_seqcount_run(moni_ctx_t* c, const moni_seqcount_params_t* prm) {
    if (!c || !seqcount_params_ok(prm)) return MONI_EINVAL;
    return seqcount_run_resident(c, prm);
}

int moni_seqcount_sizes(moni_ctx_t* c, uint64_t* n_tasks, uint32_t* n_seq) {
    if (!c || !c->sc.valid) return MONI_EINVAL;
    if (n_tasks) *n_tasks = c->sc.n_tasks;
    if (n_seq) *n_seq = c->sc.n_seq;
    return MONI_OK;
}

int moni_seqcount_fetch(moni_ctx_t* c, moni_seqcount_res_t* res, uint64_t* counts) {
    if (!c || !c->sc.valid) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    const auto& B = c->sc;
    if (res && B.n_tasks) HIPCHK(hipMemcpy(res, B.res.p, B.n_tasks * sizeof(moni_seqcount_res_t), hipMemcpyDeviceToHost));
    if (counts && B.n_tasks && B.n_seq) HIPCHK(hipMemcpy(counts, B.counts.p, B.n_tasks * B.n_seq * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MONI_OK;
}

int moni_seqcount_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_seqcount_params_t* prm, moni_seqcount_res_t* res, uint64_t* counts) {
    if (!c || !b || !seqcount_params_ok(prm)) return MONI_EINVAL;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    if (!b->n_reads) return MONI_OK;
    if ((rc = seqcount_run_resident(c, prm))) return rc;
    return moni_seqcount_fetch(c, res, counts);
}
