// Host side of the loci query (included inside extern "C" of moni_hip.hip): the kernels are in loci_kernels.hip.
// One run = pack_kernel + count_kernel (max_occ 0: the search alone), seqcount_plan_kernel and the scan of the segment counts as in a seqcount run,
// loci_plan_kernel and the scan of the walked counts, one 16-byte copy of the two totals (they size the grid and the buffers and decide
// MONI_ENOMEM), loci_walk_kernel, the rocPRIM radix sort of the keys over the bits that can differ, loci_head_kernel, the scan of its flags, one
// 8-byte copy of the number of loci, loci_emit_kernel and loci_finish_kernel; the results stay on the device until fetched.
// Three buffers of walked-total words carry it: the walk's keys, the sorted keys, the scan.  The unsorted keys are dead after the sort: their
// buffer takes the head flags, and after the scan the head indices.

void moni_loci_params_default(moni_loci_params_t* p) {
    if (!p) return;
    p->strands = 1; p->lift = 1; p->max_walk = 1ull << 20; p->max_total = 1ull << 28; p->reserved[0] = p->reserved[1] = 0;
}

static int loci_params_ok(const moni_loci_params_t* p) { return p && (p->strands == 1 || p->strands == 2) && p->lift <= 1 && !p->reserved[0] && !p->reserved[1]; }

static int loci_sort(moni_ctx* c, uint64_t* in, uint64_t* out, uint64_t n, unsigned bits) {
    size_t tmp_bytes = 0;
    if (rocprim::radix_sort_keys(nullptr, tmp_bytes, in, out, (size_t)n, 0u, bits, c->stream) != hipSuccess) return MONI_ENODEV;
    int rc = c->loci.sort_tmp.ensure(tmp_bytes + 16);
    if (rc) return rc;
    if (rocprim::radix_sort_keys(c->loci.sort_tmp.p, tmp_bytes, in, out, (size_t)n, 0u, bits, c->stream) != hipSuccess) return MONI_ENODEV;
    return MONI_OK;
}

static int loci_run_resident(moni_ctx* c, const moni_loci_params_t* prm) {
    moni_index* I = c->idx;
    SearchDims D; int rc;
    if ((rc = search_dims(c, prm->strands, D))) return rc;
    auto& B = c->loci;
    B.valid = false;
    const uint64_t nr = D.nr, n_tasks = D.n_tasks;
    const unsigned task_grid = D.task_grid;
    if (n_tasks > LOCI_MAX_TASKS) return MONI_ERANGE;
    if ((rc = B.s.ensure(n_tasks)) || (rc = B.occ_off.ensure(n_tasks + 2)) || (rc = B.sres.ensure(n_tasks + 1)) || (rc = B.k_lo.ensure(n_tasks + 1)) || (rc = B.res.ensure(n_tasks + 1)))
        return refused(rc);
    if ((rc = search_pack(c, D)) || (rc = search_count(c, D, prm->strands, 0u, B.s))) return rc;
    rec(c, EV_PC0);
    uint64_t totals[2] = {0, 0};          // walked occurrences, segments
    if (nr) {
        hipLaunchKernelGGL(seqcount_plan_kernel, dim3(task_grid), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_rows.p, n_tasks, prm->max_walk, B.s.res.p, B.sres.p, B.k_lo.p, B.s.cnt.p);
        HIPCHK(hipGetLastError());
        if ((rc = exclusive_scan_u64(c, B.s.cnt.p, B.s.off.p, n_tasks + 1))) return rc;
        hipLaunchKernelGGL(loci_plan_kernel, dim3(task_grid), dim3(MS_BLOCK), 0, c->stream, n_tasks, B.sres.p, B.s.off.p, B.s.cnt.p, B.occ_off.p);
        HIPCHK(hipGetLastError());
        if ((rc = exclusive_scan_u64(c, B.s.cnt.p, B.occ_off.p, n_tasks + 1))) return rc;
        HIPCHK(hipMemcpyAsync(totals, B.occ_off.p + n_tasks, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    const uint64_t total = totals[0], n_segs = totals[1];
    if (prm->max_total && total > prm->max_total) return MONI_ENOMEM;          // nothing of the result was written
    if (total) {
        if ((rc = B.keys.ensure(total + 2)) || (rc = B.sorted.ensure(total + 2)) || (rc = B.idx.ensure(total + 2))) return refused(rc);
        phi_tab_t P; P.recs = I->d_phi.p; P.dir = I->d_phi_dir.p;
        loci_lift_t T; T.pdir = I->d_pdir.p; T.seqs = I->d_lift_seqs.p; T.runs = I->d_lift_runs.p; T.n_text = I->K.n - 1; T.n_seq = I->K.n_seq;
        const uint64_t blocks = (n_segs + MS_BLOCK - 1) / MS_BLOCK;
        hipLaunchKernelGGL(loci_walk_kernel, dim3((unsigned)std::min<uint64_t>(blocks, SC_MAX_GRID)), dim3(MS_BLOCK), 0, c->stream, I->K, P, T, I->d_rows.p, I->d_cr.p, I->d_recs.p,
                           n_tasks, n_segs, prm->lift, B.sres.p, B.s.toe.p, B.k_lo.p, B.s.off.p, B.occ_off.p, B.keys.p, c->d_counters.p);
        HIPCHK(hipGetLastError());
    }
    rec(c, EV_PC1);
    rec(c, EV_PE0);
    uint64_t n_loci = 0;
    if (total) {
        if ((rc = loci_sort(c, B.keys.p, B.sorted.p, total, loci_key_bits(n_tasks)))) return refused(rc);
        const unsigned key_grid = (unsigned)((total + 1 + MS_BLOCK - 1) / MS_BLOCK);
        hipLaunchKernelGGL(loci_head_kernel, dim3(key_grid), dim3(MS_BLOCK), 0, c->stream, B.sorted.p, total, B.keys.p);
        HIPCHK(hipGetLastError());
        if ((rc = exclusive_scan_u64(c, B.keys.p, B.idx.p, total + 1))) return rc;
        HIPCHK(hipMemcpyAsync(&n_loci, B.idx.p + total, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if ((rc = B.lpos.ensure(n_loci)) || (rc = B.lseq.ensure(n_loci)) || (rc = B.lseq_off.ensure(n_loci)) || (rc = B.support.ensure(n_loci))) return refused(rc);
        hipLaunchKernelGGL(loci_emit_kernel, dim3(key_grid), dim3(MS_BLOCK), 0, c->stream, B.sorted.p, total, B.idx.p, I->d_seq_starts.p, I->K.n_seq, B.lpos.p, B.lseq.p, B.lseq_off.p,
                           B.keys.p);
    }
    if (n_tasks)
        hipLaunchKernelGGL(loci_finish_kernel, dim3((unsigned)((std::max(n_tasks, n_loci) + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, n_tasks, n_loci, B.sres.p, B.occ_off.p,
                           total ? B.idx.p : nullptr, B.keys.p, B.support.p, B.res.p);
    rec(c, EV_PE1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    B.n_tasks = n_tasks; B.n_loci = n_loci; B.n_segs = n_segs; B.valid = true;
    return MONI_OK;
}

int moni_loci_run(moni_ctx_t* c, const moni_loci_params_t* prm) {
    if (!c || !loci_params_ok(prm)) return MONI_EINVAL;
    return loci_run_resident(c, prm);
}

int moni_loci_sizes(moni_ctx_t* c, uint64_t* n_tasks, uint64_t* n_loci) {
    if (!c || !c->loci.valid) return MONI_EINVAL;
    if (n_tasks) *n_tasks = c->loci.n_tasks;
    if (n_loci) *n_loci = c->loci.n_loci;
    return MONI_OK;
}

int moni_loci_fetch(moni_ctx_t* c, moni_loci_res_t* res, uint64_t* lpos, uint32_t* lseq, uint64_t* lseq_off, uint64_t* support) {
    if (!c || !c->loci.valid) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    const auto& B = c->loci;
    if (res && B.n_tasks) HIPCHK(hipMemcpy(res, B.res.p, B.n_tasks * sizeof(moni_loci_res_t), hipMemcpyDeviceToHost));
    if (lpos && B.n_loci) HIPCHK(hipMemcpy(lpos, B.lpos.p, B.n_loci * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (lseq && B.n_loci) HIPCHK(hipMemcpy(lseq, B.lseq.p, B.n_loci * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (lseq_off && B.n_loci) HIPCHK(hipMemcpy(lseq_off, B.lseq_off.p, B.n_loci * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (support && B.n_loci) HIPCHK(hipMemcpy(support, B.support.p, B.n_loci * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MONI_OK;
}

int moni_loci_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_loci_params_t* prm, moni_loci_res_t* res, uint64_t** lpos, uint32_t** lseq,
                    uint64_t** lseq_off, uint64_t** support, uint64_t* n_loci) {
    if (!c || !b || !loci_params_ok(prm)) return MONI_EINVAL;
    if (lpos) *lpos = nullptr;
    if (lseq) *lseq = nullptr;
    if (lseq_off) *lseq_off = nullptr;
    if (support) *support = nullptr;
    if (n_loci) *n_loci = 0;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    if (!b->n_reads) return MONI_OK;
    if ((rc = loci_run_resident(c, prm))) return rc;
    const uint64_t n = c->loci.n_loci;
    HostArrays H;
    uint64_t* hp = H.want(lpos, n); uint32_t* hs = H.want(lseq, n); uint64_t* ho = H.want(lseq_off, n); uint64_t* hu = H.want(support, n);
    if (!H.ok) return MONI_ENOMEM;
    if ((rc = moni_loci_fetch(c, res, hp, hs, ho, hu))) return rc;
    H.release();
    if (n_loci) *n_loci = n;
    return MONI_OK;
}
