// Host side of pseudo-matching lengths (included inside extern "C" of moni_hip.hip): the kernel is in pml_kernels.hip.
// One run = pack_kernel (the patterns of the resident batch into the workspace) + pml_kernel; the results stay on the device until fetched.

static int pml_run_resident(moni_ctx* c, uint32_t thr) {
    moni_index* I = c->idx;
    HIPCHK(hipSetDevice(I->device));
    if (c->h_blk.empty()) return MONI_EINVAL;          // no batch was made resident
    auto& B = c->pml;
    B.valid = false;
    const uint64_t nr = c->n_reads, n_tasks = 2 * nr;
    int rc;
    if ((rc = c->pat.ensure(c->h_blk.back().y + 1)) || (rc = c->pflag.ensure(n_tasks + 8)) || (rc = B.lens.ensure(c->total_len + 4)) || (rc = B.mx.ensure(nr + 1)) ||
        (rc = B.hits.ensure(nr + 1)))
        return rc;
    HIPCHK(hipMemsetAsync(c->d_counters.p, 0, 4 * sizeof(unsigned long long), c->stream));
    rec(c, EV_ALL0);
    if (nr)
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n_tasks + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, c->seq.p, c->offs.p, c->blk.p, n_tasks,
                           c->pat.p, c->pflag.p);
    rec(c, EV_MS0);
    if (nr)
        hipLaunchKernelGGL(pml_kernel, dim3((unsigned)((nr + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, I->d_rows.p, I->d_frows.p, I->d_cr.p, I->d_recs.p,
                           c->pat.p, c->offs.p, c->blk.p, nr, thr, B.lens.p, B.mx.p, B.hits.p, c->d_counters.p);
    rec(c, EV_MS1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    B.n_reads = nr; B.total = c->total_len; B.valid = true;
    return MONI_OK;
}

int moni_pml_run(moni_ctx_t* c, uint32_t thr) {
    if (!c) return MONI_EINVAL;
    return pml_run_resident(c, thr);
}

int moni_pml_fetch(moni_ctx_t* c, uint32_t* lengths, uint32_t* read_max, uint32_t* read_hits) {
    if (!c || !c->pml.valid) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    const auto& B = c->pml;
    if (lengths && B.total) HIPCHK(hipMemcpy(lengths, B.lens.p, B.total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (read_max && B.n_reads) HIPCHK(hipMemcpy(read_max, B.mx.p, B.n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (read_hits && B.n_reads) HIPCHK(hipMemcpy(read_hits, B.hits.p, B.n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MONI_OK;
}

int moni_pml_sizes(moni_ctx_t* c, uint64_t* n_reads, uint64_t* total_len) {
    if (!c || !c->pml.valid) return MONI_EINVAL;
    if (n_reads) *n_reads = c->pml.n_reads;
    if (total_len) *total_len = c->pml.total;
    return MONI_OK;
}

int moni_pml_batch(moni_ctx_t* c, const moni_read_batch_t* b, uint32_t thr, uint32_t* lengths, uint32_t* read_max, uint32_t* read_hits) {
    if (!c || !b || (!lengths && !read_max && !read_hits)) return MONI_EINVAL;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    if (!b->n_reads) return MONI_OK;
    if ((rc = pml_run_resident(c, thr))) return rc;
    return moni_pml_fetch(c, lengths, read_max, read_hits);
}
