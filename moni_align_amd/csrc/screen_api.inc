// Host side of read screening (included inside extern "C" of moni_hip.hip): the kernel is in screen_kernels.hip.
// One run = pack_kernel (the patterns of the resident batch into the workspace) + screen_kernel; one record per read stays on the device until fetched.

void moni_screen_params_default(moni_screen_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->window = 50; p->min_win = 25; p->ks_num = 1; p->ks_den = 4; p->strands = 2;
}

static int screen_run_resident(moni_ctx* c, const moni_screen_params_t* prm) {
    if (!prm || !screen_params_ok(*prm)) return MONI_EINVAL;
    moni_index* I = c->idx;
    HIPCHK(hipSetDevice(I->device));
    if (c->h_blk.empty()) return MONI_EINVAL;          // no batch was made resident
    auto& B = c->scr;
    B.valid = false;
    const uint64_t nr = c->n_reads, n_tasks = 2 * nr, n_lanes = nr * 2 * prm->strands;
    int rc;
    if ((rc = c->pat.ensure(c->h_blk.back().y + 1)) || (rc = c->pflag.ensure(n_tasks + 8)) || (rc = B.res.ensure(nr + 1))) return rc;
    HIPCHK(hipMemsetAsync(c->d_counters.p, 0, 4 * sizeof(unsigned long long), c->stream));
    rec(c, EV_ALL0);
    if (nr)
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n_tasks + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, c->seq.p, c->offs.p, c->blk.p, n_tasks,
                           c->pat.p, c->pflag.p);
    rec(c, EV_MS0);
    if (nr)
        hipLaunchKernelGGL(screen_kernel, dim3((unsigned)((n_lanes + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, I->d_tables.p, I->d_rows.p, I->d_frows.p, I->d_cr.p,
                           I->d_recs.p, c->pat.p, c->offs.p, c->blk.p, nr, *prm, B.res.p, c->d_counters.p);
    rec(c, EV_MS1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    B.n_reads = nr; B.valid = true;
    return MONI_OK;
}

int moni_screen_run(moni_ctx_t* c, const moni_screen_params_t* prm) {
    if (!c) return MONI_EINVAL;
    return screen_run_resident(c, prm);
}

int moni_screen_sizes(moni_ctx_t* c, uint64_t* n_reads) {
    if (!c || !c->scr.valid) return MONI_EINVAL;
    if (n_reads) *n_reads = c->scr.n_reads;
    return MONI_OK;
}

int moni_screen_fetch(moni_ctx_t* c, moni_screen_res_t* res) {
    if (!c || !c->scr.valid) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    const auto& B = c->scr;
    if (res && B.n_reads) HIPCHK(hipMemcpy(res, B.res.p, B.n_reads * sizeof(moni_screen_res_t), hipMemcpyDeviceToHost));
    return MONI_OK;
}

int moni_screen_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_screen_params_t* prm, moni_screen_res_t* res) {
    if (!c || !b || (!res && b->n_reads) || !prm || !screen_params_ok(*prm)) return MONI_EINVAL;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    if (!b->n_reads) return MONI_OK;
    if ((rc = screen_run_resident(c, prm))) return rc;
    return moni_screen_fetch(c, res);
}
