// Host side of the exact-match queries (included inside extern "C" of moni_hip.hip): the kernels are in locate_kernels.hip.
// One run = pack_kernel (the patterns of the resident batch into the workspace) + count_kernel, then - with max_occ > 0 - the rocPRIM exclusive scan
// of the capped counts and locate_walk_kernel; the results stay on the device until fetched.

void moni_locate_params_default(moni_locate_params_t* p) {
    if (!p) return;
    p->strands = 1; p->max_occ = 0; p->reserved[0] = p->reserved[1] = 0;
}

static int locate_params_ok(const moni_locate_params_t* p) { return p && (p->strands == 1 || p->strands == 2) && !p->reserved[0] && !p->reserved[1]; }

static int locate_run_resident(moni_ctx* c, const moni_locate_params_t* prm) {
    moni_index* I = c->idx;
    SearchDims D; int rc;
    if ((rc = search_dims(c, prm->strands, D))) return rc;
    auto& B = c->loc;
    B.valid = false;
    const uint64_t nr = D.nr, n_tasks = D.n_tasks;
    if ((rc = B.s.ensure(n_tasks))) return refused(rc);
    if ((rc = search_pack(c, D)) || (rc = search_count(c, D, prm->strands, prm->max_occ, B.s))) return rc;
    uint64_t total = 0;
    if (nr && prm->max_occ) {
        if ((rc = exclusive_scan_u64(c, B.s.cnt.p, B.s.off.p, n_tasks + 1))) return rc;
        HIPCHK(hipMemcpyAsync(&total, B.s.off.p + n_tasks, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    rec(c, EV_PC0);
    if (total) {          // no occurrence to list: no walk launch
        if ((rc = B.pos.ensure(total)) || (rc = B.seq.ensure(total)) || (rc = B.seq_off.ensure(total))) return refused(rc);
        phi_tab_t P; P.recs = I->d_phi.p; P.dir = I->d_phi_dir.p;
        hipLaunchKernelGGL(locate_walk_kernel, dim3((unsigned)((n_tasks + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, c->stream, I->K, P, I->d_seq_starts.p, n_tasks, B.s.res.p, B.s.toe.p,
                           B.s.off.p, B.pos.p, B.seq.p, B.seq_off.p, c->d_counters.p);
    }
    rec(c, EV_PC1);
    rec(c, EV_ALL1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    B.n_tasks = n_tasks; B.n_occ = total; B.valid = true;
    return MONI_OK;
}

int moni_locate_run(moni_ctx_t* c, const moni_locate_params_t* prm) {
    if (!c || !locate_params_ok(prm)) return MONI_EINVAL;
    return locate_run_resident(c, prm);
}

int moni_locate_sizes(moni_ctx_t* c, uint64_t* n_tasks, uint64_t* n_occ) {
    if (!c || !c->loc.valid) return MONI_EINVAL;
    if (n_tasks) *n_tasks = c->loc.n_tasks;
    if (n_occ) *n_occ = c->loc.n_occ;
    return MONI_OK;
}

int moni_locate_fetch(moni_ctx_t* c, moni_locate_res_t* res, uint64_t* pos, uint32_t* seq, uint64_t* seq_off) {
    if (!c || !c->loc.valid) return MONI_EINVAL;
    HIPCHK(hipSetDevice(c->idx->device));
    const auto& B = c->loc;
    if (res && B.n_tasks) HIPCHK(hipMemcpy(res, B.s.res.p, B.n_tasks * sizeof(moni_locate_res_t), hipMemcpyDeviceToHost));
    if (pos && B.n_occ) HIPCHK(hipMemcpy(pos, B.pos.p, B.n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (seq && B.n_occ) HIPCHK(hipMemcpy(seq, B.seq.p, B.n_occ * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (seq_off && B.n_occ) HIPCHK(hipMemcpy(seq_off, B.seq_off.p, B.n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MONI_OK;
}

int moni_locate_batch(moni_ctx_t* c, const moni_read_batch_t* b, const moni_locate_params_t* prm, moni_locate_res_t* res, uint64_t** pos, uint32_t** seq,
                      uint64_t** seq_off, uint64_t* n_occ) {
    if (!c || !b || !locate_params_ok(prm)) return MONI_EINVAL;
    if (pos) *pos = nullptr;
    if (seq) *seq = nullptr;
    if (seq_off) *seq_off = nullptr;
    if (n_occ) *n_occ = 0;
    int rc = moni_reads_upload(c, b);
    if (rc) return rc;
    if (!b->n_reads) return MONI_OK;
    if ((rc = locate_run_resident(c, prm))) return rc;
    const uint64_t n = c->loc.n_occ;
    HostArrays H;
    uint64_t* hp = H.want(pos, n); uint32_t* hs = H.want(seq, n); uint64_t* ho = H.want(seq_off, n);
    if (!H.ok) return MONI_ENOMEM;
    if ((rc = moni_locate_fetch(c, res, hp, hs, ho))) return rc;
    H.release();
    if (n_occ) *n_occ = n;
    return MONI_OK;
}
