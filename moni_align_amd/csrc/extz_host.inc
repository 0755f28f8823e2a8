// Host orchestration of extz_kernel (included inside extern "C" of moni_hip.hip).
// dp_run: results[i].cigar_off indexes `cig` (each CIGAR task owns qlen+tlen+2 slots there).  allow_modes lets the
// aligner pipeline name operands by position in the resident read batch / index text instead of shipping sequences.
static int dp_run(moni_ctx_t* c, const moni_dp_params_t* prm, const uint8_t* qseq, uint64_t qseq_len, const uint8_t* tseq,
                  uint64_t tseq_len, const moni_dp_task_t* tasks, uint64_t n_tasks, moni_dp_result_t* results,
                  std::vector<uint32_t>& cig, bool allow_modes) {
    if (!c || !prm || (n_tasks && (!tasks || !results)) || prm->m <= 0 || prm->m > 5) return MONI_EINVAL;
    if (!n_tasks) return MONI_OK;
    HIPCHK(hipSetDevice(c->idx->device));
    const int m = prm->m;
    if (prm->zdrop >= 0) return MONI_EINVAL;           // the reference always passes zdrop = -1 (aligner_ksw2.hpp:113)
    int min_sc = prm->mat[1];
    for (int t = 1; t < m * m; ++t) min_sc = min_sc < prm->mat[t] ? min_sc : prm->mat[t];
    const bool degenerate = -min_sc > 2 * (prm->q + prm->e);   // ksw2 returns with ez just reset
    std::vector<uint64_t> dir_off(n_tasks, 0), cig_off(n_tasks, 0);
    std::vector<uint32_t> order[5];           // [4]: problems too large for the one-wave kernels, run by extz_big_kernel in groups
    uint64_t dir_total = 0, cig_total = 0;
    for (uint64_t i = 0; i < n_tasks; ++i) {
        const moni_dp_task_t& t = tasks[i];
        if (t.qlen > DP_BIG_Q || t.tlen > DP_BIG_T) return MONI_ERANGE;
        const bool big_task = c->extz_lds ? (t.qlen > DP_LDS_Q || t.tlen > DP_LDS_T) : (t.qlen > DP_MAX_QLEN || t.tlen > 512);
        const int mode = t.reserved;
        if (mode && !allow_modes) return MONI_EINVAL;
        if (t.qlen > 0) {
            const uint64_t qcap = (mode & DP_Q_READS) ? c->total_len : qseq_len;
            if ((mode & DP_Q_REV) ? (t.q_off >= qcap || t.q_off + 1 < (uint64_t)t.qlen) : (t.q_off + (uint64_t)t.qlen > qcap)) return MONI_EINVAL;
        }
        if (t.tlen > 0 && !(mode & DP_T_TEXT)) {
            if ((mode & DP_T_REV) ? (t.t_off >= tseq_len || t.t_off + 1 < (uint64_t)t.tlen) : (t.t_off + (uint64_t)t.tlen > tseq_len)) return MONI_EINVAL;
        }
        if (t.tlen > 0 && (mode & DP_T_TEXT) && (mode & DP_T_REV) && t.t_off + 1 < (uint64_t)t.tlen) return MONI_EINVAL;
        const int big = t.qlen > t.tlen ? t.qlen : t.tlen;
        if (prm->w >= 0 && prm->w < big) return MONI_EINVAL;   // only the full matrix (w = -1) is implemented; never banded in the reference
        if (!(t.flag & DP_EZ_SCORE_ONLY) && t.qlen > 0 && t.tlen > 0) {
            if (!big_task) { dir_off[i] = dir_total; dir_total += (uint64_t)(t.qlen + t.tlen - 1) * t.tlen; }      // big ones: per group, below
            cig_off[i] = cig_total; cig_total += (uint64_t)t.qlen + t.tlen + 2;
        }
        const int nch = big_task ? 4 : t.tlen <= 64 ? 0 : t.tlen <= 128 ? 1 : t.tlen <= 256 ? 2 : 3;
        order[nch].push_back((uint32_t)i);
    }
    if (degenerate) {
        for (uint64_t i = 0; i < n_tasks; ++i) {
            moni_dp_result_t R;
            R.max = 0; R.max_q = R.max_t = R.mqe_t = R.mte_q = -1; R.mqe = R.mte = R.score = DP_NEG_INF;
            R.reach_end = 0; R.zdropped = 0; R.n_cigar = 0; R.cigar_off = 0;
            results[i] = R;
        }
        return MONI_OK;
    }
    int rc;
    if ((rc = c->dp_q.ensure(qseq_len + 16)) || (rc = c->dp_t.ensure(tseq_len + 16)) || (rc = c->dp_tasks.ensure(n_tasks)) ||
        (rc = c->dp_res.ensure(n_tasks)) || (rc = c->dp_dir.ensure(dir_total + 16)) || (rc = c->dp_cig.ensure(cig_total + 16)) ||
        (rc = c->dp_off.ensure(2 * n_tasks)) || (rc = c->dp_ws.ensure(n_tasks)))
        return rc;
    if (qseq_len) HIPCHK(hipMemcpyAsync(c->dp_q.p, qseq, qseq_len, hipMemcpyHostToDevice, c->stream));
    if (tseq_len) HIPCHK(hipMemcpyAsync(c->dp_t.p, tseq, tseq_len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->dp_tasks.p, tasks, n_tasks * sizeof(moni_dp_task_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->dp_off.p, dir_off.data(), n_tasks * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->dp_off.p + n_tasks, cig_off.data(), n_tasks * 8, hipMemcpyHostToDevice, c->stream));
    std::vector<uint32_t> ord_all;
    uint64_t ord_base[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < 5; ++b) { ord_base[b] = ord_all.size(); ord_all.insert(ord_all.end(), order[b].begin(), order[b].end()); }
    ord_base[5] = ord_all.size();
    HIPCHK(hipMemcpyAsync(c->dp_ws.p, ord_all.data(), ord_all.size() * 4, hipMemcpyHostToDevice, c->stream));
    dp_launch_t P;
    P.qseq = c->dp_q.p; P.tseq = c->dp_t.p; P.tasks = c->dp_tasks.p; P.dir_off = c->dp_off.p; P.cig_off = c->dp_off.p + n_tasks;
    P.dirs = c->dp_dir.p; P.cig_tmp = c->dp_cig.p; P.results = c->dp_res.p;
    P.sc_mch = prm->mat[0]; P.sc_mis = prm->mat[1]; P.sc_N = prm->mat[m * m - 1] == 0 ? -prm->e : prm->mat[m * m - 1];
    P.wild = m - 1; P.qo = prm->q; P.e = prm->e; P.end_bonus = prm->end_bonus;
    P.reads = c->seq.p; P.text = c->idx->d_text.p; P.n_text = c->idx->K.n_text;
    rec(c, EV_DP0);
    if (c->extz_lds) {          // LDS-tiled form for every size it takes (the one align_kernel uses)
        P.order = (const uint32_t*)c->dp_ws.p;
        if (ord_base[4]) hipLaunchKernelGGL(extz_lds_kernel, dim3((unsigned)ord_base[4]), dim3(64), 0, c->stream, P);
    } else
    for (int b = 0; b < 4; ++b) {
        const uint64_t cnt = ord_base[b + 1] - ord_base[b];
        if (!cnt) continue;
        P.order = (const uint32_t*)c->dp_ws.p + ord_base[b];
        const dim3 grid((unsigned)cnt), blk(64);
        if (b == 0) hipLaunchKernelGGL(extz_kernel<1>, grid, blk, 0, c->stream, P);
        else if (b == 1) hipLaunchKernelGGL(extz_kernel<2>, grid, blk, 0, c->stream, P);
        else if (b == 2) hipLaunchKernelGGL(extz_kernel<4>, grid, blk, 0, c->stream, P);
        else hipLaunchKernelGGL(extz_kernel<8>, grid, blk, 0, c->stream, P);
    }
    if (!order[4].empty()) {
        // oversize problems: state rows in HBM (dp_big_t per block), direction bytes from a buffer of bounded size, so they go
        // in groups; rare (long reads through the host pipeline) and slow, but the same code and the same results
        const uint64_t DIR_CAP = 1ull << 30;
        size_t at = 0;
        std::vector<uint64_t> big_off(n_tasks, 0);
        while (at < order[4].size()) {
            size_t end = at; uint64_t need = 0;
            while (end < order[4].size() && end - at < 256) {
                const moni_dp_task_t& t = tasks[order[4][end]];
                const uint64_t d = (t.flag & DP_EZ_SCORE_ONLY) || t.qlen <= 0 || t.tlen <= 0 ? 0 : (uint64_t)(t.qlen + t.tlen - 1) * t.tlen;
                if (end > at && need + d > DIR_CAP) break;
                big_off[order[4][end]] = need; need += d; ++end;
            }
            if ((rc = c->dp_dir_big.ensure(need + 64)) || (rc = c->dp_big.ensure(end - at))) return rc;
            // this group's direction offsets replace the (unused) entries of its tasks in the offset table
            for (size_t k = at; k < end; ++k) HIPCHK(hipMemcpyAsync(c->dp_off.p + order[4][k], &big_off[order[4][k]], 8, hipMemcpyHostToDevice, c->stream));
            dp_launch_t PB = P;
            PB.dirs = c->dp_dir_big.p;
            PB.order = (const uint32_t*)c->dp_ws.p + ord_base[4] + at;
            hipLaunchKernelGGL(extz_big_kernel, dim3((unsigned)(end - at)), dim3(64), 0, c->stream, PB, c->dp_big.p);
            HIPCHK(hipStreamSynchronize(c->stream));         // the host-side offsets above are reused by the next group
            at = end;
        }
    }
    rec(c, EV_DP1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(results, c->dp_res.p, n_tasks * sizeof(moni_dp_result_t), hipMemcpyDeviceToHost, c->stream));
    cig.resize(cig_total + 1);
    if (cig_total) HIPCHK(hipMemcpyAsync(cig.data(), c->dp_cig.p, cig_total * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    { float ms = 0; if (hipEventElapsedTime(&ms, c->ev[EV_DP0], c->ev[EV_DP1]) == hipSuccess) c->dp_kernel_ms_accum += ms; }
    for (uint64_t i = 0; i < n_tasks; ++i) results[i].cigar_off = (uint32_t)cig_off[i];
    return MONI_OK;
}

int moni_extz_batch(moni_ctx_t* c, const moni_dp_params_t* prm, const uint8_t* qseq, uint64_t qseq_len, const uint8_t* tseq,
                    uint64_t tseq_len, const moni_dp_task_t* tasks, uint64_t n_tasks, moni_dp_result_t* results,
                    uint32_t* cigar_pool, uint64_t cigar_pool_cap, uint64_t* cigar_pool_used) {
    if (cigar_pool_used) *cigar_pool_used = 0;
    std::vector<uint32_t> cig;
    int rc = dp_run(c, prm, qseq, qseq_len, tseq, tseq_len, tasks, n_tasks, results, cig, false);
    if (rc) return rc;
    uint64_t used = 0;
    for (uint64_t i = 0; i < n_tasks; ++i) {
        const uint32_t nc = results[i].n_cigar;
        const uint32_t src = results[i].cigar_off;
        results[i].cigar_off = (uint32_t)used;
        if (nc) {
            if (!cigar_pool || used + nc > cigar_pool_cap) return MONI_ENOMEM;
            memcpy(cigar_pool + used, cig.data() + src, (size_t)nc * 4);
            used += nc;
        }
    }
    if (cigar_pool_used) *cigar_pool_used = used;
    return MONI_OK;
}
