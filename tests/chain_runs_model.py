"""A model of the chaining of one read's anchors (chain.hpp:278-400, single-end) and of what decides whether chain_runs_kernel takes the read: its runs of
anchors, their lengths, its chain starts and kept chains.  Used by tests/test_gpu_chain_runs.py (over the seeds the GPU fetches) and by
profiles/chain_runs_hist.py (over the CPU oracle's); imports no test module."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FAST = open(os.path.join(ROOT, "moni_align_amd", "csrc", "align_fast.hip")).read()
RUN_LEN, SLOTS, CHAINS, NODES = (int(re.search(r"#define %s (\d+)" % n, _FAST).group(1)) for n in ("AF_RUN_LEN", "AF_RUN_SLOTS", "AF_RUN_CHAINS", "AF_RUN_NODES"))
L0_SEEDS = 24                         # the small instance of chain_plan_kernel: seeds (its chain starts: CHAINS)
DEFAULTS = dict(min_len=25, freq_thr=0.5, max_dist_x=500, max_dist_y=100, max_iter=10, max_pred=5, min_chain_score=40)      # moni_align_params_default


def anchors_of(seeds, prm=DEFAULTS):
    """per read: (x, rpos, len, mate) of its anchors after seed_freq_filter, in populate_anchors' order"""
    mems, occs, rmo = seeds["mems"], seeds["occs"], seeds["read_mem_off"]
    out = []
    for r in range(len(rmo) - 1):
        ms = mems[int(rmo[r]):int(rmo[r + 1])]
        total = int(ms["occ_cnt"].sum())
        an = []
        for m in ms:
            if total and int(m["occ_cnt"]) / total > prm["freq_thr"]:
                continue
            for o in occs[int(m["occ_off"]):int(m["occ_off"]) + int(m["occ_cnt"])]:
                an.append((int(o) + int(m["len"]) - 1, int(m["rpos"]), int(m["len"]), int(m["mate"])))
        out.append(an)
    return out


def route_model(an, prm=DEFAULTS, min_chain_length=1):
    """chain.hpp:278-400 over one read's anchors (single-end), sorted by x with a stable sort (the order of tied anchors may differ from libstdc++'s, which
    moves no anchor between runs).  Returns what decides the read's route and what the batches are built for."""
    import math
    an = sorted(an, key=lambda a: a[0])
    n = len(an)
    f, p, t, msc = [0] * n, [0] * n, [0] * n, [0] * n
    avg = np.float32(sum(a[2] for a in an)) / np.float32(n) if n else 0.0
    lb = 0
    for i in range(n):
        x_i, y_i, w_i, mate_i = an[i]
        max_f, max_j, n_pred = w_i, -1, 0
        if i - lb > prm["max_iter"]:
            lb = i - prm["max_iter"]
        j = i - 1
        while j >= lb:
            x_j, y_j, _, mate_j = an[j]
            jj = j
            j -= 1
            if mate_i != mate_j:
                continue
            if x_i > x_j + prm["max_dist_x"]:
                lb = jj
                continue
            x_d, y_d = x_i - x_j, y_i - y_j
            l = abs(y_d - x_d)
            if y_j >= y_i or y_d > prm["max_dist_y"]:
                continue
            alpha = min(y_d, x_d, w_i)
            beta = (int(.01 * l * float(avg)) + int(math.log2(l))) >> 1 if l > 0 else 0
            score = f[jj] + alpha - beta
            if score > max_f:
                max_f, max_j = score, jj
                n_pred = max(0, n_pred - 1)
            elif t[jj] == i:
                n_pred += 1
                if n_pred > prm["max_pred"]:
                    break
            if p[jj] > 0:
                t[p[jj]] = i
        f[i], p[i] = max_f, max_j
        msc[i] = msc[max_j] if max_j >= 0 and msc[max_j] > max_f else max_f
    run_of, k = [0] * n, 0
    for i in range(1, n):
        k += 1 if an[i][0] > an[i - 1][0] + prm["max_dist_x"] else 0
        run_of[i] = k
    run_len = np.bincount(run_of, minlength=1) if n else np.zeros(1, int)
    is_pred = [False] * n
    for i in range(n):
        if p[i] >= 0:
            is_pred[p[i]] = True
    starts, steps = [], 0
    for i in range(n):
        if not is_pred[i] and msc[i] > prm["min_chain_score"]:
            j, s = i, 0
            while f[j] < msc[j]:
                j, s = p[j], s + 1
            steps = max(steps, s)
            starts.append((f[j], j))
    starts.sort(reverse=True)
    used, kept, dropped_in_multi = [False] * n, [], False
    per_run = np.bincount([run_of[j] for _, j in starts], minlength=len(run_len)) if starts else np.zeros(len(run_len), int)
    for fs, j0 in starts:
        j, cnt = j0, 0
        while True:
            cnt += 1
            used[j] = True
            j = p[j]
            if j < 0 or used[j]:
                break
        keep = cnt >= min_chain_length if j < 0 else (fs - f[j] >= prm["min_chain_score"] and cnt >= min_chain_length)
        if keep:
            kept.append(fs)
        elif per_run[run_of[j0]] >= 2:
            dropped_in_multi = True
    return dict(n=n, n_runs=len(run_len) if n else 0, max_run=int(run_len.max()) if n else 0, run_lens=[int(x) for x in run_len] if n else [], starts=len(starts), kept=len(kept), steps=steps,
                equal_scores=len(kept) >= 2 and len(set(kept)) == 1, multi_start_dropped=dropped_in_multi, tied=any(an[i][0] == an[i - 1][0] for i in range(1, n)))


def models(seeds, prm=DEFAULTS):
    rmo, mems = seeds["read_mem_off"], seeds["mems"]
    out = []
    for r, an in enumerate(anchors_of(seeds, prm)):
        ms = mems[int(rmo[r]):int(rmo[r + 1])]
        total = int(ms["occ_cnt"].sum())
        m = route_model(an, prm)
        m["seeds"] = sum(1 for x in ms if not (total and int(x["occ_cnt"]) / total > prm["freq_thr"]))
        # the route: a read of the small instance's list whose runs fit the slots ...
        m["gate"] = 0 < m["n"] <= NODES and m["seeds"] <= L0_SEEDS and m["n_runs"] <= SLOTS and m["max_run"] <= RUN_LEN
        # ... and whose chain starts the small instance would hold (otherwise the large instance chains the read)
        m["routed"] = m["gate"] and m["starts"] <= CHAINS
        out.append(m)
    return out
