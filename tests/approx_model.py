"""The k-mismatch search in plain Python: the tree of backward-search steps of moni_align_amd/csrc/approx_core.h over LocateModel's arrays - the same
order (the substitutions A, C, G, T of a place before the pattern's own byte, depth first), the same pieces (level 0 cut into chunks of chunk_len
places), the same bound (max_steps backward-search steps per piece, asked before every step) and the same step counting - and, sharing nothing with
it but the text, a brute force over numpy sliding windows.  tests/test_approx_model.py checks the one against the other."""
import numpy as np

from tests import locate_model as lm

RES_DTYPE = np.dtype([("cnt", "<u8", (4,)), ("n_hits", "<u8"), ("hit_off", "<u8"), ("n_kept", "<u4"), ("complete", "<u4"), ("matched", "<u4"), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("task", "<u8"), ("n_mis", "<u4"), ("n_occ", "<u4"), ("sa_lo", "<u8"), ("count", "<u8"), ("occ_off", "<u8")])
assert RES_DTYPE.itemsize == 64 and HIT_DTYPE.itemsize == 40
ACGT = b"ACGT"
MAX_STEPS_DEFAULT = 1 << 20


class _Stop(Exception):
    pass


class ApproxModel(lm.LocateModel):
    def step(self, st, c):
        """one backward-search step of (lo, hi, toe) with byte c (a letter the BWT holds): the new triple, or None where the interval empties"""
        from bisect import bisect_left
        lo, hi, toe = st
        ck, before = self.runs[c], self.before[c]
        run = self.run_of_position(lo)
        j = bisect_left(ck, run)
        nlo = self.F[c] + before[j] + (lo - self.starts[run] if self.heads[run] == c else 0)
        run = self.run_of_position(hi)
        j = bisect_left(ck, run)
        if self.heads[run] == c:
            nhi = self.F[c] + before[j] + (hi - self.starts[run])
            ntoe = toe - 1
        else:
            nhi = self.F[c] + before[j] - 1
            ntoe = self.esa[ck[j - 1]] if j else 0
        return None if nlo > nhi else (nlo, nhi, ntoe)

    def root(self):
        return 0, self.n - 1, (self.esa[self.r - 1] + 1) % self.n

    def task(self, pat: bytes, k: int, chunk_len: int = 16, max_steps: int = MAX_STEPS_DEFAULT):
        """(hits, matched, complete, tree_steps): hits = [(n_mis, sa_lo, count, toehold)] of every matching string found, unsorted and uncapped;
        tree_steps counts every attempted (node, letter) step once - the exact path's in pass 1, not again when a piece walks its chunk"""
        m = len(pat)
        hits, tree = [], 0
        st, matched, ckpt = self.root(), 0, {}
        for s in range(m):                                   # pass 1: the exact path, a checkpoint at every chunk start
            if s % chunk_len == 0:
                ckpt[s // chunk_len] = st
            raw = pat[m - 1 - s]
            if raw <= 1 or raw not in self.runs:
                break
            tree += 1
            st = self.step(st, raw)
            if st is None:
                break
            matched += 1
        if m and matched == m:
            hits.append((0, st[0], st[1] - st[0] + 1, st[2]))
        complete = 1
        if k:
            for j in range((m + chunk_len - 1) // chunk_len):    # pass 2: one piece per chunk the exact path reached
                if matched < j * chunk_len:
                    continue
                used = [0, 0]                                # the piece's steps; those of them that are new

                def spend(new):
                    if max_steps and used[0] >= max_steps:
                        raise _Stop()
                    used[0] += 1
                    used[1] += new

                def level(e, s, st, end):
                    while s < end:
                        raw = pat[m - 1 - s]
                        if e < k:
                            for letter in ACGT:
                                if letter == raw or letter not in self.runs:
                                    continue
                                spend(1)
                                nxt = self.step(st, letter)
                                if nxt is not None:
                                    level(e + 1, s + 1, nxt, m)
                        if raw <= 1 or raw not in self.runs:
                            return
                        spend(1 if e else 0)
                        st = self.step(st, raw)
                        if st is None:
                            return
                        s += 1
                    if e:
                        hits.append((e, st[0], st[1] - st[0] + 1, st[2]))

                try:
                    level(0, j * chunk_len, ckpt[j], min(m, (j + 1) * chunk_len))
                except _Stop:
                    complete = 0
                tree += used[1]
        return hits, matched, complete, tree

    def approx_batch(self, patterns, strands=1, k=1, max_hits=0, max_occ=0, chunk_len=16, max_steps=MAX_STEPS_DEFAULT):
        """(res, hits, pos, seq, seq_off, tree_steps, all_hits) in the library's layout: task i * strands + s, the hits of a task sorted by
        (n_mis, sa_lo), positions by phi from the toehold.  Where a task has more than max_hits hits the first max_hits FOUND are kept - the exact
        one, then piece by piece - as a replay that runs the lanes one after the other keeps them (the GPU may keep others).
        all_hits[t]: every (n_mis, sa_lo, count) of the task, sorted"""
        res = np.zeros(len(patterns) * strands, dtype=RES_DTYPE)
        out, pos, all_hits, tree = [], [], [], 0
        for i, p in enumerate(patterns):
            for s in range(strands):
                t = i * strands + s
                hits, matched, complete, steps = self.task(lm.revcomp(p) if s else p, k, chunk_len, max_steps)
                tree += steps
                all_hits.append(sorted(h[:3] for h in hits))
                for e, _, count, _ in hits:
                    res["cnt"][t, e] += count
                kept = sorted(hits[:max_hits])
                res[t]["n_hits"], res[t]["hit_off"], res[t]["n_kept"], res[t]["complete"], res[t]["matched"] = len(hits), len(out), len(kept), complete, matched
                for e, sa_lo, count, toe in kept:
                    n_occ = min(count, max_occ)
                    out.append((t, e, n_occ, sa_lo, count, len(pos)))
                    pos += self.locate(toe, n_occ)
        hits = np.array(out, dtype=HIT_DTYPE) if out else np.zeros(0, dtype=HIT_DTYPE)
        pos = np.array(pos, dtype=np.uint64)
        sq = self.seq_of(pos).astype(np.uint32) if len(pos) else np.zeros(0, np.uint32)
        so = (pos.astype(np.int64) - self.seq_starts[sq]).astype(np.uint64) if len(pos) else np.zeros(0, np.uint64)
        return res, hits, pos, sq, so, tree, all_hits


# ---- brute force: nothing shared with the model or the library but the text ----------------------------------------------------------

_IS_ACGT = np.zeros(256, dtype=bool)
_IS_ACGT[list(ACGT)] = True


def brute(text: bytes, q: bytes, k: int):
    """{matching string: (distance, increasing positions)}: every window of len(q) that differs from q at no more than k places, each of them
    a place where the TEXT holds A, C, G or T; a pattern byte <= 1 equals nothing"""
    m = len(q)
    if m == 0 or m > len(text):
        return {}
    T = np.frombuffer(text, dtype=np.uint8)
    P = np.frombuffer(q, dtype=np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(T, m)
    differ = (win != P[None, :]) | (P <= 1)[None, :]
    dist = differ.sum(axis=1)
    ok = (dist <= k) & ~(differ & ~_IS_ACGT[win]).any(axis=1)
    out = {}
    for i in np.nonzero(ok)[0]:
        w = text[i:i + m]
        out.setdefault(w, (int(dist[i]), []))[1].append(int(i))
    return out


_rank = {}
_brute = {}


def rank_of(text: bytes):
    """the inverse of the naive suffix array of text + terminator"""
    if text not in _rank:
        sa = lm.naive_sa(text)
        inv = np.zeros(len(sa), dtype=np.int64)
        inv[np.array(sa)] = np.arange(len(sa))
        _rank[text] = inv
    return _rank[text]


def brute_task(text: bytes, q: bytes, k: int, max_occ: int, seq_starts):
    """(cnt[4], hits): hits sorted by (n_mis, sa_lo), each (n_mis, sa_lo, count, positions kept, their sequences, their offsets) - the positions
    of the max_occ highest ranks in decreasing rank order, binned by searchsorted over the sequence starts"""
    key = (text, q, k, max_occ)
    if key in _brute:                                        # computed once, shared among the tests that need it
        return _brute[key]
    rank = rank_of(text)
    ss = np.asarray(seq_starts).astype(np.int64)
    cnt, hits = [0, 0, 0, 0], []
    for w, (d, occ) in brute(text, q, k).items():
        cnt[d] += len(occ)
        occ = sorted(occ, key=lambda i: -rank[i])
        kept = np.array(occ[:max_occ], dtype=np.int64)
        sq = np.minimum(np.searchsorted(ss, kept, side="right") - 1, len(ss) - 2)
        hits.append((d, int(rank[occ[-1]]), len(occ), kept.tolist(), sq.tolist(), (kept - ss[sq]).tolist()))
    hits.sort()
    _brute[key] = (cnt, hits)
    return cnt, hits


def window_within(text: bytes, pos: int, q: bytes, n_mis: int):
    """does the window at pos differ from q at exactly n_mis places, each an A / C / G / T of the text?"""
    w = text[pos:pos + len(q)]
    if len(w) != len(q) or not q:
        return False
    bad = [i for i in range(len(q)) if w[i] != q[i] or q[i] <= 1]
    return len(bad) == n_mis and all(w[i] in ACGT for i in bad)


def check_against_brute(text: bytes, patterns, res, hits, pos, sq, so, strands, k, max_hits, max_occ, seq_starts, complete=True):
    """res / hits / pos / sq / so in the library's layout against brute force.  Full equality where a task's hits all fit max_hits; where they do not,
    n_kept and that the kept hits are a subset of the true ones, distinct and in order.  Every listed position is looked at in the text."""
    assert len(res) == len(patterns) * strands
    at_h = at_p = 0
    for i, p in enumerate(patterns):
        for s in range(strands):
            t = i * strands + s
            q = lm.revcomp(p) if s else p
            cnt, want = brute_task(text, q, k, max_occ, seq_starts)
            r = res[t]
            assert int(r["complete"]) == 1 or not complete
            assert [int(x) for x in r["cnt"]] == cnt, (t, q[:40], r, cnt)
            assert int(r["n_hits"]) == len(want) and int(r["n_kept"]) == min(len(want), max_hits), (t, r, len(want))
            nk = int(r["n_kept"])
            if nk:
                assert int(r["hit_off"]) == at_h, t
            got = hits[at_h:at_h + nk]
            assert all(int(h["task"]) == t for h in got)
            keys = [(int(h["n_mis"]), int(h["sa_lo"])) for h in got]
            assert keys == sorted(set(keys)), (t, keys)
            by_key = {(w[0], w[1]): w for w in want}
            if len(want) <= max_hits:
                assert keys == [(w[0], w[1]) for w in want], (t, keys)
            for h in got:
                w = by_key.get((int(h["n_mis"]), int(h["sa_lo"])))
                assert w is not None and int(h["count"]) == w[2] and int(h["n_occ"]) == min(w[2], max_occ), (t, h, w)
                n = int(h["n_occ"])
                if n:
                    assert int(h["occ_off"]) == at_p, (t, h)
                    gp = [int(x) for x in pos[at_p:at_p + n]]
                    assert gp == w[3] and [int(x) for x in sq[at_p:at_p + n]] == w[4] and [int(x) for x in so[at_p:at_p + n]] == w[5], (t, h, gp, w)
                    for x in gp:
                        assert window_within(text, x, q, int(h["n_mis"])), (t, x)
                    at_p += n
            at_h += nk
    assert at_h == len(hits) and at_p == len(pos) == len(sq) == len(so)


def approx_patterns():
    """(flat index, text, patterns, marks): locate_model.planted_case() and the patterns the k-mismatch search can go wrong at; marks names some of them"""
    fi, text, pats = lm.planted_case()
    s0 = text[:int(fi.seq_starts[1]) - int(fi.w)]
    pats = list(pats)
    marks = {}

    def add(name, p):
        marks[name] = len(pats)
        pats.append(p)

    add("absent byte", s0[200:220] + b"X" + s0[221:240])
    add("byte <= 1", s0[200:220] + b"\x01" + s0[221:240])
    add("lower case", s0[200:220] + s0[220:221].lower() + s0[221:240])
    add("len 15", s0[300:315])
    add("len 16", s0[300:316])
    add("len 17", s0[300:317])
    add("short", s0[700:708])
    add("N in pattern", s0[600:610] + b"N" + s0[611:620])
    marks.update({"empty": pats.index(b""), "len 1": 0, "N against N": pats.index(b"NNNN"), "dies first": pats.index(s0[100:140] + b"X"),
                  "dies middle": pats.index(s0[100:120] + b"X" + s0[121:140]), "dies last": pats.index(b"X" + s0[101:140])})
    return fi, text, pats, marks
