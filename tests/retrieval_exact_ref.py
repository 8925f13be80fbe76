"""Numpy restatement of the two retrieval statistics of the gallery path for the EXACT tests (tests/test_gpu_retrieval_exact.py):
rank statistics per query (gallery_ref.ap_stats' rules) and class-level leave-one-out statistics for a subset of the query rows
(class_stats_ref.class_stats' rules), both from float32 distances that are exact (nearest_ref.distances32 of integer features),
in ascending (distance, index) order.  Also how far a single off-by-one moves a query's AP, and the inputs of the GPU tests:
built here so that the CPU suite can assert their preconditions (tests/test_retrieval_exact_ref_host.py)."""
import numpy as np

import class_stats_ref
import nearest_ref

SEG = 16384           # items per workgroup of the row kernels below 64 * 16384 items (retrieval.hip, gallery_init)
CSEG = 65536          # items per workgroup of k_class_count (retrieval.hip, vv_gallery_class_stats)
CHUNK = 2048          # positives of one pass ("positive_chunk")


# ---------------------------------------------------------------------------------------------- rank statistics
def rank_rows(d32, q_ids, g_ids):
    """d32 [nq][ng].  dict of best_rank int64 [nq] (10000 where no positive ranks earlier), ap float64 [nq], acc1 / acc5 / acc10
    float64 [nq] (a count; counts over min(P, 5); over min(P, 10): gallery_ref.ap_stats), top5_idx int32 [nq][5] / top5_dist
    float32 [nq][5] (-1 / 0 past the gallery's end), val: per query the ranks of its positives, ascending (int64)."""
    nq, ng = d32.shape
    g_ids = np.asarray(g_ids)
    out = dict(best_rank=np.full(nq, 10000, np.int64), ap=np.zeros(nq), acc1=np.zeros(nq), acc5=np.zeros(nq), acc10=np.zeros(nq),
               top5_idx=np.full((nq, 5), -1, np.int32), top5_dist=np.zeros((nq, 5), np.float32), val=[])
    rank = np.empty(ng, np.int64)
    for i in range(nq):
        order = np.argsort(d32[i], kind="stable")                     # ascending (d, index)
        rank[order] = np.arange(1, ng + 1)
        val = np.sort(rank[g_ids == q_ids[i]])
        P = len(val)
        out["val"].append(val)
        k5 = min(5, ng)
        out["top5_idx"][i, :k5] = order[:k5]
        out["top5_dist"][i, :k5] = d32[i, order[:k5]]
        if P == 0:
            continue
        out["best_rank"][i] = min(10000, int(val[0]))
        out["ap"][i] = (np.arange(1, P + 1) / val).sum() / P
        out["acc1"][i] = (val <= 1).sum()
        out["acc5"][i] = (val <= 5).sum() / min(P, 5)
        out["acc10"][i] = (val <= 10).sum() / min(P, 10)
    return out


def rank_summary(r):
    """The five summary values of gallery_ref.rank_stats from rank_rows' per-query values (float64 means)."""
    best = np.sort(r["best_rank"])
    nq = len(best)
    med = (best[nq // 2 - 1] + best[nq // 2]) / 2.0 if nq % 2 == 0 else float(best[nq // 2])
    return dict(median_rank=med, recall_1=r["acc1"].sum() / nq, recall_5=r["acc5"].sum() / nq, recall_10=r["acc10"].sum() / nq,
                mean_ap=r["ap"].sum() / nq)


# ---------------------------------------------------------------------------------------------- class statistics
def class_rows(d_rows, rows, video_ids, cls, exclude):
    """class_stats_ref.class_stats for the query rows `rows` only: d_rows [len(rows)][n] are their distances to every item, cls
    [n] the class of every item (class_stats_ref.classes_of).  dict of ap / acc1 / acc5 float64 [len(rows)] (NaN for a query of
    negative class), top5 int64 [len(rows)][5] (-1 past the items of other videos, or skipped), val / ret: per row the `val`
    and `ret` of its positives in rank order (empty for a skipped row)."""
    video_ids, cls = np.asarray(video_ids), np.asarray(cls)
    m = len(rows)
    out = dict(ap=np.full(m, np.nan), acc1=np.full(m, np.nan), acc5=np.full(m, np.nan), top5=np.full((m, 5), -1, np.int64),
               val=[], ret=[])
    for r, i in enumerate(rows):
        if cls[i] < 0:
            out["val"].append(np.zeros(0, np.int64)); out["ret"].append(np.zeros(0, np.int64))
            continue
        order = np.argsort(d_rows[r], kind="stable")
        order = order[order != i]
        other = order[video_ids[order] != video_ids[i]]
        out["top5"][r, :min(5, len(other))] = other[:5]
        ranked = other if exclude else order
        val = np.flatnonzero(cls[ranked] == cls[i]) + 1
        ret = np.arange(1, len(val) + 1)
        out["val"].append(val); out["ret"].append(ret)
        out["ap"][r] = (ret / val).sum() / len(val) if len(val) else 0.0
        out["acc1"][r] = (val <= 1).sum()
        out["acc5"][r] = (val <= 5).sum() / 5.0
    return out


# ---------------------------------------------------------------------------------------------- sensitivity
def ap_sensitivity(val, ret=None):
    """ap = (1/P) sum ret_j / val_j.  The smallest |change of ap| that an error of +-1 in one positive's val, or in one positive's
    ret, causes (float64; inf without positives).  ret defaults to 1 .. P."""
    val = np.asarray(val, np.float64)
    P = len(val)
    if P == 0:
        return np.inf
    ret = np.arange(1, P + 1, dtype=np.float64) if ret is None else np.asarray(ret, np.float64)
    d_val_up = ret / val - ret / (val + 1)
    d_val_dn = np.where(val > 1, ret / np.maximum(val - 1, 1) - ret / val, np.inf)
    d_ret = 1.0 / val
    return float(min(d_val_up.min(), d_val_dn.min(), d_ret.min()) / P)


def ulp32(x):
    """One float32 ulp at float32(x)."""
    return float(np.spacing(np.abs(np.float32(x))))


def within_one_ulp(got32, want64):
    """|got - float32(want)| <= 1 float32 ulp, elementwise; NaN matches NaN."""
    got32, want64 = np.asarray(got32), np.asarray(want64, np.float64)
    w32 = want64.astype(np.float32)
    both_nan = np.isnan(got32) & np.isnan(w32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got32.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64)
    return ok | both_nan


# ---------------------------------------------------------------------------------------------- inputs
def place_ids(ng, background, placed):
    """g_ids [ng]: `background` (int array [ng]) with placed = {id: indices} written over it."""
    gid = np.asarray(background, np.int32).copy()
    seen = np.zeros(ng, bool)
    for v, idx in placed.items():
        idx = np.asarray(idx)
        assert not seen[idx].any(), "an index is given two ids"
        seen[idx] = True
        gid[idx] = v
    return gid


# Test a: 513 queries x 49 153 items, D = 40.  Four segments of 16384, the last of one item.
A_NG, A_NQ, A_D = 3 * SEG + 1, 513, 40
A_SINGLE = {1: 0, 2: SEG - 1, 3: SEG, 4: 2 * SEG - 1, 5: 2 * SEG, 6: 3 * SEG - 1, 7: 3 * SEG}     # id: its only item
A_TIE_BLOCKS = [(0, 8), (SEG - 8, SEG + 8), (2 * SEG - 8, 2 * SEG + 8), (3 * SEG - 8, 3 * SEG + 1)]   # [lo, hi): copies of one row
A_STRADDLE = {8: [SEG - 2, SEG + 1], 9: [2 * SEG - 2, 2 * SEG + 1, 2 * SEG + 2],                 # inside the tie blocks
              10: [SEG - 300, SEG + 200], 11: [2 * SEG - 1000, 2 * SEG - 999, 2 * SEG + 77]}     # outside them
A_BIG = {20: 2047, 21: 2048, 22: 2049, 23: 4096, 24: 4097, 25: 6000}                             # id: how many items it owns
A_ABSENT = [-5, 50, 10 ** 6]                     # below every gallery id, between two of them, above all
A_BACKGROUND = (100, 140)                        # every other item: one of these ids


def input_a():
    """Q, q_ids, G, g_ids and what the test needs to know about them: probes = query rows with exactly one positive,
    big = {id: query rows}, absent = query rows whose id the gallery does not hold."""
    Q, _, G, _ = nearest_ref.exact_input(A_NQ, A_NG, 1, 41, dim=A_D)
    rng = np.random.default_rng(42)
    for lo, hi in A_TIE_BLOCKS:
        G[lo:hi] = G[lo]
    placed = {v: [g] for v, g in A_SINGLE.items()}
    placed.update(A_STRADDLE)
    taken = np.zeros(A_NG, bool)
    for idx in placed.values():
        taken[idx] = True
    for lo, hi in A_TIE_BLOCKS:
        taken[lo:hi] = True                                             # the big ids stay out of the tie blocks
    free = rng.permutation(np.flatnonzero(~taken))
    at = 0
    for v, cnt in A_BIG.items():
        placed[v] = np.sort(free[at:at + cnt])
        at += cnt
    gid = place_ids(A_NG, rng.integers(A_BACKGROUND[0], A_BACKGROUND[1], A_NG), placed)
    # queries.  Every single-positive id three times: a random query (any rank), the positive's own row (a rank near 1, behind
    # the ties of lower index) and its negation (a rank near the end); the last one in the one-row second query block.
    qid = rng.integers(A_BACKGROUND[0], A_BACKGROUND[1], A_NQ).astype(np.int32)
    probes = []
    row = 0
    for v, g in A_SINGLE.items():
        for form in range(3):
            qid[row] = v
            if form == 1:
                Q[row] = G[g]
            elif form == 2:
                Q[row] = -G[g]
            probes.append(row)
            row += 1
    qid[A_NQ - 1] = 7                                                   # random query, positive at the last item
    probes.append(A_NQ - 1)
    qid[127], qid[128] = 2, 3                                           # the rows at the edge of the first query tile
    probes += [127, 128]
    straddle = {}
    for v in A_STRADDLE:
        straddle[v] = [row, row + 1]
        qid[row], qid[row + 1] = v, v
        Q[row + 1] = G[A_STRADDLE[v][0]]
        row += 2
    big = {}
    for v in A_BIG:
        big[v] = [row, row + 1, 200 + v, 511 - (v - 20)]
        qid[big[v]] = v
        row += 2
    absent = [row, row + 1, row + 2]
    qid[absent] = A_ABSENT
    return dict(Q=Q, qid=qid, G=G, gid=gid, probes=sorted(probes), straddle=straddle, big=big, absent=absent)


# Test b: 129 queries x 2100 items, D = 32, under two id assignments over the same features (2049 + 2048 > 2100: one gallery
# cannot hold both): an id of 2049 items (two passes, the second of one positive) and an id of 2048 (one full pass).
B_NG, B_NQ, B_D = 2100, 129, 32
B_BIG = {2049: 7, 2048: 8}                       # how many items: the id that owns them


def input_b(P):
    """Q, q_ids, G, g_ids for the assignment in which id B_BIG[P] owns P items; big = the query rows that carry it."""
    Q, _, G, _ = nearest_ref.exact_input(B_NQ, B_NG, 1, 43, dim=B_D)
    rng = np.random.default_rng(44 + P)
    perm = rng.permutation(B_NG)
    gid = place_ids(B_NG, 100 + np.arange(B_NG) % 6, {B_BIG[P]: np.sort(perm[:P])})
    qid = np.full(B_NQ, B_BIG[P], np.int32)
    other = np.array([3, 40, 65, 100, 126], np.int64)                   # (rows 0, 63, 64, 127, 128 keep the big id)
    qid[other] = [100, 103, 105, 999, 101]
    Q[5] = 0                                                            # every distance +0: the order is the index order
    Q[9] = G[perm[0]]
    Q[10] = -G[perm[1]]
    big = np.flatnonzero(qid == B_BIG[P])
    return dict(Q=Q, qid=qid, G=G, gid=gid, big=big)


# Test c: 66 049 items, D = 32: two counting segments (65536 + 513), five top-5 segments, 130 query blocks.
C_N, C_D = CSEG + 513, 32
C_LARGE = {1: 5000, 2: 2048, 3: 2049}            # class: items
C_SMALL = (100, 400)                             # 300 classes of 2 .. 8 items, each with members on both sides of item 65536
C_BACKGROUND = (10, 50)                          # classes of the rest


def input_c():
    """X, video_ids, id2class (dict), cls (class of every item, absent ids read 0), small = {class: item indices}."""
    _, _, X, _ = nearest_ref.exact_input(1, C_N, 1, 45, dim=C_D)
    rng = np.random.default_rng(46)
    cls_of = np.full(C_N, -2, np.int64)                                # -2: not yet assigned
    low = list(rng.permutation(CSEG))
    high = list(rng.permutation(np.arange(CSEG, C_N)))
    small, groups = {}, []                                             # groups: (class or None for "absent from the map", members)
    for c in range(*C_SMALL):
        size = int(rng.integers(2, 9))
        n_high = 1 if size < 4 or c % 3 else 2
        mem = [high.pop() for _ in range(n_high)] + [low.pop() for _ in range(size - n_high)]
        small[c] = np.array(sorted(mem))
        cls_of[small[c]] = c
        # videos: the first high member shares a video with the first low member in every second class (a same-video item in the
        # other counting segment); the rest are videos of one or two items.  A class of two in one video has no positive
        # under exclusion.
        m = list(mem)
        if c % 2 == 0:
            groups.append((c, [m[0], m[n_high]]))
            m = [x for x in m if x not in (m[0], m[n_high])]
        while m:
            take = min(len(m), int(rng.integers(1, 3)))
            groups.append((c, m[:take]))
            m = m[take:]
    rest = rng.permutation(np.array(low + high))
    at = 0
    plan = [(c, cnt) for c, cnt in C_LARGE.items()] + [(-1, int(0.03 * C_N)), (None, 1000)]
    for c, cnt in plan:
        idx = rest[at:at + cnt]
        at += cnt
        cls_of[idx] = 0 if c is None else c
        j = 0
        while j < cnt:
            take = min(cnt - j, int(rng.integers(1, 5)))
            groups.append((c, list(idx[j:j + take])))
            j += take
    idx = rest[at:]
    bg = rng.integers(C_BACKGROUND[0], C_BACKGROUND[1], len(idx))
    for c in range(*C_BACKGROUND):
        mem = idx[bg == c]
        cls_of[mem] = c
        j = 0
        while j < len(mem):
            take = min(len(mem) - j, int(rng.integers(1, 5)))
            groups.append((c, list(mem[j:j + take])))
            j += take
    assert (cls_of > -2).all()
    vids = 1000 + 3 * rng.permutation(len(groups))
    video_ids = np.zeros(C_N, np.int32)
    id2class = {}
    for v, (c, mem) in zip(vids, groups):
        video_ids[mem] = v
        if c is not None:
            id2class[int(v)] = int(c)
    cls = class_stats_ref.classes_of(video_ids, id2class)
    assert np.array_equal(cls, cls_of)
    return dict(X=X, vid=video_ids, map=id2class, cls=cls, small=small)


C_FIXED_ROWS = [0, 511, 512, CSEG - 1, CSEG, C_N - 1]


def rows_c(c, want_small=10, margin=4.0):
    """The reference rows of test c and their reference values under both settings of `exclude`:
    rows (sorted), d [len(rows)][n], ref = {exclude: class_rows(...)}, small_rows = the positions in `rows` of every member of
    `want_small` small classes.  Those are the first classes, in class order, all of whose members have ap_sensitivity >= margin
    ulp (or no positive at all) under both settings: an input choice made from the reference alone."""
    X, vid, cls = c["X"], c["vid"], c["cls"]
    chosen, tried = [], 0
    for k in sorted(c["small"]):
        mem = c["small"][k]
        d = nearest_ref.distances32(X[mem], X)
        tried += 1
        ok = True
        for ex in (True, False):
            r = class_rows(d, mem, vid, cls, ex)
            ok &= all(len(v) == 0 or ap_sensitivity(v, t) >= margin * ulp32(a) for v, t, a in zip(r["val"], r["ret"], r["ap"]))
        if ok:
            chosen.append(k)
        if len(chosen) == want_small:
            break
    assert len(chosen) == want_small, "only %d of %d small classes have the margin" % (len(chosen), tried)
    rows = set(C_FIXED_ROWS)
    small_items = np.concatenate([c["small"][k] for k in chosen])
    rows.update(int(i) for i in small_items)
    for k in C_LARGE:
        mem = np.flatnonzero(cls == k)
        rows.update(int(i) for i in (mem[0], mem[len(mem) // 2], mem[-1]))
    rows.update(int(i) for i in np.flatnonzero(cls < 0)[[0, 700, -1]])
    rows = np.array(sorted(rows))
    d = nearest_ref.distances32(X[rows], X)
    ref = {ex: class_rows(d, rows, vid, cls, ex) for ex in (True, False)}
    small_rows = np.flatnonzero(np.isin(rows, small_items))
    return dict(rows=rows, d=d, ref=ref, small_rows=small_rows, classes=chosen, tried=tried)


# Test d: whole rows through Gallery.nearest(Q, k = ng).  (nq, ng, D): every value of each appears.
D_SHAPES = [(1, 127, 1), (1, 2048, 32), (127, 128, 31), (127, 129, 33), (128, 127, 32), (128, 128, 64), (128, 2048, 96),
            (129, 127, 33), (129, 128, 1), (129, 129, 32), (129, 2048, 31), (127, 2048, 64)]


def input_d(nq, ng, D):
    """Q, G; the last query row (the tile's edge row) is all zero unless it is the only one."""
    Q, _, G, _ = nearest_ref.exact_input(nq, ng, 1, 47 + nq + ng + D, dim=D)
    if nq > 1:
        Q[nq - 1] = 0
    return Q, G
