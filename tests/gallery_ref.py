"""Float64 restatement of the reference's RetrievalRankStatsFixedRefLayer for the gallery tests
(src/caffe/layers/retrieval_rank_stats_fixed_ref_layer.cpp; cites are lines of that file), the issue's input generator and the
near-tie bookkeeping the tests share.  Ties are ordered by ascending reference index (the reference's std::sort, :158-162,
leaves them unspecified; the product documents this rule)."""
import numpy as np


def make_input(nq, ng, D, nid, noise, seed):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((nid, D))
    gid = rng.integers(0, nid, ng)
    qid = rng.integers(0, nid, nq)
    G = cen[gid] + noise * rng.standard_normal((ng, D))
    Q = cen[qid] + noise * rng.standard_normal((nq, D))
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return Q.astype(np.float32), qid.astype(np.int32), G.astype(np.float32), gid.astype(np.int32)


def distances(Q, G, dtype=np.float64):
    """:142-144: alpha = -2 times Q G^T."""
    return dtype(-2.0) * (Q.astype(dtype) @ G.astype(dtype).T)


def ap_stats(order_ids, qid):
    """ComputeApStats (:62-118) over one query's reference ids in sorted order."""
    ap = acc1 = acc5 = acc10 = 0.0
    ret = 0.0
    best = 10000                                                  # :70
    hits = np.flatnonzero(order_ids == qid) + 1                   # `val` at every positive (:74-75)
    for val in hits:
        if val < best:
            best = int(val)                                       # :77-79
        acc1 += val <= 1
        acc5 += val <= 5
        acc10 += val <= 10                                        # :81-89
        ret += 1
        ap += ret / val                                           # :90-91
    if ret > 0:                                                   # :95-108
        ap /= ret
        acc5 /= ret if ret < 5 else 5
        acc10 /= ret if ret < 10 else 10
    return ap, acc1, acc5, acc10, best


def rank_stats(d, qid, gid):
    """Forward_cpu (:147-230) on a distance matrix d [nq][ng].  Returns (summary dict, best [nq], ap [nq], order [nq][ng])."""
    nq = d.shape[0]
    order = np.argsort(d, axis=1, kind="stable")                  # ascending (d, index)
    best = np.empty(nq, np.int64)
    ap = np.empty(nq, np.float64)
    s1 = s5 = s10 = 0.0
    for i in range(nq):
        a, r1, r5, r10, b = ap_stats(gid[order[i]], qid[i])
        ap[i], best[i] = a, b
        s1 += r1; s5 += r5; s10 += r10                            # :172-176
    ranks = np.sort(best)
    med = (ranks[nq // 2 - 1] + ranks[nq // 2]) / 2.0 if nq % 2 == 0 else float(ranks[nq // 2])   # :218-224
    return dict(median_rank=med, recall_1=s1 / nq, recall_5=s5 / nq, recall_10=s10 / nq, mean_ap=ap.sum() / nq), best, ap, order


def best_rank_interval(d_row, pos, eps):
    """The best ranks a computation whose distances are within eps/2 of d_row can report: a positive p may rank anywhere from
    1 + #{d < d_p - eps} to #{d <= d_p + eps}; the best rank is the minimum over positives of either end (capped like :70)."""
    if len(pos) == 0:
        return 10000, 10000
    s = np.sort(d_row)
    lo = min(1 + np.searchsorted(s, d_row[p] - eps, side="left") for p in pos)
    hi = min(np.searchsorted(s, d_row[p] + eps, side="right") for p in pos)
    return min(int(lo), 10000), min(int(hi), 10000)
