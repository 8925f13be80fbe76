"""Float64 restatement of the reference's RetrievalStatsLayer for the class-level statistics tests
(src/caffe/layers/retrieval_stats_layer.cpp; cites are lines of that file), the issue's input generator and the near-tie
bookkeeping the tests share.  Ties are ordered by ascending item index (the reference's std::sort, :236, leaves them unspecified;
the product documents this rule).  Video level: pooled items in ascending video id (the reference: boost::unordered_map order)."""
import numpy as np


def make_input(n, D, nvid, ncls, noise_v, noise_s, seed, neg_frac=0.05):
    rng = np.random.default_rng(seed)
    ccen = rng.standard_normal((ncls, D))
    vcls = rng.integers(0, ncls, nvid)
    vcls[rng.random(nvid) < neg_frac] = -1
    vcen = np.where(vcls[:, None] >= 0, ccen[np.maximum(vcls, 0)], rng.standard_normal((nvid, D))) \
           + noise_v * rng.standard_normal((nvid, D))
    vid_of = rng.integers(0, nvid, n)
    X = vcen[vid_of] + noise_s * rng.standard_normal((n, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    video_ids = (1000 + 7 * np.arange(nvid))[vid_of]
    return X.astype(np.float32), video_ids.astype(np.int32), {int(1000 + 7 * v): int(c) for v, c in enumerate(vcls)}


def distances(X, dtype=np.float64):
    """:208-209: alpha = -2 times X X^T."""
    X = X.astype(dtype)
    return dtype(-2.0) * (X @ X.T)


def classes_of(video_ids, id2class):
    """operator[] of the map (:110, :117): an absent id reads as class 0."""
    return np.array([id2class.get(int(v), 0) for v in video_ids], np.int64)


def pool_by_id(X, video_ids, dtype=np.float64):
    """:165-198: one row per distinct id, ascending id: sum over its items, ascending index, of (1 / count) x_i."""
    ids = np.unique(video_ids)
    X = X.astype(dtype)
    out = np.zeros((len(ids), X.shape[1]), dtype)
    for u, v in enumerate(ids):
        idx = np.flatnonzero(video_ids == v)
        w = dtype(1.0) / dtype(len(idx))
        for i in idx:
            out[u] += w * X[i]
    return out, ids.astype(np.int32)


def class_stats(d, video_ids, id2class, exclude=True):
    """Forward_cpu (:213-304, :351-353) on a distance matrix d [n][n].  Returns (summary dict, ap, acc1, acc5 [n] with NaN for
    the skipped queries, top5 [n][5]: the five nearest items of other ids, -1 where fewer exist or the query is skipped)."""
    n = d.shape[0]
    video_ids = np.asarray(video_ids)
    cls = classes_of(video_ids, id2class)
    ap = np.full(n, np.nan)
    acc1 = np.full(n, np.nan)
    acc5 = np.full(n, np.nan)
    top5 = np.full((n, 5), -1, np.int64)
    for i in range(n):
        if cls[i] < 0:                                              # :250-252
            continue
        order = np.argsort(d[i], kind="stable")                     # ascending (d, index)
        order = order[order != i]                                   # :113, :231-232: the query itself, whatever its distance
        other = order[video_ids[order] != video_ids[i]]
        top5[i, :min(5, len(other))] = other[:5]                    # :310-316
        ranked = other if exclude else order                        # :114-115
        val = np.flatnonzero(cls[ranked] == cls[i]) + 1             # `val` at every positive
        ret = np.arange(1, len(val) + 1)
        ap[i] = (ret / val).sum() / len(val) if len(val) else 0.0   # :125, :131-133
        acc1[i] = (val <= 1).sum()                                  # :118-120
        acc5[i] = (val <= 5).sum() / 5.0                            # :121-123, :135
    scored = cls >= 0
    ns = int(scored.sum())
    summary = dict(mean_ap=ap[scored].sum() / ns, hit_at_1=acc1[scored].sum() / ns, hit_at_5=acc5[scored].sum() / ns,
                   n_scored=ns) if ns else None                     # :351-353
    return summary, ap, acc1, acc5, top5


def acc_interval(d_row, i, video_ids, cls, exclude, eps, k):
    """The numbers of positives with val <= k that a computation whose distances are within eps / 2 of d_row can report for
    query i: a positive certainly counts when fewer than k ranked items lie within d_p + eps, and certainly does not when k
    or more lie below d_p - eps."""
    keep = np.arange(len(d_row)) != i
    if exclude:
        keep &= video_ids != video_ids[i]
    s = np.sort(d_row[keep])
    pos = np.flatnonzero(keep & (cls == cls[i]))
    lo = sum(int(np.searchsorted(s, d_row[p] + eps, side="right") <= k) for p in pos)
    hi = sum(int(np.searchsorted(s, d_row[p] - eps, side="left") + 1 <= k) for p in pos)
    return lo, hi
