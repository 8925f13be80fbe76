"""Numpy restatement of the k-NN classifier of vv_gallery_knn_scores / vv_gallery_knn_scores_self for the tests, on top of
nearest_ref.nearest: the neighbour lists are that function's, the scores are the class shares of the lists' weights.

Weight of list position j, with s_j = -0.5 d_j:  UNIFORM 1;  EXP exp((s_j - s_0) / T).  score[i][c] = V_c / V, V_c the sum of
the weights of the positions whose item has class c, V the sum over the m filled positions; a row with m == 0 is all zero.

UNIFORM is computed in float32 exactly as the header states it: float32(V_c) / float32(m), integers below 2^24, one rounding.
EXP is computed in float64 from the float32 distances and the float32 temperature: what the device's fp32 result is held
against within a bound the GPU test derives.  `knn_scores_brute_force` does the same by plain Python loops."""
import math

import numpy as np

import nearest_ref

UNIFORM, EXP = 0, 1


def _lists(d, eligible, k, lists):
    """nearest_ref.nearest(d, eligible, k), or its first k columns of a longer result computed earlier (the same lists)."""
    if lists is None:
        return nearest_ref.nearest(d, eligible, k)
    assert lists[0].shape[1] >= k
    return lists[0][:, :k], lists[1][:, :k]


def knn_scores(d, eligible, labels, num_classes, k, weighting=UNIFORM, temperature=None, lists=None):
    """d [n_q][n_ref] float32, eligible bool [n_q][n_ref] or None, labels [n_ref] in [0, num_classes).  lists: None, or what
    nearest_ref.nearest(d, eligible, k') returned for a k' >= k (a test that walks several k computes them once).
    Returns (scores [n_q][num_classes], float32 under UNIFORM and float64 under EXP; m int32 [n_q])."""
    idx, dist = _lists(d, eligible, k, lists)
    labels = np.asarray(labels, np.int64)
    nq = d.shape[0]
    m = (idx >= 0).sum(axis=1).astype(np.int32)
    out = np.zeros((nq, num_classes), np.float32 if weighting == UNIFORM else np.float64)
    for i in range(nq):
        if m[i] == 0:
            continue
        cls = labels[idx[i, :m[i]]]
        if weighting == UNIFORM:
            votes = np.bincount(cls, minlength=num_classes)
            out[i] = votes.astype(np.float32) / np.float32(m[i])
        else:
            s = -0.5 * dist[i, :m[i]].astype(np.float64)
            w = np.exp((s - s[0]) / np.float64(np.float32(temperature)))
            v = np.bincount(cls, weights=w, minlength=num_classes)
            out[i] = v / v.sum()
    return out, m


def exp_sums(d, eligible, labels, num_classes, k, temperature, lists=None):
    """The float64 V of every row under EXP (0 where m == 0) and the float64 arguments (s_j - s_0) / T of the filled positions,
    -inf elsewhere [n_q][k]: what the GPU test's error bound is built from."""
    idx, dist = _lists(d, eligible, k, lists)
    arg = np.where(idx >= 0, (-0.5 * dist.astype(np.float64) - (-0.5 * dist[:, :1].astype(np.float64))) / np.float64(np.float32(temperature)),
                   -np.inf)
    return np.exp(arg).sum(axis=1), arg


def knn_scores_brute_force(d, eligible, labels, num_classes, k, weighting=UNIFORM, temperature=None):
    """The same by plain Python loops over sorted (distance, index) tuples."""
    nq, ng = d.shape
    out = np.zeros((nq, num_classes), np.float32 if weighting == UNIFORM else np.float64)
    m = np.zeros(nq, np.int32)
    for i in range(nq):
        pairs = sorted((d[i, g], g) for g in range(ng) if eligible is None or eligible[i, g])[:k]
        m[i] = len(pairs)
        if not pairs:
            continue
        if weighting == UNIFORM:
            votes = [0] * num_classes
            for _, g in pairs:
                votes[int(labels[g])] += 1
            for c in range(num_classes):
                out[i, c] = np.float32(votes[c]) / np.float32(len(pairs))
        else:
            T = float(np.float32(temperature))
            s0 = -0.5 * float(pairs[0][0])
            v = [0.0] * num_classes
            for dist, g in pairs:
                v[int(labels[g])] += math.exp((-0.5 * float(dist) - s0) / T)
            total = math.fsum(v)
            for c in range(num_classes):
                out[i, c] = v[c] / total
    return out, m
