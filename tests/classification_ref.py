"""A numpy restatement of ClassificationStatsLayer::Forward_cpu (src/caffe/layers/classification_stats_layer.cpp:36-95), written
from the layer's behaviour: what the GPU tests of vv_classification_stats compare against.

Accuracy: the predicted class of a row is the lowest column attaining the row's maximum (:50-61); count[c] = rows of label c,
correct[c] = those predicted c; accuracy[c] = float32(correct) / float32(count), 0 for an absent class; total = float32(sum
correct) / float32(n).  All integers, so these are exact.

Average precision, the layer's quirk included: per class the layer sorts n dummy entries (0, False) together with the n real
(score, label == c) pairs, descending by (score, flag), and walks only the first n.  A positive p with score s >= 0 (-0.0 included)
sits at position G + E (G = rows with score > s, E = positives with score == s and a lower index) and is the (P + E + 1)-th positive
met (P = positives with score > s); a positive with s < 0 lies behind the dummies and is never reached, though it counts in the
divisor.  ap[c] = (sum over the visited positives, ascending index, of (P + E + 1) / (G + E + 1)) / count[c], float64 throughout.

The hand-checkable case: n = 4, C = 2, labels = [0, 1, 0, 1], column-0 scores = [0.5, 0.7, -0.1, 0.0].  The positives of class 0
are items 0 and 2; item 2 is negative and never visited; item 0 has G = 1 (0.7), P = E = 0: its term is 1/2; ap[0] = 0.5 / 2 = 0.25.

`by_sorting` performs the layer's procedure literally (the 2 n entries, the sort, the walk) in float64: the host tests hold the
counting form against it."""
import numpy as np


def predict(scores):
    return np.argmax(scores, axis=1)            # the first maximum; -0.0 == 0.0


def class_ap64(col, positive):
    """float64 ap of one class: col fp32 [n], positive bool [n]."""
    pos = np.flatnonzero(positive)
    if pos.size == 0:
        return 0.0
    s = col[pos] + np.float32(0)                # -0.0 -> +0.0: equal keys get equal bits
    n = col.shape[0]
    G = n - np.searchsorted(np.sort(col), s, side="right")
    P = pos.size - np.searchsorted(np.sort(s), s, side="right")
    _, inv = np.unique(s, return_inverse=True)
    order = np.argsort(inv, kind="stable")      # equal scores together, ascending item index inside
    gi = inv[order]
    first = np.r_[0, np.flatnonzero(np.diff(gi)) + 1]
    start = np.repeat(first, np.diff(np.r_[first, gi.size]))
    E = np.empty(pos.size, np.int64)
    E[order] = np.arange(pos.size) - start
    term = np.where(s >= 0, (P + E + 1).astype(np.float64) / (G + E + 1).astype(np.float64), 0.0)
    return float(np.cumsum(term)[-1] / pos.size)        # cumsum: a serial sum in ascending item index


def classification_stats(scores, labels, num_classes):
    """dict(count int64 [C], correct int64 [C], accuracy fp32 [C], total_accuracy fp32, ap64 float64 [C], mean_ap64, classes_present)."""
    scores = np.asarray(scores, np.float32)
    labels = np.asarray(labels, np.int64)
    n, C = scores.shape
    assert C == num_classes and labels.shape == (n,) and not np.isnan(scores).any()
    pred = predict(scores)
    count = np.bincount(labels, minlength=C)
    correct = np.bincount(labels[pred == labels], minlength=C)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(count > 0, correct.astype(np.float32) / count.astype(np.float32), np.float32(0)).astype(np.float32)
    ap64 = np.array([class_ap64(scores[:, c], labels == c) for c in range(C)], np.float64)
    present = int((count > 0).sum())
    return dict(count=count, correct=correct, accuracy=acc, total_accuracy=np.float32(correct.sum()) / np.float32(n), ap64=ap64,
                mean_ap64=float(ap64[count > 0].sum() / present), classes_present=present)


def by_sorting(scores, labels, num_classes):
    """float64 ap [C] by the layer's own procedure: n dummies, the real pairs, sort by (score, flag) descending, the first n."""
    scores = np.asarray(scores, np.float32)
    n, C = scores.shape
    out = np.zeros(C)
    for c in range(C):
        entries = [(0.0, False)] * n + [(float(scores[i, c]), bool(labels[i] == c)) for i in range(n)]
        entries.sort(reverse=True)
        hits, prec = 0, 0.0
        for j in range(n):
            if entries[j][1]:
                hits += 1
                prec += hits / (j + 1)
        cnt = int((np.asarray(labels) == c).sum())
        out[c] = prec / cnt if cnt else 0.0
    return out


def ulp_diff32(a, b):
    """Distance in fp32 units in the last place between two fp32 arrays of finite, non-negative values."""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def make_case(rng, n, C, kind):
    """(scores fp32 [n][C], labels int32 [n]) of one of the families the tests walk."""
    labels = rng.integers(0, C, n).astype(np.int32)
    if kind == "random":
        scores = rng.standard_normal((n, C)).astype(np.float32)
    elif kind == "ties":                          # five values: ties dominate, exact zeros of both signs
        scores = rng.choice(np.array([-1, -0.0, 0.0, 0.5, 1], np.float32), (n, C))
    elif kind == "inf":
        scores = rng.standard_normal((n, C)).astype(np.float32)
        m = rng.random((n, C))
        scores[m < 0.1] = np.inf
        scores[m > 0.9] = -np.inf
    elif kind == "structured":                    # an absent class, a single-positive class, an all-negative column, ties
        scores = np.round(rng.standard_normal((n, C)) * 2).astype(np.float32) / 2
        if C >= 2:
            labels[labels == C - 1] = 0           # class C - 1 absent
        if C >= 3 and n >= 2:
            labels[labels == 1] = 0
            labels[rng.integers(0, n)] = 1        # class 1: a single positive
        scores[:, 0] = -np.abs(scores[:, 0]) - 1  # column 0 all below zero: ap[0] == 0 with count[0] > 0
    elif kind == "one_class":                     # a class holding every row
        labels[:] = C - 1
        scores = rng.choice(np.array([-1, -0.0, 0.0, 0.5, 1], np.float32), (n, C))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(scores, np.float32), labels
