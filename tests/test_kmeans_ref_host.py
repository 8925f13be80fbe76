"""tests/kmeans_ref.py on the host, before the GPU tests lean on it: against a plain float64 Lloyd iteration on well-separated blobs
(equal assignments; centroids within count * 2^-24 * max|x| per element, the serial chain's own bound: count - 1 additions, each off
by at most half an ulp of a partial sum that is at most count * max|x|, and one multiplication), the chunk order by hand on three tiny
cases, the objective's fold, and the tie and NaN rules; then the NaN, Inf and degenerate rules against a plain-Python twin on the inputs
the GPU tests use (tests/edge_inputs.py)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_inputs as inp   # noqa: E402
import kmeans_ref as ref   # noqa: E402

F32 = np.float32


def host_scores(x):
    """a float32 d from float64 products: not the library's bits, but blobs this far apart do not care"""
    x64 = np.asarray(x, np.float64)
    return lambda cent: (-2.0 * (x64 @ np.asarray(cent, np.float64).T)).astype(F32) + F32(0.0)


def blobs(n, k, dim, seed, spread=0.4, radius=12.0):
    rng = np.random.default_rng(seed)
    member = rng.integers(0, k, n)
    member[:k] = np.arange(k)
    x = (radius * np.eye(k, dim)[member] + spread * rng.standard_normal((n, dim))).astype(F32)
    return x, member


def lloyd64(x, cent, iters, metric):
    x, cent = np.asarray(x, np.float64), np.array(cent, np.float64)
    for _ in range(iters + 1):
        d = -2.0 * x @ cent.T
        key = d if metric == "spherical" else d + (cent * cent).sum(1)[None, :]
        a = key.argmin(1)
        if _ == iters:
            break
        for c in range(len(cent)):
            if (a == c).any():
                s = x[a == c].sum(0)
                cent[c] = s / np.sqrt((s * s).sum()) if metric == "spherical" else s / (a == c).sum()
    return a, cent


@pytest.mark.parametrize("metric", ["euclidean", "spherical"])
@pytest.mark.parametrize("n,k,dim", [(300, 3, 5), (1500, 6, 17)])
def test_restatement_against_float64_lloyd(metric, n, k, dim):
    x, member = blobs(n, k, dim, n + k)
    init = x[:k]
    got = ref.run(x, init, 3, metric, host_scores(x))
    a64, c64 = lloyd64(x, init, 3, metric)
    last = got["passes"][-1]
    assert np.array_equal(last["assign"], a64) and np.array_equal(a64, member)
    counts = np.bincount(a64, minlength=k)
    bound = counts[:, None] * 2.0 ** -24 * float(np.abs(x).max())
    # (SPHERICAL divides the sum by its norm, here far above 1: the same bound holds with room to spare)
    err = np.abs(got["centroids"].astype(np.float64) - c64)
    print("largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()
    assert got["passes"][0]["moved"] == n and last["moved"] == 0 and got["empty_last"] == 0


def test_chunk_order_by_hand():
    # 1: three rows, one chunk: ((a + b) + c), where the other order differs
    x = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], F32)
    assert ref.cluster_sum(x, np.arange(3))[0] == F32(1.0)                     # 1 + 2^-24 rounds to 1, twice
    assert (x[1, 0] + x[2, 0]) + x[0, 0] != F32(1.0)
    # 2: 257 rows: the first chunk is rows 0 .. 255, the second row 256 alone, added last
    x = np.full((257, 1), 2.0 ** -24, F32)
    x[0, 0] = 1.0
    x[256, 0] = 2.0 ** -23
    assert ref.cluster_sum(x, np.arange(257))[0] == F32(1.0) + F32(2.0 ** -23)      # the chain stays at 1; the last partial is one ulp
    # 3: 513 rows, three chunks: the second and third partials are each 256 * 2^-24 = 2^-16 exactly (and 2^-24 alone), added whole
    x = np.full((513, 1), 2.0 ** -24, F32)
    x[0, 0] = 1.0
    want = F32(F32(F32(1.0) + F32(2.0 ** -16)) + F32(2.0 ** -24))
    assert ref.cluster_sum(x, np.arange(513))[0] == want == F32(1.0) + F32(2.0 ** -16)
    # the list is the items in ascending index, whatever lies between them
    x = np.arange(10, dtype=F32)[:, None]
    new, empty, degenerate = ref.update(x, np.array([1, 0, 1, 1, 0, 1, 1, 1, 1, 1], np.int32), np.zeros((3, 1), F32) + 5, "euclidean")
    assert new[:, 0].tolist() == [2.5, F32(40.0) * (F32(1.0) / F32(8.0)), 5.0] and (empty, degenerate) == (1, 0)


def test_objective_fold():
    sel = np.arange(1, 131, dtype=F32)                                          # three slots: 64, 64, 2 items
    assert ref.objective_of(sel) == 130 * 131 / 2
    big = np.zeros(64, F32)
    big[0], big[32], big[1] = 2.0 ** 60, -2.0 ** 60, 1.0                        # x[0] += x[32] first: the 1 survives
    assert ref.objective_of(big) == 1.0
    big[32], big[1] = 1.0, -2.0 ** 60                                           # ... here it meets 2^60 before the negative does
    assert ref.objective_of(big) == 0.0


def test_ties_nan_and_degenerate():
    key = np.array([[1, 1, 0.5, 0.5], [np.nan, 2, 2, np.nan], [np.nan] * 4, [np.inf, np.nan, np.inf, 1]], F32)
    assert ref.assign_of(key).tolist() == [2, 1, 0, 3]
    st = ref.step(np.zeros((3, 2), F32), np.array([[1.0], [1.0]], F32), "euclidean", None)
    assert st["assign"].tolist() == [0, 0, 0] and st["counts"].tolist() == [3, 0] and st["moved"] == 3
    x = np.array([[1.0], [-1.0], [3.0]], F32)
    new, empty, degenerate = ref.update(x, np.array([0, 0, 1], np.int32), np.array([[7.0], [7.0]], F32), "spherical")
    assert new[:, 0].tolist() == [7.0, 1.0] and (empty, degenerate) == (0, 1)   # s = 0: the row stays


# ------------------------------------------------------------------------------------------------ the NaN, Inf and degenerate rules
# A twin of the restatement's rules in plain Python: one float32 scalar at a time, no numpy reduction, no masking, no argsort.  The
# restatement is the oracle of tests/test_gpu_kmeans_edges.py on the inputs of tests/edge_inputs.py; here it is held to the twin on
# the same inputs, the distances computed on the host.
def twin_chain_sq(row):
    q = F32(0.0)
    for v in row:
        q = F32(q + F32(v * v))
    return q


def twin_keys(d, cent, metric):
    key = np.array(d, F32, copy=True)
    if metric == "euclidean":
        for c in range(cent.shape[0]):
            nn = twin_chain_sq(cent[c])
            for i in range(key.shape[0]):
                key[i, c] = F32(d[i, c] + nn)
    return key


def twin_assign(key):
    """per row: the first cluster whose key is a number and below every earlier one; none: cluster 0"""
    out = []
    for row in key:
        best = None
        for c, k in enumerate(row):
            if math.isnan(k):
                continue                                                        # a NaN key is never selected
            if best is None or k < row[best]:                                   # (strictly: the lowest cluster keeps a tie)
                best = c
        out.append(0 if best is None else best)
    return out


def twin_update(x, a, cent, metric):
    new = np.array(cent, F32, copy=True)
    empty = degenerate = 0
    for c in range(cent.shape[0]):
        items = [i for i in range(len(a)) if a[i] == c]                         # ascending item index
        if not items:
            empty += 1                                                          # the previous centroid stays
            continue
        s = None
        for b in range(0, len(items), 256):                                     # chunks of 256 list entries, added in ascending order
            acc = [F32(v) for v in x[items[b]]]
            for i in items[b + 1:b + 256]:
                acc = [F32(u + v) for u, v in zip(acc, x[i])]
            s = acc if s is None else [F32(u + v) for u, v in zip(s, acc)]
        if metric == "spherical":
            q = twin_chain_sq(s)
            if q == 0 or math.isnan(q) or math.isinf(q):
                degenerate += 1                                                 # the previous centroid stays
                continue
            nrm = np.sqrt(q, dtype=F32)
            new[c] = [F32(v / nrm) for v in s]
        else:
            inv = F32(F32(1.0) / F32(len(items)))
            new[c] = [F32(v * inv) for v in s]
    return new, empty, degenerate


def twin_run(x, cent0, iters, metric, scores_fn):
    cent, prev, passes = np.array(cent0, F32, copy=True), None, []
    empty = degenerate = 0
    for t in range(iters + 1):
        key = twin_keys(scores_fn(cent), cent, metric)
        a = twin_assign(key)
        sel = [key[i, a[i]] for i in range(len(a))]
        counts = [0] * cent.shape[0]
        for c in a:
            counts[c] += 1
        passes.append(dict(assign=a, counts=counts, centroids=cent.copy(),
                           moved=len(a) if prev is None else sum(1 for u, v in zip(a, prev) if u != v),
                           nonfinite=sum(1 for v in sel if math.isnan(v) or math.isinf(v))))
        prev = a
        if t == iters:
            break
        cent, empty, degenerate = twin_update(x, a, cent, metric)
    return dict(passes=passes, centroids=cent, empty_last=empty, degenerate_last=degenerate)


def same_or_nan(got, want):
    """NaN where the twin has a NaN (numpy and Python need not agree on a payload), equal bits everywhere else"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def held_to_the_twin(x, init, iters, metric):
    with np.errstate(all="ignore"):
        got = ref.run(x, init, iters, metric, host_scores(x))
        want = twin_run(x, init, iters, metric, host_scores(x))
    assert len(got["passes"]) == iters + 1
    for g, w in zip(got["passes"], want["passes"]):
        assert g["assign"].tolist() == w["assign"] and g["counts"].tolist() == w["counts"]
        assert g["moved"] == w["moved"] and g["nonfinite"] == w["nonfinite"]
        assert same_or_nan(g["centroids"], w["centroids"])
    assert same_or_nan(got["centroids"], want["centroids"])
    assert (got["empty_last"], got["degenerate_last"]) == (want["empty_last"], want["degenerate_last"])
    return got


@pytest.mark.parametrize("metric", ["euclidean", "spherical"])
def test_nonfinite_rules_against_the_twin(metric):
    x, init = inp.nonfinite_case()
    got = held_to_the_twin(x, init, 2, metric)
    for t, st in enumerate(got["passes"]):
        assert st["assign"][inp.NAN_ROW] == 0 and np.isnan(st["sel"][inp.NAN_ROW])      # every key of the row is NaN: cluster 0
        assert np.isinf(st["sel"][inp.PINF_ROW]) or np.isnan(st["sel"][inp.PINF_ROW])
        assert st["nonfinite"] >= 1 and math.isnan(st["objective"])
        assert np.array_equal(st["counts"], np.bincount(st["assign"], minlength=5))
    if metric == "spherical":
        # the NaN row's cluster has a q that is not finite at every update: degenerate, its centroid kept, every centroid finite
        assert got["degenerate_last"] >= 1 and np.isfinite(got["centroids"]).all()
        assert np.array_equal(got["centroids"][0], init[0])
    else:
        assert np.isnan(got["passes"][1]["centroids"][0, 4])                            # the NaN row's column of its cluster's mean


def test_degenerate_rules_against_the_twin():
    x, init, orth = inp.zero_sum_case()
    got = held_to_the_twin(x, init, 1, "spherical")
    assert np.array_equal(np.flatnonzero(got["passes"][0]["assign"] == 0), orth)
    assert got["degenerate_last"] == 1 and got["empty_last"] == 0 and np.array_equal(got["centroids"][0], init[0])
    assert not np.array_equal(got["centroids"][1], init[1])
    x, init, big = inp.overflow_case()
    got = held_to_the_twin(x, init, 1, "spherical")
    assert np.array_equal(np.flatnonzero(got["passes"][0]["assign"] == 0), big)
    assert got["degenerate_last"] == 1 and got["empty_last"] == 0 and np.array_equal(got["centroids"][0], init[0])
    assert got["passes"][0]["nonfinite"] == 0 and np.isfinite(got["centroids"]).all()
    assert held_to_the_twin(x, init, 1, "euclidean")["degenerate_last"] == 0        # EUCLIDEAN has no such rule: the mean is 1e19 e1
    x, init = inp.pairs_case()
    got = held_to_the_twin(x, init, 1, "spherical")
    assert got["degenerate_last"] == 1 and np.array_equal(got["centroids"], init) and got["passes"][1]["moved"] == 0


def test_twin_assign_by_hand():
    nan, inf = float("nan"), float("inf")
    key = np.array([[1, 1, 0.5, 0.5], [nan, 2, 2, nan], [nan] * 4, [inf, nan, inf, 1], [nan, inf, inf, nan], [0.0, -0.0, nan, 0.0],
                    [nan, -inf, -inf, 3]], F32)
    assert twin_assign(key) == [2, 1, 0, 3, 1, 0, 1] == ref.assign_of(key).tolist()
