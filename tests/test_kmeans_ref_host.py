"""tests/kmeans_ref.py on the host, before the GPU tests lean on it: against a plain float64 Lloyd iteration on well-separated blobs
(equal assignments; centroids within count * 2^-24 * max|x| per element, the serial chain's own bound: count - 1 additions, each off
by at most half an ulp of a partial sum that is at most count * max|x|, and one multiplication), the chunk order by hand on three tiny
cases, the objective's fold, and the tie and NaN rules."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
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
