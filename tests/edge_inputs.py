"""Inputs that tests/test_gpu_kmeans_edges.py runs on the device and tests/test_kmeans_ref_host.py / tests/test_ivf_ref_host.py run
through the restatements' plain-Python twins on the host: the same arrays on both sides, so the restatement is witnessed on exactly the
inputs on which it is the device's oracle.  Nothing here computes a result."""
import numpy as np

F32 = np.float32

# ------------------------------------------------------------------------------------------------ the grouping: sizes and patterns
# KM_TILE = 1024 items a tile, k_km_scan 8 tiles a step: one tile short of full, full, one item into the second; 8 tiles (one step, no
# remainder), 8 tiles and an item (one step, a remainder of one), 9221 = 9 tiles and 5 items (one step, a remainder of two)
GROUP_NS = [1023, 1024, 1025, 8192, 8193, 9221]
GROUP_PATTERNS = ["random", "round_robin", "one_cluster", "ascending", "descending"]
# C = 257 at every n; at n = 9221 the cluster counts around k_km_starts' P = ceil(C / 256) and k_km_scan's 64 clusters a workgroup
GROUP_CASES = [(n, 257, p) for n in GROUP_NS for p in GROUP_PATTERNS] + \
              [(9221, Cn, p) for Cn in (65, 256, 300, 1000, 4095, 4096) for p in GROUP_PATTERNS]


def group_assign(n, Cn, pattern):
    rng = np.random.default_rng(n * 7 + Cn)
    if pattern == "random":
        a = rng.integers(0, Cn, n)
    elif pattern == "round_robin":                       # 64 consecutive items: 64 distinct clusters when Cn >= 64
        a = np.arange(n) % Cn
    elif pattern == "one_cluster":                       # 64 equal lanes, one scatter round; every other list empty
        a = np.full(n, Cn - 1)
    elif pattern == "ascending":                         # runs that cross lane groups and tiles
        a = np.sort(rng.integers(0, Cn, n))
    elif pattern == "descending":
        a = np.sort(rng.integers(0, Cn, n))[::-1]
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(a, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ non-finite items
NAN_ROW, PINF_ROW, NINF_ROW = 70, 200, 499              # 70 = 64 + 6 and 200 = 3 * 64 + 8: inside a 64-row slot; 499: the last item


def nonfinite_case():
    """-> (x [500][12], init centroids [5][12]): general floats; one row with a NaN, one with +inf, one with -inf, each in one column.
    The initial centroids are finite rows of x."""
    rng = np.random.default_rng(41)
    x = (rng.standard_normal((500, 12)) + 2.0 * rng.integers(-1, 2, (500, 1))).astype(F32)
    x[NAN_ROW, 4] = np.nan
    x[PINF_ROW, 3] = np.inf
    x[NINF_ROW, 9] = -np.inf
    init = x[[5, 100, 250, 300, 450]].copy()
    assert np.isfinite(init).all()
    return x, init


# ------------------------------------------------------------------------------------------------ degenerate SPHERICAL clusters
def near_e2(rng, m):
    x = np.zeros((m, 4), F32)
    x[:, 1] = 1.0
    return (x + 0.1 * rng.standard_normal((m, 4))).astype(F32)


def zero_sum_case():
    """-> (x, init, orth): centroids e1 and e2 in dim 4; the items `orth` are +-e3 and +-e4 (scaled), each next to its negative in item
    order: their keys are zeros for both centroids, the tie goes to cluster 0, whose sum is exactly zero.  The others lie near e2."""
    rng = np.random.default_rng(42)
    x = near_e2(rng, 90)
    orth = np.array([10, 11, 40, 41, 70, 71, 88, 89])
    e3, e4 = np.array([0, 0, 1, 0], F32), np.array([0, 0, 0, 1], F32)
    x[orth] = np.stack([e3, -e3, 3 * e4, -3 * e4, -0.5 * e3, 0.5 * e3, -e4, e4])
    return x, np.eye(2, 4, dtype=F32), orth


def overflow_case():
    """-> (x, init, big): centroids e1 and e2; the items `big` are 1e19 e1, so cluster 0's sum is 4e19 e1 and q = 1.6e39 is +inf in
    fp32 while every key and every sum is finite."""
    rng = np.random.default_rng(43)
    x = near_e2(rng, 80)
    big = np.array([3, 64, 65, 79])
    x[big] = 0
    x[big, 0] = 1e19
    return x, np.eye(2, 4, dtype=F32), big


def pairs_case():
    """-> (x, init): one cluster; every item is followed by its negative, so the serial chain of the sum is exactly zero."""
    rng = np.random.default_rng(44)
    half = rng.standard_normal((5, 4)).astype(F32)
    x = np.empty((10, 4), F32)
    x[0::2], x[1::2] = half, -half
    return x, x[[2]].copy()
