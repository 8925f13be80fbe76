"""k-means on a gallery at the edges tests/test_gpu_kmeans.py leaves out, bit for bit against tests/kmeans_ref.py and tests/ivf_ref.py:
the grouping (k_km_hist / k_km_starts / k_km_scan / k_km_scatter) read back through IVFIndex.lists() at the tile's and the scan step's
edges and at cluster counts that leave threads of k_km_starts and of k_km_scan without a cluster; k-means at those counts; rows of
8192 floats; an empty cluster followed through later passes; NaN and +-Inf items; degenerate SPHERICAL clusters.

Every comparison is of bits.  The one exception, in the tests whose inputs hold a NaN or an Inf and nowhere else: where the restatement
expects a NaN the library must give a NaN, of any payload and sign (the device and numpy need not agree on a payload)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_inputs as inp   # noqa: E402
import ivf_ref   # noqa: E402
import kmeans_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "spherical"]
VEC, ELEMENTWISE = 1, 2
F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def library_scores(eng, x):
    """scores_fn: the floats k_sim_f32 stores for x against the given centroids, as Gallery.scores hands them out."""
    def fn(cent):
        g = eng.gallery(cent)
        try:
            s = g.scores(x).get()
        finally:
            g.close()
        return (F32(-2.0) * s + F32(0.0)).astype(F32)
    return fn


def int_items(n, dim, seed):
    return np.random.default_rng(seed).integers(-4, 5, (n, dim)).astype(F32)


def check_pass(res, st):
    """the call's final pass against the restatement's pass st: finite inputs, every bit"""
    assert np.array_equal(res.assign, st["assign"])
    assert np.array_equal(res.counts, st["counts"])
    assert res.report["moved_last"] == st["moved"] == res.moved[-1]
    assert res.report["objective_last"] == st["objective"] == res.objective[-1]
    assert res.report["nonfinite_rows"] == st["nonfinite"]
    assert same_bits(res.centroids, st["centroids"])


# ------------------------------------------------------------------------------------------------ a. the grouping through lists()
@pytest.fixture(scope="module")
def group_galleries(eng):
    """one gallery per n: the grouping reads the assignment alone, the rows only have to be there"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = eng.gallery(np.random.default_rng(n).standard_normal((n, 8)).astype(F32))
        return made[n]
    yield get
    for g in made.values():
        g.close()


@pytest.mark.parametrize("n,Cn,pattern", inp.GROUP_CASES)
def test_grouping_is_a_stable_sort(eng, group_galleries, n, Cn, pattern):
    assign = inp.group_assign(n, Cn, pattern)
    cent = np.random.default_rng(Cn).standard_normal((Cn, 8)).astype(F32)
    start, lst = ivf_ref.lists_of(assign, Cn)
    sizes = np.bincount(assign, minlength=Cn)
    ix = eng.ivf(group_galleries(n), cent, assign=assign)
    try:
        got_start, got_lst = ix.lists()
        assert np.array_equal(got_start, start), np.flatnonzero(got_start != start)[:5]
        assert np.array_equal(got_lst, lst), np.flatnonzero(got_lst != lst)[:5]
        assert ix.get("largest_list") == sizes.max() and ix.get("empty_lists") == (sizes == 0).sum()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ b. k-means at the same cluster counts
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("Cn", [65, 257, 300, 1000])
def test_cluster_counts_past_one_stride(eng, metric, Cn):
    """C = 65: one lane into the assign sweep's second stride and k_km_scan's second workgroup; 257, 300, 1000: k_km_starts gives a
    thread 2 or 4 clusters, and the last threads a partial range or none.  Integer operands: every key of pass 0 is exact."""
    n = 3 * Cn + 7
    x = int_items(n, 8, 300 + Cn)
    rows = vv.kmeans_init_rows(7, n, Cn)
    want = ref.run(x, x[rows], 1, metric, ref.exact_scores(x))
    p0 = want["passes"][0]
    gal = eng.gallery(x)
    try:
        r0 = gal.kmeans(Cn, iters=0, metric=metric, init=rows)
        check_pass(r0, p0)
        assert eng.get_option("last_km_assign_form") == (VEC if Cn % 4 == 0 else ELEMENTWISE)
        r1 = gal.kmeans(Cn, iters=1, metric=metric, init=rows)
        assert r1.objective[0] == p0["objective"] and r1.moved[0] == n
        assert same_bits(r1.centroids, want["centroids"])
        assert r1.report["empty_last"] == want["empty_last"] and r1.report["degenerate_last"] == want["degenerate_last"]
        assert eng.get_option("last_km_assign_form") == (VEC if Cn % 4 == 0 else ELEMENTWISE)
        assert eng.get_option("last_km_chunks") == sum(-(-int(k) // ref.CHUNK) for k in p0["counts"])
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ c. the full row width
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [8185, 8192])
def test_rows_of_8192_floats(eng, metric, dim):
    """16 column slices of k_km_partial, all of k_km_finish's row buffer, a SPHERICAL chain of 8192 terms; 8185: the last slice ragged"""
    n, Cn = 300, 4
    rng = np.random.default_rng(dim)
    x = (rng.standard_normal((n, dim)) + 1.5 * rng.integers(-1, 2, (n, 1))).astype(F32)
    rows = vv.kmeans_init_rows(2, n, Cn)
    want = ref.run(x, x[rows], 2, metric, library_scores(eng, x))
    gal = eng.gallery(x)
    try:
        r = gal.kmeans(Cn, iters=2, metric=metric, init=rows)
        check_pass(r, want["passes"][2])
        assert r.objective.tolist() == [p["objective"] for p in want["passes"]]
        assert r.report["empty_last"] == want["empty_last"] and r.report["degenerate_last"] == want["degenerate_last"]
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ d. an empty cluster, carried on
@pytest.mark.parametrize("metric", METRICS)
def test_an_empty_cluster_through_later_passes(eng, metric):
    """Cluster 2 starts as cluster 0's twin, loses every tie and is empty at the first update: its centroid and (EUCLIDEAN) its nn stay.
    Pass 1 and every later one then add that nn to cluster 2's scores: a stale or rewritten nn[2] shows in assign or objective."""
    x = np.random.default_rng(6).standard_normal((500, 12)).astype(F32)
    init = np.stack([x[3], x[40], x[3]])
    gal = eng.gallery(x)
    try:
        for t in (1, 2, 3):
            want = ref.run(x, init, t, metric, library_scores(eng, x))
            r = gal.kmeans(3, iters=t, metric=metric, init=init)
            check_pass(r, want["passes"][t])
            assert r.objective.tolist() == [p["objective"] for p in want["passes"]]
            assert r.moved.tolist() == [p["moved"] for p in want["passes"]]
            assert r.report["empty_last"] == want["empty_last"] and r.report["degenerate_last"] == want["degenerate_last"]
            if t == 1:
                assert r.report["empty_last"] >= 1 and same_bits(r.centroids[2], init[2])
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ e. non-finite items
def same_bits_or_nan(got, want):
    """the stated exception: NaN where a NaN is expected (any payload and sign), equal bits everywhere else"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def same_double_or_nan(got, want):
    return math.isnan(got) if math.isnan(want) else got == want


def check_pass_nonfinite(res, st):
    assert np.array_equal(res.assign, st["assign"]), np.flatnonzero(res.assign != st["assign"])[:5]
    assert np.array_equal(res.counts, st["counts"])
    assert res.report["moved_last"] == st["moved"] == res.moved[-1]
    assert same_double_or_nan(res.report["objective_last"], st["objective"]) and same_double_or_nan(res.objective[-1], st["objective"])
    assert res.report["nonfinite_rows"] == st["nonfinite"]
    assert same_bits_or_nan(res.centroids, st["centroids"])


@pytest.mark.parametrize("metric", METRICS)
def test_nan_and_inf_items(eng, metric):
    x, init = inp.nonfinite_case()
    gal = eng.gallery(x)
    try:
        with np.errstate(all="ignore"):
            want = ref.run(x, init, 2, metric, library_scores(eng, x))
        for t in (0, 1, 2):
            st = want["passes"][t]
            assert st["nonfinite"] >= 1 and st["assign"][inp.NAN_ROW] == 0             # (the input does what it was made for)
            r = gal.kmeans(5, iters=t, metric=metric, init=init)
            check_pass_nonfinite(r, st)
            assert r.assign[inp.NAN_ROW] == 0                                           # every key NaN: cluster 0
            assert r.report["nonfinite_rows"] == st["nonfinite"] >= 1
            assert np.array_equal(r.counts, np.bincount(r.assign, minlength=5))
            assert r.moved.tolist() == [p["moved"] for p in want["passes"][:t + 1]]
            assert all(same_double_or_nan(a, p["objective"]) for a, p in zip(r.objective.tolist(), want["passes"]))
            if t:
                with np.errstate(all="ignore"):
                    _, empty, degenerate = ref.update(x, want["passes"][t - 1]["assign"], want["passes"][t - 1]["centroids"], metric)
                assert r.report["empty_last"] == empty and r.report["degenerate_last"] == degenerate
                if metric == "spherical":
                    # a sum with a NaN or an Inf has a q that is not finite: the cluster is degenerate and its centroid stays finite
                    assert degenerate >= 1 and np.isfinite(r.centroids).all()
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ f. degenerate SPHERICAL clusters
def degenerate_run(eng, x, init, Cn):
    with np.errstate(over="ignore"):
        want = ref.run(x, init, 1, "spherical", library_scores(eng, x))
    assert want["degenerate_last"] == 1 and want["empty_last"] == 0                     # (the restatement itself finds the cluster)
    gal = eng.gallery(x)
    try:
        r0 = gal.kmeans(Cn, iters=0, metric="spherical", init=init)
        check_pass(r0, want["passes"][0])
        r = gal.kmeans(Cn, iters=1, metric="spherical", init=init)
        check_pass(r, want["passes"][1])
        assert r.report["degenerate_last"] == 1 and r.report["empty_last"] == 0
        assert same_bits(r.centroids[0], init[0])
    finally:
        gal.close()
    return want, r0


def test_a_cluster_whose_sum_is_zero_keeps_its_centroid(eng):
    x, init, orth = inp.zero_sum_case()
    want, r0 = degenerate_run(eng, x, init, 2)
    assert np.array_equal(np.flatnonzero(r0.assign == 0), orth)          # the zero keys tie and go to the lower cluster; nothing else does
    assert (bits(want["passes"][0]["sel"][orth]) == 0).all()              # ... and they are +0


def test_a_cluster_whose_norm_overflows_keeps_its_centroid(eng):
    x, init, big = inp.overflow_case()
    want, r0 = degenerate_run(eng, x, init, 2)
    assert np.array_equal(np.flatnonzero(r0.assign == 0), big)
    s = ref.cluster_sum(x, big)
    with np.errstate(over="ignore"):
        assert np.isfinite(s).all() and s[0] > 3e19 and np.isinf(ref.chain_sq(s[None, :])[0])


def test_one_cluster_of_items_in_pairs(eng):
    x, init = inp.pairs_case()
    want, r0 = degenerate_run(eng, x, init, 1)
    assert r0.counts.tolist() == [len(x)]
