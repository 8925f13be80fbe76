"""GPU tests of k-means on a gallery (vv_gallery_kmeans, Gallery.kmeans) against tests/kmeans_ref.py, bit for bit.

The restatement takes its distances from scores_fn: exact host products where every key is exact in any summation order (integer
operands in [-4, 4]), otherwise the library's own stored floats (Gallery.scores on a gallery made of the restatement's OWN previous
centroids, times -2: exact).  A call returns the last pass's assignment and centroids only, so "every pass" is checked by calling
with iters = 0, 1 .. T: the call is deterministic, pass t of a longer call is the last pass of the call with iters = t.

The objective's bound against math.fsum: n additions in double, each off by at most 2^-53 of a partial sum that is at most the sum
of |key|: n * 2^-52 * sum |key| holds with a factor two to spare."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402
from videovector_amd.engine import _KmeansCfg, _KmeansReport, _ptr   # noqa: E402
from videovector_amd.synth import SyntheticVideos, init_weights   # noqa: E402

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "spherical"]
VEC, ELEMENTWISE = 1, 2


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
        return (np.float32(-2.0) * s + np.float32(0.0)).astype(np.float32)
    return fn


def int_items(n, dim, seed):
    return np.random.default_rng(seed).integers(-4, 5, (n, dim)).astype(np.float32)


def check_pass(res, st, cent_after=None):
    """the call's final pass against the restatement's pass st"""
    assert np.array_equal(res.assign, st["assign"])
    assert np.array_equal(res.counts, st["counts"])
    assert res.report["moved_last"] == st["moved"] == res.moved[-1]
    assert res.report["objective_last"] == st["objective"] == res.objective[-1]
    assert res.report["nonfinite_rows"] == st["nonfinite"]
    assert same_bits(res.centroids, st["centroids"])


# ------------------------------------------------------------------------------------------------ exactly representable operands
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("Cn", [3, 7, 64])
def test_exact_operands_one_iteration(eng, metric, Cn):
    x = int_items(1000, 40, 11 + Cn)
    rows = vv.kmeans_init_rows(5, 1000, Cn)
    want = ref.run(x, x[rows], 1, metric, ref.exact_scores(x))
    p0 = want["passes"][0]
    gal = eng.gallery(x)
    try:
        r0 = gal.kmeans(Cn, iters=0, metric=metric, init=rows)                 # pass 0: every key exact
        check_pass(r0, p0)
        assert r0.moved[0] == 1000 and r0.report["empty_last"] == 0
        assert np.array_equal(r0.counts, np.bincount(r0.assign, minlength=Cn))
        exact = math.fsum(float(v) for v in p0["sel"])
        bound = 1000 * 2.0 ** -52 * math.fsum(abs(float(v)) for v in p0["sel"])
        print("objective", r0.objective[0], "fsum", exact, "bound", bound)
        assert abs(r0.objective[0] - exact) <= bound
        assert eng.get_option("last_km_assign_form") == (VEC if Cn % 4 == 0 else ELEMENTWISE)
        r1 = gal.kmeans(Cn, iters=1, metric=metric, init=x[rows])              # the update behind it: host centroids this time
        assert r1.objective[0] == p0["objective"] and r1.moved[0] == 1000
        assert same_bits(r1.centroids, want["centroids"])
        assert r1.report["empty_last"] == want["empty_last"] and r1.report["degenerate_last"] == want["degenerate_last"]
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ general floats, step by step
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 31, 32, 33, 512])
def test_general_floats_every_pass(eng, metric, dim):
    n, Cn, T = 777, 5, 5
    rng = np.random.default_rng(100 + dim)
    x = (rng.standard_normal((n, dim)) + 2.0 * rng.integers(-1, 2, (n, 1))).astype(np.float32)
    rows = vv.kmeans_init_rows(9, n, Cn)
    want = ref.run(x, x[rows], T, metric, library_scores(eng, x))
    gal = eng.gallery(x)
    try:
        for t in range(T + 1):
            r = gal.kmeans(Cn, iters=t, metric=metric, init=rows)
            check_pass(r, want["passes"][t])
            assert r.objective.tolist() == [p["objective"] for p in want["passes"][:t + 1]]
            assert r.moved.tolist() == [p["moved"] for p in want["passes"][:t + 1]]
        assert r.report["empty_last"] == want["empty_last"] and r.report["degenerate_last"] == want["degenerate_last"]
    finally:
        gal.close()


@pytest.mark.parametrize("metric", METRICS)
def test_more_than_one_column_slice(eng, metric):
    """dim 600: rows of 608 floats, so k_km_partial runs two column slices (512 + 96 columns) and k_km_finish walks past 512."""
    n, Cn, dim = 300, 4, 600
    rng = np.random.default_rng(61)
    x = (rng.standard_normal((n, dim)) + 1.5 * rng.integers(-1, 2, (n, 1))).astype(np.float32)
    rows = vv.kmeans_init_rows(2, n, Cn)
    want = ref.run(x, x[rows], 2, metric, library_scores(eng, x))
    gal = eng.gallery(x)
    try:
        r = gal.kmeans(Cn, iters=2, metric=metric, init=rows)
        check_pass(r, want["passes"][2])
        assert r.objective.tolist() == [p["objective"] for p in want["passes"]]
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ chunk edges
@pytest.mark.parametrize("metric", METRICS)
def test_chunk_edges(eng, metric):
    sizes = [255, 256, 257, 513]
    rng = np.random.default_rng(3)
    member = rng.permutation(np.repeat(np.arange(4), sizes)).astype(np.int32)         # interleaved in item order
    centres = 10.0 * np.eye(4, 16, dtype=np.float32)
    x = (centres[member] + 0.3 * rng.standard_normal((len(member), 16))).astype(np.float32)
    init = np.array([np.flatnonzero(member == k)[0] for k in range(4)], np.int32)
    want = ref.run(x, x[init], 2, metric, library_scores(eng, x))
    gal = eng.gallery(x)
    try:
        r = gal.kmeans(4, iters=2, metric=metric, init=init)
        check_pass(r, want["passes"][2])
        assert np.array_equal(r.assign, member) and r.counts.tolist() == sizes
        assert eng.get_option("last_km_chunks") == 1 + 1 + 2 + 3
        assert r.moved.tolist() == [len(member), 0, 0]
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ blocking
@pytest.mark.parametrize("metric", METRICS)
def test_block_rows_do_not_change_a_bit(eng, metric):
    rng = np.random.default_rng(21)
    x = rng.standard_normal((1000, 24)).astype(np.float32)
    gal = eng.gallery(x)
    try:
        a = gal.kmeans(6, iters=3, metric=metric, seed=2)
        assert eng.get_option("last_km_blocks") == 1
        eng.set_option("km_block_rows", 64)
        try:
            b = gal.kmeans(6, iters=3, metric=metric, seed=2)
            assert eng.get_option("last_km_blocks") == 16 > 1
        finally:
            eng.set_option("km_block_rows", 0)
        assert same_bits(a.centroids, b.centroids) and np.array_equal(a.assign, b.assign) and np.array_equal(a.counts, b.counts)
        assert a.objective.tolist() == b.objective.tolist() and a.moved.tolist() == b.moved.tolist()
    finally:
        gal.close()


def test_more_blocks_than_timed_ones(eng):
    """2000 blocks of 64 rows: more than the 1024 whose legs get events of their own -- the same bits, and four legs that are times"""
    x = int_items(128000, 8, 9)
    rows = vv.kmeans_init_rows(4, len(x), 3)
    gal = eng.gallery(x)
    try:
        a = gal.kmeans(3, iters=1, init=rows)
        eng.set_option("km_block_rows", 64)
        try:
            b = gal.kmeans(3, iters=1, init=rows)
            assert eng.get_option("last_km_blocks") == 2000
            legs = [eng.get_option("last_km_%s_ms" % k) for k in ("sim", "assign", "group", "update")]
            assert all(0 < v < 10000 for v in legs), legs
        finally:
            eng.set_option("km_block_rows", 0)
        assert same_bits(a.centroids, b.centroids) and np.array_equal(a.assign, b.assign)
        assert a.objective.tolist() == b.objective.tolist() and a.moved.tolist() == b.moved.tolist()
    finally:
        gal.close()


def test_past_one_grid_pass_and_two_calls(eng):
    n, Cn = 70001, 5
    x = int_items(n, 8, 77)
    rows = vv.kmeans_init_rows(1, n, Cn)
    want = ref.run(x, x[rows], 1, "euclidean", ref.exact_scores(x))
    gal = eng.gallery(x)
    try:
        r0 = gal.kmeans(Cn, iters=0, init=rows)
        check_pass(r0, want["passes"][0])
        a = gal.kmeans(Cn, iters=2, init=rows)
        b = gal.kmeans(Cn, iters=2, init=rows)
        assert same_bits(a.centroids, b.centroids) and np.array_equal(a.assign, b.assign) and np.array_equal(a.counts, b.counts)
        assert a.objective.tolist() == b.objective.tolist() and a.moved.tolist() == b.moved.tolist()
        assert a.objective[0] == want["passes"][0]["objective"]
        one = gal.kmeans(Cn, iters=1, init=rows)
        assert same_bits(one.centroids, want["centroids"])
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("metric", METRICS)
def test_one_cluster(eng, metric):
    x = np.random.default_rng(4).standard_normal((300, 9)).astype(np.float32) + np.float32(1.5)
    want = ref.run(x, x[[7]], 2, metric, library_scores(eng, x))
    gal = eng.gallery(x)
    try:
        r = gal.kmeans(1, iters=2, metric=metric, init=np.array([7]))
        check_pass(r, want["passes"][2])
        assert r.counts.tolist() == [300] and r.moved.tolist() == [300, 0, 0]
    finally:
        gal.close()


def test_every_item_its_own_cluster(eng):
    x = np.unique(int_items(400, 8, 8), axis=0)
    n = len(x)
    x = x[np.random.default_rng(1).permutation(n)]
    perm = vv.kmeans_init_rows(3, n, n)
    gal = eng.gallery(x)
    try:
        r = gal.kmeans(n, iters=1, init=perm)
        assert same_bits(r.centroids, x[perm])
        assert r.moved.tolist() == [n, 0] and r.counts.tolist() == [1] * n
        assert np.array_equal(perm[r.assign], np.arange(n))
    finally:
        gal.close()


@pytest.mark.parametrize("metric", METRICS)
def test_4096_clusters(eng, metric):
    n, Cn = 4200, 4096
    x = int_items(n, 8, 5)
    rows = vv.kmeans_init_rows(12, n, Cn)
    want = ref.run(x, x[rows], 1, metric, ref.exact_scores(x))
    gal = eng.gallery(x)
    try:
        r0 = gal.kmeans(Cn, iters=0, metric=metric, init=rows)
        check_pass(r0, want["passes"][0])
        r1 = gal.kmeans(Cn, iters=1, metric=metric, init=rows)
        assert same_bits(r1.centroids, want["centroids"]) and r1.report["empty_last"] == want["empty_last"]
        assert eng.get_option("last_km_assign_form") == VEC
    finally:
        gal.close()


@pytest.mark.parametrize("metric", METRICS)
def test_identical_initial_centroids(eng, metric):
    rng = np.random.default_rng(6)
    x = rng.standard_normal((500, 12)).astype(np.float32)
    init = np.stack([x[3], x[40], x[3]])                                   # cluster 2 == cluster 0: never the lowest index at its tie
    gal = eng.gallery(x)
    try:
        r = gal.kmeans(3, iters=0, metric=metric, init=init)               # the pass against the twins: every tie goes to cluster 0
        assert r.counts[2] == 0 and r.counts[0] > 0 and not (r.assign == 2).any()
        r = gal.kmeans(3, iters=1, metric=metric, init=init)               # its update: cluster 2 is empty and stays, cluster 0 moves
        assert r.report["empty_last"] == 1 and same_bits(r.centroids[2], init[2]) and not same_bits(r.centroids[0], init[0])
    finally:
        gal.close()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
@pytest.mark.parametrize("Cn", [2, 4])                                     # both forms
def test_exact_tie_goes_to_the_lower_cluster(eng, order, Cn):
    cents = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, -1]], np.float32)[:Cn]
    cents[[0, 1]] = cents[list(order)]
    x = np.array([[0, 5, 2, 0], [3, 0, 0, 0], [-3, 0, 0, 0], [0, -1, 7, 0]], np.float32)   # items 0 and 3: the same key for every centroid
    gal = eng.gallery(x)
    try:
        for metric in METRICS:
            r = gal.kmeans(Cn, iters=0, metric=metric, init=cents)
            assert r.assign[0] == 0 and r.assign[3] == 0
            assert r.assign[1] == order.index(0) and r.assign[2] == order.index(1)
        assert eng.get_option("last_km_assign_form") == (VEC if Cn % 4 == 0 else ELEMENTWISE)
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ invariants
def test_spherical_assignment_is_topk_of_the_centroid_gallery(eng):
    rng = np.random.default_rng(31)
    x = rng.standard_normal((900, 20)).astype(np.float32)
    gal = eng.gallery(x)
    try:
        r = gal.kmeans(11, iters=4, metric="spherical", seed=4)
        cg = r.gallery()
        try:
            idx, dist = cg.topk(x, 1)
        finally:
            cg.close()
        assert np.array_equal(idx[:, 0], r.assign)
        assert np.array_equal(r.counts, np.bincount(r.assign, minlength=11))
        assert r.report["objective_last"] == ref.objective_of(dist[:, 0])
    finally:
        gal.close()


@pytest.mark.parametrize("metric", METRICS)
def test_a_converged_run_stays_put(eng, metric):
    rng = np.random.default_rng(8)
    member = rng.integers(0, 5, 600)
    x = (8.0 * np.eye(5, 10, dtype=np.float32)[member] + 0.5 * rng.standard_normal((600, 10))).astype(np.float32)
    gal = eng.gallery(x)
    try:
        init = np.array([np.flatnonzero(member == k)[0] for k in range(5)], np.int32)
        r = gal.kmeans(5, iters=12, metric=metric, init=init)
        still = np.flatnonzero(r.moved == 0)
        assert len(still) and still[0] < 12
        t = int(still[0])
        assert (r.moved[t:] == 0).all() and len(set(r.objective[t:].tolist())) == 1
        s = gal.kmeans(5, iters=t, metric=metric, init=init)
        assert same_bits(s.centroids, r.centroids) and np.array_equal(s.assign, r.assign)
        assert np.array_equal(r.counts, np.bincount(r.assign, minlength=5))
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ errors and training state
def raw_call(eng, gal_handle, cfg, cent0, rows0, n, Cn, passes, dim, null=()):
    """vv_gallery_kmeans with outputs filled with a sentinel -> (rc, outputs); null: of "cent", "report", the pointers passed as NULL"""
    outs = dict(cent=np.full((max(Cn, 1), dim), -7.5, np.float32), assign=np.full(n, -9, np.int32), counts=np.full(max(Cn, 1), -9, np.int32),
                obj=np.full(passes, -7.5), moved=np.full(passes, -9, np.int64))
    rep = _KmeansReport()
    rep.n = -9
    rc = eng.L.vv_gallery_kmeans(eng.h, gal_handle, None if cfg is None else C.byref(cfg), _ptr(cent0), _ptr(rows0),
                                 None if "cent" in null else _ptr(outs["cent"]), _ptr(outs["assign"]), _ptr(outs["counts"]),
                                 _ptr(outs["obj"]), _ptr(outs["moved"]), None if "report" in null else C.byref(rep))
    outs["rep_n"] = rep.n
    return rc, outs


def test_every_refusal_leaves_the_outputs(eng):
    n, dim = 50, 6
    x = np.random.default_rng(2).standard_normal((n, dim)).astype(np.float32)
    gal = eng.gallery(x)
    other = vv.Engine(0, "f16")
    foreign = other.gallery(x)

    def cfg(Cn=4, iters=2, metric=0):
        k = _KmeansCfg()
        eng.L.vv_kmeans_cfg_default(C.byref(k))
        assert (k.num_clusters, k.iters, k.metric) == (0, 20, 0)
        k.num_clusters, k.iters, k.metric = Cn, iters, metric
        return k

    rows4, cent4 = np.arange(4, dtype=np.int32), x[:4].copy()
    bad_rows = np.array([0, 1, n, 2], np.int32)
    cases = [
        ("NULL cfg", gal.h, None, None, rows4, 4, "NULL argument"),
        ("NULL gallery", None, cfg(), None, rows4, 4, "NULL argument"),
        ("NULL centroids_out", gal.h, cfg(), None, rows4, 4, "NULL argument", ("cent",)),
        ("NULL report", gal.h, cfg(), None, rows4, 4, "NULL argument", ("report",)),
        # the traces' record of 2^31 passes is 80 GiB: past the scratch limit, found before anything is allocated
        ("record past the scratch limit", gal.h, cfg(iters=2 ** 31 - 1), None, rows4, 4, "scratch limit"),
        ("both inits", gal.h, cfg(), cent4, rows4, 4, "exactly one"),
        ("neither init", gal.h, cfg(), None, None, 4, "exactly one"),
        ("another context", foreign.h, cfg(), None, rows4, 4, "another context"),
        ("no clusters", gal.h, cfg(Cn=0), None, rows4, 0, "num_clusters = 0"),
        ("too many clusters", gal.h, cfg(Cn=4097), None, np.zeros(4097, np.int32), 4097, "num_clusters = 4097"),
        ("more clusters than items", gal.h, cfg(Cn=n + 1), None, np.zeros(n + 1, np.int32), n + 1, "exceeds"),
        ("negative iters", gal.h, cfg(iters=-1), None, rows4, 4, "iters = -1"),
        ("unknown metric", gal.h, cfg(metric=2), None, rows4, 4, "unknown metric 2"),
        ("row past the end", gal.h, cfg(), None, bad_rows, 4, "init_rows[2] = %d" % n),
        ("negative row", gal.h, cfg(), None, np.array([0, -1, 2, 3], np.int32), 4, "init_rows[1] = -1"),
    ]
    try:
        for name, handle, k, c0, r0, Cn, word, *null in cases:
            rc, outs = raw_call(eng, handle, k, c0, r0, n, Cn, 3, dim, null=null[0] if null else ())
            assert rc == 1, name                                             # VV_ERR_ARG
            assert word in eng.L.vv_last_error().decode(), (name, eng.L.vv_last_error())
            assert (outs["cent"] == -7.5).all() and (outs["assign"] == -9).all() and (outs["counts"] == -9).all(), name
            assert (outs["obj"] == -7.5).all() and (outs["moved"] == -9).all() and outs["rep_n"] == -9, name
        rc, outs = raw_call(eng, gal.h, cfg(), None, rows4, n, 4, 3, dim)        # ... and the same call with nothing wrong runs
        assert rc == 0 and outs["rep_n"] == n and outs["moved"][0] == n
        with pytest.raises(vv.VVError):
            vv.kmeans_init_rows(1, 10, 11)
    finally:
        foreign.close(); other.close(); gal.close()


def test_a_call_between_backward_and_update_changes_nothing():
    ds = SyntheticVideos(seed=1701, n_videos=50)
    idx = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=32, context_size=5, num_negative_samples=2, max_buffer_size=500,
                     negative_swap_percentage=50).next()
    W0, b0 = init_weights(1, 32, 128, std=0.02)
    cfg = vv.StepConfig(32, 5, 2, lr=0.01)
    x = np.random.default_rng(2).standard_normal((300, 32)).astype(np.float32)
    outs = []
    for with_kmeans in (False, True):
        e = vv.Engine(0, "f16")
        e.table_synth(ds.seed, ds.n_rows, 128)
        e.params_set(W0, b0)
        e.forward_backward(cfg, idx)
        if with_kmeans:
            g = e.gallery(x)
            g.kmeans(7, iters=3)
            g.close()
        e.apply_update(cfg)
        outs.append(e.params_get())
        e.close()
    assert all(np.array_equal(u, v) for u, v in zip(outs[0], outs[1]))
