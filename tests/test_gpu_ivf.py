"""vv_ivf_* on the device, bit for bit: idx equal and dist equal as bits.  With every cluster probed the search must BE vv_gallery_topk
(the grouped similarity kernel runs k_sim_f32's tile body, so the same query and item give the same float wherever the item's row
lies); with fewer it must be tests/ivf_ref.py on the library's own stored floats -- probe order, candidate sets, counts, tiles."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_ref as ref   # noqa: E402
import kmeans_ref   # noqa: E402

import videovector_amd as vv   # noqa: E402
from videovector_amd.engine import _ptr   # noqa: E402
from videovector_amd.synth import SyntheticVideos, init_weights   # noqa: E402

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "spherical"]
F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    """(idx, dist) pairs: idx equal, dist equal as bits"""
    return np.array_equal(got[0], want[0]) and got[1].shape == want[1].shape and np.array_equal(bits(got[1]), bits(want[1]))


def stored(eng, rows, q):
    """the floats k_sim_f32 stores for q against `rows`, as Gallery.scores hands them out"""
    g = eng.gallery(rows)
    try:
        s = g.scores(q).get()
    finally:
        g.close()
    return (F32(-2.0) * s + F32(0.0)).astype(F32)


def restated(eng, x, cent, metric, assign, q, nprobe, k, block_rows=None):
    start, lst = ref.lists_of(assign, cent.shape[0])
    return ref.search(stored(eng, x, q), stored(eng, cent, q), kmeans_ref.chain_sq(cent), metric, start, lst, nprobe, k, block_rows)


def check(ix, q, k, nprobe, want):
    idx, dist, m = ix.search(q, k, nprobe)
    assert np.array_equal(idx, want["idx"]), np.argwhere(idx != want["idx"])[:5]
    assert np.array_equal(bits(dist), bits(want["dist"]))
    assert np.array_equal(m, want["n_candidates"])
    assert ix.get("last_tiles") == want["tiles"] and ix.get("last_candidates") == want["candidates"]


# ------------------------------------------------------------------------------------------------ nprobe = C is vv_gallery_topk
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("Cn", [1, 3, 64])
@pytest.mark.parametrize("dim", [1, 31, 32, 33, 512])
def test_every_cluster_probed_is_topk(eng, metric, Cn, dim):
    n, n_q = 1000, 150
    rng = np.random.default_rng(dim * 100 + Cn)
    x = rng.standard_normal((n, dim)).astype(F32)
    q = rng.standard_normal((n_q, dim)).astype(F32)
    gal = eng.gallery(x)
    ix = eng.ivf(gal, x[:Cn], metric=metric, assign=rng.integers(0, Cn, n).astype(np.int32))
    try:
        for k in (1, 5, 32):
            idx, dist, m = ix.search(q, k, Cn)
            assert same((idx, dist), gal.topk(q, k)), k
            assert (m == n).all() and ix.get("last_candidates") == n * n_q
    finally:
        ix.close(); gal.close()


# ------------------------------------------------------------------------------------------------ against the restatement
SIZES = [0, 1, 127, 128, 129, 300, 15, 0]              # the lists of the explicit assignment: n = 700 in C = 8


@pytest.fixture(scope="module")
def lists_case(eng):
    rng = np.random.default_rng(11)
    n, dim = sum(SIZES), 64
    x = rng.standard_normal((n, dim)).astype(F32)
    cent = rng.standard_normal((len(SIZES), dim)).astype(F32)
    assign = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES)).astype(np.int32)
    q = rng.standard_normal((300, dim)).astype(F32)
    d_items, d_cent = stored(eng, x, q), stored(eng, cent, q)
    gal = eng.gallery(x)
    idxs = {m: eng.ivf(gal, cent, metric=m, assign=assign) for m in METRICS}
    yield dict(x=x, cent=cent, assign=assign, q=q, d_items=d_items, d_cent=d_cent, nn=kmeans_ref.chain_sq(cent), ix=idxs,
               lists=ref.lists_of(assign, len(SIZES)))
    for ix in idxs.values():
        ix.close()
    gal.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_q", [1, 127, 128, 129, 300])
def test_lists_of_every_edge_size(lists_case, metric, n_q):
    c = lists_case
    start, lst = c["lists"]
    assert (start[1:] - start[:-1]).tolist() == SIZES
    got_start, got_lst = c["ix"][metric].lists()
    assert np.array_equal(got_start, start) and np.array_equal(got_lst, lst)
    assert c["ix"][metric].get("largest_list") == 300 and c["ix"][metric].get("empty_lists") == 2
    for nprobe in (1, 2, 7):
        want = ref.search(c["d_items"][:n_q], c["d_cent"][:n_q], c["nn"], metric, start, lst, nprobe, 10)
        check(c["ix"][metric], c["q"][:n_q], 10, nprobe, want)


@pytest.mark.parametrize("metric", METRICS)
def test_clusters_probed_by_0_1_128_and_129_queries(eng, metric):
    rng = np.random.default_rng(3)
    n, dim, Cn = 500, 64, 4
    cent = rng.standard_normal((Cn, dim)).astype(F32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True).astype(F32)           # a copy of a centroid is nearest to it under either metric
    x = rng.standard_normal((n, dim)).astype(F32)
    assign = rng.integers(0, Cn, n).astype(np.int32)
    q = np.concatenate([cent[1:2], np.repeat(cent[2:3], 128, 0), np.repeat(cent[3:4], 129, 0)])
    q = q[rng.permutation(len(q))]
    gal = eng.gallery(x)
    ix = eng.ivf(gal, cent, metric=metric, assign=assign)
    try:
        want = restated(eng, x, cent, metric, assign, q, 1, 7)
        per = np.bincount([p[0] for p in want["probes"]], minlength=Cn)
        assert per.tolist() == [0, 1, 128, 129]
        check(ix, q, 7, 1, want)
    finally:
        ix.close(); gal.close()


# ------------------------------------------------------------------------------------------------ order, short lists, NaN keys
@pytest.mark.parametrize("metric", METRICS)
def test_equal_distances_order_by_item_index_across_clusters(eng, metric):
    # integer operands: every distance is exact.  Items come in exact duplicates; the HIGHER index of every pair lies in cluster 0,
    # which the query probes first, the lower one in cluster 1
    rng = np.random.default_rng(8)
    dim, pairs = 8, 20
    base = rng.integers(-3, 4, (pairs, dim)).astype(F32)
    x = np.concatenate([base, base])                                         # item i and item i + pairs are the same row
    assign = np.concatenate([np.ones(pairs), np.zeros(pairs)]).astype(np.int32)
    cent = np.zeros((3, dim), F32)                                           # (a third centroid far away, its list empty: the probe has to select)
    cent[0, 0], cent[1, 0], cent[2, 0] = 1, -1, -6
    q = rng.integers(-3, 4, (9, dim)).astype(F32)
    q[:, 0] = 2                                                              # nearer to centroid 0 under either metric
    gal = eng.gallery(x)
    ix = eng.ivf(gal, cent, metric=metric, assign=assign)
    try:
        want = restated(eng, x, cent, metric, assign, q, 2, 6)
        assert all(p == [0, 1] for p in want["probes"])
        idx, dist, _ = ix.search(q, 6, 2)
        exact = (-2.0 * (q.astype(np.float64) @ x.T.astype(np.float64))).astype(F32)
        for i in range(len(q)):
            # the nearest item and its duplicate tie, and the lowest index of a tie is the copy in cluster 1, which is probed second
            assert dist[i, 0] == dist[i, 1] and idx[i, 0] < pairs and idx[i, 0] < idx[i, 1]
            assert all(dist[i, j] < dist[i, j + 1] or (dist[i, j] == dist[i, j + 1] and idx[i, j] < idx[i, j + 1]) for j in range(5))
            assert all((idx[i, j] + pairs) % (2 * pairs) in idx[i] for j in range(6) if dist[i, j] < dist[i, 5])
            assert np.array_equal(dist[i], exact[i, idx[i]])
        check(ix, q, 6, 2, want)
        assert same((idx, dist), gal.topk(q, 6))
    finally:
        ix.close(); gal.close()


@pytest.mark.parametrize("metric", METRICS)
def test_k_above_the_candidates(eng, metric):
    rng = np.random.default_rng(4)
    n, dim, Cn = 40, 16, 4
    cent = rng.standard_normal((Cn, dim)).astype(F32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True).astype(F32)
    x = rng.standard_normal((n, dim)).astype(F32)
    assign = np.zeros(n, np.int32)
    assign[:3] = 1                                                           # cluster 1: three items; clusters 2 and 3: none
    q = np.stack([cent[2], cent[1], cent[3]])
    gal = eng.gallery(x)
    ix = eng.ivf(gal, cent, metric=metric, assign=assign)
    try:
        idx, dist, m = ix.search(q, 5, 1)
        assert m.tolist() == [0, 3, 0]
        assert (idx[[0, 2]] == -1).all() and (bits(dist[[0, 2]]) == 0).all()
        assert sorted(idx[1, :3].tolist()) == [0, 1, 2] and (idx[1, 3:] == -1).all() and (bits(dist[1, 3:]) == 0).all()
        check(ix, q, 5, 1, restated(eng, x, cent, metric, assign, q, 1, 5))
        assert ix.get("last_tiles") == 1 and ix.get("empty_lists") == 2
    finally:
        ix.close(); gal.close()


@pytest.mark.parametrize("metric", METRICS)
def test_fewer_keys_than_nprobe_are_numbers(eng, metric):
    rng = np.random.default_rng(6)
    n, dim, Cn = 200, 16, 6
    cent = rng.standard_normal((Cn, dim)).astype(F32)
    cent[[1, 3, 4], 5] = np.nan                                              # every key of clusters 1, 3 and 4 is NaN
    x = rng.standard_normal((n, dim)).astype(F32)
    assign = rng.integers(0, Cn, n).astype(np.int32)
    q = rng.standard_normal((70, dim)).astype(F32)
    gal = eng.gallery(x)
    ix = eng.ivf(gal, cent, metric=metric, assign=assign)
    try:
        for nprobe in (2, 3, 4, 5):
            want = restated(eng, x, cent, metric, assign, q, nprobe, 8)
            for p in want["probes"]:                                         # the three numbers first, then the lowest NaN clusters
                assert set(p[:3]) <= {0, 2, 5} and len(set(p)) == nprobe and p[3:] == [1, 3][:max(nprobe - 3, 0)]
            check(ix, q, 8, nprobe, want)
    finally:
        ix.close(); gal.close()


# ------------------------------------------------------------------------------------------------ blocks, grid, repeat
@pytest.mark.parametrize("metric", METRICS)
def test_block_rows_and_grid_do_not_change_a_bit(eng, lists_case, metric):
    c, ix = lists_case, lists_case["ix"][metric]
    try:
        first = ix.search(c["q"], 10, 7)
        assert ix.get("last_blocks") == 1 and ix.get("last_grid_wgs") == 512
        again = ix.search(c["q"], 10, 7)
        assert same(first, again) and np.array_equal(first[2], again[2])
        eng.set_option("ivf_block_rows", 64)
        got = ix.search(c["q"], 10, 7)
        assert ix.get("last_blocks") == 5 and same(first, got) and np.array_equal(first[2], got[2])
        start, lst = c["lists"]
        assert ix.get("last_tiles") == ref.search(c["d_items"], c["d_cent"], c["nn"], metric, start, lst, 7, 10, block_rows=64)["tiles"]
        eng.set_option("ivf_block_rows", 0)
        for wgs in (1, 3):
            eng.set_option("ivf_grid_wgs", wgs)
            got = ix.search(c["q"], 10, 7)
            assert ix.get("last_grid_wgs") == wgs and ix.get("last_tiles") > wgs and ix.get("last_blocks") == 1
            assert same(first, got) and np.array_equal(first[2], got[2])
        assert all(ix.get("last_%s_ms" % leg) >= 0 for leg in ("probe", "group", "sim", "select")) and ix.get("last_device_ms") > 0
    finally:
        eng.set_option("ivf_block_rows", 0); eng.set_option("ivf_grid_wgs", 0)


@pytest.mark.parametrize("metric", METRICS)
def test_4096_clusters_64_probes(eng, metric):
    rng = np.random.default_rng(9)
    n, dim, Cn, n_q = 8192, 32, 4096, 130
    x = rng.standard_normal((n, dim)).astype(F32)
    q = rng.standard_normal((n_q, dim)).astype(F32)
    cent = x[rng.permutation(n)[:Cn]].copy()
    gal = eng.gallery(x)
    ix = eng.ivf(gal, cent, metric=metric)
    try:
        km = gal.kmeans(Cn, iters=0, metric=metric, init=cent)
        check(ix, q, 32, 64, restated(eng, x, cent, metric, km.assign, q, 64, 32))
    finally:
        ix.close(); gal.close()


# ------------------------------------------------------------------------------------------------ the index's own assignment, its lifetime
@pytest.mark.parametrize("metric", METRICS)
def test_own_assignment_is_kmeans_with_no_iteration(eng, metric):
    rng = np.random.default_rng(12)
    n, dim, Cn = 900, 40, 9
    x = rng.standard_normal((n, dim)).astype(F32)
    cent = x[:Cn].copy()
    gal = eng.gallery(x)
    km = gal.kmeans(Cn, iters=0, metric=metric, init=cent)
    a, b = eng.ivf(gal, cent, metric=metric), km.ivf(gal)
    try:
        start, lst = ref.lists_of(km.assign, Cn)
        for ix in (a, b):
            s, l = ix.lists()
            assert np.array_equal(s, start) and np.array_equal(l, lst)
            assert ix.get("metric") == vv.engine.KMEANS_METRICS[metric] and ix.get("num_clusters") == Cn
            assert ix.get("n_ref") == n and ix.get("dim") == dim
    finally:
        a.close(); b.close(); gal.close()


def test_the_index_outlives_its_items_gallery(eng):
    rng = np.random.default_rng(13)
    x = rng.standard_normal((600, 48)).astype(F32)
    q = rng.standard_normal((33, 48)).astype(F32)
    gal = eng.gallery(x)
    ix = eng.ivf(gal, x[:5], assign=rng.integers(0, 5, 600).astype(np.int32))
    try:
        before, exact = ix.search(q, 4, 2), gal.topk(q, 4)
        gal.close()
        filler = eng.gallery(np.zeros((600, 48), F32))                       # whatever takes the freed rows' place
        assert same(ix.search(q, 4, 2), before) and same(ix.search(q, 4, 5), exact)
        filler.close()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ errors and training state
def test_every_refusal_leaves_the_outputs(eng):
    n, dim, Cn = 50, 6, 4
    rng = np.random.default_rng(2)
    x = rng.standard_normal((n, dim)).astype(F32)
    cent = x[:Cn].copy()
    q = rng.standard_normal((3, dim)).astype(F32)
    assign = rng.integers(0, Cn, n).astype(np.int32)
    gal = eng.gallery(x)
    other = vv.Engine(0, "f16")
    foreign = other.gallery(x)
    ix = eng.ivf(gal, cent, assign=assign)
    foreign_ix = other.ivf(foreign, cent, assign=assign)
    L = eng.L
    big_gal = eng.gallery(np.zeros((4100, 2), F32))
    try:
        # ---- vv_ivf_create
        bad_hi, bad_lo = assign.copy(), assign.copy()
        bad_hi[17], bad_lo[31] = Cn, -1
        creates = [
            ("NULL items", None, cent, Cn, 0, assign, False, "items is NULL"),
            ("NULL centroids", gal.h, None, Cn, 0, assign, False, "centroids is NULL"),
            ("NULL out", gal.h, cent, Cn, 0, assign, True, "out is NULL"),
            ("another context", foreign.h, cent, Cn, 0, assign, False, "another context"),
            ("no clusters", gal.h, cent, 0, 0, assign, False, "C = 0"),
            ("too many clusters", big_gal.h, cent, 4097, 0, None, False, "C = 4097"),
            ("more clusters than items", gal.h, cent, n + 1, 0, None, False, "exceeds"),
            ("unknown metric", gal.h, cent, Cn, 2, assign, False, "unknown metric 2"),
            ("entry past the clusters", gal.h, cent, Cn, 0, bad_hi, False, "assign[17] = %d" % Cn),
            ("negative entry", gal.h, cent, Cn, 1, bad_lo, False, "assign[31] = -1"),
        ]
        for name, items, ce, cn, metric, asg, null_out, word in creates:
            h = C.c_void_p(0x5a5a)
            rc = L.vv_ivf_create(eng.h, items, _ptr(ce), cn, metric, _ptr(asg), None if null_out else C.byref(h))
            assert rc == 1, name                                             # VV_ERR_ARG
            assert word in L.vv_last_error().decode(), (name, L.vv_last_error())
            assert h.value == 0x5a5a, name
        # ---- vv_ivf_search: the outputs keep their fill, the index its record of the last search
        ix.search(q, 2, 2)
        last = {k: ix.get(k) for k in ("last_blocks", "last_tiles", "last_candidates", "last_grid_wgs", "last_device_ms", "last_sim_ms")}
        searches = [
            ("NULL index", None, q, 3, 2, 2, (), "index is NULL"),
            ("NULL q", ix.h, None, 3, 2, 2, (), "q is NULL"),
            ("NULL idx", ix.h, q, 3, 2, 2, ("idx",), "idx is NULL"),
            ("NULL dist", ix.h, q, 3, 2, 2, ("dist",), "dist is NULL"),
            ("another context", foreign_ix.h, q, 3, 2, 2, (), "another context"),
            ("no query", ix.h, q, 0, 2, 2, (), "n_q = 0"),
            ("negative n_q", ix.h, q, -1, 2, 2, (), "n_q = -1"),
            ("no probe", ix.h, q, 3, 0, 2, (), "nprobe = 0"),
            ("more probes than clusters", ix.h, q, 3, Cn + 1, 2, (), "nprobe = %d" % (Cn + 1)),
            ("no k", ix.h, q, 3, 2, 0, (), "k = 0"),
            ("k past the limit", ix.h, q, 3, 2, 33, (), "k = 33"),
        ]
        for name, handle, qq, n_q, nprobe, k, null, word in searches:
            idx, dist, m = np.full((3, 33), -9, np.int32), np.full((3, 33), -7.5, F32), np.full(3, -9, np.int32)
            rc = L.vv_ivf_search(eng.h, handle, _ptr(qq), n_q, nprobe, k, None if "idx" in null else _ptr(idx),
                                 None if "dist" in null else _ptr(dist), _ptr(m))
            assert rc == 1, name
            assert word in L.vv_last_error().decode(), (name, L.vv_last_error())
            assert (idx == -9).all() and (dist == -7.5).all() and (m == -9).all(), name
            assert {k_: ix.get(k_) for k_ in last} == last, name
        # nprobe between 64 and C, on an index of more than 64 clusters
        wide = eng.ivf(big_gal, np.zeros((100, 2), F32), assign=np.zeros(4100, np.int32))
        try:
            idx, dist = np.full((1, 2), -9, np.int32), np.full((1, 2), -7.5, F32)
            assert L.vv_ivf_search(eng.h, wide.h, _ptr(np.zeros((1, 2), F32)), 1, 65, 2, _ptr(idx), _ptr(dist), None) == 1
            assert "nprobe = 65" in L.vv_last_error().decode() and (idx == -9).all() and (dist == -7.5).all()
            assert wide.search(np.zeros((1, 2), F32), 2, 64)[0].tolist() == [[0, 1]]
            assert wide.search(np.zeros((1, 2), F32), 2, 100)[0].tolist() == [[0, 1]]
        finally:
            wide.close()
        # dim not the index's, an unknown name, and the other calls' own refusals
        with pytest.raises(vv.VVError):
            ix.search(np.zeros((3, dim + 1), F32), 2, 2)
        with pytest.raises(vv.VVError):
            ix.get("no_such_name")
        v = C.c_double(-3.0)
        assert L.vv_ivf_get(ix.h, b"no_such_name", C.byref(v)) == 1 and v.value == -3.0 and b"no_such_name" in L.vv_last_error()
        s, l = np.full(Cn + 1, -9, np.int32), np.full(n, -9, np.int32)
        assert L.vv_ivf_lists(eng.h, foreign_ix.h, _ptr(s), _ptr(l)) == 1 and (s == -9).all() and (l == -9).all()
        assert L.vv_ivf_destroy(eng.h, foreign_ix.h) == 1 and b"another context" in L.vv_last_error()
        # ... and the same calls with nothing wrong run
        idx, dist, m = ix.search(q, 2, 2)
        assert (idx >= 0).all() and (m > 0).all()
    finally:
        ix.close(); foreign_ix.close(); big_gal.close(); foreign.close(); other.close(); gal.close()


def test_a_search_between_backward_and_update_changes_nothing():
    ds = SyntheticVideos(seed=1701, n_videos=50)
    idx = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=32, context_size=5, num_negative_samples=2, max_buffer_size=500,
                     negative_swap_percentage=50).next()
    W0, b0 = init_weights(1, 32, 128, std=0.02)
    cfg = vv.StepConfig(32, 5, 2, lr=0.01)
    x = np.random.default_rng(2).standard_normal((300, 32)).astype(F32)
    outs = []
    for with_ivf in (False, True):
        e = vv.Engine(0, "f16")
        e.table_synth(ds.seed, ds.n_rows, 128)
        e.params_set(W0, b0)
        e.forward_backward(cfg, idx)
        if with_ivf:
            g = e.gallery(x)
            ix = e.ivf(g, x[:7])
            ix.search(x[:40], 5, 3)
            ix.close(); g.close()
        e.apply_update(cfg)
        outs.append(e.params_get())
        e.close()
    assert all(np.array_equal(u, v) for u, v in zip(outs[0], outs[1]))
