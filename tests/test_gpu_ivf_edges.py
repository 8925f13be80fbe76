"""vv_ivf_* at the cluster counts tests/test_gpu_ivf.py leaves out, bit for bit: more than 64 and fewer than 4096 clusters, where
k_ivf_probe's sweep over C ends in a ragged stride of 64, k_km_starts and k_ivf_tiles give a thread several clusters or none, and
k_km_scan's last workgroup is partly filled; every cluster probed through hundreds of probes; NaN keys on both sides of a stride's
edge; and one query block whose (query, cluster) pairs fill more than eight grouping tiles.  With every cluster probed the search must
be vv_gallery_topk; with fewer it must be tests/ivf_ref.py on the library's own stored floats."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_ref as ref   # noqa: E402
import kmeans_ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

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


def check(ix, q, k, nprobe, want):
    idx, dist, m = ix.search(q, k, nprobe)
    assert np.array_equal(idx, want["idx"]), np.argwhere(idx != want["idx"])[:5]
    assert np.array_equal(bits(dist), bits(want["dist"]))
    assert np.array_equal(m, want["n_candidates"])
    assert ix.get("last_tiles") == want["tiles"] and ix.get("last_candidates") == want["candidates"]


def assign_with_empty_lists(rng, n, Cn, empty):
    """a random list for every item; the clusters `empty` get none"""
    allowed = np.setdiff1d(np.arange(Cn), empty)
    return allowed[rng.integers(0, len(allowed), n)].astype(np.int32)


class Case:
    """items, centroids, an explicit assignment and queries, with the stored floats of the queries against both -- one per shape, shared
    by the tests that differ in metric and nprobe alone (neither changes a stored float)"""

    def __init__(self, eng, seed, n, dim, Cn, n_q, empty=(), nan_clusters=(), aim=()):
        rng = np.random.default_rng(seed)
        self.x = rng.standard_normal((n, dim)).astype(F32)
        self.cent = rng.standard_normal((Cn, dim)).astype(F32)
        for c in nan_clusters:
            self.cent[c, dim // 2] = np.nan
        self.assign = assign_with_empty_lists(rng, n, Cn, np.array(empty, np.int64))
        self.q = rng.standard_normal((n_q, dim)).astype(F32)
        for i, c in enumerate(aim):                                               # query i: far out along centroid c, nearest to it
            self.q[i] = F32(6.0) * self.cent[c]
        self.d_items, self.d_cent = stored(eng, self.x, self.q), stored(eng, self.cent, self.q)
        with np.errstate(invalid="ignore"):
            self.nn = kmeans_ref.chain_sq(self.cent)
        self.start, self.lst = ref.lists_of(self.assign, Cn)
        self.gal = eng.gallery(self.x)
        self.ix = {m: eng.ivf(self.gal, self.cent, metric=m, assign=self.assign) for m in METRICS}

    def want(self, metric, nprobe, k, block_rows=None):
        return ref.search(self.d_items, self.d_cent, self.nn, metric, self.start, self.lst, nprobe, k, block_rows)

    def close(self):
        for ix in self.ix.values():
            ix.close()
        self.gal.close()


# ------------------------------------------------------------------------------------------------ a. nprobe = C is vv_gallery_topk
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("Cn", [65, 257])
@pytest.mark.parametrize("dim", [8, 33])
def test_every_cluster_probed_is_topk(eng, metric, Cn, dim):
    """nprobe == C > 64: k_ivf_probe's "all" form, offsets scanned over several strides of 64 probes, k_ivf_select over C probes"""
    n, n_q = 3000, 150
    rng = np.random.default_rng(dim * 1000 + Cn)
    x = rng.standard_normal((n, dim)).astype(F32)
    q = rng.standard_normal((n_q, dim)).astype(F32)
    assign = assign_with_empty_lists(rng, n, Cn, np.array([0, 31, 64, Cn - 1]))
    gal = eng.gallery(x)
    ix = eng.ivf(gal, x[:Cn], metric=metric, assign=assign)
    try:
        assert ix.get("empty_lists") == (np.bincount(assign, minlength=Cn) == 0).sum() >= 3       # (C = 65: cluster 64 is the last)
        for k in (1, 32):
            idx, dist, m = ix.search(q, k, Cn)
            assert same((idx, dist), gal.topk(q, k)), k
            assert (m == n).all() and ix.get("last_candidates") == n * n_q
    finally:
        ix.close(); gal.close()


# ------------------------------------------------------------------------------------------------ b. a ragged last stride
@pytest.fixture(scope="module")
def ragged_cases(eng):
    made = {}

    def get(Cn):
        if Cn not in made:
            made[Cn] = Case(eng, 500 + Cn, 2000, 24, Cn, 130, empty=(1, 63), aim=(64, Cn - 1))
        return made[Cn]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nprobe", [1, 63, 64])
@pytest.mark.parametrize("Cn", [65, 100, 257])
def test_probe_sweep_with_a_ragged_last_stride(ragged_cases, metric, Cn, nprobe):
    """C = 65, 100, 257: the sweep's last stride holds 1, 36 and 1 clusters; nprobe = 1, 63 and 64 = every lane of the wave's list"""
    c = ragged_cases(Cn)
    want = c.want(metric, nprobe, 10)
    assert all(len(set(p)) == nprobe for p in want["probes"])
    assert want["probes"][0][0] == 64 and want["probes"][1][0] == Cn - 1          # (queries 0 and 1 were aimed at the last stride)
    check(c.ix[metric], c.q, 10, nprobe, want)


# ------------------------------------------------------------------------------------------------ c. NaN keys across strides
NUMBERS = [5, 70, 128]                                                            # one cluster of every stride of C = 130


@pytest.fixture(scope="module")
def nan_case(eng):
    nan = np.setdiff1d(np.arange(130), NUMBERS)                                   # 0, 63, 64, 65 and 129 among them
    c = Case(eng, 77, 1500, 16, 130, 70, nan_clusters=nan)
    yield c
    c.close()


@pytest.mark.parametrize("metric", METRICS)
def test_fewer_keys_than_nprobe_are_numbers(nan_case, metric):
    c = nan_case
    assert np.isnan(c.d_cent[:, [0, 63, 64, 65, 129]]).all() and not np.isnan(c.d_cent[:, NUMBERS]).any()
    for nprobe in (2, 3, 4, 8):
        want = c.want(metric, nprobe, 8)
        for p in want["probes"]:                                                  # the numbers in key order, then the lowest NaN clusters
            assert set(p[:3]) <= set(NUMBERS) and len(set(p)) == nprobe and p[3:] == [0, 1, 2, 3, 4][:max(nprobe - 3, 0)]
        check(c.ix[metric], c.q, 8, nprobe, want)


@pytest.mark.parametrize("metric", METRICS)
def test_exactly_nprobe_keys_are_numbers(eng, metric):
    numbers = [5, 62, 66, 70, 100, 126, 127, 128]
    c = Case(eng, 78, 1500, 16, 130, 70, nan_clusters=np.setdiff1d(np.arange(130), numbers))
    try:
        want = c.want(metric, 8, 8)
        assert all(sorted(p) == numbers for p in want["probes"])                 # nothing is filled in
        check(c.ix[metric], c.q, 8, 8, want)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ d. pair grouping past one tile
@pytest.mark.parametrize("metric", METRICS)
def test_pairs_of_one_block_past_eight_tiles(eng, metric):
    """300 queries x 64 probes = 19200 pairs in one block: 19 grouping tiles, two 8-tile steps of k_km_scan and a remainder of three;
    blocks of 64 queries: 4096 pairs, four tiles, the remainder loop alone -- the same bits"""
    c = Case(eng, 91, 3000, 16, 257, 300, empty=(2, 200))
    ix = c.ix[metric]
    try:
        want = c.want(metric, 64, 10)
        check(ix, c.q, 10, 64, want)
        assert ix.get("last_blocks") == 1
        first = ix.search(c.q, 10, 64)
        eng.set_option("ivf_block_rows", 64)
        try:
            got = ix.search(c.q, 10, 64)
            assert ix.get("last_blocks") == 5 and same(first, got) and np.array_equal(first[2], got[2])
            assert ix.get("last_tiles") == c.want(metric, 64, 10, block_rows=64)["tiles"]
            assert ix.get("last_candidates") == want["candidates"]
        finally:
            eng.set_option("ivf_block_rows", 0)
    finally:
        c.close()
