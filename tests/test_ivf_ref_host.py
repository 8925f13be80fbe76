"""tests/ivf_ref.py by hand, without a GPU: three small cases whose answers are written out -- a tie across two clusters, an empty
probed list, k above a query's candidates -- the probe's rules, and recall 1 with nprobe = C; lists_of against a bucket loop at the
sizes and patterns at which it is the oracle of the device's grouping (tests/edge_inputs.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_inputs as inp   # noqa: E402
import ivf_ref as ref   # noqa: E402

F32 = np.float32
NAN = float("nan")


def test_a_tie_across_two_clusters_orders_by_item_index():
    # items 0 .. 4; cluster 0 = {1, 4}, cluster 1 = {0, 2}, cluster 2 = {3}.  Items 4 and 0 are equally far; cluster 0 is probed first
    start, lst = ref.lists_of([1, 0, 1, 2, 0], 3)
    assert start.tolist() == [0, 2, 4, 5] and lst.tolist() == [1, 4, 0, 2, 3]
    d_items = np.array([[-6, -2, -4, -9, -6]], F32)
    d_cent = np.array([[-5, -4, 7]], F32)
    r = ref.search(d_items, d_cent, None, "spherical", start, lst, nprobe=2, k=3)
    assert r["probes"] == [[0, 1]] and r["n_candidates"].tolist() == [4]
    assert r["idx"].tolist() == [[0, 4, 2]] and r["dist"].tolist() == [[-6, -6, -4]]          # item 3, the nearest, is in no probed list
    assert r["tiles"] == 2 and r["candidates"] == 4


def test_an_empty_probed_list_adds_nothing():
    start, lst = ref.lists_of([2, 2, 0, 2], 3)                     # cluster 1 is empty
    d_items = np.array([[1, 2, 3, 0.5], [1, 2, 3, 0.5]], F32)
    d_cent = np.array([[9, -1, 0], [0, 5, 9]], F32)
    nn = np.array([0, 0, 2], F32)                                  # EUCLIDEAN: keys [9, -1, 2] and [0, 5, 11]
    r = ref.search(d_items, d_cent, nn, "euclidean", start, lst, nprobe=2, k=2)
    assert r["probes"] == [[1, 2], [0, 1]] and r["n_candidates"].tolist() == [3, 1]
    assert r["idx"].tolist() == [[3, 0], [2, -1]] and r["dist"].tolist() == [[0.5, 1], [3, 0]]
    assert r["tiles"] == 2 and r["candidates"] == 4                # clusters 2 and 0, one tile each; the empty one none


def test_k_above_the_candidates_reads_minus_one_and_zero():
    start, lst = ref.lists_of([0, 0, 0, 1], 4)                     # clusters 2 and 3 are empty
    d_items = np.array([[4, 3, 2, 1]], F32)
    r = ref.search(d_items, np.array([[5, 1, 0, 0]], F32), None, "spherical", start, lst, nprobe=2, k=3)
    assert r["probes"] == [[2, 3]] and r["n_candidates"].tolist() == [0]
    assert r["idx"].tolist() == [[-1, -1, -1]] and r["dist"].tolist() == [[0, 0, 0]] and r["tiles"] == 0
    r = ref.search(d_items, np.array([[5, 1, 0, 9]], F32), None, "spherical", start, lst, nprobe=2, k=3)
    assert r["probes"] == [[2, 1]] and r["idx"].tolist() == [[3, -1, -1]] and r["dist"].tolist() == [[1, 0, 0]]


def test_probe_rules():
    assert ref.probe_order(np.array([3, 1, 1, 0], F32), 3) == [3, 1, 2]                 # the lowest cluster at a tie
    assert ref.probe_order(np.array([0.0, -0.0, 1], F32), 2) == [0, 1]                  # -0 and +0 are one key
    assert ref.probe_order(np.array([NAN, 2, NAN, NAN], F32), 3) == [1, 0, 2]           # the slots left: the lowest unused clusters
    assert ref.probe_order(np.array([NAN, NAN], F32), 1) == [0]
    assert ref.probe_order(np.array([5, NAN, -1], F32), 3) == [0, 1, 2]                 # nprobe == C: every cluster, ascending
    assert ref.probe_keys(np.array([[1, 2]], F32), np.array([0.5, 1e9], F32), "euclidean").tolist() == [[1.5, 1e9]]


def test_tiles_count_per_block_and_past_one_tile():
    n, C = 700, 3
    assign = np.concatenate([np.zeros(300), np.ones(129), np.full(271, 2)]).astype(np.int32)
    start, lst = ref.lists_of(assign, C)
    n_q = 200
    d_items = np.zeros((n_q, n), F32)
    d_cent = np.tile(np.array([[0, 1, 2]], F32), (n_q, 1))            # every query probes cluster 0, then 1
    r = ref.search(d_items, d_cent, None, "spherical", start, lst, nprobe=2, k=1)
    assert r["tiles"] == 2 * 3 + 2 * 2 and r["candidates"] == n_q * 429            # 200 queries: 2 query tiles; 300 items: 3; 129: 2
    r = ref.search(d_items, d_cent, None, "spherical", start, lst, nprobe=2, k=1, block_rows=64)
    assert r["tiles"] == 4 * (3 + 2)                                               # four blocks of at most 64 queries: one query tile each
    assert r["idx"][:, 0].tolist() == [0] * n_q                                    # all distances equal: the lowest item index


def test_recall_is_one_with_every_cluster_probed():
    rng = np.random.default_rng(5)
    n, C, n_q, k = 300, 7, 40, 5
    d_items = rng.standard_normal((n_q, n)).astype(F32)
    d_items[:, 17] = d_items[:, 3]                                   # ties
    d_cent = rng.standard_normal((n_q, C)).astype(F32)
    start, lst = ref.lists_of(rng.integers(0, C, n), C)
    exact = np.stack([np.lexsort((np.arange(n), row))[:k] for row in d_items]).astype(np.int32)
    full = ref.search(d_items, d_cent, None, "spherical", start, lst, nprobe=C, k=k)
    assert np.array_equal(full["idx"], exact) and (full["n_candidates"] == n).all()
    assert ref.recall(full["idx"], exact, 1) == 1.0 and ref.recall(full["idx"], exact, k) == 1.0
    part = ref.search(d_items, d_cent, None, "spherical", start, lst, nprobe=2, k=k)
    assert 0.0 < ref.recall(part["idx"], exact, k) < 1.0


@pytest.mark.parametrize("n,C,pattern", inp.GROUP_CASES)
def test_lists_of_against_a_bucket_loop(n, C, pattern):
    """lists_of is the oracle of the device's grouping at these sizes and patterns (tests/test_gpu_kmeans_edges.py): here against one
    bucket per cluster, filled in item order"""
    assign = inp.group_assign(n, C, pattern)
    assert assign.shape == (n,) and assign.min() >= 0 and assign.max() < C
    buckets = [[] for _ in range(C)]
    for i, c in enumerate(assign.tolist()):
        buckets[c].append(i)
    want_start, want_lst = [0], []
    for b in buckets:
        want_lst += b
        want_start.append(len(want_lst))
    start, lst = ref.lists_of(assign, C)
    assert start.dtype == np.int32 and lst.dtype == np.int32
    assert start.tolist() == want_start and lst.tolist() == want_lst
    # the patterns are what they were made for
    if pattern == "one_cluster":
        assert want_start[C - 1] == 0 and want_start[C] == n
    if pattern == "round_robin" and C >= 64:
        assert all(len(set(assign[j:j + 64].tolist())) == 64 for j in range(0, n - 63, 64))
    if pattern in ("ascending", "descending"):
        step = np.diff(assign.astype(np.int64))
        assert (step >= 0).all() if pattern == "ascending" else (step <= 0).all()
