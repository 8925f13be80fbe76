"""GPU tests that hold the two retrieval statistics paths of csrc/kernels_retrieval.hip EXACTLY, past one segment and one pass:
k_rank_count / k_rank_final (Gallery.rank_stats), k_class_sort / k_class_count / k_class_final and k_topk_part<OTHER_ID>
(Gallery.class_stats), and k_sim_f32 at its tile edges (Gallery.nearest with k = n_ref) -- against tests/retrieval_exact_ref.py.

Exact inputs (nearest_ref.exact_input): integer features in [-3, 3], so every fp32 dot product is exact in any summation order
and all distances come from nearest_ref.distances32.  Comparison rules, no near-tie exemption and no query left out:
  * integers (best_rank, acc1, acc5 * 5, n_scored, median_rank, top5_idx): ==;  top5_dist and the lists of test d: the bits;
  * per-query ap: |got - float32(ap64)| <= 1 float32 ulp.  The device sums the exact quotients ret / rank in double in another
    order than the reference: relative error <= P * 2^-53 < 1e-12 for the P <= 6000 used here, so only the final cast to float
    can differ, by at most one ulp;
  * summary means: the same bound against the float64 mean of the reference's per-query values -- except the class summary of
    test c, which is a CONSISTENCY check against the float64 mean of the returned per-query values (1e-6): the full float64
    summary over 66 049^2 pairs is not computed on the host;
  * a query with one positive has ap = 1 / rank: rank = round(1 / ap) is compared with ==.
The preconditions that make these bounds tell a one-off error from none (ap_sensitivity >= 3 or 4 ulp, the tie blocks, ranks on
both sides of the 10000 cap, class-mates and same-video items in both counting segments) are asserted on the CPU by
tests/test_retrieval_exact_ref_host.py on the same inputs.  Every test asserts the launch shape it claims."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nearest_ref   # noqa: E402
import retrieval_exact_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_rank_stats(st, want, nq):
    """st = Gallery.rank_stats(..., per_query=True) against ref.rank_rows' values, by the module's rules."""
    bad = np.flatnonzero(st["best_rank"] != want["best_rank"])
    assert len(bad) == 0, (bad[:5], st["best_rank"][bad[:5]], want["best_rank"][bad[:5]])
    assert np.array_equal(st["top5_idx"], want["top5_idx"]), np.argwhere(st["top5_idx"] != want["top5_idx"])[:5]
    assert np.array_equal(bits(st["top5_dist"]), bits(want["top5_dist"]))
    ok = ref.within_one_ulp(st["ap"], want["ap"])
    worst = np.abs(st["ap"].astype(np.float64) - want["ap"]).max()
    print("largest |ap - ap64| %.3g; queries off by more than one ulp: %d of %d" % (worst, int((~ok).sum()), nq))
    assert ok.all(), [(int(i), float(st["ap"][i]), float(want["ap"][i]), len(want["val"][i])) for i in np.flatnonzero(~ok)[:8]]
    s = ref.rank_summary(want)
    assert st["median_rank"] == s["median_rank"]
    for f in ("recall_1", "recall_5", "recall_10", "mean_ap"):
        assert ref.within_one_ulp(np.float32(st[f]), s[f]).all(), (f, st[f], s[f])


# ---------------------------------------------------------------------------------------------- a
def case_a():
    if "a" not in _cache:
        c = ref.input_a()
        c["ref"] = ref.rank_rows(nearest_ref.distances32(c["Q"], c["G"]), c["qid"], c["gid"])
        _cache["a"] = c
    return _cache["a"]


def test_rank_stats_four_segments(eng):
    """49 153 items: four segments, the last of one item; 513 queries: two query blocks, the second of one row.  Single positives
    at both ends of every segment inside blocks of exact ties, positives straddling segment edges, ids absent from the gallery,
    2047 .. 6000 positives (one, two and three passes)."""
    c = case_a()
    nq = len(c["qid"])
    g = eng.gallery(c["G"], c["gid"])
    try:
        st = g.rank_stats(c["Q"], c["qid"], per_query=True)
        passes, block, scratch, limit = int(g.get("last_passes")), int(g.get("query_block")), g.scratch_bytes, g.get("scratch_limit_bytes")
        again = g.rank_stats(c["Q"], c["qid"], per_query=True)
    finally:
        g.close()
    assert passes == 3 and block < nq and 0 < scratch <= limit
    want = c["ref"]
    check_rank_stats(st, want, nq)
    for i in c["probes"]:                                              # ap as a rank probe
        assert st["ap"][i] > 0
        assert round(1.0 / float(st["ap"][i])) == int(want["val"][i][0]), (i, st["ap"][i], want["val"][i])
    for i in c["absent"]:
        assert st["best_rank"][i] == 10000 and bits(st["ap"])[i] == 0
    for f in ("best_rank", "ap", "top5_idx", "top5_dist"):
        assert st[f].tobytes() == again[f].tobytes(), f


# ---------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("P", [2049, 2048])
def test_rank_stats_pass_edges(eng, P):
    """2100 items of which one id owns P: every positive's rank and ordinal is visible in the float32 AP (ap_sensitivity >= 3 ulp
    against a bound of 1).  2049: two passes, the second of one positive, ordinals counted from the ids; 2048: one full pass,
    ordinals are the slots.  D = 32: no column padding and one K tile in k_sim_f32; 129 queries: an M tile with one live row."""
    c = ref.input_b(P)
    want = ref.rank_rows(nearest_ref.distances32(c["Q"], c["G"]), c["qid"], c["gid"])
    g = eng.gallery(c["G"], c["gid"])
    try:
        assert int(g.get("row_floats")) == ref.B_D
        st = g.rank_stats(c["Q"], c["qid"], per_query=True)
        passes = int(g.get("last_passes"))
    finally:
        g.close()
    assert passes == (2 if P == 2049 else 1)
    check_rank_stats(st, want, len(c["qid"]))


# ---------------------------------------------------------------------------------------------- c
def case_c():
    if "c" not in _cache:
        c = ref.input_c()
        c.update(ref.rows_c(c))
        _cache["c"] = c
    return _cache["c"]


@pytest.mark.parametrize("exclude", [True, False])
def test_class_stats_two_counting_segments(eng, exclude):
    """66 049 items: k_class_count with two segments per row (65536 + 513) whose bins merge in global memory, five segments of the
    top-5 of other videos, 130 query blocks, three passes."""
    c = case_c()
    n = len(c["vid"])
    assert n > 65536
    g = eng.gallery(c["X"], c["vid"])
    try:
        got = g.class_stats(c["map"], exclude_same_video=exclude, per_query=True)
        passes, block, scratch, limit = int(g.get("last_passes")), int(g.get("query_block")), g.scratch_bytes, g.get("scratch_limit_bytes")
        again = g.class_stats(c["map"], exclude_same_video=exclude, per_query=True)
    finally:
        g.close()
    assert passes == 3 and block < n and 0 < scratch <= limit
    rows, want = c["rows"], c["ref"][exclude]
    skipped = c["cls"][rows] < 0
    ok = ref.within_one_ulp(got["ap"][rows], want["ap"])
    assert ok.all(), [(int(rows[j]), float(got["ap"][rows[j]]), float(want["ap"][j])) for j in np.flatnonzero(~ok)[:8]]
    assert np.array_equal(got["acc1"][rows], want["acc1"].astype(np.float32), equal_nan=True), (got["acc1"][rows], want["acc1"])
    assert np.array_equal(np.round(got["acc5"][rows] * 5), np.round(want["acc5"] * 5), equal_nan=True), (got["acc5"][rows], want["acc5"])
    assert np.array_equal(got["acc5"][rows], want["acc5"].astype(np.float32), equal_nan=True)
    assert np.array_equal(got["top5_idx"][rows], want["top5"]), np.argwhere(got["top5_idx"][rows] != want["top5"])[:5]
    assert np.isnan(got["ap"][rows][skipped]).all() and (got["top5_idx"][rows][skipped] == -1).all() and skipped.any()
    for j in np.flatnonzero(~skipped):                                 # one positive: ap = 1 / val
        if len(want["val"][j]) == 1:
            assert round(1.0 / float(got["ap"][rows[j]])) == int(want["val"][j][0])
    # every row: skipped rows read NaN / -1, scored rows do not
    scored = c["cls"] >= 0
    for f in ("ap", "acc1", "acc5"):
        assert np.isnan(got[f][~scored]).all() and not np.isnan(got[f][scored]).any()
    assert (got["top5_idx"][~scored] == -1).all() and (got["top5_idx"][scored] >= 0).all()
    vid = c["vid"]
    assert (vid[got["top5_idx"][scored]] != vid[scored][:, None]).all()
    # summary: n_scored exact; the means are consistent with the returned per-query values (see the module docstring)
    assert got["n_scored"] == int(scored.sum())
    for f, k in (("mean_ap", "ap"), ("hit_at_1", "acc1"), ("hit_at_5", "acc5")):
        assert abs(got[f] - got[k][scored].astype(np.float64).mean()) <= 1e-6, f
    for f in ("ap", "acc1", "acc5", "top5_idx"):
        assert got[f].tobytes() == again[f].tobytes(), f
    for f in ("mean_ap", "hit_at_1", "hit_at_5", "n_scored"):
        assert got[f] == again[f]


# ---------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("nq,ng,D", ref.D_SHAPES)
def test_similarity_tile_edges(eng, nq, ng, D):
    """Every distance of every row, sorted: k_sim_f32 at one live row of a tile, full tiles, one K tile, padded and unpadded
    columns.  The last query row is all zero: +0 everywhere, the items in index order."""
    Q, G = ref.input_d(nq, ng, D)
    want = nearest_ref.nearest(nearest_ref.distances32(Q, G), None, ng)
    g = eng.gallery(G)
    try:
        assert int(g.get("row_floats")) == -(-D // 32) * 32
        idx, dist = g.nearest(Q, ng)
    finally:
        g.close()
    assert np.array_equal(idx, want[0]), np.argwhere(idx != want[0])[:5]
    assert np.array_equal(bits(dist), bits(want[1])), np.argwhere(bits(dist) != bits(want[1]))[:5]
    if nq > 1:
        assert (bits(dist)[nq - 1] == 0).all() and np.array_equal(idx[nq - 1], np.arange(ng))
