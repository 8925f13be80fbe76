"""CPU tests of tests/retrieval_exact_ref.py: its two restatements equal the ones the older retrieval tests use
(gallery_ref.rank_stats, class_stats_ref.class_stats) on small inputs, and every precondition that
tests/test_gpu_retrieval_exact.py relies on holds for the inputs it uses -- asserted here, where no GPU is needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import class_stats_ref   # noqa: E402
import gallery_ref   # noqa: E402
import nearest_ref   # noqa: E402
import retrieval_exact_ref as ref   # noqa: E402

_cache = {}


def cached(name, fn):
    if name not in _cache:
        _cache[name] = fn()
    return _cache[name]


def exact_distances(Q, G, D):
    d = nearest_ref.distances32(Q, G)
    assert d.dtype == np.float32 and (d == np.round(d)).all() and np.abs(d).max() <= 2 * 9 * D
    assert not (np.signbit(d) & (d == 0)).any()
    return d


# ---------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("exact", [False, True])
def test_rank_rows_equals_gallery_ref(exact):
    if exact:
        Q, qid, G, gid = nearest_ref.exact_input(23, 700, 9, 31, dim=8)        # heavy ties
        qid[[2, 11]] = 77                                                      # no positive
        d = nearest_ref.distances32(Q, G)
    else:
        Q, qid, G, gid = gallery_ref.make_input(nq=24, ng=900, D=16, nid=12, noise=1.0, seed=32)
        d = gallery_ref.distances(Q, G, np.float32)
    summary, best, ap, order = gallery_ref.rank_stats(d, qid, gid)
    r = ref.rank_rows(d, qid, gid)
    assert np.array_equal(r["best_rank"], best)
    assert np.abs(r["ap"] - ap).max() <= 1e-14                                # (float64, summed in another order)
    assert np.array_equal(r["top5_idx"], order[:, :5])
    assert np.array_equal(r["top5_dist"], d[np.arange(len(qid))[:, None], order[:, :5]])
    for i in range(len(qid)):
        a, r1, r5, r10, b = gallery_ref.ap_stats(gid[order[i]], qid[i])
        assert (r["acc1"][i], r["acc5"][i], r["acc10"][i]) == (r1, r5, r10)
        assert np.array_equal(r["val"][i], np.flatnonzero(gid[order[i]] == qid[i]) + 1)
    s = ref.rank_summary(r)
    assert s["median_rank"] == summary["median_rank"]
    for f in ("recall_1", "recall_5", "recall_10", "mean_ap"):
        assert abs(s[f] - summary[f]) <= 1e-15, f


def test_rank_rows_of_a_tiny_gallery():
    d = np.array([[0, -2, -2]], np.float32)
    r = ref.rank_rows(d, np.array([4]), np.array([4, 5, 4]))
    assert r["top5_idx"].tolist() == [[1, 2, 0, -1, -1]] and r["top5_dist"].tolist() == [[-2, -2, 0, 0, 0]]
    assert r["val"][0].tolist() == [2, 3] and r["best_rank"][0] == 2 and r["ap"][0] == (1 / 2 + 2 / 3) / 2


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("exact", [False, True])
def test_class_rows_equals_class_stats_ref(exact, exclude):
    X, vid, m = class_stats_ref.make_input(400, 12, 60, 5, 1.0, 1.0, 33)
    if exact:
        X = np.random.default_rng(34).integers(-3, 4, (400, 6)).astype(np.float32)
        d = nearest_ref.distances32(X, X)
    else:
        d = class_stats_ref.distances(X, np.float32)
    m.pop(int(vid[7]))                                                        # an id absent from the map: class 0
    cls = class_stats_ref.classes_of(vid, m)
    assert (cls < 0).any() and (cls >= 0).any()
    _, ap, a1, a5, t5 = class_stats_ref.class_stats(d, vid, m, exclude)
    rows = np.array([0, 7, 399, 13, 200] + [int(i) for i in np.flatnonzero(cls < 0)[:3]])
    r = ref.class_rows(d[rows], rows, vid, cls, exclude)
    assert np.array_equal(r["ap"], ap[rows], equal_nan=True)
    assert np.array_equal(r["acc1"], a1[rows], equal_nan=True) and np.array_equal(r["acc5"], a5[rows], equal_nan=True)
    assert np.array_equal(r["top5"], t5[rows])
    every = ref.class_rows(d, np.arange(400), vid, cls, exclude)
    assert np.array_equal(every["ap"], ap, equal_nan=True) and np.array_equal(every["top5"], t5)


def test_ap_sensitivity():
    assert ref.ap_sensitivity([]) == np.inf
    assert ref.ap_sensitivity([7]) == 1 / 7 - 1 / 8                            # one positive: ap = 1 / rank
    val = np.array([2, 3, 9])
    ap = lambda v, t: (np.asarray(t) / np.asarray(v)).sum() / 3   # noqa: E731
    base = ap(val, [1, 2, 3])
    moves = []
    for j in range(3):
        for dv in (-1, 1):
            v = val.copy(); v[j] += dv
            moves.append(abs(ap(v, [1, 2, 3]) - base))
            t = np.array([1, 2, 3]); t[j] += dv
            moves.append(abs(ap(val, t) - base))
    assert abs(ref.ap_sensitivity(val) - min(moves)) <= 1e-15
    assert ref.within_one_ulp(np.float32([0.1, np.nan, 0]), [0.1 + 5e-9, np.nan, 0]).all()
    assert not ref.within_one_ulp(np.float32([0.1]), [0.1 + 2e-8]).any()
    assert not ref.within_one_ulp(np.float32([np.nan, 0.5]), [0.5, np.nan]).any()


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
def case_a():
    def make():
        c = ref.input_a()
        c["d"] = exact_distances(c["Q"], c["G"], ref.A_D)
        c["ref"] = ref.rank_rows(c["d"], c["qid"], c["gid"])
        return c
    return cached("a", make)


def test_input_a_shape_and_ids():
    c = case_a()
    ng, nq = ref.A_NG, ref.A_NQ
    assert c["G"].shape == (ng, 40) and c["Q"].shape == (nq, 40) and ng % 4 == 1 and ng == 3 * 16384 + 1 and nq == 513
    assert -(-ng // ref.SEG) == 4 and ng - 3 * ref.SEG == 1
    count = lambda v: int((c["gid"] == v).sum())   # noqa: E731
    for v, g in ref.A_SINGLE.items():
        assert np.flatnonzero(c["gid"] == v).tolist() == [g]
    assert sorted(ref.A_SINGLE.values()) == [0, 16383, 16384, 32767, 32768, 49151, 49152]
    for v, idx in ref.A_STRADDLE.items():
        assert np.flatnonzero(c["gid"] == v).tolist() == idx and len(idx) in (2, 3)
        assert len(set(i // ref.SEG for i in idx)) == 2                        # both sides of one segment edge
    assert [count(v) for v in ref.A_BIG] == [2047, 2048, 2049, 4096, 4097, 6000]
    assert -(-max(ref.A_BIG.values()) // ref.CHUNK) == 3                       # last_passes
    for v in ref.A_ABSENT:
        assert count(v) == 0
    assert min(c["gid"]) < 50 < max(c["gid"])
    for rows, ids in ((c["absent"], ref.A_ABSENT),):
        assert c["qid"][rows].tolist() == ids
    for v, rows in list(c["big"].items()) + list(c["straddle"].items()):
        assert (c["qid"][rows] == v).all()
    # every kind of query is present, the one-row second block holds a probe
    assert 512 in c["probes"] and 127 in c["probes"] and 128 in c["probes"]
    for i in c["probes"]:
        assert len(c["ref"]["val"][i]) == 1


def test_input_a_tie_blocks():
    c = case_a()
    for lo, hi in ref.A_TIE_BLOCKS:
        assert (c["G"][lo:hi] == c["G"][lo]).all() and (c["d"][:, lo:hi] == c["d"][:, lo:lo + 1]).all()
    for g in ref.A_SINGLE.values():
        lo, hi = next(b for b in ref.A_TIE_BLOCKS if b[0] <= g < b[1])
        assert (g == 0 or lo < g) and (g == ref.A_NG - 1 or g + 1 < hi)         # ties on both sides in index order
        assert lo == 0 or hi == ref.A_NG or lo // ref.SEG != (hi - 1) // ref.SEG   # ... and across the segment edge
    # a tie block moves the positive's rank: for a probe whose positive is not the block's first item, the rank counts the
    # ties of lower index
    for i in c["probes"]:
        g = ref.A_SINGLE[int(c["qid"][i])]
        row = c["d"][i]
        assert c["ref"]["val"][i][0] == 1 + (row < row[g]).sum() + (row[:g] == row[g]).sum()
        assert g == 0 or (row[:g] == row[g]).sum() >= 7


def test_input_a_probe_margins():
    c = case_a()
    ranks = np.array([int(c["ref"]["val"][i][0]) for i in c["probes"]])
    assert (ranks < 10000).any() and (ranks > 10000).any() and (ranks <= 10).any()
    for i, r in zip(c["probes"], ranks):
        ap = c["ref"]["ap"][i]
        assert ap == 1.0 / r
        assert ref.ap_sensitivity(c["ref"]["val"][i]) >= 4 * ref.ulp32(ap)
        # 1 / ap read back from a float32 one ulp off still rounds to the rank
        for off in (-1, 0, 1):
            a32 = np.float32(ap) + np.float32(off) * np.spacing(np.float32(ap))
            assert round(1.0 / float(a32)) == r
    assert c["ref"]["best_rank"][c["absent"]].tolist() == [10000] * 3 and (c["ref"]["ap"][c["absent"]] == 0).all()
    assert (c["ref"]["best_rank"] == 10000).sum() > 3                          # the cap, not only the absent ids


def case_b(P):
    def make():
        c = ref.input_b(P)
        c["d"] = exact_distances(c["Q"], c["G"], ref.B_D)
        c["ref"] = ref.rank_rows(c["d"], c["qid"], c["gid"])
        return c
    return cached(("b", P), make)


@pytest.mark.parametrize("P", [2049, 2048])
def test_input_b(P):
    c = case_b(P)
    assert c["G"].shape == (2100, 32) and c["Q"].shape == (129, 32)
    assert int((c["gid"] == ref.B_BIG[P]).sum()) == P and len(c["big"]) >= 120 and {0, 63, 64, 127, 128} <= set(c["big"].tolist())
    assert -(-P // ref.CHUNK) == (2 if P == 2049 else 1)
    margins = [ref.ap_sensitivity(c["ref"]["val"][i]) / ref.ulp32(c["ref"]["ap"][i]) for i in c["big"]]
    print("P = %d: smallest ap_sensitivity %.2f ulp" % (P, min(margins)))
    assert min(margins) >= 3
    assert (c["d"][5] == 0).all()
    assert (c["ref"]["ap"][c["qid"] == 999] == 0).all() and (c["qid"] == 999).sum() == 1


def case_c():
    def make():
        c = ref.input_c()
        c.update(ref.rows_c(c))
        return c
    return cached("c", make)


def test_input_c_layout():
    c = case_c()
    n, cls, vid = ref.C_N, c["cls"], c["vid"]
    assert n == 65536 + 513 and c["X"].shape == (n, 32) and -(-n // ref.CSEG) == 2 and -(-n // ref.SEG) == 5
    assert -(-n // 512) == 130
    d = exact_distances(c["X"][:64], c["X"], ref.C_D)
    assert d.shape == (64, n)
    sizes = np.bincount(np.unique(vid, return_inverse=True)[1])
    assert sizes.min() == 1 and sizes.max() == 4
    for v in np.unique(vid)[:2000]:                                            # one video, one class
        assert len(set(cls[vid == v].tolist())) == 1
    assert [(cls == k).sum() for k in (1, 2, 3)] == [5000, 2048, 2049]
    assert -(-5000 // ref.CHUNK) == 3
    assert len(c["small"]) == 300
    for k, mem in c["small"].items():
        assert 2 <= len(mem) <= 8 and np.array_equal(np.flatnonzero(cls == k), mem)
        assert mem[0] < ref.CSEG <= mem[-1]                                    # members on both sides of item 65536
    assert 0.025 * n <= (cls < 0).sum() <= 0.035 * n
    absent = ~np.isin(vid, np.array(list(c["map"])))
    assert absent.sum() == 1000 and (cls[absent] == 0).all() and (cls == 0).sum() == 1000


def test_input_c_reference_rows():
    c = case_c()
    rows, cls, vid = c["rows"], c["cls"], c["vid"]
    print("%d reference rows; %d small classes tried for %d" % (len(rows), c["tried"], len(c["classes"])))
    assert 50 <= len(rows) <= 90 and set(ref.C_FIXED_ROWS) <= set(rows.tolist())
    assert len(c["classes"]) == 10
    for k in c["classes"]:
        assert set(c["small"][k].tolist()) <= set(rows.tolist())
    for k in ref.C_LARGE:
        assert (cls[rows] == k).sum() >= 3
    skipped = cls[rows] < 0
    assert skipped.sum() >= 3
    for ex in (True, False):
        r = c["ref"][ex]
        assert np.isnan(r["ap"][skipped]).all() and (r["top5"][skipped] == -1).all() and not np.isnan(r["ap"][~skipped]).any()
        for j in c["small_rows"]:
            if len(r["val"][j]):
                assert ref.ap_sensitivity(r["val"][j], r["ret"][j]) >= 4 * ref.ulp32(r["ap"][j]), (ex, j)
    # some small-class row has positives under exclusion, some has none (a class of two in one video)
    r = c["ref"][True]
    assert any(len(r["val"][j]) for j in c["small_rows"])
    # a class-mate in each counting segment; a same-video item in the other counting segment
    both = [i for i in rows if cls[i] >= 0 and len(set((np.flatnonzero((cls == cls[i]) & (np.arange(len(cls)) != i)) >= ref.CSEG).tolist())) == 2]
    assert both
    cross = [i for i in rows[c["small_rows"]] if (((np.flatnonzero(vid == vid[i]) >= ref.CSEG) != (i >= ref.CSEG)).any())]
    assert cross
    # the two settings differ on such a row, so the test tells them apart
    j = int(np.flatnonzero(rows == cross[0])[0])
    assert c["ref"][True]["ap"][j] != c["ref"][False]["ap"][j] or len(c["ref"][True]["val"][j]) != len(c["ref"][False]["val"][j])


def test_input_d_shapes():
    nqs, ngs, Ds = zip(*ref.D_SHAPES)
    assert len(ref.D_SHAPES) == 12 and len(set(ref.D_SHAPES)) == 12
    assert set(nqs) == {1, 127, 128, 129} and set(ngs) == {127, 128, 129, 2048} and set(Ds) == {1, 31, 32, 33, 64, 96}
    for nq, ng, D in ref.D_SHAPES:
        Q, G = ref.input_d(nq, ng, D)
        d = exact_distances(Q, G, D)
        assert d.shape == (nq, ng) and ng <= ref.CHUNK
        if nq > 1:
            assert (d[nq - 1].view(np.uint32) == 0).all()
    assert any(nq > 1 and nq % 128 in (0, 1, 127) for nq, _, _ in ref.D_SHAPES)
