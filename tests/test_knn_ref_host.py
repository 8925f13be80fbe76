"""CPU tests of tests/knn_ref.py, the restatement the GPU tests of vv_gallery_knn_scores compare against: it equals a plain-Python
brute force, its rows sum to 1 (exactly under UNIFORM where m is a power of two), rows without an eligible item are zero, a case
worked by hand comes out, and every float64 V of the EXP cases is at least 1 (w_0 = 1 by construction)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_ref as ref   # noqa: E402
import nearest_ref   # noqa: E402


def small_case():
    Q, qid, G, gid = nearest_ref.exact_input(9, 300, 6, 31)
    gid = nearest_ref.one_id_owns_all_but(gid, 6, 7, 32)           # id 6 owns all but 7 items
    qid = qid.copy()
    qid[2] = 6                                                     # 7 eligible items
    d = nearest_ref.distances32(Q, G)
    labels = np.random.default_rng(33).integers(0, 5, 300).astype(np.int32)
    return d, gid[None, :] != qid[:, None], labels


def test_restatement_equals_the_brute_force():
    d, el, labels = small_case()
    for k in (1, 5, 8, 64):
        for e in (None, el):
            a, ma = ref.knn_scores(d, e, labels, 5, k)
            b, mb = ref.knn_scores_brute_force(d, e, labels, 5, k)
            assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(ma, mb)
            for T in (8.0, 0.5):
                a, ma = ref.knn_scores(d, e, labels, 5, k, ref.EXP, T)
                b, mb = ref.knn_scores_brute_force(d, e, labels, 5, k, ref.EXP, T)
                assert a.dtype == np.float64 and np.abs(a - b).max() <= 1e-14 and np.array_equal(ma, mb)
    assert ma[2] == 7 and (np.delete(ma, 2) == 64).all()


def test_rows_sum_to_one():
    d, el, labels = small_case()
    for k in (1, 2, 8, 64, 256):
        s, m = ref.knn_scores(d, None, labels, 5, k)
        assert (m == min(k, 300)).all() and (m & (m - 1) == 0).all()
        assert (s.sum(axis=1, dtype=np.float32) == 1).all()        # multiples of 2^-j: every partial sum is exact
    s, m = ref.knn_scores(d, el, labels, 5, 33)
    assert np.abs(s.astype(np.float64).sum(axis=1) - 1).max() <= 5 * 2.0 ** -24
    s, _ = ref.knn_scores(d, el, labels, 5, 33, ref.EXP, 0.5)
    assert np.abs(s.sum(axis=1) - 1).max() <= 1e-15


def test_rows_without_an_eligible_item_are_zero():
    d, _, labels = small_case()
    el = np.ones(d.shape, bool)
    el[4] = False
    for w, T in ((ref.UNIFORM, None), (ref.EXP, 0.5)):
        s, m = ref.knn_scores(d, el, labels, 5, 10, w, T)
        assert m[4] == 0 and (s[4] == 0).all() and not np.signbit(s[4]).any()
        assert (np.delete(m, 4) == 10).all() and (np.delete(s, 4, axis=0).sum(axis=1) > 0.999).all()


def test_known_answer():
    """One query, five items at distances d = -8, -6, -6, -2, 0 (s = 4, 3, 3, 1, 0), classes 1, 0, 1, 2, 0.
    k = 4 takes items 0, 1, 2, 3 (the tie of items 1 and 2 in index order).
    UNIFORM: votes [1, 2, 1] of 4 -> [0.25, 0.5, 0.25].
    EXP, T = 1: weights 1, e^-1, e^-1, e^-3 -> V_0 = e^-1, V_1 = 1 + e^-1, V_2 = e^-3.
    k = 2, item 1 not eligible: items 0 and 2, both class 1 -> [0, 1, 0] under either weighting."""
    d = np.array([[-8, -6, -6, -2, 0]], np.float32)
    labels = np.array([1, 0, 1, 2, 0], np.int32)
    s, m = ref.knn_scores(d, None, labels, 3, 4)
    assert s.tolist() == [[0.25, 0.5, 0.25]] and m.tolist() == [4]
    s, _ = ref.knn_scores(d, None, labels, 3, 4, ref.EXP, 1.0)
    e1, e3 = np.exp(-1.0), np.exp(-3.0)
    V = 1 + 2 * e1 + e3
    assert np.abs(s - np.array([[e1 / V, (1 + e1) / V, e3 / V]])).max() <= 1e-15
    el = np.array([[True, False, True, True, True]])
    for w in (ref.UNIFORM, ref.EXP):
        s, m = ref.knn_scores(d, el, labels, 3, 2, w, 0.25)
        assert s.tolist() == [[0, 1, 0]] and m.tolist() == [2]
    s, m = ref.knn_scores(d, None, labels, 3, 9)                   # fewer items than k: its own denominator
    assert m.tolist() == [5] and np.array_equal(s, (np.array([[2, 2, 1]], np.float32) / np.float32(5)))


def test_exp_sums_are_at_least_one():
    """The guard of the GPU test's EXP cases: w_0 = exp(0) = 1, so V >= 1 in float64 wherever m >= 1, whatever T."""
    d, el, labels = small_case()
    for T in (8.0, 0.5, 1e-3):
        for k in (5, 256):
            V, arg = ref.exp_sums(d, el, labels, 5, k, T)
            assert (V >= 1).all() and (arg[:, 0] == 0).all() and (arg[np.isfinite(arg)] <= 0).all()
