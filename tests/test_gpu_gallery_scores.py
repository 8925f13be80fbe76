"""GPU tests of vv_gallery_scores (Gallery.scores): the score matrix is, bit for bit, -0.5 x the distances the other gallery calls
return, and it feeds vv_classification_stats on the device -- a nearest-class-mean classifier end to end.

Bit equality: at n_ref <= 2048 vv_gallery_nearest(k = n_ref) lists every reference item with its distance, so every entry of the
score matrix is checked: scores[i][idx] == -0.5 * dist as bits.  dim = 1, 31, 32, 33, 512 (around the 32-float padding of the
similarity's operand rows); n_q = 600 passes one query block (512 rows).

End to end on exact inputs: integer embeddings clustered around centres of entries +-4, eight training items per class -- every class mean
is a multiple of 1/8 and every dot product a multiple of 1/8 below 2^13, exact in fp32 in any summation order.  The numpy restatement
of the pipeline on the downloaded prototype rows therefore has the very same scores, and everything downstream is held as tightly
as in tests/test_gpu_classification_stats.py; the restatement's top-two margin is checked to exceed 1e-3 in every row, so no
prediction hinges on a tie."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classification_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("dim,n_q,n_ref", [(1, 7, 100), (31, 65, 257), (32, 64, 2048), (33, 600, 100), (512, 130, 300)])
def test_scores_are_minus_half_the_distances_bit_for_bit(eng, dim, n_q, n_ref):
    rng = np.random.default_rng(100 * dim + n_q)
    G = rng.standard_normal((n_ref, dim)).astype(np.float32)
    Q = rng.standard_normal((n_q, dim)).astype(np.float32)
    g = eng.gallery(G)
    try:
        assert (n_q > g.get("query_block")) == (n_q == 600)
        idx, dist = g.nearest(Q, n_ref)
        buf = g.scores(Q)
        s = buf.get()
        buf.free()
    finally:
        g.close()
    assert s.shape == (n_q, n_ref) and (np.sort(idx, axis=1) == np.arange(n_ref)).all()
    got = np.take_along_axis(s, idx, axis=1)
    assert np.array_equal(bits(got), bits(np.float32(-0.5) * dist))
    assert np.allclose(s, Q.astype(np.float64) @ G.astype(np.float64).T, atol=1e-4 * np.sqrt(dim) + 1e-5 * dim)


def test_nearest_class_mean_classifier_end_to_end(eng):
    rng = np.random.default_rng(77)
    Cn, dim, per, n_test = 6, 24, 8, 333
    centres = 4 * rng.choice([-1, 1], (Cn, dim))          # equal norms: the largest dot product is the nearest mean
    tr_lab = rng.permutation(np.repeat(np.arange(Cn), per)).astype(np.int32)
    train = (centres[tr_lab] + rng.integers(-1, 2, (Cn * per, dim))).astype(np.float32)
    te_lab = rng.integers(0, Cn, n_test).astype(np.int32)
    test = (centres[te_lab] + rng.integers(-1, 2, (n_test, dim))).astype(np.float32)
    te_lab[::17] = (te_lab[::17] + 1) % Cn                     # some rows carry another class's label: accuracy below one
    items = eng.gallery(train, tr_lab)
    protos = items.pool_by_id()
    try:
        assert protos.ids.tolist() == list(range(Cn))          # prototypes come out in ascending class
        P = protos.rows()
        buf = protos.scores(test)
        got = eng.classification_stats(buf, te_lab, Cn)
        s_dev = buf.get()
        buf.free()
    finally:
        protos.close()
        items.close()
    # the same pipeline in numpy on the downloaded fp32 prototype rows
    means = np.stack([train[tr_lab == c].astype(np.float64).mean(axis=0) for c in range(Cn)])
    assert np.array_equal(P.astype(np.float64), means)
    s64 = test.astype(np.float64) @ P.astype(np.float64).T
    top2 = np.sort(s64, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] > 1e-3).all()
    assert np.array_equal(s_dev.astype(np.float64), s64)        # exact inputs: the device's fp32 scores are the exact ones
    want = ref.classification_stats(s64.astype(np.float32), te_lab, Cn)
    acc, ap, cnt, rep = got
    assert np.array_equal(cnt, want["count"]) and np.array_equal(acc, want["accuracy"]) and rep["total_accuracy"] == want["total_accuracy"]
    assert 0.5 < rep["total_accuracy"] < 1.0
    assert (ref.ulp_diff32(ap, want["ap64"].astype(np.float32)) <= 1).all()
    assert ref.ulp_diff32([rep["mean_ap"]], [np.float32(want["mean_ap64"])])[0] <= 1


def test_argument_errors(eng):
    g = eng.gallery(np.ones((4, 3), np.float32))
    try:
        with pytest.raises(vv.VVError) as e:
            eng._chk(eng.L.vv_gallery_scores(eng.h, g.h, None, 1, None))
        assert e.value.code == 1
        with pytest.raises(vv.VVError):
            g.scores(np.ones((2, 5), np.float32))
    finally:
        g.close()
