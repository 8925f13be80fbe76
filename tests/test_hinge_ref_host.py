"""Host tests of the hinge loss's restatement (tests/hinge_ref.py): hand-worked cases for both norms, the float64 gradient against
central differences on inputs kept away from the kink, a direct transcription of the formulas at cols = 1, the NaN rule, and the
guard condition of tests/test_gpu_linear_hinge_fit.py -- every |1 + t| of the float64 runs at least 2^-10 -- on exactly the seeds
those tests use.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hinge_ref as hr   # noqa: E402
import linear_ref as ref   # noqa: E402


def test_hand_worked_cases():
    # row 0, label 1: t = (0.5, -2, -3) -> m = (1.5, 0, 0);  row 1, label 0: t = (0.25, 0, -1) -> m = (1.25, 1, 0)
    z = np.array([[0.5, 2.0, -3.0], [-0.25, 0.0, -1.0]])
    y = np.array([1, 0])
    dz, loss, correct, gap = hr.hinge_loss(z, y, hr.L1, 0.5)
    assert loss == 0.5 * (1.5 + 1.25 + 1.0) / 2 and correct == 1 and gap == 0.0
    assert np.array_equal(dz, np.array([[0.25, 0.0, 0.0], [-0.25, 0.25, 0.0]]))
    dz, loss, correct, _ = hr.hinge_loss(z, y, hr.L2, 0.5)
    assert loss == 0.5 * (2.25 + 1.5625 + 1.0) / 2 and correct == 1
    assert np.array_equal(dz, np.array([[0.75, 0.0, 0.0], [-0.625, 0.5, 0.0]]))
    for norm in (hr.L1, hr.L2):
        d32, l32, c32, l64 = hr.hinge_loss_f32(z, y, norm, 0.5)             # every value here is exact in fp32
        d64, want, _, _ = hr.hinge_loss(z, y, norm, 0.5)
        assert np.array_equal(d32, d64) and float(l32) == want == l64 and c32 == 1 and d32.dtype == np.float32


def test_logits_of_exactly_one_sit_on_the_kink():
    z = np.array([[1.0, -1.0, -0.0]])
    for norm in (hr.L1, hr.L2):
        dz, loss, _, gap = hr.hinge_loss(z, np.array([0]), norm)
        assert gap == 0.0 and loss == 1.0 and np.array_equal(dz[0, :2], [0.0, 0.0]) and dz[0, 2] == (1.0 if norm == hr.L1 else 2.0)


def test_one_column_is_the_binary_formula():
    rs = np.random.RandomState(4)
    z = rs.randn(50, 1)
    y = np.zeros(50, np.int64)                       # the only column is every row's label: t = -z
    m = np.maximum(0.0, 1.0 - z[:, 0])
    for norm, want, wdz in ((hr.L1, 0.7 * m.sum() / 50, -1.0 * (m > 0) * (0.7 / 50)), (hr.L2, 0.7 * (m * m).sum() / 50, -m * (0.7 * 2.0 / 50))):
        dz, loss, correct, _ = hr.hinge_loss(z, y, norm, 0.7)
        assert abs(loss - want) <= 1e-15 * abs(want) and np.allclose(dz[:, 0], wdz, rtol=1e-15, atol=0) and correct == 50


def test_nan_gives_zero_and_infinity_stays():
    z = np.array([[np.nan, 0.0, np.nan], [np.inf, -np.inf, 0.0], [-np.inf, np.inf, 0.0]], np.float32)
    y = np.array([2, 0, 0])
    for norm in (hr.L1, hr.L2):
        for dz, loss in (hr.hinge_loss(z[:2], y[:2], norm)[:2], hr.hinge_loss_f32(z[:2], y[:2], norm)[:2]):
            assert float(loss) == 1.0 and not dz[0, [0, 2]].any() and not dz[1, :2].any()      # (only the two zeros count: m = 1 each)
        dz, loss, correct, l64 = hr.hinge_loss_f32(z, y, norm)
        assert np.isinf(loss) and l64 == np.inf and correct == 1 and hr.nonfinite_rows(z) == 3    # (row 1's +Inf is its label)
    assert list(ref.first_max(z)) == [1, 0, 1]


def test_gradient_matches_central_differences():
    rs = np.random.RandomState(1)
    X, y = ref.blobs(n=24, C=3, dim=5, seed=2)
    st = ref.State(5, 3)
    st.W, st.b = rs.randn(3, 5), rs.randn(3)
    h = 1e-6
    for norm in (hr.L1, hr.L2):
        dW, db, _, _, gap = hr.gradient(st, X, y, norm, loss_weight=0.25)
        assert gap > 1e-3                            # every margin is further from the kink than any difference step moves it

        def loss_at(W, b):
            s = ref.State(5, 3)
            s.W, s.b = W, b
            return hr.gradient(s, X, y, norm, loss_weight=0.25)[2]
        for c in range(3):
            for d in range(5):
                Wp, Wm = st.W.copy(), st.W.copy()
                Wp[c, d] += h
                Wm[c, d] -= h
                assert abs((loss_at(Wp, st.b) - loss_at(Wm, st.b)) / (2 * h) - dW[c, d]) < 1e-8
            bp, bm = st.b.copy(), st.b.copy()
            bp[c] += h
            bm[c] -= h
            assert abs((loss_at(st.W, bp) - loss_at(st.W, bm)) / (2 * h) - db[c]) < 1e-8


def test_lanes_and_rows_per_pass():
    assert [hr.lanes_of(c) for c in (1, 3, 4, 5, 13, 31, 32, 33, 128, 129, 256, 257, 4096)] == [1, 1, 1, 2, 4, 8, 8, 16, 32, 64, 64, 64, 64]
    assert hr.rows_per_pass(1) == 131072 and hr.rows_per_pass(4096) == 2048
    assert hr.form_of(32) == 1 and hr.form_of(33) == 2 and hr.form_of(32, 1, 1) == 2 and hr.form_of(32, 4, 4) == 1


def test_the_fit_tests_inputs_keep_clear_of_the_kink():
    """The guard condition of test_gpu_linear_hinge_fit.py, for the exact inputs it uses: no element is excluded there because none
    needs to be."""
    X, y = ref.blobs(seed=hr.FIT_BLOB_SEED)
    for norm in (hr.L1, hr.L2):
        for batch in hr.FIT_BATCHES:
            st = ref.State(8, 4)
            _, _, gap = hr.fit(st, X, y, norm, hr.FIT_STEPS, batch=batch, **hr.FIT_HP)
            assert gap >= hr.GUARD, (norm, batch, gap)
        st = ref.State(8, 4, bias=False)
        _, _, gap = hr.fit(st, X, y, norm, hr.FIT_STEPS, batch=100, **hr.FIT_HP)
        assert gap >= hr.GUARD, (norm, "no bias", gap)
    X, y = ref.blobs(seed=hr.GRAD_BLOB_SEED)
    W, b = hr.grad_params()
    st = ref.State(8, 4)
    st.W, st.b = W.astype(np.float64), b.astype(np.float64)
    for first, count, w in hr.GRAD_CASES:
        gap = hr.gradient(st, X[first:first + count], y[first:first + count], hr.L1, w)[4]
        assert gap >= hr.GUARD, (first, count, gap)
        # the fp32 logits' distance from float64's is far below the guard: (dim + 2) 2^-24 (sum |x w| + |b|)
        Xb = X[first:first + count].astype(np.float64)
        assert ((8 + 2) * 2.0 ** -24 * (np.abs(Xb) @ np.abs(st.W).T + np.abs(st.b))).max() < hr.GUARD / 64


def test_blob_fit_separates_the_classes():
    X, y = ref.blobs(seed=hr.FIT_BLOB_SEED)
    for norm in (hr.L1, hr.L2):
        for batch in hr.FIT_BATCHES:
            st = ref.State(8, 4)
            trace, acc, _ = hr.fit(st, X, y, norm, 60, batch=batch, **hr.FIT_HP)
            z = X.astype(np.float64) @ st.W.T + st.b
            assert acc == 1.0 and (np.argmax(z, axis=1) == y).all() and trace[-1] < trace[0]
