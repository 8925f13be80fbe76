"""The linear classifier under the hinge loss (vv_linear_loss_set, then vv_linear_fit / vv_linear_grad) against tests/hinge_ref.py on
linear_ref.blobs: n = 256 items, C = 4, dim = 8.

Guard condition (not a measurement): the inputs are chosen so that in the float64 reference every |1 + t| of every step is at least
2^-10 (hinge_ref.GUARD); the fp32 logits differ from float64's by (dim + 2) 2^-24 (sum |x w| + |b|), orders of magnitude less, so the
active set m > 0 is the same in both precisions and no element needs to be excluded.  tests/test_hinge_ref_host.py asserts the
condition on the CPU for the exact seeds used here (hinge_ref.FIT_BLOB_SEED, GRAD_BLOB_SEED, GRAD_SEED).

Five steps: W, b, both histories and the loss trace against the float64 fit within 4 x the float32 restatement's own deviation from it
plus one ulp of the array's largest magnitude: tests/test_gpu_linear_fit.py's rule.

The gradient bound (vv_linear_grad against float64 at a W loaded with put), eps = 2^-23, the way tests/test_gpu_linear_fit.py counts:
  z_i      a dim-term fp32 product sum and the bias: |dz_i| <= (dim + 2) 2^-24 (sum_d |x_id w_cd| + |b_c|), the largest over c
  m        = fl(1 + t) on the same active set: |dm| <= dz_i + (eps / 2) m
  dzeta    L1: +-s1, s1 = fl(w / count): eps / 2 of its value (1 eps allowed)
           L2: +-m s2, s2 two roundings, the product one: s2 (dz_i + 2.5 eps m) (3 eps allowed)
  dW_cd    = sum_i dzeta_ic x_id: `count` fp32 products in one chain at worst: count 2^-24 sum_i |dzeta_ic x_id|
  bound_cd = sum_i |x_id| e_ic + count 2^-24 sum_i |dzeta_ic x_id|;  db: x_id = 1.
  loss     L1: w mean_i sum_c |dm|;  L2: w mean_i sum_c (2 m |dm| + dm^2);  plus eps of the loss for its one rounding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hinge_ref as hr   # noqa: E402
import linear_ref as ref   # noqa: E402
import videovector_amd as vv   # noqa: E402
from videovector_amd.synth import SyntheticVideos, init_weights   # noqa: E402

pytestmark = pytest.mark.gpu

HP = hr.FIT_HP
NORMS = ((hr.L1, "L1"), (hr.L2, "L2"))


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.set_option("lin_split_rows", 0)
    e.close()


@pytest.fixture(scope="module")
def data(eng):
    X, y = ref.blobs(seed=hr.FIT_BLOB_SEED)
    return X, y, eng.gallery(X)


@pytest.fixture(scope="module")
def grad_data(eng):
    X, y = ref.blobs(seed=hr.GRAD_BLOB_SEED)
    return X, y, eng.gallery(X)


def ref_fit(X, y, norm, iters, dtype, bias=True, **kw):
    st = ref.State(X.shape[1], 4, dtype, bias)
    trace, acc, gap = hr.fit(st, X, y, norm, iters, **kw)
    return st, trace, gap


def assert_rule(got, r32, r64, what):
    tol = 4 * np.abs(np.asarray(r32, np.float64) - r64).max() + np.spacing(np.float32(np.abs(r64).max()))
    err = np.abs(np.asarray(got, np.float64) - r64).max()
    print("HINGE %s: error %.3e, bound %.3e" % (what, err, tol))
    assert err <= tol, what


def check_five(eng, data, norm, name, bias=True, **kw):
    X, y, gal = data
    args = dict(HP, **kw)
    s64, t64, gap = ref_fit(X, y, norm, hr.FIT_STEPS, np.float64, bias, **args)
    s32, t32, _ = ref_fit(X, y, norm, hr.FIT_STEPS, np.float32, bias, **args)
    assert gap >= hr.GUARD                                                  # (the condition; asserted without a GPU too)
    lin = eng.linear(8, 4, bias=bias)
    trace, rep = lin.fit(gal, y, iters=hr.FIT_STEPS, loss="hinge", norm=name, **args)
    assert lin.loss == ("hinge", name) and eng.get_option("last_hinge_form") == 1
    W, b, hW, hb, steps = lin.get()
    lin.close()
    assert steps == hr.FIT_STEPS and rep["steps"] == hr.FIT_STEPS and rep["nonfinite_rows"] == 0
    for what, got in (("W", W), ("b", b), ("hW", hW), ("hb", hb)):
        if bias or what in ("W", "hW"):
            assert_rule(got, getattr(s32, what), getattr(s64, what), "%s %s" % (name, what))
        else:
            assert not got.any()
    assert_rule(trace, t32, t64, "%s loss trace" % name)
    assert rep["loss_first"] == trace[0] and rep["loss_last"] == trace[-1]
    return W, b, hW, hb, trace


@pytest.mark.parametrize("norm,name", NORMS)
@pytest.mark.parametrize("batch", hr.FIT_BATCHES)
def test_five_steps_match_float64(eng, data, norm, name, batch):
    check_five(eng, data, norm, name, batch=batch)


@pytest.mark.parametrize("norm,name", NORMS)
def test_five_steps_without_bias(eng, data, norm, name):
    check_five(eng, data, norm, name, bias=False, batch=100)


@pytest.mark.parametrize("norm,name", NORMS)
@pytest.mark.parametrize("split_rows,want", [(256, (1, 1)), (96, (3, 1)), (1, (128, 2))])
def test_gradient_matches_float64(eng, grad_data, norm, name, split_rows, want):
    """lin_split_rows 256: one split of the full batch; 96: three (96 + 96 + 64); 1: 128 splits per row block, so two row blocks."""
    X, y, gal = grad_data
    W, b = hr.grad_params()
    lin = eng.linear(8, 4)
    lin.put(W=W, b=b)
    lin.set_loss("hinge", name)
    try:
        eng.set_option("lin_split_rows", split_rows)
        for k, (first, count, w) in enumerate(hr.GRAD_CASES):
            dW, db, loss = lin.grad(gal, y, first, count, w)
            if k == 0:
                assert (eng.get_option("last_lin_splits"), eng.get_option("last_lin_blocks")) == want
            st = ref.State(8, 4)
            st.W, st.b = W.astype(np.float64), b.astype(np.float64)
            Xb, yb = X[first:first + count].astype(np.float64), y[first:first + count]
            rW, rb, rloss, _, gap = hr.gradient(st, Xb, yb, norm, w)
            assert gap >= hr.GUARD
            z = Xb @ st.W.T + st.b
            sign = np.ones_like(z)
            sign[np.arange(count), yb] = -1.0
            m = np.maximum(0.0, 1.0 + sign * z)
            dzl = ((8 + 2) * 2.0 ** -24 * (np.abs(Xb) @ np.abs(st.W).T + np.abs(st.b)).max(axis=1))[:, None]
            assert dzl.max() < hr.GUARD / 64
            dm = (m > 0) * (dzl + ref.EPS / 2 * m)
            if norm == hr.L1:
                dzeta = (m > 0) * (w / count)
                e_dz = ref.EPS * dzeta
                loss_b = w * dm.sum() / count
            else:
                s2 = 2.0 * w / count
                dzeta = m * s2
                e_dz = s2 * (m > 0) * (dzl + 3 * ref.EPS * m)
                loss_b = w * (2 * m * dm + dm * dm).sum() / count
            chain = count * 2.0 ** -24
            bW = e_dz.T @ np.abs(Xb) + chain * (dzeta.T @ np.abs(Xb))
            bb = e_dz.sum(axis=0) + chain * dzeta.sum(axis=0)
            print("HINGE %s grad count %d split_rows %d: dW at %.3f of its bound, db at %.3f, loss at %.3f" %
                  (name, count, split_rows, (np.abs(dW - rW) / bW).max(), (np.abs(db - rb) / bb).max(), abs(float(loss) - rloss) / (loss_b + ref.EPS * abs(rloss))))
            assert (np.abs(dW - rW) <= bW).all() and (np.abs(db - rb) <= bb).all()
            assert abs(float(loss) - rloss) <= loss_b + ref.EPS * abs(rloss)
    finally:
        eng.set_option("lin_split_rows", 0)
    assert np.array_equal(lin.get()[0], W)                               # nothing was updated
    lin.close()


@pytest.mark.parametrize("norm,name", NORMS)
@pytest.mark.parametrize("batch", hr.FIT_BATCHES)
def test_sixty_steps_classify_everything_and_feed_the_statistics(eng, data, norm, name, batch):
    X, y, gal = data
    lin = eng.linear(8, 4)
    lin.set_loss("hinge", name)
    _, rep = lin.fit(gal, y, iters=60, batch=batch, **HP)
    assert rep["accuracy_last"] == 1.0 and rep["loss_last"] < rep["loss_first"]
    from_host, from_gallery = lin.scores(X), lin.scores(gal)
    assert np.array_equal(from_host.get(), from_gallery.get())
    acc, ap, cnt, r = eng.classification_stats(from_gallery, y, 4)      # the scores are read on the device
    assert r["total_accuracy"] == 1.0 and (ap == 1.0).all() and (cnt == 64).all()
    lin.close()


@pytest.mark.parametrize("norm,name", NORMS)
def test_fits_reproduce_and_the_cursor_is_carried(eng, data, norm, name):
    X, y, gal = data

    def fresh(iters):
        lin = eng.linear(8, 4)
        trace, _ = lin.fit(gal, y, iters=iters, batch=100, loss="hinge", norm=name, **HP)
        return lin, trace
    a, ta = fresh(5)
    b, tb = fresh(5)
    assert all(np.array_equal(u, v) for u, v in zip(a.get()[:4], b.get()[:4])) and ta.tobytes() == tb.tobytes()
    c, tc = fresh(3)
    tc2, _ = c.fit(gal, y, iters=2, batch=100, **HP)                     # 100, 100, 56 | 100, 100; the loss stays set
    assert c.loss == ("hinge", name)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a.get()[:4], c.get()[:4])) and ta.tobytes() == np.concatenate([tc, tc2]).tobytes()
    assert a.get()[4] == c.get()[4] == 5
    for lin in (a, b, c):
        lin.close()


def test_switching_the_loss_moves_nothing(eng, data):
    """SOFTMAX -> HINGE -> SOFTMAX around a softmax fit: parameters, histories, step counter, cursor and the following softmax fit are
    those of an object that never switched."""
    X, y, gal = data
    plain, switched = eng.linear(8, 4), eng.linear(8, 4)
    assert plain.loss == ("softmax", None)
    t0 = plain.fit(gal, y, iters=3, batch=100, **HP)[0]
    t1 = switched.fit(gal, y, iters=3, batch=100, **HP)[0]
    before = switched.get()
    switched.set_loss("hinge", "L1")
    assert switched.loss == ("hinge", "L1")
    switched.set_loss("hinge", "L2")
    switched.set_loss("softmax")
    assert switched.loss == ("softmax", None)
    after = switched.get()
    assert all(u.tobytes() == v.tobytes() for u, v in zip(before[:4], after[:4])) and before[4] == after[4] == 3
    t2 = plain.fit(gal, y, iters=4, batch=100, **HP)[0]                   # from the cursor: 100, 100, 56, 100
    t3 = switched.fit(gal, y, iters=4, batch=100, **HP)[0]
    assert t0.tobytes() == t1.tobytes() and t2.tobytes() == t3.tobytes()
    assert all(u.tobytes() == v.tobytes() for u, v in zip(plain.get()[:4], switched.get()[:4])) and plain.get()[4] == switched.get()[4] == 7
    # and a hinge fit in between does move the parameters, so the comparison above compares something
    switched.fit(gal, y, iters=1, loss="hinge", norm="L1", **HP)
    assert not np.array_equal(plain.get()[0], switched.get()[0])
    plain.close()
    switched.close()


def test_nonfinite_rows_are_counted(eng):
    X, y = ref.blobs(n=40)
    X[5, 2] = np.inf
    gal = eng.gallery(X)
    lin = eng.linear(8, 4)
    _, rep = lin.fit(gal, y, iters=2, batch=0, loss="hinge", norm="L2", **HP)      # step 1: row 5's logits are 0 * inf; step 2: W is NaN
    assert rep["nonfinite_rows"] == 1 + 40
    lin.close()


def test_a_hinge_fit_between_backward_and_update_changes_nothing(data):
    X, y, _ = data
    ds = SyntheticVideos(seed=1701, n_videos=50)
    idx = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=32, context_size=5, num_negative_samples=2, max_buffer_size=500,
                     negative_swap_percentage=50).next()
    W0, b0 = init_weights(1, 32, 128, std=0.02)
    cfg = vv.StepConfig(32, 5, 2, lr=0.01)
    outs = []
    for with_fit in (False, True):
        e = vv.Engine(0, "f16")
        e.table_synth(ds.seed, ds.n_rows, 128)
        e.params_set(W0, b0)
        e.forward_backward(cfg, idx)
        if with_fit:
            lin = e.linear(8, 4)
            lin.fit(e.gallery(X), y, iters=3, batch=100, loss="hinge", norm="L1", **HP)
            lin.close()
        e.apply_update(cfg)
        outs.append(e.params_get())
        e.close()
    assert all(np.array_equal(u, v) for u, v in zip(outs[0], outs[1]))


def test_bad_arguments_are_refused(eng, data):
    X, y, gal = data
    lin = eng.linear(8, 4)
    other_eng = vv.Engine(0, "f16")
    foreign = other_eng.linear(8, 4)
    L = eng.L
    loss, norm = vv.engine.C.c_int32(), vv.engine.C.c_int32()
    for call in (lambda: L.vv_linear_loss_set(eng.h, lin.h, 2, hr.L2), lambda: L.vv_linear_loss_set(eng.h, lin.h, -1, hr.L2),
                 lambda: L.vv_linear_loss_set(eng.h, lin.h, hr.HINGE, 0), lambda: L.vv_linear_loss_set(eng.h, lin.h, hr.HINGE, 3),
                 lambda: L.vv_linear_loss_set(eng.h, foreign.h, hr.HINGE, hr.L2), lambda: L.vv_linear_loss_set(eng.h, None, hr.HINGE, hr.L2),
                 lambda: L.vv_linear_loss_get(eng.h, foreign.h, vv.engine.C.byref(loss), vv.engine.C.byref(norm))):
        with pytest.raises(vv.VVError):
            eng._chk(call())
    assert lin.loss == ("softmax", None)                                  # a refused call changed nothing
    eng._chk(L.vv_linear_loss_set(eng.h, lin.h, hr.SOFTMAX, 99))          # the norm is read for HINGE only
    with pytest.raises(vv.VVError):
        lin.set_loss("logistic")
    with pytest.raises(vv.VVError):
        lin.set_loss("hinge", "L3")
    lin.set_loss("hinge", "L1")
    bad = y.copy()
    bad[9] = 4
    for call in (lambda: lin.fit(gal, bad, iters=1), lambda: lin.fit(gal, y, iters=0), lambda: lin.grad(gal, y, 250, 7)):
        with pytest.raises(vv.VVError):
            call()
    foreign.close()
    other_eng.close()
    lin.close()
