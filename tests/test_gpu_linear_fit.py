"""The softmax linear classifier on the device (vv_linear_*) against tests/linear_ref.py on the blob inputs: n = 256 items, C = 4,
dim = 8, label i % 4, class mean 3 e_c, noise 0.5 N(0, 1) from RandomState(7) rounded to fp32.  The five-step rule and the gradient
bound are written in dim, C and count, and also run at 515 x 130 x 33 (Dp 160, Cp 64: two column tiles of the weight gradient, five
splits) and 300 x 40 x 3 with ragged batches; the hinge loss is held exactly at such shapes by tests/test_gpu_linear_step_exact.py.

Five steps: W, b, both histories and the loss trace against the float64 fit within 4 x the float32 restatement's own deviation from
it (largest over the array) plus one ulp of the array's largest magnitude -- the project's rule of test_gpu_score_seg_exact.py.

The gradient bound (vv_linear_grad against float64 at a W loaded with put), eps = 2^-23:
  z_i      a dim-term fp32 product sum and the bias: |dz_i| <= (dim + 2) 2^-24 (sum_d |x_id w_cd| + |b_c|), the largest over c
  p_i      the softmax test's relative bound R_i = p_bound(C, T_i + 2 dz_i) on top of the logits' own shift, which moves p by at most
           2 dz_i relatively (numerator and denominator by dz_i each)
  dzeta    (p - onehot) scale: one subtraction and one product, 2 eps of its value; scale itself within eps / 2
  dW_cd    = sum_i dzeta_ic x_id: `count` fp32 products in one chain at worst (split-K shortens it): count 2^-24 sum_i |dzeta_ic x_id|
  bound_cd = sum_i |x_id| scale (p_ic (R_i + 2 dz_i) + 3 eps |p_ic - onehot|) + count 2^-24 sum_i |dzeta_ic x_id|;  db: x_id = 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_ref as ref   # noqa: E402
import videovector_amd as vv   # noqa: E402
from videovector_amd.synth import SyntheticVideos, init_weights   # noqa: E402

pytestmark = pytest.mark.gpu

HP = dict(lr=0.5, momentum=0.9, weight_decay=1e-4)
BLOBS = (256, 8, 4)                               # (n, dim, C): linear_ref.blobs' defaults
LARGER = {(515, 130, 33): 41, (300, 40, 3): 42}   # ... and the seeds of the larger shapes


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.set_option("lin_split_rows", 0)
    e.close()


@pytest.fixture(scope="module")
def data(eng):
    X, y = ref.blobs()
    return X, y, eng.gallery(X)


@pytest.fixture(scope="module")
def sets(eng, data):
    """{(n, dim, C): (X, y, gallery)}; never written to."""
    out = {BLOBS: data}
    for (n, dim, C), seed in LARGER.items():
        X, y = ref.blobs(n=n, C=C, dim=dim, seed=seed)
        out[(n, dim, C)] = (X, y, eng.gallery(X))
    return out


def ref_fit(X, y, iters, dtype, bias=True, **kw):
    st = ref.State(X.shape[1], int(y.max()) + 1, dtype, bias)
    trace, acc = ref.fit(st, X, y, iters, **kw)
    return st, trace, acc


def assert_rule(got, r32, r64, what):
    tol = 4 * np.abs(np.asarray(r32, np.float64) - r64).max() + np.spacing(np.float32(np.abs(r64).max()))
    err = np.abs(np.asarray(got, np.float64) - r64).max()
    print("LINEAR %s: error %.3e, bound %.3e" % (what, err, tol))
    assert err <= tol, what


def check_five(eng, data, bias=True, schedule=None, **kw):
    X, y, gal = data
    args = dict(HP, **kw)
    if schedule is not None:
        args["lr_schedule"] = schedule
    s64, t64, _ = ref_fit(X, y, 5, np.float64, bias, **args)
    s32, t32, _ = ref_fit(X, y, 5, np.float32, bias, **args)
    lin = eng.linear(X.shape[1], int(y.max()) + 1, bias=bias)
    trace, rep = lin.fit(gal, y, iters=5, **args)
    W, b, hW, hb, steps = lin.get()
    lin.close()
    assert steps == 5 and rep["steps"] == 5 and rep["nonfinite_rows"] == 0
    for name, got in (("W", W), ("b", b), ("hW", hW), ("hb", hb)):
        if bias or name in ("W", "hW"):
            assert_rule(got, getattr(s32, name), getattr(s64, name), name)
        else:
            assert not got.any()
    assert_rule(trace, t32, t64, "loss trace")
    assert rep["loss_first"] == trace[0] and rep["loss_last"] == trace[-1]
    return W, b, hW, hb, trace


@pytest.mark.parametrize("batch,shape", [pytest.param(0, BLOBS, id="0"), pytest.param(64, BLOBS, id="64"), pytest.param(100, BLOBS, id="100"),
                                         pytest.param(0, (515, 130, 33), id="515x130x33-0"), pytest.param(200, (515, 130, 33), id="515x130x33-200"),
                                         pytest.param(0, (300, 40, 3), id="300x40x3-0"), pytest.param(128, (300, 40, 3), id="300x40x3-128")])
def test_five_steps_match_float64(eng, sets, batch, shape):
    """Batches of 200 over 515 items: 200, 200, 115, 200, 200; of 128 over 300: 128, 128, 44, 128, 128."""
    check_five(eng, sets[shape], batch=batch)


def test_five_steps_without_bias_and_with_a_schedule(eng, data):
    check_five(eng, data, bias=False, batch=100)
    sched = np.array([0.5, 0.25, 0.5, 0.125, 0.3], np.float32)
    a = check_five(eng, data, batch=64, schedule=sched)
    X, y, gal = data
    lin = eng.linear(8, 4)
    lin.fit(gal, y, iters=5, batch=64, lr_schedule=np.full(5, 0.5, np.float32), **dict(HP, lr=123.0))      # the schedule replaces cfg.lr
    b = check_five(eng, data, batch=64)
    assert np.array_equal(lin.get()[0], b[0]) and not np.array_equal(a[0], b[0])
    lin.close()


@pytest.mark.parametrize("shape", [BLOBS] + list(LARGER), ids=lambda s: "%dx%dx%d" % s)
def test_gradient_matches_float64(eng, sets, shape):
    X, y, gal = sets[shape]
    n, dim, C = shape
    rs = np.random.RandomState(3)
    W, b = (0.5 * rs.randn(C, dim)).astype(np.float32), (0.5 * rs.randn(C)).astype(np.float32)
    lin = eng.linear(dim, C)
    lin.put(W=W, b=b)
    for first, count, w in ((0, n, 1.0), (37, 100, 0.25)):
        dW, db, loss = lin.grad(gal, y, first, count, w)
        st = ref.State(dim, C)
        st.W, st.b = W.astype(np.float64), b.astype(np.float64)
        Xb, yb = X[first:first + count].astype(np.float64), y[first:first + count]
        rW, rb, rloss, _ = ref.gradient(st, Xb, yb, w)
        z = Xb @ st.W.T + st.b
        p = ref.softmax_loss(z, yb, w)[0]
        dzl = (dim + 2) * 2.0 ** -24 * (np.abs(Xb) @ np.abs(st.W).T + np.abs(st.b)).max(axis=1)
        R = np.array([ref.p_bound(C, t) for t in (z.max(axis=1) - z.min(axis=1)) + 2 * dzl])
        onehot = np.zeros_like(p)
        onehot[np.arange(count), yb] = 1.0
        scale = w / count
        e_dz = scale * (p * (R + 2 * dzl)[:, None] + 3 * ref.EPS * np.abs(p - onehot))
        chain = count * 2.0 ** -24
        bW = e_dz.T @ np.abs(Xb) + chain * (np.abs((p - onehot) * scale).T @ np.abs(Xb))
        bb = e_dz.sum(axis=0) + chain * np.abs((p - onehot) * scale).sum(axis=0)
        print("LINEAR grad %dx%dx%d count %d: dW at %.3f of its bound, db at %.3f" % (n, dim, C, count, (np.abs(dW - rW) / bW).max(), (np.abs(db - rb) / bb).max()))
        assert (np.abs(dW - rW) <= bW).all() and (np.abs(db - rb) <= bb).all()
        assert abs(float(loss) - rloss) <= (R + 2 * dzl + 3 * ref.EPS * 88).mean() * w + ref.EPS * abs(rloss)
    assert np.array_equal(lin.get()[0], W)                               # nothing was updated
    lin.close()


@pytest.mark.parametrize("batch", [0, 64, 100])
def test_sixty_steps_classify_everything(eng, data, batch):
    X, y, gal = data
    lin = eng.linear(8, 4)
    _, rep = lin.fit(gal, y, iters=60, batch=batch, **HP)
    assert rep["accuracy_last"] == 1.0
    from_host, from_gallery = lin.scores(X), lin.scores(gal)
    assert np.array_equal(from_host.get(), from_gallery.get())
    for buf in (from_host, from_gallery):
        acc, ap, cnt, r = eng.classification_stats(buf, y, 4)
        assert r["total_accuracy"] == 1.0 and (ap == 1.0).all()
    lin.close()


def test_fits_reproduce_and_resume(eng, data):
    X, y, gal = data

    def fresh(iters, **kw):
        lin = eng.linear(8, 4)
        trace, _ = lin.fit(gal, y, iters=iters, batch=100, **dict(HP, **kw))
        return lin, trace
    a, ta = fresh(5)
    b, tb = fresh(5)
    assert all(np.array_equal(u, v) for u, v in zip(a.get()[:4], b.get()[:4])) and np.array_equal(ta, tb)
    c, tc = fresh(3)
    tc2, _ = c.fit(gal, y, iters=2, batch=100, **HP)                     # the cursor is carried: 100, 100, 56 | 100, 100
    assert all(np.array_equal(u, v) for u, v in zip(a.get()[:4], c.get()[:4])) and np.array_equal(ta, np.concatenate([tc, tc2]))
    # get -> put into a fresh object at an epoch boundary (put returns the cursor to 0) continues identically
    d, _ = fresh(3)
    e = eng.linear(8, 4)
    W, bb, hW, hb, steps = d.get()
    e.put(W, bb, hW, hb, steps)
    t1, r1 = d.fit(gal, y, iters=4, batch=100, **HP)
    t2, r2 = e.fit(gal, y, iters=4, batch=100, **HP)
    assert np.array_equal(t1, t2) and r1["steps"] == r2["steps"] == 7
    assert all(np.array_equal(u, v) for u, v in zip(d.get()[:4], e.get()[:4]))
    for lin in (a, b, c, d, e):
        lin.close()


def test_splits_and_row_blocks(eng, data):
    """lin_split_rows = 96: three splits of the full batch (96 + 96 + 64).  lin_split_rows = 1: a row block holds 128 splits, so the
    256 rows run in two row blocks, the second adding into the first's slabs.  Both within the five-step bound."""
    try:
        eng.set_option("lin_split_rows", 96)
        check_five(eng, data, batch=0)
        assert (eng.get_option("last_lin_splits"), eng.get_option("last_lin_blocks")) == (3, 1)
        eng.set_option("lin_split_rows", 1)
        check_five(eng, data, batch=0)
        assert (eng.get_option("last_lin_splits"), eng.get_option("last_lin_blocks")) == (128, 2)
    finally:
        eng.set_option("lin_split_rows", 0)


def test_nonfinite_rows_are_counted(eng):
    X, y = ref.blobs(n=40)
    X[5, 2] = np.inf
    gal = eng.gallery(X)
    lin = eng.linear(8, 4)
    _, rep = lin.fit(gal, y, iters=2, batch=0, **HP)                     # step 1: row 5's logits are 0 * inf; step 2: W is NaN
    assert rep["nonfinite_rows"] == 1 + 40
    lin.close()


def test_a_fit_between_backward_and_update_changes_nothing(data):
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
            lin.fit(e.gallery(X), y, iters=3, batch=100, **HP)
            lin.close()
        e.apply_update(cfg)
        outs.append(e.params_get())
        e.close()
    assert all(np.array_equal(u, v) for u, v in zip(outs[0], outs[1]))


def test_bad_arguments_are_refused(eng, data):
    X, y, gal = data
    for C_ in (0, 4097):
        with pytest.raises(vv.VVError):
            eng.linear(8, C_)
    lin, other = eng.linear(8, 4), eng.linear(7, 4)
    bad = y.copy()
    bad[9] = 4
    neg = y.copy()
    neg[0] = -1
    for call in (lambda: other.fit(gal, y, iters=1), lambda: lin.fit(gal, bad, iters=1), lambda: lin.fit(gal, neg, iters=1),
                 lambda: lin.fit(gal, y, iters=0), lambda: lin.fit(gal, y, iters=1, batch=-1), lambda: lin.grad(gal, y, -1, 4),
                 lambda: lin.grad(gal, y, 250, 7), lambda: lin.grad(gal, y, 0, 0), lambda: lin.grad(gal, bad, 0, 4),
                 lambda: other.scores(gal), lambda: other.grad(gal, y, 0, 4)):
        with pytest.raises(vv.VVError):
            call()
    out = lin.scores(X[:3])
    for src, q in ((gal.h, X.ctypes.data), (None, None)):                # both sources, or neither
        with pytest.raises(vv.VVError):
            eng._chk(eng.L.vv_linear_scores(eng.h, lin.h, src, q, 256, out.ptr))
    lin.close()
    other.close()
