"""The linear classifier on row lists (vv_linear_fit_rows / _grad_rows / _scores_rows, Linear.cross_validate).

The oracle needs NO tolerance: a call over a list L of gallery items must equal, bit for bit, the existing contiguous call on a second
gallery built from X[L] with labels y[L] -- the same arithmetic in the same order on the same values; the gathered forms of the two
products differ from the contiguous ones in a row's address only.  The contiguous path itself is held to float64 at these shapes by
tests/test_gpu_linear_step_exact.py (the whole hinge step, bit for bit) and tests/test_gpu_linear_fit.py (softmax, within its derived
bounds); the loss kernels alone by test_gpu_softmax_exact.py and test_gpu_hinge_exact.py.

Shapes are where a gather can go wrong: n_ref 300 .. 700, dim 40 / 64 / 130 (Dp 64 / 64 / 160: padded and unpadded rows), C 3 / 33 (Cp 32 /
64), list lengths on both sides of the 128-row tile and the 32-row K-tile, 1 / 3 / 128 splits and two row blocks, every loss, with and
without bias."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_ref as ref   # noqa: E402
import videovector_amd as vv   # noqa: E402
from videovector_amd.engine import cv_best, cv_mean   # noqa: E402
from videovector_amd.synth import SyntheticVideos, init_weights   # noqa: E402

pytestmark = pytest.mark.gpu

VV_ERR_ARG = 1
SHAPES = ((300, 40, 3), (515, 130, 33), (700, 64, 33))          # (n_ref, dim, C)
LOSSES = (("softmax", None), ("hinge", "L1"), ("hinge", "L2"))
HP = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)
LENGTHS = (1, 31, 33, 127, 129, 257)


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.set_option("lin_split_rows", 0)
    e.close()


@pytest.fixture(scope="module")
def sets(eng):
    """{shape: (X, y, gallery)}; X and y are never written to."""
    out = {}
    for k, (n, dim, C) in enumerate(SHAPES):
        X, y = ref.blobs(n=n, C=C, dim=dim, seed=31 + k)
        out[(n, dim, C)] = (X, y, eng.gallery(X))
    return out


def new_lin(eng, dim, C, loss, bias=True, seed=None):
    lin = eng.linear(dim, C, bias=bias)
    if loss[0] == "hinge":
        lin.set_loss("hinge", loss[1])
    if seed is not None:
        rs = np.random.RandomState(seed)
        lin.put(W=(0.3 * rs.randn(C, dim)).astype(np.float32), b=(0.3 * rs.randn(C)).astype(np.float32))
    return lin


def snapshot(lin):
    W, b, hW, hb, steps = lin.get()
    return (W.tobytes(), b.tobytes(), hW.tobytes(), hb.tobytes(), steps)


def same_report(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def lists_of(n, rs):
    """The lists of the 'any list' tests: a permutation, one with repeats, one longer than n_ref, and the edge lengths."""
    out = [rs.permutation(n), rs.randint(0, n, n), rs.randint(0, n, n + 77)]
    out += [rs.permutation(n)[:k] if k > 1 else np.array([n - 1]) for k in LENGTHS]
    return [np.ascontiguousarray(L, dtype=np.int32) for L in out]


# ---------------------------------------------------------------------------------------------- identity list
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_identity_list_equals_the_contiguous_fit(eng, sets, shape, loss):
    n, dim, C = shape
    X, y, gal = sets[shape]
    ident = np.arange(n, dtype=np.int32)
    # one split; three; 128 splits of 1 .. 3 rows in two row blocks (test_gpu_linear_hinge_fit.py's gradient settings, scaled to n)
    per_block = -(-n // 256)
    plans = ((n, (1, 1)), (-(-n // 3), (3, 1)), (per_block, (128, -(-n // (128 * per_block)))))
    try:
        for split_rows, want in plans:
            eng.set_option("lin_split_rows", split_rows)
            for batch in (0, 97):
                for bias in (True, False):
                    a, b = new_lin(eng, dim, C, loss, bias), new_lin(eng, dim, C, loss, bias)
                    ta, ra = a.fit(gal, y, iters=4, batch=batch, **HP)
                    if batch == 0:
                        assert (eng.get_option("last_lin_splits"), eng.get_option("last_lin_blocks")) == want
                    assert eng.get_option("last_lin_gather") == 1
                    tb, rb = b.fit(gal, y, iters=4, batch=batch, rows=ident, **HP)
                    if batch == 0:
                        assert (eng.get_option("last_lin_splits"), eng.get_option("last_lin_blocks")) == want
                    assert eng.get_option("last_lin_gather") == 2
                    assert snapshot(a) == snapshot(b) and ta.tobytes() == tb.tobytes() and same_report(ra, rb)
                    assert ra["nonfinite_rows"] == 0 and a.get()[0].any()
                    a.close()
                    b.close()
    finally:
        eng.set_option("lin_split_rows", 0)


# ---------------------------------------------------------------------------------------------- any list
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_any_list_equals_the_fit_on_the_listed_rows(eng, sets, shape, loss):
    """fit(G, y, rows=L) == fit(gallery(X[L]), y[L]) for every list; whole-list steps and 5 steps of a batch that leaves a ragged last
    batch and wraps the position (len 257, batch 100: 100, 100, 57, 100, 100)."""
    n, dim, C = shape
    X, y, gal = sets[shape]
    for k, L in enumerate(lists_of(n, np.random.RandomState(5))):
        twin_gal = eng.gallery(X[L])
        for batch, bias in ((0, True), (100, k % 2 == 0)):
            a, b = new_lin(eng, dim, C, loss, bias), new_lin(eng, dim, C, loss, bias)
            ta, ra = a.fit(gal, y, iters=5, batch=batch, rows=L, **HP)
            assert eng.get_option("last_lin_gather") == 2
            tb, rb = b.fit(twin_gal, y[L], iters=5, batch=batch, **HP)
            assert eng.get_option("last_lin_gather") == 1
            assert snapshot(a) == snapshot(b), "list %d (%d entries), batch %d" % (k, len(L), batch)
            assert ta.tobytes() == tb.tobytes() and same_report(ra, rb) and ra["steps"] == 5 and ra["nonfinite_rows"] == 0
            a.close()
            b.close()
        twin_gal.close()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("loss", LOSSES)
def test_any_list_gradient(eng, sets, shape, loss):
    n, dim, C = shape
    X, y, gal = sets[shape]
    lin = new_lin(eng, dim, C, loss, seed=3)
    before = snapshot(lin)
    try:
        for k, L in enumerate(lists_of(n, np.random.RandomState(6))):
            twin_gal = eng.gallery(X[L])
            # the library's plan, and splits of 32 rows: the tail tile of a split and the zero-filled rows behind k_end
            for split_rows in (0, 32):
                eng.set_option("lin_split_rows", split_rows)
                dW, db, l0 = lin.grad(gal, y, rows=L, loss_weight=0.75)
                assert eng.get_option("last_lin_gather") == 2
                rW, rb, l1 = lin.grad(twin_gal, y[L], loss_weight=0.75)
                assert dW.tobytes() == rW.tobytes() and db.tobytes() == rb.tobytes() and l0.tobytes() == l1.tobytes(), (k, len(L), split_rows)
                assert np.isfinite(dW).all() and dW.any()
            twin_gal.close()
    finally:
        eng.set_option("lin_split_rows", 0)
    assert snapshot(lin) == before                                        # nothing was updated
    lin.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_unlisted_rows_are_never_read_into_a_result(eng, sets, shape):
    n, dim, C = shape
    X, y, gal = sets[shape]
    L = np.ascontiguousarray(np.random.RandomState(8).permutation(n)[:129], dtype=np.int32)
    Xn = np.full_like(X, np.nan)
    Xn[L] = X[L]
    nan_gal = eng.gallery(Xn)
    for loss in LOSSES:
        for batch in (0, 50):
            a, b = new_lin(eng, dim, C, loss), new_lin(eng, dim, C, loss)
            ta, ra = a.fit(gal, y, iters=4, batch=batch, rows=L, **HP)
            tb, rb = b.fit(nan_gal, y, iters=4, batch=batch, rows=L, **HP)
            assert snapshot(a) == snapshot(b) and ta.tobytes() == tb.tobytes() and same_report(ra, rb)
            assert rb["nonfinite_rows"] == 0 and np.isfinite(b.get()[0]).all()
            ga, gb = a.grad(gal, y, rows=L), b.grad(nan_gal, y, rows=L)
            assert all(u.tobytes() == v.tobytes() for u, v in zip(ga, gb)) and np.isfinite(gb[0]).all()
            assert a.scores(gal, rows=L).get().tobytes() == b.scores(nan_gal, rows=L).get().tobytes()
            a.close()
            b.close()
    nan_gal.close()


# ---------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("shape", SHAPES)
def test_scores_of_a_list(eng, sets, shape):
    n, dim, C = shape
    X, y, gal = sets[shape]
    lin = new_lin(eng, dim, C, LOSSES[0], seed=4)
    whole = lin.scores(gal).get()
    for L in lists_of(n, np.random.RandomState(9)):
        buf = lin.scores(gal, rows=L)
        assert buf.shape == (len(L), C)
        assert buf.get().tobytes() == whole[L].tobytes()
        dev = eng.classification_stats(buf, y[L], C)                      # the scores are read on the device
        host = eng.classification_stats(np.ascontiguousarray(whole[L]), y[L], C)
        assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(dev[:3], host[:3])) and same_report(dev[3], host[3])
        buf.free()
    lin.close()


# ---------------------------------------------------------------------------------------------- the object's state
def test_the_cursor_is_independent(eng, sets):
    """a and b are put to the same parameters and moved to cursor 200 by two steps that change nothing (lr 0, momentum 0).  a then runs
    a fit_rows (again lr 0): its cursor must still be b's, so the following fits take the same batches.  c, at cursor 0, shows that the
    comparison sees the cursor."""
    shape = SHAPES[0]
    n, dim, C = shape
    X, y, gal = sets[shape]
    still = dict(lr=0.0, momentum=0.0, weight_decay=0.0)
    a, b, c = (new_lin(eng, dim, C, LOSSES[2], seed=12) for _ in range(3))
    start = snapshot(c)
    for lin in (a, b):
        lin.fit(gal, y, iters=2, batch=100, **still)
    a.fit(gal, y, iters=3, batch=70, rows=np.arange(n - 1, -1, -1, dtype=np.int32), **still)
    assert snapshot(a)[:4] == snapshot(b)[:4] == start[:4] and (a.get()[4], b.get()[4]) == (5, 2)
    ta, tb, tc = (lin.fit(gal, y, iters=3, batch=100, **HP)[0] for lin in (a, b, c))
    assert ta.tobytes() == tb.tobytes() and snapshot(a)[:4] == snapshot(b)[:4]
    assert ta.tobytes() != tc.tobytes()
    for lin in (a, b, c):
        lin.close()


@pytest.mark.parametrize("loss", LOSSES)
def test_two_fit_rows_give_the_same_bits(eng, sets, loss):
    shape = SHAPES[1]
    n, dim, C = shape
    X, y, gal = sets[shape]
    L = np.random.RandomState(10).randint(0, n, 400).astype(np.int32)
    a, b = new_lin(eng, dim, C, loss), new_lin(eng, dim, C, loss)
    ta, ra = a.fit(gal, y, iters=6, batch=150, rows=L, **HP)
    tb, rb = b.fit(gal, y, iters=6, batch=150, rows=L, **HP)
    assert snapshot(a) == snapshot(b) and ta.tobytes() == tb.tobytes() and same_report(ra, rb)
    a.close()
    b.close()


def test_shuffle_seed_is_the_shuffled_list(eng, sets):
    shape = SHAPES[0]
    n, dim, C = shape
    X, y, gal = sets[shape]
    a, b = new_lin(eng, dim, C, LOSSES[0]), new_lin(eng, dim, C, LOSSES[0])
    ta, _ = a.fit(gal, y, iters=7, batch=128, shuffle_seed=7, epochs=2, **HP)
    tb, _ = b.fit(gal, y, iters=7, batch=128, rows=vv.rows_shuffled(7, n, 2), **HP)
    assert snapshot(a) == snapshot(b) and ta.tobytes() == tb.tobytes()
    with pytest.raises(ValueError):
        a.fit(gal, y, iters=1, rows=np.arange(4), shuffle_seed=1, epochs=1)
    a.close()
    b.close()


def test_a_fit_rows_between_backward_and_update_changes_nothing(sets):
    shape = SHAPES[0]
    n, dim, C = shape
    X, y, _ = sets[shape]
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
            lin = e.linear(dim, C)
            g = e.gallery(X)
            lin.fit(g, y, iters=3, batch=100, rows=vv.rows_shuffled(3, n, 1), loss="hinge", norm="L1", **HP)
            lin.scores(g, rows=np.arange(10)).free()
            lin.close()
        e.apply_update(cfg)
        outs.append(e.params_get())
        e.close()
    assert all(np.array_equal(u, v) for u, v in zip(outs[0], outs[1]))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_everything_as_it_was(eng, sets):
    shape = SHAPES[0]
    n, dim, C = shape
    X, y, gal = sets[shape]
    lin = new_lin(eng, dim, C, LOSSES[1], seed=14)
    lin.fit(gal, y, iters=2, batch=100, **HP)                             # histories, a counter of 2 and a cursor of 200 to lose
    twin = new_lin(eng, dim, C, LOSSES[1], seed=14)
    twin.fit(gal, y, iters=2, batch=100, **HP)
    before = snapshot(lin)
    good = np.arange(50, dtype=np.int32)
    bad_label = y.copy()
    bad_label[17] = C
    neg_label = y.copy()
    neg_label[3] = -1
    cases = [("index -1", np.array([4, -1, 5], np.int32), y, "rows[1]"),
             ("index n_ref", np.array([0, 1, 2, n], np.int32), y, "rows[3]"),
             ("no rows", np.zeros(0, np.int32), y, "n_rows"),
             ("a listed bad label", good, bad_label, "label"),
             ("a listed negative label", good, neg_label, "label")]
    for what, rows, labels, word in cases:
        for call in (lambda: lin.fit(gal, labels, iters=2, rows=rows, **HP), lambda: lin.grad(gal, labels, rows=rows)):
            with pytest.raises(vv.VVError) as e:
                call()
            assert e.value.code == VV_ERR_ARG and word in str(e.value), what
        assert snapshot(lin) == before, what
    for what, rows in (("index -1", cases[0][1]), ("index n_ref", cases[1][1]), ("no rows", cases[2][1])):
        with pytest.raises(vv.VVError) as e:
            lin.scores(gal, rows=rows)
        assert e.value.code == VV_ERR_ARG, what
    # a NULL list with a positive count, through the C ABI itself
    L, C_ = eng.L, vv.engine.C
    lab = np.ascontiguousarray(y)
    cfg, rep = vv.engine._LinearCfg(2, 0, 0.1, 0.9, 0.0, 1.0), vv.engine._LinearReport()
    out = vv.engine.DevBuf(eng, (5, C))
    assert L.vv_linear_fit_rows(eng.h, lin.h, gal.h, vv.engine._ptr(lab), None, 5, C_.byref(cfg), None, None, C_.byref(rep)) == VV_ERR_ARG
    assert L.vv_linear_grad_rows(eng.h, lin.h, gal.h, vv.engine._ptr(lab), None, 5, 1.0, None, None, None) == VV_ERR_ARG
    assert L.vv_linear_scores_rows(eng.h, lin.h, gal.h, None, 5, out.ptr) == VV_ERR_ARG
    assert b"rows is NULL" in L.vv_last_error()
    # the checks the contiguous calls make
    with pytest.raises(vv.VVError):
        lin.fit(gal, y, iters=0, rows=good)
    with pytest.raises(vv.VVError):
        lin.fit(gal, y, iters=1, batch=-1, rows=good)
    assert snapshot(lin) == before
    # ... and the cursor: the next contiguous fit takes the batches the twin's takes
    ta, tb = lin.fit(gal, y, iters=3, batch=100, **HP)[0], twin.fit(gal, y, iters=3, batch=100, **HP)[0]
    assert ta.tobytes() == tb.tobytes() and snapshot(lin) == snapshot(twin)
    lin.close()
    twin.close()


def test_a_bad_label_on_an_unlisted_item_is_not_read(eng, sets):
    """The header's decision: labels of items that are not listed are never read, so a bad one there is accepted -- and changes nothing."""
    shape = SHAPES[0]
    n, dim, C = shape
    X, y, gal = sets[shape]
    L = np.arange(0, 200, dtype=np.int32)
    odd = y.copy()
    odd[250], odd[299] = C + 5, -3
    a, b = new_lin(eng, dim, C, LOSSES[0]), new_lin(eng, dim, C, LOSSES[0])
    ta, ra = a.fit(gal, y, iters=3, batch=64, rows=L, **HP)
    tb, rb = b.fit(gal, odd, iters=3, batch=64, rows=L, **HP)
    assert snapshot(a) == snapshot(b) and ta.tobytes() == tb.tobytes() and same_report(ra, rb)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a.grad(gal, y, rows=L), b.grad(gal, odd, rows=L)))
    with pytest.raises(vv.VVError):
        b.fit(gal, odd, iters=1)                                         # the contiguous call reads every label, as before
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- cross-validation
def test_cross_validate_is_the_hand_written_loop(eng, sets):
    shape = SHAPES[0]
    n, dim, C = shape
    X, y, gal = sets[shape]
    decays, folds, seed = (0.5, 1e-3, 0.0), 3, 11
    kw = dict(iters=12, batch=64, lr=0.05, momentum=0.9)
    lin = new_lin(eng, dim, C, ("hinge", "L2"))
    got = lin.cross_validate(gal, y, folds, decays, seed=seed, **kw)
    last = snapshot(lin)
    hand = new_lin(eng, dim, C, ("hinge", "L2"))
    want = []
    for wd in decays:
        ap, acc = [], []
        for f in range(folds):
            train, held = vv.rows_fold(seed, n, folds, f)
            hand.put(W=np.zeros((C, dim), np.float32), b=np.zeros(C, np.float32), hW=np.zeros((C, dim), np.float32), hb=np.zeros(C, np.float32), steps=0)
            hand.fit(gal, y, rows=train, weight_decay=wd, **kw)
            buf = hand.scores(gal, rows=held)
            rep = eng.classification_stats(buf, y[held], C)[3]
            buf.free()
            ap.append(rep["mean_ap"])
            acc.append(rep["total_accuracy"])
        want.append((wd, np.array(ap, np.float32), np.array(acc, np.float32)))
    assert [r["weight_decay"] for r in got["results"]] == list(decays)
    for r, (wd, ap, acc) in zip(got["results"], want):
        assert r["mean_ap"].tobytes() == ap.tobytes() and r["total_accuracy"].tobytes() == acc.tobytes()
        assert r["mean_ap_mean"].tobytes() == cv_mean(ap).tobytes() and r["total_accuracy_mean"].tobytes() == cv_mean(acc).tobytes()
    assert got["best"] == cv_best([dict(weight_decay=wd, mean_ap_mean=cv_mean(ap)) for wd, ap, _ in want])
    assert snapshot(hand) == last                                         # the classifier is left holding the last fit
    lin.close()
    hand.close()


def test_cross_validate_on_separable_blobs_and_the_tie_rule(eng):
    _, y = ref.blobs(n=320, C=4, dim=8, seed=7)
    X = (6 * np.eye(8)[y] + 0.1 * np.random.RandomState(7).randn(320, 8)).astype(np.float32)      # class means 6 e_c, far apart
    gal = eng.gallery(X)
    lin = eng.linear(8, 4)
    lin.set_loss("hinge", "L1")
    got = lin.cross_validate(gal, y, 4, (1e-3, 0.0, 1e-4), seed=2, iters=40, batch=0, lr=0.1, momentum=0.9)
    for r in got["results"]:
        assert (r["total_accuracy"] == 1.0).all() and (r["mean_ap"] == 1.0).all() and r["mean_ap_mean"] == 1.0
    assert got["best"] == 0.0                                             # all tie at 1: the smallest decay
    assert cv_best([dict(weight_decay=0.1, mean_ap_mean=np.float32(0.5)), dict(weight_decay=0.01, mean_ap_mean=np.float32(0.75)),
                    dict(weight_decay=0.3, mean_ap_mean=np.float32(0.75))]) == 0.01
    lin.close()
    gal.close()
