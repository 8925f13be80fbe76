"""The linear classifier's whole step (vv_linear_fit / _grad / _scores under the hinge loss) against the float64 run of tests/hinge_ref.py, BIT
FOR BIT, past its smallest shape.

The inputs are tests/linear_exact.py's: dyadic operands of few bits on which every operation of a step -- the logits' product, the margins,
dz, the weight-gradient product with its splits, slabs, row blocks and column sums, the rule -- is exact in fp32 in any order of summation, so
the float64 run IS the fp32 result and every comparison is np.array_equal (the loss: == the float64 value rounded once to fp32).  No tolerance
appears.  The condition is not measured here: tests/test_linear_exact_host.py asserts it on the CPU for exactly these cases.

What the cases reach (Dp = dim rounded up to 32, Cp = C rounded up to 32; the weight gradient is m = Cp by n = Dp in 128 x 128 tiles):
  dim 1 / 31 / 32 / 33 / 130     padded and unpadded rows, a second K tile of the logits (Dp 64), a second column tile of the weight gradient (160)
  C 1 .. 257                     every group width of k_hinge (1 .. 64 lanes) and two chunks a lane; C 129: a second row tile (m = 160); C 257:
                                 the bias loop of k_lin_update past its 256 threads (Cp 288)
  rows 1 / 127 / 128 / 129 / 257 one split +- 1 and three splits under the library's plan; S = 2 is where a slab sum can first lose a slab
  one_call_*                     one fit call whose batches differ: 256, 128, 256 rows run 2, 1, 2 splits, so a stale slab lies behind step 2's
  ragged_*                       batches of 188 and of 1 row at a cursor > 0
  two / three_row_blocks         lin_split_rows 2 (1): 300 rows = 256 + 44 (128 + 128 + 44), later blocks accumulate into the slabs and write
                                 fewer of them than the update sums, and read their labels at an offset
  nobias_*                       dbs is not passed: b and hb stay zero
  update_grid_plus               Cp Dp / 4 = 270336 float4 > the 262144 one pass of k_lin_update's grid covers, every element compared
Every case asserts last_lin_splits and last_lin_blocks as worked out by hand in linear_exact.py (and held to lin_plan's restatement by the host
test), so a case cannot silently stop reaching the path it names."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hinge_ref as hr   # noqa: E402
import linear_exact as le   # noqa: E402
import videovector_amd as vv   # noqa: E402
from videovector_amd.engine import DevBuf   # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
NORM_NAMES = {hr.L1: "L1", hr.L2: "L2"}


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.set_option("lin_split_rows", 0)
    e.close()


@pytest.fixture(scope="module")
def second():
    """A second engine object, for the fits that must come out with the same bits."""
    e = vv.Engine(0, "f16")
    yield e
    e.set_option("lin_split_rows", 0)
    e.close()


def same(got, want):
    """Equal as values at every element (fp32 against the float64 reference), and nothing NaN."""
    got = np.asarray(got)
    return got.dtype == F32 and got.shape == want.shape and np.array_equal(got.astype(np.float64), want)


def new_lin(e, case):
    _, _, W, b, hW, hb = le.inputs(case)
    lin = e.linear(case.dim, case.C, bias=case.bias)
    lin.put(W, b, hW, hb)
    lin.set_loss("hinge", NORM_NAMES[case.norm])
    return lin


def fit(e, case):
    """The case's steps on engine e: (loss trace, last report, (W, b, hW, hb, steps), [(splits, blocks) behind every call])."""
    X, y = le.inputs(case)[:2]
    gal = e.gallery(X)
    lin = new_lin(e, case)
    hp = dict(batch=case.batch, lr=le.LR, momentum=le.MOMENTUM, weight_decay=le.weight_decay(case.dim))
    trace, plans = [], []
    try:
        e.set_option("lin_split_rows", case.split_rows)
        calls = [(case.steps, case.loss_weight)] if case.loss_weight is not None else [(1, w) for _, _, w in le.batches(case)]
        for iters, w in calls:
            t, rep = lin.fit(gal, y, iters=iters, loss_weight=w, **hp)
            trace.append(t)
            plans.append((e.get_option("last_lin_splits"), e.get_option("last_lin_blocks")))
    finally:
        e.set_option("lin_split_rows", 0)
    state = lin.get()
    lin.close()
    gal.close()
    return np.concatenate(trace), rep, state, plans


@pytest.mark.parametrize("case", le.FIT_CASES, ids=le.ids(le.FIT_CASES))
def test_fit_is_the_float64_run_bit_for_bit(eng, second, case):
    steps = le.reference(case)
    trace, rep, (W, b, hW, hb, n_steps), plans = fit(eng, case)
    last = steps[-1]
    assert plans[-1] == case.plan
    if case.loss_weight is None:                                         # one call per step: every batch's plan
        Cp, Dp = le.padded(case)
        assert plans == [le.batch_plan(s.count, Cp, Dp, case.split_rows) for s in steps]
    assert n_steps == case.steps == rep["steps"] and rep["nonfinite_rows"] == 0
    for name, got in (("W", W), ("b", b), ("hW", hW), ("hb", hb)):
        assert same(got, getattr(last, name)), name
    if not case.bias:
        assert not b.any() and not hb.any()
    want = np.array([F32(s.loss) for s in steps])
    assert trace.dtype == F32 and trace.tobytes() == want.tobytes()
    assert rep["loss_last"] == want[-1] and rep["accuracy_last"] == F32(last.correct) / F32(last.count)
    # a second engine object, fitted the same way
    trace2, rep2, state2, plans2 = fit(second, case)
    assert trace2.tobytes() == trace.tobytes() and plans2 == plans and rep2 == rep and state2[4] == n_steps
    assert all(u.tobytes() == v.tobytes() for u, v in zip((W, b, hW, hb), state2[:4]))


@pytest.mark.parametrize("case", le.GRAD_CASES, ids=le.ids(le.GRAD_CASES))
def test_grad_is_exact_at_an_offset_and_moves_nothing(eng, case):
    (step,) = le.reference(case)
    X, y, W0, b0, hW0, hb0 = le.inputs(case)
    assert step.first == case.first > 0
    gal = eng.gallery(X)
    lin = new_lin(eng, case)
    try:
        eng.set_option("lin_split_rows", case.split_rows)
        dW, db, loss = lin.grad(gal, y, step.first, step.count, step.loss_weight)
        assert (eng.get_option("last_lin_splits"), eng.get_option("last_lin_blocks")) == case.plan
    finally:
        eng.set_option("lin_split_rows", 0)
    assert same(dW, step.dW) and same(db, step.db) and loss == F32(step.loss)
    assert case.bias or not db.any()
    W, b, hW, hb, n_steps = lin.get()
    assert n_steps == 0 and all(u.tobytes() == v.tobytes() for u, v in zip((W, b, hW, hb), (W0, b0, hW0, hb0)))
    lin.close()
    gal.close()


@pytest.mark.parametrize("case", le.SCORE_CASES, ids=le.ids(le.SCORE_CASES))
def test_scores_are_x_wt_plus_b(eng, case):
    """From the gallery and from host rows: n x C floats, C (not Cp) a row, and the float behind the last row untouched."""
    z, _ = le.scores_reference(case)
    X = le.inputs(case)[0]
    assert case.n % 256 != 0
    gal = eng.gallery(X)
    lin = new_lin(eng, case)
    for src in (gal, X):
        buf = DevBuf(eng, np.full(case.n * case.C + 1, np.nan, F32))
        lin.scores(src, out=buf)
        got = buf.get()
        buf.free()
        assert np.isnan(got[-1])
        assert same(got[:-1].reshape(case.n, case.C), z)
    lin.close()
    gal.close()
