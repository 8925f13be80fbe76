"""vv_op_softmax_loss (k_softmax_xent) against tests/linear_ref.py's float64 softmax from the same fp32 logits.

Exact: `correct` (the first maximum: the lowest column wins a tie); dz's pad columns are 0; dz == p * (w / rows) bit for bit at the
columns that are not the label's, w / rows formed once in fp32, when both outputs are requested.

The bound on p, counting roundings, eps = 2^-23 (one ulp relative to the value at most), T = the row's logit spread max - min:
  t = z - max       one fp32 subtraction: |dt| <= 2^-24 |t| <= (T / 2) eps
  e = expf(t)       OpenCL full profile, which OCML's default expf is built to (ROCm ships no tighter statement of its own here):
                    3 ulp; the argument's error is amplified by |t|: exp(t + dt) = exp(t) (1 + dt), so (3 + T / 2) eps in all
  s = sum e         cols non-negative terms, lane-strided ascending then folded by halves: every term passes through at most
                    ceil(cols / wd) + log2(wd) additions of 2^-24 each, and carries its own (3 + T / 2) eps
  p = e / s         2.5 ulp (OpenCL's limit for x / y)
  relative: [2 (3 + T / 2) + (ceil(cols / wd) + log2 wd) / 2 + 2.5] eps, times 1.01 for the second-order terms  (linear_ref.p_bound)
  absolute floor: 2^-126 = FLT_MIN.  The ulp limits are stated for normal results; a p below the normal range may lose its low bits
  or be flushed whole.
The loss: a row's term -logf(max(p, FLT_MIN)) errs by p's relative error (d log p = dp / p) plus logf's 3 ulp of the term; rows
whose label's p lies below FLT_MIN / 2 clamp on both sides and err by logf's 3 ulp of 87.34 alone; the cases keep every label's p
out of (FLT_MIN / 2, 2 FLT_MIN), which the test asserts.  The terms are summed in double; the result is rounded once (eps / 2).

The largest observed share of each bound is printed per case (pytest -s); DESIGN.md, 'Softmax linear classifier', records them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_ref as ref   # noqa: E402
import videovector_amd as vv
from videovector_amd.engine import DevBuf

pytestmark = pytest.mark.gpu

COLS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 300, 4096)
SPREADS = (0.0, 16.0, 100.0, 200.0)
FLOOR = 2.0 ** -126


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def make_case(rs, rows, cols):
    """Row i: spread SPREADS[i % 4] (0: a row of equal logits); its maximum 0 at a random column, tied at a second column in every
    third row; the smallest logit -spread at another; the label on the maximum, on the smallest column, or anywhere, in turn."""
    z = np.zeros((rows, cols), np.float32)
    labels = np.zeros(rows, np.int32)
    for i in range(rows):
        T = SPREADS[i % 4]
        z[i] = -T * rs.rand(cols)
        hi, lo = rs.randint(cols), rs.randint(cols)
        z[i, lo] = -T
        z[i, hi] = 0.0
        if i % 3 == 0:
            z[i, rs.randint(cols)] = z[i].max()
        labels[i] = (int(np.argmax(z[i])), lo, rs.randint(cols))[(i // 4) % 3]
        if -90.0 < z[i, labels[i]] < -77.0:                  # keep the label's p clear of FLT_MIN (log p = t - log sum, sum <= cols)
            z[i, labels[i]] = -70.0
    return z, labels


def run(eng, z, labels, w, pad=3, want_p=True, want_dz=True):
    rows, cols = z.shape
    pitch = cols + pad
    zp = np.full((rows, pitch), np.nan, np.float32)
    zp[:, :cols] = z
    dzb = DevBuf(eng, np.full((rows, pitch), np.nan, np.float32)) if want_dz else None
    pb = DevBuf(eng, np.full((rows, pitch), np.nan, np.float32)) if want_p else None
    zb = DevBuf(eng, zp)
    loss, correct = eng.op_softmax_loss(zb, rows, cols, pitch, labels, w, pb, dzb)
    out = (loss, correct, pb.get() if want_p else None, dzb.get() if want_dz else None)
    for b in (zb, pb, dzb):
        if b is not None:
            b.free()
    return out


def check(eng, z, labels, w, tag):
    rows, cols = z.shape
    loss, correct, p, dz = run(eng, z, labels, w)
    p64, dz64, loss64, correct64 = ref.softmax_loss(z, labels, w)
    assert correct == correct64
    assert np.isnan(p[:, cols:]).all()                                   # the pad of prob is not written
    assert np.array_equal(dz[:, cols:], np.zeros((rows, 3), np.float32))
    p, dz = p[:, :cols], dz[:, :cols]
    scale = np.float32(w) / np.float32(rows)
    other = np.ones((rows, cols), bool)
    other[np.arange(rows), labels] = False
    assert np.array_equal(dz[other], (p * scale)[other])
    T = (z.max(axis=1) - z.min(axis=1)).astype(np.float64)
    rel = np.array([ref.p_bound(cols, t) for t in T])
    share_p = (np.abs(p.astype(np.float64) - p64) / (rel[:, None] * p64 + FLOOR)).max()
    pl = p64[np.arange(rows), labels]
    assert not ((pl > float(ref.FLT_MIN) / 2) & (pl < 2 * float(ref.FLT_MIN))).any()
    terms = -np.log(np.maximum(pl, float(ref.FLT_MIN)))
    row_b = np.where(pl >= 2 * float(ref.FLT_MIN), rel, 0.0) + 3 * ref.EPS * terms
    loss_b = w * row_b.sum() / rows + ref.EPS / 2 * abs(loss64) + 1e-45
    share_l = abs(float(loss) - loss64) / loss_b
    print("SOFTMAX %s rows %d cols %d w %g: p at %.3f of its bound, loss at %.3f of its bound (%.3e)" % (tag, rows, cols, w, share_p, share_l, loss_b))
    assert share_p <= 1.0 and share_l <= 1.0


@pytest.mark.parametrize("cols", COLS)
def test_softmax_against_float64(eng, cols):
    rs = np.random.RandomState(cols)
    for rows in (1, 63, 64, 65, ref.rows_per_pass(cols) + 1):
        z, labels = make_case(rs, rows, cols)
        check(eng, z, labels, 1.0 if rows % 2 else 0.25, "case")


def test_outputs_may_be_null(eng):
    z, labels = make_case(np.random.RandomState(5), 130, 100)
    full = run(eng, z, labels, 0.25)
    only_p = run(eng, z, labels, 0.25, want_dz=False)
    only_dz = run(eng, z, labels, 0.25, want_p=False)
    none = run(eng, z, labels, 0.25, want_p=False, want_dz=False)
    assert full[:2] == only_p[:2] == only_dz[:2] == none[:2]
    assert np.array_equal(full[2], only_p[2], equal_nan=True) and np.array_equal(full[3], only_dz[3], equal_nan=True)


def test_ties_take_the_lowest_column(eng):
    z = np.zeros((4, 70), np.float32)
    z[1, [5, 69]] = 2.0
    z[2, [64, 3]] = 7.0
    z[3, :] = -1.0
    for labels, want in (([0, 5, 3, 0], 4), ([1, 69, 64, 1], 0)):
        assert run(eng, z, np.array(labels, np.int32), 1.0)[1] == want


def test_nonfinite_rows_are_ordinary_rows(eng):
    z = np.zeros((3, 40), np.float32)
    z[0, 7] = np.inf
    z[1, 0] = np.nan
    z[1, 9] = 1.0
    z[2, 3] = 2.0
    loss, correct, p, dz = run(eng, z, np.array([7, 9, 3], np.int32), 1.0)
    assert correct == 3                                      # +Inf is the first maximum of row 0; row 1's NaN is passed over
    assert np.isfinite(p[2, :40]).all() and not np.isfinite(p[1, :40]).all()


@pytest.mark.parametrize("kw", [dict(rows=0), dict(cols=0), dict(cols=4097), dict(pitch=3), dict(label=4), dict(label=-1)])
def test_refuses_bad_arguments(eng, kw):
    a = dict(rows=2, cols=4, pitch=4, label=0)
    a.update(kw)
    buf = DevBuf(eng, (2 * 4200,))
    labels = np.full(max(a["rows"], 1), a["label"], np.int32)
    with pytest.raises(vv.VVError):
        eng._chk(eng.L.vv_op_softmax_loss(eng.h, buf.ptr, a["rows"], a["cols"], a["pitch"], labels.ctypes.data, 1.0, None, None, None, None))
