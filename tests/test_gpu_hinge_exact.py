"""vv_op_hinge_loss (k_hinge) on the caller's logits against tests/hinge_ref.py.

dz is compared with == (numerically: -0 equals 0) to the float32 restatement at EVERY element, the pad columns (zero) included, and the
floats in front of and behind the buffer must be left alone; `correct` with ==.  The loss: every term (m, or m m formed in double) is
exact in double, so the device's value differs from loss_weight / rows times the exact sum of those terms by the error of a double sum
of rows cols terms (at most rows cols 2^-53 relative, every term being non-negative) and one rounding to fp32 (one ulp allowed).
Every case asserts last_hinge_form: 1 (16-byte accesses) needs both base pointers on 16 bytes and pitch % 4 == 0.

Shapes: cols over every group width (1, 2, 4, 8, 16, 32, 64 lanes), ragged float4 chunks and more than one chunk per lane; pitch = cols,
cols rounded up to 32, and one that is no multiple of 4; a base pointer one float past a 16-byte boundary; rows 1, 2 and one pass of
the grid + 1 for the narrowest (cols = 1) and the widest (cols = 4096) group; labels on column 0 and on the last column."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hinge_ref as hr   # noqa: E402
import videovector_amd as vv   # noqa: E402
from videovector_amd.engine import DevBuf   # noqa: E402

pytestmark = pytest.mark.gpu

COLS = (1, 3, 4, 5, 13, 31, 32, 33, 128, 129, 256, 257, 4096)
TAIL = 4                                                  # guard floats behind the last row


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def make_case(rs, rows, cols):
    """Logits 2 N(0, 1), so margins fall on both sides of the kink; every third row repeats its maximum at a second column; the first
    row's label is column 0 and the last row's the last column."""
    z = (2.0 * rs.standard_normal((rows, cols))).astype(np.float32)
    for i in range(0, rows, 3):
        z[i, rs.randint(cols)] = z[i].max()
    labels = rs.randint(0, cols, rows).astype(np.int32)
    labels[0] = 0
    labels[-1] = cols - 1
    return z, labels


def run(eng, z, labels, norm, w, pitch=None, offset=0, want_dz=True):
    """offset: floats between a 16-byte boundary and the first logit (and the first dz).  Returns (loss, correct, dz [rows][pitch],
    the floats around dz, form, nonfinite)."""
    rows, cols = z.shape
    pitch = cols if pitch is None else pitch
    front = 4 + offset
    host = np.full(front + rows * pitch + TAIL, np.nan, np.float32)
    body = host[front:front + rows * pitch].reshape(rows, pitch)
    body[:, :cols] = z
    zb = DevBuf(eng, host)
    db = DevBuf(eng, np.full(host.shape, np.nan, np.float32)) if want_dz else None
    try:
        loss, correct = eng.op_hinge_loss(zb.ptr.value + 4 * front, rows, cols, pitch, labels, norm, w, None if db is None else db.ptr.value + 4 * front)
        form, nonfinite = int(eng.get_option("last_hinge_form")), int(eng.get_option("last_hinge_nonfinite"))
        out = db.get() if want_dz else None
    finally:
        zb.free()
        if db is not None:
            db.free()
    if out is None:
        return loss, correct, None, None, form, nonfinite
    return loss, correct, out[front:front + rows * pitch].reshape(rows, pitch), np.concatenate([out[:front], out[front + rows * pitch:]]), form, nonfinite


def check(eng, z, labels, norm, w, pitch=None, offset=0):
    rows, cols = z.shape
    pitch = cols if pitch is None else pitch
    loss, correct, dz, around, form, nonfinite = run(eng, z, labels, norm, w, pitch, offset)
    rdz, _, rcorrect, l64 = hr.hinge_loss_f32(z, labels, norm, w)
    assert form == hr.form_of(pitch, offset, offset), (cols, pitch, offset)
    assert np.isnan(around).all(), "a float outside the buffer was written"
    assert np.array_equal(dz[:, :cols], rdz), (rows, cols, pitch, offset, norm)
    assert not dz[:, cols:].any() and not np.isnan(dz[:, cols:]).any()
    assert correct == rcorrect and nonfinite == hr.nonfinite_rows(z)
    if np.isfinite(l64):
        tol = float(np.spacing(np.float32(abs(l64)))) + rows * cols * 2.0 ** -53 * abs(l64)
        err = abs(float(loss) - l64)
        print("HINGE rows %d cols %d pitch %d offset %d norm %d w %g form %d: loss error %.3e of %.3e allowed" % (rows, cols, pitch, offset, norm, w, form, err, tol))
        assert err <= tol
    else:
        assert float(loss) == l64
    return loss, dz


def layouts(cols):
    """(pitch, offset): the three pitches on an aligned base, and the 32-column pitch one float past a 16-byte boundary."""
    p32 = -(-cols // 32) * 32
    odd = cols + 1 if (cols + 1) % 4 else cols + 2
    return ((cols, 0), (p32, 0), (odd, 0), (p32, 1))


@pytest.mark.parametrize("cols", COLS)
def test_against_the_restatement(eng, cols):
    rs = np.random.RandomState(1000 + cols)
    forms = set()
    for rows in (1, 2):
        z, labels = make_case(rs, rows, cols)
        for k, (pitch, offset) in enumerate(layouts(cols)):
            for norm in (hr.L1, hr.L2):
                check(eng, z, labels, norm, 1.0 if (k + norm) % 2 else 0.125, pitch, offset)
                forms.add(hr.form_of(pitch, offset, offset))
    assert forms == {1, 2}
    if cols in (COLS[0], COLS[-1]):                       # the narrowest and the widest group: one row behind a whole pass of the grid
        rows = hr.rows_per_pass(cols) + 1
        z, labels = make_case(rs, rows, cols)
        p32 = -(-cols // 32) * 32
        check(eng, z, labels, hr.L1, 0.125, p32, 0)
        check(eng, z, labels, hr.L2, 1.0, p32, 1)


def test_both_label_ends_on_a_single_row(eng):
    z, _ = make_case(np.random.RandomState(2), 1, 257)
    for label in (0, 256):
        for norm in (hr.L1, hr.L2):
            check(eng, z, np.array([label], np.int32), norm, 1.0, 260)


def test_the_kink_and_negative_zero(eng):
    """Logits of exactly +1 on the label's column and -1 elsewhere give 1 + t == 0: m = 0 and dz = 0 under both norms; -0.0 is an
    ordinary zero (m = 1)."""
    z = np.full((3, 9), -1.0, np.float32)
    labels = np.array([0, 8, 4], np.int32)
    z[np.arange(3), labels] = 1.0
    z[2, :2] = -0.0
    for norm in (hr.L1, hr.L2):
        for pitch in (9, 12):
            loss, dz = check(eng, z, labels, norm, 1.0, pitch)
            assert not dz[:2].any() and (dz[2, :2] > 0).all() and not dz[2, 2:].any()
            assert float(loss) == np.float32(2.0 / 3.0)


def test_nonfinite_logits(eng):
    """NaN gives m = 0 and is passed over by the first maximum; -Inf off the label and +Inf on it give m = 0; +Inf off the label makes
    the loss +Inf.  Every such row counts in `nonfinite`."""
    z = np.zeros((5, 40), np.float32)
    z[0, [3, 39]] = np.nan
    z[0, 9] = 1.5
    z[1, 7] = np.inf                                      # its label
    z[1, 8] = -np.inf
    z[2, :] = np.nan
    z[3, 5] = 0.5
    labels = np.array([9, 7, 0, 5, 1], np.int32)
    for norm in (hr.L1, hr.L2):
        for pitch, offset in ((40, 0), (64, 1), (41, 0)):
            loss, dz = check(eng, z[:4], labels[:4], norm, 1.0, pitch, offset)
            assert np.isfinite(loss) and not dz[2, :40].any() and not dz[0, [3, 39]].any() and not dz[1, 7:9].any()
            _, correct, _, _, _, nonfinite = run(eng, z[:4], labels[:4], norm, 1.0, pitch, offset)
            assert correct == 4 and nonfinite == 3        # row 2 has no maximum: column 0, its label
    z[4, 20] = np.inf
    for norm in (hr.L1, hr.L2):
        loss, dz = check(eng, z, labels, norm, 1.0, 64)
        assert float(loss) == np.inf and np.isfinite(dz[:4]).all() and dz[4, 20] == (np.float32(0.2) if norm == hr.L1 else np.inf)


def test_two_calls_give_the_same_bits_and_dz_may_be_null(eng):
    z, labels = make_case(np.random.RandomState(8), 3000, 100)
    for norm in (hr.L1, hr.L2):
        for pitch in (128, 101):
            a, b = run(eng, z, labels, norm, 0.125, pitch), run(eng, z, labels, norm, 0.125, pitch)
            assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
            c = run(eng, z, labels, norm, 0.125, pitch, want_dz=False)
            assert c[0].tobytes() == a[0].tobytes() and c[1] == a[1] and c[4] == a[4]


@pytest.mark.parametrize("kw", [dict(rows=0), dict(cols=0), dict(cols=4097), dict(pitch=3), dict(label=4), dict(label=-1), dict(norm=0),
                                dict(norm=3)])
def test_refuses_bad_arguments(eng, kw):
    a = dict(rows=2, cols=4, pitch=4, label=0, norm=hr.L1)
    a.update(kw)
    buf = DevBuf(eng, (2 * 4200,))
    labels = np.full(max(a["rows"], 1), a["label"], np.int32)
    with pytest.raises(vv.VVError):
        eng._chk(eng.L.vv_op_hinge_loss(eng.h, buf.ptr, a["rows"], a["cols"], a["pitch"], labels.ctypes.data, a["norm"], 1.0, None, None, None))
    for null in ("z", "labels"):
        with pytest.raises(vv.VVError):
            eng._chk(eng.L.vv_op_hinge_loss(eng.h, None if null == "z" else buf.ptr, 2, 4, 4, None if null == "labels" else labels.ctypes.data,
                                            hr.L1, 1.0, None, None, None))
    buf.free()
