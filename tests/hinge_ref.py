"""Restatement of the one-vs-rest hinge loss of the linear classifier (include/videovec.h: vv_linear_loss_set, vv_op_hinge_loss; the
reference's hinge_loss_layer.cpp:13-77) in numpy: float64, and a float32 twin in which every operation is rounded where the device
rounds it.  The classifier's state, the batches and the blob inputs are tests/linear_ref.py's.

  t = (c == label) ? -z : z                      (:25)
  m = (0 < 1 + t) ? 1 + t : 0                    (:29-30; a NaN gives 0)
  L1: loss = w sum(m) / rows,    dz = +-[m > 0] s1,  s1 = w / rows             (:36, :61-69)
  L2: loss = w sum(m m) / rows,  dz = +-m s2,        s2 = (w * 2) / rows       (:39, :71)       - on the label's column"""
import math

import numpy as np

import linear_ref as ref

F32 = np.float32
L1, L2 = 1, 2                     # VV_NORM_L1, VV_NORM_L2
SOFTMAX, HINGE = 0, 1             # VV_LIN_LOSS_*
GRID_BLOCKS, WAVES = 512, 4       # k_hinge's fixed grid: LIN_SM_BLOCKS workgroups of four waves
GUARD = 2.0 ** -10                # the fit tests' inputs keep every |1 + t| of the float64 run at least this far from the kink


def lanes_of(cols):
    """Lanes that share one row in k_hinge: the power of two that covers ceil(cols / 4) four-column chunks, 1 .. 64."""
    wd = 1
    while wd < 64 and wd * 4 < cols:
        wd *= 2
    return wd


def rows_per_pass(cols):
    """Rows one pass of k_hinge's fixed grid covers."""
    return GRID_BLOCKS * WAVES * (64 // lanes_of(cols))


def form_of(pitch, z_offset_floats=0, dz_offset_floats=0):
    """last_hinge_form for buffers that start that many floats behind a 16-byte boundary: 1 (16-byte accesses) or 2 (element-wise)."""
    return 1 if pitch % 4 == 0 and z_offset_floats % 4 == 0 and dz_offset_floats % 4 == 0 else 2


def _margins(z, labels):
    """(m, sign) in z's dtype: sign is -1 on the label's column, +1 elsewhere."""
    rows = z.shape[0]
    sign = np.ones(z.shape, z.dtype)
    sign[np.arange(rows), labels] = -1
    with np.errstate(invalid="ignore"):
        u = z.dtype.type(1) + sign * z                   # (the product with +-1 is exact)
        m = np.where(u > 0, u, z.dtype.type(0))          # NaN > 0 is false: 0
    return m, sign


def nonfinite_rows(z):
    return int((~np.isfinite(np.asarray(z))).any(axis=1).sum())


def hinge_loss(z, labels, norm, loss_weight=1.0):
    """float64: (dz, loss, correct, gap) of logits z [rows][cols]; gap = the smallest |1 + t|."""
    z = np.asarray(z, np.float64)
    rows = z.shape[0]
    m, sign = _margins(z, labels)
    with np.errstate(invalid="ignore"):
        gap = float(np.nanmin(np.abs(1.0 + sign * z))) if np.isfinite(z).any() else float("inf")
    if norm == L1:
        dz = sign * (m > 0) * (loss_weight / rows)
        loss = loss_weight * m.sum() / rows
    else:
        dz = sign * m * (loss_weight * 2.0 / rows)
        loss = loss_weight * (m * m).sum() / rows
    return dz, loss, int((ref.first_max(z) == labels).sum()), gap


def hinge_loss_f32(z, labels, norm, loss_weight=1.0):
    """The float32 twin: (dz fp32, loss fp32, correct, loss64).  loss64 is loss_weight / rows times the EXACT sum (math.fsum) of the
    fp32 terms m, or of m m formed in double, before the one rounding to fp32 that gives `loss`."""
    z = np.asarray(z, F32)
    rows = z.shape[0]
    m, sign = _margins(z, labels)
    if norm == L1:
        s1 = F32(loss_weight) / F32(rows)
        dz = np.where(m > 0, sign * s1, F32(0)).astype(F32)
        terms = m.astype(np.float64)
    else:
        s2 = (F32(loss_weight) * F32(2)) / F32(rows)
        dz = ((sign * m) * s2).astype(F32)
        terms = m.astype(np.float64) * m.astype(np.float64)
    total = math.fsum(terms.ravel().tolist())
    loss64 = float(np.float64(F32(loss_weight)) * total / rows)
    return dz, F32(loss64), int((ref.first_max(z) == labels).sum()), loss64


def gradient(st, X, y, norm, loss_weight=1.0):
    """(dW, db, loss, correct, gap) of one batch at st's parameters, in st's dtype (gap: float64 only, else None)."""
    if st.dtype == np.float64:
        X = np.asarray(X, np.float64)
        z = X @ st.W.T + (st.b if st.bias else 0.0)
        dz, loss, correct, gap = hinge_loss(z, y, norm, loss_weight)
    else:
        X = np.asarray(X, F32)
        z = (X @ st.W.T).astype(F32)
        if st.bias:
            z = z + st.b
        dz, loss, correct, _ = hinge_loss_f32(z, y, norm, loss_weight)
        gap = None
    dW = (dz.T @ X).astype(st.dtype)
    db = dz.sum(axis=0).astype(st.dtype) if st.bias else np.zeros_like(st.b)
    return dW, db, loss, correct, gap


def step(st, X, y, norm, lr, momentum, weight_decay, loss_weight=1.0):
    """linear_ref.step with the hinge gradient: h = lr (g + weight_decay W) + momentum h; W -= h; no decay on b."""
    t = st.dtype
    dW, db, loss, correct, gap = gradient(st, X, y, norm, loss_weight)
    lr, momentum, weight_decay = t(lr), t(momentum), t(weight_decay)
    st.hW = lr * (dW + weight_decay * st.W) + momentum * st.hW
    st.W = st.W - st.hW
    if st.bias:
        st.hb = lr * db + momentum * st.hb
        st.b = st.b - st.hb
    st.steps += 1
    return loss, correct, gap


def fit(st, X, y, norm, iters, batch=0, lr=0.1, momentum=0.9, weight_decay=0.0, loss_weight=1.0):
    """(loss trace, accuracy of the last batch, smallest gap of any step); st.cursor is carried."""
    y = np.asarray(y)
    plan, cursor = ref.batches(len(X), batch, iters, st.cursor)
    trace, acc, gap = [], 0.0, float("inf")
    for first, count in plan:
        loss, correct, g = step(st, X[first:first + count], y[first:first + count], norm, lr, momentum, weight_decay, loss_weight)
        trace.append(loss)
        acc = correct / count
        gap = gap if g is None else min(gap, g)
    st.cursor = cursor
    return np.array(trace), acc, gap


# ---- the inputs of tests/test_gpu_linear_hinge_fit.py, stated once so that tests/test_hinge_ref_host.py asserts the guard condition on
# exactly these: in the float64 run every |1 + t| of every step is at least GUARD, so the active set of the fp32 run (whose logits
# differ from float64 by far less) cannot differ.
FIT_BLOB_SEED = 104               # linear_ref.blobs(seed=...) of the five-step fits: both norms, all FIT_BATCHES keep the guard
GRAD_BLOB_SEED = 7                # ... and of the gradient cases (linear_ref.blobs' default)
FIT_HP = dict(lr=0.5, momentum=0.9, weight_decay=1e-4)
FIT_BATCHES = (0, 64, 100)
FIT_STEPS = 5
GRAD_SEED = 3                     # W, b = 0.5 N(0, 1) from RandomState(GRAD_SEED)
GRAD_CASES = ((0, 256, 1.0), (37, 100, 0.25))


def grad_params():
    rs = np.random.RandomState(GRAD_SEED)
    return (0.5 * rs.randn(4, 8)).astype(F32), (0.5 * rs.randn(4)).astype(F32)
