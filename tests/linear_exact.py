"""Inputs on which a whole step of the linear classifier under the hinge loss is EXACT in fp32, the cases tests/test_gpu_linear_step_exact.py
runs on them, and the check that they are exact (asserted without a GPU by tests/test_linear_exact_host.py for exactly these cases).

The family: every operand is a dyadic number of few bits -- X = integers -3 .. 3 over 2, W = integers -4 .. 4 over 16, b over 8, the histories
over 64 and 32, lr = 2^-3, momentum = 2^-1, weight_decay = 2^-4 (0 from dim 100 up), and loss_weight = count / 64 so that the L1 scale
loss_weight / (float)count is exactly 2^-6 (L2: 2^-5).  Then the logit is a sum of dyadic products, the margin 1 +- z, dz = +-scale (L2: +-m
scale), dW and db sums of dyadic terms, and the rule h = lr (g + wd w) + momentum h, w -= h only shifts and adds them.

A sum is exact IN ANY ORDER when the sum of its terms' absolute values, divided by the terms' common granularity (the largest power of two
that divides them all), is below 2^24: every partial sum of every grouping -- MFMA chains, K tiles, splits, slabs, row blocks, BLAS -- is
then an integer below 2^24 times that granularity.  Under that condition the float64 run of tests/hinge_ref.py IS the fp32 result, and the GPU
test compares with np.array_equal.  The loss is a double sum on both sides: the same condition with 2^53, then one division and one rounding
to fp32 that both sides perform alike.

Under the L2 norm dz carries the margin's bits, so every step multiplies the state's width: the L2 cases run as many steps as the check
allows -- two -- from a put state with every array nonzero, on coarser rows (integers -1 .. 1 over 2), which is what buys the second step."""
import collections
import functools
import zlib

import numpy as np

import hinge_ref as hr
import linear_ref as ref

F32 = np.float32
LR, MOMENTUM = 2.0 ** -3, 2.0 ** -1
F32_BITS, F64_BITS = 24, 53
UPD_GRID_FLOATS = 1024 * 256 * 4          # floats one pass of k_lin_update's fixed grid covers (LIN_UPD_BLOCKS x 256 float4)
SCORES_GRID = 4096 * 256                  # elements one pass of k_lin_scores_out's grid covers at most


def weight_decay(dim):
    return 2.0 ** -4 if dim < 100 else 0.0


# name; gallery rows, dim, classes; batch (0: all rows); norm; steps; bias; lin_split_rows; loss_weight of ONE fit call of `steps` steps (None:
# one fit call per step with loss_weight = count / 64); (last_lin_splits, last_lin_blocks) of the last batch, worked out by hand from
# lin_plan / batch_plan; x_max: rows are integers -x_max .. x_max over 2; first: vv_linear_grad's first row (gradient cases only).
Case = collections.namedtuple("Case", "name n dim C batch norm steps bias split_rows loss_weight plan x_max first seed")


def _case(name, n, dim, C, batch, plan, norm=hr.L1, steps=3, bias=True, split_rows=0, loss_weight=None, x_max=3, first=0, seed=0):
    return Case(name, n, dim, C, batch, norm, steps, bias, split_rows, loss_weight, plan, x_max, first, seed)


def _seeded(kind, cases):
    """Every case's seed comes from its name, so adding a case moves no other case's inputs."""
    return tuple(c._replace(seed=zlib.crc32(("%s %s" % (kind, c.name)).encode())) for c in cases)


def _fit_cases():
    out = []
    # one axis at a time around dim 32, C 32, 128 rows per batch (everything a whole tile, nothing padded); n = 3 batches + 7 rows, so the
    # three steps read rows 0 .., batch .., 2 batch .. and the gallery is longer than what they read
    for dim in (1, 31, 32, 33, 130):                       # Dp 32 / 32 / 32 / 64 / 160
        out.append(_case("dim%d" % dim, 391, dim, 32, 128, (1, 1)))
    for C in (1, 3, 5, 13, 33, 128, 129, 257):             # Cp 32 .. 288; k_hinge lanes 1 / 1 / 2 / 4 / 16 / 32 / 64 / 64 (two chunks a lane)
        out.append(_case("C%d" % C, 391, 32, C, 128, (1, 1)))
    for rows, S in ((1, 1), (127, 1), (129, 2), (257, 3)):  # 128-row splits under the library's plan
        out.append(_case("rows%d" % rows, 3 * rows + 7, 32, 32, rows, (S, 1)))
    out.append(_case("corner", 394, 33, 33, 129, (2, 1)))
    # one fit call of three steps: one loss_weight, so every count must give a dyadic scale
    out.append(_case("whole515", 515, 130, 33, 0, (5, 1), loss_weight=515 / 64))          # two column tiles; 5 splits of 128 (the last 3 rows)
    out.append(_case("one_call_256_128_256", 384, 32, 32, 256, (2, 1), loss_weight=4.0))   # 2, 1, 2 splits: slab 1 of step 1 is stale in step 2
    out.append(_case("one_call_96_96_48", 240, 40, 3, 96, (1, 1), loss_weight=1.5))
    # ragged last batches, one call per step
    out.append(_case("ragged_700", 700, 64, 129, 256, (2, 1)))                             # 256, 256, 188; two row tiles of the weight gradient
    out.append(_case("ragged_129", 129, 33, 32, 128, (1, 1)))                              # 128, 1, 128
    out.append(_case("one_row_one_class", 257, 1, 1, 0, (3, 1), loss_weight=257 / 64))
    # lin_split_rows 2: row blocks of 256 rows = 128 slabs; 300 rows = 256 + 44, the second block writes 22 slabs.  1: 128 + 128 + 44 rows
    out.append(_case("two_row_blocks", 300, 33, 33, 0, (128, 2), split_rows=2, loss_weight=300 / 64))
    out.append(_case("three_row_blocks", 300, 33, 33, 0, (128, 3), split_rows=1, loss_weight=300 / 64))
    # the same without a bias
    for rows, S in ((1, 1), (127, 1), (128, 1), (129, 2), (257, 3)):
        out.append(_case("nobias_rows%d" % rows, 3 * rows + 7, 32, 32, rows, (S, 1), bias=False))
    out.append(_case("nobias_two_row_blocks", 300, 33, 33, 0, (128, 2), bias=False, split_rows=2, loss_weight=300 / 64))
    out.append(_case("nobias_three_row_blocks", 300, 33, 33, 0, (128, 3), bias=False, split_rows=1, loss_weight=300 / 64))
    # Cp Dp / 4 = 270336 float4 > 262144 = one pass of k_lin_update's grid; 72 tiles of the weight gradient
    out.append(_case("update_grid_plus", 64, 1000, 1025, 0, (1, 1), steps=1, loss_weight=1.0))
    # L2: the steps tests/test_linear_exact_host.py proves
    out.append(_case("L2_middle", 263, 32, 32, 128, (1, 1), norm=hr.L2, steps=2, x_max=1))
    out.append(_case("L2_corner", 265, 33, 33, 129, (2, 1), norm=hr.L2, steps=2, x_max=1))
    out.append(_case("L2_C257", 263, 32, 257, 128, (1, 1), norm=hr.L2, steps=2, x_max=1))
    out.append(_case("L2_dim130", 265, 130, 33, 129, (2, 1), norm=hr.L2, steps=2, x_max=1))
    # fewer rows than under L1, which is what keeps the second step inside fp32: lin_split_rows 1, 150 rows = 128 + 22, the second block
    # writes 22 slabs of the 128; 260 rows = 128 + 128 + 4
    out.append(_case("L2_two_row_blocks", 150, 33, 33, 0, (128, 2), norm=hr.L2, steps=2, split_rows=1, loss_weight=150 / 64, x_max=1))
    out.append(_case("L2_three_row_blocks", 260, 33, 33, 0, (128, 3), norm=hr.L2, steps=2, split_rows=1, loss_weight=260 / 64, x_max=1))
    out.append(_case("L2_nobias_three_row_blocks", 300, 33, 33, 0, (128, 3), norm=hr.L2, steps=2, bias=False, split_rows=1, loss_weight=300 / 64,
                     x_max=1))
    return _seeded("fit", out)


def _grad_cases():
    """vv_linear_grad over rows [first, first + batch) of n = first + batch + 5, first = 37: one gradient at a put state, both norms."""
    out = []
    for norm, tag in ((hr.L1, "L1"), (hr.L2, "L2")):
        def g(name, dim, C, rows, plan, **kw):
            out.append(_case("%s_%s" % (tag, name), 37 + rows + 5, dim, C, rows, plan, norm=norm, steps=1, first=37, **kw))
        for dim in (1, 31, 32, 33, 130):
            g("dim%d" % dim, dim, 32, 128, (1, 1))
        for C in (1, 3, 5, 13, 33, 128, 129, 257):
            g("C%d" % C, 32, C, 128, (1, 1))
        for rows, S in ((1, 1), (127, 1), (129, 2), (257, 3)):
            g("rows%d" % rows, 32, 32, rows, (S, 1))
        g("corner", 33, 33, 129, (2, 1))
        g("two_tiles_each_way", 130, 129, 257, (3, 1))
        g("two_row_blocks", 33, 33, 300, (128, 2), split_rows=2)
        g("three_row_blocks", 33, 33, 300, (128, 3), split_rows=1)
        g("nobias_corner", 33, 33, 129, (2, 1), bias=False)
        g("nobias_two_row_blocks", 33, 33, 300, (128, 2), bias=False, split_rows=2)
        g("update_grid_plus", 1000, 1025, 64, (1, 1))
    return _seeded("grad", out)


def _score_cases():
    """vv_linear_scores of n rows (never a multiple of 256) at a put state; only n, dim, C, bias and the seed are read."""
    out = []
    for bias in (True, False):
        tag = "" if bias else "nobias_"
        for dim in (1, 31, 32, 33, 130):
            out.append(_case("%sdim%d" % (tag, dim), 300, dim, 33, 0, None, bias=bias))
        for C in (1, 3, 32, 129, 257):
            out.append(_case("%sC%d" % (tag, C), 300, 33, C, 0, None, bias=bias))
        out.append(_case("%sgrid_plus" % tag, 1100, 32, 1025, 0, None, bias=bias))       # 1100 x 1025 > 4096 x 256: k_lin_scores_out's loop strides
    return _seeded("scores", out)


FIT_CASES, GRAD_CASES, SCORE_CASES = _fit_cases(), _grad_cases(), _score_cases()


def ids(cases):
    return [c.name for c in cases]


# ---- the plan, restated from kernels_linear.hip (lin_plan) and linear.hip (batch_plan); the cases' hand-worked plans are checked against it
def padded(case):
    """(Cp, Dp)"""
    return -(-case.C // 32) * 32, -(-case.dim // 32) * 32


def batch_plan(count, Cp, Dp, forced_split_rows=0):
    """(splits of the first row block, row blocks) of a batch of `count` rows."""
    tiles = -(-Cp // 128) * -(-Dp // 128)
    if forced_split_rows > 0:
        split_rows = forced_split_rows
    else:
        want = max(1, 512 // tiles)
        split_rows = max(128, -(-(-(-count // want)) // 32) * 32)
    block_rows = split_rows * 128
    fit = max(1, (1 << 30) // (2 * Cp * 4))
    rows = min(block_rows, fit // split_rows * split_rows)
    if rows < 1:
        rows = min(block_rows, fit)
    rows = min(rows, count)
    return -(-rows // split_rows), -(-count // rows)


def batches(case):
    """[(first, count, loss_weight)] of the case's steps."""
    if case.first:
        return [(case.first, case.batch, case.batch / 64)]
    plan, _ = ref.batches(case.n, case.batch, case.steps)
    return [(f, c, c / 64 if case.loss_weight is None else case.loss_weight) for f, c in plan]


# ---- inputs
@functools.lru_cache(maxsize=None)
def inputs(case):
    """(X fp32 [n][dim], y int32 [n], W, b, hW, hb fp32): never written to."""
    rs = np.random.RandomState(case.seed)
    X = (rs.randint(-case.x_max, case.x_max + 1, (case.n, case.dim)) / 2.0).astype(F32)
    y = rs.randint(0, case.C, case.n).astype(np.int32)
    W = (rs.randint(-4, 5, (case.C, case.dim)) / 16.0).astype(F32)
    b = (rs.randint(-4, 5, case.C) / 8.0).astype(F32)
    hW = (rs.randint(-4, 5, (case.C, case.dim)) / 64.0).astype(F32)
    hb = (rs.randint(-4, 5, case.C) / 32.0).astype(F32)
    if not case.bias:
        b, hb = np.zeros_like(b), np.zeros_like(hb)
    for a in (X, y, W, b, hW, hb):
        a.setflags(write=False)
    return X, y, W, b, hW, hb


def start_state(case, dtype=np.float64):
    _, _, W, b, hW, hb = inputs(case)
    st = ref.State(case.dim, case.C, dtype, case.bias)
    st.W, st.b, st.hW, st.hb = W.astype(dtype), b.astype(dtype), hW.astype(dtype), hb.astype(dtype)
    return st


# ---- the condition
def granularity(a):
    """The largest power of two that divides every element of a (float64, finite); None when all are zero."""
    a = np.asarray(a, np.float64).ravel()
    a = a[a != 0]
    if a.size == 0:
        return None
    m, e = np.frexp(np.abs(a))
    mi = np.ldexp(m, F64_BITS).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return float(np.ldexp(low, e - F64_BITS).min())


def is_f32(a):
    """Every element of the float64 array is finite and a float32 value."""
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore"):
        return bool(np.isfinite(a).all() and np.array_equal(a.astype(F32).astype(np.float64), a))


def width(abs_sum, gran):
    """log2 of (the largest sum of absolute values / the terms' granularity): below 24 (53) the sum is exact in fp32 (double) in any order."""
    top = float(np.max(abs_sum)) if np.size(abs_sum) else 0.0
    return -np.inf if top == 0 or gran is None else float(np.log2(top / gran))


def _gmul(*gs):
    out = 1.0
    for g in gs:
        if g is None:
            return None
        out *= g
    return out


def _gmin(*gs):
    gs = [g for g in gs if g is not None]
    return min(gs) if gs else None


def check_logits(st, Xb):
    """(z float64, failures) of the logits of rows Xb at st's float64 parameters."""
    Xb = np.asarray(Xb, np.float64)
    z = Xb @ st.W.T + (st.b if st.bias else 0.0)
    g = _gmin(_gmul(granularity(Xb), granularity(st.W)), granularity(st.b) if st.bias else None)
    w = width(np.abs(Xb) @ np.abs(st.W).T + (np.abs(st.b) if st.bias else 0.0), g)
    bad = []
    if not w < F32_BITS:
        bad.append("logit sum: 2^%.1f" % w)
    if not is_f32(z):
        bad.append("logits are not fp32 values")
    return z, bad, w


def check_step(st, Xb, yb, norm, loss_weight, wd, update=True):
    """Every intermediate of one step at st (float64, not changed) over rows Xb: (failures, the largest fp32 width met)."""
    Xb = np.asarray(Xb, np.float64)
    count = Xb.shape[0]
    z, bad, top = check_logits(st, Xb)
    sign = np.ones_like(z)
    sign[np.arange(count), yb] = -1.0
    u = 1.0 + sign * z
    if not is_f32(u):
        bad.append("a margin 1 + t is not an fp32 value")
    scale = loss_weight / count if norm == hr.L1 else loss_weight * 2.0 / count
    if not (is_f32(loss_weight) and is_f32(scale) and np.frexp(scale)[0] == 0.5 and float(F32(loss_weight) / F32(count)) == loss_weight / count):
        bad.append("the scale %r is not a power of two" % scale)
    dz, loss, _, _ = hr.hinge_loss(z, yb, norm, loss_weight)
    m = np.maximum(u, 0.0)
    terms = m if norm == hr.L1 else m * m
    if not is_f32(dz):
        bad.append("dz is not fp32")
    wl = width(terms.sum(), granularity(terms))
    if not wl < F64_BITS:
        bad.append("loss sum: 2^%.1f" % wl)
    gdz = granularity(dz)
    sums = (("dW", np.abs(dz).T @ np.abs(Xb), _gmul(gdz, granularity(Xb))),) + ((("db", np.abs(dz).sum(axis=0), gdz),) if st.bias else ())
    for what, a, g in sums:
        w = width(a, g)
        top = max(top, w)
        if not w < F32_BITS:
            bad.append("%s sum: 2^%.1f" % (what, w))
    dW, db = dz.T @ Xb, dz.sum(axis=0)
    if not (is_f32(dW) and is_f32(db)):
        bad.append("dW or db is not fp32")
    if update:
        t2 = dW + wd * st.W
        hW = LR * t2 + MOMENTUM * st.hW
        hb = LR * db + MOMENTUM * st.hb
        for what, a in (("wd W", wd * st.W), ("g + wd W", t2), ("lr (g + wd W)", LR * t2), ("momentum hW", MOMENTUM * st.hW), ("hW", hW),
                        ("W", st.W - hW)) + ((("lr db", LR * db), ("momentum hb", MOMENTUM * st.hb), ("hb", hb), ("b", st.b - hb)) if st.bias else ()):
            if not is_f32(a):
                bad.append("%s is not fp32" % what)
            g = granularity(a)
            if g is not None:
                top = max(top, float(np.log2(np.abs(a).max() / g)))
    return bad, top


Step = collections.namedtuple("Step", "first count loss_weight loss correct dW db W b hW hb")


def run(case, dtype=np.float64, check=False):
    """The case's steps through tests/hinge_ref.py in `dtype`: ([Step], failures, largest width).  dW, db: the gradient the step used."""
    X, y = inputs(case)[:2]
    st = start_state(case, dtype)
    wd = weight_decay(case.dim)
    out, bad, top = [], [], -np.inf
    for k, (first, count, w) in enumerate(batches(case)):
        Xb, yb = X[first:first + count], y[first:first + count]
        if check:
            b_, t_ = check_step(st, Xb, yb, case.norm, w, wd)
            bad += ["step %d: %s" % (k, s) for s in b_]
            top = max(top, t_)
        dW, db, _, _, _ = hr.gradient(st, Xb, yb, case.norm, w)
        loss, correct, _ = hr.step(st, Xb, yb, case.norm, LR, MOMENTUM, wd, w)
        if check and not all(is_f32(a) for a in (st.W, st.b, st.hW, st.hb)):
            bad.append("step %d: the state is not fp32" % k)
        out.append(Step(first, count, w, loss, correct, dW, db, st.W.copy(), st.b.copy(), st.hW.copy(), st.hb.copy()))
    return out, bad, top


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 run, computed once per case and shared; its arrays are not to be written to."""
    return run(case)[0]


def scores_reference(case):
    """(X W^T + b in float64, failures) at the case's put state."""
    z, bad, _ = check_logits(start_state(case), inputs(case)[0])
    return z, bad
