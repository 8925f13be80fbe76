"""Plain numpy restatements of the per-layer operators (videovector_amd/csrc/ops.hip: vv_op_*), the inputs they are tested on and the
report of a mismatch.  No GPU is needed here: tests/test_ops_ref_host.py checks this file against the oracle and against its own claims,
tests/test_gpu_ops_edges.py holds the kernels to it.

Values come back as float64, or as fp32 where the kernel's result is ONE correctly rounded fp32 operation per element (then numpy's
fp32 arithmetic is the kernel's and the comparison is np.array_equal).

Two kinds of input:

  exact       integers -8 .. 8 times 2^-3, about a third of them zero.  A product of two such values is a multiple of 2^-6 of
              magnitude <= 1; a sum of <= 1000 such products is an integer count of 2^-6 units <= 64000, far below 2^24: exact in
              fp32 in any summation order and with or without FMA contraction (the library is built with plain -O3: a * b + c may or
              may not be fused).  The float64 result is then THE result.
  arbitrary   standard_normal fp32, for operators that round once per element or whose summation order is restated here
              (wave_order_sum) and holds no products.
"""
import numpy as np

from videovector_amd.synth import mix64

F32 = np.float32
U = 2.0 ** -24                       # fp32 unit roundoff: one correctly rounded operation is within U relative
EB = 256                             # threads of a workgroup of the elementwise kernels (ops.hip: EB)
PASS = 4096 * EB                     # elements one pass of their grid-stride loop covers (ops.hip: egrid caps the grid at 4096)
EPS = F32(1e-10)                     # the 1e-10f of the normalisation kernels


# ------------------------------------------------------------------------------- inputs
def exact_values(rng, shape):
    """Integers -8 .. 8 times 2^-3, about a third of them zero (fp32)."""
    v = rng.integers(-8, 9, size=shape) * (rng.random(shape) >= 1.0 / 3.0)
    return (v / 8.0).astype(F32)


def is_exact_input(x):
    """What exact_values claims: multiples of 2^-3 of magnitude <= 1, in fp32."""
    x = np.asarray(x)
    return bool(x.dtype == F32 and np.array_equal(x * 8, np.rint(x * 8)) and (np.abs(x) <= 1).all())


def is_exact_result(ref, unit_log2):
    """ref (float64) is an integer count of 2^unit_log2 units below 2^24: the same number in fp32, however it was summed."""
    units = np.asarray(ref, np.float64) * 2.0 ** -unit_log2
    return bool(np.array_equal(units, np.rint(units)) and (units.size == 0 or np.abs(units).max() < 2 ** 24))


def arbitrary_values(rng, shape):
    return rng.standard_normal(shape).astype(F32)


MARGIN_WEIGHTS = np.array([0, 0.25, 1, 2.25, 4], F32)          # exact square roots 0, 0.5, 1, 1.5, 2; weight 0 included


def margin_case(count, weighted, seed=0):
    """(s_true, s_bogus, weight or None) of a MAX_MARGIN_LOSS test with margin 1: exact scores; every 5th d = st - sb is exactly 0
    (not a violation, hinge = margin) and every 7th (from 3) is exactly 1 = margin (hinge exactly 0: inactive)."""
    rng = np.random.default_rng(1000 + count + seed)
    st, sb = exact_values(rng, count), exact_values(rng, count)
    i = np.arange(count)
    sb[i % 5 == 0] = st[i % 5 == 0]
    at = i % 7 == 3
    st[at], sb[at] = F32(0.5), F32(-0.5)
    w = MARGIN_WEIGHTS[rng.integers(0, len(MARGIN_WEIGHTS), size=count)] if weighted else None
    return st, sb, w


# ------------------------------------------------------------------------------- elementwise (fp32)
def copy2d(src, src_stride, dst, dst_stride, rows, cols, accumulate):
    """dst[r * dst_stride + c] (+)= src[r * src_stride + c] on flat fp32 arrays; returns the new dst (one fp32 add per element)."""
    out = np.array(dst, F32).reshape(-1)
    src = np.asarray(src, F32).reshape(-1)
    if rows * cols == 0:
        return out
    r, c = np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]
    v = src[r * src_stride + c]
    out[r * dst_stride + c] = out[r * dst_stride + c] + v if accumulate else v
    return out


def axpby(a, x, b, y):
    """y = a x (b == 0: y is not read) or a x + b y.  With b != 0 this rounds each product and the sum; the kernel may fuse one
    product into the add: equal on exact inputs only."""
    a, b, x, y = F32(a), F32(b), np.asarray(x, F32), np.asarray(y, F32)
    return a * x if b == 0 else a * x + b * y


def mul(a, b, y=None, accumulate=0):
    """y = a b, or y + a b (exact inputs only, as for axpby)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.asarray(y, F32) + a * b if accumulate else a * b


def relu(x, slope):
    x = np.asarray(x, F32)
    return np.where(x > 0, x, x * F32(slope))


def relu_bwd(x, dy, slope):
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    return dy * np.where(x > 0, F32(1), F32(slope))


def dropout_mask(seed, n, ratio):
    """Element i is kept when (mix64(seed, i) >> 40) 2^-24 >= ratio: 24 random bits, exact in fp32."""
    h = mix64(seed, np.arange(n, dtype=np.uint64))
    assert h.dtype == np.uint64 and h.shape == (n,)                # mix64 is vectorised over a uint64 array
    u = (h >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)
    return u >= F32(ratio)


def dropout_scale(ratio):
    return F32(1) / (F32(1) - F32(ratio))


def dropout(x, mask, ratio):
    x = np.asarray(x, F32)
    return np.where(mask, x * dropout_scale(ratio), F32(0))


# ------------------------------------------------------------------------------- row operators (float64)
def rowsum(x, num_output):
    """y[r][o] = sum_c x[r][c] for every o < num_output"""
    s = np.asarray(x, np.float64).sum(1, keepdims=True)
    return np.repeat(s, num_output, 1)


def rowsum_bwd(dy, cols):
    """dx[r][c] = sum_o dy[r][o]"""
    return rowsum(dy, cols)


def normalize(x):
    """y = x / (sqrt(sum x^2) + 1e-10)"""
    x = np.asarray(x, np.float64)
    return x / (np.sqrt((x * x).sum(1, keepdims=True)) + float(EPS))


def normalize_f32(x):
    """The kernel's four inexact steps in fp32, for rows whose s = sum x^2 is exact in fp32 (asserted): sqrtf, + 1e-10f, the reciprocal
    and one multiply, each correctly rounded."""
    x = np.asarray(x, F32)
    s64 = (x.astype(np.float64) ** 2).sum(1, keepdims=True)
    s = s64.astype(F32)
    assert np.array_equal(s.astype(np.float64), s64), "sum x^2 is not exact in fp32: the inputs are wrong"
    inv = F32(1) / (np.sqrt(s) + EPS)
    assert inv.dtype == F32
    return x * inv


def normalize_bwd(x, dy):
    """(dx, bound): dx = (s dy - x d) / (s^1.5 + 1e-10) with s = sum x^2, d = x . dy, in float64, and the per-element bound of the fp32
    kernel on inputs with exact s and d:  4 U (|s dy| + |x d|) inv  covers either contraction of the numerator,  6 U |dx|  covers
    s * sqrtf(s), the add, the divide and the final multiply."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    s = (x * x).sum(1, keepdims=True)
    d = (x * dy).sum(1, keepdims=True)
    inv = 1.0 / (s ** 1.5 + float(EPS))
    dx = (s * dy - x * d) * inv
    bound = 4 * U * (np.abs(s * dy) + np.abs(x * d)) * inv + 6 * U * np.abs(dx)
    return dx, bound


def hinge(st, sb, w, margin, norm):
    """(d, h): d = st - sb and the weighted hinge term the forward pass sums (L2: max(0, margin - d) sqrt(w), L1: ... w), float64."""
    d = np.asarray(st, np.float64) - np.asarray(sb, np.float64)
    h = np.maximum(0.0, float(margin) - d)
    if w is not None:
        h = h * (np.sqrt(np.asarray(w, np.float64)) if norm == 2 else np.asarray(w, np.float64))
    return d, h


def max_margin(st, sb, w, margin, norm):
    """(loss, violations): mean of h^2 (L2) or |h| (L1) and the number of d < 0 (d = 0 is no violation)."""
    d, h = hinge(st, sb, w, margin, norm)
    total = (h * h).sum() if norm == 2 else np.abs(h).sum()
    return total / len(d), int((d < 0).sum())


def max_margin_bwd(st, sb, w, margin, norm, loss_weight):
    """(g, active): g = d loss / d s_bogus = -d loss / d s_true, float64.  L2: max(0, margin - d) w 2 lw / count; L1: w lw / count where
    the weighted hinge is positive, exactly 0 elsewhere (weight 0 and margin - d = 0 included)."""
    d = np.asarray(st, np.float64) - np.asarray(sb, np.float64)
    wt = np.ones_like(d) if w is None else np.asarray(w, np.float64)
    h = np.maximum(0.0, float(margin) - d) * wt
    active = h > 0
    if norm == 2:
        g = h * (2.0 * float(loss_weight) / len(d))
    else:
        g = np.where(active, wt * (float(loss_weight) / len(d)), 0.0)
    return g, active


# ------------------------------------------------------------------------------- the row kernels' own summation order (fp32)
def wave_order_sum(x):
    """Row sums of x [rows][n] in the order of k_rowsum / k_rowsum_bwd: lane l of the row's wave adds x[l], x[l + 64], ... one after the
    other in fp32, then six butterfly steps p = p + p[lane ^ o] for o = 32, 16, 8, 4, 2, 1.  Both operands of a step's addition are
    swapped between partner lanes and fp32 addition is commutative, so every lane ends with the same value: asserted."""
    x = np.asarray(x, F32)
    assert x.ndim == 2
    rows, n = x.shape
    trips = -(-n // 64) if n else 0
    pad = np.zeros((rows, trips * 64), F32)
    pad[:, :n] = x
    live = np.arange(trips * 64).reshape(trips, 64) < n
    p = np.zeros((rows, 64), F32)
    for k in range(trips):
        p = np.where(live[k], p + pad[:, k * 64:(k + 1) * 64], p)          # lanes past the end skip the trip
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ o]
    assert p.dtype == F32
    assert (p.view(np.uint32) == p.view(np.uint32)[:, :1]).all() or np.isnan(p).any(), "the lanes of a wave disagree"
    return p[:, 0].copy()


# ------------------------------------------------------------------------------- the report of a mismatch
def describe_mismatch(bad, got, ref, what, cols=None):
    """None when no element of `bad` is set; else a message naming the first bad element: flat index and pass of the grid-stride loop
    (index // 1 048 576), or with cols (row, column), the row's workgroup (row // 4) and the lane (column % 64), and both values."""
    bad = np.asarray(bad).reshape(-1)
    if not bad.any():
        return None
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    idx = np.flatnonzero(bad)
    i = int(idx[0])
    if cols:
        r, c = divmod(i, cols)
        where = "(row %d, column %d): workgroup %d, wave %d, lane %d, trip %d" % (r, c, r // 4, r % 4, c % 64, c // 64)
    else:
        where = "index %d: pass %d, workgroup %d, thread %d" % (i, i // PASS, (i % PASS) // EB, i % EB)
    last = int(idx[-1])
    return "%s: %d of %d elements differ; first at %s: got %r, expected %r; last at index %d" % (
        what, len(idx), bad.size, where, got[i].item(), ref[i].item(), last)
