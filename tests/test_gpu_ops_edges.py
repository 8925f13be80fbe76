"""The per-layer operators (videovector_amd/csrc/ops.hip: vv_op_*) past one wave, one workgroup and one pass of the grid.

tests/test_gpu_ops.py checks each operator the way the reference checks its layers, at one small shape.  At those shapes most of a
kernel's loop structure never runs.  Here every operator runs at the sizes where that structure changes:

  elementwise kernels   grid-stride loops over a grid capped at 4096 x 256 threads: n = 1, 255 / 256 / 257 (one workgroup's edge),
                        1 048 576 / 1 048 577 (the end of the first pass, one element into the second), 2 097 152 + 300 (the third)
  row kernels           one wave per row, lanes stride by 64, a six-step butterfly, four rows per workgroup: cols and num_output at
                        63 / 64 / 65, 127 / 128 / 129 (a full wave, a second trip), rows 1, 3, 4, 5 and 1027 (257 workgroups)
  max_margin            one workgroup of 256 threads striding by 256: count 255 / 256 / 257, 1000 and 1 048 579

against tests/ops_ref.py (checked on the CPU by tests/test_ops_ref_host.py), element by element.  Two kinds of input, named in every
test:  EXACT inputs (multiples of 2^-3 in [-1, 1]) make every product and every sum of up to 1000 products exact in fp32 whatever
the order and whatever the compiler fuses, so the float64 result is the expected fp32 result and the comparison is np.array_equal;
ARBITRARY inputs (standard normal) are used where the kernel rounds once per element, or where its summation order is restated
(ops_ref.wave_order_sum) -- also np.array_equal.  The few bounds that are not equality are derived where they are used, in units of
U = 2^-24 (one correctly rounded fp32 operation is within U relative); each prints the largest error it saw before it asserts.

The library is built without fast-math options: hipcc then emits the correctly rounded fp32 square root and division (in the
disassembly of k_normalize: v_sqrt_f32 with its two correction steps, v_div_scale_f32 / v_div_fmas_f32 / v_div_fixup_f32), which is
what lets the NORMALIZATION forward test ask for equality.

Every output buffer carries a tail of 1024 sentinel values (copy2d: the gaps between cols and the stride too) that must come back
intact, and starts out filled with the sentinel, so an element the kernel skips is seen as well as one it writes wrongly.  A mismatch
names the first differing index with its pass, workgroup and thread, or its (row, column) with workgroup, wave, lane and trip.
"""
import ctypes

import numpy as np
import pytest

from tests import ops_ref as R
from tests.test_gpu_ops import assert_grad, eng, numeric_grad  # noqa: F401  (eng: fixture)
from tests.test_gpu_update_exact import half_scale

pytestmark = pytest.mark.gpu

U = R.U
TAIL = 1024
SENTINEL = np.float32(-12345.0)                # no result of these inputs
MASK_SENTINEL = np.uint8(0xA5)                 # no mask byte (0 / 1)
SIZES = [1, 255, 256, 257, R.PASS, R.PASS + 1, 2 * R.PASS + 300]
_CACHE = {}                                    # host inputs and references, made once and never modified


def cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def arbitrary(n, seed):
    """ARBITRARY input of n values, with +0.0, -0.0 and a few exact values at the front, the back and around the pass boundary."""
    def make():
        x = R.arbitrary_values(np.random.default_rng(seed * 7919 + n), n)
        for at, v in ((0, 0.0), (1, -0.0), (R.PASS - 1, -0.0), (R.PASS, 0.0), (n - 1, -0.0), (n - 2, 0.0), (R.EB - 1, -1.0), (R.EB, 1.0)):
            if 0 <= at < n:
                x[at] = v
        return x
    return cached(("arb", n, seed), make)


def exact(n, seed):
    return cached(("exact", n, seed), lambda: R.exact_values(np.random.default_rng(seed * 104729 + n), n))


class Guarded:
    """A device buffer of n values followed by a tail of TAIL sentinels; the body starts as `init` or as sentinels."""

    def __init__(self, eng, n, init=None, dtype=np.float32):  # noqa: F811
        self.n, self.sent = int(n), (MASK_SENTINEL if dtype == np.uint8 else SENTINEL)
        host = np.full(self.n + TAIL, self.sent, dtype)
        if init is not None:
            host[:self.n] = np.asarray(init, dtype).reshape(-1)
        self.buf = eng.dev(host)
        self.ptr = self.buf.ptr

    def read(self, what):
        host = self.buf.get()
        self.buf.free()
        tail = host[self.n:]
        if not (tail == self.sent).all():
            at = int(np.flatnonzero(tail != self.sent)[0])
            pytest.fail("%s: wrote past the end of its output: element n + %d = %r" % (what, at, tail[at].item()))
        return host[:self.n]


def op(eng, name, *args):  # noqa: F811
    eng.op(name, *[a.buf if isinstance(a, Guarded) else a for a in args])


def check(bad, got, ref, what, cols=None):
    msg = R.describe_mismatch(bad, got, ref, what, cols)
    if msg:
        print(msg)
        pytest.fail(msg)


def assert_same(got, ref, what, cols=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        check(~(got == ref), got, ref, what, cols)


def assert_within(got, ref, bound, what, cols=None):
    """|got - ref| <= bound element by element (ref, bound float64); prints the largest error in units of the bound first."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("%s: largest error / bound = %.4f" % (what, share.max() if share.size else 0.0))
    check(~(err <= bound), got, ref, what, cols)


# =============================================================================== elementwise kernels
@pytest.mark.parametrize("n", SIZES)
def test_relu_forward_and_backward_at_every_pass(eng, n):  # noqa: F811
    """ARBITRARY inputs with +-0.0: one rounding per element."""
    x, dy = arbitrary(n, 1), arbitrary(n, 2)
    X, DY = eng.dev(x), eng.dev(dy)
    for slope in (0.0, 0.01):
        Y, DX = Guarded(eng, n), Guarded(eng, n)
        op(eng, "relu", n, X, Y, slope)
        op(eng, "relu_bwd", n, X, DY, DX, slope)
        assert_same(Y.read("relu"), R.relu(x, slope), "relu (n %d, slope %g)" % (n, slope))
        assert_same(DX.read("relu_bwd"), R.relu_bwd(x, dy, slope), "relu_bwd (n %d, slope %g)" % (n, slope))
    X.free(); DY.free()


@pytest.mark.parametrize("n", SIZES)
def test_mul_and_scale_on_arbitrary_inputs(eng, n):  # noqa: F811
    """ARBITRARY inputs: mul without accumulate and axpby with b = 0 round once per element (y is not read: it starts as sentinels)."""
    a, b = arbitrary(n, 3), arbitrary(n, 4)
    A, B = eng.dev(a), eng.dev(b)
    Y, Z = Guarded(eng, n), Guarded(eng, n)
    op(eng, "mul", n, A, B, Y, 0)
    op(eng, "axpby", n, 1.7, A, 0.0, Z)
    assert_same(Y.read("mul"), R.mul(a, b), "mul (n %d)" % n)
    assert_same(Z.read("axpby"), R.axpby(1.7, a, 0.0, a), "axpby b = 0 (n %d)" % n)
    A.free(); B.free()


@pytest.mark.parametrize("n", SIZES)
def test_sum_with_coefficients_and_mul_accumulate_exact(eng, n):  # noqa: F811
    """EXACT inputs: y = a - 0.5 b + 2 c by three axpby calls (multiples of 2^-4 up to 3.5), then y += a b (multiples of 2^-6)."""
    a, b, c3 = exact(n, 5), exact(n, 6), exact(n, 7)
    ref1 = a.astype(np.float64) - 0.5 * b.astype(np.float64) + 2.0 * c3.astype(np.float64)
    ref2 = ref1 + a.astype(np.float64) * b.astype(np.float64)
    assert R.is_exact_input(a) and R.is_exact_input(b) and R.is_exact_input(c3) and R.is_exact_result(ref1, -4) and R.is_exact_result(ref2, -6)
    A, B, C3 = eng.dev(a), eng.dev(b), eng.dev(c3)
    Y = Guarded(eng, n)
    op(eng, "axpby", n, 1.0, A, 0.0, Y)
    op(eng, "axpby", n, -0.5, B, 1.0, Y)
    op(eng, "axpby", n, 2.0, C3, 1.0, Y)
    Y2 = Guarded(eng, n, init=ref1)
    op(eng, "mul", n, A, B, Y2, 1)
    assert_same(Y.read("axpby"), ref1, "axpby chain 1, -0.5, 2 (n %d)" % n)
    assert_same(Y2.read("mul"), ref2, "mul accumulate (n %d)" % n)
    A.free(); B.free(); C3.free()


@pytest.mark.parametrize("ratio", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("n", SIZES)
def test_dropout_mask_is_keyed_on_the_element(eng, n, ratio):  # noqa: F811
    """ARBITRARY inputs.  Mask byte i is the hash of (seed, i) against the ratio, bit for bit; y is x * scale or 0, bit for bit; a
    second input with make_mask = 0 reuses the stored mask."""
    x, x2 = arbitrary(n, 8), arbitrary(n, 9)
    X, X2 = eng.dev(x), eng.dev(x2)
    for seed in (12345, (1 << 40) + 12345):                    # the second: above 2^32, same low bits
        m_ref = cached(("mask", n, ratio, seed), lambda: R.dropout_mask(seed, n, ratio))
        what = "dropout (n %d, ratio %g, seed %d)" % (n, ratio, seed)
        Y, M = Guarded(eng, n), Guarded(eng, n, dtype=np.uint8)
        op(eng, "dropout", n, X, Y, M, ratio, seed, 1)
        Y2 = Guarded(eng, n)
        op(eng, "dropout", n, X2, Y2, M, ratio, seed + 1, 0)   # (the seed is not used without make_mask)
        m = M.read(what + " mask")
        assert_same(m, m_ref.astype(np.uint8), what + ": mask")
        assert_same(Y.read(what), R.dropout(x, m_ref, ratio), what + ": y")
        assert_same(Y2.read(what), R.dropout(x2, m_ref, ratio), what + ": y of the stored mask")
    if ratio == 0.5 and n > 256:
        a, b = _CACHE[("mask", n, ratio, 12345)], _CACHE[("mask", n, ratio, (1 << 40) + 12345)]
        assert not np.array_equal(a, b), "the inputs are wrong: both seeds give one mask"
    X.free(); X2.free()


def test_elementwise_calls_of_no_elements_touch_nothing(eng):  # noqa: F811
    x = arbitrary(257, 1)
    X = eng.dev(x)
    outs = [Guarded(eng, 257) for _ in range(7)]
    M = Guarded(eng, 257, dtype=np.uint8)
    op(eng, "relu", 0, X, outs[0], 0.01)
    op(eng, "relu_bwd", 0, X, X, outs[1], 0.01)
    op(eng, "axpby", 0, 2.0, X, 0.0, outs[2])
    op(eng, "axpby", 0, 2.0, X, 1.0, outs[3])
    op(eng, "mul", 0, X, X, outs[4], 0)
    op(eng, "dropout", 0, X, outs[5], M, 0.5, 1, 1)
    op(eng, "copy2d", X, 257, outs[6], 257, 0, 257, 0)
    op(eng, "copy2d", X, 257, outs[6], 257, 1, 0, 1)
    for o in outs:
        assert (o.read("n = 0") == SENTINEL).all()
    assert (M.read("n = 0") == MASK_SENTINEL).all()
    X.free()


# =============================================================================== copy2d
N1 = R.PASS + 1
COPY_SHAPES = [(1, 1, 1, 1), (5, 18, 42, 18), (4099, 257, 300, 263), (1, N1, N1, N1)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,cols,ss,ds", COPY_SHAPES)
def test_copy2d_strides_gaps_and_second_pass(eng, rows, cols, ss, ds, accumulate):  # noqa: F811
    """accumulate 0: ARBITRARY source over a sentinel destination.  accumulate 1: EXACT source and destination, applied twice:
    dst0 + 2 src (multiples of 2^-3 up to 3).  The gaps between cols and the destination stride keep the sentinel."""
    n_src, n_dst = rows * ss, rows * ds
    what = "copy2d (%d x %d, strides %d -> %d, accumulate %d)" % (rows, cols, ss, ds, accumulate)
    in_row = (np.arange(n_dst) % ds) < cols
    if accumulate:
        src, dst0 = exact(n_src, 10), np.where(in_row, exact(n_dst, 11), SENTINEL)
        ref = R.copy2d(src, ss, R.copy2d(src, ss, dst0, ds, rows, cols, 1), ds, rows, cols, 1)
        r64 = np.where(in_row, dst0.astype(np.float64) + 2.0 * R.copy2d(src, ss, np.zeros(n_dst), ds, rows, cols, 0), SENTINEL)
        assert R.is_exact_result(r64[in_row], -3) and np.array_equal(ref.astype(np.float64), r64)
    else:
        src, dst0 = arbitrary(n_src, 12), np.full(n_dst, SENTINEL)
        ref = R.copy2d(src, ss, dst0, ds, rows, cols, 0)
    assert (ref[~in_row] == SENTINEL).all() and not (ref[in_row] == SENTINEL).any()
    S, D = eng.dev(src), Guarded(eng, n_dst, init=dst0)
    for _ in range(2 if accumulate else 1):
        op(eng, "copy2d", S, ss, D, ds, rows, cols, accumulate)
    assert_same(D.read(what), ref, what, cols=ds)
    S.free()


# =============================================================================== row kernels
ROWS = [1, 3, 4, 5, 1027]
COLS = [1, 63, 64, 65, 127, 128, 129, 1000]
OUTS = [1, 63, 64, 65, 200]


def row_input(kind, rows, cols, seed):
    gen = R.exact_values if kind == "exact" else R.arbitrary_values
    return cached((kind, rows, cols, seed), lambda: gen(np.random.default_rng(seed * 1009 + rows * 2003 + cols), (rows, cols)))


def same_bits_along_rows(y):
    b = np.ascontiguousarray(y).view(np.uint32)
    return b == b[:, :1]


@pytest.mark.parametrize("kind", ["exact", "arbitrary"])
@pytest.mark.parametrize("rows", ROWS)
def test_rowsum_at_every_wave_edge(eng, rows, kind):  # noqa: F811
    """The whole cross product of cols and num_output.  EXACT inputs: equal to the float64 sum.  ARBITRARY inputs: equal to the sum in
    the wave's own order.  Every replica of a row's sum is one bit pattern."""
    for cols in COLS:
        x = row_input(kind, rows, cols, 20)
        if kind == "exact":
            s = R.rowsum(x, 1)
            assert R.is_exact_input(x) and R.is_exact_result(s, -3)
        else:
            s = cached(("wos", rows, cols, 20), lambda: R.wave_order_sum(x)).reshape(rows, 1)
        X = eng.dev(x)
        outs = [(no, Guarded(eng, rows * no)) for no in OUTS]
        for no, Y in outs:
            op(eng, "rowsum", rows, cols, X, no, Y)
        for no, Y in outs:
            what = "rowsum (%s, %d x %d, num_output %d)" % (kind, rows, cols, no)
            y = Y.read(what).reshape(rows, no)
            assert_same(y, np.repeat(s, no, 1), what, cols=no)
            check(~same_bits_along_rows(y), y, np.repeat(y[:, :1], no, 1), what + ": replicas of one sum differ in their bits", cols=no)
        X.free()


@pytest.mark.parametrize("kind", ["exact", "arbitrary"])
@pytest.mark.parametrize("rows", ROWS)
def test_rowsum_backward_at_every_wave_edge(eng, rows, kind):  # noqa: F811
    """As the forward test, with the roles of cols and num_output exchanged: dx[r][c] = sum_o dy[r][o]."""
    for no in OUTS:
        dy = row_input(kind, rows, no, 21)
        if kind == "exact":
            s = R.rowsum_bwd(dy, 1)
            assert R.is_exact_input(dy) and R.is_exact_result(s, -3)
        else:
            s = cached(("wos", rows, no, 21), lambda: R.wave_order_sum(dy)).reshape(rows, 1)
        DY = eng.dev(dy)
        outs = [(cols, Guarded(eng, rows * cols)) for cols in COLS]
        for cols, DX in outs:
            op(eng, "rowsum_bwd", rows, cols, no, DY, DX)
        for cols, DX in outs:
            what = "rowsum_bwd (%s, %d x %d, num_output %d)" % (kind, rows, cols, no)
            dx = DX.read(what).reshape(rows, cols)
            assert_same(dx, np.repeat(s, cols, 1), what, cols=cols)
            check(~same_bits_along_rows(dx), dx, np.repeat(dx[:, :1], cols, 1), what + ": replicas of one sum differ in their bits", cols=cols)
        DY.free()


def normalize_input(rows, cols, seed):
    """EXACT rows; the last row all zero and, from three rows on, row 1 with a single non-zero in its last column."""
    def make():
        x = R.exact_values(np.random.default_rng(seed * 31 + rows * 2003 + cols), (rows, cols))
        x[0, 0] = 0.625                                            # (no accidental second zero row)
        if rows > 1:
            x[1:, -1][x[1:, -1] == 0] = -0.25
            x[-1] = 0
        if rows > 2:
            x[1] = 0
            x[1, -1] = -0.375
        return x
    return cached(("norm-x", rows, cols, seed), make)


@pytest.mark.parametrize("rows", ROWS)
def test_normalize_at_every_wave_edge(eng, rows):  # noqa: F811
    """EXACT inputs, every cols: s = sum x^2 is exact, and what is left -- sqrtf, + 1e-10f, the reciprocal, one multiply -- is four
    correctly rounded fp32 operations (no fast-math flag in the build; see the module docstring), so the result is held to
    np.array_equal against their fp32 restatement (ops_ref.normalize_f32) instead of the 6 U such a chain could drift from float64; the
    distance to float64 is printed.  Zero rows give exactly 0; the others have norm 1 within 4 U sqrt(cols)."""
    worst = 0.0
    for cols in COLS:
        x = normalize_input(rows, cols, 22)
        s = R.rowsum(x.astype(np.float64) ** 2, 1)
        assert R.is_exact_input(x) and R.is_exact_result(s, -6)
        zero = (x == 0).all(1)
        assert zero[-1] == (rows > 1) and zero.sum() == (rows > 1)
        X, Y = eng.dev(x), Guarded(eng, rows * cols)
        op(eng, "normalize", rows, cols, X, Y)
        what = "normalize (%d x %d)" % (rows, cols)
        y = Y.read(what).reshape(rows, cols)
        X.free()
        assert_same(y, R.normalize_f32(x), what, cols=cols)
        y64 = R.normalize(x)
        live = y64 != 0
        worst = max(worst, (np.abs(y - y64)[live] / np.abs(y64[live])).max() / U)
        assert (y[zero] == 0).all(), what + ": a zero row is not exactly zero"
        if rows > 2:
            assert np.count_nonzero(y[1]) == 1 and y[1, -1] < 0, what + ": the row with a single non-zero"
        nrm = np.sqrt((y.astype(np.float64) ** 2).sum(1))
        assert (np.abs(nrm[~zero] - 1) <= 4 * U * np.sqrt(cols)).all(), (what, np.abs(nrm[~zero] - 1).max())
    print("normalize (rows %d): largest distance to float64 = %.3f U (the derived bound of the four steps: 6 U)" % (rows, worst))
    assert worst <= 6


@pytest.mark.parametrize("rows", ROWS)
def test_normalize_backward_at_every_wave_edge(eng, rows):  # noqa: F811
    """EXACT x and dy, every cols: s and d = x . dy are exact.  Per element |dx - ref| <= 4 U (|s dy| + |x d|) inv + 6 U |ref|: the
    first term covers either contraction of the numerator, the second s * sqrtf(s), the add, the divide and the final multiply
    (ops_ref.normalize_bwd).  Zero rows give exactly 0."""
    for cols in COLS:
        x, dy = normalize_input(rows, cols, 23), row_input("exact", rows, cols, 24)
        x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
        assert R.is_exact_input(x) and R.is_exact_input(dy)
        assert R.is_exact_result((x64 * x64).sum(1), -6) and R.is_exact_result((x64 * dy64).sum(1), -6)
        ref, bound = R.normalize_bwd(x, dy)
        X, DY, DX = eng.dev(x), eng.dev(dy), Guarded(eng, rows * cols)
        op(eng, "normalize_bwd", rows, cols, X, DY, DX)
        what = "normalize_bwd (%d x %d)" % (rows, cols)
        dx = DX.read(what).reshape(rows, cols)
        X.free(); DY.free()
        assert_within(dx, ref, bound, what, cols=cols)
        zero = (x == 0).all(1)
        assert (dx[zero] == 0).all(), what + ": a zero row is not exactly zero"


def test_normalize_backward_is_the_gradient_at_5_x_65(eng):  # noqa: F811
    """One finite-difference check past one trip of the lanes (the reference's GradientChecker recipe, as tests/test_gpu_ops.py)."""
    rng = np.random.default_rng(25)
    x, dy = R.arbitrary_values(rng, (5, 65)), R.arbitrary_values(rng, (5, 65))
    X, DY, DX = eng.dev(x), eng.dev(dy), Guarded(eng, 5 * 65)
    op(eng, "normalize_bwd", 5, 65, X, DY, DX)
    dx = DX.read("normalize_bwd").reshape(5, 65)
    X.free(); DY.free()
    assert_grad(dx.astype(np.float64), numeric_grad(R.normalize, x, dy))


def test_row_calls_of_no_rows_touch_nothing(eng):  # noqa: F811
    X = eng.dev(exact(256, 1))
    outs = [Guarded(eng, 256) for _ in range(4)]
    op(eng, "rowsum", 0, 64, X, 64, outs[0])
    op(eng, "rowsum_bwd", 0, 64, 64, X, outs[1])
    op(eng, "normalize", 0, 64, X, outs[2])
    op(eng, "normalize_bwd", 0, 64, X, X, outs[3])
    for o in outs:
        assert (o.read("rows = 0") == SENTINEL).all()
    X.free()


# =============================================================================== max_margin
COUNTS = [1, 255, 256, 257, 1000, R.PASS + 3]
MARGIN, LOSS_WEIGHT = 1.0, 1.5


@pytest.mark.parametrize("norm,weighted", [(2, False), (1, False), (2, True), (1, True)])
@pytest.mark.parametrize("count", COUNTS)
def test_max_margin_counts_every_term(eng, count, norm, weighted):  # noqa: F811
    """EXACT scores with d = 0 (no violation, hinge = margin) and margin - d = 0 among them, weights with exact square roots, 0
    included (ops_ref.margin_case).  Every h and h^2 is exact and their double sum is an exact count of 2^-8 units: the loss is
    float32(sum / count) within one fp32 ulp (the final divide and cast), the violations are the integer count.

    Backward: |g - ref| <= 3 U |ref| (the fp32 coefficient lw 2 / count: one rounding, lw 2 is exact; the product with h w: one more; a
    third for the L1 form's lw / count times w), d_true == -d_bogus bit for bit, an inactive hinge gives exactly 0."""
    st, sb, w = cached(("margin", count, weighted), lambda: R.margin_case(count, weighted))
    ST, SB = eng.dev(st), eng.dev(sb)
    Wd = eng.dev(w) if weighted else None
    what = "max_margin (count %d, L%d, %s)" % (count, norm, "weighted" if weighted else "unweighted")
    loss, viol = ctypes.c_float(-1), ctypes.c_float(-1)
    op(eng, "max_margin", count, ST, SB, Wd, MARGIN, norm, ctypes.byref(loss), ctypes.byref(viol))
    ref_loss, ref_viol = R.max_margin(st, sb, w, MARGIN, norm)
    assert viol.value == ref_viol, "%s: %r violations, expected %d" % (what, viol.value, ref_viol)
    want = np.float32(ref_loss)
    print("%s: loss %r, expected %r: %.2f ulp" % (what, loss.value, float(want), abs(np.float64(loss.value) - np.float64(want)) / np.spacing(want)))
    assert abs(np.float64(loss.value) - np.float64(want)) <= np.spacing(want), (what, loss.value, float(want))
    DT, DB = Guarded(eng, count), Guarded(eng, count)
    op(eng, "max_margin_bwd", count, ST, SB, Wd, MARGIN, norm, LOSS_WEIGHT, DT, DB)
    dt, db = DT.read(what + " d_true"), DB.read(what + " d_bogus")
    g, active = R.max_margin_bwd(st, sb, w, MARGIN, norm, LOSS_WEIGHT)
    assert_within(db, g, 3 * U * np.abs(g), what + ": d_bogus")
    assert_same(dt.view(np.uint32), (-db).view(np.uint32), what + ": d_true is not -d_bogus bit for bit")
    check(~active & (db != 0), db, g, what + ": an inactive hinge has a gradient")
    for d in (ST, SB, Wd):
        if d is not None:
            d.free()


# =============================================================================== argument checks
def test_bad_arguments_are_refused_and_the_engine_lives_on(eng):  # noqa: F811
    import videovector_amd as vv
    n = 300
    x = arbitrary(n, 30)
    X = eng.dev(x)
    st, sb, w = R.margin_case(257, True)
    ST, SB, Wd = eng.dev(st), eng.dev(sb), eng.dev(w)
    for ratio in (1.0, -0.1, float("nan")):
        Y, M = Guarded(eng, n), Guarded(eng, n, dtype=np.uint8)
        with pytest.raises(vv.VVError, match="dropout_ratio"):
            op(eng, "dropout", n, X, Y, M, ratio, 7, 1)
        assert (Y.read("refused dropout") == SENTINEL).all() and (M.read("refused dropout") == MASK_SENTINEL).all()
        Y, M = Guarded(eng, n), Guarded(eng, n, dtype=np.uint8)
        op(eng, "dropout", n, X, Y, M, 0.5, 7, 1)
        assert_same(Y.read("dropout"), R.dropout(x, R.dropout_mask(7, n, 0.5), 0.5), "dropout after a refused call")
        M.read("dropout")
    loss, viol = ctypes.c_float(), ctypes.c_float()
    for count, norm in ((0, 2), (0, 1), (257, 3), (257, 0), (-1, 2)):
        DT, DB = Guarded(eng, 257), Guarded(eng, 257)
        with pytest.raises(vv.VVError, match="vv_op_max_margin:"):
            op(eng, "max_margin", count, ST, SB, Wd, MARGIN, norm, ctypes.byref(loss), ctypes.byref(viol))
        with pytest.raises(vv.VVError, match="vv_op_max_margin_bwd:"):
            op(eng, "max_margin_bwd", count, ST, SB, Wd, MARGIN, norm, LOSS_WEIGHT, DT, DB)
        assert (DT.read("refused max_margin_bwd") == SENTINEL).all() and (DB.read("refused max_margin_bwd") == SENTINEL).all()
        op(eng, "max_margin", 257, ST, SB, Wd, MARGIN, 2, ctypes.byref(loss), ctypes.byref(viol))
        ref_loss, ref_viol = R.max_margin(st, sb, w, MARGIN, 2)
        assert viol.value == ref_viol and abs(np.float64(loss.value) - np.float64(np.float32(ref_loss))) <= np.spacing(np.float32(ref_loss))
    for d in (X, ST, SB, Wd):
        d.free()


# =============================================================================== related: an all-zero dY through INNER_PRODUCT backward
def test_inner_product_backward_of_zero_gradients_is_zero(eng):  # noqa: F811
    """max |dY| = 0 must leave the f16 gradient scale at 1 (half_scale(0); the scale itself is not readable on the per-layer path, its
    host restatement is): dW and db come out exactly 0, not 0 x inf."""
    assert eng.prec == "f16" and half_scale(0.0, "f16") == 1.0
    ds, W, b = eng._case
    R_ = 300
    x = ds.table(64)[:R_]
    X, Y, DY = eng.dev(x), eng.dev((R_, 24)), eng.dev(np.zeros((R_, 24), np.float32))
    eng.op("inner_product", X, R_, Y)
    eng.op("inner_product_bwd", DY, R_, 0.0)
    dW, db = eng.grads()
    assert dW.shape == W.shape and db.shape == b.shape
    assert not np.isnan(dW).any() and not np.isnan(db).any()
    assert (dW == 0).all() and (db == 0).all()
    X.free(); Y.free(); DY.free()
