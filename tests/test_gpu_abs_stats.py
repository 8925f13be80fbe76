"""vv_op_asum (k_abs_stats; Blob::asum_data / asum_diff without the download, blob.cpp:138-165) against numpy float64.

(a) Exactly representable operands: small integers times a power of two, signs mixed, total below 2^53 -- every partial sum is exact in
    double whatever the order, so asum, amax, count and nonfinite must EQUAL the float64 values.  Sizes: around the wave (63, 64, 65), the
    workgroup (255, 256, 257), the 16-byte item (1, 3, 4, 5), around one pass of the kernel's grid (GRID_ELEMS = STAT_BLOCKS x 256 threads x
    4 floats, read from vv_internal.h's constant; +-1 and 2 x + 7), and buffers that start one, two and three floats past a 16-byte boundary
    (a scalar head and tail).
(b) Random fp32 values: k_abs_stats adds n non-negative doubles (|x| of an fp32 is exact in double), every addition correctly rounded, so
    its sum is within (n - 1) 2^-53 relatively of the true sum in any order; numpy's float64 sum carries the same kind of error.  With
    n <= 2^24 both are within 2^-29 of the true sum, 2^-5 of fp32's half-ulp: the two SINGLE roundings to fp32 can differ only where a
    rounding boundary lies between them, by at most 1 ulp -- the bound tests/test_gpu_clip_gradients.py holds the norm to, for the same
    reason.  amax is exact.
(c) NaN, +Inf, -Inf planted at the first, a middle and the last element and in the scalar head and tail count in nonfinite and nowhere
    else; -0 and subnormals are finite values like any other.
(d) Two calls return bit-identical records.
(e) A zero-only buffer.

Without the feature the binding has no op_asum: every case fails.
"""
import os
import re

import numpy as np
import pytest

from tests.test_gpu_parity import vv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_elems():
    """one pass of k_abs_stats' grid in floats: STAT_BLOCKS workgroups x 256 threads x one 16-byte item"""
    src = open(os.path.join(ROOT, "videovector_amd", "csrc", "vv_internal.h")).read()
    return int(re.search(r"constexpr int STAT_BLOCKS = (\d+);", src).group(1)) * 256 * 4


GRID_ELEMS = grid_elems()
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, GRID_ELEMS - 1, GRID_ELEMS, GRID_ELEMS + 1, 2 * GRID_ELEMS + 7]


@pytest.fixture(scope="module")
def eng(vv):  # noqa: F811
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    assert a >= 0 and b >= 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def ref64(x):
    """(asum, amax, count, nonfinite) in float64 over the finite elements"""
    fin = np.isfinite(x)
    a = np.abs(x[fin].astype(np.float64))
    return float(a.sum()), np.float32(a.max() if a.size else 0.0), int(x.size), int(x.size - fin.sum())


def measure(eng, x, shift=0):
    """x uploaded `shift` floats past a 16-byte boundary"""
    host = np.zeros(x.size + shift + 4, np.float32)
    host[shift:shift + x.size] = x
    buf = eng.dev(host)
    try:
        assert buf.ptr.value % 16 == 0
        return eng.op_asum(buf, x.size, offset=shift)
    finally:
        buf.free()


def exact_operands(rng, n):
    """integers in [-255, 255] times 2^-9: |x| sums below 2^53 ulps of 2^-9, every double partial sum exact"""
    return (rng.integers(-255, 256, size=n) * 2.0 ** -9).astype(np.float32)


# ------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("n", SIZES)
def test_exact_operands_equal_float64(eng, n):
    assert GRID_ELEMS == 262144
    x = exact_operands(np.random.default_rng(n), n)
    got, want = measure(eng, x), ref64(x)
    print("n = %d: %r against %r" % (n, got, want))
    assert got == want


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 257, GRID_ELEMS + 6])
def test_buffers_that_start_off_a_16_byte_boundary(eng, shift, n):
    x = exact_operands(np.random.default_rng(100 * n + shift), n)
    got, want = measure(eng, x, shift), ref64(x)
    print("n = %d, %d floats past the boundary: %r against %r" % (n, shift, got, want))
    assert got == want


# ------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("n,shift", [(257, 0), (4099, 1), (GRID_ELEMS + 5, 0), (3 * GRID_ELEMS + 2, 3)])
def test_random_values_within_one_ulp_of_float64(eng, n, shift):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, size=n))).astype(np.float32)
    asum, amax, count, nonfinite = measure(eng, x, shift)
    r = ref64(x)
    print("n = %d: asum %r against float64 %r; amax %r against %r" % (n, asum, r[0], amax, r[1]))
    assert ulps(np.float32(asum), np.float32(r[0])) <= 1
    assert amax == r[1] and count == n and nonfinite == 0


# ------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("n,shift", [(1031, 0), (1030, 1), (1030, 3), (GRID_ELEMS + 9, 2)])
def test_non_finite_values_count_in_nonfinite_only(eng, bad, n, shift):
    """first, middle, last; with shift != 0 the first lies in the scalar head (4 - shift floats), and the last in the scalar tail"""
    x = exact_operands(np.random.default_rng(n + shift), n)
    if shift:
        assert (n - (4 - shift)) % 4 != 0, "the case needs a scalar tail"
    clean = ref64(x)
    for where in ([0], [n // 2], [n - 1], [0, 1, n // 2, n - 2, n - 1]):
        y = x.copy()
        y[where] = bad
        got, want = measure(eng, y, shift), ref64(y)
        assert got == want, (where, got, want)
        assert got[3] == len(where) and got[2] == n and np.isfinite(got[0]) and np.isfinite(got[1]) and got[0] <= clean[0]


def test_all_non_finite(eng):
    x = np.array([np.nan, np.inf, -np.inf, np.nan, np.inf], np.float32)
    assert measure(eng, x, 1) == (0.0, np.float32(0), 5, 5)


def test_negative_zero_and_subnormals(eng):
    tiny = np.float32(2.0 ** -149)
    x = np.array([-0.0, tiny, -tiny, np.float32(2.0 ** -127), -0.0, np.float32(-3 * 2.0 ** -149), 0.0], np.float32)
    got = measure(eng, x)
    assert got == ref64(x) and got[0] == float(5 * 2.0 ** -149 + 2.0 ** -127) and got[1] == np.float32(2.0 ** -127) and got[3] == 0
    z = np.full(9, -0.0, np.float32)
    assert measure(eng, z, 2) == (0.0, np.float32(0), 9, 0)


# ------------------------------------------------------------------------------- (d), (e)
def test_two_calls_return_the_same_bits(eng):
    n = 2 * GRID_ELEMS + 1001
    rng = np.random.default_rng(5)
    buf = eng.dev(rng.standard_normal(n).astype(np.float32))
    try:
        a, b = eng.op_asum(buf), eng.op_asum(buf)
    finally:
        buf.free()
    assert np.float64(a[0]).view(np.uint64) == np.float64(b[0]).view(np.uint64) and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2:] == b[2:]


@pytest.mark.parametrize("n", [1, 7, GRID_ELEMS + 3])
def test_zero_only_buffer(eng, n):
    assert measure(eng, np.zeros(n, np.float32)) == (0.0, np.float32(0), n, 0)


def test_arguments(eng, vv):  # noqa: F811
    buf = eng.dev((8,))
    try:
        for n in (0, -1):
            with pytest.raises(vv.VVError) as e:
                eng.op_asum(buf, n)
            assert "videovec error 1" in str(e.value), str(e.value)      # VV_ERR_ARG
    finally:
        buf.free()
