"""tests/ops_ref.py is right before a kernel is held to it: every restatement agrees with the oracle (the fp32 C restatement of the
reference's layers) at the shapes of tests/test_gpu_ops.py, the kernel-order sum equals the exact sum on exact inputs, and the input
generators deliver what they claim.  A failure here means a wrong reference or a wrong input, not a wrong kernel.

The oracle works in fp32 in its own order, the restatements in float64: the bounds below are the oracle's rounding, n U per n-term
fp32 sum (U = 2^-24) relative to the sum of magnitudes, plus one U per further operation.
"""
import math

import numpy as np
import pytest

from tests import ops_ref as R

U = R.U


def test_input_generators_keep_their_promises():
    rng = np.random.default_rng(0)
    x = R.exact_values(rng, (1027, 1000))
    assert R.is_exact_input(x)
    assert set(np.unique(x * 8).astype(int)) == set(range(-8, 9))
    zeros = (x == 0).mean()
    assert 0.33 < zeros < 0.43                                     # a third forced to zero plus the 1 / 17 drawn as zero
    y = R.exact_values(rng, x.shape)
    prod = x.astype(np.float64) * y.astype(np.float64)
    assert R.is_exact_result(prod, -6) and np.array_equal((x * y).astype(np.float64), prod)          # every product exact in fp32
    assert R.is_exact_result(prod.sum(1), -6) and R.is_exact_result(x.astype(np.float64).sum(1), -3)  # every <= 1000-term sum
    assert not R.is_exact_input(np.array([0.3], np.float32)) and not R.is_exact_input(np.array([1.125], np.float32))
    assert not R.is_exact_result(np.array([2.0 ** 24]), 0) and not R.is_exact_result(np.array([0.5]), 0)
    a = R.arbitrary_values(rng, 1000)
    assert a.dtype == np.float32 and not R.is_exact_input(a)


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000, 1048579])
def test_margin_case_is_exact_and_holds_its_edges(count):
    st, sb, w = R.margin_case(count, True)
    assert R.is_exact_input(st) and R.is_exact_input(sb)
    assert set(np.unique(w)) <= set(R.MARGIN_WEIGHTS.tolist())
    assert np.array_equal(np.sqrt(w).astype(np.float64) ** 2, w.astype(np.float64))                  # exact square roots
    d = st.astype(np.float64) - sb.astype(np.float64)
    assert np.array_equal((st - sb).astype(np.float64), d)                                           # d exact in fp32
    assert (d == 0).any()
    if count > 3:
        assert (d == 1).any() and (w == 0).any() and (d < 0).any() and ((d > 0) & (d < 1)).any()
    for norm in (1, 2):
        _, h = R.hinge(st, sb, w, 1.0, norm)
        assert np.array_equal(h.astype(np.float32).astype(np.float64), h)                             # every term exact in fp32
        term = h * h if norm == 2 else h
        assert np.array_equal(term * 256, np.rint(term * 256)) and (term * 256).sum() < 2 ** 53       # ... and the double sum exact
        assert math.fsum(term) == term.sum()


def test_wave_order_sum_is_the_exact_sum_on_exact_inputs():
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 127, 128, 129, 200, 1000):
        x = R.exact_values(rng, (9, n))
        got = R.wave_order_sum(x)
        assert got.dtype == np.float32 and got.shape == (9,)
        assert [float(v) for v in got] == [math.fsum(float(v) for v in row) for row in x]
    assert np.array_equal(R.wave_order_sum(np.zeros((3, 0), np.float32)), np.zeros(3, np.float32))


def test_wave_order_sum_follows_the_lanes_on_arbitrary_inputs():
    """The order matters on arbitrary inputs (else the restatement would test nothing): spelled out lane by lane for one row."""
    rng = np.random.default_rng(2)
    x = R.arbitrary_values(rng, (4, 129))
    got = R.wave_order_sum(x)
    p = [np.float32(0)] * 64
    for c in range(129):
        p[c % 64] = np.float32(p[c % 64] + x[2, c])
    for o in (32, 16, 8, 4, 2, 1):
        p = [np.float32(p[l] + p[l ^ o]) for l in range(64)]
    assert len({v.tobytes() for v in p}) == 1 and got[2].tobytes() == p[0].tobytes()
    exact = x.astype(np.float64).sum(1)
    assert (np.abs(got - exact) <= 129 * U * np.abs(x).astype(np.float64).sum(1)).all()
    seq = np.zeros(4, np.float32)
    for c in range(129):
        seq = seq + x[:, c]
    assert (seq != got).any()                                      # ... and differs from the plain left-to-right fp32 sum


def test_elementwise_restatements_match_the_oracle(oracle):
    rng = np.random.default_rng(0)
    x, dy = R.arbitrary_values(rng, (6, 50)), R.arbitrary_values(rng, (6, 50))
    x[0, :4] = [0.0, -0.0, 1.0, -1.0]
    for slope in (0.0, 0.01):
        assert np.array_equal(R.relu(x, slope), oracle.relu_fwd(x, slope))
        assert np.array_equal(R.relu_bwd(x, dy, slope), oracle.relu_bwd(x, dy, slope))
    a, b, c3 = [R.exact_values(rng, (4, 30)) for _ in range(3)]
    y = R.axpby(2.0, c3, 1.0, R.axpby(-0.5, b, 1.0, R.axpby(1.0, a, 0.0, np.zeros_like(a))))
    assert np.array_equal(y, oracle.eltwise_fwd("SUM", [a, b, c3], [1, -0.5, 2]))
    assert np.array_equal(y.astype(np.float64), a.astype(np.float64) - 0.5 * b + 2.0 * c3)
    p, q = R.arbitrary_values(rng, (4, 30)), R.arbitrary_values(rng, (4, 30))
    assert np.array_equal(R.mul(p, q), oracle.eltwise_fwd("PROD", [p, q]))
    assert np.array_equal(R.mul(a, b, y, 1).astype(np.float64), y.astype(np.float64) + a.astype(np.float64) * b)
    d0, d1, d2 = [R.arbitrary_values(rng, 5 * 7 * 6) for _ in range(3)]
    s = R.copy2d(d0, d0.size, np.zeros_like(d0), d0.size, 1, d0.size, 0)
    s = R.copy2d(d2, d0.size, R.copy2d(d1, d0.size, s, d0.size, 1, d0.size, 1), d0.size, 1, d0.size, 1)
    assert np.array_equal(s, oracle.split_bwd([d0, d1, d2]))
    x3 = R.arbitrary_values(rng, (5, 7, 6))
    t0 = R.copy2d(x3, 42, np.zeros(5 * 18, np.float32), 18, 5, 18, 0)
    t1 = R.copy2d(x3.reshape(-1)[18:], 42, np.zeros(5 * 24, np.float32), 24, 5, 24, 0)
    o0, o1 = oracle.slice_fwd(x3, 1, [3, 4])
    assert np.array_equal(t0, o0.reshape(-1)) and np.array_equal(t1, o1.reshape(-1))
    assert np.array_equal(R.copy2d(x3, 42, t0, 18, 0, 18, 0), t0) and np.array_equal(R.copy2d(x3, 42, t0, 18, 5, 0, 1), t0)


def test_dropout_restatement(oracle):
    n = 200000
    x = R.arbitrary_values(np.random.default_rng(1), n)
    for ratio in (0.0, 0.5, 0.6, 0.9):
        for seed in (12345, (1 << 40) + 77):
            m = R.dropout_mask(seed, n, ratio)
            assert m.dtype == bool and abs(m.mean() - (1 - ratio)) <= 4 * np.sqrt(ratio * (1 - ratio) / n)
            assert np.array_equal(R.dropout(x, m, ratio), oracle.dropout_fwd(x, m, ratio))
    assert R.dropout_mask(5, n, 0.0).all() and R.dropout_scale(0.0) == 1 and R.dropout_scale(0.5) == 2
    assert R.dropout_scale(0.9).dtype == np.float32
    assert not np.array_equal(R.dropout_mask(12345, n, 0.5), R.dropout_mask((1 << 40) + 12345, n, 0.5))       # the high seed bits count
    h = R.mix64(12345, np.arange(4, dtype=np.uint64))                                                        # element i is keyed on i
    assert [int(v) for v in h] == [int(R.mix64(12345, np.uint64(i))) for i in range(4)]
    assert np.array_equal(R.dropout_mask(9, 70, 0.5), R.dropout_mask(9, n, 0.5)[:70])


@pytest.mark.parametrize("num_output", [1, 10])
def test_sum_restatements_match_the_oracle(oracle, num_output):
    rng = np.random.default_rng(4)
    x, dy = R.arbitrary_values(rng, (6, 20)), R.arbitrary_values(rng, (6, num_output))
    y, dx = R.rowsum(x, num_output), R.rowsum_bwd(dy, 20)
    assert y.dtype == np.float64 and y.shape == (6, num_output) and dx.shape == (6, 20)
    assert (np.abs(oracle.sum_fwd(x, num_output) - y) <= 20 * U * np.abs(x).sum(1, keepdims=True)).all()
    assert (np.abs(oracle.sum_bwd(dy, 20) - dx) <= num_output * U * np.abs(dy).sum(1, keepdims=True)).all()
    xe, dye = R.exact_values(rng, (6, 20)), R.exact_values(rng, (6, num_output))
    assert np.array_equal(oracle.sum_fwd(xe, num_output), R.rowsum(xe, num_output))
    assert np.array_equal(oracle.sum_bwd(dye, 20), R.rowsum_bwd(dye, 20))
    assert np.array_equal(R.wave_order_sum(xe), R.rowsum(xe, 1)[:, 0])


def test_normalize_restatements_match_the_oracle(oracle):
    rng = np.random.default_rng(5)
    x, dy = R.arbitrary_values(rng, (7, 33)), R.arbitrary_values(rng, (7, 33))
    x[3] = 0
    y = R.normalize(x)
    assert (np.abs(oracle.normalize_fwd(x) - y) <= (33 + 4) * U * np.abs(y)).all() and (y[3] == 0).all()
    dx, _ = R.normalize_bwd(x, dy)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    s = (x64 * x64).sum(1, keepdims=True)
    mag = (np.abs(s * dy64) + np.abs(x64) * np.abs(x64 * dy64).sum(1, keepdims=True)) / (s ** 1.5 + 1e-10)
    assert (np.abs(oracle.normalize_bwd(x, dy) - dx) <= (2 * 33 + 8) * U * mag).all() and (dx[3] == 0).all()
    # exact rows: the fp32 restatement of the four inexact steps is within their 6 U of float64, and the oracle's x / nrm within 3 U
    xe = R.exact_values(rng, (7, 33))
    xe[3] = 0
    xe[5] = 0
    xe[5, 17] = -0.375
    y32, y64 = R.normalize_f32(xe), R.normalize(xe)
    assert y32.dtype == np.float32 and (np.abs(y32 - y64) <= 6 * U * np.abs(y64)).all()
    assert (np.abs(oracle.normalize_fwd(xe) - y64) <= 3 * U * np.abs(y64)).all()
    assert (y32[3] == 0).all() and y32[5, 17] == -1 and np.count_nonzero(y32[5]) == 1
    with pytest.raises(AssertionError):
        R.normalize_f32(x)                                                                           # arbitrary rows are refused
    dxe, bound = R.normalize_bwd(xe, R.exact_values(rng, (7, 33)))
    assert (dxe[3] == 0).all() and (bound[3] == 0).all() and (bound >= 0).all() and np.isfinite(bound).all()


@pytest.mark.parametrize("norm,weighted", [(2, False), (1, False), (2, True), (1, True)])
def test_max_margin_restatements_match_the_oracle(oracle, norm, weighted):
    rng = np.random.default_rng(6)
    cnt, margin, lw = 60, 2.0, 1.5
    st, sb = R.arbitrary_values(rng, cnt), R.arbitrary_values(rng, cnt)
    w = (rng.random(cnt).astype(np.float32) * 2) if weighted else None
    loss, viol = R.max_margin(st, sb, w, margin, norm)
    ol, ov = oracle.max_margin_fwd(st, sb, margin, norm, weight=w)
    # fp32 d = st - sb is off by U |d| ABSOLUTE (margin - d cancels): that much times the term's slope, besides the relative roundings
    # of margin - d, sqrt, the product (squared: twice) and the cast / of margin - d, the weight, the coefficient and the product
    d, h = R.hinge(st, sb, w, margin, norm)
    wt = np.ones(cnt) if w is None else w.astype(np.float64)
    slope = 2 * h * np.sqrt(wt) if norm == 2 else wt
    assert abs(ol - loss) <= 10 * U * loss + U * (np.abs(d) * slope).mean() and ov == viol
    g, active = R.max_margin_bwd(st, sb, w, margin, norm, lw)
    ot, ob = oracle.max_margin_bwd(st, sb, margin, norm, loss_weight=lw, weight=w)
    dg = U * np.abs(d) * wt * (2 * lw / cnt) if norm == 2 else 0.0
    assert (np.abs(ob - g) <= 6 * U * np.abs(g) + dg).all() and np.array_equal(ot, -ob) and np.array_equal(ob != 0, active)
    for count in (1, 257, 1000):                                              # the exact cases: the oracle gives THE numbers
        st, sb, w = R.margin_case(count, weighted)
        loss, viol = R.max_margin(st, sb, w, 1.0, norm)
        ol, ov = oracle.max_margin_fwd(st, sb, 1.0, norm, weight=w)
        assert ol == np.float32(loss) and ov == viol
        g, active = R.max_margin_bwd(st, sb, w, 1.0, norm, lw)
        _, ob = oracle.max_margin_bwd(st, sb, 1.0, norm, loss_weight=lw, weight=w)
        assert (np.abs(ob - g) <= 3 * U * np.abs(g)).all() and np.array_equal(ob != 0, active)
        assert (g[~active] == 0).all() and (g[active] > 0).all()
