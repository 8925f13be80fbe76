"""tests/eval_head_ref.py is right before a kernel is held to it: for the inputs of tests/test_gpu_eval_head_exact.py the exactness
assertions hold, the reference alone stays inside every condition, and each deliberately wrong model of a kernel -- truncation instead
of round-to-nearest-even, the last window slot dropped, column F - 1 of the mean taken from slot 0 only, the Gram matrix without its
last K-tile, its edge tile written one row down, ties broken by descending index -- is rejected by the same comparison the GPU test
makes.  A failure here means a wrong reference or a wrong input, not a wrong kernel.  No GPU."""
import numpy as np
import pytest

from tests import eval_head_ref as R
from tests.test_gpu_eval_head_exact import MEAN_COEFF, MEAN_SHAPES
from tests.test_gpu_parity import round_operand

NS = [1, 37, 257]


@pytest.mark.parametrize("prec", R.PRECS)
def test_table_and_identity_layer_are_exact_operands(prec):
    for F in (100, 320):
        T = R.table(F)
        assert set(np.unique(T)) == {0.0, 1.0, 2.0, 3.0} and 0.4 < (T == 0).mean() < 0.6
        assert not T[list(R.ZERO_ROWS)].any()
        assert np.array_equal(R.round_rows(T.astype(np.float64), prec), T)
        for D in (63, 64, 65, 100, 250, 320):
            if D <= F:
                W, b = R.identity_layer(D, F, prec)
                assert np.array_equal(round_operand(W, prec), W) and not b.any()
                assert np.array_equal(T.astype(np.float64) @ W.astype(np.float64).T, T[:, :D])      # the layer reads columns 0 .. D-1 out


def test_window_rows_hold_the_edges():
    seen_first = seen_last = False
    for n in (1, 3, 4, 5, 37, 257, 1100):
        for k in (1, 2, 4, 7):
            rows = R.window_rows(n, k)
            assert rows.shape == (n, k) and rows.min() >= 0 and rows.max() < R.N_ROWS
            seen_first |= bool((rows == 0).any())
            seen_last |= bool((rows == R.N_ROWS - 1).any())
            if k > 1 or n >= 4:
                assert (rows == 0).any() and (rows == R.N_ROWS - 1).any()
            if n >= 3:
                assert (rows[1] == rows[1, 0]).all() and set(rows[2]) <= set(R.ZERO_ROWS)
    assert seen_first and seen_last


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("k,kind", MEAN_COEFF)
@pytest.mark.parametrize("D,F", MEAN_SHAPES)
def test_mean_reference_is_exact_and_rejects_the_wrong_kernels(prec, D, F, k, kind):
    T = R.table(F)
    rejected_col = False
    for n in NS:
        rows, coeff = R.window_rows(n, k), R.coefficients(k, kind)
        m = R.mean64(T, rows, coeff)                                    # (asserts exactness in fp32, in any order)
        ref = R.mean_ref(T, rows, coeff, prec, D)
        assert ref.shape == (n, D)
        if prec == "f16":
            assert np.array_equal(ref, m[:, :D])                        # 11 bits hold every mean of these coefficients
        if n >= 3:
            assert not ref[2].any()                                     # the all-zero window
            if kind == "uniform":
                assert np.array_equal(ref[1], T[123, :D])               # one row in every slot (the coefficients sum to 1)
        if k > 1 and n > 1:
            wrong = R.round_rows(R.mean_last_slot_dropped(T, rows, coeff), prec)[:, :D]
            assert not np.array_equal(wrong, ref), "a dropped last slot would pass"
            if D == F:
                wrong = R.round_rows(R.mean_last_column_from_slot0(T, rows, coeff), prec)[:, :D]
                assert np.array_equal(wrong[:, :-1], ref[:, :-1])
                rejected_col |= not np.array_equal(wrong, ref)
    if k > 1 and D == F:
        assert rejected_col, "a last column taken from slot 0 only would pass at every n"


def test_one_row_in_every_slot_reads_as_that_row_only_under_uniform_coefficients():
    # (what the n >= 3 assertion above relies on: sum coeff = 1 for 'uniform'; 'distinct' sums to 1 - 2^-k, so it is skipped there)
    T = R.table(100)
    for k, kind in MEAN_COEFF:
        rows = R.window_rows(5, k)
        m = R.mean64(T, rows, R.coefficients(k, kind))
        scale = 1.0 if kind == "uniform" else 1.0 - 2.0 ** -k
        assert np.array_equal(m[1], scale * T[123])


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("F", [100, 320])
def test_tie_inventory_is_non_empty_in_both_directions_and_rejects_truncation(prec, F):
    T = R.table(F)
    rows, coeff = R.window_rows(257, 2), R.coefficients(2, "tie", prec)
    down, up = R.tie_inventory(T, rows, prec)
    assert down.sum() > 100 and up.sum() > 100
    m = R.mean64(T, rows, coeff)
    ref, trunc = R.round_rows(m, prec), R.truncate_rows(m, prec)
    assert np.array_equal(trunc[down], ref[down]) and (trunc[up] < ref[up]).all()        # truncation is wrong exactly where RNE goes up
    assert not np.array_equal(trunc, ref)
    # the truncating model itself: never above, less than one 16-bit ulp below, idempotent
    x = np.abs(np.random.default_rng(0).standard_normal(1000)) * 3
    t = R.truncate_rows(x, prec)
    assert (t <= x.astype(np.float32)).all() and np.array_equal(R.truncate_rows(t, prec), t) and np.array_equal(R.round_rows(t, prec), t)
    assert ((x.astype(np.float32) - t) < np.maximum(t, 2.0 ** -14) * 2.0 ** (-10 if prec == "f16" else -7)).all()


def test_range_scale_case_is_exact_in_scaled_f16():
    T = R.table(100, R.RANGE_SCALE)
    assert T.max() == 3 * R.RANGE_SCALE > 16384.0                     # outside [2^-8, 2^14]: the f16 table leaves scale 1
    with np.errstate(over="ignore"):
        assert np.isinf(T.astype(np.float16)).any()                   # ... and would not survive at scale 1
    assert 2 ** 7 <= T.max() * R.RANGE_SX < 2 ** 8
    rows = R.window_rows(37, 4)
    m = R.mean64(T, rows, None)
    assert np.array_equal(R.round_rows(m, "f16", R.RANGE_SX), m)
    assert np.array_equal(R.round_rows(T.astype(np.float64), "f16", R.RANGE_SX), T)
    wrong = R.round_rows(R.mean_last_slot_dropped(T, rows, None), "f16", R.RANGE_SX)
    assert not np.array_equal(wrong, m)


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("D", [63, 64, 65, 250, 320])
def test_normalize_reference_and_bound(prec, D):
    T = R.table(320)
    for n in (1, 3, 4, 5, 37):
        rows, win = R.norm_rows(n), R.window_rows(n, 4)
        for e, zero in ((T[rows][:, :D].astype(np.float64), 1), (R.mean_ref(T, win, None, prec, D), 2)):
            ref = R.normalize_ref(e)                                   # (asserts that sum e^2 is exact in fp32)
            assert np.isfinite(ref).all()
            if n >= 3:
                assert not ref[zero].any()
            live = e.any(1)
            assert np.allclose((ref[live] ** 2).sum(1), 1.0, rtol=1e-9)
            model = R.normalize_fp32_model(e)
            assert model.dtype == np.float32 and R.within_normalize_bound(model, ref)       # the four roundings stay inside the bound
            if live.any():                                             # ... a result 8 x 2^-24 off does not, nor a zero row that moved
                assert not R.within_normalize_bound(model * np.float32(1 + 2.0 ** -21), ref)
            if n >= 3:
                moved = model.copy()
                moved[zero, 0] = np.float32(1e-30)
                assert not R.within_normalize_bound(moved, ref)


@pytest.mark.parametrize("n,dim", R.GRAM_CASES)
def test_gram_reference_is_exact_and_rejects_the_wrong_kernels(n, dim):
    X = R.gram_operand(n, dim)
    assert set(np.unique(X)) <= set(range(-3, 4))
    ref = R.gram_ref(X)                                                # (asserts integers below 2^24)
    assert np.array_equal(ref, ref.T) and np.array_equal(np.diag(ref), -2.0 * (X.astype(np.float64) ** 2).sum(1))
    assert np.array_equal((np.float32(-2.0) * (X @ X.T)).astype(np.float64), ref)          # fp32 in numpy's order: the same integers
    assert not np.array_equal(R.gram_last_ktile_dropped(X), ref), "a dropped last K-tile would pass"
    assert not np.array_equal(R.gram_edge_tile_shifted(X), ref), "an edge tile written one row down would pass"


def test_gram_cases_cover_what_the_issue_lists():
    assert {n for n, d in R.GRAM_CASES if d == 17} == set(R.GRAM_N) == {n for n, d in R.GRAM_CASES if d == 96}
    assert {d for n, d in R.GRAM_CASES if n == 65} == set(R.GRAM_DIM)


def test_gram_bound_holds_for_fp32_in_another_order_and_rejects_a_dropped_term():
    X = np.random.default_rng(5).standard_normal((130, 100)).astype(np.float32)
    ref = -2.0 * (X.astype(np.float64) @ X.astype(np.float64).T)
    bound = R.gram_bound(X)
    acc = np.zeros((130, 130), np.float32)
    for d in range(100):                                               # sequential fp32 accumulation, the kernel's order
        acc += X[:, d:d + 1] * X[:, d:d + 1].T
    assert (np.abs((np.float32(-2.0) * acc).astype(np.float64) - ref) <= bound).all()
    assert (np.abs((np.float32(-2.0) * (X @ X.T)).astype(np.float64) - ref) <= bound).all()
    assert not (np.abs(R.gram_last_ktile_dropped(X) - ref) <= bound).all()
    assert not (np.abs(-2.0 * (X.astype(np.float16).astype(np.float64) @ X.astype(np.float16).astype(np.float64).T) - ref) <= bound).all()


@pytest.mark.parametrize("exclude", [True, False])
def test_stats_case_holds_what_it_claims_and_rejects_descending_ties(exclude):
    X, vid, id2class, lonely = R.stats_case()
    assert X.shape == (130, 17) and len(np.unique(vid)) == 12
    cls = np.array([id2class.get(int(v), 0) for v in vid])
    assert set(cls[cls >= 0]) == {0, 1, 2, 3} and (cls < 0).sum() >= 2
    assert len(set(int(v) for v in vid) - set(id2class)) == 2                                  # ids absent from the map
    dup = [(i, j) for i in range(130) for j in range(i + 1, 130) if np.array_equal(X[i], X[j])]
    assert len(dup) >= 10 and all(vid[i] != vid[j] and cls[i] != cls[j] for i, j in dup)
    ap = R.stats_query_ap(X, vid, id2class, exclude)
    assert ap[lonely] == 0.0 and cls[lonely] == 3 and (cls == 3).sum() == 1
    assert np.isnan(ap[cls < 0]).all() and not np.isnan(ap[cls >= 0]).any()
    ref = R.stats_ref(X, vid, id2class, exclude)
    wrong = R.stats_ref(X, vid, id2class, exclude, descending_ties=True)
    assert all(R.within_one_ulp(np.float32(ref[k]), ref[k]) for k in R.STAT_KEYS)              # the double figure cast once passes
    assert any(not R.within_one_ulp(np.float32(wrong[k]), ref[k]) for k in R.STAT_KEYS), "ties by descending index would pass"


def test_descending_tie_model_is_the_same_ranking_without_ties():
    # on distinct distances the reversed-order model IS the reference: what it changes is the tie rule and nothing else
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 9)).astype(np.float32)
    vid = rng.integers(0, 6, 40).astype(np.int32)
    id2class = {v: v % 3 for v in range(6)}
    from tests.class_stats_ref import class_stats, distances
    d = distances(X)
    a = class_stats(d, vid, id2class, True)[0]
    b = class_stats(d[::-1, ::-1], vid[::-1], id2class, True)[0]
    assert all(abs(a[k] - b[k]) <= 1e-12 for k in R.STAT_KEYS)


def test_one_ulp_comparison():
    ref = 0.7833333333333333
    g = np.float32(ref)
    up, down = np.nextafter(g, np.float32(1)), np.nextafter(g, np.float32(0))
    assert R.within_one_ulp(g, ref) and (R.within_one_ulp(up, ref) or R.within_one_ulp(down, ref))      # the neighbour on ref's side
    assert not R.within_one_ulp(np.nextafter(up, np.float32(1)), ref) and not R.within_one_ulp(np.nextafter(down, np.float32(0)), ref)
    assert not R.within_one_ulp(np.float32(ref + 1e-4), ref)
