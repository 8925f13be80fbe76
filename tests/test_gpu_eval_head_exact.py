"""The evaluation head, element for element against float64: the average_for_test window mean (k_mean_rows), the in-place L2
normalisation (k_row_normalize), the distance matrix (k_gram, through vv_op_gram) and the statistics vv_retrieval_stats ranks from it.

tests/test_gpu_testbranch.py bounds a norm over a whole batch and three aggregate figures to 2e-4 .. 5e-3, in f16, at F in {512, 4096},
k = 4 uniform, dim = 96.  That cannot see one wrong column of a mean row, a dropped last window slot, truncation instead of
round-to-nearest-even into the 16-bit scratch row, a Gram edge tile written one row off or an mAP that moves in its fourth digit.  Here,
as in tests/test_gpu_gemm_exact.py, the operands are chosen so that every value on the path is exactly representable
(tests/eval_head_ref.py asserts that on the CPU, and tests/test_eval_head_ref_host.py that each of those wrong kernels would be caught),
and the comparison is np.array_equal.  The two exceptions are derived, not measured:

  k_row_normalize   |got - ref| <= 4.5 x 2^-24 |ref|: sqrt, add, reciprocal, product, each correctly rounded, plus second-order terms
  k_gram, arbitrary |got - ref| <= (dim + 2) 2^-24 x 2 sum_d |x_id x_jd|: the dot-product bound plus the product with alpha

and the three statistics are held to one fp32 ulp of the float64 figure (the product sums in double and casts once).

  k_mean_rows       f16 and bf16; F = D in {100, 320} (Fp 256 and 512: F = 320 runs the column loop's second pass and has padded columns)
                    and D = 64 < F = 320; k in {1, 2, 4} uniform, k in {4, 7} with distinct dyadic coefficients; n in {1, 37, 257}; the
                    table's first and last row, one row in every slot, an all-zero window; ties of the 16-bit rounding in both directions;
                    the f16 range scale; the scratch region grown past its first capacity (n = 5, 1100, 3 on one engine)
  k_row_normalize   D in {63, 64, 65, 250, 320} x n in {1, 3, 4, 5, 37}, behind vv_embed and vv_embed_mean, an all-zero row among them
  k_gram            n in {1, 2, 63, 64, 65, 130} x dim in {17, 96} and dim in {1, 15, 16, 100} at n = 65; standard-normal 130 x 100
  vv_retrieval_stats  n = 130, dim = 17 and n = 2, exclude_same_video on and off
"""
import numpy as np
import pytest

from tests import eval_head_ref as R
from tests.test_gpu_gemm_exact import assert_exact
from tests.test_gpu_parity import vv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PRECS = R.PRECS
SENTINEL = np.float32(-12345.0)          # no value of these operands
FWD_TILE = 128                           # rows of the forward GEMM's smallest tile: what assert_exact reports a mismatch in


@pytest.fixture(scope="module")
def engines(vv):  # noqa: F811
    """engines(prec, D, F, scale) -> (engine, table): table of tests/eval_head_ref.py behind the identity layer; one engine per key for
    the whole module, closed at its end."""
    made = {}

    def get(prec, D, F, scale=1.0):
        key = (prec, D, F, scale)
        if key not in made:
            T = R.table(F, scale)
            W, b = R.identity_layer(D, F, prec)
            eng = vv.Engine(0, prec)
            eng.table_set(T)
            eng.params_set(W, b)
            made[key] = (eng, T)
            assert np.array_equal(eng.table_get(n=R.N_ROWS), T), "vv_table_get does not return the table (%s, F %d, scale %g)" % (prec, F, scale)
        return made[key]

    yield get
    for eng, _ in made.values():
        eng.close()


@pytest.fixture(scope="module")
def gram_engine(vv):  # noqa: F811
    eng = vv.Engine(0, "f16")
    yield eng
    eng.close()


# ------------------------------------------------------------------------------- 1. k_mean_rows through an identity layer
MEAN_SHAPES = [(100, 100), (320, 320), (64, 320)]                                         # (D, F)
MEAN_COEFF = [(1, "uniform"), (2, "uniform"), (4, "uniform"), (4, "distinct"), (7, "distinct")]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 37, 257])
@pytest.mark.parametrize("k,kind", MEAN_COEFF)
@pytest.mark.parametrize("D,F", MEAN_SHAPES)
def test_mean_rows_exact(engines, prec, D, F, k, kind, n):
    eng, T = engines(prec, D, F)
    rows, coeff = R.window_rows(n, k), R.coefficients(k, kind)
    ref = R.mean_ref(T, rows, coeff, prec, D)
    got = eng.embed_mean(rows, coeff, relu=False, l2norm=False)
    assert_exact(got, ref, "window mean (%s, D %d, F %d, k %d %s, n %d)" % (prec, D, F, k, kind, n), FWD_TILE)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("F", [100, 320])
def test_mean_rows_round_to_nearest_even(engines, prec, F):
    """coeff = [1, 2^-p]: x0 + x1 2^-p is exact in fp32 and, for x0 in {2, 3} and odd x1, exactly half-way between two 16-bit values."""
    eng, T = engines(prec, F, F)
    rows, coeff = R.window_rows(257, 2), R.coefficients(2, "tie", prec)
    down, up = R.tie_inventory(T, rows, prec)
    assert down.any() and up.any(), "the input holds no tie in one direction"
    m = R.mean64(T, rows, coeff)
    ref = R.mean_ref(T, rows, coeff, prec, F)
    assert not np.array_equal(R.truncate_rows(m, prec)[up], ref[up]), "truncation would pass: the case proves nothing"
    got = eng.embed_mean(rows, coeff, relu=False, l2norm=False)
    assert_exact(got, ref, "window mean at the ties of the 16-bit rounding (%s, F %d)" % (prec, F), FWD_TILE)


def test_mean_rows_under_the_f16_range_scale(engines):
    """The same table times 2^16: max |x| leaves f16's range, the table takes a power-of-two scale (the fixture asserts that vv_table_get
    still returns it exactly); the uniform mean of four rows is exact in 16 bits at that scale, so the fp32 output is the float64 mean."""
    D = F = 100
    eng, T = engines("f16", D, F, R.RANGE_SCALE)
    assert T.max() == 3 * R.RANGE_SCALE
    rows = R.window_rows(37, 4)
    ref = R.mean_ref(T, rows, None, "f16", D, sx=R.RANGE_SX)
    assert np.array_equal(ref, R.mean64(T, rows, None)[:, :D])
    got = eng.embed_mean(rows, None, relu=False, l2norm=False)
    assert_exact(got, ref, "window mean under the range scale (f16, F %d)" % F, FWD_TILE)


@pytest.mark.parametrize("prec", PRECS)
def test_scratch_region_grows_and_keeps_the_table(vv, prec):  # noqa: F811
    """n = 5 allocates the scratch rows behind the table (1024 of them), n = 1100 does not fit: the table moves to a larger allocation."""
    D = F = 320
    T = R.table(F)
    W, b = R.identity_layer(D, F, prec)
    eng = vv.Engine(0, prec)
    try:
        eng.table_set(T)
        eng.params_set(W, b)
        for n in (5, 1100, 3):
            rows = R.window_rows(n, 4)
            got = eng.embed_mean(rows, None, relu=False, l2norm=False)
            assert_exact(got, R.mean_ref(T, rows, None, prec, D), "window mean (%s, n %d) around the scratch region's growth" % (prec, n), FWD_TILE)
        assert np.array_equal(eng.table_get(n=R.N_ROWS), T), "the table changed when the scratch region grew"
        idx = np.array([-1, 0, -1, R.N_ROWS - 1], np.int32)
        out = eng.dev(np.full((len(idx), F), SENTINEL, np.float32))
        try:
            eng.op("gather_rows", idx, len(idx), out)
            g = out.get()
        finally:
            out.free()
        assert not g[[0, 2]].any(), "an empty slot (-1) no longer reads the all-zero row"
        assert np.array_equal(g[[1, 3]], T[[0, R.N_ROWS - 1]])
        rows = np.array([0, R.N_ROWS - 1, 17, R.ZERO_ROWS[0], 17], np.int32)
        assert_exact(eng.embed(rows, relu=False, l2norm=False), T[rows][:, :D].astype(np.float64), "vv_embed after the growth (%s)" % prec, FWD_TILE)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 2. k_row_normalize
def check_normalized(call, e_ref, zero_row, what):
    """call(l2norm) -> [n][D].  The un-normalised output is exact; the normalised one is inside the derived bound, keeps an all-zero row
    exactly zero and comes out with the same bits twice."""
    assert_exact(call(False), e_ref, what + ", before the normalisation", FWD_TILE)
    ref = R.normalize_ref(e_ref)
    got, again = call(True), call(True)
    assert got.tobytes() == again.tobytes(), what + ": two calls on the same input differ"
    assert not np.isnan(got).any(), what + ": NaN"
    if zero_row is not None:
        assert not e_ref[zero_row].any() and not got[zero_row].any(), what + ": the all-zero row did not stay zero"
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.where(ref != 0, np.abs(ref), 1.0)).max() / R.U)
    print("%s: max |got - ref| / |ref| = %.3f x 2^-24" % (what, worst))
    assert R.within_normalize_bound(got, ref), "%s: %.3f x 2^-24 relative, the bound is 4.5" % (what, worst)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 37])
@pytest.mark.parametrize("D", [63, 64, 65, 250, 320])
def test_row_normalize_within_four_roundings(engines, prec, D, n):
    F = 320
    eng, T = engines(prec, D, F)
    rows = R.norm_rows(n)
    e_ref = np.maximum(T[rows][:, :D].astype(np.float64), 0.0)
    check_normalized(lambda l2: eng.embed(rows, relu=True, l2norm=l2), e_ref, 1 if n >= 3 else None,
                     "vv_embed (%s, D %d, n %d)" % (prec, D, n))
    win = R.window_rows(n, 4)
    m_ref = np.maximum(R.mean_ref(T, win, None, prec, D), 0.0)
    check_normalized(lambda l2: eng.embed_mean(win, None, relu=True, l2norm=l2), m_ref, 2 if n >= 3 else None,
                     "vv_embed_mean (%s, D %d, n %d)" % (prec, D, n))


# ------------------------------------------------------------------------------- 3. k_gram as an operator
def run_gram(eng, X, alpha):
    n, dim = X.shape
    Xd = eng.dev(X)
    Od = eng.dev(np.full(n * n + 256, SENTINEL, np.float32))
    try:
        eng.op("gram", Xd, n, dim, alpha, Od)
        o = Od.get()
    finally:
        Xd.free(); Od.free()
    assert np.array_equal(o[n * n:], np.full(256, SENTINEL, np.float32)), "elements past n x n were written"
    G = o[:n * n].reshape(n, n)
    assert G.tobytes() == np.ascontiguousarray(G.T).tobytes(), "the Gram matrix is not bit-symmetric"
    return G


@pytest.mark.parametrize("n,dim", R.GRAM_CASES)
def test_gram_exact(gram_engine, n, dim):
    X = R.gram_operand(n, dim)
    ref = R.gram_ref(X)
    assert_exact(run_gram(gram_engine, X, -2.0), ref, "-2 X X^T (n %d, dim %d)" % (n, dim), 64, 64)


def test_gram_arbitrary_values_within_the_dot_product_bound(gram_engine):
    X = np.random.default_rng(5).standard_normal((130, 100)).astype(np.float32)
    ref = -2.0 * (X.astype(np.float64) @ X.astype(np.float64).T)
    got = run_gram(gram_engine, X, -2.0)
    err, bound = np.abs(got.astype(np.float64) - ref), R.gram_bound(X)
    print("k_gram 130 x 100: max error / bound = %.4f" % float((err / bound).max()))
    assert (err <= bound).all()


def test_gram_argument_checks(vv, gram_engine):  # noqa: F811
    Xd, Od = gram_engine.dev(np.ones((2, 3), np.float32)), gram_engine.dev(np.full(4, SENTINEL, np.float32))
    try:
        for n, dim in ((0, 3), (2, 0), (-1, 3)):
            with pytest.raises(vv.VVError, match="videovec error 1: vv_op_gram"):          # VV_ERR_ARG
                gram_engine.op("gram", Xd, n, dim, -2.0, Od)
        with pytest.raises(vv.VVError, match="videovec error 1: vv_op_gram"):
            gram_engine.op("gram", None, 2, 3, -2.0, Od)
        assert np.array_equal(Od.get(), np.full(4, SENTINEL, np.float32))
    finally:
        Xd.free(); Od.free()


# ------------------------------------------------------------------------------- 4. vv_retrieval_stats, per statistic
def check_stats(got, ref, what):
    for g, k in zip(got, R.STAT_KEYS):
        print("%s %s: got %.9g, float64 %.17g" % (what, k, g, ref[k]))
    for g, k in zip(got, R.STAT_KEYS):
        assert R.within_one_ulp(g, ref[k]), "%s: %s = %.9g, the float64 figure is %.17g" % (what, k, g, ref[k])


@pytest.mark.parametrize("exclude", [True, False])
def test_retrieval_stats_each_figure_to_one_ulp(gram_engine, exclude):
    X, vid, id2class, lonely = R.stats_case()
    ref = R.stats_ref(X, vid, id2class, exclude)
    assert R.stats_query_ap(X, vid, id2class, exclude)[lonely] == 0.0          # a scored query without any positive
    wrong = R.stats_ref(X, vid, id2class, exclude, descending_ties=True)
    assert any(not R.within_one_ulp(np.float32(wrong[k]), ref[k]) for k in R.STAT_KEYS), "the tie rule decides nothing here"
    got = gram_engine.retrieval_stats(X, vid, id2class, exclude)
    check_stats(got, ref, "retrieval_stats (n %d, exclude %s)" % (len(X), exclude))


@pytest.mark.parametrize("exclude", [True, False])
def test_retrieval_stats_smallest_call(gram_engine, exclude):
    X = R.gram_operand(2, 17)
    vid, id2class = np.array([10, 13], np.int32), {10: 1, 13: 1}
    ref = R.stats_ref(X, vid, id2class, exclude)
    assert ref == dict(mean_ap=1.0, hit_at_1=1.0, hit_at_5=0.2)
    check_stats(gram_engine.retrieval_stats(X, vid, id2class, exclude), ref, "retrieval_stats (n 2, exclude %s)" % exclude)
