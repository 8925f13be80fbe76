"""The parameter update, element by element against float64, in each of its five forms -- and the 16-bit weight copy it leaves behind.

Five kernels own the fp32 master weights, the history, the bias and the 16-bit copy every later forward pass reads: k_sgd with 16-byte
accesses (form 1) and scalar (form 2, F % 4 != 0), k_reduce_sgd (3), k_reduce_sgd over f16 slabs (4) and the epilogue of the
weight-gradient GEMM (5).  The other tests bound a Frobenius norm at one shape where every thread has one element, or compare the forms
with each other -- all of which call the same SolverRule::step.  Here the reference is that rule restated in numpy float64 (step64), every
case asserts the form it ran ("last_update_form", and "last_wgrad_splits" where the form depends on it) and no element is exempt.  This
file holds no copy of the dispatch rules: a shape that lands in another form fails its assertion and has to move.

EXACT cases (k_sgd, forms 1 and 2; SGD and Nesterov, L1 and L2).  The per-layer operators give the test the gradient: with X the F x F
identity, vv_op_inner_product_bwd makes dW[d, f] = dY[f, d] and db an integer column sum, asserted with np.array_equal before the update.
All inputs are dyadic: W integers -512 .. 512 times 2^-8 (5 % exact zeros, some -0.0), histories and bias integers -256 .. 256 times 2^-8,
dY integers -2 .. 2, lr 2^-3, momentum 0.5, weight_decay 2^-4, lr_mult (0.5, 2), decay_mult (2, 0.5).  Then every intermediate of the rule
-- dc r, g + dc r, lr g', momentum h, their sum, Nesterov's combination, w - u -- is exactly representable in fp32.  step64 asserts that on
the CPU for each of them (a failure there is a wrong input, not a wrong kernel), so whether the compiler contracts a product and a sum
into an fma or not cannot change a bit, and the comparison is np.array_equal on W, hW, b, hb.  After an exact update W has left the 2^-8
grid, so every exact update starts from fresh dyadic state (vv_params_set).

BOUNDED cases (every form behind a real vv_forward_backward; SGD, Nesterov, AdaGrad).  The test cannot choose that gradient, so the
reference takes the GPU's own fp32 gradient (read back AFTER the update: asking before it would turn the step into the two-launch form;
form 5 never materialises it, a twin engine with wgrad_update = 0 provides it and must end with bit-equal parameters) and applies the
float64 rule to the fp32 (w, h, g).  Bound per element: n x 2^-24 x M (+ n x 2^-126 for an underflow), where M is the sum of the absolute
values of every term of the expanded rule in float64 and n counts the rule's fp32 operations, uncontracted (the Makefile sets no fast-math
flag: add, mul, fma, div and sqrt are correctly rounded, |delta| <= u = 2^-24 each; an fma only removes a rounding).  With G = |g| + |dc||r|:
  SGD       dc*r, g + ., lr * ., momentum * h, + (-> h'), w - h'                                  n = 6
            M(h') = lr G + momentum |h|,  M(w') = |w| + M(h').  The deepest term (dc r) passes 5 roundings: (1 + u)^5 - 1 < 6 u.
  Nesterov  SGD's five to h', then 1 + momentum, * h', momentum * h0, -, w - u                     n = 10
            M(w') = |w| + (1 + momentum) M(h') + momentum |h0|; deepest term 8 roundings (the rounded coefficient 1 + momentum included).
  AdaGrad   dc*r, g + . (-> g'), g' * g', h + . (-> h'), sqrt, + delta, g' / ., lr * ., w - .       9 operations, n = 11
            g' enters the quotient twice -- as the numerator and, squared, under the root -- so its two roundings count twice: to first
            order |err h'| <= (4 G^2 + G^2 + (h + G^2)) u <= 6 u M(h'), M(h') = h + G^2, and with d = sqrt(h') + delta
            |err w'| <= u |w| + 10 u lr G / d <= 11 u M(w'), M(w') = |w| + lr G / d.  (G, not |g'|: a cancellation in g + dc r does not
            shrink the error it carries.)
The count is derived, not measured.  A skipped element is off by about lr |g|, orders of magnitude above this; every case also asserts
that more than 99 % of the weights moved.  Two consecutive updates per case with a forward_backward between them.

THE 16-BIT COPY after every update above is read as a forward pass reads it: vv_op_inner_product with the F x F identity returns
Y[f, d] = fl32(q[d, f] + b[d]) -- one product per output, power-of-two scales, one rounding -- and q must be the round-to-nearest-even of
the new fp32 W (read back from the GPU) to f16 at the power-of-two scale half_scale() derives from max |W| BEFORE that update (after
vv_params_set its seed counts in the next fold as well: the second update's scale comes from max(max |W0|, max |W1|)), or to bf16 with no
scale.  Elements with 0 < |w| < 2^-20 max |w| are left out (below f16's normal range the value depends on which admissible scale was
used) and must be fewer than 1e-5 of all; the dyadic cases have none.  The exact cases land on multiples of 2^-16 with 11-bit (8-bit)
targets: the test asserts on the CPU that exact ties occur, so ties-to-even is really tested.  One case drives max |W| across a power of
two in its first update and lets a second follow: both copies must be the exact rounding (the one-update lag of Scales::sw_next).
After the D = 130 and the 4090 x 4092 cases an inner product with features in every column must equal the float64 product with q
(nothing non-finite was written into the padding a K-tile reads): dense integer features at 130 x 256, where the dyadic q keeps every
fp32 partial sum exact (asserted on the CPU); at 4090 x 4092 q is not dyadic and no fp32 sum of two products is exact in general, so
the rows there carry ONE feature 1 .. 3 each, in a permuted order that covers every column.
"""
import numpy as np
import pytest

from tests.test_gpu_gemm_exact import features
from tests.test_gpu_parity import vv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PRECS = ["f16", "bf16"]
U = 2.0 ** -24
SOLVER = {"SGD": 0, "NESTEROV": 1, "ADAGRAD": 2}
N_OPS = {0: 6, 1: 10, 2: 11}             # the docstring's derivation
SGD_GRID = 1024                          # k_sgd's workgroups, for the failure report only (which pass of the grid-stride loop)
FORM_NAME = {1: "k_sgd 16-byte", 2: "k_sgd scalar", 3: "k_reduce_sgd", 4: "k_reduce_sgd over f16 slabs", 5: "weight-gradient epilogue"}


# ------------------------------------------------------------------------------- the rule in float64
def f32(x):
    return np.float64(np.float32(x))


def survives_f32(x, what):
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x), "%s is not exact in fp32: the inputs are wrong" % what


def step64(w, h, g, lr, dc, mom, reg, solver, delta=0.0, exact=False):
    """SolverRule::step (solver.cpp:502-531, 599-655, 714-781; blob.cpp:118-120) in float64 -> w', h', M(w'), M(h').
    exact: assert that every intermediate is representable in fp32."""
    w, h, g = (np.asarray(a, np.float64) for a in (w, h, g))
    chk = survives_f32 if exact else (lambda x, what: None)
    G = np.abs(g)
    if dc != 0.0:
        r = w if reg == 2 else np.sign(w)
        t = dc * r; chk(t, "dc * r")
        g = g + t; chk(g, "g + dc * r")
        G = G + abs(dc) * np.abs(r)
    if solver == 2:
        hn = h + g * g
        den = np.sqrt(hn) + delta
        u = lr * (g / den)
        Mh = np.abs(h) + G * G
        Mw = np.abs(w) + lr * G / den
    else:
        a = lr * g; chk(a, "lr * g'")
        m = mom * h; chk(m, "momentum * h")
        hn = a + m; chk(hn, "lr * g' + momentum * h")
        Mh = lr * G + mom * np.abs(h)
        if solver == 1:
            u = (1.0 + mom) * hn - m; chk((1.0 + mom) * hn, "(1 + momentum) * h'"); chk(u, "Nesterov's combination")
            Mw = np.abs(w) + (1.0 + mom) * Mh + mom * np.abs(h)
        else:
            u = hn
            Mw = np.abs(w) + Mh
    wn = w - u; chk(wn, "w - u")
    return wn, hn, Mw, Mh


class Rule:
    """The solver's settings as the kernels see them: fp32 values, held in float64."""

    def __init__(self, solver, reg, lr, mom, wd, delta=0.0):
        self.solver, self.reg, self.name = SOLVER[solver], {"L1": 1, "L2": 2}[reg], "%s/%s/wd %g" % (solver, reg, wd)
        self.lr, self.mom, self.wd, self.delta = f32(lr), f32(mom), f32(wd), f32(delta)
        self.kw = dict(lr=lr, momentum=mom, weight_decay=wd, solver_type=solver, reg=reg, delta=delta, lr_mult=(0.5, 2), decay_mult=(2, 0.5))

    def cfg(self, vv, B=1, C=2, Nn=1):  # noqa: F811
        return vv.StepConfig(B, C, Nn, **self.kw)

    def weights(self, w, h, g, exact=False):
        return step64(w, h, g, self.lr * 0.5, self.wd * 2.0, self.mom, self.reg, self.solver, self.delta, exact)

    def bias(self, w, h, g, exact=False):
        return step64(w, h, g, self.lr * 2.0, self.wd * 0.5, self.mom, self.reg, self.solver, self.delta, exact)


# ------------------------------------------------------------------------------- comparisons
def assert_same(got, ref64, what, per=1):
    """np.array_equal against the float64 reference (itself exact in fp32); reports the first differing element and its pass."""
    survives_f32(ref64, what)
    if np.array_equal(got, ref64):
        return
    g2, r2 = np.atleast_2d(got), np.atleast_2d(ref64)
    bad = np.argwhere(~(g2 == r2))
    d, f = (int(v) for v in bad[0])
    flat = d * g2.shape[1] + f
    msg = ("%s: %d of %d elements differ; first at (d %d, f %d), flat index %d = pass %d of a %d-workgroup grid-stride loop over %d-element "
           "items: got %r, expected %r" % (what, len(bad), r2.size, d, f, flat, flat // per // (256 * SGD_GRID), SGD_GRID, per,
                                           float(g2[d, f]), float(r2[d, f])))
    print(msg)
    pytest.fail(msg)


def assert_bounded(got, ref64, M, n, what):
    err = np.abs(got.astype(np.float64) - ref64)
    bound = n * (U * M + 2.0 ** -126)
    worst = float((err / bound).max())
    print("%s: largest error / bound = %.3f (n = %d)" % (what, worst, n))
    if worst <= 1.0:
        return
    g2, e2, b2, r2 = (np.atleast_2d(a) for a in (got, err, bound, ref64))
    bad = np.argwhere(e2 > b2)
    d, f = (int(v) for v in bad[0])
    msg = ("%s: %d of %d elements beyond %d x 2^-24 x M; first at (d %d, f %d): got %r, float64 rule %r, error %.3e, bound %.3e; worst "
           "error / bound %.3g" % (what, len(bad), r2.size, n, d, f, float(g2[d, f]), float(r2[d, f]), float(e2[d, f]), float(b2[d, f]), worst))
    print(msg)
    pytest.fail(msg)


def half_scale(m, prec):
    """vv_internal.h: half_scale -- f16 places the largest magnitude in [2^11, 2^12); bf16 needs none"""
    return 2.0 ** (12 - int(np.frexp(np.float32(m))[1])) if prec == "f16" and m > 0 else 1.0


def copy_of(W, m, prec):
    """The 16-bit copy of W as a forward pass reads it: round-to-nearest-even at the scale of the maximum m."""
    W = np.asarray(W, np.float32)
    if prec == "f16":
        s = np.float32(half_scale(m, prec))
        return ((W * s).astype(np.float16).astype(np.float32) / s).astype(np.float32)
    u = W.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def rounding_census(W, m, prec):
    """(fraction of the elements the copy has to round, number of exact ties among them)"""
    x = W.astype(np.float64) * half_scale(m, prec)
    q = copy_of(W, m, prec).astype(np.float64) * half_scale(m, prec)
    ulp = 2.0 ** (np.frexp(x)[1] - (11 if prec == "f16" else 8))          # x = f 2^e, f in [0.5, 1): 11 (8) significant bits
    return float((q != x).mean()), int(((x != 0) & (np.abs(x - q) == 0.5 * ulp)).sum())


class CopyReader:
    """Reads the 16-bit copy through vv_op_inner_product with the F x F identity (allocated once per engine)."""

    def __init__(self, eng, D, F):
        self.eng, self.D, self.F = eng, D, F
        self.I = eng.dev(np.eye(F, dtype=np.float32))
        self.Y = eng.dev((F, D))

    def read(self):
        self.eng.op("inner_product", self.I, self.F, self.Y)
        return self.Y.get().T                     # [D][F]: fl32(q[d, f] + b[d])

    def check(self, W_new, b_new, m_before, prec, what):
        got = self.read()
        q = copy_of(W_new, m_before, prec)
        exp = (q.astype(np.float64) + b_new.astype(np.float64)[:, None]).astype(np.float32)
        a = np.abs(W_new)
        tiny = (a > 0) & (a < 2.0 ** -20 * a.max())
        assert tiny.sum() < 1e-5 * tiny.size, "%s: %d elements below 2^-20 max |w|" % (what, int(tiny.sum()))
        ok = (got == exp) | tiny
        if not ok.all():
            bad = np.argwhere(~ok)
            d, f = (int(v) for v in bad[0])
            msg = ("%s: the 16-bit copy differs in %d of %d elements; first at (d %d, f %d): w %r, scale of max %r, read %r, expected "
                   "fl32(%r + %r) = %r" % (what, len(bad), ok.size, d, f, float(W_new[d, f]), float(m_before), float(got[d, f]), float(q[d, f]),
                                           float(b_new[d]), float(exp[d, f])))
            print(msg)
            pytest.fail(msg)
        return q

    def free(self):
        self.I.free(); self.Y.free()


def check_dense_product(eng, X, q, b, what):
    """vv_op_inner_product of X against the float64 product with the copy q; the caller has made that product exact in fp32."""
    R, D = len(X), len(b)
    acc = X.astype(np.float64) @ q.astype(np.float64).T
    exp = (acc + b.astype(np.float64)).astype(np.float32)
    Xd, Yd = eng.dev(X), eng.dev((R, D))
    try:
        eng.op("inner_product", Xd, R, Yd)
        y = Yd.get()
    finally:
        Xd.free(); Yd.free()
    assert np.isfinite(y).all(), what + ": non-finite outputs (something in the padding of the 16-bit copy?)"
    if not np.array_equal(y, exp):
        bad = np.argwhere(~(y == exp))
        r, d = (int(v) for v in bad[0])
        pytest.fail("%s: %d of %d outputs differ from the float64 product with the copy; first at (row %d, d %d): got %r, expected %r"
                    % (what, len(bad), exp.size, r, d, float(y[r, d]), float(exp[r, d])))


# ------------------------------------------------------------------------------- exact cases: k_sgd through the operator route
def dyadic_state(D, F, seed):
    rng = np.random.default_rng(seed)
    W = (rng.integers(-512, 513, size=(D, F)) / 256.0).astype(np.float32)
    z = rng.random((D, F))
    W[z < 0.05] = 0.0
    W[z < 0.002] = -0.0
    W[0, 0], W[D - 1, F - 1] = 2.0, -2.0                   # the extremes, at the first and the last element
    hW = (rng.integers(-256, 257, size=(D, F)) / 256.0).astype(np.float32)
    b = (rng.integers(-256, 257, size=D) / 256.0).astype(np.float32)
    hb = (rng.integers(-256, 257, size=D) / 256.0).astype(np.float32)
    assert (W == 0).mean() > 0.04 and np.signbit(W[W == 0]).any() and not np.signbit(W[W == 0]).all()
    return W, b, hW, hb


def operator_gradient(eng, reader, dYd, dY, F):
    """X = identity: dW[d, f] = dY[f, d], db its integer column sums -- asserted, so a failure here is not the update's."""
    eng.op("inner_product", reader.I, F, reader.Y)
    eng.op("inner_product_bwd", dYd, F, 0.0)
    dW, db = eng.grads()
    assert np.array_equal(dW, dY.T), "dW of the operator route is not dY^T: an input or GEMM problem, not an update problem"
    assert np.array_equal(db, dY.sum(0)), "db of the operator route is not the column sum"
    return dW, db


# (D, F, form): 258 x 1021 -- 263 418 elements, 1274 more than the scalar form's 262 144 threads (its loop wraps), F % 4 = 1, D > 256 (the
# bias loop leaves workgroup 0); 30 x 101 -- most workgroups idle, their maxima must read 0; 516 x 2052 -- 264 708 16-byte items, a second
# pass, F / 4 = 513 odd (row boundaries inside a wave); 130 x 256 -- no wrap, D % 4 = 2.
EXACT_SHAPES = [(258, 1021, 2), (30, 101, 2), (516, 2052, 1), (130, 256, 1)]
EXACT_RULES = [("SGD", "L2", 2.0 ** -4), ("SGD", "L1", 2.0 ** -4), ("NESTEROV", "L2", 2.0 ** -4), ("NESTEROV", "L1", 2.0 ** -4),
               ("SGD", "L2", 0.0)]                         # (weight_decay 0: the rule's dc != 0 branch not taken)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("D,F,form", EXACT_SHAPES)
def test_k_sgd_exact_element_by_element(vv, prec, D, F, form):  # noqa: F811
    eng = vv.Engine(0, prec)
    assert eng.get_option("last_update_form") == 0
    eng.set_option("fuse_update", 0)                       # (the operator route reduces eagerly anyway)
    eng.table_set(np.ones((1, F), np.float32))             # defines F; scale 1
    dY = np.random.default_rng(D + F).integers(-2, 3, size=(F, D)).astype(np.float32)
    reader = dYd = None
    try:
        for k, (solver, reg, wd) in enumerate(EXACT_RULES):
            rule = Rule(solver, reg, 2.0 ** -3, 0.5, wd)
            what = "%s, %d x %d, %s" % (prec, D, F, rule.name)
            W, b, hW, hb = dyadic_state(D, F, 1000 * k + D)
            eng.params_set(W, b, hW, hb)
            if reader is None:
                reader, dYd = CopyReader(eng, D, F), eng.dev(dY)
            dW, db = operator_gradient(eng, reader, dYd, dY, F)
            Wr, hWr, _, _ = rule.weights(W, hW, dW, exact=True)
            br, hbr, _, _ = rule.bias(b, hb, db, exact=True)
            eng.apply_update(rule.cfg(vv))
            got_form = int(eng.get_option("last_update_form"))
            assert got_form == form, "%s ran form %d (%s), the case is written for %d: move the shape" % (what, got_form, FORM_NAME.get(got_form), form)
            Wg, bg, hWg, hbg = eng.params_get()
            per = 4 if form == 1 else 1
            assert_same(Wg, Wr, "W after " + what, per)
            assert_same(hWg, hWr, "hW after " + what, per)
            assert_same(bg, br, "b after " + what)
            assert_same(hbg, hbr, "hb after " + what)
            assert (Wg != W).mean() > 0.99
            m0 = float(np.abs(W).max())
            frac, ties = rounding_census(Wg, m0, prec)
            print("%s: the copy rounds %.1f %% of the elements, %d exact ties" % (what, 100 * frac, ties))
            if reg == "L2" and wd != 0:                    # (these land on the 2^-15 / 2^-16 grid; L1 and no decay stay on a coarser one)
                assert frac > 0.01 and ties > 0, "the copy's rounding and its ties are not exercised: the inputs are wrong"
                assert prec != "f16" or frac < 0.90
            q = reader.check(Wg, bg, m0, prec, what)
            if D == 130 and k == 0:
                # dense integer features (0 .. 3, every column used): q is a multiple of 2^-15 here (plain SGD), every partial sum an integer
                # count of such units below 2^24 -- exact in fp32 in any order (asserted), so the product must equal float64's
                X = features(77, 300, F)
                assert (X != 0).any(0).all()
                units = q.astype(np.float64) * 2.0 ** 15
                assert np.array_equal(units, np.rint(units)) and (X.astype(np.float64) @ np.abs(units).T).max() < 2 ** 24
                check_dense_product(eng, X, q, bg, "dense product after " + what)
    finally:
        if reader is not None:
            reader.free(); dYd.free()
        eng.close()


@pytest.mark.parametrize("D,F,form", [(130, 256, 1), (30, 101, 2)])
def test_copy_scale_lags_one_update_across_a_binade(vv, D, F, form):  # noqa: F811
    """f16.  max |W0| = 2; SGD with lr_w = 1 and integer gradients takes max |W1| beyond 4: the first copy is still written at the scale
    of [2, 4) (Scales::sw_next as vv_params_set left it), the second -- same gradient, no vv_params_set -- at the scale of max |W1|.  Both
    updates are exact (dyadic values throughout), both copies must be the exact rounding at THEIR scale."""
    rule = Rule("SGD", "L2", 2.0, 0.5, 0.0)
    eng = vv.Engine(0, "f16")
    eng.set_option("fuse_update", 0)
    eng.table_set(np.ones((1, F), np.float32))
    W, b, hW, hb = dyadic_state(D, F, 5)
    dY = np.random.default_rng(9).integers(-2, 3, size=(F, D)).astype(np.float32)
    eng.params_set(W, b, hW, hb)
    reader, dYd = CopyReader(eng, D, F), eng.dev(dY)
    try:
        dW, db = operator_gradient(eng, reader, dYd, dY, F)
        state, maxima = (W, b, hW, hb), [float(np.abs(W).max())]
        for k in (1, 2):
            Wr, hWr, _, _ = rule.weights(state[0], state[2], dW, exact=True)
            br, hbr, _, _ = rule.bias(state[1], state[3], db, exact=True)
            eng.apply_update(rule.cfg(vv))
            assert int(eng.get_option("last_update_form")) == form
            Wg, bg, hWg, hbg = eng.params_get()
            what = "update %d across the binade (%d x %d)" % (k, D, F)
            assert_same(Wg, Wr, "W after " + what, 4 if form == 1 else 1)
            assert_same(hWg, hWr, "hW after " + what, 4 if form == 1 else 1)
            assert_same(bg, br, "b after " + what)
            assert_same(hbg, hbr, "hb after " + what)
            reader.check(Wg, bg, max(maxima), "f16", what)
            maxima.append(float(np.abs(Wg).max()))
            state = (Wg, bg, hWg, hbg)
        assert half_scale(maxima[0], "f16") > half_scale(maxima[1], "f16"), "max |W| did not cross a power of two: the inputs are wrong"
        assert half_scale(max(maxima[:2]), "f16") != half_scale(maxima[0], "f16")
    finally:
        reader.free(); dYd.free()
        eng.close()


# ------------------------------------------------------------------------------- bounded cases: every form behind a real step
# (form, D, F, splits allowed): 1028 x 2048 -- 526 336 16-byte items, more than the one-launch form's 2048 x 256 threads (its loop wraps),
# 65 bias workgroups of which the last has 4 live columns; the same shape with fuse_update = 0 for form 1; 100 x 128 -- one parameter
# workgroup in part beside 7 bias workgroups and the loss workgroup (the special workgroups' renumbering in a tiny grid); 1028 x 4096 with
# f16 slabs -- 526 336 eight-element items, that loop wraps too; 4090 x 4092 and 4096 x 4096 -- 256 tiles, one split, the update in the
# weight-gradient GEMM's epilogue, a ragged last tile row and column.
SPLITS = {1: range(1, 1 << 20), 3: range(1, 9), 4: range(2, 9), 5: range(1, 2)}
STEP_CASES = [
    (1, 1028, 2048, "f16", "SGD", "L2"), (1, 1028, 2048, "f16", "NESTEROV", "L2"), (1, 1028, 2048, "bf16", "ADAGRAD", "L2"), (1, 1028, 2048, "f16", "SGD", "L1"),
    (3, 1028, 2048, "f16", "SGD", "L2"), (3, 1028, 2048, "bf16", "NESTEROV", "L2"), (3, 1028, 2048, "f16", "ADAGRAD", "L2"), (3, 1028, 2048, "f16", "NESTEROV", "L1"),
    (3, 100, 128, "f16", "SGD", "L2"), (3, 100, 128, "bf16", "ADAGRAD", "L2"),
    (4, 1028, 4096, "f16", "SGD", "L2"), (4, 1028, 4096, "bf16", "SGD", "L2"), (4, 1028, 4096, "f16", "NESTEROV", "L2"), (4, 1028, 4096, "bf16", "ADAGRAD", "L2"),
    (4, 1028, 4096, "f16", "ADAGRAD", "L1"),
    (5, 4090, 4092, "f16", "SGD", "L2"), (5, 4090, 4092, "bf16", "NESTEROV", "L2"), (5, 4090, 4092, "f16", "ADAGRAD", "L2"), (5, 4090, 4092, "f16", "SGD", "L1"),
    (5, 4096, 4096, "f16", "SGD", "L2"),
]


def make_engine(vv, prec, form, D, F, n_rows, state):  # noqa: F811
    eng = vv.Engine(0, prec)
    eng.set_dedup(False)                                   # (an idle GPU plans a de-duplicated step from its own distinct count; dense is deterministic)
    eng.set_option("fuse_update", 0 if form == 1 else 1)
    eng.set_option("slab16", 1 if form == 4 else 0)
    eng.set_option("wgrad_update", 1)
    eng.table_synth(7, n_rows, F)
    eng.params_set(*state)
    return eng


@pytest.mark.parametrize("form,D,F,prec,solver,reg", STEP_CASES)
def test_update_within_the_rounding_bound_in_every_form(vv, form, D, F, prec, solver, reg):  # noqa: F811
    B, C, Nn, n_rows = 32, 5, 4, 3000
    rule = Rule(solver, reg, 0.05, 0.0 if solver == "ADAGRAD" else 0.9, 5e-4, 1e-6 if solver == "ADAGRAD" else 0.0)
    n = N_OPS[rule.solver]
    rng = np.random.default_rng(D + F + form)
    # (uniform, not gaussian: the density of |w| near zero decides how many elements fall below 2^-20 max |w|, about 2^-20 of them here)
    W = rng.uniform(-0.02, 0.02, size=(D, F)).astype(np.float32)
    b = (rng.standard_normal(D) * 0.01).astype(np.float32)
    if solver == "ADAGRAD":                                # (from a non-zero history, as the parity test: with h = 0 the first step is lr sign(g))
        hW, hb = np.full_like(W, 1e-4), np.full_like(b, 1e-4)
    else:
        hW, hb = (rng.standard_normal((D, F)) * 1e-4).astype(np.float32), (rng.standard_normal(D) * 1e-4).astype(np.float32)
    state = (W, b, hW, hb)
    eng = make_engine(vv, prec, form, D, F, n_rows, state)
    twin = None
    reader = CopyReader(eng, D, F)
    try:
        if form == 5:                                      # the same calls with the update as its own launch: the only holder of this gradient
            twin = make_engine(vv, prec, form, D, F, n_rows, state)
            twin.set_option("wgrad_update", 0)
        cfg = rule.cfg(vv, B, C, Nn)
        maxima = [float(np.abs(W).max())]
        for k in (1, 2):
            idx = rng.integers(0, n_rows, size=(B, C + Nn)).astype(np.int32)
            for e in (eng, twin):
                if e is not None:
                    if form == 5:
                        e.update_hint(cfg)
                    e.forward_backward(cfg, idx)
                    e.apply_update(cfg)
            got_form, S = int(eng.get_option("last_update_form")), int(eng.get_option("last_wgrad_splits"))
            what = "%s, %d x %d, %s, form %d, update %d" % (prec, D, F, rule.name, form, k)
            print("%s: ran form %d (%s) behind %d split(s)" % (what, got_form, FORM_NAME.get(got_form), S))
            assert got_form == form, "%s ran form %d (%s): move the shape" % (what, got_form, FORM_NAME.get(got_form))
            assert S in SPLITS[form], "%s: %d splits of K, the form needs %r: move the shape" % (what, S, SPLITS[form])
            Wg, bg, hWg, hbg = eng.params_get()
            if form == 5:
                assert int(twin.get_option("last_update_form")) == 3 and int(twin.get_option("last_wgrad_splits")) == 1
                dW, db = twin.grads()
            else:
                dW, db = eng.grads()                       # (after the update: the fused forms left the slabs untouched)
            assert np.isfinite(dW).all() and np.abs(dW).max() > 0 and np.abs(db).max() > 0
            Wr, hWr, Mw, Mh = rule.weights(state[0], state[2], dW)
            assert_bounded(Wg, Wr, Mw, n, "W after " + what)
            assert_bounded(hWg, hWr, Mh, n, "hW after " + what)
            del Wr, hWr, Mw, Mh
            br, hbr, Mw, Mh = rule.bias(state[1], state[3], db)
            assert_bounded(bg, br, Mw, n, "b after " + what)
            assert_bounded(hbg, hbr, Mh, n, "hb after " + what)
            moved = float((Wg != state[0]).mean())
            assert moved > 0.99, "%s: only %.2f %% of the weights changed" % (what, 100 * moved)
            q = reader.check(Wg, bg, max(maxima), prec, what)
            maxima.append(float(np.abs(Wg).max()))
            state = (Wg, bg, hWg, hbg)
        if twin is not None:
            for name, a, t in zip(("W", "b", "hW", "hb"), state, twin.params_get()):
                assert np.array_equal(a, t), "%s: %s differs from the twin's whose update was its own launch" % (what, name)
        if (D, F) == (4090, 4092):
            # one feature 1 .. 3 per row (a single product per output: exact whatever q is), rows in a permuted order, every column covered
            R = F + 300
            cols = np.concatenate([rng.permutation(F), rng.integers(0, F, size=300)])
            X = np.zeros((R, F), np.float32)
            X[np.arange(R), cols] = rng.integers(1, 4, size=R)
            assert (X != 0).any(0).all()
            check_dense_product(eng, X, q, bg, "product after " + what)
    finally:
        reader.free()
        eng.close()
        if twin is not None:
            twin.close()
