"""RMSProp and Adam, element by element against float64, in every form of the parameter update.

The two rules are BVLC Caffe's RMSPropSolver and AdamSolver (the reference tree has neither); the library states them in
SolverRule::step (RMSProp, solver_type 3: all five forms) and SolverRule::step2 (Adam, solver_type 5: the two-history instantiations of
k_sgd and k_reduce_sgd, forms 1 - 4; the weight-gradient GEMM's epilogue declines it).  This file restates them in numpy float64 beside
tests/test_gpu_update_exact.py's step64 and reuses that file's comparisons, its reader of the 16-bit copy and its engines.  Every case
asserts the form it ran ("last_update_form", "last_wgrad_splits"); the shapes are the smallest that file uses to land in each form, and
this file holds no copy of the dispatch rules either.

The reference applies the float64 rule to the GPU's own fp32 (w, m, v, g), read back as the existing file does (the gradient AFTER the
update; form 5 from a twin engine with wgrad_update = 0, which must end bit-equal).  The coefficients are the kernels' own: 1 - x is
formed once in fp32 (np.float32(1) - np.float32(x)), corr_t = sqrt(1 - beta2^t) / (1 - beta1^t) in double and rounded once to fp32.
Bound per element: n x 2^-24 x M (+ n x 2^-126), M the sum of the absolute values of every term of the expanded rule in float64, n the
rule's fp32 operations (u = 2^-24 each, correctly rounded add, mul, div, sqrt), with G = |g| + |dc| |r| as there:

  RMSProp   dc*r, g + . (-> g'), g' * g', om2 * ., decay * h, + (-> h'), sqrt, + delta, g' / ., lr * ., w - .     11 operations, n = 13
            g' carries two roundings and enters twice (numerator; squared under the root), so they count twice, as for AdaGrad:
            |err h'| <= (om2 (4 + 1 + 1) G^2 + decay |h| + M(h')) u <= 7 u M(h'), M(h') = decay |h| + om2 G^2 (= h' for h >= 0);
            d = sqrt(h') + delta carries 3.5 u + u + u = 5.5 u relatively; the quotient times lr: (2 + 5.5 + 1 + 1) u lr G / d; the final
            subtraction u M(w'): |err w'| <= u |w| + 10.5 u lr G / d <= 11.5 u M(w') < 13 u M(w'), M(w') = |w| + lr G / d.
  Adam      dc*r, g + . (-> g'), beta1 * m, om1 * g', + (-> m'), g' * g', om2 * ., beta2 * v, + (-> v'), sqrt, + delta, m' / .,
            lr * corr, * ., w - .                                                                                    15 operations, n = 15
            |err m'| <= (2 beta1 |m| + 4 om1 G) u <= 4 u M(m'), M(m') = beta1 |m| + om1 G; |err v'| <= 7 u M(v') as RMSProp's h';
            d as above 5.5 u; u = (lr corr) m' / d: (4 + 5.5 + 1 + 1 + 1) u (lr corr) M(m') / d; the subtraction u M(w'):
            |err w'| <= u |w| + 13.5 u (lr corr) M(m') / d <= 13.5 u M(w') < 15 u M(w'), M(w') = |w| + (lr corr) M(m') / d.
The counts are derived, not measured; no element is exempt; every case asserts that more than 99 % of the weights moved, and runs two
consecutive updates with a forward_backward between them (Adam: t = 1 and t = 2, two different corr_t).

Zero-gradient elements: feature columns that are zero in every table row give dW = 0 there; with decay_mult 0 and zero histories
g' = 0, m = v = 0 and u = 0 / (0 + delta) = 0: W, m and v must be unchanged bit for bit there and nothing anywhere may be non-finite.

On the parent commit solver_type 3 and 5 return VV_ERR_ARG ("Unknown SolverType"): every case here fails without the feature.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import vv  # noqa: F401  (fixture)
from tests.test_gpu_update_exact import FORM_NAME, SPLITS, CopyReader, Rule, assert_bounded, f32, make_engine

pytestmark = pytest.mark.gpu

VV_ERR_ARG = 1
N_OPS = {"RMSPROP": 13, "ADAM": 15}      # the docstring's derivation
# (form) -> D, F: the smallest shapes tests/test_gpu_update_exact.py lands in each form with
SHAPE = {1: (130, 256), 2: (30, 101), 3: (100, 128), 4: (1028, 4096), 5: (4090, 4092)}


# ------------------------------------------------------------------------------- the rules in float64
def regularise64(w, g, dc, reg):
    G = np.abs(g)
    if dc != 0.0:
        r = w if reg == 2 else np.sign(w)
        g = g + dc * r
        G = G + abs(dc) * np.abs(r)
    return g, G


def rmsprop64(w, h, g, lr, dc, reg, decay, om2, delta):
    """SolverRule::step, solver_type 3 -> w', h', M(w'), M(h')"""
    w, h, g = (np.asarray(a, np.float64) for a in (w, h, g))
    g, G = regularise64(w, g, dc, reg)
    hn = decay * h + om2 * (g * g)
    den = np.sqrt(hn) + delta
    return w - lr * (g / den), hn, np.abs(w) + lr * G / den, decay * np.abs(h) + om2 * G * G


def adam64(w, m, v, g, lr, dc, reg, b1, om1, b2, om2, corr, delta):
    """SolverRule::step2 -> w', m', v', M(w'), M(m'), M(v')"""
    w, m, v, g = (np.asarray(a, np.float64) for a in (w, m, v, g))
    g, G = regularise64(w, g, dc, reg)
    mn = b1 * m + om1 * g
    vn = b2 * v + om2 * (g * g)
    den = np.sqrt(vn) + delta
    Mm = b1 * np.abs(m) + om1 * G
    return w - (lr * corr) * (mn / den), mn, vn, np.abs(w) + (lr * corr) * Mm / den, Mm, b2 * np.abs(v) + om2 * G * G


def one_minus(x):
    """1 - x as the host forms it: once, in fp32"""
    return np.float64(np.float32(1.0) - np.float32(x))


class Rule2:
    """RMSProp / Adam settings as the kernels see them: fp32 values held in float64."""

    def __init__(self, solver, reg, lr=1e-3, wd=5e-4, beta1=0.9, beta2=0.999, rms_decay=0.99, delta=1e-8, decay_mult=(2, 0.5)):
        self.solver, self.reg, self.name = solver, {"L1": 1, "L2": 2}[reg], "%s/%s/wd %g" % (solver, reg, wd)
        self.lr, self.wd, self.delta = f32(lr), f32(wd), f32(delta)
        self.b1, self.b2, self.decay = f32(beta1), f32(beta2), f32(rms_decay)
        self.lr_mult, self.decay_mult = (0.5, 2.0), tuple(float(x) for x in decay_mult)
        self.kw = dict(lr=lr, momentum=beta1 if solver == "ADAM" else 0.0, weight_decay=wd, solver_type=solver, reg=reg, delta=delta,
                       lr_mult=self.lr_mult, decay_mult=self.decay_mult, momentum2=beta2, rms_decay=rms_decay)

    def cfg(self, vv, B=1, C=2, Nn=1):  # noqa: F811
        return vv.StepConfig(B, C, Nn, **self.kw)

    def corr(self, t):
        return np.float64(np.float32(np.sqrt(1.0 - float(self.b2) ** t) / (1.0 - float(self.b1) ** t)))

    def apply(self, k, w, m, v, g, t):
        """blob k (0 weights, 1 bias) -> (w', m', v' or None), (M(w'), M(m'), M(v') or None)"""
        lr, dc = self.lr * self.lr_mult[k], self.wd * self.decay_mult[k]
        if self.solver == "ADAM":
            r = adam64(w, m, v, g, lr, dc, self.reg, self.b1, one_minus(self.b1), self.b2, one_minus(self.b2), self.corr(t), self.delta)
            return r[:3], r[3:]
        wn, hn, Mw, Mh = rmsprop64(w, m, g, lr, dc, self.reg, self.decay, one_minus(self.decay), self.delta)
        return (wn, hn, None), (Mw, Mh, None)


def read_state(eng, adam):
    W, b, hW, hb = eng.params_get()
    vW, vb = eng.history2_get() if adam else (None, None)
    return W, b, hW, hb, vW, vb


def check_update(rule, before, after, dW, db, t, what):
    """after against the float64 rule applied to before (both read_state tuples) and the GPU's own gradient"""
    n = N_OPS[rule.solver]
    for k, blob, g in ((0, "W", dW), (1, "b", db)):
        w0, m0, v0 = before[k], before[2 + k], before[4 + k]
        ref, M = rule.apply(k, w0, m0, v0, g, t)
        assert_bounded(after[k], ref[0], M[0], n, "%s after %s" % (blob, what))
        assert_bounded(after[2 + k], ref[1], M[1], n, "h%s after %s" % (blob, what))
        if rule.solver == "ADAM":
            assert_bounded(after[4 + k], ref[2], M[2], n, "v%s after %s" % (blob, what))
    for a in after:
        assert a is None or np.isfinite(a).all(), what + ": non-finite values"
    moved = float((after[0] != before[0]).mean())
    assert moved > 0.99, "%s: only %.2f %% of the weights changed" % (what, 100 * moved)


def start_state(rng, D, F, zero_hist=False):
    W = rng.uniform(-0.02, 0.02, size=(D, F)).astype(np.float32)
    b = (rng.standard_normal(D) * 0.01).astype(np.float32)
    if zero_hist:
        return W, b, np.zeros_like(W), np.zeros_like(b), np.zeros_like(W), np.zeros_like(b)
    hW, hb = (rng.standard_normal((D, F)) * 1e-4).astype(np.float32), (rng.standard_normal(D) * 1e-4).astype(np.float32)
    vW, vb = rng.uniform(1e-9, 1e-7, size=(D, F)).astype(np.float32), rng.uniform(1e-9, 1e-7, size=D).astype(np.float32)
    return W, b, hW, hb, vW, vb


def engine_for(vv, prec, form, D, F, n_rows, st, solver, table=None):  # noqa: F811
    """make_engine of the existing file; RMSProp's single history is the non-negative one"""
    first = st[:4] if solver == "ADAM" else (st[0], st[1], st[4], st[5])
    if table is None:
        eng = make_engine(vv, prec, 1 if form == 2 else form, D, F, n_rows, first)
    else:
        eng = vv.Engine(0, prec)
        eng.set_dedup(False)
        eng.set_option("fuse_update", 0 if form in (1, 2) else 1)
        eng.set_option("slab16", 1 if form == 4 else 0)
        eng.set_option("wgrad_update", 1)
        eng.table_set(table)
        eng.params_set(*first)
    if solver == "ADAM":
        eng.history2_set(st[4], st[5])
    return eng


# ------------------------------------------------------------------------------- bounded, every form
CASES = [
    ("RMSPROP", 1, "f16", "L2"), ("RMSPROP", 2, "bf16", "L1"), ("RMSPROP", 3, "f16", "L1"), ("RMSPROP", 3, "bf16", "L2"),
    ("RMSPROP", 4, "f16", "L2"), ("RMSPROP", 4, "bf16", "L1"), ("RMSPROP", 5, "f16", "L2"), ("RMSPROP", 5, "bf16", "L1"),
    ("ADAM", 1, "f16", "L2"), ("ADAM", 1, "bf16", "L1"), ("ADAM", 2, "f16", "L1"), ("ADAM", 2, "bf16", "L2"),
    ("ADAM", 3, "f16", "L2"), ("ADAM", 3, "bf16", "L1"), ("ADAM", 4, "f16", "L1"), ("ADAM", 4, "bf16", "L2"),
    ("ADAM", 5, "f16", "L2"),                  # hinted on the form-5 shape: must run form 3 or 4, and end bit-equal to an un-hinted twin
]


@pytest.mark.parametrize("solver,form,prec,reg", CASES)
def test_rule_within_the_rounding_bound_in_every_form(vv, solver, form, prec, reg):  # noqa: F811
    B, C, Nn, n_rows = 32, 5, 4, 3000
    D, F = SHAPE[form]
    adam = solver == "ADAM"
    rule = Rule2(solver, reg)
    rng = np.random.default_rng(D + F + form)
    st = start_state(rng, D, F)
    eng = engine_for(vv, prec, form, D, F, n_rows, st, solver)
    twin, reader = None, CopyReader(eng, D, F)
    try:
        if form == 5:                                      # the same calls with the update as its own launch
            twin = engine_for(vv, prec, form, D, F, n_rows, st, solver)
            twin.set_option("wgrad_update", 0)
        cfg = rule.cfg(vv, B, C, Nn)
        before = read_state(eng, adam)
        maxima = [float(np.abs(before[0]).max())]
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
            if adam and form == 5:
                assert got_form in (3, 4), "%s: a hinted Adam step ran form %d (%s)" % (what, got_form, FORM_NAME.get(got_form))
            else:
                assert got_form == form, "%s ran form %d (%s): move the shape" % (what, got_form, FORM_NAME.get(got_form))
                assert S in SPLITS.get(form, SPLITS[1]), "%s: %d splits of K: move the shape" % (what, S)
            if adam:
                assert eng.solver_iter == k
            after = read_state(eng, adam)
            if form == 5 and not adam:
                assert int(twin.get_option("last_update_form")) == 3 and int(twin.get_option("last_wgrad_splits")) == 1
                dW, db = twin.grads()
            else:
                dW, db = eng.grads()
            assert np.isfinite(dW).all() and np.abs(dW).max() > 0 and np.abs(db).max() > 0
            check_update(rule, before, after, dW, db, k, what)
            reader.check(after[0], after[1], max(maxima), prec, what)
            maxima.append(float(np.abs(after[0]).max()))
            before = after
        if twin is not None:
            for name, a, t in zip(("W", "b", "hW", "hb", "vW", "vb"), before, read_state(twin, adam)):
                assert a is None or np.array_equal(a, t), "%s: %s differs from the twin's" % (what, name)
    finally:
        reader.free()
        eng.close()
        if twin is not None:
            twin.close()


# ------------------------------------------------------------------------------- zero-gradient elements
@pytest.mark.parametrize("solver", ["ADAM", "RMSPROP"])
@pytest.mark.parametrize("form", [1, 2, 3])
def test_zero_gradient_elements_stay_bit_for_bit(vv, solver, form):  # noqa: F811
    B, C, Nn, n_rows = 16, 3, 2, 200
    D, F = SHAPE[form]
    adam = solver == "ADAM"
    rng = np.random.default_rng(form)
    zero_cols = np.array([0, 5, F // 2, F - 1])
    table = rng.standard_normal((n_rows, F)).astype(np.float32)
    table[:, zero_cols] = 0.0
    rule = Rule2(solver, "L2", decay_mult=(0, 0))          # dc = 0: g' is the bare gradient
    st = start_state(rng, D, F, zero_hist=True)
    st[0][0, zero_cols[0]] = 0.0                           # (an exact zero and a negative zero among them)
    st[0][1, zero_cols[1]] = -0.0
    eng = engine_for(vv, "f16", form, D, F, n_rows, st, solver, table=table)
    try:
        cfg = rule.cfg(vv, B, C, Nn)
        before = read_state(eng, adam)
        for k in (1, 2):
            eng.forward_backward(cfg, rng.integers(0, n_rows, size=(B, C + Nn)).astype(np.int32))
            eng.apply_update(cfg)
            assert int(eng.get_option("last_update_form")) == form
            after = read_state(eng, adam)
            dW, db = eng.grads()
            assert not dW[:, zero_cols].any(), "the gradient of an all-zero feature column is not zero: the inputs are wrong"
            for name, a, a0 in zip(("W", "b", "hW", "hb", "vW", "vb"), after, before):
                if a is None:
                    continue
                assert np.isfinite(a).all(), "%s, form %d, update %d: non-finite %s" % (solver, form, k, name)
                if a.ndim == 2:
                    assert np.array_equal(a[:, zero_cols].view(np.uint32), a0[:, zero_cols].view(np.uint32)), \
                        "%s, form %d, update %d: %s changed where g' = 0" % (solver, form, k, name)
            other = np.setdiff1d(np.arange(F), zero_cols)
            assert (after[0][:, other] != before[0][:, other]).mean() > 0.9          # (no decay here: a unit no row activates keeps its weights)
            before = after
    finally:
        eng.close()


# ------------------------------------------------------------------------------- edges: t, the second history, vv_params_set
def test_iter_set_history2_round_trip_and_params_set(vv):  # noqa: F811
    B, C, Nn, n_rows = 32, 5, 4, 3000
    D, F = SHAPE[1]
    rule = Rule2("ADAM", "L2")
    rng = np.random.default_rng(11)
    st = start_state(rng, D, F)
    eng = make_engine(vv, "f16", 1, D, F, n_rows, st[:4])
    try:
        assert eng.solver_iter == 0 and eng.solver_ext_get() == (np.float32(0.999), np.float32(0.99))
        z = eng.history2_get()
        assert not z[0].any() and not z[1].any(), "the second history reads as zeros before its first use"
        eng.history2_set(st[4], st[5])
        got = eng.history2_get()
        assert np.array_equal(got[0], st[4]) and np.array_equal(got[1], st[5])
        cfg = rule.cfg(vv, B, C, Nn)
        before = read_state(eng, True)
        eng.forward_backward(cfg, rng.integers(0, n_rows, size=(B, C + Nn)).astype(np.int32))
        eng.solver_iter = 1000
        eng.apply_update(cfg)
        assert eng.solver_iter == 1001 and int(eng.get_option("last_update_form")) == 1
        after = read_state(eng, True)
        dW, db = eng.grads()
        assert abs(rule.corr(1001) / rule.corr(1) - 1.0) > 0.5          # (the two corrections are far apart: a wrong t fails the bound)
        check_update(rule, before, after, dW, db, 1001, "one update after vv_solver_iter_set(1000)")
        eng.params_set(*st[:4])
        assert eng.solver_iter == 0, "vv_params_set resets t"
        z = eng.history2_get()
        assert not z[0].any() and not z[1].any(), "vv_params_set clears the second history"
        # an SGD update in between does not count
        sgd = Rule("SGD", "L2", 0.01, 0.9, 5e-4).cfg(vv, B, C, Nn)
        eng.forward_backward(sgd, rng.integers(0, n_rows, size=(B, C + Nn)).astype(np.int32))
        eng.apply_update(sgd)
        assert eng.solver_iter == 0, "t counts Adam updates only"
    finally:
        eng.close()


# ------------------------------------------------------------------------------- argument checks
def test_argument_checks(vv):  # noqa: F811
    B, C, Nn, n_rows = 8, 3, 2, 100
    D, F = SHAPE[3]
    rng = np.random.default_rng(3)
    st = start_state(rng, D, F)
    eng = make_engine(vv, "f16", 3, D, F, n_rows, st[:4])
    idx = rng.integers(0, n_rows, size=(B, C + Nn)).astype(np.int32)

    def refused(**kw):
        cfg = vv.StepConfig(B, C, Nn, **kw)
        with pytest.raises(vv.VVError) as e:
            eng.forward_backward(cfg, idx)
        assert "videovec error %d" % VV_ERR_ARG in str(e.value), str(e.value)
        return str(e.value)

    try:
        refused(solver_type="RMSPROP", momentum=0.9)
        refused(solver_type="RMSPROP", momentum=0.0, rms_decay=1.0)
        refused(solver_type="ADAM", momentum=0.9, momentum2=1.0)
        assert "not implemented" in refused(solver_type=4, momentum=0.0)
        refused(solver_type=6)
        for kw in (dict(solver_type="RMSPROP", momentum=0.0, rms_decay=0.99), dict(solver_type="ADAM", momentum=0.9, momentum2=0.999),
                   dict(solver_type=3, momentum=0.0, rms_decay=0.0), dict(solver_type=5, momentum=0.0, momentum2=0.0)):
            cfg = vv.StepConfig(B, C, Nn, lr=1e-3, **kw)
            eng.params_set(st[0], st[1])                   # (zero histories: RMSProp's and Adam's v must not start negative)
            eng.forward_backward(cfg, idx)
            eng.apply_update(cfg)
            assert all(np.isfinite(a).all() for a in eng.params_get())
    finally:
        eng.close()


# ------------------------------------------------------------------------------- the existing solvers are untouched
@pytest.mark.parametrize("form", [1, 2, 3, 4, 5])
def test_existing_solvers_ignore_the_new_values(vv, form):  # noqa: F811
    """SGD, Nesterov and AdaGrad after vv_solver_ext_set with non-default values: bit for bit a fresh context's that never called it."""
    B, C, Nn, n_rows = 32, 5, 4, 3000
    D, F = SHAPE[form]
    rng = np.random.default_rng(form)
    W, b, hW, hb, vW, vb = start_state(rng, D, F)
    idx = rng.integers(0, n_rows, size=(B, C + Nn)).astype(np.int32)
    engs = [make_engine(vv, "f16", 1 if form == 2 else form, D, F, n_rows, (W, b, hW, hb)) for _ in range(2)]
    try:
        engs[0].solver_ext_set(0.5, 0.25)
        for solver in ("SGD", "NESTEROV", "ADAGRAD"):
            ada = solver == "ADAGRAD"
            cfg = Rule(solver, "L2", 0.05, 0.0 if ada else 0.9, 5e-4, 1e-6 if ada else 0.0).cfg(vv, B, C, Nn)
            res = []
            for e in engs:
                e.params_set(W, b, vW if ada else hW, vb if ada else hb)
                if form == 5:
                    e.update_hint(cfg)
                e.forward_backward(cfg, idx)
                e.apply_update(cfg)
                assert int(e.get_option("last_update_form")) == form, "move the shape"
                res.append(e.params_get())
            for name, x, y in zip(("W", "b", "hW", "hb"), *res):
                assert np.array_equal(x, y), "%s, form %d: %s differs after vv_solver_ext_set" % (solver, form, name)
            assert (res[0][0] != W).mean() > 0.99
    finally:
        for e in engs:
            e.close()
