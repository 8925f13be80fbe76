"""Gradient clipping by the global L2 norm (vv_clip_gradients_set; BVLC Caffe's SGDSolver::ClipGradients -- the reference tree has no such
function), against float64, in front of every solver rule.

Every case runs two engines on the same batch: `eng` with clipping, and a `twin` with clipping disabled whose gradient before the update is
bit-identical to eng's (dense execution is deterministic; case (c) asserts the premise with np.array_equal).  The twin is stepped first,
its gradient g is read back after its update (as tests/test_gpu_update_exact.py does; on the form-5 shape a hinted twin never stores its
gradient, so there a third engine with wgrad_update = 0 provides it), the threshold is derived from g, and then eng takes the same step.
The shapes are the smallest that file uses to land in each form; its engines, step64, assert_bounded and CopyReader and the float64 rules
of tests/test_gpu_update_adam_rmsprop.py are imported, nothing is copied.

(a) The norm.  k_grad_sumsq squares each fp32 element exactly in double (24 x 24 bits fit 53) and adds the n squares in double: every
    addition is correctly rounded, so the computed sum differs from the true sum S by at most (n - 1) 2^-53 S relatively, whatever the
    order (all terms are >= 0: no cancellation).  numpy's float64 reference carries the same kind of error.  sqrt halves a relative
    error and adds 2^-53.  With n <= 16.8 M = 2^24 both norms are within 2^-29 of the true one -- 2^-5 of fp32's half-ulp -- so the two
    SINGLE roundings to fp32 see inputs that differ by far less than one ulp and can differ only when a rounding boundary lies between
    them: by at most 1 ulp.  That is the bound; it is derived, not measured.
(b) A clipped step (threshold = float64 norm / 3): scale against float32(clip / norm) formed in double from the read-back norm, 1 ulp
    (the kernel divides by the double norm, the test by its fp32 rounding: relative difference 2^-24, one ulp after rounding); the
    gradient read back is np.array_equal to float32(g) * float32(scale) -- one fp32 multiply --; the update ran form 1 (2 at F % 4 != 0)
    while the twin still ran 3, 4, 5; W, b and the histories are held to the float64 rule applied to that clipped gradient with the
    per-element bounds and operation counts of the two existing files.
(c) Not clipped (threshold 2 x norm, and the read-back norm itself: > is strict): everything bit-identical to the twin.
(d) A zero gradient (zero table, loss weight 0) with clip 1 and clip 0: norm 0, scale 1, nothing non-finite, W as the twin's.
(e) clip 0 on a non-zero gradient: scale 0, the gradient reads back as zeros.
(f) Two consecutive clipped steps: the counters read 2 and 2 (Adam: t = 1, 2).
(g) vv_update_hint / vv_step on the form-5 shape with clipping active run form 1 and end bit-equal to the un-hinted calls; a hint under
    one threshold followed by vv_apply_update under another is refused like any other parameter mismatch.
(h) Arguments.

Without the feature the binding has no vv_clip_gradients_set: every case fails.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import vv  # noqa: F401  (fixture)
from tests.test_gpu_update_adam_rmsprop import SHAPE, Rule2, check_update, engine_for, read_state, start_state
from tests.test_gpu_update_exact import FORM_NAME, N_OPS, CopyReader, Rule, assert_bounded

pytestmark = pytest.mark.gpu

VV_ERR_ARG, VV_ERR_STATE = 1, 3
B, C, Nn, N_ROWS = 32, 5, 4, 3000


def ulps(a, b):
    """distance of two positive fp32 values in units of the last place"""
    a, b = np.float32(a), np.float32(b)
    assert a >= 0 and b >= 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def norm64(dW, db):
    return float(np.sqrt((dW.astype(np.float64) ** 2).sum() + (db.astype(np.float64) ** 2).sum()))


def make_rule(solver, reg="L2"):
    if solver in ("RMSPROP", "ADAM"):
        return Rule2(solver, reg)
    ada = solver == "ADAGRAD"
    return Rule(solver, reg, 0.05, 0.0 if ada else 0.9, 5e-4, 1e-6 if ada else 0.0)


class Pair:
    """eng (clips), twin (does not), and where the twin never stores its gradient (form 5, hinted) a third engine that does."""

    def __init__(self, vv, form, solver="SGD", prec="f16", hinted_twin=False, table=None, cfg_kw=None):  # noqa: F811
        self.form, self.solver, self.adam = form, solver, solver == "ADAM"
        self.D, self.F = SHAPE[form]
        self.rng = np.random.default_rng(self.D + self.F + form)
        self.st = start_state(self.rng, self.D, self.F)
        self.rule = make_rule(solver)
        mk = lambda: engine_for(vv, prec, form, self.D, self.F, N_ROWS, self.st, solver, table=table)
        self.eng, self.twin = mk(), mk()
        self.gsrc, self.all = self.twin, [self.twin, self.eng]
        if form == 5 and hinted_twin:
            self.gsrc = mk()
            self.all.insert(0, self.gsrc)
        if form == 5:
            self.gsrc.set_option("wgrad_update", 0)
        self.cfg = self.rule.cfg(vv, B, C, Nn)
        for k, v in (cfg_kw or {}).items():
            self.cfg.set(k, v)
        self.steps = 0

    def batch(self):
        return self.rng.integers(0, N_ROWS, size=(B, C + Nn)).astype(np.int32)

    def run(self, e, idx):
        if self.form == 5:
            e.update_hint(self.cfg)
        e.forward_backward(self.cfg, idx)
        e.apply_update(self.cfg)

    def step(self, clip_of, idx=None):
        """the engines without clipping first; clip_of(g's float64 norm) -> eng's threshold; -> (dW, db) of the unclipped gradient"""
        idx = self.batch() if idx is None else idx
        for e in self.all[:-1]:
            self.run(e, idx)
        dW, db = self.gsrc.grads()
        assert np.isfinite(dW).all() and np.isfinite(db).all()
        self.eng.clip_gradients_set(clip_of(norm64(dW, db)))
        self.run(self.eng, idx)
        self.steps += 1
        return dW, db

    def reset(self):
        for e in self.all:
            first = self.st[:4] if self.adam else (self.st[0], self.st[1], self.st[4], self.st[5])
            e.params_set(*first)
            if self.adam:
                e.history2_set(self.st[4], self.st[5])

    def forms(self):
        return int(self.eng.get_option("last_update_form")), int(self.twin.get_option("last_update_form"))

    def assert_forms(self, what):
        got, twin = self.forms()
        want = 2 if self.F % 4 else 1
        assert got == want, "%s: the clipped update ran form %d (%s), not %d" % (what, got, FORM_NAME.get(got), want)
        # (form-5 shape: a twin with wgrad_update = 0 runs k_reduce_sgd, and so does a hinted Adam twin -- the epilogue declines two histories,
        # as tests/test_gpu_update_adam_rmsprop.py asserts)
        want_twin = (3, 4) if self.form == 5 and self.adam else (3,) if self.form == 5 and self.gsrc is self.twin else (self.form,)
        assert twin in want_twin, "%s: the twin ran form %d (%s): move the shape" % (what, twin, FORM_NAME.get(twin))

    def close(self):
        for e in self.all:
            e.close()


def assert_states_equal(p, what):
    for name, a, t in zip(("W", "b", "hW", "hb", "vW", "vb"), read_state(p.eng, p.adam), read_state(p.twin, p.adam)):
        assert a is None or np.array_equal(a.view(np.uint32), t.view(np.uint32)), "%s: %s differs from the twin's" % (what, name)


def check_rule(rule, before, after, dW, db, t, what):
    """after against the float64 rule on (before, the clipped gradient); the float64 reference itself must move > 99 % of the weights"""
    if isinstance(rule, Rule2):
        ref, _ = rule.apply(0, before[0], before[2], before[4], dW, t)
        moved = float((ref[0].astype(np.float32) != before[0]).mean())
        assert moved > 0.99, "%s: the float64 rule moves only %.2f %% of the weights: the inputs are wrong" % (what, 100 * moved)
        check_update(rule, before, after, dW, db, t, what)
        return
    n = N_OPS[rule.solver]
    Wr, hWr, Mw, Mh = rule.weights(before[0], before[2], dW)
    moved = float((Wr.astype(np.float32) != before[0]).mean())
    assert moved > 0.99, "%s: the float64 rule moves only %.2f %% of the weights: the inputs are wrong" % (what, 100 * moved)
    assert_bounded(after[0], Wr, Mw, n, "W after " + what)
    assert_bounded(after[2], hWr, Mh, n, "hW after " + what)
    del Wr, hWr, Mw, Mh
    br, hbr, Mw, Mh = rule.bias(before[1], before[3], db)
    assert_bounded(after[1], br, Mw, n, "b after " + what)
    assert_bounded(after[3], hbr, Mh, n, "hb after " + what)
    moved = float((after[0] != before[0]).mean())
    assert moved > 0.99, "%s: only %.2f %% of the weights changed" % (what, 100 * moved)


# ------------------------------------------------------------------------------- (a) the norm
@pytest.mark.parametrize("form", [1, 2, 3, 4, 5])
def test_norm_within_one_ulp_of_float64(vv, form):  # noqa: F811
    """n = D F + D: 33 410 (130 x 256), 3 060 (30 x 101: not a multiple of 4, less than one pass of the 65 536-thread grid and of its
    16-byte items), 12 900, 4 211 716 and 16 740 370 (many passes, a scalar tail of 2)."""
    p = Pair(vv, form)
    try:
        dW, db = p.step(lambda nrm: 1e30)                  # active, never reached
        s = p.eng.clip_stats()
        ref = np.float32(norm64(dW, db))
        print("form-%d shape, n = %d: norm %r, float64 %r" % (form, dW.size + db.size, float(s["norm"]), float(ref)))
        assert ref > 0 and np.isfinite(s["norm"])
        assert ulps(s["norm"], ref) <= 1, "norm %r against float32(sqrt(sum float64(g)^2)) = %r" % (float(s["norm"]), float(ref))
        assert s["scale"] == 1.0 and s["clipped"] == 0 and s["updates"] == 1 and s["clipped_updates"] == 0
        p.assert_forms("never reached")
    finally:
        p.close()


# ------------------------------------------------------------------------------- (b) a clipped step
CLIPPED = [("SGD", 1), ("SGD", 3), ("SGD", 5), ("ADAGRAD", 1), ("ADAGRAD", 3), ("ADAGRAD", 5), ("ADAM", 1), ("ADAM", 3), ("ADAM", 5),
           ("RMSPROP", 1), ("NESTEROV", 1), ("SGD", 2), ("SGD", 4)]


@pytest.mark.parametrize("solver,form", CLIPPED)
def test_clipped_step_against_the_float64_rule(vv, solver, form):  # noqa: F811
    p = Pair(vv, form, solver, hinted_twin=True)
    # (the 16-bit copy is read where CopyReader's own condition on elements below 2^-20 max |w| -- fewer than 1e-5 of all -- leaves room for
    # the handful a random update produces: the two large shapes)
    reader = CopyReader(p.eng, p.D, p.F) if p.D * p.F >= 1 << 22 else None
    try:
        what = "%s, %d x %d, clipped" % (solver, p.D, p.F)
        before = read_state(p.eng, p.adam)
        clip = []
        dW, db = p.step(lambda nrm: clip.append(np.float32(nrm / 3.0)) or clip[0])
        s = p.eng.clip_stats()
        assert s["clipped"] == 1 and s["updates"] == 1 and s["clipped_updates"] == 1
        assert ulps(s["norm"], np.float32(norm64(dW, db))) <= 1
        want = np.float32(np.float64(clip[0]) / np.float64(s["norm"]))
        assert ulps(s["scale"], want) <= 1, "scale %r against float32(clip / norm) = %r" % (float(s["scale"]), float(want))
        p.assert_forms(what)
        gW, gb = p.eng.grads()
        cW, cb = dW * s["scale"], db * s["scale"]           # fp32 x fp32: one rounding
        assert cW.dtype == np.float32 and np.array_equal(gW, cW) and np.array_equal(gb, cb), what + ": the gradient read back is not g * scale"
        after = read_state(p.eng, p.adam)
        check_rule(p.rule, before, after, cW, cb, 1, what)
        if reader is not None:
            reader.check(after[0], after[1], float(np.abs(before[0]).max()), "f16", what)
        assert not np.array_equal(after[0], p.twin.params_get()[0]), what + ": the clipped update equals the unclipped one"
    finally:
        if reader is not None:
            reader.free()
        p.close()


# ------------------------------------------------------------------------------- (c) not clipped
@pytest.mark.parametrize("solver,form", [("SGD", 1), ("ADAM", 2), ("NESTEROV", 3), ("SGD", 4)])
def test_below_or_at_the_threshold_nothing_changes(vv, solver, form):  # noqa: F811
    p = Pair(vv, form, solver)
    try:
        idx = p.batch()
        dW, db = p.step(lambda nrm: 2.0 * nrm, idx)
        gW, gb = p.eng.grads()
        assert np.array_equal(gW, dW) and np.array_equal(gb, db), "the two engines' gradients differ: the premise of this file"
        assert_states_equal(p, "threshold 2 x norm")
        p.assert_forms("threshold 2 x norm")
        s = p.eng.clip_stats()
        assert (s["clipped"], s["scale"], s["updates"], s["clipped_updates"]) == (0, 1.0, 1, 0)
        # the same state and batch again (the same gradient, so the same norm bit for bit), the threshold the read-back norm itself
        p.reset()
        dW2, db2 = p.step(lambda nrm: s["norm"], idx)
        assert np.array_equal(dW2, dW)
        s2 = p.eng.clip_stats()
        assert s2["norm"] == s["norm"] and p.eng.clip_gradients_get() == s["norm"]
        assert (s2["clipped"], s2["scale"], s2["updates"], s2["clipped_updates"]) == (0, 1.0, 2, 0), "norm == clip must not clip (> is strict)"
        gW, gb = p.eng.grads()
        assert np.array_equal(gW, dW) and np.array_equal(gb, db)
        assert_states_equal(p, "threshold == norm")
    finally:
        p.close()


# ------------------------------------------------------------------------------- (d) zero gradient
@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_zero_gradient(vv, clip):  # noqa: F811
    D, F = SHAPE[1]
    p = Pair(vv, 1, "SGD", table=np.zeros((N_ROWS, F), np.float32), cfg_kw={"loss_weight": 0.0})
    try:
        W0 = p.st[0]
        dW, db = p.step(lambda nrm: clip)
        assert not dW.any() and not db.any(), "the gradient is not zero: the inputs are wrong"
        s = p.eng.clip_stats()
        assert s["norm"] == 0.0 and s["scale"] == 1.0 and s["clipped"] == 0 and s["updates"] == 1 and s["clipped_updates"] == 0
        gW, gb = p.eng.grads()
        assert np.array_equal(gW, np.zeros_like(gW)) and np.array_equal(gb, np.zeros_like(gb))
        for a in read_state(p.eng, False)[:4]:
            assert np.isfinite(a).all()
        assert_states_equal(p, "zero gradient, clip %g" % clip)
        assert (p.eng.params_get()[0] != W0).mean() > 0.99, "the regulariser and the momentum still move W"
    finally:
        p.close()


# ------------------------------------------------------------------------------- (e) clip = 0
def test_threshold_zero_zeroes_the_gradient(vv):  # noqa: F811
    p = Pair(vv, 2, "SGD")
    try:
        dW, db = p.step(lambda nrm: 0.0)
        assert dW.any() and db.any()
        s = p.eng.clip_stats()
        assert s["scale"] == 0.0 and s["clipped"] == 1 and s["norm"] > 0
        gW, gb = p.eng.grads()
        assert np.array_equal(gW, np.zeros_like(gW)) and np.array_equal(gb, np.zeros_like(gb))      # (a -0 compares equal)
        assert all(np.isfinite(a).all() for a in p.eng.params_get())
    finally:
        p.close()


# ------------------------------------------------------------------------------- (f) two consecutive clipped steps
@pytest.mark.parametrize("solver", ["ADAM", "SGD"])
def test_two_consecutive_clipped_steps(vv, solver):  # noqa: F811
    p = Pair(vv, 1, solver)
    try:
        for k in (1, 2):
            what = "%s, update %d" % (solver, k)
            before = read_state(p.eng, p.adam)
            for name, a, t in zip(("W", "b"), before, read_state(p.twin, p.adam)):
                assert k == 2 or np.array_equal(a, t)
            # (from the second step on eng's parameters are its own: its gradient comes from a twin moved to eng's state)
            if k == 2:
                p.twin.params_set(*before[:4])
                if p.adam:
                    p.twin.history2_set(before[4], before[5])
                    p.twin.solver_iter = 1
            dW, db = p.step(lambda nrm: nrm / 3.0)
            s = p.eng.clip_stats()
            assert s["updates"] == k and s["clipped_updates"] == k and s["clipped"] == 1
            assert ulps(s["norm"], np.float32(norm64(dW, db))) <= 1
            cW, cb = dW * s["scale"], db * s["scale"]
            gW, gb = p.eng.grads()
            assert np.array_equal(gW, cW) and np.array_equal(gb, cb)
            if p.adam:
                assert p.eng.solver_iter == k
            check_rule(p.rule, before, read_state(p.eng, p.adam), cW, cb, k, what)
    finally:
        p.close()


# ------------------------------------------------------------------------------- (g) hint and step
def test_hint_and_step_with_clipping_run_form_1(vv):  # noqa: F811
    D, F = SHAPE[5]
    rng = np.random.default_rng(5)
    st = start_state(rng, D, F)
    rule = make_rule("SGD")
    cfg = rule.cfg(vv, B, C, Nn)
    idx = rng.integers(0, N_ROWS, size=(B, C + Nn)).astype(np.int32)
    engs = [engine_for(vv, "f16", 5, D, F, N_ROWS, st, "SGD") for _ in range(3)]
    plain, hinted, stepped = engs
    try:
        plain.forward_backward(cfg, idx)                   # no clipping, no hint: the norm of this batch's gradient
        plain.apply_update(cfg)
        assert int(plain.get_option("last_update_form")) == 3
        clip = norm64(*plain.grads()) / 3.0
        plain.params_set(st[0], st[1], st[4], st[5])       # (engine_for's start for a one-history rule)
        for e in engs:
            e.clip_gradients_set(clip)
        plain.forward_backward(cfg, idx)
        plain.apply_update(cfg)
        hinted.update_hint(cfg)
        hinted.forward_backward(cfg, idx)
        hinted.apply_update(cfg)
        stepped.step(cfg, idx)
        res = []
        for e in engs:
            assert int(e.get_option("last_update_form")) == 1 and int(e.get_option("last_wgrad_splits")) == 1
            s = e.clip_stats()
            assert s["clipped"] == 1 and s["clipped_updates"] == 1
            res.append(e.params_get() + e.grads() + (s["norm"], s["scale"]))
        for other, name in ((res[1], "vv_update_hint"), (res[2], "vv_step")):
            for a, b_ in zip(res[0], other):
                assert np.array_equal(a, b_), name + " with clipping differs from the un-hinted calls"
        # a hint under one threshold, the update under another: refused, and nothing was half-applied -- the announced threshold works
        for first, second in ((-1.0, clip), (clip, 2 * clip), (clip, -1.0)):
            hinted.clip_gradients_set(first)
            hinted.update_hint(cfg)
            hinted.forward_backward(cfg, idx)
            hinted.clip_gradients_set(second)
            with pytest.raises(vv.VVError) as err:
                hinted.apply_update(cfg)
            assert "videovec error %d" % VV_ERR_ARG in str(err.value) and "vv_update_hint" in str(err.value), str(err.value)
            hinted.clip_gradients_set(first)
            hinted.apply_update(cfg)
            assert int(hinted.get_option("last_update_form")) == (5 if first < 0 else 1)
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------------------- (h) arguments
def test_arguments(vv):  # noqa: F811
    eng = vv.Engine(0, "f16")
    try:
        assert eng.clip_gradients_get() == -1.0, "a fresh context has clipping disabled"
        s = eng.clip_stats()
        assert (s["norm"], s["scale"], s["clipped"], s["updates"], s["clipped_updates"]) == (0.0, 1.0, 0, 0, 0)
        with pytest.raises(vv.VVError) as err:
            eng.clip_gradients_set(float("nan"))
        assert "videovec error %d" % VV_ERR_ARG in str(err.value)
        assert eng.clip_gradients_get() == -1.0
        for v in (0.0, 35.0, 1e-3, -1.0, -5.0, 2.5):
            eng.clip_gradients_set(v)
            assert eng.clip_gradients_get() == np.float32(v)
        cfg = vv.StepConfig(4, 3, 2, clip_gradients=7.0)
        assert cfg.clip_gradients == 7.0 and vv.StepConfig(4, 3, 2).clip_gradients is None
        D, F = SHAPE[3]
        st = start_state(np.random.default_rng(1), D, F)
        eng.table_synth(7, 100, F)
        eng.params_set(*st[:4])
        eng.forward_backward(cfg, np.zeros((4, 5), np.int32))          # the keyword is forwarded in front of the call, like momentum2
        assert eng.clip_gradients_get() == 7.0
    finally:
        eng.close()
