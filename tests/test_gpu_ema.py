"""The exponential moving average of the parameters (vv_ema_set / _get / _use / _stats; Engine.ema_set / ema_get / ema_use / ema_stats / ema()).

  k_ema bit for bit   e' = decay * e + om * w with om = 1.0f - decay, restated in numpy float32 (every product and the sum rounded as
                      written); w is the GPU's own fp32 W / b read back after each update, so the update's arithmetic is not part of the
                      comparison and np.array_equal is the condition.  Three consecutive updates per case; every case asserts the update
                      form it ran ("last_update_form") and that the weights moved.
                      Shapes: one per update form, those of tests/test_gpu_update_exact.py (1028 x 2048 for k_sgd with 16-byte accesses
                      and for k_reduce_sgd, 258 x 1021 for k_sgd scalar, 1028 x 4096 over f16 slabs, 4090 x 4092 for the weight-gradient
                      epilogue of a hinted step); 30 x 101 for k_ema's scalar form with most workgroups idle; 516 x 2052 = 264 708 16-byte
                      items and 258 x 1021 = 263 418 scalars, each past one pass of k_ema's 1024 x 256 threads; D F of 63, 64, 65 and 252
                      (with D % 4 = 1: the bias ends in a scalar), 255, 256 around one wave and one workgroup.
                      Decay 0, 0.5, 0.999 x all five solvers; a clipped and an accumulated update (one k_ema per UPDATE: ema_stats).
  training untouched  W, b, the histories, the 16-bit copy, every loss and the gradients of a run with the average are those of a run
                      without it: lazily reduced steps, Adam, the hinted form 5.
  evaluation          under ema_use: forward + eval_stats (with ip2 and the score blobs), embed, embed_mean, gallery_from_table + topk
                      bit for bit those of a twin engine given params_set(*ema_get()), in score forms 1 and 4; after ema_use(0) the next
                      training step is that of an undisturbed run.
  errors              every VV_ERR_ARG / VV_ERR_STATE case of include/videovec.h's section (the schedules: tests/test_gpu_comm_ema.py).
"""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_forward_only import FORMS, N_ROWS, engine as fwd_engine, half_copy, same_tree
from tests.test_gpu_parity import vv  # noqa: F401  (fixture)
from tests.test_gpu_score_seg_exact import batch, world  # noqa: F401  (the shared (table, W, b))
from tests.test_gpu_update_exact import FORM_NAME, CopyReader, operator_gradient

pytestmark = pytest.mark.gpu

VV_ERR_ARG, VV_ERR_STATE = 1, 3
EMA_GRID = 1024 * 256                    # k_ema's threads, for the "past one pass" assertions and the failure report
B, C, NN, ROWS = 32, 5, 4, 3000          # the batch of tests/test_gpu_update_exact.py's real steps

SOLVER_KW = {
    "SGD": dict(lr=0.05, momentum=0.9, weight_decay=5e-4),
    "NESTEROV": dict(lr=0.05, momentum=0.9, weight_decay=5e-4),
    "ADAGRAD": dict(lr=0.05, momentum=0.0, weight_decay=5e-4, delta=1e-6),
    "RMSPROP": dict(lr=0.01, momentum=0.0, weight_decay=5e-4, delta=1e-6, rms_decay=0.9),
    "ADAM": dict(lr=0.01, momentum=0.9, momentum2=0.999, weight_decay=5e-4, delta=1e-6),
}


def step_cfg(vv, solver="SGD", b=B, c=C, nn=NN, **extra):  # noqa: F811
    kw = dict(SOLVER_KW[solver], solver_type=solver)
    kw.update(extra)
    return vv.StepConfig(b, c, nn, **kw)


def ema_ref(e, w, decay):
    """the rule in numpy float32: two products and one sum, each rounded"""
    d = np.float32(decay)
    om = np.float32(1.0) - d
    out = d * e + om * w
    assert out.dtype == np.float32
    return out


def assert_ema(got, ref, what, per):
    if np.array_equal(got, ref):
        return
    g, r = np.atleast_2d(got), np.atleast_2d(ref)
    bad = np.argwhere(~(g == r))
    d, f = (int(v) for v in bad[0])
    flat = d * g.shape[1] + f
    msg = ("%s: %d of %d elements differ from decay * e + om * w in float32; first at (d %d, f %d), flat %d = pass %d of k_ema's grid over "
           "%d-element items: got %r, expected %r" % (what, len(bad), r.size, d, f, flat, flat // per // EMA_GRID, per, float(g[d, f]), float(r[d, f])))
    print(msg)
    pytest.fail(msg)


def start_state(D, F, seed):
    rng = np.random.default_rng(seed)
    W = rng.uniform(-0.02, 0.02, size=(D, F)).astype(np.float32)
    b = (rng.standard_normal(D) * 0.01).astype(np.float32)
    hW, hb = np.full_like(W, 1e-4), np.full_like(b, 1e-4)       # (non-zero: AdaGrad's first step from h = 0 is lr sign(g))
    return W, b, hW, hb


def step_engine(vv, form, D, F, state, prec="f16"):  # noqa: F811
    """An engine whose real steps land in update form `form` at the shapes of tests/test_gpu_update_exact.py (asserted by the callers)."""
    eng = vv.Engine(0, prec)
    eng.set_dedup(False)
    eng.set_option("fuse_update", 0 if form in (1, 2) else 1)
    eng.set_option("slab16", 1 if form == 4 else 0)
    eng.set_option("wgrad_update", 1)
    eng.table_synth(7, ROWS, F)
    eng.params_set(*state)
    return eng


class Follower:
    """The average restated on the host beside an engine: started from the parameters at the activation, advanced from the GPU's own
    W and b after each update."""

    def __init__(self, eng, decay, F):
        self.eng, self.decay, self.per = eng, decay, 4 if F % 4 == 0 else 1
        eng.ema_set(decay)
        W, b, _, _ = eng.params_get()
        self.eW, self.eb, self.W, self.n = W, b, W, 0
        self.check("at the activation")

    def check(self, what):
        gW, gb = self.eng.ema_get()
        assert_ema(gW, self.eW, "eW " + what, self.per)
        assert_ema(gb, self.eb, "eb " + what, self.per)

    def after_update(self, what):
        W, b, _, _ = self.eng.params_get()
        assert np.isfinite(W).all() and np.isfinite(b).all(), what + ": non-finite parameters -- the case's inputs are wrong"
        moved = float((W != self.W).mean())
        assert moved > 0.99, "%s: only %.2f %% of the weights changed -- the case tests nothing" % (what, 100 * moved)
        self.eW, self.eb, self.W, self.n = ema_ref(self.eW, W, self.decay), ema_ref(self.eb, b, self.decay), W, self.n + 1
        self.check(what)
        st = self.eng.ema_stats()
        assert st["updates"] == self.n and st["decay"] == np.float32(self.decay) and not st["in_use"], (what, st)


# ------------------------------------------------------------------------------- k_ema behind each form of the update
# (form, D, F): see the docstring
FORM_CASES = [(1, 1028, 2048), (2, 258, 1021), (3, 1028, 2048), (4, 1028, 4096), (5, 4090, 4092), (2, 30, 101), (1, 516, 2052)]


@pytest.mark.parametrize("form,D,F", FORM_CASES)
def test_k_ema_bit_for_bit_behind_every_update_form(vv, form, D, F):  # noqa: F811
    if (D, F) in ((258, 1021), (516, 2052)):
        assert D * F // (4 if F % 4 == 0 else 1) > EMA_GRID                 # past one pass of the grid
    eng = step_engine(vv, form, D, F, start_state(D, F, D + F + form))
    try:
        cfg = step_cfg(vv)
        fol = Follower(eng, 0.999, F)
        rng = np.random.default_rng(form)
        for k in (1, 2, 3):
            idx = rng.integers(0, ROWS, size=(B, C + NN)).astype(np.int32)
            if form == 5:
                eng.update_hint(cfg)
            eng.forward_backward(cfg, idx)
            eng.apply_update(cfg)
            got = int(eng.get_option("last_update_form"))
            what = "%d x %d, form %d, update %d" % (D, F, form, k)
            assert got == form, "%s ran form %d (%s): move the shape" % (what, got, FORM_NAME.get(got))
            fol.after_update(what)
        assert not np.array_equal(fol.eW, fol.W)                             # (the average lags the weights)
    finally:
        eng.close()


# D x F = 63, 64, 65, 252 (D % 4 = 1), 255, 256 elements: below, at and above one wave and one workgroup of k_ema
SMALL = [(7, 9), (8, 8), (5, 13), (9, 28), (5, 51), (8, 32)]


@pytest.mark.parametrize("D,F", SMALL)
def test_k_ema_bit_for_bit_around_a_wave_and_a_workgroup(vv, D, F):  # noqa: F811
    """Through the per-layer operators (X the F x F identity: dW = dY^T), as tests/test_gpu_update_exact.py's exact cases."""
    eng = vv.Engine(0, "f16")
    eng.set_option("fuse_update", 0)
    eng.table_set(np.ones((1, F), np.float32))
    rng = np.random.default_rng(D * F)
    eng.params_set(*start_state(D, F, D * F))
    reader = CopyReader(eng, D, F)
    dYd = None
    try:
        cfg = vv.StepConfig(1, 2, 1, lr=2.0 ** -3, momentum=0.5, weight_decay=2.0 ** -4)
        fol = Follower(eng, 0.5, F)
        for k in (1, 2, 3):
            dY = rng.integers(1, 3, size=(F, D)).astype(np.float32) * rng.choice([-1.0, 1.0], size=(F, D)).astype(np.float32)
            if dYd is None:
                dYd = eng.dev(dY)
            else:
                dYd.set(dY)
            operator_gradient(eng, reader, dYd, dY, F)
            eng.apply_update(cfg)
            assert int(eng.get_option("last_update_form")) == (1 if F % 4 == 0 else 2)
            fol.after_update("%d x %d = %d elements, update %d" % (D, F, D * F, k))
    finally:
        reader.free()
        if dYd is not None:
            dYd.free()
        eng.close()


@pytest.mark.parametrize("D,F,form", [(100, 128, 3), (30, 101, 2)])
def test_k_ema_every_decay_under_every_solver(vv, D, F, form):  # noqa: F811
    eng = step_engine(vv, form, D, F, start_state(D, F, 11))
    try:
        rng = np.random.default_rng(12)
        for solver in SOLVER_KW:
            cfg = step_cfg(vv, solver)
            eng.ema_set(-1)
            eng.params_set(*start_state(D, F, 11))                           # (a momentum history is signed: no start for AdaGrad's square root)
            for decay in (0.0, 0.5, 0.999):
                eng.ema_set(-1)                                              # off: the next activation starts from the current parameters
                assert eng.ema_stats() == {"updates": 0, "decay": np.float32(-1), "in_use": False}
                fol = Follower(eng, decay, F)
                for k in (1, 2, 3):
                    eng.forward_backward(cfg, rng.integers(0, ROWS, size=(B, C + NN)).astype(np.int32))
                    eng.apply_update(cfg)
                    assert int(eng.get_option("last_update_form")) == form
                    fol.after_update("%s, decay %g, %d x %d, update %d" % (solver, decay, D, F, k))
                if decay == 0.0:
                    assert np.array_equal(fol.eW, fol.W + np.float32(0))     # decay 0: the average is the weights (0 * e + 1 * w)
    finally:
        eng.close()


def test_k_ema_once_per_clipped_and_per_accumulated_update(vv):  # noqa: F811
    D, F = 100, 128
    eng = step_engine(vv, 1, D, F, start_state(D, F, 21))
    try:
        rng = np.random.default_rng(22)
        nxt = lambda: rng.integers(0, ROWS, size=(B, C + NN)).astype(np.int32)  # noqa: E731
        fol = Follower(eng, 0.5, F)
        cfg = step_cfg(vv, clip_gradients=1e-3)                              # (far below the gradient's norm: every update is clipped)
        for k in (1, 2, 3):
            eng.forward_backward(cfg, nxt())
            eng.apply_update(cfg)
            assert eng.clip_stats()["clipped"] == 1 and int(eng.get_option("last_update_form")) == 1
            fol.after_update("clipped update %d" % k)
        cfg = step_cfg(vv, clip_gradients=-1)
        for k in (1, 2, 3):
            for _ in range(3):                                               # three gradients banked, ONE update, ONE k_ema
                eng.forward_backward(cfg, nxt())
                eng.grads_bank()
            assert eng.ema_stats()["updates"] == fol.n
            eng.apply_update(cfg)
            assert eng.accum_stats()["last_count"] == 3 and int(eng.get_option("last_update_form")) == 1
            fol.after_update("accumulated update %d" % k)
        eng.ema_set(0.25)                                                    # another decay while active: the average is kept
        fol.decay = 0.25
        fol.check("after another decay")
        eng.forward_backward(cfg, nxt())
        eng.apply_update(cfg)
        fol.after_update("the update after another decay")
        W2, b2 = start_state(D, F, 23)[:2]
        eng.params_set(W2, b2)                                               # new parameters: the average starts again from them
        gW, gb = eng.ema_get()
        assert np.array_equal(gW, W2) and np.array_equal(gb, b2)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- training untouched
def run_training(vv, scenario, ema):  # noqa: F811
    form, D, F, solver = {"lazy": (3, 1028, 2048, "SGD"), "adam": (3, 100, 128, "ADAM"), "hinted": (5, 4090, 4092, "SGD")}[scenario]
    eng = step_engine(vv, form, D, F, start_state(D, F, 31))
    out = {}
    try:
        cfg = step_cfg(vv, solver)
        if ema:
            eng.ema_set(0.999)
        rng = np.random.default_rng(32)
        for k in (1, 2, 3):
            idx = rng.integers(0, ROWS, size=(B, C + NN)).astype(np.int32)
            if form == 5:
                eng.update_hint(cfg)
            eng.forward_backward(cfg, idx)
            eng.apply_update(cfg)
            assert int(eng.get_option("last_update_form")) == form
            out["loss%d" % k] = eng.loss()
            if form != 5:                                                    # (a hinted step never stores its gradient)
                out["grads%d" % k] = eng.grads()
        out["params"] = eng.params_get()
        if solver == "ADAM":
            out["hist2"] = eng.history2_get()
        out["copy"] = half_copy(eng, vv, F, D)
        if ema:
            assert eng.ema_stats()["updates"] == 3
            assert not np.array_equal(eng.ema_get()[0], out["params"][0])
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("scenario", ["lazy", "adam", "hinted"])
def test_training_is_untouched_by_the_average(vv, scenario):  # noqa: F811
    ref = run_training(vv, scenario, False)
    got = run_training(vv, scenario, True)
    same_tree(got, ref, scenario)


# ------------------------------------------------------------------------------- evaluation on the averaged parameters
def evaluate(eng, cfg, idx, rows, mean_rows):
    eng.eval_reset()
    eng.forward(cfg, idx)
    st = eng.eval_stats()
    out = dict(loss=(st.last_loss, st.last_violations, st.mean_loss, st.mean_violations, st.passes), form=int(eng.get_option("last_score_form")),
               **eng.blobs(cfg))
    out["embed"] = eng.embed(rows, relu=True, l2norm=True)
    out["embed_raw"] = eng.embed(rows, relu=False, l2norm=False)
    out["embed_mean"] = eng.embed_mean(mean_rows, coeff=[0.5, 0.25, 0.25])
    g = eng.gallery_from_table(mean_rows, ids=np.arange(len(mean_rows), dtype=np.int32))
    try:
        out["gallery_rows"] = g.rows()
        out["topk"] = g.topk(out["embed"][:40], 5)
    finally:
        g.close()
    return out


@pytest.mark.parametrize("name", ["f1_rpw2", "f4_dense"])
def test_evaluation_reads_the_average_and_leaves_training_alone(vv, world, name):  # noqa: F811
    D, Bf, Cf, Nf, form, dedup, seg_bwd = FORMS[name]
    cfg = vv.StepConfig(Bf, Cf, Nf, lr=0.05)
    batches = [batch(s, Bf, Cf, Nf) for s in (700, 701, 702)]
    held_out = batch(703, Bf, Cf, Nf)
    rows = np.arange(0, 300, dtype=np.int32)
    mean_rows = np.random.default_rng(704).integers(0, N_ROWS, size=(200, 3)).astype(np.int32)

    def trained(ema):
        e = fwd_engine(vv, world, D, dedup, seg_bwd)
        if ema:
            e.ema_set(0.9)
        for idx in batches[:2]:
            e.forward_backward(cfg, idx)
            e.apply_update(cfg)
        return e

    eng, twin, plain = trained(True), trained(True), trained(False)
    try:
        eW, eb = eng.ema_get()
        W, b, _, _ = eng.params_get()
        assert not np.array_equal(eW, W) and not np.array_equal(eW, world(D, N_ROWS)[1])
        twin.ema_set(-1)
        twin.params_set(eW, eb)
        want = evaluate(twin, cfg, held_out, rows, mean_rows)
        own = evaluate(eng, cfg, held_out, rows, mean_rows)                  # the training view: the last iterate
        with eng.ema():
            assert eng.ema_stats()["in_use"]
            got = evaluate(eng, cfg, held_out, rows, mean_rows)
            again = evaluate(eng, cfg, held_out, rows, mean_rows)            # (the cached 16-bit copy)
        assert not eng.ema_stats()["in_use"]
        assert got["form"] == form, "%s ran score form %d, written for %d" % (name, got["form"], form)
        same_tree(got, want, name + " under ema_use against the twin given params_set(ema_get())")
        same_tree(again, want, name + " a second time under ema_use")
        assert not np.array_equal(own["ip2"], got["ip2"]) and not np.array_equal(own["embed"], got["embed"])      # (the view did switch)
        same_tree(evaluate(eng, cfg, held_out, rows, mean_rows), own, name + " after ema_use(0)")
        # ... and the next training step is that of the run that never evaluated
        res = []
        for e in (eng, plain):
            e.forward_backward(cfg, batches[2])
            o = dict(loss=e.loss(), grads=e.grads())
            e.apply_update(cfg)
            o["params"] = e.params_get()
            o["copy"] = half_copy(e, vv, 128, D)
            res.append(o)
        same_tree(res[0], res[1], name + " the training step after ema_use(0)")
        assert eng.ema_stats()["updates"] == 3
    finally:
        for e in (eng, twin, plain):
            e.close()


# ------------------------------------------------------------------------------- the refusals
def raises(vv, code, fn, *a):  # noqa: F811
    with pytest.raises(vv.VVError) as err:
        fn(*a)
    assert "videovec error %d" % code in str(err.value), str(err.value)


def test_error_cases(vv, world):  # noqa: F811
    D, Bf, Cf, Nf = FORMS["f1_rpw2"][:4]
    cfg = vv.StepConfig(Bf, Cf, Nf, lr=0.01)
    idx = batch(800, Bf, Cf, Nf)
    table, W, b = world(D, N_ROWS)
    eng = vv.Engine(0, "f16")
    try:
        for bad in (float("nan"), 1.0, 1.5, float("inf")):
            raises(vv, VV_ERR_ARG, eng.ema_set, bad)
        raises(vv, VV_ERR_STATE, eng.ema_set, 0.9)                           # no parameters to start from
        eng.table_set(table)
        eng.params_set(W, b)
        assert eng.ema_stats() == {"updates": 0, "decay": np.float32(-1), "in_use": False}
        raises(vv, VV_ERR_STATE, eng.ema_get)                                # off
        raises(vv, VV_ERR_STATE, eng.ema_use, True)                          # off
        eng.ema_use(False)                                                   # (the training view is always allowed)
        eng.ema_set(0.9)
        for bad in (float("nan"), 1.0):
            raises(vv, VV_ERR_ARG, eng.ema_set, bad)
        assert eng.ema_stats()["decay"] == np.float32(0.9)                   # (a refused call changed nothing)
        eng.update_hint(cfg)
        eng.forward_backward(cfg, idx)
        raises(vv, VV_ERR_STATE, eng.ema_use, True)                          # between a hinted backward pass and its update
        eng.apply_update(cfg)
        assert eng.ema_stats()["updates"] == 1
        eng.forward_backward(cfg, idx)                                       # a gradient is held: the update is refused for the view, not for want of one
        eng.ema_use(True)
        raises(vv, VV_ERR_STATE, eng.forward_backward, cfg, idx)
        raises(vv, VV_ERR_STATE, eng.step, cfg, idx)
        assert eng.L.vv_step(eng.h, ctypes.byref(cfg.c), idx.ctypes.data_as(ctypes.c_void_p), 0) == VV_ERR_STATE      # (the ABI's own vv_step)
        raises(vv, VV_ERR_STATE, eng.apply_update, cfg)
        raises(vv, VV_ERR_STATE, eng.params_set, W, b)
        raises(vv, VV_ERR_STATE, eng.ema_set, -1)
        last = np.empty((Bf, Cf + Nf), np.int32)
        last[:] = idx
        raises(vv, VV_ERR_STATE, eng.forward_backward_q1, cfg, idx, last)
        eng.forward(cfg, idx)                                                # what the view is for
        eng.ema_use(False)
        assert eng.ema_stats()["updates"] == 1
        eng.apply_update(cfg)                                                # the held gradient is still there
        assert eng.ema_stats()["updates"] == 2
        eng.step(cfg, idx)
        assert eng.ema_stats()["updates"] == 3
        eng.ema_set(-1)
        raises(vv, VV_ERR_STATE, eng.ema_get)
    finally:
        eng.close()
