"""vv_debug_stats_queue / vv_debug_mark_update / vv_debug_stats_get (the reference's debug_info lines, net.cpp:580-636) on the fused
training step, against numpy float64 of what the existing accessors return.

Every value is held to the accessor's array summed in float64: (float)asum within 1 ulp of float32(float64 sum) -- the bound derived in
tests/test_gpu_abs_stats.py (b): both sums add n <= 2^24 non-negative doubles, each within 2^-29 of the true sum, and are rounded to fp32
once -- amax and count exact, nonfinite 0.  Shapes: D = 512 with B, C, Nn = 32, 5, 4 as the other exact tests use, F = 256 (16-byte form of
the update) and F = 101 (F % 4 != 0: update form 2, a gradient buffer of D F + D = 52 224 floats whose db starts off a 16-byte boundary
where the buffer is bound one float past one).

  W / B / HIST     against params_get
  DW / DB          against grads_get: lazily reduced (queued first, read after) and once more after grads_get; a bound buffer one float past
                   a boundary; under clipping (the clipped buffer after the update); with a banked gradient (the normalised buffer)
  scores           against blobs_get, de-duplication on and off, h16 on and off, bf16
  UPD_W / UPD_B    against float32(W_before - W_after) of two params_get calls, summed in float64, for all five solver rules
  VV_ERR_STATE     every case of include/videovec.h
  twin             a run that queues every entry each step is bit-equal to one that queues none (parameters, histories, loss, gradients):
                   Adam, a hinted step around which only non-gradient entries are queued, f16 slabs, bf16
  divergence       an Inf planted in W shows in W's nonfinite and nowhere else

Without the feature the binding has no debug_stats_queue: every case fails.
"""
import numpy as np
import pytest

from tests.test_gpu_clip_gradients import make_rule
from tests.test_gpu_parity import vv  # noqa: F401  (fixture)
from tests.test_gpu_update_adam_rmsprop import read_state, start_state

pytestmark = pytest.mark.gpu

VV_ERR_ARG, VV_ERR_STATE = 1, 3
B, C, Nn, N_ROWS = 32, 5, 4, 3000
D = 512
PARAMS = ["W", "B", "HIST_W", "HIST_B"]
GRADS = ["DW", "DB"]
SCORES = ["TARGET_SCORE", "NEGATIVE_SCORES"]
UPD = ["UPD_W", "UPD_B"]


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    assert a >= 0 and b >= 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def check(stat, ref, what):
    """stat = (asum, amax, count, nonfinite) against the array ref in float64"""
    a = np.abs(ref.astype(np.float64))
    print("%s: asum %r against float64 %r, amax %r against %r" % (what, stat[0], float(a.sum()), stat[1], a.max()))
    assert np.isfinite(ref).all()
    assert ulps(np.float32(stat[0]), np.float32(a.sum())) <= 1, what
    assert stat[1] == np.float32(a.max()) and stat[2] == ref.size and stat[3] == 0, what


class Run:
    def __init__(self, vv, F=256, solver="SGD", prec="f16", dedup=False, opts=(), D_=D, seed=0):  # noqa: F811
        self.vv, self.D, self.F, self.adam = vv, D_, F, solver == "ADAM"
        self.rng = np.random.default_rng(D_ + F + seed)
        self.st = start_state(self.rng, D_, F)
        self.rule = make_rule(solver)
        self.cfg = self.rule.cfg(vv, B, C, Nn)
        self.prec, self.dedup, self.opts, self.solver = prec, dedup, dict(opts), solver
        self.engs, self.bufs = [], []

    def engine(self):
        e = self.vv.Engine(0, self.prec)
        e.set_dedup(self.dedup)
        for k, v in self.opts.items():
            e.set_option(k, v)
        e.table_synth(7, N_ROWS, self.F)
        st = self.st
        e.params_set(*(st[:4] if self.adam else (st[0], st[1], st[4], st[5])))      # (RMSProp / AdaGrad: the non-negative history)
        if self.adam:
            e.history2_set(st[4], st[5])
        self.engs.append(e)
        return e

    def batch(self):
        return self.rng.integers(0, N_ROWS, size=(B, C + Nn)).astype(np.int32)

    def bind_offset(self, e):
        buf = e.dev((self.D * self.F + self.D + 8,))
        self.bufs.append(buf)
        assert buf.ptr.value % 16 == 0
        e.grads_bind(buf.ptr.value + 4)

    def close(self):
        for b_ in self.bufs:
            b_.free()
        for e in self.engs:
            e.close()


@pytest.fixture
def run(vv, request):  # noqa: F811
    made = []

    def make(**kw):
        made.append(Run(vv, **kw))
        return made[-1]
    yield make
    for r in made:
        r.close()


def state_error(vv, fn, *args):  # noqa: F811
    with pytest.raises(vv.VVError) as err:
        fn(*args)
    assert "videovec error %d" % VV_ERR_STATE in str(err.value), str(err.value)
    return str(err.value)


# ------------------------------------------------------------------------------- W / B / HIST
@pytest.mark.parametrize("F", [256, 101])
def test_parameters_and_histories_against_params_get(run, F):
    r = run(F=F)
    e = r.engine()
    for _ in range(2):
        e.forward_backward(r.cfg, r.batch())
        e.apply_update(r.cfg)
    assert int(e.get_option("last_update_form")) in ((2,) if F % 4 else (1, 3, 4))
    e.debug_stats_queue(PARAMS)
    s = e.debug_stats()
    for name, ref in zip(PARAMS, e.params_get()):
        check(s[name], ref, "%s at F = %d" % (name, F))
    for name in GRADS + SCORES + UPD:
        assert s[name] == (0.0, np.float32(0), 0, 0), "an entry never queued reads all-zero"


# ------------------------------------------------------------------------------- DW / DB
@pytest.mark.parametrize("F,bound", [(256, False), (101, False), (256, True), (101, True)])
def test_gradient_lazily_reduced_and_after_grads_get(run, F, bound):
    r = run(F=F)
    e = r.engine()
    if bound:
        r.bind_offset(e)
    e.forward_backward(r.cfg, r.batch())
    e.debug_stats_queue(GRADS)               # the reduction is still due: the queue brings the gradient into the buffer
    s = e.debug_stats()
    dW, db = e.grads()
    check(s["DW"], dW, "DW, lazily reduced")
    check(s["DB"], db, "DB, lazily reduced")
    e.debug_stats_queue(GRADS)
    assert e.debug_stats() == s, "the same buffer gives the same bits"
    e.apply_update(r.cfg)
    e.debug_stats_queue(GRADS)               # (an un-hinted step keeps its gradient)
    assert e.debug_stats() == s
    assert all(np.array_equal(a, b_) for a, b_ in zip(e.grads(), (dW, db)))


@pytest.mark.parametrize("F", [256, 101])
def test_gradient_under_clipping(run, F):
    r = run(F=F)
    e = r.engine()
    e.forward_backward(r.cfg, r.batch())
    dW, db = e.grads()
    norm = float(np.sqrt((dW.astype(np.float64) ** 2).sum() + (db.astype(np.float64) ** 2).sum()))
    e.clip_gradients_set(norm / 3)
    e.debug_stats_queue(GRADS)
    before = e.debug_stats()
    e.apply_update(r.cfg)
    e.debug_stats_queue(GRADS)
    s = e.debug_stats()
    assert e.clip_stats()["clipped"] == 1
    cW, cb = e.grads()
    check(before["DW"], dW, "DW in front of the clipping update")
    check(s["DW"], cW, "DW, clipped")
    check(s["DB"], cb, "DB, clipped")
    assert s["DW"][0] < 0.5 * before["DW"][0]


def test_gradient_banked(run):
    r = run(F=101)
    e = r.engine()
    for _ in range(3):
        e.forward_backward(r.cfg, r.batch())
        e.debug_stats_queue(GRADS)           # the last micro-batch's gradient
        last = e.grads()
        e.grads_bank()
    s = e.debug_stats()
    check(s["DW"], last[0], "DW of the last micro-batch")
    check(s["DB"], last[1], "DB of the last micro-batch")
    e.apply_update(r.cfg)
    e.debug_stats_queue(GRADS)               # the normalised sum the accumulated update consumed
    s = e.debug_stats()
    nW, nb = e.grads()
    assert not np.array_equal(nW, last[0])
    check(s["DW"], nW, "DW, accumulated and normalised")
    check(s["DB"], nb, "DB, accumulated and normalised")


# ------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("prec,dedup,h16", [("f16", True, 1), ("f16", True, 0), ("f16", False, 1), ("bf16", True, 1), ("bf16", False, 0)])
def test_scores_against_blobs_get(run, prec, dedup, h16):
    r = run(prec=prec, dedup=dedup, opts={"h16": h16})
    e = r.engine()
    e.forward_backward(r.cfg, r.batch())
    e.debug_stats_queue(SCORES)
    s = e.debug_stats()
    bl = e.blobs(r.cfg, ip2=False)
    st, sn = bl["target_score"], bl["negative_scores"]
    assert (st == st[:, :1]).all()           # (the blob repeats an item's score Nn times; the library holds it once)
    check(s["TARGET_SCORE"], st[:, 0], "target_score (%s, dedup %d, h16 %d)" % (prec, dedup, h16))
    check(s["NEGATIVE_SCORES"], sn, "negative_scores (%s, dedup %d, h16 %d)" % (prec, dedup, h16))
    e.forward(r.cfg, r.batch())              # the forward-only pass: its scores
    e.debug_stats_queue(SCORES)
    s2 = e.debug_stats()
    bl = e.blobs(r.cfg, ip2=False)
    check(s2["TARGET_SCORE"], bl["target_score"][:, 0], "target_score of a forward-only pass")
    check(s2["NEGATIVE_SCORES"], bl["negative_scores"], "negative_scores of a forward-only pass")


# ------------------------------------------------------------------------------- UPD_W / UPD_B
@pytest.mark.parametrize("solver,F,hinted", [("SGD", 256, False), ("NESTEROV", 256, False), ("ADAGRAD", 256, False), ("RMSPROP", 256, False),
                                             ("ADAM", 256, False), ("SGD", 101, False), ("ADAM", 101, False), ("SGD", 256, True)])
def test_update_against_the_difference_of_two_params_get(run, solver, F, hinted):
    r = run(F=F, solver=solver)
    e = r.engine()
    for it in range(2):
        W0, b0 = e.params_get()[:2]
        e.debug_mark_update()
        if hinted:
            e.step(r.cfg, r.batch())
        else:
            e.forward_backward(r.cfg, r.batch())
            e.apply_update(r.cfg)
        e.debug_stats_queue(UPD)
        s = e.debug_stats()
        W1, b1 = e.params_get()[:2]
        uW, ub = W0 - W1, b0 - b1            # float32: one subtraction per element
        assert uW.dtype == np.float32 and (uW != 0).mean() > 0.99
        what = "%s, F = %d, update %d (form %d)" % (solver, F, it + 1, int(e.get_option("last_update_form")))
        check(s["UPD_W"], uW, "UPD_W, " + what)
        check(s["UPD_B"], ub, "UPD_B, " + what)


# ------------------------------------------------------------------------------- VV_ERR_STATE
def test_state_errors(run, vv):  # noqa: F811
    r = run()
    e = r.engine()
    assert "backward" in state_error(vv, e.debug_stats_queue, "DW")
    assert "backward" in state_error(vv, e.debug_stats_queue, GRADS + PARAMS)
    assert "forward" in state_error(vv, e.debug_stats_queue, "TARGET_SCORE")
    assert "forward" in state_error(vv, e.debug_stats_queue, "NEGATIVE_SCORES")
    assert "vv_debug_mark_update" in state_error(vv, e.debug_stats_queue, "UPD_W")
    assert "vv_debug_mark_update" in state_error(vv, e.debug_stats_queue, "UPD_B")
    e.debug_stats_queue(PARAMS)              # parameters exist: allowed
    # a step announced by vv_update_hint: between its backward pass and its update, and after it
    e.debug_mark_update()
    e.update_hint(r.cfg)
    e.forward_backward(r.cfg, r.batch())
    for names in ("DW", "DB", GRADS + SCORES):
        assert "vv_update_hint" in state_error(vv, e.debug_stats_queue, names)
    e.debug_stats_queue(SCORES)
    e.apply_update(r.cfg)
    for names in ("DW", "DB"):
        assert "vv_update_hint" in state_error(vv, e.debug_stats_queue, names)
    e.debug_stats_queue(PARAMS + SCORES + UPD)
    # ... and the next un-hinted pass has a gradient again
    e.forward_backward(r.cfg, r.batch())
    e.debug_stats_queue(GRADS)
    # new parameters: the mark and the gradient go with the old ones
    e.params_set(*r.st[:4])
    assert "vv_debug_mark_update" in state_error(vv, e.debug_stats_queue, "UPD_W")
    assert "backward" in state_error(vv, e.debug_stats_queue, "DW")
    # arguments
    for mask in (0, 1 << 10, 0xFFFFFFFF):
        assert e.L.vv_debug_stats_queue(e.h, mask) == VV_ERR_ARG
    with pytest.raises(vv.VVError):
        e.debug_stats_queue("dW")


def test_state_errors_without_parameters(vv):  # noqa: F811
    e = vv.Engine(0, "f16")
    try:
        e.table_synth(7, N_ROWS, 64)
        assert all(v == (0.0, np.float32(0), 0, 0) for v in e.debug_stats().values())
        state_error(vv, e.debug_stats_queue, "W")
        state_error(vv, e.debug_mark_update)
    finally:
        e.close()


def test_sharded_schedule_refuses_the_master_copy(run, vv):  # noqa: F811
    """while schedule 2 is selected: W / history / UPD entries and the mark are refused, b is not (the selection alone decides: no communicator)"""
    r = run()
    e = r.engine()
    e.comm_schedule("sharded")
    for names in ("W", "HIST_W", "HIST_B"):
        assert "sharded" in state_error(vv, e.debug_stats_queue, names)
    assert "sharded" in state_error(vv, e.debug_mark_update)
    e.debug_stats_queue("B")
    e.comm_schedule("sync")
    e.debug_stats_queue(PARAMS)


# ------------------------------------------------------------------------------- the twin
def queueing_step(r, e, idx, hinted):
    if hinted:                               # only non-gradient entries around a hinted step
        e.debug_mark_update()
        e.step(r.cfg, idx)
        e.debug_stats_queue(PARAMS + SCORES + UPD)
        return
    e.forward_backward(r.cfg, idx)
    e.debug_stats_queue(SCORES + GRADS + PARAMS)
    e.debug_mark_update()
    e.apply_update(r.cfg)
    e.debug_stats_queue(PARAMS + GRADS + SCORES + UPD)      # all ten: two launches


@pytest.mark.parametrize("solver,prec,hinted,D_,F,opts", [
    ("ADAM", "f16", False, 512, 256, {}), ("ADAM", "f16", False, 512, 101, {}), ("SGD", "f16", True, 512, 256, {}),
    ("SGD", "f16", True, 4090, 4092, {"wgrad_update": 1}),                  # the update in the weight-gradient GEMM's epilogue (form 5)
    ("SGD", "f16", False, 1028, 4096, {"slab16": 1}),                        # f16 slabs (form 4 in the twin)
    ("RMSPROP", "bf16", False, 512, 256, {}), ("SGD", "f16", False, 512, 256, {"fuse_update": 0})])
def test_a_run_that_queues_everything_is_bit_equal_to_one_that_queues_nothing(run, solver, prec, hinted, D_, F, opts):
    r = run(F=F, solver=solver, prec=prec, opts=opts, D_=D_)
    eng, twin = r.engine(), r.engine()
    for it in range(3):
        idx = r.batch()
        if hinted:
            twin.step(r.cfg, idx)
        else:
            twin.forward_backward(r.cfg, idx)
            twin.apply_update(r.cfg)
        queueing_step(r, eng, idx, hinted)
        what = "%s %s %d x %d, step %d (forms %d / %d)" % (solver, prec, D_, F, it + 1, int(eng.get_option("last_update_form")),
                                                           int(twin.get_option("last_update_form")))
        s = eng.debug_stats()
        assert s["W"][2] == D_ * F and s["UPD_W"][0] > 0 and all(v[3] == 0 for v in s.values()), what
        assert np.float32(eng.loss()[0]).view(np.uint32) == np.float32(twin.loss()[0]).view(np.uint32) and eng.loss()[1] == twin.loss()[1], what
        for name, a, t in zip(("W", "b", "hW", "hb", "vW", "vb"), read_state(eng, r.adam), read_state(twin, r.adam)):
            assert a is None or np.array_equal(a.view(np.uint32), t.view(np.uint32)), "%s: %s differs from the twin's" % (what, name)
        if not hinted:
            for name, a, t in zip(("dW", "db"), eng.grads(), twin.grads()):
                assert np.array_equal(a.view(np.uint32), t.view(np.uint32)), "%s: %s differs from the twin's" % (what, name)


# ------------------------------------------------------------------------------- divergence
def test_a_planted_inf_shows_in_nonfinite_only(run):
    r = run()
    e = r.engine()
    W = r.st[0].copy()
    W[3, 5], W[400, 255] = np.inf, np.nan
    e.params_set(W, r.st[1], r.st[2], r.st[3])
    e.debug_stats_queue(PARAMS)
    s = e.debug_stats()
    fin = np.abs(W[np.isfinite(W)].astype(np.float64))
    assert s["W"][3] == 2 and s["W"][2] == W.size and s["W"][1] == np.float32(fin.max())
    assert ulps(np.float32(s["W"][0]), np.float32(fin.sum())) <= 1
    for name, ref in zip(PARAMS[1:], (r.st[1], r.st[2], r.st[3])):
        check(s[name], ref, name + " beside a non-finite W")
