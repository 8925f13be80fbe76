"""Gradient accumulation (vv_grads_bank / vv_grads_bank_reset / vv_accum_stats; BVLC Caffe's SolverParameter.iter_size, Solver::Step and
SGDSolver::Normalize -- the reference tree has no iter_size), bit for bit against a numpy-float32 restatement and, for the parameters,
against the float64 rules of tests/test_gpu_update_exact.py and tests/test_gpu_update_adam_rmsprop.py.

A cycle: m x (forward_backward, grads_bank), then apply_update.  Each micro-batch's gradient is read with vv_grads_get BEFORE it is banked
(a twin that reads nothing in between must end bit-equal), and the cycle is restated as the header states it:
    acc = g1;  acc = acc + gk (k = 2 .. m, float32, in banking order);  acc * (float32(1) / float32(m))
-- with clipping, float32(float32(acc * scale) * inv).  After the update vv_grads_get must return exactly those bits (uint32 views).
The parameters and histories are then held to the float64 rule applied to the GPU's own w, h and THAT gradient, with the bounds and the
operation counts the two existing files derive (imported; tests/test_gpu_clip_gradients.py's check_rule dispatches between them).

Shapes, the smallest that reach each edge (D, F; n = D F + D floats in the flat buffer):
  130 x 256     n = 33 410: the 16-byte form of k_sgd (form 1), less than one pass of k_grad_bank's grid, a scalar tail of 2
  31 x 101      n = 3 162, not a multiple of 4, F % 4 != 0: form 2
  1028 x 4096   n = 4 214 788 = 1 053 697 16-byte items: past one pass of k_grad_bank's BANK_GRID_THREADS = 1024 x 256 = 262 144 threads
                (four full passes and a fifth); the shape the plain update runs form 4 at (fused, f16 slabs): the bank takes the gradient
                out of the slabs as a reader does, the accumulated update runs form 1
  130 x 256 with a bound buffer that starts one float past a 16-byte boundary: 3 scalar floats in front, 8 351 items, 3 behind
m: 1 (inv = 1: must equal a plain update bit for bit), 2 and 8 (inv exact), 3 (1 / 3 is inexact).

Meaning: two micro-batches of B items, each normalised by the 2 B Nn terms of the whole (global_count), accumulate to half the gradient
of the concatenated 2 B-item batch: 2 x the normalised sum against the oracle's dW of that batch, at tests/test_gpu_parity.py's smallest
shape (its config-1 case) with de-duplication on, within the two bounds that file holds a single step's dW to there (TOL: grad_q against
the oracle on the rounded operands, grad against the fp32-operand oracle).  The bounds are taken from that file.

Without the feature the binding has no grads_bank: every case fails.
"""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_clip_gradients import check_rule, make_rule, norm64, ulps
from tests.test_gpu_parity import TOL, make_case, rel_fro, round_operand, round_table, vv  # noqa: F401  (fixture)
from tests.test_gpu_update_adam_rmsprop import SHAPE, engine_for, read_state, start_state

pytestmark = pytest.mark.gpu

VV_ERR_STATE = 3
B, C, Nn, N_ROWS = 32, 5, 4, 3000
BANK_GRID_THREADS = 1024 * 256           # vv_internal.h: BANK_BLOCKS workgroups of 256 threads, one 16-byte item per thread and pass
ODD = (31, 101)


def bits_equal(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def restate(gs, scale=None):
    """the cycle in numpy float32 -> (sum dW, sum db, normalised dW, normalised db, inv)"""
    inv = np.float32(1) / np.float32(len(gs))
    sW, sb = gs[0][0].copy(), gs[0][1].copy()
    for gW, gb in gs[1:]:
        sW, sb = sW + gW, sb + gb
    cW, cb = (sW, sb) if scale is None else (sW * np.float32(scale), sb * np.float32(scale))
    out = cW * inv, cb * inv
    assert all(a.dtype == np.float32 for a in (sW, sb) + out)
    return sW, sb, out[0], out[1], inv


def restate_means(ls):
    inv = np.float32(1) / np.float32(len(ls))
    sl, sv = np.float32(ls[0][0]), np.float32(ls[0][1])
    for l, v in ls[1:]:
        sl, sv = sl + np.float32(l), sv + np.float32(v)
    return sl * inv, sv * inv


def cycle(eng, cfg, batches, read=True, before_update=None):
    gs, ls = [], []
    for idx in batches:
        eng.forward_backward(cfg, idx)
        if read:
            gs.append(eng.grads())
            ls.append(eng.loss())
        eng.grads_bank()
        if read:
            assert eng.accum_stats()["banked"] == len(gs)
    if before_update is not None:
        before_update(gs)
    eng.apply_update(cfg)
    return gs, ls


def assert_form(eng, F, what):
    form = int(eng.get_option("last_update_form"))
    assert form in (1, 2) and form == (2 if F % 4 else 1), "%s: the accumulated update ran form %d" % (what, form)


def batches_of(rng, m):
    return [rng.integers(0, N_ROWS, size=(B, C + Nn)).astype(np.int32) for _ in range(m)]


class Engines:
    def __init__(self):
        self.all, self.bufs = [], []

    def make(self, vv, form, D, F, st, solver="SGD", prec="f16"):  # noqa: F811
        e = engine_for(vv, prec, form, D, F, N_ROWS, st, solver)
        self.all.append(e)
        return e

    def bind_offset(self, eng, D, F):
        """a gradient buffer that starts one float past a 16-byte boundary"""
        buf = eng.dev((D * F + D + 8,))
        self.bufs.append(buf)
        assert buf.ptr.value % 16 == 0
        eng.grads_bind(buf.ptr.value + 4)

    def close(self):
        for b_ in self.bufs:
            b_.free()
        for e in self.all:
            e.close()


# ------------------------------------------------------------------------------- the bank, bit for bit; the twin; the parameters
# (form of make_engine's options, D, F, m, bound buffer)
BANK_CASES = [(1, 130, 256, 1, False), (1, 130, 256, 2, False), (1, 130, 256, 3, False), (1, 130, 256, 8, False),
              (1, ODD[0], ODD[1], 3, False), (4, 1028, 4096, 3, False), (1, 130, 256, 3, True), (3, 100, 128, 2, False)]


@pytest.mark.parametrize("form,D,F,m,bound", BANK_CASES)
def test_bank_bit_for_bit_and_twin(vv, form, D, F, m, bound):  # noqa: F811
    rng = np.random.default_rng(D + F + m)
    st = start_state(rng, D, F)
    rule = make_rule("SGD")
    cfg = rule.cfg(vv, B, C, Nn)
    es = Engines()
    try:
        eng, twin = es.make(vv, form, D, F, st), es.make(vv, form, D, F, st)
        if bound:
            es.bind_offset(eng, D, F)
            es.bind_offset(twin, D, F)
        n = D * F + D
        if (D, F) == ODD:
            assert n % 4 != 0
        if D == 1028:
            assert n // 4 > 4 * BANK_GRID_THREADS, "the case must go past one pass of k_grad_bank's grid"
        what = "%d x %d, m = %d%s" % (D, F, m, ", bound buffer" if bound else "")
        bt = batches_of(rng, m)
        before = read_state(eng, False)
        gs, ls = cycle(eng, cfg, bt)
        cycle(twin, cfg, bt, read=False)                   # never reads the gradient (nor the loss) between backward and bank
        assert_form(eng, F, what)
        assert_form(twin, F, what + " (twin)")
        sW, sb, nW, nb, inv = restate(gs)
        assert (np.float64(inv) * m == 1.0) == (m in (1, 2, 8))       # (1 / 3 is inexact in float32)
        gW, gb = eng.grads()
        assert bits_equal(gW, nW) and bits_equal(gb, nb), what + ": vv_grads_get after the update is not (g1 + ... + gm) * (1 / m) in float32"
        tW, tb = twin.grads()
        assert bits_equal(tW, nW) and bits_equal(tb, nb), what + ": the twin's buffer differs"
        after = read_state(eng, False)
        for name, a, t in zip(("W", "b", "hW", "hb"), after, read_state(twin, False)):
            assert bits_equal(a, t), "%s: %s differs from the twin that never read its gradient" % (what, name)
        check_rule(rule, before, after, nW, nb, 1, what)
        s = eng.accum_stats()
        ml, mv = restate_means(ls)
        assert (s["banked"], s["last_count"], s["updates"]) == (0, m, 1)
        assert s["last_mean_loss"] == ml and s["last_mean_violations"] == mv, (s, ml, mv)
        assert twin.accum_stats() == s
    finally:
        es.close()


@pytest.mark.parametrize("form,D,F", [(1, 130, 256), (4, 1028, 4096), (1, ODD[0], ODD[1])])
def test_one_banked_gradient_is_the_plain_update(vv, form, D, F):  # noqa: F811
    rng = np.random.default_rng(D + F)
    st = start_state(rng, D, F)
    cfg = make_rule("SGD").cfg(vv, B, C, Nn)
    es = Engines()
    try:
        eng, plain = es.make(vv, form, D, F, st), es.make(vv, form, D, F, st)
        other, idx = batches_of(rng, 2)
        eng.forward_backward(cfg, other)                   # a second forward_backward without banking replaces the gradient
        eng.forward_backward(cfg, idx)
        eng.grads_bank()
        eng.apply_update(cfg)
        plain.forward_backward(cfg, idx)
        plain.apply_update(cfg)
        assert_form(eng, F, "m = 1")
        assert int(plain.get_option("last_update_form")) == (2 if F % 4 else form)
        for name, a, t in zip(("W", "b", "hW", "hb"), read_state(eng, False), read_state(plain, False)):
            assert bits_equal(a, t), "%d x %d: %s after one banked gradient differs from the plain update's" % (D, F, name)
        assert (eng.params_get()[0] != st[0]).mean() > 0.99
        for a, t in zip(eng.grads(), plain.grads()):
            assert bits_equal(a, t)
    finally:
        es.close()


@pytest.mark.parametrize("solver", ["SGD", "NESTEROV", "ADAGRAD", "RMSPROP", "ADAM"])
def test_every_rule_on_the_accumulated_gradient(vv, solver):  # noqa: F811
    D, F = SHAPE[1]
    adam = solver == "ADAM"
    rng = np.random.default_rng(len(solver))
    st = start_state(rng, D, F)
    rule = make_rule(solver)
    cfg = rule.cfg(vv, B, C, Nn)
    es = Engines()
    try:
        eng = es.make(vv, 1, D, F, st, solver)
        for t in (1, 2) if adam else (1,):                 # Adam over two cycles: t counts updates, not passes
            what = "%s, cycle %d" % (solver, t)
            before = read_state(eng, adam)
            gs, _ = cycle(eng, cfg, batches_of(rng, 2))
            assert_form(eng, F, what)
            _, _, nW, nb, _ = restate(gs)
            gW, gb = eng.grads()
            assert bits_equal(gW, nW) and bits_equal(gb, nb)
            if adam:
                assert eng.solver_iter == t
            check_rule(rule, before, read_state(eng, adam), nW, nb, t, what)
            assert eng.accum_stats()["updates"] == t
    finally:
        es.close()


# ------------------------------------------------------------------------------- clipping takes the norm of the SUM
@pytest.mark.parametrize("D,F", [(130, 256), ODD])
def test_clipping_sees_the_sum(vv, D, F):  # noqa: F811
    m = 3
    rng = np.random.default_rng(D * F)
    st = start_state(rng, D, F)
    rule = make_rule("SGD")
    cfg = rule.cfg(vv, B, C, Nn)
    es = Engines()
    try:
        eng = es.make(vv, 1, D, F, st)
        before = read_state(eng, False)
        clip = []

        def set_threshold(gs):
            sW, sb = restate(gs)[:2]
            clip.append(np.float32(norm64(sW, sb) / 3.0))
            eng.clip_gradients_set(clip[0])

        gs, _ = cycle(eng, cfg, batches_of(rng, m), before_update=set_threshold)
        assert_form(eng, F, "clipped")
        s = eng.clip_stats()
        sW, sb = restate(gs)[:2]
        nW, nb = restate(gs, s["scale"])[2:4]
        assert s["clipped"] == 1 and s["updates"] == 1
        # (1 ulp: tests/test_gpu_clip_gradients.py derives it; the norm of the MEAN would be a third of this one)
        assert ulps(s["norm"], np.float32(norm64(sW, sb))) <= 1, "the norm is not that of the sum: %r against %r" % (float(s["norm"]), norm64(sW, sb))
        assert ulps(s["scale"], np.float32(np.float64(clip[0]) / np.float64(s["norm"]))) <= 1
        gW, gb = eng.grads()
        assert bits_equal(gW, nW) and bits_equal(gb, nb), "the buffer is not float32(float32(sum * scale) * inv)"
        check_rule(rule, before, read_state(eng, False), nW, nb, 1, "clipped, %d x %d" % (D, F))
    finally:
        es.close()


# ------------------------------------------------------------------------------- bookkeeping
def state_error(vv, fn, word=None):  # noqa: F811
    with pytest.raises(vv.VVError) as err:
        fn()
    assert "videovec error %d" % VV_ERR_STATE in str(err.value), str(err.value)
    assert word is None or word in str(err.value), str(err.value)


def test_state_errors_and_the_hint(vv):  # noqa: F811
    D, F = SHAPE[3]
    rng = np.random.default_rng(9)
    st = start_state(rng, D, F)
    cfg = make_rule("SGD").cfg(vv, B, C, Nn)
    es = Engines()
    try:
        eng = es.make(vv, 3, D, F, st)
        idx = batches_of(rng, 1)[0]
        assert eng.accum_stats() == {"banked": 0, "last_count": 0, "last_mean_loss": 0.0, "last_mean_violations": 0.0, "updates": 0}
        state_error(vv, eng.grads_bank, "no backward pass")                        # before any backward pass
        eng.forward_backward(cfg, idx)
        eng.grads_bank()
        state_error(vv, eng.grads_bank, "already")                                 # twice for one backward pass
        eng.apply_update(cfg)
        state_error(vv, eng.grads_bank)                                            # ... nor the normalised buffer in its place
        eng.update_hint(cfg)                                                       # a step announced by vv_update_hint
        eng.forward_backward(cfg, idx)
        state_error(vv, eng.grads_bank, "vv_update_hint")
        eng.apply_update(cfg)
        eng.step(cfg, idx)
        state_error(vv, eng.grads_bank, "vv_update_hint")
        for sched in ("overlap", "sharded"):                                       # while schedule 1 or 2 is selected
            eng.comm_schedule(sched)
            eng.forward_backward(cfg, idx)
            state_error(vv, eng.grads_bank, "sync")
        eng.comm_schedule("sync")
        eng.forward_backward(cfg, idx)
        eng.grads_bank()
        assert eng.accum_stats()["banked"] == 1
        state_error(vv, lambda: eng.comm_schedule("overlap"), "sync")              # while the bank is non-empty
        state_error(vv, lambda: eng.comm_schedule("sharded"), "sync")
        state_error(vv, lambda: eng.comm_overlap(True), "sync")
        eng.forward_backward(cfg, idx)                                             # the last backward's gradient not banked
        state_error(vv, lambda: eng.apply_update(cfg), "banked")
        rc = eng.L.vv_step(eng.h, ctypes.byref(cfg.c), idx.ctypes.data_as(ctypes.c_void_p), 0)  # (Engine.step spells vv_step out: the entry point itself)
        assert rc == VV_ERR_STATE and b"banked" in eng.L.vv_last_error()
        W0 = eng.params_get()[0]
        eng.update_hint(cfg)                                                       # announces nothing while the bank is non-empty
        eng.forward_backward(cfg, idx)
        eng.grads_bank()
        eng.apply_update(cfg)
        assert_form(eng, F, "after a hint that announced nothing")
        s = eng.accum_stats()
        assert (s["banked"], s["last_count"]) == (0, 2)
        assert (eng.params_get()[0] != W0).mean() > 0.99
    finally:
        es.close()


@pytest.mark.parametrize("how", ["reset", "params_set"])
def test_after_a_reset_a_plain_step_is_a_fresh_engines(vv, how):  # noqa: F811
    D, F = SHAPE[1]
    rng = np.random.default_rng(17)
    st = start_state(rng, D, F)
    cfg = make_rule("SGD").cfg(vv, B, C, Nn)
    es = Engines()
    try:
        eng, fresh = es.make(vv, 1, D, F, st), es.make(vv, 1, D, F, st)
        a, b_ = batches_of(rng, 2)
        eng.forward_backward(cfg, a)
        eng.grads_bank()
        if how == "reset":
            eng.grads_bank_reset()
        else:
            eng.params_set(st[0], st[1], st[4], st[5])      # (engine_for's start for a one-history rule)
        assert eng.accum_stats()["banked"] == 0
        for e in (eng, fresh):
            e.forward_backward(cfg, b_)
            e.apply_update(cfg)
        assert_form(eng, F, how)
        for name, x, y in zip(("W", "b", "hW", "hb"), read_state(eng, False), read_state(fresh, False)):
            assert bits_equal(x, y), "after %s: %s differs from a fresh engine's" % (how, name)
        assert (eng.params_get()[0] != st[0]).mean() > 0.99
        assert eng.accum_stats()["updates"] == 0, "a plain update is not an accumulated one"
    finally:
        es.close()


# ------------------------------------------------------------------------------- meaning
def test_two_micro_batches_are_the_concatenated_batch(vv, oracle):  # noqa: F811
    Bm, Cm, Nm, Fm, Dm = 32, 5, 2, 128, 32                 # tests/test_gpu_parity.py::test_config1_plumbing_shapes, its smallest
    ds, table, idx, W, b = make_case(3, 50, 2 * Bm, Cm, Nm, Fm, Dm, wstd=0.02)
    eng = vv.Engine(0, "f16")
    try:
        eng.set_dedup(True)
        eng.table_set(table)
        eng.params_set(W, b)
        cfg = vv.StepConfig(Bm, Cm, Nm, global_count=2 * Bm * Nm, lr=0.01)
        gs, _ = cycle(eng, cfg, [idx[:Bm], idx[Bm:]])
        assert_form(eng, Fm, "meaning")
        assert (eng.params_get()[0] != W).mean() > 0.99
        nW, nb = eng.grads()
        assert bits_equal(nW, restate(gs)[2])
        okw = dict(C_=Cm, Nn=Nm, want=("dW", "db"))
        ref = oracle.forward_backward(table, idx, W, b, **okw)
        q = oracle.forward_backward(round_table(table, "f16"), idx, round_operand(W, "f16"), b, **okw)
        dq, d = rel_fro(2 * nW, q["dW"]), rel_fro(2 * nW, ref["dW"])
        print("2 x accumulated dW against the 2B-item oracle: rounded operands %.3e (bound %g), fp32 operands %.3e (bound %g)"
              % (dq, TOL["f16"]["grad_q"], d, TOL["f16"]["grad"]))
        assert dq <= TOL["f16"]["grad_q"] and d <= TOL["f16"]["grad"]
        assert rel_fro(2 * nb, q["db"]) <= TOL["f16"]["grad_q"]
    finally:
        eng.close()
