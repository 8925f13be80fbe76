"""The forward-only pass (vv_forward, vv_eval_reset, vv_eval_stats; Engine.forward / eval_reset / eval_stats).

  bit equality   for equal weights, idx and cfg the pass's loss, violations, ip2 and both score blobs are those of a twin engine's
                 forward_backward + loss_get: score forms 1 - 4 (shapes of tests/test_gpu_score_seg_exact.py and
                 tests/test_gpu_drop_dedup_wide.py; last_score_form asserted, the dispatch rules are not restated), dedup 0 / 1 where the
                 form has both, h16 0 / 1, one explicit dropout mask per form
  oracle         one case per form against the fp32 oracle under tests/test_gpu_parity.py's TOL (imported, not restated)
  non-interference   fb(A); forward(B); forward(B'); apply_update; fb(C); apply_update against a twin without the forward passes: W, b,
                 histories, the 16-bit copy, every loss_get, grads_get, vv_h16_stats, vv_grad_scale_stats bit-equal -- in the lazily
                 reduced state, after grads_get, with counter-based dropout (the counter did not move), with Adam (t), with a banked gradient
  VV_ERR_STATE   vv_forward after a hinted fb; vv_blobs_get(ip1_diff) and vv_dedup_groups_get after vv_forward
  the record     passes / terms / double sums over three batches, means rounded once, eval_reset, params_set, an all -1 batch
"""
import os

import numpy as np
import pytest

from tests.test_gpu_parity import TOL, make_case, rel_rows, vv  # noqa: F401
from tests.test_gpu_score_seg_exact import batch, world  # noqa: F401  (the shapes' batches and the shared (table, W, b))

pytestmark = pytest.mark.gpu

VV_ERR_STATE = 3
N_ROWS = 640

# (D, B, C, Nn, form, dedup, seg_bwd env): the smallest shapes of each form in the two files named above
FORMS = {
    "f1": (512, 24, 5, 20, 1, True, None),
    "f1_rpw2": (512, 24, 5, 10, 1, True, None),
    "f1_rpw7": (512, 24, 5, 55, 1, True, None),
    "f2": (512, 24, 5, 70, 2, True, None),
    "f2_ctx": (512, 24, 8, 10, 2, True, None),
    "f3": (1024, 16, 5, 20, 3, True, None),
    "f4_dense_reg": (512, 24, 5, 20, 4, False, None),
    "f4_rows_reg": (512, 24, 5, 20, 4, True, False),
    "f4_rows": (320, 24, 5, 20, 4, True, None),
    "f4_dense": (320, 24, 5, 20, 4, False, None),
}


def engine(vv, world, D, dedup=True, seg_bwd=None, opts=None, prec="f16"):  # noqa: F811
    table, W, b = world(D, N_ROWS)
    if seg_bwd is not None:
        os.environ["VV_SEG_BWD"] = "1" if seg_bwd else "0"
    try:
        eng = vv.Engine(0, prec)
    finally:
        os.environ.pop("VV_SEG_BWD", None)
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    eng.set_dedup(dedup)
    eng.table_set(table)
    eng.params_set(W, b)
    return eng


def pair(vv, world, name, idx=None, opts=None, prec="f16", seed=300, **kw):  # noqa: F811
    """(training twin's values, forward-only pass's values) on one batch"""
    D, B, C, Nn, form, dedup, seg_bwd = FORMS[name]
    if idx is None:
        idx = batch(seed, B, C, Nn)
    out = []
    for fwd in (False, True):
        eng = engine(vv, world, D, dedup, seg_bwd, opts, prec)
        cfg = vv.StepConfig(B, C, Nn, **kw)
        if fwd:
            eng.forward(cfg, idx)
            st = eng.eval_stats()
            loss = (st.last_loss, st.last_violations)
            assert st.passes == 1 and st.terms == B * Nn
        else:
            eng.forward_backward(cfg, idx)
            loss = tuple(np.float32(x) for x in eng.loss())
        o = dict(loss=loss, form=int(eng.get_option("last_score_form")), h16=int(eng.get_option("last_h16")),
                 tile=int(eng.get_option("last_fwd_tile_rows")), stats=eng.dedup_stats(), **eng.blobs(cfg))
        eng.close()
        assert o["form"] == form, "%s ran score form %d, written for form %d" % (name, o["form"], form)
        out.append(o)
    return out


def assert_same(t, e, tag):
    print("FWD %s form %d h16 %d tile %d: loss %r violations %r (training twin %r %r)" % (tag, e["form"], e["h16"], e["tile"], e["loss"][0], e["loss"][1], t["loss"][0], t["loss"][1]))
    assert e["form"] == t["form"] and e["h16"] == t["h16"] and e["tile"] == t["tile"] and e["stats"] == t["stats"], tag
    assert e["loss"][0] == t["loss"][0] and e["loss"][1] == t["loss"][1], (tag, e["loss"], t["loss"])
    assert np.isfinite(e["loss"][0]) and e["loss"][0] > 0
    for k in ("ip2", "target_score", "negative_scores"):
        assert np.array_equal(e[k], t[k]), "%s: %s differs from the training pass's" % (tag, k)


# ------------------------------------------------------------------------------- bit equality with the training pass
@pytest.mark.parametrize("h16", [0, 1])
@pytest.mark.parametrize("name", list(FORMS))
def test_bit_equal_to_the_training_pass(vv, world, name, h16):  # noqa: F811
    t, e = pair(vv, world, name, opts=dict(h16=h16))
    seg = FORMS[name][4] != 4
    assert e["h16"] == (h16 if seg else 0)
    if FORMS[name][5]:
        assert e["stats"][1] < e["stats"][0]                              # de-duplicated: the batch repeats rows
    else:
        assert e["stats"][1] == e["stats"][0]
    assert_same(t, e, "%s h16=%d" % (name, h16))


@pytest.mark.parametrize("prec", ["bf16"])
@pytest.mark.parametrize("name", ["f1", "f3", "f4_dense_reg", "f4_rows"])
def test_bit_equal_with_bf16_operands(vv, world, name, prec):  # noqa: F811
    t, e = pair(vv, world, name, prec=prec)
    assert_same(t, e, "%s %s" % (name, prec))


@pytest.mark.parametrize("name,dd", [("f1", 1), ("f2", 2), ("f3", 2), ("f4_dense_reg", 0), ("f4_dense", 0)])
def test_bit_equal_with_an_explicit_dropout_mask(vv, world, name, dd):  # noqa: F811
    D, B, C, Nn = FORMS[name][:4]
    mask = (np.random.default_rng(310).random(((C + Nn) * B, D)) >= 0.5).astype(np.uint8)
    t, e = pair(vv, world, name, opts=dict(drop_dedup=dd), dropout_ratio=0.5, dropout_mask=mask)
    assert 0.6 < (e["ip2"] == 0).mean() < 0.9                             # ReLU leaves about half, the mask half of that
    assert_same(t, e, "%s mask" % name)


@pytest.mark.parametrize("opt", ["L1", "item_weight", "loss_weight", "global_count", "ctx_coeff"])
def test_bit_equal_under_the_options_of_the_loss(vv, world, opt):  # noqa: F811
    kw = {"L1": dict(norm="L1", margin=0.1), "item_weight": dict(item_weight=(1 + np.arange(24) % 4).astype(np.float32)),
          "loss_weight": dict(loss_weight=2.0), "global_count": dict(global_count=4 * 24 * 20), "ctx_coeff": dict(ctx_coeff=[0.1, 0.2, 0.3, 0.4])}[opt]
    t, e = pair(vv, world, "f1", **kw)
    assert_same(t, e, "f1 " + opt)


# ------------------------------------------------------------------------------- against the fp32 oracle
@pytest.mark.parametrize("D,B,C,Nn,form,dedup", [(512, 32, 5, 20, 1, True), (512, 32, 5, 60, 2, True), (1024, 16, 5, 20, 3, True),
                                                  (32, 32, 5, 2, 4, None)])
def test_against_the_fp32_oracle(vv, oracle, D, B, C, Nn, form, dedup):  # noqa: F811
    """tests/test_gpu_parity.py's check() for the forward quantities, with its TOL: embeddings per row, loss, scores; violations equal
    where no d_k lies within the score tolerance of zero."""
    F = 128 if form == 4 else 256
    ds, table, idx, W, b = make_case(7 + form, 40, B, C, Nn, F, D)
    eng = vv.Engine(0, "f16")
    if dedup is not None:
        eng.set_dedup(dedup)
    eng.table_set(table)
    eng.params_set(W, b)
    cfg = vv.StepConfig(B, C, Nn)
    eng.forward(cfg, idx)
    st = eng.eval_stats()
    assert int(eng.get_option("last_score_form")) == form
    got = eng.blobs(cfg)
    eng.close()
    ref = oracle.forward_backward(table, idx, W, b, C_=C, Nn=Nn, want=("H", "s_true", "s_bogus"))
    tol = TOL["f16"]
    m = dict(emb=rel_rows(got["ip2"], ref["H"]), loss=abs(st.last_loss - ref["loss"]) / max(abs(ref["loss"]), 1e-30),
             score=max(np.abs(got["target_score"] - ref["s_true"]).max(), np.abs(got["negative_scores"] - ref["s_bogus"]).max()))
    print("FWD-ORACLE form %d %s violations %r (oracle %r)" % (form, " ".join("%s=%.3e" % kv for kv in m.items()), st.last_violations, ref["violations"]))
    for k in ("emb", "loss", "score"):
        assert m[k] <= tol[k], (k, m[k], tol[k])
    d = np.asarray(ref["s_true"], np.float64) - np.asarray(ref["s_bogus"], np.float64)
    lo, hi = float((d < -tol["score"]).sum()), float((d < tol["score"]).sum())
    assert lo <= st.last_violations <= hi, (lo, st.last_violations, hi)


# ------------------------------------------------------------------------------- the training state is left alone
def half_copy(eng, vv, F, D):  # noqa: F811
    """the 16-bit copy as a forward pass reads it (+ the bias): tests/test_gpu_comm_adam.py's reading"""
    I, Y = eng.dev(np.eye(F, dtype=np.float32)), eng.dev((F, D))
    eng.op("inner_product", I, F, Y)
    out = Y.get()
    I.free(); Y.free()
    return out


def trajectory(vv, world, scenario, with_forward):  # noqa: F811
    D, B, C, Nn = 512, 16, 5, 20                 # (400 rows: few enough K-tiles for the weight gradient to stay in its slabs -- asserted below)
    F = 128
    A, Bh, Bh2, Cc, A0 = (batch(s, B, C, Nn) for s in (400, 401, 402, 403, 404))
    eng = engine(vv, world, D)
    kw = dict(lr=0.05)
    if scenario == "dropout":
        kw.update(dropout_ratio=0.5, dropout_seed=5)
    if scenario == "adam":
        kw.update(solver_type="ADAM", momentum=0.9, momentum2=0.999, lr=1e-3)
    cfg = vv.StepConfig(B, C, Nn, **kw)
    ecfg = vv.StepConfig(B, C, Nn, **kw)
    out = {}

    def evaluate():
        if not with_forward:
            return
        before = eng.accum_stats()["banked"]
        eng.forward(ecfg, Bh)
        eng.forward(ecfg, Bh2)
        out["eval"] = eng.eval_stats()
        assert eng.accum_stats()["banked"] == before
        assert int(eng.get_option("last_score_form")) == 1

    if scenario == "banked":
        eng.forward_backward(cfg, A0)
        eng.grads_bank()
        assert eng.accum_stats()["banked"] == 1
        evaluate()
        assert eng.accum_stats()["banked"] == 1
        eng.forward_backward(cfg, A)
        out["l0"] = eng.loss()
        eng.grads_bank()
        evaluate()
        eng.apply_update(cfg)
        out["accum"] = eng.accum_stats()
    else:
        eng.forward_backward(cfg, A)
        if scenario == "grads":
            out["g0"] = eng.grads()
        if scenario != "lazy":
            out["l0"] = eng.loss()
        evaluate()
        eng.apply_update(cfg)
        out["l0_after"] = eng.loss()                                      # (vv_loss_get keeps the TRAINING pass's loss)
        if scenario == "lazy":
            assert int(eng.get_option("last_update_form")) in (3, 4)       # the reduction was still due: reduced and updated in one launch
    if scenario == "adam":
        assert eng.solver_iter == 1
    eng.forward_backward(cfg, Cc)
    out["l1"] = eng.loss()
    out["g1"] = eng.grads()
    eng.apply_update(cfg)
    out["params"] = eng.params_get()
    if scenario == "adam":
        out["hist2"] = eng.history2_get()
        assert eng.solver_iter == 2
    out["copy"] = half_copy(eng, vv, F, D)
    out["h16"] = eng.h16_stats()
    out["gscale"] = eng.grad_scale_stats()
    eng.close()
    return out


def same_tree(a, b, path):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            same_tree(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), "%s differs from the twin without the forward-only passes" % path
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("scenario", ["lazy", "grads", "dropout", "adam", "banked"])
def test_training_state_is_left_alone(vv, world, scenario):  # noqa: F811
    ref = trajectory(vv, world, scenario, False)
    got = trajectory(vv, world, scenario, True)
    ev = got.pop("eval")
    assert ev.passes == (4 if scenario == "banked" else 2) and np.isfinite(ev.mean_loss) and ev.mean_loss > 0
    assert not np.array_equal(ref["params"][0], world(512, N_ROWS)[1])     # the updates did move W
    same_tree(got, ref, scenario)


# ------------------------------------------------------------------------------- VV_ERR_STATE
def test_state_errors(vv, world):  # noqa: F811
    D, B, C, Nn = 512, 24, 5, 20
    eng = engine(vv, world, D)
    cfg = vv.StepConfig(B, C, Nn, lr=0.01)
    idx = batch(500, B, C, Nn)
    eng.update_hint(cfg)
    eng.forward_backward(cfg, idx)
    with pytest.raises(vv.VVError) as err:
        eng.forward(cfg, idx)
    assert "videovec error %d" % VV_ERR_STATE in str(err.value), str(err.value)
    eng.apply_update(cfg)                                                  # the announced step still finishes
    eng.forward(cfg, idx)
    eng.blobs(cfg)                                                         # ip2 and the score blobs of the pass
    with pytest.raises(vv.VVError) as err:
        eng.blobs(cfg, ip2=False, scores=False, ip1_diff=True)
    assert "videovec error %d" % VV_ERR_STATE in str(err.value), str(err.value)
    with pytest.raises(vv.VVError) as err:
        eng.dedup_groups(dyu=False)
    assert "videovec error %d" % VV_ERR_STATE in str(err.value), str(err.value)
    with pytest.raises(vv.VVError) as err:                                 # another shape while the step's state is alive
        eng.forward(vv.StepConfig(B, C, Nn + 1), batch(501, B, C, Nn + 1))
    assert "videovec error %d" % VV_ERR_STATE in str(err.value), str(err.value)
    eng.forward_backward(cfg, idx)                                         # after a training pass both accessors are what they were
    eng.blobs(cfg, ip1_diff=True)
    eng.dedup_groups(dyu=False)
    eng.close()


# ------------------------------------------------------------------------------- the record
def test_record(vv, world):  # noqa: F811
    D, B, C, Nn = 512, 24, 5, 20
    eng = engine(vv, world, D)
    z = eng.eval_stats()
    assert (z.passes, z.terms, z.loss_sum, z.viol_sum, z.last_loss, z.last_violations, z.mean_loss, z.mean_violations) == (0, 0, 0.0, 0.0, 0, 0, 0, 0)
    cfg = vv.StepConfig(B, C, Nn)
    last = []
    for s in (600, 601, 602):
        eng.forward(cfg, batch(s, B, C, Nn))
        st = eng.eval_stats()
        last.append((st.last_loss, st.last_violations))
    assert len({l for l, _ in last}) == 3                                  # three different batches
    ls, vs = sum(float(np.float64(l)) for l, _ in last), sum(float(np.float64(v)) for _, v in last)
    assert st.passes == 3 and st.terms == 3 * B * Nn
    assert st.loss_sum == ls and st.viol_sum == vs
    assert st.mean_loss == np.float32(ls / 3) and st.mean_violations == np.float32(vs / 3)      # rounded once, from the double
    table, W, b = world(D, N_ROWS)
    eng.params_set(W, b)
    st2 = eng.eval_stats()
    assert (st2.passes, st2.loss_sum, st2.viol_sum) == (3, ls, vs)         # vv_params_set does not reset the record
    eng.eval_reset()
    z = eng.eval_stats()
    assert (z.passes, z.terms, z.loss_sum, z.viol_sum, z.last_loss, z.mean_loss) == (0, 0, 0.0, 0.0, 0, 0)
    eng.forward(cfg, np.full((B, C + Nn), -1, np.int32))
    e = eng.eval_stats()
    assert e.passes == 1 and np.isfinite(e.last_loss) and np.isfinite(e.last_violations)
    eng.close()
