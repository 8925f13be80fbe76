"""Dropout on the de-duplicated path beyond the register-resident shapes (option "drop_dedup" = 2): the one-sweep score kernel
k_score_stream and k_seg_bwd's two-chunk form carry the per-instance masks too -- D = 512 with more than 55 negatives or more than
6 context rows, and every D = 1024 shape.  Every case asserts that the de-duplicated execution really ran (distinct rows < rows) and which
score kernel the forward pass launched (read-only option "last_score_form": 1 k_score_fwd, 2 / 3 k_score_stream at D = 512 / 1024, 4 the
per-instance kernels), so that none can pass on the dense path.

Bounds: against the oracle, tests/test_gpu_parity.py's TOL.  With ip2 stored as f16 (h16 = 1) the step is also held against the fp32-row
form of the same engine at tests/test_gpu_h16.py's bounds (scores 2e-4, loss 2e-5 relative, dW / db 2e-3), and its gradients against the
oracle on the rounded operands at grad_q + 2e-3: the triangle inequality over those two bounds."""
import numpy as np
import pytest

from tests.test_gpu_parity import TOL, check, make_case, rel_fro, run_both, vv  # noqa: F401

pytestmark = pytest.mark.gpu

F = 256
COEFF = {5: np.array([0.4, 0.3, 0.2, 0.1], np.float32),
         9: np.array([0.25, 0.2, 0.15, 0.12, 0.1, 0.08, 0.06, 0.04], np.float32)}
H16_BOUND = dict(score=2e-4, loss=2e-5, grad=2e-3)        # tests/test_gpu_h16.py: f16 rows of ip2 against the fp32 rows of the same engine


def form_of(D):
    return 3 if D == 1024 else 2


class MemoOracle:
    """oracle.forward_backward computed once per (case, operands) and shared by the variants of a case (h16, v16 change nothing for it)."""
    cache = {}

    def __init__(self, oracle, key):
        self.oracle, self.key = oracle, key

    def forward_backward(self, table, idx, W, b, **kw):
        k = (self.key, tuple(kw["want"]))
        if k not in self.cache:
            self.cache[k] = self.oracle.forward_backward(table, idx, W, b, **kw)
        return {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in self.cache[k].items()}


def setenv(monkeypatch, drop_dedup=2, h16=None, v16=None):
    # (the options' environment variables are read when a context is created: run_both creates the engine itself)
    monkeypatch.setenv("VV_DROP_DEDUP", str(drop_dedup))
    if h16 is not None:
        monkeypatch.setenv("VV_H16", str(h16))
    if v16 is not None:
        monkeypatch.setenv("VV_V16", str(v16))


def masked_case(seed, D, B, C, Nn, pool, ratio=0.6, holes=True):
    ds, table, idx, W, b = make_case(seed, 30, B, C, Nn, F, D, wstd=0.01)
    rng = np.random.default_rng(seed + 100)
    idx = rng.integers(0, pool, size=(B, C + Nn)).astype(np.int32)         # rows repeat inside and across items
    if holes:
        idx[1, 2] = -1; idx[5, C + 1] = -1; idx[B - 1, 0] = -1             # a context row, a negative and a target as empty slots
    mask = (rng.random(((C + Nn) * B, D)) > ratio).astype(np.uint8)
    return table, idx, W, b, mask


def assert_dedup_ran(eng, idx, B, C, Nn, form):
    rows, uniq = eng.dedup_stats()
    assert rows == B * (C + Nn), (rows, B * (C + Nn))
    assert uniq == len(np.unique(idx)) < rows, "the de-duplicated path did not run: %d distinct of %d rows" % (uniq, rows)
    assert eng.get_option("last_score_form") == form, (eng.get_option("last_score_form"), form)


def check_against_fp32_rows(got, base, tag):
    e_s = max(np.abs(got["target_score"] - base["target_score"]).max(), np.abs(got["negative_scores"] - base["negative_scores"]).max())
    m = dict(score=e_s, loss=abs(got["loss"] - base["loss"]) / abs(base["loss"]), dW=rel_fro(got["dW"], base["dW"]), db=rel_fro(got["db"], base["db"]))
    print("H16-VS-FP32 %s %s" % (tag, " ".join("%s=%.3e" % kv for kv in m.items())))
    assert m["score"] <= H16_BOUND["score"] and m["loss"] <= H16_BOUND["loss"]
    assert m["dW"] <= H16_BOUND["grad"] and m["db"] <= H16_BOUND["grad"]


def check_violations(got, ref, tol):
    """A violation flag is [s_true < s_bogus]; the scores are held to tol["score"] each, so only the pairs whose reference scores lie within
    twice that of each other can land on the other side: the counts differ by at most their number."""
    near = int((np.abs(ref["s_true"] - ref["s_bogus"]) <= 2 * tol["score"]).sum())
    print("VIOLATIONS %d / %d (%d pairs within 2 x %.0e of a tie)" % (got["viol"], ref["violations"], near, tol["score"]))
    assert abs(got["viol"] - ref["violations"]) <= near, (got["viol"], ref["violations"], near)


def tol_for(prec, h16):
    t = dict(TOL[prec])
    if h16:
        t["grad_q"] = t["grad_q"] + H16_BOUND["grad"]
    return t


SHAPES = [(1024, 16, 5, 7),       # the smallest D = 1024 item
          (1024, 16, 5, 9),       # eight waves: one takes two negatives, the others one
          (512, 16, 5, 56),       # 57 target / negative rows: the first shape past the register-resident kernel
          (512, 16, 9, 10)]       # 8 context rows
CASES1 = [(D, B, C, Nn, h16, v16) for (D, B, C, Nn) in SHAPES for h16 in (0, 1) for v16 in ((0, 1) if D == 1024 else (1,))]


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("D,B,C,Nn,h16,v16", CASES1)
def test_wide_dropout_dedup_matches_oracle(vv, oracle, monkeypatch, prec, D, B, C, Nn, h16, v16):
    """Explicit mask, every blob against the oracle: ip2, scores, loss, violations, ip1_diff, dW, db."""
    table, idx, W, b, mask = masked_case(41 + D + Nn, D, B, C, Nn, pool=60)
    kw = dict(dropout_ratio=0.6, dropout_mask=mask, ctx_coeff=COEFF[C], loss_weight=0.7, global_count=4 * B * Nn, margin=1.5)
    setenv(monkeypatch, 2, h16, v16)
    memo = MemoOracle(oracle, ("t1", D, B, C, Nn, prec))
    eng, _, got, ref = run_both(vv, memo, prec, table, idx, W, b, C, Nn, **kw)
    assert eng.get_option("drop_dedup") == 2 and eng.get_option("h16") == h16 and eng.get_option("v16") == v16
    assert_dedup_ran(eng, idx, B, C, Nn, form_of(D))
    tag = "wide-drop D%d C%d Nn%d %s h16=%d v16=%d" % (D, C, Nn, prec, h16, v16)
    check(got, ref, tol_for(prec, h16), tag)
    check_violations(got, ref, TOL[prec])
    if h16:
        setenv(monkeypatch, 2, 0, v16)
        eng0, _, base, _ = run_both(vv, memo, prec, table, idx, W, b, C, Nn, **kw)
        assert_dedup_ran(eng0, idx, B, C, Nn, form_of(D))
        check_against_fp32_rows(got, base, tag)
        eng0.close()
    eng.close()


@pytest.mark.parametrize("h16", [0, 1])
def test_wide_dropout_dedup_l1_weighted_pairwise_d1024(vv, oracle, monkeypatch, h16):
    """The options that change the backward's coefficients, at D = 1024: L1 hinge, per-item weights, C = 2 (one context row), 30 negatives."""
    D, B, C, Nn = 1024, 24, 2, 30
    ds, table, idx, W, b = make_case(29, 30, B, C, Nn, F, D, wstd=0.01)
    rng = np.random.default_rng(7)
    idx = rng.integers(0, 90, size=(B, C + Nn)).astype(np.int32)
    mask = (rng.random(((C + Nn) * B, D)) > 0.5).astype(np.uint8)
    iw = (0.5 + rng.random(B)).astype(np.float32)
    setenv(monkeypatch, 2, h16)
    eng, _, got, ref = run_both(vv, MemoOracle(oracle, ("t2",)), "f16", table, idx, W, b, C, Nn, dropout_ratio=0.5, dropout_mask=mask, norm=1,
                                item_weight=iw, margin=1.0)
    assert_dedup_ran(eng, idx, B, C, Nn, 3)
    check(got, ref, tol_for("f16", h16), "wide-drop-l1w D1024 h16=%d" % h16)
    eng.close()


@pytest.mark.parametrize("h16", [0, 1])
@pytest.mark.parametrize("D", [1024, 512])
def test_wide_dropout_dedup_long_segments(vv, oracle, monkeypatch, D, h16):
    """A pool of 12 rows: every distinct row has ~100 instances, past the 64-record strip -- k_seg_bwd's order-independent f64 sums, with masks,
    in every chunk.  Against the oracle; and two engines agree bit for bit although the records' arrival order differs from run to run."""
    B, C, Nn = 16, 5, 70
    table, idx, W, b, mask = masked_case(57 + D, D, B, C, Nn, pool=12, holes=False)
    assert np.bincount(idx.reshape(-1)).min() > 64
    kw = dict(dropout_ratio=0.6, dropout_mask=mask, ctx_coeff=COEFF[C], loss_weight=0.7, global_count=4 * B * Nn, margin=1.5)
    setenv(monkeypatch, 2, h16)
    memo = MemoOracle(oracle, ("t3", D))
    eng, _, got, ref = run_both(vv, memo, "f16", table, idx, W, b, C, Nn, **kw)
    assert_dedup_ran(eng, idx, B, C, Nn, form_of(D))
    check(got, ref, tol_for("f16", h16), "wide-drop-long D%d h16=%d" % (D, h16))
    eng2, _, got2, _ = run_both(vv, memo, "f16", table, idx, W, b, C, Nn, **kw)
    assert got2["loss"] == got["loss"] and np.array_equal(got2["dW"], got["dW"]) and np.array_equal(got2["db"], got["db"])
    eng.close(); eng2.close()


@pytest.mark.parametrize("D,B,C,Nn", [(1024, 32, 5, 20), (512, 32, 5, 60)])
def test_wide_counter_based_dropout_dedup_equals_dense(vv, fp32_ip2, D, B, C, Nn):
    """Counter-hash masks: value 2 and value 0 evaluate the same mask function -- the same elements dropped, loss equal to rounding, gradients
    to the reassociation of the sums (the bounds of test_counter_based_dropout_dedup_equals_dense)."""
    ds, table, idx, W, b = make_case(23, 60, B, C, Nn, F, D, wstd=0.02)
    idx = np.random.default_rng(5).integers(0, 300, size=(B, C + Nn)).astype(np.int32)
    out = {}
    for dd in (2, 0):
        eng = vv.Engine(0, "f16")
        eng.set_option("drop_dedup", dd)
        eng.table_set(table); eng.params_set(W, b)
        cfg = vv.StepConfig(B, C, Nn, dropout_ratio=0.9, dropout_seed=4242)
        eng.forward_backward(cfg, idx)
        if dd == 2:
            assert_dedup_ran(eng, idx, B, C, Nn, form_of(D))
        else:
            assert eng.dedup_stats() == (B * (C + Nn), B * (C + Nn)) and eng.get_option("last_score_form") == 4
        out[dd] = (eng.loss(), eng.blobs(cfg)["ip2"], eng.grads())
        eng.close()
    (l2, h2, (dW2, db2)), (l0, h0, (dW0, db0)) = out[2], out[0]
    kept = h2 != 0
    assert np.array_equal(kept, h0 != 0) and 0.02 < kept.mean() < 0.12
    assert np.allclose(h2, h0, rtol=1e-5, atol=1e-6)
    print("WIDE DROP-DEDUP D %d: loss %.7f / %.7f; dW %.2e db %.2e" % (D, l2[0], l0[0], rel_fro(dW2, dW0), rel_fro(db2, db0)))
    assert abs(l2[0] - l0[0]) <= 1e-6 * l0[0] and l2[1] == l0[1]
    assert rel_fro(dW2, dW0) <= 2e-3 and rel_fro(db2, db0) <= 1e-4


def run_step(vv, table, idx, W, b, B, C, Nn, opts, **kw):
    eng = vv.Engine(0, "f16")
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.table_set(table); eng.params_set(W, b)
    cfg = vv.StepConfig(B, C, Nn, **kw)
    eng.forward_backward(cfg, idx)
    out = dict(loss=eng.loss(), stats=eng.dedup_stats(), form=eng.get_option("last_score_form"), **eng.blobs(cfg))
    out["dW"], out["db"] = eng.grads()
    return eng, out


def test_drop_dedup_switch(vv, monkeypatch):
    """The default (1) is unchanged: dropout at D = 1024 runs dense, at the register-resident shapes de-duplicated; 2 changes nothing there."""
    monkeypatch.delenv("VV_DROP_DEDUP", raising=False)
    B, C, Nn = 16, 5, 7
    t1, i1, W1, b1, m1 = masked_case(71, 1024, B, C, Nn, pool=60)
    t5, i5, W5, b5, m5 = masked_case(72, 512, B, C, Nn, pool=60)
    kw1 = dict(dropout_ratio=0.6, dropout_mask=m1)
    kw5 = dict(dropout_ratio=0.6, dropout_mask=m5)
    eng, o = run_step(vv, t1, i1, W1, b1, B, C, Nn, {}, **kw1)
    assert eng.get_option("drop_dedup") == 1
    assert o["stats"] == (B * (C + Nn), B * (C + Nn)) and o["form"] == 4
    # without dropout the D = 1024 step is the one-sweep kernel's, whatever the option says
    for dd in (0, 1, 2):
        eng.set_option("drop_dedup", dd)
        assert eng.get_option("drop_dedup") == dd
        eng.forward_backward(vv.StepConfig(B, C, Nn), i1)
        assert eng.get_option("last_score_form") == 3 and eng.dedup_stats()[1] == len(np.unique(i1))
    # values outside {0, 1, 2} are refused and leave the option as it is; the read-only option refuses every value
    for bad in (3, -1, 0.5):
        with pytest.raises(vv.VVError):
            eng.set_option("drop_dedup", bad)
    assert eng.get_option("drop_dedup") == 2
    with pytest.raises(vv.VVError, match="read-only"):
        eng.set_option("last_score_form", 1)
    eng.close()
    fresh = vv.Engine(0, "f16")
    assert fresh.get_option("last_score_form") == 0           # before the first step
    fresh.close()
    # the register-resident shape: de-duplicated under 1 and 2, by the same kernels -- identical blobs
    e1, o1 = run_step(vv, t5, i5, W5, b5, B, C, Nn, {}, **kw5)
    e2, o2 = run_step(vv, t5, i5, W5, b5, B, C, Nn, {"drop_dedup": 2}, **kw5)
    for o_ in (o1, o2):
        assert o_["stats"] == (B * (C + Nn), len(np.unique(i5))) and o_["form"] == 1
    for k in ("ip2", "target_score", "negative_scores", "dW", "db"):
        assert np.array_equal(o1[k], o2[k]), k
    assert o1["loss"] == o2["loss"]
    e1.close(); e2.close()
    # the environment variable: read when a context is created; an invalid value leaves the default
    monkeypatch.setenv("VV_DROP_DEDUP", "2")
    e = vv.Engine(0, "f16")
    assert e.get_option("drop_dedup") == 2
    e.close()
    monkeypatch.setenv("VV_DROP_DEDUP", "3")
    e = vv.Engine(0, "f16")
    assert e.get_option("drop_dedup") == 1
    e.close()


def test_one_update_through_the_wide_dropout_path(vv):
    """One solver step at D = 1024 under dropout: W, b and both histories against the dense engine (drop_dedup 0) on the same inputs, within
    the f16 bounds of test_sgd_steps_match_oracle (W 1e-3, b 2e-3, histories 4e-3)."""
    D, B, C, Nn = 1024, 16, 5, 7
    table, idx, W, b, mask = masked_case(83, D, B, C, Nn, pool=60)
    res = {}
    for dd in (2, 0):
        eng = vv.Engine(0, "f16")
        eng.set_option("drop_dedup", dd)
        eng.table_set(table); eng.params_set(W, b)
        cfg = vv.StepConfig(B, C, Nn, lr=0.05, momentum=0.9, weight_decay=5e-4, dropout_ratio=0.6, dropout_mask=mask, ctx_coeff=COEFF[C],
                            loss_weight=0.7, global_count=4 * B * Nn, margin=1.5)
        eng.step(cfg, idx)
        if dd == 2:
            assert_dedup_ran(eng, idx, B, C, Nn, 3)
        else:
            assert eng.dedup_stats()[1] == B * (C + Nn)
        res[dd] = eng.params_get()
        eng.close()
    (W2, b2, hW2, hb2), (W0, b0, hW0, hb0) = res[2], res[0]
    assert not np.array_equal(W0, W)
    m = (rel_fro(W2, W0), rel_fro(b2, b0), rel_fro(hW2, hW0), rel_fro(hb2, hb0))
    print("WIDE DROP-DEDUP update: W=%.3e b=%.3e hW=%.3e hb=%.3e" % m)
    assert m[0] <= 1e-3 and m[1] <= 2e-3 and m[2] <= 4e-3 and m[3] <= 4e-3
