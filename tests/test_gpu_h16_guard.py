"""Range loss of the f16 ip2 rows, counted on the device (option "h16_guard", vv_h16_stats / Engine.h16_stats).

The segment-wise backward holds every distinct row of a step once; with "h16_guard" >= 1 it counts the elements stored as 65504
(saturated) and the rows whose largest element is > 0 and < 2^-14 (faint), and value 2 switches the engine to fp32 rows once a step's
report shows either.  Every operand here is exactly representable -- features are small integers, one-hot rows and powers of two, weights
integers times 2^-6 and powers of two -- so ip2 is exact in float64 numpy and the counts are compared with ==.  The expected counts come
from numpy alone (expected(): float64 product, bias, ReLU, min(., 65504), astype(float16)) over the distinct rows Engine.dedup_groups()
names; nothing is taken from the library's own f16 rows.

Every case asserts the path it ran: "last_h16", "last_score_form" (1 k_score_fwd, 2 / 3 the one-sweep kernel at D = 512 / 1024) and
distinct rows < rows.  The lag: the host reads the report of step s when it issues step s + 4 (LAG below; include/videovec.h)."""
import numpy as np
import pytest

from tests.test_gpu_parity import round_operand, round_table, vv  # noqa: F401  (vv: fixture)

pytestmark = pytest.mark.gpu

F = 256
LAG = 4                          # include/videovec.h: the report of step s is read when step s + 4 is issued
SEGB_BLOCKS = 1024               # k_seg_bwd's persistent grid: four waves, one row each, per workgroup and pass
BIG = np.float32(131072.0)       # a bias entry that saturates every row's column (|x W^T| <= 3 * 8 * F / 64 = 96)
F_SAT, F_FAINT, F_EDGE, F_DEAD = 3, 5, 7, 9        # feature columns kept for the planted rows (zero in every ordinary row)


# ------------------------------------------------------------------------------- operands
def features(seed, n):
    rng = np.random.default_rng(seed)
    T = (rng.integers(1, 4, size=(n, F)) * (rng.random((n, F)) < 0.5)).astype(np.float32)
    T[:, [F_SAT, F_FAINT, F_EDGE, F_DEAD]] = 0
    return T


def weights(D):
    rng = np.random.default_rng(7 * D + F)
    W = (rng.integers(-8, 9, size=(D, F)) / 64.0).astype(np.float32)
    W[:, [F_SAT, F_FAINT, F_EDGE, F_DEAD]] = 0
    return W, np.zeros(D, np.float32)


def batch(seed, B, C, Nn, pool):
    return np.random.default_rng(seed).integers(0, pool, size=(B, C + Nn)).astype(np.int32)


def expected(T, W, b, uniq_rows):
    """(saturated elements, faint rows) of the distinct rows, from numpy alone.  Table row len(T) is the library's all-zero row (index -1)."""
    Tz = np.vstack([T, np.zeros((1, T.shape[1]), T.dtype)]).astype(np.float64)
    ip2 = np.maximum(Tz[uniq_rows] @ W.astype(np.float64).T + b.astype(np.float64), 0.0)
    h = np.minimum(ip2, 65504.0).astype(np.float16)
    mx = h.max(axis=1).astype(np.float64)
    return int((h == np.float16(65504.0)).sum()), int(((mx > 0) & (mx < 2.0 ** -14)).sum())


def make_engine(vv, prec, T, W, b, guard=1, **opts):  # noqa: F811
    assert np.array_equal(round_table(T, prec), T) and np.array_equal(round_operand(W, prec), W), "the operands are not exact: wrong inputs"
    eng = vv.Engine(0, prec)
    eng.set_option("h16_guard", guard)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.table_set(T)
    eng.params_set(W, b)
    return eng


def ran(eng, idx, form, f16_rows=1):
    """The path of the last pass; returns the table rows of its distinct rows."""
    rows, uniq = eng.dedup_stats()
    assert rows == idx.size and uniq == len(np.unique(idx)) < rows, (rows, uniq)
    assert eng.get_option("last_h16") == f16_rows
    if form is not None:
        assert eng.get_option("last_score_form") == form, (eng.get_option("last_score_form"), form)
    g = eng.dedup_groups(dyu=False)
    return g["uniq_rows"][:g["U"]]


def counts(eng):
    st = eng.h16_stats()
    return st["saturated"], st["faint_rows"]


# ------------------------------------------------------------------------------- 1, 2: clean batch, saturation by column
#         D,   B, C, Nn, form, options
SHAPES = [(512, 16, 5, 10, 1, {}),                               # k_score_fwd, one chunk (the early row load)
          (512, 16, 5, 70, 2, {}),                               # the one-sweep form at D = 512: more than 56 target / negative rows
          (512, 16, 9, 10, 2, {}),                               # ... more than 6 context rows
          (1024, 8, 5, 60, 3, {"v16": 0}),                       # two chunks (the late row load)
          (1024, 8, 5, 60, 3, {"v16": 1}),                       # ... with f16 per-item vectors
          (512, 16, 5, 10, 1, {"drop_dedup": 2, "drop": 0.5}),   # the DROP instantiations
          (1024, 8, 5, 60, 3, {"drop_dedup": 2, "drop": 0.5})]


def shape_id(s):
    return "D%d-B%d-C%d-Nn%d-%s" % (s[0], s[1], s[2], s[3], "-".join("%s%s" % kv for kv in s[5].items()) or "plain")


def run_shape(vv, prec, shape, b_plant):  # noqa: F811
    D, B, C, Nn, form, opts = shape
    opts = dict(opts)
    drop = opts.pop("drop", 0.0)
    T = features(11, 60)
    W, b = weights(D)
    for col in b_plant:
        b[col] = BIG
    idx = batch(5 + Nn, B, C, Nn, 40)
    idx[1, 2] = -1                                                  # an empty slot: the all-zero row is a distinct row too (its ip2 is the bias)
    eng = make_engine(vv, prec, T, W, b, 1, **opts)
    eng.forward_backward(vv.StepConfig(B, C, Nn, dropout_ratio=drop, dropout_seed=3), idx)
    uniq = ran(eng, idx, form)
    return eng, counts(eng), expected(T, W, b, uniq), len(uniq)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_clean_batch_counts_nothing(vv, shape):  # noqa: F811
    eng, got, exp, U = run_shape(vv, "f16", shape, [])
    assert exp == (0, 0) and got == (0, 0), (got, exp)
    st = eng.h16_stats()
    assert (st["flagged_steps"], st["first_flagged_step"], st["fallback"], st["rows_f16"]) == (0, -1, 0, 1), st
    eng.close()


@pytest.mark.parametrize("where", ["first", "511", "512", "last"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_saturated_column_counts_every_distinct_row(vv, shape, where):  # noqa: F811
    """One bias entry past f16's range: every distinct row saturates in that column -- lane 0, lane 63 and both 512-column chunks in turn."""
    D = shape[0]
    col = {"first": 0, "511": 511, "512": 512 % D, "last": D - 1}[where]
    eng, got, exp, U = run_shape(vv, "f16", shape, [col])
    assert exp == (U, 0), "wrong inputs: %r for %d distinct rows" % (exp, U)
    assert got == exp, (got, exp)
    assert eng.h16_stats()["rows_f16"] == 1
    eng.close()


def test_bf16_operands_count_the_same(vv):  # noqa: F811
    """The rows of H are f16 with bf16 operands too: same counts, and the report is read there as well (flagged_steps moves)."""
    eng, got, exp, U = run_shape(vv, "bf16", SHAPES[0], [0, 300])
    assert exp == (2 * U, 0) and got == exp, (got, exp)
    assert eng.h16_stats()["flagged_steps"] == 0                    # (nothing has been read yet: the lag)
    eng.loss()                                                      # (the step's reduction publishes its report)
    D, B, C, Nn = SHAPES[0][:4]
    for _ in range(LAG):
        eng.step(vv.StepConfig(B, C, Nn, lr=0.0), batch(5 + Nn, B, C, Nn, 40))
    st = eng.h16_stats()
    assert st["flagged_steps"] == 1 and st["first_flagged_step"] == 0 and st["fallback"] == 0 and st["rows_f16"] == 1, st
    eng.close()


# ------------------------------------------------------------------------------- 3: saturation by row
def saturating_row_case(D, k_cols):
    """Table row 0 is one-hot (2048 at F_SAT) against 32 in k_cols of W's column F_SAT: ip2 = 65536 there, only in that row."""
    T = features(21, 60)
    W, b = weights(D)
    T[0] = 0
    T[0, F_SAT] = 2048.0
    W[k_cols, F_SAT] = 32.0
    return T, W, b


@pytest.mark.parametrize("D,B,C,Nn,form,repeat", [(512, 16, 5, 10, 1, 1), (1024, 8, 5, 60, 3, 1),
                                                  (512, 16, 5, 10, 1, 100), (1024, 8, 5, 60, 3, 200)])
def test_saturated_row_is_counted_once(vv, D, B, C, Nn, form, repeat):  # noqa: F811
    """One row saturates in k columns: count k -- also when the batch repeats that row more than 64 times (the f64 segment path): a distinct
    row is counted once."""
    k_cols = [0, 7, 8, 63, 64, 255, 504, 511, D - 512, D - 1, D - 9]
    k = len(set(k_cols))
    T, W, b = saturating_row_case(D, k_cols)
    idx = batch(31, B, C, Nn, 40)
    idx[idx == 0] = 1
    flat = idx.reshape(-1)
    flat[np.random.default_rng(3).choice(flat.size, repeat, replace=False)] = 0
    assert int((idx == 0).sum()) == repeat
    eng = make_engine(vv, "f16", T, W, b)
    eng.forward_backward(vv.StepConfig(B, C, Nn), idx)
    uniq = ran(eng, idx, form)
    exp = expected(T, W, b, uniq)
    assert exp == (k, 0), exp
    assert counts(eng) == exp, (counts(eng), exp)
    eng.close()


# ------------------------------------------------------------------------------- 4: faint rows
@pytest.mark.parametrize("D,B,C,Nn,form", [(512, 16, 5, 10, 1), (1024, 8, 5, 60, 3)])
def test_faint_rows(vv, D, B, C, Nn, form):  # noqa: F811
    """Row 0: one-hot against a weight column of 2^-16 -- ip2 = 2^-16 everywhere: faint.  Row 1: the same against 2^-14, the smallest normal
    f16: not faint.  Row 2: a row dead behind the ReLU, and index -1 with zero bias: all-zero rows, not faint."""
    T = features(41, 60)
    W, b = weights(D)
    T[:3] = 0
    T[0, F_FAINT] = 1.0; W[:, F_FAINT] = 2.0 ** -16
    T[1, F_EDGE] = 1.0; W[:, F_EDGE] = 2.0 ** -14
    T[2, F_DEAD] = 1.0; W[:, F_DEAD] = -1.0 / 64
    idx = batch(43, B, C, Nn, 40)
    idx[0, :4] = [0, 1, 2, -1]
    eng = make_engine(vv, "f16", T, W, b)
    eng.forward_backward(vv.StepConfig(B, C, Nn), idx)
    uniq = ran(eng, idx, form)
    assert {0, 1, 2, len(T)} <= set(uniq.tolist())
    exp = expected(T, W, b, uniq)
    assert exp == (0, 1), exp
    assert counts(eng) == exp, (counts(eng), exp)
    eng.close()


# ------------------------------------------------------------------------------- 5: more than one pass of the grid, and idle waves
def test_more_rows_than_one_pass_of_the_grid(vv):  # noqa: F811
    """U > 4 SEGB_BLOCKS distinct rows: waves take a second row.  Saturating rows sit in the first and in the last distinct slots."""
    D, B, C, Nn, n = 512, 128, 5, 50, 8192
    T = features(51, n)
    W, b = weights(D)
    k_cols = [0, 200, 511]
    W[k_cols, F_SAT] = 32.0
    idx = batch(53, B, C, Nn, n)
    eng = make_engine(vv, "f16", T, W, b)
    cfg = vv.StepConfig(B, C, Nn)
    eng.forward_backward(cfg, idx)
    uniq = ran(eng, idx, 1)
    U = len(uniq)
    assert U > 4 * SEGB_BLOCKS, U
    assert counts(eng) == expected(T, W, b, uniq) == (0, 0)
    slots = [0, 5, 4 * SEGB_BLOCKS - 1, 4 * SEGB_BLOCKS, U - 2, U - 1]
    planted = uniq[slots]
    T[planted, F_SAT] = 2048.0
    eng.table_set(T)
    eng.forward_backward(cfg, idx)
    uniq2 = ran(eng, idx, 1)
    at = sorted(int(np.flatnonzero(uniq2 == r)[0]) for r in planted)
    assert at[0] < 4 * SEGB_BLOCKS <= at[-1], at                     # both passes of the grid hold a saturating row
    exp = expected(T, W, b, uniq2)
    assert exp == (len(slots) * len(k_cols), 0), exp
    assert counts(eng) == exp, (counts(eng), exp)
    eng.close()


def test_fewer_rows_than_waves(vv):  # noqa: F811
    """U < 4: some waves of the first workgroup, and every other workgroup, take no row."""
    D, B, C, Nn = 512, 2, 5, 10
    T, W, b = saturating_row_case(D, [1, 510])
    idx = batch(61, B, C, Nn, 3)
    eng = make_engine(vv, "f16", T, W, b)
    eng.forward_backward(vv.StepConfig(B, C, Nn), idx)
    uniq = ran(eng, idx, 1)
    assert len(uniq) == 3
    exp = expected(T, W, b, uniq)
    assert exp == (2, 0) and counts(eng) == exp, (counts(eng), exp)
    eng.close()


# ------------------------------------------------------------------------------- 6: counting changes nothing
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("D,B,C,Nn,form", [(512, 16, 5, 10, 1), (1024, 8, 5, 60, 3)])
def test_counting_changes_no_value(vv, prec, D, B, C, Nn, form):  # noqa: F811
    T, W, b = saturating_row_case(D, [0, 511, D - 1])
    b[5] = BIG
    idx = batch(71, B, C, Nn, 40)
    out = {}
    for guard in (0, 1):
        eng = make_engine(vv, prec, T, W, b, guard)
        cfg = vv.StepConfig(B, C, Nn, lr=0.05, momentum=0.9, weight_decay=0.001)
        eng.forward_backward(cfg, idx)
        uniq = ran(eng, idx, form)
        loss, viol = eng.loss()
        dW, db = eng.grads()
        got = counts(eng)
        eng.step(cfg, idx)
        Wn, bn, hW, hb = eng.params_get()
        out[guard] = dict(loss=loss, viol=viol, dW=dW, db=db, W=Wn, b=bn, hW=hW, hb=hb)
        exp = expected(T, W, b, uniq)
        assert exp[0] >= len(uniq) and got == (exp if guard else (0, 0)), (guard, got, exp)
        eng.close()
    assert not np.array_equal(out[0]["W"], W)                        # (the update did move the parameters)
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


# ------------------------------------------------------------------------------- 7: fallback
def fallback_sequence(vv, guard, n_clean=2, n_steps=9):  # noqa: F811
    """n_clean clean steps, then the same saturating batch each step; lr 0, so W stays fixed.  Returns the engine and the stats per step."""
    D, B, C, Nn = 512, 16, 5, 10
    T, W, b = saturating_row_case(D, [0, 100, 511])
    idx_sat = batch(81, B, C, Nn, 40)
    idx_sat[0, 0] = 0
    idx_clean = np.where(idx_sat == 0, 1, idx_sat).astype(np.int32)
    eng = make_engine(vv, "f16", T, W, b, guard)
    cfg = vv.StepConfig(B, C, Nn, lr=0.0, momentum=0.0, weight_decay=0.0)
    trace = []
    for s in range(n_steps):
        eng.step(cfg, idx_clean if s < n_clean else idx_sat)
        trace.append(eng.h16_stats())
    return eng, cfg, (T, W, b, idx_sat, idx_clean), trace


def test_guard_2_falls_back_to_fp32_rows_at_the_lag(vv):  # noqa: F811
    n_clean = 2
    eng, cfg, (T, W, b, idx_sat, idx_clean), trace = fallback_sequence(vv, 2, n_clean)
    for s, st in enumerate(trace):
        if s < n_clean + LAG:                                        # the flagged step and the LAG - 1 after it still ran f16 rows
            assert st["rows_f16"] == 1 and st["fallback"] == 0, (s, st)
            assert st["saturated"] == (0 if s < n_clean else 3), (s, st)
        else:                                                        # the step exactly LAG after it, and every later one: fp32 rows
            assert st["rows_f16"] == 0 and st["fallback"] == 1 and st["saturated"] == 0, (s, st)
            assert st["first_flagged_step"] == n_clean, (s, st)
    for s, st in enumerate(trace):                                   # (steps n_clean .. n_clean + LAG - 1 counted; each is read LAG steps later)
        assert st["flagged_steps"] == min(LAG, max(0, s - LAG - n_clean + 1)), (s, st)
    assert eng.get_option("h16_fallback") == 1 and eng.get_option("h16_flagged_step") == n_clean
    assert eng.get_option("h16_flagged_saturated") == 3 and eng.get_option("h16_flagged_faint_rows") == 0
    # the fallback is exactly the execution of h16 = 0
    eng.forward_backward(cfg, idx_sat)
    ran(eng, idx_sat, 1, f16_rows=0)
    got = dict(loss=eng.loss(), dW=eng.grads(), **eng.blobs(cfg))
    ref_eng = make_engine(vv, "f16", T, W, b, 2, h16=0)
    ref_eng.forward_backward(cfg, idx_sat)
    ran(ref_eng, idx_sat, 1, f16_rows=0)
    assert counts(ref_eng) == (0, 0)
    ref = dict(loss=ref_eng.loss(), dW=ref_eng.grads(), **ref_eng.blobs(cfg))
    assert got["loss"] == ref["loss"]
    for k in ("target_score", "negative_scores", "ip2"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["dW"][0], ref["dW"][0]) and np.array_equal(got["dW"][1], ref["dW"][1])
    ref_eng.close()
    # a second run of the whole sequence switches at the same step
    eng2, _, _, trace2 = fallback_sequence(vv, 2, n_clean)
    assert [(t["rows_f16"], t["fallback"], t["first_flagged_step"]) for t in trace2] == \
           [(t["rows_f16"], t["fallback"], t["first_flagged_step"]) for t in trace]
    eng2.close()
    # setting h16 again re-arms the guard; on clean batches the engine stays on f16 rows (the reports of the earlier flagged steps,
    # still due, start no new fallback)
    eng.set_option("h16", 1)
    assert eng.h16_stats()["fallback"] == 0 and eng.get_option("h16_fallback") == 0
    for s in range(LAG + 2):
        eng.step(cfg, idx_clean)
        st = eng.h16_stats()
        assert st["rows_f16"] == 1 and st["fallback"] == 0 and st["saturated"] == 0, (s, st)
    # ... and a batch that saturates after the re-arming switches it again, LAG steps later
    for s in range(LAG + 1):
        eng.step(cfg, idx_sat)
        st = eng.h16_stats()
        assert st["rows_f16"] == (1 if s < LAG else 0) and st["fallback"] == (0 if s < LAG else 1), (s, st)
    eng.close()


def test_guard_1_reports_and_never_switches(vv):  # noqa: F811
    n_clean = 2
    eng, _, _, trace = fallback_sequence(vv, 1, n_clean)
    for s, st in enumerate(trace):
        assert st["rows_f16"] == 1 and st["fallback"] == 0 and st["saturated"] == (0 if s < n_clean else 3), (s, st)
        assert st["flagged_steps"] == max(0, s - LAG - n_clean + 1), (s, st)
        assert st["first_flagged_step"] == (n_clean if s >= n_clean + LAG else -1), (s, st)
    eng.close()


# ------------------------------------------------------------------------------- 8: fixed inputs
def test_option_values(vv):  # noqa: F811
    eng = vv.Engine(0, "f16")
    assert eng.get_option("h16_guard") == 1 and eng.get_option("last_h16") == 0
    for name in ("last_h16", "h16_fallback", "h16_flagged_step", "h16_flagged_saturated", "h16_flagged_faint_rows"):
        with pytest.raises(vv.VVError, match="videovec error 1: .*read-only"):          # VV_ERR_ARG
            eng.set_option(name, 1)
    for bad in (3, -1, 0.5):
        with pytest.raises(vv.VVError, match="videovec error 1: .*h16_guard"):
            eng.set_option("h16_guard", bad)
    for v in (0, 2, 1):
        eng.set_option("h16_guard", v)
        assert eng.get_option("h16_guard") == v
    with pytest.raises(vv.VVError, match="no forward pass yet"):
        eng.h16_stats()
    eng.close()


def test_fp32_rows_count_nothing(vv):  # noqa: F811
    """The dense path and h16 = 0 run fp32 rows: the counters read 0 although the bias is past f16's range."""
    D, B, C, Nn = 512, 16, 5, 10
    T = features(11, 60)
    W, b = weights(D)
    b[0] = BIG
    idx = batch(15, B, C, Nn, 40)
    for opts in ({"h16": 0}, {"dedup": 0}):
        eng = make_engine(vv, "f16", T, W, b, 1, **opts)
        eng.forward_backward(vv.StepConfig(B, C, Nn), idx)
        st = eng.h16_stats()
        assert eng.get_option("last_h16") == 0 and (st["saturated"], st["faint_rows"], st["rows_f16"]) == (0, 0, 0), (opts, st)
        eng.close()
