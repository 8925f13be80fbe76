"""The score / loss forward and the segment-wise backward, element by element against float64 (kernels_score.hip: k_score_fwd,
k_score_stream, k_seg_bwd, k_seg_bwd_cnt; and the per-instance kernels k_score_loss / k_score_loss_reg through ip1_diff).

Every case runs ONE forward_backward under the shipped defaults (f16 rows of ip2: h16 = 1; no fp32_ip2 fixture), asserts which forms ran
(last_score_form, last_h16, dedup_stats), reads ip2 back and hands it to tests/score_ref.py: the reference restates the math of
kernels_score.hip's head in float64 from the very rows the kernels read, with the grouping of tests/pyref.py, so what is compared is the
pair alone.  Then

  scores      |got - ref64| <= eps_s for every pair;                       eps_s = 4 max |ref32 - ref64| over the case's scores
  violations  ==   (the reference has no |d_k| <= eps_s and no |margin - d_k| <= eps_s: asserted -- a condition on the inputs)
  loss        |got - ref64| <= eps_s sum_k |dloss / dd_k|
  dyu x scale every element of rows 0 .. U-1: |got - ref64 scale| <= ulp16 / 2 + eps_g[row];
              eps_g[row] = 4 max |ref32 - ref64| scale over the slot's row; ulp16: the spacing of the run's 16-bit type at
              |ref64 scale| + eps_g[row], the largest magnitude the kernel can have rounded
  padding     rows U .. ceil(U / 64) 64 - 1 exactly 0, behind a batch of many more distinct rows in the same context
  zeros       (without dropout) exactly 0 wherever the slot's shared ip2 value is 0

ref32 is the same numpy function in float32; the factor 4 between two float32 summation orders is tests/test_gpu_gallery.py's
convention.  Nothing is measured against another form of the engine.  The V16 form (D = 1024, option v16: Ah_b and dA_b leave as f16) adds
its own rounding's half-ulp, carried linearly through the float64 formulas (score_ref.v16_term); the same shape runs with v16 = 0 without it.

Two of the listed degenerate batches have items whose rows are all equal (idx all equal; one item all -1): there d_k = 0 in exact
arithmetic, so the sign of the kernel's d_k is rounding noise.  Those items are NAMED by the case; every other item must satisfy the
boundary condition, and the violations must lie between the count without and with the named items' pairs.

Observed on an MI355X, 55 cases, 4.2 s for the whole file (every case prints its own "SSE ..." lines: the form it ran, eps_s, the largest
eps_g and the worst share of each bound): eps_s 1.9e-7 .. 6.3e-7; the worst score at 0.43 of eps_s (D = 320, per-instance kernel), the
worst loss at 0.83 of its bound (dropout, D = 512); eps_g between 0.001 and 0.007 of the largest half ulp, so the bound on dyu is the
16-bit rounding itself and the worst element of every case sits at 0.99 .. 1.00 of it, as a correct rounding of thousands of elements
must; the nearest hinge / sign boundary 9 eps_s away (segments, D = 1024).  Run against mutated kernels (scratch builds only): a dropped
last record of k_seg_bwd's unroll tail fails 48 cases, t_q = 0 for the last row of a wave's share in k_score_fwd 14 (the 16 / 32 / 56-row
bands, B = 1 .. 24, the degenerate batches), a context alpha without drop_scale the three dropout cases; taking the order-independent path
at 64 instances instead of 65 fails none -- both paths form the same sums (the strip exists for speed, the f64 path is valid for any length).

The tiny-gradient cases (bf16, loss_weight 2^-108: the largest |dA_b| below 2^-113, the sums still normal bf16 values) hold the two
power-of-two scales that carry dA_b (k_score_stream's V16 form) and the split-K partial products (k_wgrad_gemm_ph, slab16) as f16: both
exponents are clamped so that the scale and its inverse stay normal floats.  Before the clamp both cases produced inf / NaN: 14 - e and 15 - e
passed 127, the scale was inf and its inverse 0 (the V16 case lost dyu and dW, the tile-scale case every element of dW).
"""
import os

import numpy as np
import pytest

from tests.score_ref import instance_order, score_ref, ulp16, v16_term
from tests.test_gpu_parity import vv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PRECS = ["f16", "bf16"]
N_ROWS, F = 640, 128
POOL_T, POOL = 100, 250                 # targets come from rows [0, 100), negatives from [100, 250), contexts from [0, 250)


@pytest.fixture(scope="module")
def world():
    """(D, n_rows) -> (table, W, b): signed features, so that embeddings are not nearly parallel (cosines around 0.3, d_k spread over
    tenths: the boundary conditions hold for ordinary seeds).  Computed once, shared, never modified."""
    cache = {}

    def get(D, n_rows=N_ROWS):
        if (D, n_rows) not in cache:
            rng = np.random.default_rng(1000 + D + n_rows)
            table = rng.standard_normal((n_rows, F)).astype(np.float32)
            W = (rng.standard_normal((D, F)) * 0.05).astype(np.float32)
            b = (rng.standard_normal(D) * 0.05).astype(np.float32)
            cache[(D, n_rows)] = (table, W, b)
        return cache[(D, n_rows)]
    return get


def batch(seed, B, C, Nn):
    """Heavy repeats; no item's target row among its own negatives (that pair's d_k would be 0: the sign boundary); every third item's
    first context row is its target (a high target score: hinges on both sides of small margins)."""
    rng = np.random.default_rng(seed)
    idx = np.empty((B, C + Nn), np.int32)
    idx[:, 0] = rng.integers(0, POOL_T, B)
    idx[:, 1:C] = rng.integers(0, POOL, (B, C - 1))
    idx[:, C:] = rng.integers(POOL_T, POOL, (B, Nn))
    idx[::3, 1] = idx[::3, 0]
    idx[0, C + 1] = idx[0, C]                                            # (a repeat even in a batch of one item)
    return idx


def run_case(vv, world, prec, D, idx, C, Nn, opts=None, seg_bwd=None, dedup=True, n_rows=N_ROWS, form4=False, prime=True, **kw):  # noqa: F811
    table, W, b = world(D, n_rows)
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
    B = idx.shape[0]
    cfg = vv.StepConfig(B, C, Nn, **kw)
    if prime and dedup:          # as many distinct rows as the table has: rows of dYu past this case's U hold stale sums
        eng.forward_backward(cfg, (np.arange(idx.size, dtype=np.int32) % n_rows).reshape(idx.shape))
    eng.forward_backward(cfg, idx)
    out = dict(form=int(eng.get_option("last_score_form")), h16=int(eng.get_option("last_h16")), stats=eng.dedup_stats() if dedup else None,
               splits=int(eng.get_option("last_wgrad_splits")), loss=eng.loss(), prec=prec, B=B, C=C, Nn=Nn, D=D, idx=idx, n_rows=n_rows, kw=kw)
    out["dW"], out["db"] = eng.grads()
    # the f16 gradient-scale guard's records of this step (tests/test_gpu_grad_guard_exact.py): the host's scale, what the device took off it
    out["sg"], out["grad_shift"] = eng.grad_scale_stats()[1], int(eng.get_option("last_grad_shift"))
    out["grad_shift_round1"], out["grad_repeat"] = int(eng.get_option("last_grad_shift_round1")), int(eng.get_option("last_grad_repeat"))
    real = float(np.ldexp(np.float64(out["sg"]), -out["grad_shift"]))
    if dedup:
        out["groups"] = eng.dedup_groups(dyu=True)
        out["scale"] = out["groups"]["scale"]
        assert out["scale"] == real, "dedup_groups' scale %r, the host's %r shifted by %d" % (out["scale"], out["sg"], out["grad_shift"])
    else:
        # (dense: the host's scale times 2^-last_grad_shift, what the guard's repeat took off it on the device)
        out["scale"] = real
    out.update(eng.blobs(cfg, ip1_diff=form4))
    assert int(eng.get_option("last_score_form")) == out["form"]
    eng.close()
    return out


def refs(o):
    kw = {k: v for k, v in o["kw"].items() if k in ("margin", "norm", "loss_weight", "item_weight", "ctx_coeff", "global_count", "dropout_ratio")}
    if "norm" in kw:
        kw["norm"] = {"L1": 1, "L2": 2}.get(kw["norm"], kw["norm"])
    a = (o["ip2"], o["idx"], o["n_rows"], o["C"], o["Nn"])
    return score_ref(*a, h16=bool(o["h16"]), **kw), score_ref(*a, dtype=np.float32, **kw), kw


def check_forward(o, r64, r32, kw, tag, degenerate=(), loss_slack=0.0):
    """loss_slack: added to the loss's bound (tests/test_gpu_grad_guard_exact.py: the fp32 sum's own rounding where eps_s is unusually small)"""
    B, Nn = o["B"], o["Nn"]
    margin = kw.get("margin", 2.0)
    eps_s = 4 * max(np.abs(r32["target_score"] - r64["target_score"]).max(), np.abs(r32["negative_scores"] - r64["negative_scores"]).max())
    assert 0 < eps_s < 1e-5, eps_s
    d = r64["d"]
    near = np.abs(d) <= eps_s
    ordinary = np.ones(B, bool)
    ordinary[list(degenerate)] = False
    assert not near[ordinary].any(), "%s: a d_k within eps_s of 0 in an ordinary item: choose another seed" % tag
    assert not (np.abs(margin - d) <= eps_s).any(), "%s: a d_k within eps_s of the margin: choose another seed" % tag
    es = max(np.abs(o["target_score"][:, 0] - r64["target_score"]).max(), np.abs(o["negative_scores"] - r64["negative_scores"]).max())
    assert np.array_equal(o["target_score"], np.repeat(o["target_score"][:, :1], Nn, 1))
    lo = float((d < -eps_s).sum())
    el = abs(o["loss"][0] - r64["loss"])
    print("SSE %s: form %d h16 %d, eps_s %.3e, scores share %.3f, loss share %.3f (loss %.6g, sensitivity %.3g), violations %d, nearest boundary %.1f eps_s"
          % (tag, o["form"], o["h16"], eps_s, es / eps_s, el / (eps_s * r64["sens"]), r64["loss"], r64["sens"], int(o["loss"][1]),
             min(np.abs(d[ordinary]).min(initial=np.inf), np.abs(margin - d).min()) / eps_s))
    assert es <= eps_s, "%s: a score is %.3e from float64, bound %.3e" % (tag, es, eps_s)
    assert lo <= o["loss"][1] <= lo + near.sum(), "%s: violations %r, reference %r" % (tag, o["loss"][1], lo)
    assert el <= eps_s * r64["sens"] + loss_slack, "%s: loss %r, float64 %r, bound %.3e" % (tag, o["loss"][0], r64["loss"], eps_s * r64["sens"] + loss_slack)
    return eps_s


def first_bad(bad, got, want, bound, groups, CN, what):
    u, c = np.argwhere(bad)[0]
    inst = np.flatnonzero(groups["map"] == u)
    return "%s: %d elements in %d rows outside their bound; first at (slot %d, column %d): segment of %d instances (b, ch) %s: got %r, float64 %r, bound %.3e" % (
        what, int(bad.sum()), len(np.unique(np.argwhere(bad)[:, 0])), u, c, len(inst), [(int(i) // CN, int(i) % CN) for i in inst[:8]],
        got[u, c], want[u, c], bound[u, c])


def check_rows(got, ref64, ref32, scale, prec, tag, what, groups=None, CN=1, extra=None):
    """got, ref64, ref32 [n][D] in unscaled units -> the rule of the module docstring in scaled units"""
    sc = np.float64(scale)
    assert sc > 0 and np.frexp(sc)[0] == 0.5 and (prec == "f16" or sc == 1.0), "the gradient scale %r is no power of two" % scale
    g, w = got.astype(np.float64) * sc, ref64 * sc
    eps_g = 4 * np.abs(ref32.astype(np.float64) - ref64).max(1) * sc
    slack = eps_g[:, None] + (0 if extra is None else extra * sc)
    # the value the kernel rounds lies within `slack` of the reference: it is rounded at ITS magnitude, at most |reference| + slack -- the
    # spacing there, not at the reference, bounds the rounding (they differ only where the slack reaches into the next binade)
    half = ulp16(np.abs(w) + slack, prec) / 2
    bound = half + slack
    err = np.abs(g - w)
    assert np.abs(w).max() > 0 and np.isfinite(g).all()
    print("SSE %s %s: scale 2^%d, max |value| %.3e scaled, largest eps_g %.3e (%.3f of the largest half ulp), worst share of the bound %.3f%s"
          % (tag, what, int(np.log2(sc)), np.abs(w).max(), eps_g.max(), eps_g.max() / half.max(), (err / bound).max(),
             "" if extra is None else ", largest v16 term %.3e" % (extra * sc).max()))
    bad = err > bound
    if bad.any():
        if groups is None:
            groups = dict(map=np.arange(len(got)))
        raise AssertionError(first_bad(bad, g, w, bound, groups, CN, tag + " " + what))


def check_case(o, tag, want_form, want_h16=1, degenerate=(), v16=False):
    CN = o["C"] + o["Nn"]
    assert o["form"] == want_form, "%s ran score form %d, written for form %d" % (tag, o["form"], want_form)
    assert o["h16"] == want_h16, "%s: last_h16 %d" % (tag, o["h16"])
    r64, r32, kw = refs(o)
    check_forward(o, r64, r32, kw, tag, degenerate)
    gr, ex = o["groups"], r64["groups"]
    U = ex["U"]
    assert o["stats"] == (ex["R"], U) and np.array_equal(gr["map"], ex["map"])
    dyu = gr["dyu"]
    check_rows(dyu[:U], r64["dyu"], r32["dyu"], o["scale"], o["prec"], tag, "dyu", ex, CN, v16_term(r64, o["B"], o["C"], o["Nn"]) if v16 else None)
    Uk = (U + 63) // 64 * 64
    assert not dyu[U:Uk].any(), "%s: rows U .. ceil(U / 64) 64 of dYu are not zero (%d nonzero elements)" % (tag, np.count_nonzero(dyu[U:Uk]))
    if not kw.get("dropout_ratio"):
        first = np.full(U, -1)
        first[ex["map"][::-1]] = np.arange(ex["R"])[::-1]
        shared = instance_order(o["ip2"], o["B"])[first]
        assert not dyu[:U][shared <= 0].any(), "%s: a gradient where the shared ip2 value is 0" % tag
    return r64, U


def dedup_case(vv, world, prec, D, B, C, Nn, seed, tag, want_form, **more):  # noqa: F811
    o = run_case(vv, world, prec, D, batch(seed, B, C, Nn), C, Nn, **more)
    assert o["stats"][1] < o["stats"][0]
    check_case(o, "%s %s D %d B %d C %d Nn %d" % (tag, prec, D, B, C, Nn), want_form)
    return o


# ------------------------------------------------------------------------------- k_score_fwd: rows per wave, context bound, item map
@pytest.mark.parametrize("Nn", [15, 16, 31, 32, 55])
def test_rows_per_wave_bands(vv, world, Nn):  # noqa: F811
    """1 + Nn = 16 | 17, 32 | 33, 56: the last row of a wave's share in the RPW 2 / 4 / 7 instantiations"""
    dedup_case(vv, world, "f16", 512, 24, 5, Nn, 100 + Nn, "bands", 1)


@pytest.mark.parametrize("C,form", [(7, 1), (8, 2)])
def test_context_bound(vv, world, C, form):  # noqa: F811
    dedup_case(vv, world, "f16", 512, 24, C, 10, 110 + C, "context", form)


@pytest.mark.parametrize("B", [1, 7, 8, 9, 24])
def test_item_to_workgroup_map(vv, world, B):  # noqa: F811
    dedup_case(vv, world, "bf16" if B == 8 else "f16", 512, B, 5, 10, 120 + B, "items", 1)


# ------------------------------------------------------------------------------- k_score_stream on f16 rows, both chunk counts
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C,Nn", [(5, 56), (9, 10), (5, 70)])
def test_one_sweep_kernel_at_d512_on_f16_rows(vv, world, prec, C, Nn):  # noqa: F811
    dedup_case(vv, world, prec, 512, 24, C, Nn, 130 + C + Nn, "stream512", 2)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("v16", [0, 1])
@pytest.mark.parametrize("C,Nn", [(5, 20), (4, 200)])
def test_two_chunk_forms(vv, world, prec, v16, C, Nn):  # noqa: F811
    o = run_case(vv, world, prec, 1024, batch(140 + Nn, 16, C, Nn), C, Nn, opts=dict(v16=v16))
    check_case(o, "stream1024 v16=%d %s C %d Nn %d" % (v16, prec, C, Nn), 3, v16=bool(v16))


@pytest.mark.parametrize("D,C,Nn,form", [(512, 5, 20, 1), (512, 5, 70, 2), (1024, 5, 20, 3)])
def test_fp32_rows(vv, world, D, C, Nn, form):  # noqa: F811
    o = run_case(vv, world, "f16", D, batch(150 + form, 16, C, Nn), C, Nn, opts=dict(h16=0))
    check_case(o, "fp32 rows D %d C %d Nn %d" % (D, C, Nn), form, want_h16=0)


# ------------------------------------------------------------------------------- k_seg_bwd: segment lengths, degenerate segments, grid
@pytest.mark.parametrize("prec,D", [("f16", 512), ("bf16", 512), ("f16", 1024)])
def test_segment_lengths(vv, world, prec, D):  # noqa: F811
    """Slots of exactly 1, 2, 3, 4, 5, 63, 64, 65 and 130 instances: the unroll tails (4 at D = 512, 2 at D = 1024), the instance-order
    strip up to 64, the order-independent sums from 65.  The long rows sit in negative and context positions only."""
    B, C, Nn = 24, 5, 20
    CN = C + Nn
    rng = np.random.default_rng(160)
    lens = [130, 65, 64, 63, 5, 4, 3, 2, 1]
    rows = 300 + np.arange(len(lens))
    idx = np.empty((B, CN), np.int32)
    idx[:, 0] = 400 + np.arange(B)                                       # targets: a row each
    free = rng.permutation([(b, ch) for b in range(B) for ch in range(1, CN)])
    fill = np.concatenate([np.repeat(rows, lens), 450 + np.arange(len(free) - sum(lens)) // 2])      # the rest: pairs
    for (b, ch), r in zip(free, fill):
        idx[b, ch] = r
    o = run_case(vv, world, prec, D, idx, C, Nn)
    r64, U = check_case(o, "segments %s D %d" % (prec, D), 1 if D == 512 else 3, v16=D == 1024)         # (v16 is on by default at D = 1024)
    cnt = r64["groups"]["cnt"][:U]
    assert set(lens) <= set(cnt.tolist()) and cnt.max() == 130


def test_one_slot_holds_everything(vv, world):  # noqa: F811
    B, C, Nn = 24, 5, 10
    o = run_case(vv, world, "f16", 512, np.full((B, C + Nn), 7, np.int32), C, Nn)
    assert o["stats"] == (B * (C + Nn), 1)
    check_case(o, "one slot", 1, degenerate=range(B))


def test_no_repeats(vv, world):  # noqa: F811
    B, C, Nn = 24, 5, 10
    idx = np.random.default_rng(170).permutation(N_ROWS)[:B * (C + Nn)].astype(np.int32).reshape(B, C + Nn)
    o = run_case(vv, world, "f16", 512, idx, C, Nn)
    assert o["stats"] == (idx.size, idx.size)
    check_case(o, "no repeats", 1)


def test_empty_slots(vv, world):  # noqa: F811
    """-1 in a target, a context and a negative position of three items, and item 5 all -1: every one of them reads the zero row's slot"""
    B, C, Nn = 24, 5, 10
    idx = batch(171, B, C, Nn)
    idx[2, 0] = -1; idx[9, 2] = -1; idx[14, C + 3] = -1
    idx[5] = -1
    o = run_case(vv, world, "f16", 512, idx, C, Nn)
    r64, U = check_case(o, "empty slots", 1, degenerate=[5])
    u = r64["groups"]["map"][5 * (C + Nn)]
    assert r64["groups"]["uniq_rows"][u] == N_ROWS and r64["groups"]["cnt"][u] == C + Nn + 3


def test_past_one_pass_of_the_persistent_grid(vv, world):  # noqa: F811
    """U > 4096 = SEGB_BLOCKS x 4 waves: every wave's second row, reached through the prefetched segment bounds"""
    B, C, Nn, n_rows = 80, 5, 50, 4400
    flat = np.random.default_rng(173).permutation(n_rows)[:B * (C + Nn)].astype(np.int32)
    flat[-100:] = flat[:100]                                             # (the last two items repeat rows of items 0 and 1)
    o = run_case(vv, world, "f16", 512, flat.reshape(B, C + Nn), C, Nn, n_rows=n_rows)
    r64, U = check_case(o, "persistent grid", 1)
    assert U == 4300 and o["stats"][1] < o["stats"][0]


# ------------------------------------------------------------------------------- dropout masks, options of the loss, counting twin
@pytest.mark.parametrize("dd,D,C,Nn,form", [(1, 512, 5, 10, 1), (2, 512, 5, 70, 2), (2, 1024, 5, 20, 3)])
def test_dropout_masks(vv, world, dd, D, C, Nn, form):  # noqa: F811
    """ratio 0.5: one slot carries differently masked instances (the per-column beta sums of the DROP forms)"""
    o = run_case(vv, world, "f16", D, batch(180 + form, 24, C, Nn), C, Nn, opts=dict(drop_dedup=dd), dropout_ratio=0.5, dropout_seed=5)
    assert o["stats"][1] < o["stats"][0]
    assert 0.65 < (o["ip2"] == 0).mean() < 0.85                           # ReLU leaves about half, the masks half of that
    check_case(o, "dropout drop_dedup=%d D %d C %d Nn %d" % (dd, D, C, Nn), form)


LOSS_OPTIONS = {"L1": dict(norm="L1", margin=0.1), "item_weight": dict(item_weight=(1 + np.arange(24) % 4).astype(np.float32)),
                "loss_weight": dict(loss_weight=2.0), "global_count": dict(global_count=4 * 24 * 20), "ctx_coeff": dict(ctx_coeff=[0.1, 0.2, 0.3, 0.4]),
                "margin": dict(margin=0.5)}


@pytest.mark.parametrize("name", list(LOSS_OPTIONS))
def test_options_of_the_loss(vv, world, name):  # noqa: F811
    o = run_case(vv, world, "f16", 512, batch(190, 24, 5, 20), 5, 20, **LOSS_OPTIONS[name])
    r64, U = check_case(o, "option " + name, 1)
    if name in ("L1", "margin"):
        act = r64["d"] < LOSS_OPTIONS[name]["margin"]
        assert 0 < act.sum() < act.size                                  # hinges on both sides


@pytest.mark.parametrize("D,C,Nn,form,opts", [(512, 5, 20, 1, {}), (1024, 5, 20, 3, dict(v16=1))])
def test_counting_twin(vv, world, D, C, Nn, form, opts):  # noqa: F811
    idx = batch(200 + form, 16, C, Nn)
    a = run_case(vv, world, "f16", D, idx, C, Nn, opts=dict(h16_guard=0, **opts))
    b = run_case(vv, world, "f16", D, idx, C, Nn, opts=dict(h16_guard=1, **opts))
    check_case(b, "counting twin D %d" % D, form, v16=bool(opts))
    assert a["scale"] == b["scale"] and np.array_equal(a["groups"]["dyu"], b["groups"]["dyu"]) and a["loss"] == b["loss"]
    assert np.array_equal(a["negative_scores"], b["negative_scores"]) and np.array_equal(a["dW"], b["dW"])


# ------------------------------------------------------------------------------- the per-instance kernels (form 4)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("how,D", [("dense", 512), ("rows", 512), ("rows", 320)])
def test_per_instance_kernels(vv, world, prec, how, D):  # noqa: F811
    """Dense execution and VV_SEG_BWD=0 (k_score_loss_reg at D = 512), D = 320 (k_score_loss): ip1_diff, per instance and times the scale,
    is held to dY by the rule that holds dyu on the segment-wise path."""
    B, C, Nn = 24, 5, 20
    o = run_case(vv, world, prec, D, batch(210, B, C, Nn), C, Nn, dedup=how != "dense", seg_bwd=False if (how, D) == ("rows", 512) else None, form4=True)
    tag = "per-instance %s %s D %d" % (how, prec, D)
    assert o["form"] == 4 and o["h16"] == 0
    # the guard is idle here: a repeat that took a power of two off the scale without need would be wrong, although the rows would still pass
    assert (o["grad_shift"], o["grad_shift_round1"], o["grad_repeat"]) == (0, 0, 0) and o["scale"] == o["sg"]
    r64, r32, kw = refs(o)
    check_forward(o, r64, r32, kw, tag)
    check_rows(instance_order(o["ip1_diff"], B), r64["dY"], r32["dY"], o["scale"], prec, tag, "ip1_diff", None, C + Nn)


# ------------------------------------------------------------------------------- the small end of the two power-of-two scales
TINY = 2.0 ** -108


def rel64(a, ref):
    """relative Frobenius distance in float64 (float32 squares of values near 2^-116 underflow)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def tiny_run(vv, world, D, **opts):  # noqa: F811
    C, Nn = 5, 20
    return run_case(vv, world, "bf16", D, batch(220, 16, C, Nn), C, Nn, opts=opts, loss_weight=TINY)


def test_tiny_gradients_through_the_f16_vector_scale(vv, world):  # noqa: F811
    """D = 1024, v16 = 1, slab16 = 1: dA_b leaves k_score_stream as f16 times 2^(14 - e), the split-K partial products leave the weight
    gradient as f16 times 2^(15 - e); with the largest |dA_b| below 2^-113 an unclamped 14 - e passes 127."""
    s = tiny_run(vv, world, 1024, v16=1, slab16=1)
    r64, U = check_case(s, "tiny v16 slab16 D 1024", 3, v16=True)
    assert np.abs(r64["dA"]).max() < 2.0 ** -113 and np.abs(r64["dyu"]).max() >= 2.0 ** -120
    a = tiny_run(vv, world, 1024, v16=0, slab16=0)
    assert 1 < s["splits"] <= 8                                          # (the f16 partial products need several splits, at most eight)
    assert np.isfinite(s["dW"]).all() and np.abs(a["dW"]).max() > 0
    print("SSE tiny D 1024: max |dA_b| 2^%.1f, max |dyu| 2^%.1f, dW %.3e db %.3e from the fp32 forms" % (
        np.log2(np.abs(r64["dA"]).max()), np.log2(np.abs(r64["dyu"]).max()), rel64(s["dW"], a["dW"]), rel64(s["db"], a["db"])))
    # tests/test_gpu_h16.py: v16 moves a bf16 run's dW by at most 4e-3 and db by 1e-3, slab16 dW by 1e-3 more
    assert 0 < rel64(s["dW"], a["dW"]) <= 4e-3 + 1e-3 and rel64(s["db"], a["db"]) <= 1e-3


def test_tiny_gradients_through_the_f16_tile_scale(vv, world):  # noqa: F811
    s = tiny_run(vv, world, 512, slab16=1)
    a = tiny_run(vv, world, 512, slab16=0)
    r64, U = check_case(s, "tiny slab16 D 512", 1)
    assert 1 < s["splits"] <= 8
    assert np.abs(a["dW"]).max() < 2.0 ** -112 and np.abs(a["dW"]).max() > 0
    assert np.array_equal(s["groups"]["dyu"], a["groups"]["dyu"]) and np.array_equal(s["db"], a["db"])
    assert np.isfinite(s["dW"]).all()
    tile_max = np.abs(a["dW"]).reshape(512 // 256, 256, 1, F).max(axis=(1, 3))
    slack = np.repeat(tile_max, 256, axis=0)
    print("SSE tiny D 512: max |dW| 2^%.1f, slab16 moves dW by %.3e" % (np.log2(np.abs(a["dW"]).max()), rel64(s["dW"], a["dW"])))
    # tests/test_gpu_h16.py's bounds (without its absolute 1e-12, which would swallow these values)
    assert 0 < rel64(s["dW"], a["dW"]) <= 1e-3 and np.all(np.abs(s["dW"] - a["dW"]) <= 16 * 2.0 ** -11 * 8 * slack)
