"""The f16 gradient-scale guard (vv_internal.h: GradGuard) held to tests/guard_ref.py and to float64, with the guard ACTIVE: the shifts of the
conditional repeats, the rows they write, the proactive form of the segment-wise backward, the guard's multiplier in every update form and
the host's steering at its fixed lag.  tests/test_gpu_score_seg_exact.py runs the same kernels with the guard idle; its world, batches,
run_case and rules are used here.

Paths (B = 24, C = 5, Nn = 20, F = 128, 640 table rows; magnitudes are loss_weight = 2^k, so that everything scales exactly):
  seg    de-duplicated, segment-wise backward: D = 512 (k_score_fwd), D = 1024 (k_score_stream, two chunks); proactive, no repeat
  sum    de-duplicated, VV_SEG_BWD=0: D = 512 (k_score_loss_reg + k_segsum), D = 320 (k_score_loss + k_segsum); two guard rounds
  dense  de-duplication off: D = 512, D = 320; one guard round
The records "last_grad_shift", "last_grad_shift_round1", "last_grad_repeat" say what the device decided; on the reactive paths they must
EQUAL guard_ref's, after guard_ref has shown that every decision of the case is a factor 1 +- 2^-10 from its threshold (a condition on the
inputs).  The rows are held by check_rows' rule at the step's real scale S = grad_scale_stats()[1] 2^-last_grad_shift:
|got S - ref64 S| <= ulp16 / 2 + eps_g.

On the `sum` path dyu is a sum of rows that were rounded already (k_segsum adds the stored rows in double and rounds once more), so the
rule cannot hold for it as it stands; there the per-instance rows (ip1_diff) are held to the rule, dyu S must be the f16 rounding of the
double sum of the rows as read back, and dyu is held to the rule widened by exactly the rows' own half ulps (check_rows' `extra`).  The
exact-sum bound is ulp16 / 2 (1 + 2^-12): k_segsum converts double -> float -> f16, and rounding twice can pass half an f16 ulp only by
half an fp32 ulp, 2^-13 of an f16 ulp for a normal value; the factor covers that and nothing else.

Observed on an MI355X, 41 cases, 5.5 s for the whole file (every case prints "GG ..." lines: form, scale, shifts, looseness, worst share):
  a   seg: proactive shift 11 at k = 18, -27 at k = -20 (scale 2^-2 / 2^36), max |dyu| scaled 187.9 (D = 512) and 123.2 (D = 1024), looseness
      87 and 133.  sum / dense, k = 18: shift 7 (D = 512), 8 (D = 320), round 2 idle; nearest decision at 0.73 / 1.20 of its threshold; the
      worst element of every row check at 0.99 .. 1.00 of its bound; dyu at 0.9998 of the half ulp around the double sums of the stored rows.
  b   sums_only: k = 12 (D = 512), 11 (D = 320), shift 4, the sums at 1.29 / 1.23 of the limit.  both_rounds (k = 24, the batch of equal
      items): round 1 takes 13, round 2 five more (18); the sums of clipped rows reported 480 x 65504.  idle: all records 0.
  c   looseness 43.7 / 66.3 with distinct negatives (D = 512 / 1024), 791 / 1345 with the 480-fold row: past the 2^10 that the kernel's
      comment ("tens to hundreds") allowed.  The values stay normal f16 numbers (largest 20.7 and 12.2) and every element passes rule (a), so
      the comment in kernels_score.hip now states the measured values and the bound asserted here is 2^11.  cnt_max: 480 against 3, log2 of
      the products' ratio 7.28 / 7.32, shifts 17 - 10 = 7.
  d   seg: shifts -27, -7, 11 for k = -20, 0, 18; dyu, dW, db, loss bit-identical.  sum / dense: k = 18 and 24 bit-identical (shifts 7 / 13,
      8 / 14); against k = 0 under 1 % of the non-zero elements are subnormal in one run (a sum counts as such when one of its rows is).
  e   W, b and both histories bit-identical across k in all five forms on both paths; forms 4 and 5 on the dense path at k = 24 / 30 (the
      update file's shapes are idle at k = 18).
  f   scale 512 for four steps, then 1 (k = 18) or 2^38 (k = -20) from the fifth; repeats 0 0 0 0 1 2 3 4 4 ...; shift 7 with a repeat in the
      first four steps at k = 18, none afterwards; the same with a run_state round trip behind the third step.
Two comments were wrong and are corrected with this file: the looseness above, and api.hip's steering window (the code and the protocol
move the scale when the exponent leaves 5 .. 13, that is [2^4, 2^13), not [2^5, 2^13)).

Run against mutated kernels (scratch builds only, one change each; this file and tests/test_gpu_dedup.py, 56 cases; every mutant gives
wrong numbers only):
  shift e - 11 in gg_begin                  16 fail: a's four reactive cases and b's sums_only / both_rounds (records != reference), d's four
                                            reactive cases, f at k = 18 (the shift of the first four steps).  test_gpu_dedup.py: none
  cnt_max dropped from the proactive G      2 fail: c at D = 512 and 1024 (the shift difference).  test_gpu_dedup.py: none
  gg->mul out of grad_unscale               22 fail: all ten cases of e, d's six, and 6 of test_gpu_dedup.py
    ... at the GEMM epilogue's call only    2 fail: e's two form-5 cases, nothing else anywhere
    ... at k_reduce's call only             16 fail: e's four cases of forms 1 and 2, d's six, 6 of test_gpu_dedup.py
    ... at k_reduce_sgd's call only         5 fail: e's four cases of forms 3 and 4, test_gpu_dedup.py's long run
  round 2 removed (n_rounds 1, rows + sums) 2 fail: b both_rounds at D = 512 and 320, nothing else
  kLag 3                                    8 fail: every case of f.  test_gpu_dedup.py: none
No mutant fails none.  Five of the eight are seen by this file alone.
"""
import os

import numpy as np
import pytest

from tests.guard_ref import LIMIT, guard_rounds, margin_ok, steering_run
from tests.score_ref import instance_order, ulp16, v16_term
from tests.test_gpu_parity import vv  # noqa: F401  (fixture)
from tests.test_gpu_score_seg_exact import N_ROWS, batch, check_case, check_forward, check_rows, refs, run_case, world  # noqa: F401

pytestmark = pytest.mark.gpu

B, C, Nn = 24, 5, 20
CN = C + Nn
PATHS = {"seg": dict(dedup=True, seg_bwd=None), "sum": dict(dedup=True, seg_bwd=False), "dense": dict(dedup=False)}
FORM = {("seg", 512): 1, ("seg", 1024): 3}
SEED = 310


def ordinary():
    return batch(SEED, B, C, Nn)


def shared_negative():
    """one negative row shared by all B Nn = 480 negative instances (cnt_max = 480)"""
    idx = batch(SEED, B, C, Nn)
    idx[:, C:] = 137
    return idx


def distinct_negatives():
    """the same targets and contexts, every negative instance a row of its own"""
    idx = batch(SEED, B, C, Nn)
    idx[:, C:] = (100 + np.random.default_rng(SEED).permutation(B * Nn)).reshape(B, Nn)
    return idx


def run(vv, world, path, D, idx, k, prec="f16", **more):  # noqa: F811
    o = run_case(vv, world, prec, D, idx, C, Nn, form4=path != "seg", loss_weight=2.0 ** k, **PATHS[path], **more)
    o["path"], o["k"] = path, k
    return o


def guard_of(o, r64, tag):
    """guard_ref's answer for a reactive case, its margin condition asserted; the records compared with =="""
    g = guard_rounds(r64["dY"], float(o["sg"]), o["path"], seg_map=r64["groups"]["map"] if o["path"] == "sum" else None)
    ok, worst = margin_ok(g["decisions"])
    print("GG %s: sg 2^%d, reference rounds %s, nearest decision %s at %.6f of its threshold; records shift %d, round 1 %d, repeat %d"
          % (tag, int(np.log2(o["sg"])), [(q["active"], q["shift"]) for q in g["rounds"]], worst[0], worst[1], o["grad_shift"],
             o["grad_shift_round1"], o["grad_repeat"]))
    assert ok, "%s: %s lies at %.6f of its threshold: move the seed or k" % (tag, worst[0], worst[1])
    assert (o["grad_repeat"], o["grad_shift"], o["grad_shift_round1"]) == (g["repeat"], g["shift"], g["shift_round1"]), \
        "%s: records (repeat, shift, round 1) %r, reference %r" % (tag, (o["grad_repeat"], o["grad_shift"], o["grad_shift_round1"]), (g["repeat"], g["shift"], g["shift_round1"]))
    assert o["scale"] == g["scale"]
    return g


def rows_extra(r64, S):
    """[U][D], unscaled: the half ulps of the rows as the score kernel stored them, summed per slot (the `sum` path's first rounding)"""
    per = ulp16(np.abs(r64["dY"]) * S * (1 + 2.0 ** -20), "f16") / 2 / S * (r64["dY"] != 0)
    out = np.zeros_like(r64["dyu"])
    np.add.at(out, r64["groups"]["map"].astype(np.int64), per)
    return out


def check_reactive(o, tag, loss_rel=0.0):
    """rule (a) of a `sum` / `dense` case at the step's real scale; returns (r64, guard_ref's answer)"""
    assert o["form"] == 4 and o["h16"] == 0
    r64, r32, kw = refs(o)
    check_forward(o, r64, r32, kw, tag, loss_slack=loss_rel * abs(float(r64["loss"])))
    g = guard_of(o, r64, tag)
    S = np.float64(o["scale"])
    top = np.abs(r64["dY"]).max() * S
    rows = instance_order(o["ip1_diff"], B)
    check_rows(rows, r64["dY"], r32["dY"], o["scale"], "f16", tag, "ip1_diff", None, CN)
    if o["path"] == "sum":
        U = r64["groups"]["U"]
        assert o["stats"] == (B * CN, U) and np.array_equal(o["groups"]["map"], r64["groups"]["map"])
        top = max(top, np.abs(r64["dyu"]).max() * S)
        stored = rows.astype(np.float64) * S
        assert np.array_equal(stored, stored.astype(np.float16).astype(np.float64)), "ip1_diff x scale is no f16 value"
        sums = np.zeros((U, o["D"]))
        np.add.at(sums, r64["groups"]["map"].astype(np.int64), stored)
        got = o["groups"]["dyu"][:U].astype(np.float64) * S
        err = np.abs(got - sums)
        bound = ulp16(sums, "f16") / 2 * (1 + 2.0 ** -12)
        print("GG %s: dyu against the double sums of the stored rows: worst share of the half ulp %.4f" % (tag, (err / bound).max()))
        assert (err <= bound).all(), "%s: %d elements of dyu are not the rounded sum of the stored rows" % (tag, int((err > bound).sum()))
        check_rows(o["groups"]["dyu"][:U], r64["dyu"], r32["dyu"], o["scale"], "f16", tag, "dyu", r64["groups"], CN, rows_extra(r64, S))
    assert top < 65504, "%s: the reference itself passes f16's range at this scale (%.4g)" % (tag, top)
    if g["rounds"][-1]["active"]:
        assert 2.0 ** 11 * (1 + 2.0 ** -10) <= top <= 2.0 ** 12 * (1 - 2.0 ** -10), "%s: after an active final round the maximum is %.6g" % (tag, top)
    return r64, g


def check_seg(o, tag):
    """rule (a) and the proactive form's own claims; returns (r64, looseness)"""
    r64, U = check_case(o, tag, FORM[("seg", o["D"])], v16=o["D"] == 1024)
    top = np.abs(r64["dyu"]).max() * np.float64(o["scale"])
    L = 2.0 ** 14 / top
    print("GG %s: proactive shift %d, scale 2^%d, max |dyu| scaled %.4g, looseness %.1f" % (tag, o["grad_shift"], int(np.log2(o["scale"])), top, L))
    assert o["grad_repeat"] == 0 and top < 2.0 ** 14, (tag, o["grad_repeat"], top)
    assert L <= 2.0 ** 11, "%s: the bound is %.0f times the true maximum; the bound asserted is what kernels_score.hip's comment states" % (tag, L)
    return r64, L


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert np.array_equal(a, b), "%s: %d of %d elements differ" % (what, int((a != b).sum()), a.size)


def descaled(o, k):
    """the step's outputs times 2^-k (exact in float32)"""
    s = np.float32(2.0 ** -k)
    d = dict(dW=o["dW"] * s, db=o["db"] * s, loss=np.float32(o["loss"][0]) * s)
    if o["path"] != "dense":
        d["dyu"] = o["groups"]["dyu"][:o["stats"][1]] * s
    if o["path"] != "seg":
        d["ip1_diff"] = o["ip1_diff"] * s
    return d


# ------------------------------------------------------------------------------- a. element by element under an active guard
@pytest.mark.parametrize("D", [512, 1024])
@pytest.mark.parametrize("k", [18, -20])
def test_segment_path_rows_exact_under_a_shift(vv, world, D, k):  # noqa: F811
    o = run(vv, world, "seg", D, ordinary(), k)
    assert o["grad_shift"] != 0 and (o["grad_shift"] > 0) == (k > 0)
    check_seg(o, "a seg D %d k %d" % (D, k))


@pytest.mark.parametrize("path,D", [("sum", 512), ("sum", 320), ("dense", 512), ("dense", 320)])
def test_repeat_rows_exact_and_shift_equal_to_the_reference(vv, world, path, D):  # noqa: F811
    o = run(vv, world, path, D, ordinary(), 18)
    r64, g = check_reactive(o, "a %s D %d k 18" % (path, D))
    assert g["repeat"] == 1 and o["grad_shift"] > 0


def test_bf16_has_no_guard(vv, world):  # noqa: F811
    for path in ("seg", "dense"):
        o = run(vv, world, path, 512, ordinary(), 18, prec="bf16")
        assert (o["grad_shift"], o["grad_shift_round1"], o["grad_repeat"], o["scale"], o["sg"]) == (0, 0, 0, 1.0, 1.0)


# ------------------------------------------------------------------------------- b. the two-round cases, named by what they reach
# (k chosen from the reference; the case asserts that it reaches what it is named for).  With the shared negative row the largest sum is
# only 7 to 8 times the largest row (the items' gradients of the row partly cancel): from k = 21 the sums of clipped rows saturate at
# 480 x 65504 < 2^25, a shift of 13, and the true sums pass 2^15 x 2^13 only from k = 25 -- where the rows' own true maximum has taken the
# decision over.  No k makes round 2 active with that batch.  `both_rounds` therefore runs the batch whose items are all item 1 of it (every
# negative instance the same gradient: the sums are 24 times the largest row), where k = 24 clips the rows and round 1's true sums pass again.
TWO_ROUND = {("sums_only", 512): 12, ("sums_only", 320): 11, ("both_rounds", 512): 24, ("both_rounds", 320): 24, ("idle", 512): 0, ("idle", 320): 0}


def coherent_negative():
    idx = shared_negative()
    idx[:] = idx[1]
    return idx


@pytest.mark.parametrize("D", [512, 320])
@pytest.mark.parametrize("name", ["sums_only", "both_rounds", "idle"])
def test_two_rounds(vv, world, D, name):  # noqa: F811
    k = TWO_ROUND[(name, D)]
    o = run(vv, world, "sum", D, coherent_negative() if name == "both_rounds" else shared_negative(), k)
    tag = "b %s D %d k %d" % (name, D, k)
    # (both_rounds: 24 equal items leave eps_s at 5e-8 -- few distinct scores -- and eps_s x sensitivity, 3.1 at D = 320, below the half ulp32
    # of the loss itself, 4 at 6.85e7; the kernel's loss was 11.2 away.  The scores and the violations are held as everywhere; the loss's bound
    # gains the rounding of its own fp32 sum: Nn terms per item in turn, B items, the scale and the result, (Nn + B + 2) 2^-24 |loss| = 188)
    r64, g = check_reactive(o, tag, loss_rel=(Nn + B + 2) * 2.0 ** -24 if name == "both_rounds" else 0.0)
    r1, r2 = g["rounds"]
    assert r64["groups"]["cnt"].max() == B * Nn
    if name == "sums_only":
        assert r1["rows_max"] < LIMIT < r1["sums_max"] and r1["active"] and not r2["active"], (tag, g["rounds"])
    elif name == "both_rounds":
        assert r1["rows_max"] > 65504 and r1["active"] and r2["active"] and r2["sums_max"] > LIMIT and g["shift"] > g["shift_round1"] > 0, (tag, g["rounds"])
    else:
        assert not r1["active"] and not r2["active"] and (o["grad_shift"], o["grad_shift_round1"], o["grad_repeat"]) == (0, 0, 0)


# ------------------------------------------------------------------------------- c. the proactive form
@pytest.mark.parametrize("D", [512, 1024])
def test_proactive_bound_and_cnt_max(vv, world, D):  # noqa: F811
    """Looseness of the bound (2^14 over the true scaled maximum), and cnt_max in it: with the 480-fold row the shift must exceed the shift
    of the same batch with distinct negatives by log2 of the ratio of (largest instance count x largest |dY| element), +- 1."""
    s = run(vv, world, "seg", D, shared_negative(), 18)
    d = run(vv, world, "seg", D, distinct_negatives(), 18)
    rs, Ls = check_seg(s, "c shared D %d" % D)
    rd, Ld = check_seg(d, "c distinct D %d" % D)
    ps = rs["groups"]["cnt"].max() * np.abs(rs["dY"]).max()
    pd = rd["groups"]["cnt"].max() * np.abs(rd["dY"]).max()
    assert rs["groups"]["cnt"].max() == B * Nn and rd["groups"]["cnt"].max() < 16
    ratio = np.log2(ps / pd)
    diff = s["grad_shift"] - d["grad_shift"]
    print("GG c D %d: cnt_max %d / %d, log2 of the products' ratio %.2f, shifts %d - %d = %d" % (
        D, rs["groups"]["cnt"].max(), rd["groups"]["cnt"].max(), ratio, s["grad_shift"], d["grad_shift"], diff))
    assert np.floor(ratio) - 1 <= diff <= np.ceil(ratio) + 1


# ------------------------------------------------------------------------------- d. exact invariance under powers of two
@pytest.mark.parametrize("D", [512, 1024])
def test_segment_path_invariant_under_powers_of_two(vv, world, D):  # noqa: F811
    ks = (-20, 0, 18)
    outs = [run(vv, world, "seg", D, ordinary(), k) for k in ks]
    base = descaled(outs[1], 0)
    for o, k in zip(outs, ks):
        assert o["grad_shift"] - outs[1]["grad_shift"] == k, [q["grad_shift"] for q in outs]
        for name, v in descaled(o, k).items():
            same_bits(v, base[name], "seg D %d: %s at k = %d against k = 0" % (D, name, k))
    print("GG d seg D %d: shifts %r, bit-identical dyu, dW, db, loss" % (D, [q["grad_shift"] for q in outs]))


@pytest.mark.parametrize("path,D", [("sum", 512), ("sum", 320), ("dense", 512), ("dense", 320)])
def test_repeat_paths_invariant_under_powers_of_two(vv, world, path, D):  # noqa: F811
    o18, o24, o0 = (run(vv, world, path, D, ordinary(), k) for k in (18, 24, 0))
    tag = "d %s D %d" % (path, D)
    r64, g18 = check_reactive(o18, tag + " k 18")
    _, g24 = check_reactive(o24, tag + " k 24")
    assert g18["repeat"] == 1 and g24["repeat"] == 1 and not o0["grad_repeat"]
    # the two active runs end at the same effective scale (asserted from the reference: a condition on the inputs) ...
    assert g18["scale"] * 2.0 ** 18 == g24["scale"] * 2.0 ** 24, "%s: the reference's final scales differ: %r, %r" % (tag, g18["rounds"], g24["rounds"])
    a, b = descaled(o18, 18), descaled(o24, 24)
    for name in a:
        same_bits(a[name], b[name], "%s: %s at k = 24 against k = 18" % (tag, name))
    # ... and against the idle run every element that is a normal f16 number in both
    key = "ip1_diff" if path == "dense" else "dyu"
    ref = r64["dY"] if path == "dense" else r64["dyu"]
    got18 = instance_order(a[key], B) if path == "dense" else a[key]
    got0 = instance_order(o0["ip1_diff"], B) if path == "dense" else o0["groups"]["dyu"][:o0["stats"][1]]
    low = 2.0 ** -14 * (1 + 2.0 ** -10)
    sub = (np.abs(ref) * o18["scale"] < low) | (np.abs(ref) * 2.0 ** -18 * o0["scale"] < low)      # (ref: at k = 18)
    sub &= ref != 0
    if path == "sum":                                     # a sum is left out too where one of ITS rows is subnormal in one of the runs
        rsub = ((np.abs(r64["dY"]) * o18["scale"] < low) | (np.abs(r64["dY"]) * 2.0 ** -18 * o0["scale"] < low)) & (r64["dY"] != 0)
        any_row = np.zeros(ref.shape, np.int64)
        np.add.at(any_row, r64["groups"]["map"].astype(np.int64), rsub.astype(np.int64))
        sub |= any_row > 0
    share = sub.sum() / max(1, (ref != 0).sum())
    print("GG %s: %.3f %% of the non-zero elements are subnormal in one of the runs and left to rule (a)" % (tag, 100 * share))
    assert share < 0.05
    same_bits(got18[~sub], got0[~sub], "%s: %s at k = 18 against k = 0 (normal elements)" % (tag, key))


# ------------------------------------------------------------------------------- e. the guard's multiplier in every update form
# (form, path, D, F, options): forms 1 and 2 at this file's shapes (F = 126: the scalar k_sgd).  Forms 3 and 4 need at most 8 splits of K
# (512 x 128 has 12: it runs form 1 whatever fuse_update says), form 5 one split: tests/test_gpu_update_exact.py's smallest shapes for them
# (100 x 128, 1028 x 4096, 4090 x 4092; B = 32, C = 5, Nn = 4, 3000 rows), which only the dense path runs; on the segment path, which needs
# D = 512 or 1024, F = 4096 gives 8 splits (forms 3 and 4) and 1024 x 16384 one (form 5).
UPDATE_CASES = [
    (1, "seg", 512, 128, dict(fuse_update=0)), (2, "seg", 512, 126, dict(fuse_update=0)), (3, "seg", 512, 4096, dict(fuse_update=1)),
    (4, "seg", 512, 4096, dict(fuse_update=1, slab16=1)), (5, "seg", 1024, 16384, dict(fuse_update=1, wgrad_update=1)),
    (1, "dense", 512, 128, dict(fuse_update=0)), (2, "dense", 512, 126, dict(fuse_update=0)), (3, "dense", 100, 128, dict(fuse_update=1)),
    (4, "dense", 1028, 4096, dict(fuse_update=1, slab16=1)), (5, "dense", 4090, 4092, dict(fuse_update=1, wgrad_update=1)),
]


@pytest.mark.parametrize("form,path,D,F,opts", UPDATE_CASES)
def test_guard_multiplier_in_every_update_form(vv, form, path, D, F, opts):  # noqa: F811
    big = path == "dense" and form >= 3
    b_, c_, n_, n_rows = (32, 5, 4, 3000) if big else (B, C, Nn, N_ROWS)
    rng = np.random.default_rng(D + F + form)
    W = rng.uniform(-0.05, 0.05, size=(D, F)).astype(np.float32)
    b = (rng.standard_normal(D) * 0.05).astype(np.float32)
    hW, hb = (rng.standard_normal((D, F)) * 1e-4).astype(np.float32), (rng.standard_normal(D) * 1e-4).astype(np.float32)
    idx = rng.integers(0, n_rows, size=(b_, c_ + n_)).astype(np.int32) if big else ordinary()
    ends, shifts = [], []
    # (the dense path at the update file's shapes -- 128 triplets, smaller gradients -- is idle at k = 18: 24 and 30 are both active there)
    ks = (0, 18) if path == "seg" else (24, 30) if big and form >= 4 else (18, 24)
    for k in ks:
        eng = vv.Engine(0, "f16")
        try:
            eng.set_dedup(path != "dense")
            for name, v in {"slab16": 0, "wgrad_update": 1, **opts}.items():
                eng.set_option(name, v)
            eng.table_synth(7, n_rows, F)
            eng.params_set(W, b, hW, hb)
            cfg = vv.StepConfig(b_, c_, n_, lr=0.05 * 2.0 ** -k, loss_weight=2.0 ** k, momentum=0.9, weight_decay=0.0)
            if form == 5:                                  # (as tests/test_gpu_update_exact.py reaches the forms)
                eng.update_hint(cfg)
            eng.forward_backward(cfg, idx)
            eng.apply_update(cfg)
            got = int(eng.get_option("last_update_form"))
            assert got == form, "%s D %d F %d ran update form %d, written for form %d (%d splits)" % (path, D, F, got, form, int(eng.get_option("last_wgrad_splits")))
            assert int(eng.get_option("last_score_form")) == (FORM[("seg", D)] if path == "seg" else 4)
            shifts.append((int(eng.get_option("last_grad_shift")), int(eng.get_option("last_grad_repeat"))))
            ends.append(eng.params_get())
        finally:
            eng.close()
    print("GG e form %d %s %d x %d: (shift, repeat) %r" % (form, path, D, F, shifts))
    assert shifts[1][0] - shifts[0][0] == (18 if path == "seg" else 6) and (path == "seg" or shifts[0][1] == shifts[1][1] == 1)
    assert float((ends[0][0] != W).mean()) > 0.9
    for name, x, y in zip(("W", "b", "hW", "hb"), ends[0], ends[1]):
        same_bits(x, y, "form %d %s: %s after the step across k" % (form, path, name))


# ------------------------------------------------------------------------------- f. steering at the fixed lag
def make_engine(vv, world, path, D):  # noqa: F811
    table, W, b = world(D, N_ROWS)
    os.environ["VV_SEG_BWD"] = "0"
    try:
        eng = vv.Engine(0, "f16")
    finally:
        os.environ.pop("VV_SEG_BWD", None)
    eng.set_dedup(path != "dense")
    eng.table_set(table)
    eng.params_set(W, b)
    return eng


@pytest.mark.parametrize("roundtrip", [False, True])
@pytest.mark.parametrize("k", [18, -20])
@pytest.mark.parametrize("path,D", [("dense", 512), ("sum", 512)])
def test_steering_at_the_fixed_lag(vv, world, path, D, k, roundtrip):  # noqa: F811
    idx, steps = ordinary(), 12
    cfg = vv.StepConfig(B, C, Nn, loss_weight=2.0 ** k)
    eng = make_engine(vv, world, path, D)
    seen, want, r64 = [], None, None
    try:
        for i in range(steps):
            if roundtrip and i == 3:                      # between the third and the fourth step: a fresh context takes the state over
                # (the state is taken behind an update: one with lr = 0 and no momentum, which leaves W and the zero histories as they are)
                eng.apply_update(vv.StepConfig(B, C, Nn, lr=0.0, momentum=0.0, weight_decay=0.0))
                state, blob = eng.params_get(), eng.run_state()
                assert np.array_equal(state[0], world(D, N_ROWS)[1]) and not state[2].any()
                eng.close()
                eng = make_engine(vv, world, path, D)
                eng.params_set(*state)
                eng.set_run_state(blob)
            eng.forward_backward(cfg, idx)
            dW, db = eng.grads()                          # (the reduction runs: the step writes its report)
            assert np.isfinite(dW).all()
            reps, sg = eng.grad_scale_stats()
            rec = (int(eng.get_option("last_grad_repeat")), int(eng.get_option("last_grad_shift")))
            o = dict(form=int(eng.get_option("last_score_form")), h16=int(eng.get_option("last_h16")), loss=eng.loss(), prec="f16", B=B, C=C, Nn=Nn,
                     D=D, idx=idx, n_rows=N_ROWS, kw=dict(loss_weight=2.0 ** k), **eng.blobs(cfg, ip1_diff=True))
            r64, r32, kw = refs(o)                        # (from this step's own ip2)
            check_forward(o, r64, r32, kw, "f %s k %d step %d" % (path, k, i + 1))
            if want is None:
                want = steering_run(r64["dY"], B * Nn, path, steps, seg_map=r64["groups"]["map"] if path == "sum" else None)
                ok, worst = margin_ok(want[-1]["all_decisions"])
                assert ok, "f %s k %d: %s lies at %.6f of its threshold: move the seed or k" % (path, k, worst[0], worst[1])
            w = want[i]
            seen.append((reps, sg, rec))
            assert (reps, sg, rec) == (w["repeats"], w["sg"], (w["repeat"], w["shift"])), \
                "step %d: (repeats, scale, (repeat, shift)) %r, reference %r; so far %r" % (i + 1, (reps, sg, rec), (w["repeats"], w["sg"], (w["repeat"], w["shift"])), seen)
            S = sg * 2.0 ** -rec[1]
            tag = "f %s k %d step %d" % (path, k, i + 1)
            check_rows(instance_order(o["ip1_diff"], B), r64["dY"], r32["dY"], S, "f16", tag, "ip1_diff", None, CN)
            if path == "sum":
                gr = eng.dedup_groups(dyu=True)
                assert gr["scale"] == S
                check_rows(gr["dyu"][:r64["groups"]["U"]], r64["dyu"], r32["dyu"], S, "f16", tag, "dyu", r64["groups"], CN, rows_extra(r64, np.float64(S)))
    finally:
        eng.close()
    print("GG f %s k %d roundtrip %d: (repeats, scale, (repeat, shift)) per step %r" % (path, k, roundtrip, seen))
    # what the fixed lag of 4 means, spelled out
    sgs = [s[1] for s in seen]
    assert sgs[:4] == [512.0] * 4 and sgs[4] != 512.0 and len(set(sgs[4:])) == 1
    assert [s[0] for s in seen] == ([0, 0, 0, 0, 1, 2, 3, 4, 4, 4, 4, 4] if k > 0 else [0] * 12)
    assert [s[2][0] for s in seen] == ([1] * 4 + [0] * 8 if k > 0 else [0] * 12)
    # (the reported maximum itself is not readable from the device: this is the REFERENCE's, which the device's scale, repeat and shift were
    # compared with by == above and under which every row passed rule (a) -- a device maximum elsewhere would have moved one of those)
    for w in want[4:]:
        assert 2.0 ** 9 <= w["gmax"] * w["sg"] < 2.0 ** 10
