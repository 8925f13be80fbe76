"""Host tests of the exact input family (tests/linear_exact.py): for exactly the cases, seeds, steps and hyper-parameters
tests/test_gpu_linear_step_exact.py runs, the float64 run of tests/hinge_ref.py stays inside fp32 -- every logit, margin, dz, dW, db, every
intermediate of the rule and every state array after every step is an fp32 value, and every sum meets the any-order condition (the sum of
absolute values over the terms' granularity below 2^24; the loss's double sum below 2^53) -- and the float32 twin of hinge_ref gives the same
bits.  A case that fails is a wrong INPUT: change the input in linear_exact.py; nothing here is ever loosened or skipped.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hinge_ref as hr   # noqa: E402
import linear_exact as le   # noqa: E402

F32 = np.float32


def test_granularity_and_width_on_hand_worked_values():
    assert le.granularity([0.75, 2.0, 0.0, -5.0]) == 0.25 and le.granularity([0.0, 0.0]) is None and le.granularity([3 * 2.0 ** -40]) == 2.0 ** -40
    assert le.is_f32([1.0 + 2.0 ** -23, -2.0 ** -149, 0.0]) and not le.is_f32([1.0 + 2.0 ** -24]) and not le.is_f32([np.inf]) and not le.is_f32([1e300])
    assert le.width(np.array([3.0, 2.0 ** 20]), 2.0 ** -3) == 23.0 and le.width(np.zeros(3), None) == -np.inf
    # 2^24 + 1 is the first integer fp32 cannot hold: a sum whose width reaches 24 can round
    assert F32(2.0 ** 24) + F32(1) == F32(2.0 ** 24) and F32(2.0 ** 24 - 1) + F32(1) == F32(2.0 ** 24)


def test_the_check_refuses_inputs_that_leave_fp32():
    """The condition is not vacuous: the same case on rows of 20 more bits, five steps under the decay, or a scale that is no power of two fails it."""
    c = {k.name: k for k in le.FIT_CASES}["dim33"]
    assert le.run(c, check=True)[1] == []
    assert le.run(c._replace(steps=5), check=True)[1] != []
    X = le.inputs(c)[0].astype(np.float64) * (1.0 + 2.0 ** -20)
    st = le.start_state(c)
    assert le.check_step(st, X[:128], le.inputs(c)[1][:128], c.norm, 2.0, le.weight_decay(c.dim))[0] != []
    assert le.check_step(st, le.inputs(c)[0][:128], le.inputs(c)[1][:128], c.norm, 1.9, le.weight_decay(c.dim))[0] != []       # scale 1.9 / 128


@pytest.mark.parametrize("case", le.FIT_CASES + le.GRAD_CASES, ids=le.ids(le.FIT_CASES) + ["grad_" + s for s in le.ids(le.GRAD_CASES)])
def test_every_step_of_every_case_stays_in_fp32(case):
    steps, bad, top = le.run(case, check=True)
    print("EXACT %s: %d steps, widest sum or array 2^%.1f" % (case.name, len(steps), top))
    assert bad == []
    assert len(steps) == case.steps and all(s.count >= 1 for s in steps)
    # the float32 twin, rounding where the device rounds, gives the same bits: nothing rounded
    twin = le.run(case, np.float32)[0]
    for s64, s32 in zip(steps, twin):
        for name in ("dW", "db", "W", "b", "hW", "hb"):
            a32 = getattr(s32, name)
            assert a32.dtype == F32 and np.array_equal(a32.astype(np.float64), getattr(s64, name)), name
        assert s32.loss.dtype == F32 and F32(s64.loss) == s32.loss and s64.correct == s32.correct
    # the reference the GPU test reads is this run
    assert all(np.array_equal(a.W, b.W) and a.loss == b.loss for a, b in zip(le.reference(case), steps))


@pytest.mark.parametrize("case", le.FIT_CASES + le.GRAD_CASES, ids=le.ids(le.FIT_CASES) + ["grad_" + s for s in le.ids(le.GRAD_CASES)])
def test_the_hand_worked_plans_are_the_plans(case):
    Cp, Dp = le.padded(case)
    last = le.batches(case)[-1]
    assert le.batch_plan(last[1], Cp, Dp, case.split_rows) == case.plan
    assert case.n % 256 != 0 and last[0] + last[1] <= case.n and (not case.first or case.first + case.batch < case.n)


def test_the_cases_reach_what_they_name():
    fit = {c.name: c for c in le.FIT_CASES}
    assert sorted({le.padded(c)[1] for c in le.FIT_CASES if c.name.startswith("dim")}) == [32, 64, 160]
    assert sorted({hr.lanes_of(c.C) for c in le.FIT_CASES}) == [1, 2, 4, 8, 16, 32, 64]
    assert le.padded(fit["C257"])[0] == 288 > 256                                    # the bias loop of k_lin_update strides
    assert [n for _, n, _ in le.batches(fit["one_call_256_128_256"])] == [256, 128, 256]
    assert [n for _, n, _ in le.batches(fit["ragged_129"])] == [128, 1, 128] and [n for _, n, _ in le.batches(fit["ragged_700"])] == [256, 256, 188]
    Cp, Dp = le.padded(fit["update_grid_plus"])
    assert Cp * Dp > le.UPD_GRID_FLOATS
    assert all(c.n * c.C > le.SCORES_GRID for c in le.SCORE_CASES if c.name.endswith("grid_plus"))
    # momentum and decay both act in every fit: the put state has nonzero W, b and histories
    for c in le.FIT_CASES:
        _, _, W, b, hW, hb = le.inputs(c)
        assert W.any() and hW.any() and (not c.bias or (b.any() and hb.any())) and (c.bias or not (b.any() or hb.any()))
    assert all(c.steps >= 1 for c in le.FIT_CASES if c.norm == hr.L2) and any(c.steps == 3 for c in le.FIT_CASES if c.norm == hr.L1)
    assert all(c.first > 0 for c in le.GRAD_CASES)


@pytest.mark.parametrize("case", le.SCORE_CASES, ids=le.ids(le.SCORE_CASES))
def test_the_scores_are_exact(case):
    z, bad = le.scores_reference(case)
    assert bad == [] and z.shape == (case.n, case.C) and case.n % 256 != 0
    X, _, W, b = le.inputs(case)[:4]
    assert np.array_equal((X @ W.T + b).astype(np.float64), z)                       # the fp32 product, in BLAS's order
