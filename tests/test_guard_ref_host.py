"""tests/guard_ref.py against hand-computed answers (no GPU): maxima -> shifts in both forms, the steering sequence, both clamps, reports
that carry the repeat bit; and a changed rule (shift e - 11, lag 3, sums of unclipped rows) changes the answer on the same inputs, so the
GPU tests that compare the engine with this reference would see each of them."""
import numpy as np

from tests.guard_ref import LIMIT, Steering, exponent, f16_stored, guard_rounds, margin_ok, steering_run


def test_stored_rows_round_and_saturate():
    x = np.array([0.0, 1.0, 2049.0, 65504.0, 65519.0, 70000.0, -1e9, 2.0 ** -25, 3 * 2.0 ** -25])
    assert np.array_equal(f16_stored(x), [0.0, 1.0, 2048.0, 65504.0, 65504.0, 65504.0, -65504.0, 0.0, 2.0 ** -23])
    assert exponent(32768.0) == 16 and exponent(32767.0) == 15 and exponent(0.75) == 0


def test_one_round_by_hand():
    # 100 x 512 = 51200 = 0.78125 x 2^16 > 32768: shift 16 - 12 = 4, the maximum comes to 3200 in [2^11, 2^12)
    g = guard_rounds([[3.0, -100.0]], 512.0, "dense")
    assert (g["repeat"], g["shift"], g["shift_round1"], g["scale"], g["gmax"]) == (1, 4, 4, 32.0, 100.0)
    assert g["rounds"] == [dict(active=True, shift=4, rows_max=51200.0, sums_max=0.0)]
    assert margin_ok(g["decisions"])[0]
    # 60 x 512 = 30720: idle
    g = guard_rounds([[3.0, -60.0]], 512.0, "dense")
    assert (g["repeat"], g["shift"], g["scale"]) == (0, 0, 512.0) and not g["rounds"][0]["active"]
    # the same rows as segments of one slot: 51200 + 1536 in the sums ... no: column-wise, the sums are the rows' own columns added
    g = guard_rounds([[3.0, -100.0], [4.0, -100.0]], 512.0, "sum", seg_map=[0, 0])
    assert g["rounds"][0] == dict(active=True, shift=5, rows_max=51200.0, sums_max=102400.0)      # 102400 = 0.78125 x 2^17
    assert g["rounds"][1] == dict(active=False, shift=5, rows_max=1600.0, sums_max=3200.0) and g["shift"] == 5 and g["gmax"] == 200.0


def test_margin_condition():
    assert not margin_ok([("x", LIMIT * (1 + 2.0 ** -11), LIMIT)])[0] and not margin_ok([("x", LIMIT * (1 - 2.0 ** -11), LIMIT)])[0]
    ok, worst = margin_ok([("far", 3.0, 2.0), ("near", LIMIT * (1 + 2.0 ** -10), LIMIT)])
    assert ok and worst == ("near", 1 + 2.0 ** -10)
    # a maximum just past a power of two: its shift would hang on the last bits of an fp32 maximum
    g = guard_rounds([[(2.0 ** 17) * (1 + 2.0 ** -12) / 512]], 512.0, "dense")
    assert g["shift"] == 6 and not margin_ok(g["decisions"])[0]


def clipped_case(**kw):
    """40 instances of one slot, every row 2560 in its one column, sg 512: a row is 1310720 scaled, stored as 65504.
    Round 0: rows 1310720, sums of the rows as stored 40 x 65504 = 2620160 = 0.6247 x 2^22 -> shift 10 (the true sum is 52428800 = 0.78 x 2^26)
    Round 1: rows 1280 (unclipped), sums 51200 = 0.78125 x 2^16 > 32768 -> 4 more: shift 14, the sums come to 3200"""
    return guard_rounds(np.full((40, 1), 2560.0), 512.0, "sum", seg_map=np.zeros(40, int), **kw)


def test_two_rounds_sums_of_clipped_rows_under_report():
    g = clipped_case()
    assert g["rounds"][0] == dict(active=True, shift=10, rows_max=1310720.0, sums_max=2620160.0)
    assert g["rounds"][1] == dict(active=True, shift=14, rows_max=1280.0, sums_max=51200.0)
    assert (g["shift"], g["shift_round1"], g["repeat"], g["scale"]) == (14, 10, 1, 2.0 ** -5) and margin_ok(g["decisions"])[0]
    assert g["gmax"] == 2620160.0 / 512          # what the step reports: the round-0 maximum, clipped sums and all


def test_a_changed_rule_changes_the_answer():
    # shift e - 11
    assert guard_rounds([[3.0, -100.0]], 512.0, "dense", place=11)["shift"] == 5 != guard_rounds([[3.0, -100.0]], 512.0, "dense")["shift"]
    m = clipped_case(place=11)                                # (round 1's true sums come to 25600: round 2 stays idle)
    assert (m["shift_round1"], m["shift"]) == (11, 11) and not m["rounds"][1]["active"]
    # sums taken from unclipped rows: round 1 takes everything, round 2 never runs
    m = clipped_case(clip=False)
    assert m["rounds"][0]["sums_max"] == 52428800.0 and m["shift_round1"] == 14 and not m["rounds"][1]["active"]
    assert m["shift_round1"] != clipped_case()["shift_round1"]
    # lag 3: the scale moves one step early
    a = [s["sg"] for s in steering_run([[768.0]], 480, "dense", 8)]
    b = [s["sg"] for s in steering_run([[768.0]], 480, "dense", 8, lag=3)]
    assert a == [512.0] * 4 + [1.0] * 4 and b == [512.0] * 3 + [1.0] * 5


def test_steering_too_large():
    """count 480 = 0.94 x 2^9: sg 512.  gmax 768 = 0.75 x 2^10: ex = 10 + 9 = 19 > 13 -> sg_adj = -9 at the fifth step: 768 in [2^9, 2^10)"""
    run = steering_run([[768.0]], 480, "dense", 12)
    assert [s["sg"] for s in run] == [512.0] * 4 + [1.0] * 8
    assert [s["repeat"] for s in run] == [1] * 4 + [0] * 8 and [s["shift"] for s in run] == [7] * 4 + [0] * 8     # 393216 = 0.75 x 2^19
    assert [s["repeats"] for s in run] == [0, 0, 0, 0, 1, 2, 3, 4, 4, 4, 4, 4]
    assert all(2 ** 9 <= s["gmax"] * s["sg"] < 2 ** 10 for s in run[4:]) and margin_ok(run[-1]["all_decisions"])[0]


def test_steering_too_small():
    """gmax 1.5 x 2^-20 = 0.75 x 2^-19: ex = -19 + 9 = -10 < 5 -> sg_adj = 20"""
    run = steering_run([[1.5 * 2.0 ** -20]], 480, "dense", 12)
    assert [s["sg"] for s in run] == [512.0] * 4 + [2.0 ** 29] * 8
    assert [s["repeats"] for s in run] == [0] * 12 and not any(s["repeat"] for s in run)
    assert all(s["gmax"] * s["sg"] == 768.0 for s in run[4:])


def test_steering_window_edges():
    """ex in 5 .. 13 stays: the scaled maximum in [2^4, 2^13)"""
    for g, moves in ((2.0 ** 4, False), (2.0 ** 4 * 0.99, True), (2.0 ** 13 * 0.99, False), (2.0 ** 13, True)):
        st = Steering(480)
        for seq in range(1, 6):
            st.begin(seq)
            st.report(seq, g / 512, 0)
        assert (st.sg_adj != 0) == moves, (g, st.sg_adj)


def test_both_clamps():
    st = Steering(480)
    for seq in range(1, 9):
        sg = st.begin(seq)
        st.report(seq, 1.5 * 2.0 ** -120, 0)
    assert st.sg_adj == 91 and sg == 2.0 ** 100              # -110 asks for +120, then +29 more: held at 100 - 9 each time
    st = Steering(480)
    for seq in range(1, 9):
        sg = st.begin(seq)
        st.report(seq, 1.5 * 2.0 ** 120, 1)
    assert st.sg_adj == -109 and sg == 2.0 ** -100 and st.repeats == 4


def test_reports_with_the_repeat_bit_and_missing_reports():
    st = Steering(480)
    bits = {1: 1, 2: 0, 3: 1, 5: 1}                           # step 4 never reported (its reduction did not run)
    seen = []
    for seq in range(1, 11):
        st.begin(seq)
        if seq in bits:
            st.report(seq, 100.0 / 512, bits[seq])
        seen.append(st.repeats)
    assert seen == [0, 0, 0, 0, 1, 1, 2, 2, 3, 3] and st.sg_adj == 0
    # a later first step: nothing moves before seq0 + 4
    st = Steering(480)
    for seq in range(7, 12):
        sg = st.begin(seq)
        st.report(seq, 768.0, 1)
        assert (sg == 512.0) == (seq < 11)
