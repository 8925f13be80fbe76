"""CPU test of the checker that tests/test_gpu_dedup_groups.py holds the grouping kernels to (tests/pyref.py: dedup_groups_expected,
dedup_groups_check): it accepts a valid grouping with any arrival order inside the slots and rejects a corrupted one."""
import numpy as np
import pytest

from tests.pyref import dedup_groups_check, dedup_groups_expected


def valid_grouping(idx, n_rows, seed):
    """The expected arrays plus a random valid `ord` (a shuffled range(cnt[u]) per slot) and the `pos` that follows from it."""
    exp = dedup_groups_expected(idx, n_rows)
    rng = np.random.default_rng(seed)
    got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in exp.items()}
    ordv = np.empty(exp["R"], np.int32)
    for u in range(exp["U"]):
        members = np.flatnonzero(exp["map"] == u)
        ordv[members] = rng.permutation(len(members))
    got["ord"] = ordv
    got["pos"] = (exp["seg_start"][exp["map"]] + ordv).astype(np.int32)
    return exp, got


def test_expected_grouping_of_a_small_batch_by_hand():
    # rows 5 and 2 repeat, -1 and 9 (outside a table of 9 rows) share the zero row's slot; slots in order of first appearance
    exp = dedup_groups_expected(np.array([[5, 2, -1], [2, 9, 5], [7, 5, 0]]), n_rows=9)
    assert (exp["R"], exp["Rp"], exp["U"]) == (9, 256, 5)
    assert exp["rows"][:9].tolist() == [5, 2, 9, 2, 9, 5, 7, 5, 0] and (exp["rows"][9:] == 9).all()
    assert exp["uniq_rows"][:5].tolist() == [5, 2, 9, 7, 0] and (exp["uniq_rows"][5:] == 9).all()
    assert exp["map"].tolist() == [0, 1, 2, 1, 2, 0, 3, 0, 4]
    assert exp["cnt"][:5].tolist() == [3, 2, 2, 1, 1] and (exp["cnt"][5:] == 0).all()
    assert exp["seg_start"].tolist() == [0, 3, 5, 7, 8, 9]


def test_checker_accepts_any_arrival_order_and_rejects_a_cross_slot_swap():
    rng = np.random.default_rng(0)
    idx = rng.integers(-1, 40, size=(41, 25))
    exp, got = valid_grouping(idx, 40, seed=1)
    dedup_groups_check(got, exp)
    # two pos entries swapped across slots: every array is still a permutation / a valid prefix sum on its own
    a = 0
    b = int(np.flatnonzero(exp["map"] != exp["map"][a])[0])
    bad = dict(got, pos=got["pos"].copy())
    bad["pos"][[a, b]] = bad["pos"][[b, a]]
    with pytest.raises(AssertionError, match="pos"):
        dedup_groups_check(bad, exp)
    # the same arrival number twice inside one slot
    members = np.flatnonzero(exp["map"] == exp["map"][a])
    assert len(members) >= 2
    bad = dict(got, ord=got["ord"].copy())
    bad["ord"][members[0]] = bad["ord"][members[1]]
    with pytest.raises(AssertionError, match="ord"):
        dedup_groups_check(bad, exp)
    # slots numbered by row number instead of first appearance
    srt = dedup_groups_expected(np.sort(idx.reshape(-1)).reshape(idx.shape), 40)
    bad = dict(got, uniq_rows=srt["uniq_rows"])
    with pytest.raises(AssertionError, match="uniq_rows"):
        dedup_groups_check(bad, exp)
    # a total one short
    bad = dict(got, seg_start=got["seg_start"].copy())
    bad["seg_start"][-1] -= 1
    with pytest.raises(AssertionError, match="seg_start"):
        dedup_groups_check(bad, exp)
