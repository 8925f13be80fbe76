"""GPU tests of vv_classification_stats (Engine.classification_stats) against tests/classification_ref.py.

count, accuracy and total_accuracy are integers behind one fp32 division: compared with ==.  ap[c] is a double sum of count_c terms
(its own error <= count_c 2^-53 relative) rounded once to fp32: within 1 ulp (fp32) of np.float32(reference).  Two calls, host and
device scores, one column block and many, one counting launch and many must all return identical bits.

Shapes: n = 1, 63, 64, 65, 255, 256, 257 (around one wave and one 256-positive tile), C = 1, 2, 3, 64, 65 (around the 64 lanes of
the row pass), and n = 9001 -- three 4096-item segments of the counting pass -- with "cls_pass_tiles" = 3, which makes the
counting pass of every block several launches ("last_cls_passes", "last_cls_segments" are asserted).  Across them: a class with a
single positive, a class holding every row, an absent class, a column all below zero (ap == 0 with count > 0), scores drawn from
{-1, -0.0, 0.0, 0.5, 1} so that ties dominate, +-Inf, labels in random order."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classification_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

VV_ERR_ARG = 1
_cache = {}


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def case(n, Cn, kind):
    key = (n, Cn, kind)
    if key not in _cache:
        rng = np.random.default_rng(7919 * n + 31 * Cn + len(kind))
        scores, labels = ref.make_case(rng, n, Cn, kind)
        _cache[key] = (scores, labels, ref.classification_stats(scores, labels, Cn))
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(got, want):
    acc, ap, cnt, rep = got
    assert np.array_equal(cnt, want["count"])
    assert np.array_equal(acc, want["accuracy"]) and rep["total_accuracy"] == want["total_accuracy"]
    ulps = ref.ulp_diff32(ap, want["ap64"].astype(np.float32))
    print("ap: max ulp distance", ulps.max(), "mean_ap", rep["mean_ap"], "reference", want["mean_ap64"])
    assert (ulps <= 1).all(), (ap, want["ap64"])
    assert ref.ulp_diff32([rep["mean_ap"]], [np.float32(want["mean_ap64"])])[0] <= 1
    assert rep["classes_present"] == want["classes_present"] and rep["n"] == int(want["count"].sum())


def same_bits(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
            and bits([a[3]["total_accuracy"], a[3]["mean_ap"]]).tolist() == bits([b[3]["total_accuracy"], b[3]["mean_ap"]]).tolist())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("kind", ["ties", "structured"])
def test_rows_around_a_wave_and_a_tile(eng, n, kind):
    scores, labels, want = case(n, 3, kind)
    got = eng.classification_stats(scores, labels, 3)
    check(got, want)
    assert same_bits(got, eng.classification_stats(scores, labels, 3))                     # a second call: identical bits
    assert eng.get_option("last_cls_blocks") == 1 and eng.get_option("last_cls_segments") == 1


@pytest.mark.parametrize("Cn", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("kind", ["random", "ties", "inf", "one_class"])
def test_columns_around_the_row_pass_width(eng, Cn, kind):
    scores, labels, want = case(300, Cn, kind)
    check(eng.classification_stats(scores, labels, Cn), want)


def test_structured_case_has_what_it_promises(eng):
    scores, labels, want = case(257, 5, "structured")
    assert want["count"][4] == 0 and want["count"][1] == 1 and want["count"][0] > 0 and want["ap64"][0] == 0.0
    acc, ap, cnt, rep = eng.classification_stats(scores, labels, 5)
    check((acc, ap, cnt, rep), want)
    assert ap[0] == 0.0 and cnt[0] > 0 and ap[4] == 0.0 and acc[4] == 0.0 and rep["classes_present"] == 4


@pytest.mark.parametrize("kind", ["ties", "random"])
def test_several_segments_and_several_counting_launches(eng, kind):
    n, Cn = 9001, 4
    scores, labels, want = case(n, Cn, kind)
    whole = eng.classification_stats(scores, labels, Cn)
    check(whole, want)
    assert eng.get_option("last_cls_segments") == 3 and eng.get_option("last_cls_passes") == 1
    eng.set_option("cls_pass_tiles", 3)
    try:
        split = eng.classification_stats(scores, labels, Cn)
        assert eng.get_option("last_cls_passes") > 1 and eng.get_option("last_cls_segments") == 3
    finally:
        eng.set_option("cls_pass_tiles", 16384)
    assert same_bits(whole, split)


@pytest.mark.parametrize("Cn,kind", [(65, "ties"), (7, "inf")])
def test_host_scores_device_scores_and_column_blocks_agree(eng, Cn, kind):
    scores, labels, want = case(1000, Cn, kind)
    host = eng.classification_stats(scores, labels, Cn)
    check(host, want)
    assert eng.get_option("last_cls_blocks") == 1
    buf = eng.dev(scores)
    try:
        dev = eng.classification_stats(buf, labels, Cn)
        eng.set_option("cls_block_cols", 3)                       # a host matrix larger than one column block, and a device one
        try:
            host_blocks = eng.classification_stats(scores, labels, Cn)
            assert eng.get_option("last_cls_blocks") == (Cn + 2) // 3
            dev_blocks = eng.classification_stats(buf, labels, Cn)
        finally:
            eng.set_option("cls_block_cols", 0)
    finally:
        buf.free()
    assert same_bits(host, dev) and same_bits(host, host_blocks) and same_bits(host, dev_blocks)


def test_every_argument_error(eng):
    scores, labels, _ = case(64, 3, "random")
    bad = scores.copy()
    bad[5, 1] = np.nan
    bad[9, 2] = np.nan
    with pytest.raises(vv.VVError) as e:
        eng.classification_stats(bad, labels, 3)
    assert e.value.code == VV_ERR_ARG and "2 NaN" in str(e.value)
    for wrong in (-1, 3):
        lab = labels.copy()
        lab[7] = wrong
        with pytest.raises(vv.VVError) as e:
            eng.classification_stats(scores, lab, 3)
        assert e.value.code == VV_ERR_ARG
    with pytest.raises(vv.VVError) as e:
        eng.classification_stats(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), 3)
    assert e.value.code == VV_ERR_ARG
    with pytest.raises(vv.VVError) as e:
        eng.classification_stats(np.zeros((4, 0), np.float32), np.zeros(4, np.int32), 0)
    assert e.value.code == VV_ERR_ARG
    with pytest.raises(vv.VVError) as e:
        eng.set_option("last_cls_passes", 1)
    assert e.value.code == VV_ERR_ARG
    check(eng.classification_stats(scores, labels, 3), case(64, 3, "random")[2])          # the context is fine afterwards
