"""tests/pq_ref.py against cases worked out by hand, without a GPU: the table chain and the ADC chain (one of each where the order of
the sums changes the float), the order of equal distances, and a query with fewer candidates than k."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pq_ref as ref   # noqa: E402

F32 = np.float32
BIG = F32(16777216.0)          # 2^24: BIG + 1 rounds back to BIG in fp32


def test_table_chain_by_hand():
    # M = 2, dsub = 3, ksub = 2.  Sub-space 0 codeword 0: 2^24 + 1 - 2^24 in column order is ((0 + 2^24) + 1) - 2^24 = 0, not 1.
    q = np.array([[1, 1, 1, 2, -3, 0.5]], F32)
    cb = np.array([[[BIG, 1, -BIG], [1, 2, 3]],
                   [[1, 1, 4], [0, 0, 0]]], F32)
    lut = ref.table(q, cb)
    assert lut.shape == (1, 2, 2) and lut.dtype == F32
    # [0][0]: s = 0 -> -2 * 0 + 0 = +0 (never -0); [0][1]: 1 + 2 + 3 = 6 -> -12; [1][0]: 2 - 3 + 2 = 1 -> -2; [1][1]: 0
    assert lut.tolist() == [[[0.0, -12.0], [-2.0, 0.0]]]
    assert not np.signbit(lut[0, 0, 0]) and not np.signbit(lut[0, 1, 1])
    # the other order of the same three products gives 1: the chain's order is part of the result
    assert float((F32(BIG * 1) + F32(-BIG * 1)) + F32(1)) == 1.0
    # every product is rounded before it is added: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11, so subtracting that leaves 0, not 2^-24
    x = F32(1.0 + 2.0 ** -12)
    lut2 = ref.table(np.array([[x, 1]], F32), np.array([[[x, -F32(1.0 + 2.0 ** -11)]]], F32))
    assert lut2.tolist() == [[[0.0]]]


def test_adc_chain_by_hand():
    # M = 3 over ksub = 2: item 0 adds 2^24, 1, -2^24 in that order -> 0; item 1 adds 1, 2, 3 -> 6; item 2 takes the first look-up alone
    lut = np.array([[[BIG, 1], [1, 2], [-BIG, 3]]], F32)
    codes = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0]], np.uint8)
    a = ref.adc(lut, codes)
    assert a.dtype == F32 and a.tolist() == [[0.0, 6.0, 1.0 + 1.0 - 16777216.0]]
    assert ref.adc(lut[:, :1], codes[:, :1]).tolist() == [[16777216.0, 1.0, 1.0]]          # M = 1: the look-up itself
    # ascending m, not descending: the reverse chain of item 0 is (-2^24 + 1) + 2^24 = 1 - in fp32 -2^24 + 1 = -16777215 exactly, so 1
    assert float(F32(F32(-BIG + F32(1)) + BIG)) == 1.0 and a[0, 0] == 0.0


def case():
    # 6 items in 3 lists; dim 2, M = 2, dsub = 1, ksub = 2 with codewords 0 and 1 in both sub-spaces; items 1 and 4 share a code, as do 0 and 5
    cb = np.array([[[0], [1]], [[0], [1]]], F32)
    codes = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [1, 0], [0, 0]], np.uint8)
    assign = np.array([2, 0, 1, 1, 2, 0])
    start, lst = ref.ivf_ref.lists_of(assign, 3)
    return cb, codes, start, lst


def test_equal_distances_order_by_item_index_across_lists():
    cb, codes, start, lst = case()
    assert start.tolist() == [0, 2, 4, 6] and lst.tolist() == [1, 5, 2, 3, 0, 4]
    q = np.array([[3, 1]], F32)
    # a = -2 (3 c0) + -2 (1 c1): items 0, 5 -> 0; 1, 4 -> -6; 2 -> -8; 3 -> -2
    d_cent = np.array([[0.0, 1.0, 2.0]], F32)
    r = ref.search(q, cb, codes, d_cent, None, "spherical", start, lst, 3, 6)
    assert r["idx"].tolist() == [[2, 1, 4, 3, 0, 5]] and r["dist"].tolist() == [[-8.0, -6.0, -6.0, -2.0, 0.0, 0.0]]
    assert r["n_candidates"].tolist() == [6]
    # lists 0 and 2 only (the two smallest keys): item 4 of list 2 ties with item 1 of list 0 and comes second; 0 before 5 likewise
    r = ref.search(q, cb, codes, np.array([[0.0, 9.0, 2.0]], F32), None, "spherical", start, lst, 2, 4)
    assert r["probes"] == [[0, 2]] and r["idx"].tolist() == [[1, 4, 0, 5]] and r["n_candidates"].tolist() == [4]


def test_k_above_the_candidates():
    cb, codes, start, lst = case()
    q = np.array([[3, 1], [0, 0]], F32)
    r = ref.search(q, cb, codes, np.array([[5.0, 1.0, 2.0], [1.0, 5.0, 2.0]], F32), np.zeros(3, F32), "euclidean", start, lst, 1, 4)
    assert r["probes"] == [[1], [0]] and r["n_candidates"].tolist() == [2, 2]
    assert r["idx"].tolist() == [[2, 3, -1, -1], [1, 5, -1, -1]]
    assert r["dist"].tolist() == [[-8.0, -2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
