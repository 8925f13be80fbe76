"""GPU tests of the nearest-neighbour lists (vv_gallery_nearest, vv_gallery_nearest_self, Gallery.nearest / nearest_self) against
tests/nearest_ref.py.

Exact inputs: integer features in [-3, 3], dim 40 (padded to 64 on the device).  Every dot product is an integer of magnitude
<= 360, so every fp32 distance is exact in any summation order and the lists are compared with np.array_equal on the indices
and on the BITS of the distances: no near-tie exemption anywhere.  Such inputs have at most 1441 distinct distances, so every
threshold bin of the selection form is full of ties.  Every test asserts the form it ran ("last_nearest_form": 1 streaming,
2 selection)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gallery_ref   # noqa: E402
import nearest_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

STREAMING, SELECTION = 1, 2
_cache = {}


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


@pytest.fixture
def select_always(eng):
    eng.set_option("nearest_select_min_k", 1)
    yield
    eng.set_option("nearest_select_min_k", 33)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def host_case():
    """Cases 1, 2, 7: 64 queries against 50 001 items (four segments of the row kernels, not a multiple of 4), 50 ids."""
    if "host" not in _cache:
        Q, qid, G, gid = ref.exact_input(64, 50001, 50, 21)
        d = ref.distances32(Q, G)
        _cache["host"] = dict(Q=Q, qid=qid, G=G, gid=gid, d=d, all=ref.nearest(d, None, 2048))
    return _cache["host"]


def self_case():
    """Cases 5, 7: 3000 items (several query blocks), 60 ids."""
    if "self" not in _cache:
        _, _, G, gid = ref.exact_input(1, 3000, 60, 23)
        d = ref.distances32(G, G)
        _cache["self"] = dict(G=G, gid=gid, d=d, other=~np.eye(3000, dtype=bool))
    return _cache["self"]


def strictly_ascending(idx, dist):
    d0, d1, i0, i1 = dist[:, :-1], dist[:, 1:], idx[:, :-1], idx[:, 1:]
    return bool(((d0 < d1) | ((d0 == d1) & (i0 < i1))).all())


@pytest.mark.parametrize("k", [33, 100, 2047, 2048])
def test_multi_segment_host_queries(eng, k):
    c = host_case()
    g = eng.gallery(c["G"])
    try:
        a = g.nearest(c["Q"], k)
        assert g.get("last_nearest_form") == SELECTION
        b = g.nearest(c["Q"], k)
        assert g.get("last_nearest_form") == SELECTION
        assert 0 < g.scratch_bytes <= g.get("scratch_limit_bytes")
        assert g.get("last_device_ms") >= g.get("last_sim_ms") > 0
    finally:
        g.close()
    want = (c["all"][0][:, :k], c["all"][1][:, :k])
    assert same(a, want), (np.argwhere(a[0] != want[0])[:5], np.argwhere(bits(a[1]) != bits(want[1]))[:5])
    assert same(a, b)


def test_exclusion_by_id(eng):
    c = host_case()
    g = eng.gallery(c["G"], c["gid"])
    try:
        got = g.nearest(c["Q"], 64, c["qid"])
        assert g.get("last_nearest_form") == SELECTION
    finally:
        g.close()
    assert same(got, ref.nearest(c["d"], c["gid"][None, :] != c["qid"][:, None], 64))
    assert (c["gid"][got[0]] != c["qid"][:, None]).all()
    # one more id owns all but 10 items: a query carrying it has 10 eligible items
    gid2 = ref.one_id_owns_all_but(c["gid"], 50, 10, 22)
    qid2 = c["qid"].copy()
    qid2[[0, 17, 63]] = 50
    g = eng.gallery(c["G"], gid2)
    try:
        got = g.nearest(c["Q"], 64, qid2)
        assert g.get("last_nearest_form") == SELECTION
    finally:
        g.close()
    assert same(got, ref.nearest(c["d"], gid2[None, :] != qid2[:, None], 64))
    for i in (0, 17, 63):
        assert (got[0][i, :10] >= 0).all() and (got[0][i, 10:] == -1).all() and (bits(got[1])[i, 10:] == 0).all()
        assert sorted(got[0][i, :10]) == sorted(np.flatnonzero(gid2 != 50))


@pytest.mark.parametrize("ng,k,form", [(40, 64, SELECTION), (1, 1, STREAMING), (1, 33, SELECTION)])
def test_tiny_galleries(eng, ng, k, form):
    Q, _, G, _ = ref.exact_input(5, ng, 3, 24)
    g = eng.gallery(G)
    try:
        got = g.nearest(Q, k)
        assert g.get("last_nearest_form") == form
    finally:
        g.close()
    assert same(got, ref.nearest(ref.distances32(Q, G), None, k))
    assert (got[0][:, min(ng, k):] == -1).all() and (got[0][:, :min(ng, k)] >= 0).all()


def test_all_tie_rows(eng):
    """20 000 identical rows: every distance of a query is the same float, the threshold bin holds the whole row, and the k
    items of lowest index are taken.  An all-zero query: every distance is +0 (the -0 fold)."""
    rng = np.random.default_rng(25)
    row = rng.integers(-3, 4, 40).astype(np.float32)
    G = np.tile(row, (20000, 1))
    Q = rng.integers(-3, 4, (7, 40)).astype(np.float32)
    Q[3] = 0
    Q[5] = -row                                                      # the largest distance there is; Q[3] @ row = +-0
    g = eng.gallery(G)
    try:
        idx, dist = g.nearest(Q, 100)
        assert g.get("last_nearest_form") == SELECTION
        idx2, dist2 = g.nearest(Q, 2048)
    finally:
        g.close()
    assert np.array_equal(idx, np.tile(np.arange(100, dtype=np.int32), (7, 1)))
    assert np.array_equal(idx2, np.tile(np.arange(2048, dtype=np.int32), (7, 1)))
    want = ref.distances32(Q, G[:1])                                 # [7][1]
    assert np.array_equal(bits(dist), np.tile(bits(want), (1, 100)))
    assert (bits(dist)[3] == 0).all() and (bits(dist2)[3] == 0).all()
    # rows that differ only in their last items: the ties are cut at the same place in every segment
    G[19990:] = -row
    Qz = np.zeros((2, 40), np.float32)
    g = eng.gallery(G)
    try:
        idx, dist = g.nearest(Qz, 64)
        assert g.get("last_nearest_form") == SELECTION
    finally:
        g.close()
    assert np.array_equal(idx, np.tile(np.arange(64, dtype=np.int32), (2, 1))) and (bits(dist) == 0).all()


@pytest.mark.parametrize("exclude", [False, True])
def test_self_form(eng, exclude):
    c = self_case()
    el = c["other"] & (c["gid"][None, :] != c["gid"][:, None]) if exclude else c["other"]
    g = eng.gallery(c["G"], c["gid"])
    try:
        assert g.get("query_block") < 3000
        a = g.nearest_self(64, exclude)
        assert g.get("last_nearest_form") == SELECTION
        b = g.nearest_self(64, exclude)
        assert 0 < g.scratch_bytes <= g.get("scratch_limit_bytes")
    finally:
        g.close()
    assert same(a, ref.nearest(c["d"], el, 64))
    assert same(a, b)
    assert (a[0] != np.arange(3000)[:, None]).all()
    if exclude:
        assert (c["gid"][a[0]] != c["gid"][:, None]).all()


def test_self_form_without_ids_and_single_item(eng):
    c = self_case()
    g = eng.gallery(c["G"][:700])
    try:
        got = g.nearest_self(40)
        assert g.get("last_nearest_form") == SELECTION
    finally:
        g.close()
    assert same(got, ref.nearest(c["d"][:700, :700], c["other"][:700, :700], 40))
    g = eng.gallery(c["G"][:1])
    try:
        for k, form in ((1, STREAMING), (33, SELECTION)):
            idx, dist = g.nearest_self(k)
            assert g.get("last_nearest_form") == form
            assert (idx == -1).all() and (bits(dist) == 0).all()
    finally:
        g.close()


def input_b():
    if "B" not in _cache:
        Q, qid, G, gid = gallery_ref.make_input(nq=193, ng=50001, D=96, nid=700, noise=1.8, seed=6)
        _cache["B"] = (Q, G)
    return _cache["B"]


def test_selection_equals_streaming_on_real_valued_input(eng, select_always):
    """Both forms read the same stored floats, so they agree bit for bit whatever the fp32 summation order."""
    Q, G = input_b()
    g = eng.gallery(G)
    try:
        for k in (1, 5, 32):
            want = g.topk(Q, k)
            got = g.nearest(Q, k)
            assert g.get("last_nearest_form") == SELECTION
            assert same(got, want), k
            assert k == 1 or strictly_ascending(*got)
        far = g.nearest(Q, 2048)
        assert g.get("last_nearest_form") == SELECTION
        assert same((far[0][:, :32], far[1][:, :32]), want)
        assert strictly_ascending(*far) and (far[0] >= 0).all()
        assert all(len(set(r)) == 2048 for r in far[0].tolist())
    finally:
        g.close()


def test_streaming_equals_topk_under_the_default_option(eng):
    Q, G = input_b()
    assert eng.get_option("nearest_select_min_k") == 33
    g = eng.gallery(G)
    try:
        want = g.topk(Q, 32)
        got = g.nearest(Q, 32)
        assert g.get("last_nearest_form") == STREAMING
        far = g.nearest(Q, 2048)
        assert g.get("last_nearest_form") == SELECTION
    finally:
        g.close()
    assert same(got, want) and strictly_ascending(*got)
    assert same((far[0][:, :32], far[1][:, :32]), want)


def test_streaming_form_with_the_new_predicates(eng):
    c = host_case()
    g = eng.gallery(c["G"], c["gid"])
    try:
        got = g.nearest(c["Q"], 10, c["qid"])
        assert g.get("last_nearest_form") == STREAMING
    finally:
        g.close()
    assert same(got, ref.nearest(c["d"], c["gid"][None, :] != c["qid"][:, None], 10))
    gid2 = ref.one_id_owns_all_but(c["gid"], 50, 10, 22)
    qid2 = c["qid"].copy()
    qid2[[0, 17, 63]] = 50
    g = eng.gallery(c["G"], gid2)
    try:
        got = g.nearest(c["Q"], 12, qid2)
        assert g.get("last_nearest_form") == STREAMING
    finally:
        g.close()
    assert same(got, ref.nearest(c["d"], gid2[None, :] != qid2[:, None], 12))
    assert (got[0][0, 10:] == -1).all()
    s = self_case()
    g = eng.gallery(s["G"], s["gid"])
    try:
        a = g.nearest_self(10, True)
        assert g.get("last_nearest_form") == STREAMING
        b = g.nearest_self(10, False)
        assert g.get("last_nearest_form") == STREAMING
    finally:
        g.close()
    assert same(a, ref.nearest(s["d"], s["other"] & (s["gid"][None, :] != s["gid"][:, None]), 10))
    assert same(b, ref.nearest(s["d"], s["other"], 10))


def test_forms_agree_on_the_exact_inputs(eng, select_always):
    """k = 10 through the selection form equals the streaming form's lists of the test above (both equal the restatement)."""
    c = host_case()
    g = eng.gallery(c["G"], c["gid"])
    try:
        got = g.nearest(c["Q"], 10, c["qid"])
        assert g.get("last_nearest_form") == SELECTION
    finally:
        g.close()
    assert same(got, ref.nearest(c["d"], c["gid"][None, :] != c["qid"][:, None], 10))


def test_argument_errors(eng):
    c = host_case()
    Q, G = c["Q"][:4], c["G"][:100]
    g = eng.gallery(G)
    try:
        for k in (0, 2049):
            with pytest.raises(vv.VVError, match="error 1"):
                g.nearest(Q, k)
            with pytest.raises(vv.VVError, match="error 1"):
                g.nearest_self(k)
        with pytest.raises(vv.VVError, match="error 1"):
            g.nearest(Q, 5, c["qid"][:4])
        with pytest.raises(vv.VVError, match="error 1"):
            g.nearest_self(5, True)
        for v in (0, 34):
            with pytest.raises(vv.VVError, match="error 1"):
                eng.set_option("nearest_select_min_k", v)
        assert eng.get_option("nearest_select_min_k") == 33
        with pytest.raises(vv.VVError, match="error 1"):
            g.topk(Q, 33)
        idx, _ = g.nearest(Q, 5)
        assert g.get("last_nearest_form") == STREAMING and idx.shape == (4, 5)
    finally:
        g.close()
