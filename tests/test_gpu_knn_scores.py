"""GPU tests of the k-NN classifier (vv_gallery_knn_scores, vv_gallery_knn_scores_self, Gallery.knn_scores / knn_scores_self)
against tests/knn_ref.py.

Exact inputs (nearest_ref.exact_input): integer features in [-3, 3], dim 40, so every fp32 distance is exact in any summation order
and ties are plentiful.  UNIFORM scores are (float)V_c / (float)m, one rounding: held to np.array_equal, as are n_used, the two list
forms against each other and the two store forms.  EXP scores are fp32 sums of expf weights: held to the float64 restatement within a
bound counted rounding by rounding (exp_bound), and to bit equality between two calls and between the two list forms."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classification_ref   # noqa: E402
import knn_ref as ref   # noqa: E402
import nearest_ref   # noqa: E402

import videovector_amd as vv   # noqa: E402
from videovector_amd.engine import DevBuf   # noqa: E402

pytestmark = pytest.mark.gpu

STREAMING, SELECTION = 1, 2
VEC, ELEMENTWISE = 1, 2
NQ = 37
SENTINEL = np.float32(-7.5)
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


def host_case(n_ref):
    """37 queries against n_ref items, 12 ids; the restated lists at k = 2048 once (a shorter list is their head)."""
    if n_ref not in _cache:
        Q, qid, G, gid = nearest_ref.exact_input(NQ, n_ref, 12, 41 + n_ref)
        d = nearest_ref.distances32(Q, G)
        _cache[n_ref] = dict(Q=Q, qid=qid, G=G, gid=gid, d=d, lists=nearest_ref.nearest(d, None, 2048))
    return _cache[n_ref]


def self_case():
    """3000 items (several query blocks), 60 ids: the input of test_gpu_nearest.py's self form."""
    if "self" not in _cache:
        _, _, G, gid = nearest_ref.exact_input(1, 3000, 60, 23)
        _cache["self"] = dict(G=G, gid=gid, d=nearest_ref.distances32(G, G), other=~np.eye(3000, dtype=bool))
    return _cache["self"]


def labels_for(n_ref, Cn, seed=5):
    lab = np.random.default_rng(seed + Cn).integers(0, Cn, n_ref).astype(np.int32)
    lab[0], lab[-1] = Cn - 1, 0                                     # the last bin is in use
    return lab


@pytest.mark.parametrize("n_ref", [40, 2500])
@pytest.mark.parametrize("k", [1, 5, 32, 33, 256, 2048])
def test_uniform_exact(eng, n_ref, k):
    c = host_case(n_ref)
    g = eng.gallery(c["G"])
    try:
        for Cn in (1, 2, 3, 20, 257, 4096):
            lab = labels_for(n_ref, Cn)
            want, want_m = ref.knn_scores(c["d"], None, lab, Cn, k, lists=c["lists"])
            assert (want_m == min(k, n_ref)).all()
            buf, m = g.knn_scores(c["Q"], lab, Cn, k, n_used=True)
            assert g.get("last_nearest_form") == (STREAMING if k < 33 else SELECTION)
            assert eng.get_option("last_knn_form") == (VEC if Cn % 4 == 0 else ELEMENTWISE)
            assert g.get("last_device_ms") >= g.get("last_sim_ms") > 0 and g.get("last_knn_vote_ms") > 0
            got = buf.get()
            assert np.array_equal(got, want), (Cn, np.argwhere(got != want)[:5])
            assert np.array_equal(m, want_m)
            eng.set_option("nearest_select_min_k", 1)
            try:
                g.knn_scores(c["Q"], lab, Cn, k, out=buf)
                assert g.get("last_nearest_form") == SELECTION
            finally:
                eng.set_option("nearest_select_min_k", 33)
            assert np.array_equal(bits(buf.get()), bits(got)), Cn
            buf.free()
    finally:
        g.close()


@pytest.mark.parametrize("exclude", [False, True])
def test_self_form_writes_every_blocks_rows(eng, exclude):
    c = self_case()
    el = c["other"] & (c["gid"][None, :] != c["gid"][:, None]) if exclude else c["other"]
    lab = labels_for(3000, 7)
    want, want_m = ref.knn_scores(c["d"], el, lab, 7, 40)
    g = eng.gallery(c["G"], c["gid"])
    try:
        assert g.get("query_block") < 3000
        buf, m = g.knn_scores_self(lab, 7, 40, exclude, n_used=True)
        assert g.get("last_nearest_form") == SELECTION and eng.get_option("last_knn_form") == ELEMENTWISE
        got = buf.get()
        buf.free()
    finally:
        g.close()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(m, want_m) and (m == 40).all()


@pytest.mark.parametrize("k", [12, 64])
def test_q_ids_rows_with_few_or_no_eligible_items(eng, k):
    c = host_case(2500)
    lab = labels_for(2500, 20)
    # id 12 owns all but 10 items: a query carrying it has 10 eligible items and its own denominator
    gid2 = nearest_ref.one_id_owns_all_but(c["gid"], 12, 10, 22)
    qid2 = c["qid"].copy()
    qid2[[0, 17, 36]] = 12
    el = gid2[None, :] != qid2[:, None]
    want, want_m = ref.knn_scores(c["d"], el, lab, 20, k)
    g = eng.gallery(c["G"], gid2)
    try:
        buf, m = g.knn_scores(c["Q"], lab, 20, k, q_ids=qid2, n_used=True)
        assert g.get("last_nearest_form") == (STREAMING if k < 33 else SELECTION)
        got = buf.get()
        buf.free()
    finally:
        g.close()
    assert np.array_equal(got, want) and np.array_equal(m, want_m)
    assert (m[[0, 17, 36]] == 10).all() and (np.delete(m, [0, 17, 36]) == k).all()
    tenths = np.round(got[[0, 17, 36]].astype(np.float64) * 10)
    assert np.array_equal(got[[0, 17, 36]], (tenths.astype(np.float32) / np.float32(10))) and (tenths.sum(axis=1) == 10).all()
    # id 12 owns every item: no eligible item, m = 0, a row of +0.0f
    gid3 = np.full_like(c["gid"], 12)
    g = eng.gallery(c["G"], gid3)
    try:
        buf = DevBuf(eng, np.full((NQ, 20), SENTINEL, np.float32))
        _, m = g.knn_scores(c["Q"], lab, 20, k, q_ids=qid2, out=buf, n_used=True)
        got = buf.get()
        buf.free()
    finally:
        g.close()
    want, want_m = ref.knn_scores(c["d"], gid3[None, :] != qid2[:, None], lab, 20, k, lists=None)
    assert np.array_equal(m, want_m) and (m[[0, 17, 36]] == 0).all()
    assert (bits(got)[[0, 17, 36]] == 0).all() and np.array_equal(got, want)


def test_all_tie_rows_vote_by_the_tie_rule(eng):
    """5000 identical rows: every distance of a query is one float, the list is items 0 .. k - 1, labels = g % C."""
    rng = np.random.default_rng(25)
    row = rng.integers(-3, 4, 40).astype(np.float32)
    G = np.tile(row, (5000, 1))
    Q = rng.integers(-3, 4, (7, 40)).astype(np.float32)
    Q[3] = 0
    lab = (np.arange(5000) % 7).astype(np.int32)
    g = eng.gallery(G)
    try:
        for k, form in ((5, STREAMING), (100, SELECTION), (2048, SELECTION)):
            buf, m = g.knn_scores(Q, lab, 7, k, n_used=True)
            assert g.get("last_nearest_form") == form
            want = np.bincount(np.arange(k) % 7, minlength=7).astype(np.float32) / np.float32(k)
            assert np.array_equal(buf.get(), np.tile(want, (7, 1))) and (m == k).all()
            e = g.knn_scores(Q, lab, 7, k, weighting="exp", temperature=0.5, out=buf).get()       # every weight is expf(0) = 1
            assert np.array_equal(e, np.tile(want, (7, 1)))         # sums of ones are exact integers: the UNIFORM quotient
            buf.free()
    finally:
        g.close()


def test_store_forms_and_sentinels(eng):
    c = host_case(2500)
    g = eng.gallery(c["G"])
    results = {}
    try:
        for name, Cn, off, form in (("vec", 8, 4, VEC), ("shifted", 8, 1, ELEMENTWISE), ("odd", 7, 4, ELEMENTWISE)):
            lab = labels_for(2500, 7, seed=9)                       # the same classes for the three (class 7 of 8 stays empty)
            for w in ("uniform", "exp"):
                hold = DevBuf(eng, np.full(NQ * Cn + 8, SENTINEL, np.float32))
                g.knn_scores(c["Q"], lab, Cn, 64, weighting=w, temperature=8.0, out=hold.ptr.value + 4 * off)
                assert eng.get_option("last_knn_form") == form, name
                a = hold.get()
                hold.free()
                assert (a[:off] == SENTINEL).all() and (a[off + NQ * Cn:] == SENTINEL).all()
                body = a[off:off + NQ * Cn].reshape(NQ, Cn)
                assert (body != SENTINEL).all()
                results[name, w] = body
    finally:
        g.close()
    for w in ("uniform", "exp"):
        assert np.array_equal(bits(results["vec", w]), bits(results["shifted", w]))
        assert np.array_equal(bits(results["vec", w][:, :7]), bits(results["odd", w])) and (bits(results["vec", w][:, 7]) == 0).all()
    want, _ = ref.knn_scores(c["d"], None, labels_for(2500, 7, seed=9), 7, 64, lists=c["lists"])
    assert np.array_equal(results["odd", "uniform"], want)


def exp_bound(idx, arg, lab, Cn):
    """|device score - float64 score| at most this, element by element [n_q][Cn].  u = 2^-24.  Per weight: the difference and the
    quotient are one rounding each, so the argument is off by a factor within (1 + u)^2 and the weight by expm1(|arg| ((1 + u)^2 - 1))
    relative; expf is within 1 ulp of the result (ROCm's documented bound for OCML's expf), at most 2 u relative; a weight below the
    normal range is off by at most 2^-126 absolutely, flushed or not.  Sums: a weight passes through at most (n_c - 1) additions
    inside its class and (classes with a vote - 1) across classes (additions of +0 are exact), together at most m - 1: gamma =
    (m - 1) u / (1 - (m - 1) u) on V_c and on V.  The quotient V_c / V: first-order propagation over V - E, then one rounding."""
    u = 2.0 ** -24
    nq, k = idx.shape
    out = np.zeros((nq, Cn))
    for i in range(nq):
        m = int((idx[i] >= 0).sum())
        if m == 0:
            continue
        a = -arg[i, :m]
        w = np.exp(-a)
        rel = (1 + np.expm1(a * ((1 + u) ** 2 - 1))) * (1 + 2 * u) - 1
        e = w * rel + 2.0 ** -126
        cls = lab[idx[i, :m]]
        Vc, ec = np.bincount(cls, weights=w, minlength=Cn), np.bincount(cls, weights=e, minlength=Cn)
        V = Vc.sum()
        gam = (m - 1) * u / (1 - (m - 1) * u)
        Ec, E = (1 + gam) * ec + gam * Vc, (1 + gam) * e.sum() + gam * V
        p = Vc / V
        prop = (Ec + p * E) / (V - E)
        out[i] = prop + u * (p + prop) + 2.0 ** -126 + 1e-15
    return out


@pytest.mark.parametrize("T", [8.0, 0.5, 1e-3])
@pytest.mark.parametrize("k", [5, 256, 2048])
def test_exp_against_float64(eng, T, k, capsys):
    c = host_case(2500)
    lab = labels_for(2500, 20)
    want, want_m = ref.knn_scores(c["d"], None, lab, 20, k, ref.EXP, T, lists=c["lists"])
    V, arg = ref.exp_sums(c["d"], None, lab, 20, k, T, lists=c["lists"])
    assert (V >= 1).all()                                           # w_0 = 1: the bound's divisor V - E is safe
    bound = exp_bound(c["lists"][0][:, :k], arg, lab, 20)
    g = eng.gallery(c["G"])
    try:
        buf, m = g.knn_scores(c["Q"], lab, 20, k, weighting="exp", temperature=T, n_used=True)
        assert g.get("last_nearest_form") == (STREAMING if k < 33 else SELECTION)
        a = buf.get()
        b = g.knn_scores(c["Q"], lab, 20, k, weighting="exp", temperature=T, out=buf).get()
        eng.set_option("nearest_select_min_k", 1)
        try:
            s = g.knn_scores(c["Q"], lab, 20, k, weighting="exp", temperature=T, out=buf).get()
            assert g.get("last_nearest_form") == SELECTION
        finally:
            eng.set_option("nearest_select_min_k", 33)
        buf.free()
    finally:
        g.close()
    err = np.abs(a.astype(np.float64) - want)
    with capsys.disabled():
        print("\nknn exp T = %g k = %d: largest error %.3g, largest error / bound %.3f, row sums within %.3g of 1"
              % (T, k, err.max(), (err / bound).max(), np.abs(a.astype(np.float64).sum(axis=1) - 1).max()))
    assert np.array_equal(m, want_m)
    assert (err <= bound).all(), (np.argwhere(err > bound)[:5], err.max())
    assert (a >= 0).all() and (a <= 1).all()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(s))


@pytest.mark.parametrize("weighting,T", [("uniform", 0.07), ("exp", 8.0), ("exp", 0.5), ("exp", 1e-3)])
def test_one_class_rows_are_exactly_one(eng, weighting, T):
    c = host_case(2500)
    lab = np.full(2500, 3, np.int32)
    want = np.zeros((NQ, 5), np.float32)
    want[:, 3] = 1
    g = eng.gallery(c["G"])
    try:
        for k in (5, 256, 2048):
            buf = g.knn_scores(c["Q"], lab, 5, k, weighting=weighting, temperature=T)
            assert np.array_equal(bits(buf.get()), bits(want)), k
            buf.free()
    finally:
        g.close()


def test_refusals_leave_the_output_alone(eng):
    c = host_case(40)
    Q, G = c["Q"], c["G"]
    lab = labels_for(40, 5)
    g = eng.gallery(G)
    other = vv.Engine(0, "f16")
    hold = DevBuf(eng, np.full((NQ, 5), SENTINEL, np.float32))
    L, vp = eng.L, C.c_void_p

    def raw(ctx=eng.h, gal=None, labels=lab, Cn=5, q=Q, n_q=NQ, k=3, w=0, T=1.0, out=hold.ptr):
        p = lambda a: None if a is None else a.ctypes.data_as(vp)   # noqa: E731
        return L.vv_gallery_knn_scores(ctx, g.h if gal is None else gal, p(labels), Cn, p(q), n_q, None, k, w, T, out, None)

    def raw_self(ctx=eng.h, labels=lab, Cn=5, k=3, excl=0, w=0, T=1.0, out=hold.ptr):
        return L.vv_gallery_knn_scores_self(ctx, g.h, None if labels is None else labels.ctypes.data_as(vp), Cn, k, excl, w, T, out, None)

    try:
        assert raw() == 0 and (hold.get() != SENTINEL).all()        # the arguments the refusals vary are good ones
        hold.set(np.full((NQ, 5), SENTINEL, np.float32))
        bad = np.array(lab)
        bad[7] = 5
        neg = np.array(lab)
        neg[39] = -1
        for rc in (raw(ctx=None), raw(labels=None), raw(q=None), raw(out=None), raw(ctx=other.h),
                   raw(k=0), raw(k=2049), raw(Cn=0), raw(Cn=4097), raw(n_q=0), raw(labels=bad), raw(labels=neg), raw(w=2), raw(w=-1),
                   raw(w=1, T=0.0), raw(w=1, T=-1.0), raw(w=1, T=float("inf")), raw(w=1, T=float("nan")),
                   raw_self(ctx=None), raw_self(labels=None), raw_self(out=None), raw_self(ctx=other.h), raw_self(k=0), raw_self(k=2049),
                   raw_self(Cn=0), raw_self(Cn=4097), raw_self(labels=bad), raw_self(w=2), raw_self(w=1, T=0.0), raw_self(excl=1)):
            assert rc == 1
        with pytest.raises(vv.VVError, match="error 1"):
            g.knn_scores(Q, lab, 5, 3, q_ids=c["qid"], out=hold)    # q_ids on a gallery without ids
        with pytest.raises(vv.VVError):
            g.knn_scores(Q, lab, 5, 3, weighting="gaussian", out=hold)
        assert raw(w=0, T=float("nan")) == 0                        # the temperature is read under EXP only
        assert raw(Cn=4, labels=lab % 4) == 0                       # (the buffer is large enough for [NQ][4])
        hold.set(np.full((NQ, 5), SENTINEL, np.float32))
        assert raw(labels=bad) == 1 and (hold.get() == SENTINEL).all()
    finally:
        hold.free()
        g.close()
        other.close()


def test_nearest_is_unchanged_by_a_knn_call(eng):
    c = host_case(2500)
    lab = labels_for(2500, 20)
    g = eng.gallery(c["G"], c["gid"])
    try:
        for k in (10, 300):
            before = g.nearest(c["Q"], k, c["qid"])
            g.knn_scores(c["Q"], lab, 20, k, q_ids=c["qid"], weighting="exp", temperature=0.5).free()
            g.knn_scores(c["Q"], lab, 20, 2048).free()
            after = g.nearest(c["Q"], k, c["qid"])
            assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1]))
            want = nearest_ref.nearest(c["d"], c["gid"][None, :] != c["qid"][:, None], k)
            assert np.array_equal(after[0], want[0]) and np.array_equal(bits(after[1]), bits(want[1]))
    finally:
        g.close()


def test_scores_feed_classification_stats_on_the_device(eng):
    """Items of 4 classes around integer centres; the votes of the 15 nearest training items classify the queries."""
    rng = np.random.default_rng(17)
    Cn, dim = 4, 40
    centres = rng.choice([-2, 2], (Cn, dim))
    tr_lab = rng.integers(0, Cn, 600).astype(np.int32)
    train = (centres[tr_lab] + rng.integers(-1, 2, (600, dim))).astype(np.float32)
    te_lab = rng.integers(0, Cn, 150).astype(np.int32)
    test = (centres[te_lab] + rng.integers(-3, 4, (150, dim))).astype(np.float32)
    te_lab[::11] = (te_lab[::11] + 1) % Cn
    scores, _ = ref.knn_scores(nearest_ref.distances32(test, train), None, tr_lab, Cn, 15)
    want = classification_ref.classification_stats(scores, te_lab, Cn)
    g = eng.gallery(train)
    try:
        buf = g.knn_scores(test, tr_lab, Cn, 15)
        acc, ap, cnt, rep = eng.classification_stats(buf, te_lab, Cn)
        assert np.array_equal(buf.get(), scores)
        buf.free()
    finally:
        g.close()
    assert np.array_equal(cnt, want["count"]) and np.array_equal(acc, want["accuracy"]) and rep["total_accuracy"] == want["total_accuracy"]
    assert 0.5 < rep["total_accuracy"] < 1.0
    assert (classification_ref.ulp_diff32(ap, want["ap64"].astype(np.float32)) <= 1).all()
    assert classification_ref.ulp_diff32([rep["mean_ap"]], [np.float32(want["mean_ap64"])])[0] <= 1
