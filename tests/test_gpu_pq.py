"""vv_pq_* and vv_ivfpq_* on the device, bit for bit (np.array_equal; dist compared as bits).  Codebooks and codes must be what the
per-sub-space Gallery.kmeans calls give; a search must be tests/pq_ref.py -- the table chain, the ADC chain, and ivf_ref's selection on
the library's own stored centroid floats; and where every product and sum is exact (integer codewords, items made of them) the search
must equal the fp32 IVFIndex and, with every cluster probed, Gallery.topk."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivf_ref   # noqa: E402
import kmeans_ref   # noqa: E402
import pq_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402
from videovector_amd.engine import _ptr   # noqa: E402

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "spherical"]
F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def stored(eng, rows, q):
    """the floats k_sim_f32 stores for q against `rows`, as Gallery.scores hands them out"""
    g = eng.gallery(rows)
    try:
        s = g.scores(q).get()
    finally:
        g.close()
    return (F32(-2.0) * s + F32(0.0)).astype(F32)


def kmeans_codes(eng, x, cb):
    """code[g][m]: the assignment Gallery(x[:, cols]).kmeans(iters=0, init=cb[m]) returns -- the call the header names, made M times"""
    M, ksub, dsub = cb.shape
    codes = np.zeros((x.shape[0], M), np.int64)
    for m in range(M):
        sub = eng.gallery(np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub]))
        try:
            codes[:, m] = sub.kmeans(ksub, iters=0, init=cb[m]).assign
        finally:
            sub.close()
    return codes


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("ksub", [4, 256])
@pytest.mark.parametrize("M", [1, 3])
def test_train_is_kmeans_per_sub_space(eng, M, ksub):
    n, dim, iters, seed = 300, 24, 2, 9
    x = np.random.default_rng(M * 1000 + ksub).standard_normal((n, dim)).astype(F32)
    gal = eng.gallery(x)
    try:
        cb, obj = eng.pq_train(gal, M, ksub, iters=iters, seed=seed)
        cb2, obj2 = eng.pq_train(gal, M, ksub, iters=iters, seed=seed)
    finally:
        gal.close()
    dsub = dim // M
    assert cb.shape == (M, ksub, dsub) and obj.shape == (M,)
    assert np.array_equal(bits(cb), bits(cb2)) and np.array_equal(obj, obj2)
    for m in range(M):
        sub = eng.gallery(np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub]))
        try:
            r = sub.kmeans(ksub, iters=iters, seed=seed + m)
        finally:
            sub.close()
        assert np.array_equal(bits(cb[m]), bits(r.centroids)), m
        assert obj[m] == r.report["objective_last"] == r.objective[-1], m


# ------------------------------------------------------------------------------------------------ encoding
@pytest.mark.parametrize("ksub", [4, 256])
@pytest.mark.parametrize("M", [1, 3])
def test_encode_is_kmeans_assignment_and_codes_follow_the_lists(eng, M, ksub):
    n, dim, Cn = 300, 24, 5
    rng = np.random.default_rng(M * 77 + ksub)
    x = rng.standard_normal((n, dim)).astype(F32)
    dsub = dim // M
    # codewords that are items' own sub-vectors: the item a codeword was taken from lies on it, so codes 0 and ksub - 1 occur by construction
    rows = np.stack([rng.permutation(n)[:ksub] for _ in range(M)])
    cb = np.stack([x[rows[m], m * dsub:(m + 1) * dsub] for m in range(M)]).astype(F32)
    want = kmeans_codes(eng, x, cb)
    for m in range(M):
        assert want[rows[m, 0], m] == 0 and want[rows[m, ksub - 1], m] == ksub - 1
    assert want.min() == 0 and want.max() == ksub - 1
    gal = eng.gallery(x)
    try:
        got = eng.pq_encode(gal, cb)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assign = rng.integers(0, Cn, n).astype(np.int32)
        ix = eng.ivfpq(gal, x[:Cn], cb, assign=assign)
        try:
            start, lst = ix.lists()
            rs, rl = ivf_ref.lists_of(assign, Cn)
            assert np.array_equal(start, rs) and np.array_equal(lst, rl)
            assert np.array_equal(ix.codes(), want[lst])
            assert (ix.get("M"), ix.get("ksub"), ix.get("n_ref"), ix.get("dim"), ix.get("num_clusters")) == (M, ksub, n, dim, Cn)
            assert ix.get("last_scan_form") == 0
        finally:
            ix.close()
        # the index that assigns for itself: the lists of the clustering's own assignment
        km = gal.kmeans(Cn, iters=1, metric="spherical", seed=3)
        ix = km.ivfpq(gal, cb)
        try:
            start, lst = ix.lists()
            rs, rl = ivf_ref.lists_of(km.assign, Cn)
            assert np.array_equal(start, rs) and np.array_equal(lst, rl) and ix.get("metric") == 1
            assert np.array_equal(ix.codes(), want[lst])
        finally:
            ix.close()
    finally:
        gal.close()


# ------------------------------------------------------------------------------------------------ search against the restatement
SIZES = [0, 1, 63, 64, 65, 257, 1025]         # the lists: empty, one item, around one wave, past one workgroup pass (256), past four
SHAPES = [(1, 8, 256, 3), (3, 3, 16, 3), (4, 1, 2, 2), (8, 3, 16, 2), (16, 8, 2, 1), (64, 1, 16, 1), (64, 8, 256, 1)]   # M, dsub, ksub, scan form
_cases = {}


def search_case(eng, M, dsub, ksub):
    """built once per shape and left unchanged"""
    key = (M, dsub, ksub)
    if key not in _cases:
        rng = np.random.default_rng(M * 10000 + dsub * 1000 + ksub)
        n, dim, Cn = sum(SIZES), M * dsub, len(SIZES)
        x = rng.standard_normal((n, dim)).astype(F32)
        cent = rng.standard_normal((Cn, dim)).astype(F32)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True).astype(F32)       # a copy of a centroid is nearest to it under either metric
        assign = rng.permutation(np.repeat(np.arange(Cn), SIZES)).astype(np.int32)
        q = rng.standard_normal((70, dim)).astype(F32)
        if dim > 1:
            q[0], q[1], q[2] = cent[0], cent[1], cent[6]                       # nprobe = 1: the empty list, the list of one, the largest
        gal = eng.gallery(x)
        try:
            cb, _ = eng.pq_train(gal, M, ksub, iters=1, seed=5)
        finally:
            gal.close()
        codes = kmeans_codes(eng, x, cb)
        a = ref.adc(ref.table(q, cb), codes)
        _cases[key] = dict(x=x, cent=cent, assign=assign, q=q, cb=cb, codes=codes, a=a, d_cent=stored(eng, cent, q),
                           nn=kmeans_ref.chain_sq(cent), lists=ivf_ref.lists_of(assign, Cn))
    return _cases[key]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("M,dsub,ksub,form", SHAPES)
def test_search_is_the_restatement(eng, M, dsub, ksub, form, metric):
    c = search_case(eng, M, dsub, ksub)
    start, lst = c["lists"]
    Cn = len(SIZES)
    gal = eng.gallery(c["x"])
    ix = eng.ivfpq(gal, c["cent"], c["cb"], metric=metric, assign=c["assign"])
    gal.close()                                                               # the index owns what it needs
    try:
        assert ix.get("last_scan_form") == 0 and ix.get("largest_list") == 1025 and ix.get("empty_lists") == 1
        assert np.array_equal(ix.codes(), c["codes"][lst])
        short = 0
        for n_q in (1, 5, 70):
            eng.set_option("ivf_block_rows", 64 if n_q == 70 else 0)
            for nprobe in (1, 3, Cn):
                for k in (1, 32):
                    want = ivf_ref.search(c["a"][:n_q], c["d_cent"][:n_q], c["nn"], metric, start, lst, nprobe, k)
                    idx, dist, m = ix.search(c["q"][:n_q], k, nprobe)
                    at = (M, dsub, ksub, metric, n_q, nprobe, k)
                    assert np.array_equal(idx, want["idx"]), (at, np.argwhere(idx != want["idx"])[:5])
                    assert np.array_equal(bits(dist), bits(want["dist"])), at
                    assert np.array_equal(m, want["n_candidates"]), at
                    assert ix.get("last_candidates") == want["candidates"] and ix.get("last_scan_form") == form, at
                    assert ix.get("last_blocks") == (2 if n_q == 70 else 1), at
                    again = ix.search(c["q"][:n_q], k, nprobe)
                    assert np.array_equal(again[0], idx) and np.array_equal(bits(again[1]), bits(dist)) and np.array_equal(again[2], m), at
                    short += int((want["n_candidates"] < k).sum())
                    if M * dsub > 1 and nprobe == 1 and n_q >= 5:
                        assert want["n_candidates"][:3].tolist() == [0, 1, 1025], at
                        assert (idx[0] == -1).all() and (dist[0] == 0).all() and idx[1, 0] >= 0 and (idx[1, 1:] == -1).all(), at
        assert short or M * dsub == 1                                        # k > m_i was met
    finally:
        eng.set_option("ivf_block_rows", 0)
        ix.close()


# ------------------------------------------------------------------------------------------------ the exactness anchor
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("M,dsub,ksub", [(8, 4, 16), (64, 8, 256)])
def test_exact_arithmetic_makes_it_the_fp32_index(eng, M, dsub, ksub, metric):
    # integer codewords with |entry| <= 4, distinct within a sub-space; every item is a concatenation of codewords, every query integer: all
    # products and sums are small integers, exact in fp32 in any order, so a(i, g) IS d(i, g) and each sub-vector's nearest codeword is itself
    n, n_q, Cn, dim = 600, 40, 5, M * dsub
    rng = np.random.default_rng(M + ksub)
    cb = np.zeros((M, ksub, dsub), F32)
    for m in range(M):
        words = set()
        while len(words) < ksub:
            words.add(tuple(rng.integers(-4, 5, dsub).tolist()))
        cb[m] = np.array(sorted(words), F32)[rng.permutation(ksub)]
    codes = rng.integers(0, ksub, (n, M))
    codes[0], codes[1] = 0, ksub - 1
    x = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1).astype(F32)
    q = rng.integers(-4, 5, (n_q, dim)).astype(F32)
    cent = rng.integers(-4, 5, (Cn, dim)).astype(F32)
    assign = rng.integers(0, Cn, n).astype(np.int32)
    gal = eng.gallery(x)
    pq = eng.ivfpq(gal, cent, cb, metric=metric, assign=assign)
    flat = eng.ivf(gal, cent, metric=metric, assign=assign)
    try:
        assert np.array_equal(eng.pq_encode(gal, cb), codes)
        for nprobe in (1, 2, Cn):
            for k in (1, 32):
                got, want = pq.search(q, k, nprobe), flat.search(q, k, nprobe)
                assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2]), (nprobe, k)
                if nprobe == Cn:
                    top = gal.topk(q, k)
                    assert np.array_equal(got[0], top[0]) and np.array_equal(bits(got[1]), bits(top[1])), k
    finally:
        pq.close(); flat.close(); gal.close()


# ------------------------------------------------------------------------------------------------ memory
def test_the_index_keeps_codes_not_rows(eng):
    n, Cn, M, ksub, dsub = 2000, 7, 64, 256, 8
    dim = M * dsub
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n, dim)).astype(F32)
    gal = eng.gallery(x)
    ix = eng.ivfpq(gal, x[:Cn], x[:ksub].reshape(ksub, M, dsub).transpose(1, 0, 2), assign=rng.integers(0, Cn, n).astype(np.int32))
    try:
        # codes, codebooks, centroids, nn, start, list: with Dp = dim = 512 the codes and the list are 68 bytes an item against 2048, and
        # the codebooks are 256 rows' worth -- below n rows by construction once n > 256 + C + a few
        want = n * M + M * ksub * dsub * 4 + Cn * dim * 4 + Cn * 4 + (Cn + 1) * 4 + n * 4
        assert ix.get("index_bytes") == want and want < n * dim * 4
        ix.search(x[:3], 4, 2)
        assert ix.get("index_bytes") == want                                  # scratch is not counted
    finally:
        ix.close(); gal.close()


# ------------------------------------------------------------------------------------------------ errors
def test_every_refusal_names_its_argument_and_leaves_the_context_usable(eng):
    n, dim, Cn, M, ksub = 50, 24, 4, 3, 4
    rng = np.random.default_rng(2)
    x = rng.standard_normal((n, dim)).astype(F32)
    cent = x[:Cn].copy()
    cb = np.ascontiguousarray(x[:ksub].reshape(ksub, M, dim // M).transpose(1, 0, 2))
    q = rng.standard_normal((3, dim)).astype(F32)
    assign = rng.integers(0, Cn, n).astype(np.int32)
    gal = eng.gallery(x)
    other = vv.Engine(0, "f16")
    foreign = other.gallery(x)
    ix = eng.ivfpq(gal, cent, cb, assign=assign)
    foreign_ix = other.ivfpq(foreign, cent, cb, assign=assign)
    big_gal = eng.gallery(np.zeros((4100, 2), F32))
    L = eng.L
    shapes = [("no sub-space", 0, ksub, "M = 0"), ("too many sub-spaces", 65, ksub, "M = 65"), ("M does not divide dim", 5, ksub, "M = 5"),
              ("one codeword", M, 1, "ksub = 1"), ("too many codewords", M, 257, "ksub = 257"), ("more codewords than items", M, 64, "ksub = 64")]
    try:
        # ---- vv_pq_train / vv_pq_encode: the outputs keep their fill
        big = np.full(65 * 257 * dim, -7.5, F32)
        for name, m_, k_, word in shapes:
            obj, codes = np.full(65, -7.5), np.full(n * 65, 9, np.uint8)
            assert L.vv_pq_train(eng.h, gal.h, m_, k_, 1, 0, _ptr(big), _ptr(obj)) == 1, name
            assert word in L.vv_last_error().decode() and "vv_pq_train" in L.vv_last_error().decode(), (name, L.vv_last_error())
            assert L.vv_pq_encode(eng.h, gal.h, _ptr(big), m_, k_, _ptr(codes)) == 1, name
            assert word in L.vv_last_error().decode() and "vv_pq_encode" in L.vv_last_error().decode(), (name, L.vv_last_error())
            assert (big == -7.5).all() and (obj == -7.5).all() and (codes == 9).all(), name
        for name, args, word in [("NULL items", (None, M, ksub, 1, 0, _ptr(big), None), "items is NULL"),
                                 ("NULL codebooks_out", (gal.h, M, ksub, 1, 0, None, None), "codebooks_out is NULL"),
                                 ("another context", (foreign.h, M, ksub, 1, 0, _ptr(big), None), "another context"),
                                 ("negative iters", (gal.h, M, ksub, -1, 0, _ptr(big), None), "iters = -1")]:
            assert L.vv_pq_train(eng.h, *args) == 1 and word in L.vv_last_error().decode(), (name, L.vv_last_error())
        codes = np.full(n * M, 9, np.uint8)
        for name, args, word in [("NULL items", (None, _ptr(cb), M, ksub, _ptr(codes)), "items is NULL"),
                                 ("NULL codebooks", (gal.h, None, M, ksub, _ptr(codes)), "codebooks is NULL"),
                                 ("NULL codes_out", (gal.h, _ptr(cb), M, ksub, None), "codes_out is NULL"),
                                 ("another context", (foreign.h, _ptr(cb), M, ksub, _ptr(codes)), "another context")]:
            assert L.vv_pq_encode(eng.h, *args) == 1 and word in L.vv_last_error().decode(), (name, L.vv_last_error())
        assert (big == -7.5).all() and (codes == 9).all()
        # ---- vv_ivfpq_create
        bad_hi, bad_lo = assign.copy(), assign.copy()
        bad_hi[17], bad_lo[31] = Cn, -1
        creates = [
            ("NULL items", None, cent, Cn, 0, assign, cb, M, ksub, False, "items is NULL"),
            ("NULL centroids", gal.h, None, Cn, 0, assign, cb, M, ksub, False, "centroids is NULL"),
            ("NULL codebooks", gal.h, cent, Cn, 0, assign, None, M, ksub, False, "codebooks is NULL"),
            ("NULL out", gal.h, cent, Cn, 0, assign, cb, M, ksub, True, "out is NULL"),
            ("another context", foreign.h, cent, Cn, 0, assign, cb, M, ksub, False, "another context"),
            ("no clusters", gal.h, cent, 0, 0, assign, cb, M, ksub, False, "C = 0"),
            ("too many clusters", big_gal.h, cent, 4097, 0, None, cb, 1, 2, False, "C = 4097"),
            ("more clusters than items", gal.h, cent, n + 1, 0, None, cb, M, ksub, False, "exceeds"),
            ("unknown metric", gal.h, cent, Cn, 2, assign, cb, M, ksub, False, "unknown metric 2"),
            ("entry past the clusters", gal.h, cent, Cn, 0, bad_hi, cb, M, ksub, False, "assign[17] = %d" % Cn),
            ("negative entry", gal.h, cent, Cn, 1, bad_lo, cb, M, ksub, False, "assign[31] = -1"),
        ] + [(name, gal.h, cent, Cn, 0, assign, big, m_, k_, False, word) for name, m_, k_, word in shapes]
        for name, items, ce, cn, metric, asg, books, m_, k_, null_out, word in creates:
            h = C.c_void_p(0x5a5a)
            rc = L.vv_ivfpq_create(eng.h, items, _ptr(ce), cn, metric, _ptr(asg), _ptr(books), m_, k_, None if null_out else C.byref(h))
            assert rc == 1, name                                             # VV_ERR_ARG
            assert word in L.vv_last_error().decode(), (name, L.vv_last_error())
            assert h.value == 0x5a5a, name
        # ---- vv_ivfpq_search: the outputs keep their fill, the index its record of the last search
        ix.search(q, 2, 2)
        last = {k: ix.get(k) for k in ("last_blocks", "last_candidates", "last_scan_form", "last_device_ms", "last_scan_ms", "last_lut_ms")}
        assert last["last_scan_form"] == 3
        searches = [
            ("NULL index", None, q, 3, 2, 2, (), "index is NULL"),
            ("NULL q", ix.h, None, 3, 2, 2, (), "q is NULL"),
            ("NULL idx", ix.h, q, 3, 2, 2, ("idx",), "idx is NULL"),
            ("NULL dist", ix.h, q, 3, 2, 2, ("dist",), "dist is NULL"),
            ("another context", foreign_ix.h, q, 3, 2, 2, (), "another context"),
            ("no query", ix.h, q, 0, 2, 2, (), "n_q = 0"),
            ("negative n_q", ix.h, q, -1, 2, 2, (), "n_q = -1"),
            ("no probe", ix.h, q, 3, 0, 2, (), "nprobe = 0"),
            ("more probes than clusters", ix.h, q, 3, Cn + 1, 2, (), "nprobe = %d" % (Cn + 1)),
            ("no k", ix.h, q, 3, 2, 0, (), "k = 0"),
            ("k past the limit", ix.h, q, 3, 2, 33, (), "k = 33"),
        ]
        for name, handle, qq, n_q, nprobe, k, null, word in searches:
            idx, dist, m = np.full((3, 33), -9, np.int32), np.full((3, 33), -7.5, F32), np.full(3, -9, np.int32)
            rc = L.vv_ivfpq_search(eng.h, handle, _ptr(qq), n_q, nprobe, k, None if "idx" in null else _ptr(idx),
                                   None if "dist" in null else _ptr(dist), _ptr(m))
            assert rc == 1, name
            assert word in L.vv_last_error().decode(), (name, L.vv_last_error())
            assert (idx == -9).all() and (dist == -7.5).all() and (m == -9).all(), name
            assert {k_: ix.get(k_) for k_ in last} == last, name
        # nprobe between 64 and C on an index of more than 64 clusters; nprobe == C is always allowed
        wide = eng.ivfpq(big_gal, np.zeros((100, 2), F32), np.arange(4, dtype=F32).reshape(1, 2, 2), assign=np.zeros(4100, np.int32))
        try:
            idx, dist = np.full((1, 2), -9, np.int32), np.full((1, 2), -7.5, F32)
            assert L.vv_ivfpq_search(eng.h, wide.h, _ptr(np.zeros((1, 2), F32)), 1, 65, 2, _ptr(idx), _ptr(dist), None) == 1
            assert "nprobe = 65" in L.vv_last_error().decode() and (idx == -9).all() and (dist == -7.5).all()
            assert wide.search(np.zeros((1, 2), F32), 2, 64)[0].tolist() == [[0, 1]]
            assert wide.search(np.zeros((1, 2), F32), 2, 100)[0].tolist() == [[0, 1]]
        finally:
            wide.close()
        # dim not the index's, codebooks of another dim, an unknown name, and the other calls' own refusals
        with pytest.raises(vv.VVError):
            ix.search(np.zeros((3, dim + 1), F32), 2, 2)
        with pytest.raises(vv.VVError):
            eng.ivfpq(gal, cent, cb[:, :, :-1], assign=assign)
        with pytest.raises(vv.VVError):
            ix.get("last_tiles")
        v = C.c_double(-3.0)
        assert L.vv_ivfpq_get(ix.h, b"no_such_name", C.byref(v)) == 1 and v.value == -3.0 and b"no_such_name" in L.vv_last_error()
        s, l, cd = np.full(Cn + 1, -9, np.int32), np.full(n, -9, np.int32), np.full(n * M, 9, np.uint8)
        assert L.vv_ivfpq_lists(eng.h, foreign_ix.h, _ptr(s), _ptr(l)) == 1 and (s == -9).all() and (l == -9).all()
        assert L.vv_ivfpq_codes(eng.h, foreign_ix.h, _ptr(cd)) == 1 and (cd == 9).all()
        assert L.vv_ivfpq_destroy(eng.h, foreign_ix.h) == 1 and b"another context" in L.vv_last_error()
        # ... and the same calls with nothing wrong run
        idx, dist, m = ix.search(q, 2, 2)
        assert (idx >= 0).all() and (m > 0).all()
        assert eng.pq_train(gal, M, ksub, iters=1)[0].shape == cb.shape and eng.pq_encode(gal, cb).shape == (n, M)
    finally:
        ix.close(); foreign_ix.close(); big_gal.close(); foreign.close(); other.close(); gal.close()
