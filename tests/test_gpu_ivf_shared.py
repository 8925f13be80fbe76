"""What IVFIndex and IVFPQIndex take from the one coarse index and the one search loop under them (csrc/ivf_coarse.hip), on one small
pair of indexes over the same gallery, centroids and assignment: every refusal begins with the refusing index's own function name, each
index answers the shared names alike and only its own beside them, and a search cut into blocks returns what the uncut one does."""
import ctypes as C

import numpy as np
import pytest

import videovector_amd as vv
from videovector_amd.engine import _ptr

pytestmark = pytest.mark.gpu

F32 = np.float32
N, DIM, CN, M, KSUB = 300, 48, 7, 4, 16
SHARED = ["n_ref", "dim", "num_clusters", "metric", "largest_list", "empty_lists", "last_blocks", "last_candidates", "last_probe_ms",
          "last_select_ms", "last_device_ms"]


@pytest.fixture(scope="module")
def case():
    eng = vv.Engine(0, "f16")
    rng = np.random.default_rng(20)
    x = rng.standard_normal((N, DIM)).astype(F32)
    cent = x[:CN].copy()
    assign = rng.integers(0, CN - 1, N).astype(np.int32)                        # cluster CN - 1 stays empty
    q = rng.standard_normal((5, DIM)).astype(F32)
    gal = eng.gallery(x)
    cb, _ = eng.pq_train(gal, M, KSUB, iters=2)
    idxs = {"vv_ivf": eng.ivf(gal, cent, metric="euclidean", assign=assign),
            "vv_ivfpq": eng.ivfpq(gal, cent, cb, metric="euclidean", assign=assign)}
    yield dict(eng=eng, gal=gal, cent=cent, assign=assign, cb=cb, q=q, ix=idxs)
    for ix in idxs.values():
        ix.close()
    gal.close()
    eng.close()


def refused(L, who, rc):
    msg = L.vv_last_error().decode()
    assert rc == 1 and msg.startswith(who + ":"), (who, rc, msg)
    return msg


@pytest.mark.parametrize("fn", ["vv_ivf", "vv_ivfpq"])
def test_every_refusal_begins_with_the_index_s_own_function(case, fn):
    eng, ix, q, L = case["eng"], case["ix"][fn], case["q"], case["eng"].L
    search, create = getattr(L, fn + "_search"), getattr(L, fn + "_create")
    other = vv.Engine(0, "f16")
    try:
        for ctx, n_q, nprobe, k, word in [(eng.h, 5, 0, 3, "nprobe = 0"), (eng.h, 5, CN + 1, 3, "nprobe = 8"), (eng.h, 5, 2, 0, "k = 0"),
                                          (eng.h, 5, 2, 33, "k = 33"), (eng.h, 0, 2, 3, "n_q = 0"), (other.h, 5, 2, 3, "another context")]:
            idx, dist, m = np.full((5, 33), -9, np.int32), np.full((5, 33), -7.5, F32), np.full(5, -9, np.int32)
            msg = refused(L, fn + "_search", search(ctx, ix.h, _ptr(q), n_q, nprobe, k, _ptr(idx), _ptr(dist), _ptr(m)))
            assert word in msg and (idx == -9).all() and (dist == -7.5).all() and (m == -9).all(), msg
    finally:
        other.close()
    bad = case["assign"].copy()
    bad[0] = CN
    books = () if fn == "vv_ivf" else (_ptr(case["cb"]), M, KSUB)
    for cn, metric, asg, word in [(0, 0, case["assign"], "C = 0"), (N + 1, 0, case["assign"], "C = 301"), (CN, 9, case["assign"], "metric 9"),
                                  (CN, 0, bad, "assign[0] = 7")]:
        h = C.c_void_p(0x5a5a)
        msg = refused(L, fn + "_create", create(eng.h, case["gal"].h, _ptr(case["cent"]), cn, metric, _ptr(asg), *books, C.byref(h)))
        assert word in msg and h.value == 0x5a5a, msg
    assert ix.search(q, 3, 2)[0].shape == (5, 3)                                # ... and the context still runs


def test_shared_names_answer_alike_and_own_names_only_on_their_index(case):
    flat, pq = case["ix"]["vv_ivf"], case["ix"]["vv_ivfpq"]
    for ix, names in [(flat, ["M", "ksub", "index_bytes", "last_scan_form", "last_lut_ms", "last_scan_ms"]),
                      (pq, ["last_tiles", "last_grid_wgs", "last_group_ms", "last_sim_ms"])]:
        for name in names:
            with pytest.raises(vv.VVError):
                ix.get(name)
    flat.search(case["q"], 3, 2); pq.search(case["q"], 3, 2)
    counts = np.bincount(case["assign"], minlength=CN)
    want = dict(n_ref=N, dim=DIM, num_clusters=CN, metric=0, largest_list=counts.max(), empty_lists=(counts == 0).sum(), last_blocks=1)
    for name in SHARED:
        a, b = flat.get(name), pq.get(name)                                     # every shared name answers on both
        if name in want:
            assert a == b == want[name], name
    assert flat.get("last_candidates") == pq.get("last_candidates") > 0 and want["empty_lists"] == 1
    assert flat.get("last_tiles") > 0 and pq.get("M") == M and pq.get("ksub") == KSUB
    for got, ref in zip(flat.lists(), pq.lists()):
        assert np.array_equal(got, ref)
    assert np.array_equal(np.diff(flat.lists()[0]), counts) and np.array_equal(np.sort(flat.lists()[1]), np.arange(N))


def test_blocks_change_nothing_on_either_index(case):
    eng, q = case["eng"], case["q"]
    cands = {}
    try:
        for fn, ix in case["ix"].items():
            for nprobe, k in [(2, 3), (CN, 32)]:                                # (the second grows the scratch, the third call reuses it)
                eng.set_option("ivf_block_rows", 0)
                whole = ix.search(q, k, nprobe)
                assert ix.get("last_blocks") == 1
                eng.set_option("ivf_block_rows", 2)
                cut = ix.search(q, k, nprobe)
                assert ix.get("last_blocks") == 3
                for a, b in zip(whole, cut):
                    assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), (fn, nprobe, k)
                assert ix.get("last_candidates") == whole[2].sum()
                cands[fn, nprobe] = whole[2]
    finally:
        eng.set_option("ivf_block_rows", 0)
    for nprobe in (2, CN):
        assert np.array_equal(cands["vv_ivf", nprobe], cands["vv_ivfpq", nprobe]), nprobe
    assert (cands["vv_ivf", CN] == N).all() and (cands["vv_ivf", 2] < N).all()
