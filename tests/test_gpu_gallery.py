"""GPU tests of gallery retrieval (vv_gallery_*, Engine.gallery, the facade's RETRIEVAL_RANK_STATS_FIXED_REF layer and the
rank_stats tool) against tests/gallery_ref.py, the float64 restatement of the reference layer.

Tolerances.  A top-k slot or a best rank may differ from the float64 order only as a NEAR TIE: the float64 distances of the
returned and the expected item differ by at most eps, where eps is four times the largest |d32 - d64| that numpy's own float32
product shows on the same input (a factor of four lies between two float32 summation orders on these inputs).  At most 1 % of
the slots / queries may use the exemption.  Per-query AP and the summary values: 1e-4; median rank and everything integer: exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gallery_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402
from videovector_amd.synth import SyntheticVideos, init_weights   # noqa: E402

pytestmark = pytest.mark.gpu

INPUTS = {"A": dict(nq=256, ng=100000, D=512, nid=2000, noise=4.0, seed=5),
          "B": dict(nq=193, ng=50001, D=96, nid=700, noise=1.8, seed=6)}
EXPECT64 = {"A": dict(median_rank=25, recall_1=0.0820, mean_ap=0.00980),
            "B": dict(median_rank=1, recall_1=0.658, recall_5=0.528, mean_ap=0.1696)}
_cache = {}


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def case(name):
    if name not in _cache:
        Q, qid, G, gid = ref.make_input(**INPUTS[name])
        d64 = ref.distances(Q, G)
        d32 = ref.distances(Q, G, np.float32)
        eps = 4.0 * float(np.abs(d32.astype(np.float64) - d64).max())
        summary, best, ap, order = ref.rank_stats(d64, qid, gid)
        _cache[name] = dict(Q=Q, qid=qid, G=G, gid=gid, d64=d64, eps=eps, summary=summary, best=best, ap=ap, order=order)
    return _cache[name]


def check_against(e, Q, qid, G, gid, k, exact=False):
    """Top-k and rank statistics of the engine against float64 (exact: no near-tie exemption at all)."""
    d64 = ref.distances(Q, G)
    eps = 0.0 if exact else 4.0 * float(np.abs(ref.distances(Q, G, np.float32).astype(np.float64) - d64).max())
    summary, best, ap, order = ref.rank_stats(d64, qid, gid)
    g = e.gallery(G, gid)
    try:
        idx, dist = g.topk(Q, k)
        st = g.rank_stats(Q, qid, per_query=True)
        passes = int(g.get("last_passes"))
        assert g.scratch_bytes <= 1 << 30
    finally:
        g.close()
    rows = np.arange(Q.shape[0])[:, None]
    near = np.abs(d64[rows, idx] - d64[rows, order[:, :k]])
    assert (near <= eps).all(), near.max()
    assert (idx != order[:, :k]).sum() <= 0.01 * idx.size
    assert np.abs(dist - d64[rows, idx]).max() <= max(eps, 1e-6)
    assert np.array_equal(st["top5_idx"][:, :min(5, k)], idx[:, :min(5, k)]) or k < 5
    bad = 0
    for i in np.flatnonzero(st["best_rank"] != best):
        lo, hi = ref.best_rank_interval(d64[i], np.flatnonzero(gid == qid[i]), eps)
        assert lo <= st["best_rank"][i] <= hi, (i, st["best_rank"][i], best[i], lo, hi)
        bad += 1
    assert bad <= 0.01 * len(best)
    assert np.abs(st["ap"] - ap).max() <= 1e-4
    assert st["median_rank"] == summary["median_rank"] or bad
    for f in ("recall_1", "recall_5", "recall_10", "mean_ap"):
        assert abs(st[f] - summary[f]) <= 1e-4, (f, st[f], summary[f])
    return passes


def test_known_answer(eng):
    Q = np.array([[1, 0], [0, 1], [.6, .8], [1, 0]], np.float32)
    qid = np.array([7, 7, 9, 3], np.int32)
    G = np.array([[1, 0], [.8, .6], [0, 1], [.6, .8], [1, 0], [-1, 0]], np.float32)
    gid = np.array([9, 7, 7, 9, 7, 5], np.int32)
    g = eng.gallery(G, gid)
    idx, dist = g.topk(Q, 5)
    st = g.rank_stats(Q, qid, per_query=True)
    g.close()
    assert idx.tolist() == [[0, 4, 1, 3, 2], [2, 3, 1, 0, 4], [3, 1, 2, 0, 4], [0, 4, 1, 3, 2]]
    assert st["top5_idx"].tolist() == idx.tolist()
    assert np.abs(dist - ref.distances(Q, G)[np.arange(4)[:, None], idx]).max() <= 1e-6
    assert st["best_rank"].tolist() == [2, 1, 1, 10000]
    assert np.abs(st["ap"] - np.array([0.588889, 0.755556, 0.75, 0])).max() <= 1e-6
    assert abs(st["ap"][0] - (1 / 2 + 2 / 3 + 3 / 5) / 3) <= 1e-6
    assert st["median_rank"] == 1.5
    for f, v in (("recall_1", 0.5), ("recall_5", 0.75), ("recall_10", 0.75), ("mean_ap", 0.523611)):
        assert abs(st[f] - v) <= 1e-6, (f, st[f])


@pytest.mark.parametrize("name", ["A", "B"])
def test_float64_reference_figures(name):
    """The generator reproduces the figures the float64 reference gives on the two inputs (a check of the test's own inputs)."""
    c = case(name)
    for f, v in EXPECT64[name].items():
        assert abs(c["summary"][f] - v) <= (0 if f == "median_rank" else 6e-4), (f, c["summary"][f])


@pytest.mark.parametrize("name", ["A", "B"])
def test_top10_against_float64(eng, name):
    c = case(name)
    g = eng.gallery(c["G"], c["gid"])
    idx, dist = g.topk(c["Q"], 10)
    scratch = g.scratch_bytes
    g.close()
    rows = np.arange(c["Q"].shape[0])[:, None]
    want = c["order"][:, :10]
    gap = np.abs(c["d64"][rows, idx] - c["d64"][rows, want])
    print("%s: eps %.3g, slots that differ %d of %d, largest gap %.3g, largest |dist - d64| %.3g, scratch %d bytes"
          % (name, c["eps"], int((idx != want).sum()), idx.size, gap.max(), np.abs(dist - c["d64"][rows, idx]).max(), scratch))
    assert (gap <= c["eps"]).all()
    assert (idx != want).sum() <= 0.01 * idx.size
    assert np.abs(dist - c["d64"][rows, idx]).max() <= c["eps"]
    assert 0 < scratch <= 1 << 30


@pytest.mark.parametrize("name", ["A", "B"])
def test_rank_stats_against_float64(eng, name):
    c = case(name)
    g = eng.gallery(c["G"], c["gid"])
    st = g.rank_stats(c["Q"], c["qid"], per_query=True)
    scratch = g.scratch_bytes
    g.close()
    differ = np.flatnonzero(st["best_rank"] != c["best"])
    print("%s: best ranks that differ %d of %d, largest |ap - ap64| %.3g, summary %s, float64 %s"
          % (name, len(differ), len(c["best"]), np.abs(st["ap"] - c["ap"]).max(),
             {f: st[f] for f in c["summary"]}, c["summary"]))
    for i in differ:
        lo, hi = ref.best_rank_interval(c["d64"][i], np.flatnonzero(c["gid"] == c["qid"][i]), c["eps"])
        assert lo <= st["best_rank"][i] <= hi, (i, st["best_rank"][i], c["best"][i])
    assert len(differ) <= 0.01 * len(c["best"])
    assert np.abs(st["ap"] - c["ap"]).max() <= 1e-4
    assert st["median_rank"] == c["summary"]["median_rank"]
    for f in ("recall_1", "recall_5", "recall_10", "mean_ap"):
        assert abs(st[f] - c["summary"][f]) <= 1e-4, (f, st[f], c["summary"][f])
    assert 0 < scratch <= 1 << 30


@pytest.mark.parametrize("k", [1, 32])
def test_k_extremes(eng, k):
    Q, qid, G, gid = ref.make_input(nq=37, ng=3001, D=40, nid=50, noise=1.0, seed=11)
    check_against(eng, Q, qid, G, gid, k)


def test_single_query(eng):
    Q, qid, G, gid = ref.make_input(nq=1, ng=2000, D=64, nid=20, noise=1.0, seed=12)
    check_against(eng, Q, qid, G, gid, 10)


def test_single_reference_and_k_beyond_gallery(eng):
    Q, qid, G, gid = ref.make_input(nq=5, ng=1, D=16, nid=1, noise=1.0, seed=13)
    check_against(eng, Q, qid, G, gid, 1)
    g = eng.gallery(G, gid)
    with pytest.raises(vv.VVError, match="error 1"):
        g.topk(Q, 2)
    with pytest.raises(vv.VVError, match="error 1"):
        g.topk(Q, 0)
    g.close()
    Q, qid, G, gid = ref.make_input(nq=5, ng=7, D=16, nid=3, noise=1.0, seed=14)
    g = eng.gallery(G, gid)
    with pytest.raises(vv.VVError, match="error 1"):
        g.topk(Q, 8)
    with pytest.raises(vv.VVError, match="error 1"):
        g.topk(Q, 33)
    g.close()
    g = eng.gallery(G)                                   # no ids: top-k only
    g.topk(Q, 3)
    with pytest.raises(vv.VVError, match="error 1"):
        g.rank_stats(Q, qid)
    g.close()


def test_query_id_absent_from_gallery(eng):
    Q, qid, G, gid = ref.make_input(nq=9, ng=1500, D=32, nid=12, noise=1.0, seed=15)
    qid = qid.copy()
    qid[[0, 4]] = 999
    check_against(eng, Q, qid, G, gid, 5)


def test_one_id_owns_a_third_of_the_gallery(eng):
    """20 000 positives for some queries: more than one pass of positives holds, so their ranks come from several passes."""
    rng = np.random.default_rng(16)
    ng, D, big = 60000, 48, 20000
    gid = rng.integers(1, 40, ng).astype(np.int32)
    gid[rng.permutation(ng)[:big]] = 0
    own = int((gid == 0).sum())
    qid = np.array([0, 3, 0, 17, 0, 999], np.int32)
    G = rng.standard_normal((ng, D))
    Q = rng.standard_normal((len(qid), D))
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    passes = check_against(eng, Q.astype(np.float32), qid, G.astype(np.float32), gid, 10)
    g = eng.gallery(G[:8].astype(np.float32), gid[:8])
    chunk = int(g.get("positive_chunk"))
    g.close()
    assert own >= 3 * chunk, "raise the count: %d positives are fewer than three passes of %d" % (own, chunk)
    assert passes >= 3 and passes == -(-own // chunk)


def test_query_bit_identical_to_gallery_rows(eng):
    """Queries that ARE gallery rows, in a gallery that holds every row twice: exact ties, ordered by index as the reference
    restatement orders them.  Integer-valued features make every float32 product exact, so nothing is exempted."""
    rng = np.random.default_rng(17)
    base = rng.integers(-3, 4, (600, 24)).astype(np.float32)
    G = np.concatenate([base, base])
    gid = np.concatenate([np.arange(600) % 50, np.arange(600) % 50]).astype(np.int32)
    Q = G[[5, 605, 17, 300, 1199]].copy()
    qid = gid[[5, 605, 17, 300, 1199]].copy()
    check_against(eng, Q, qid, G, gid, 12, exact=True)


def test_gallery_from_table_equals_gallery_of_embeddings():
    ds = SyntheticVideos(seed=1701, n_videos=50)
    F, D = 128, 32
    W, b = init_weights(1, D, F, std=0.02)
    e = vv.Engine(0, "f16")
    e.table_synth(ds.seed, ds.n_rows, F)
    e.params_set(W, b)
    rng = np.random.default_rng(18)
    n = min(900, ds.n_rows)
    rows = rng.integers(0, ds.n_rows, (n, 3)).astype(np.int32)
    coeff = np.array([0.5, 0.25, 0.25], np.float32)
    ids = rng.integers(0, 30, n).astype(np.int32)
    qrows = rng.integers(0, ds.n_rows, (40, 3)).astype(np.int32)
    Q = e.embed_mean(qrows, coeff, relu=True, l2norm=True)
    for r, cf, emb in ((rows, coeff, e.embed_mean(rows, coeff, relu=True, l2norm=True)),
                       (rows[:, 0], None, e.embed(rows[:, 0], relu=True, l2norm=True))):
        g1 = e.gallery(emb, ids)
        g2 = e.gallery_from_table(r, ids, coeff=cf, relu=True, l2norm=True)
        i1, d1 = g1.topk(Q, 10)
        i2, d2 = g2.topk(Q, 10)
        s1 = g1.rank_stats(Q, ids[:40], per_query=True)
        s2 = g2.rank_stats(Q, ids[:40], per_query=True)
        g1.close(); g2.close()
        assert np.array_equal(i1, i2)
        assert np.abs(d1 - d2).max() <= 1e-6
        assert np.array_equal(s1["best_rank"], s2["best_rank"])
    e.close()


# ---------------------------------------------------------------------------------------------- facade
def _write_features(path, X):
    with open(path, "w") as f:
        f.write("#features\n")
        for row in X:
            f.write("".join("%.6g," % v for v in row) + "\n")     # what operator<<(float) prints (extract_features.cpp)


def _read_features(path):
    return np.array([[float(x) for x in ln.rstrip(",\n").split(",")] for ln in open(path) if not ln.startswith("#")], np.float32)


def test_rank_stats_tool_and_stats_output_file(tmp_path):
    c = case("A")
    G, gid, Q, qid = c["G"][:20000], c["gid"][:20000], c["Q"][:64], c["qid"][:64]
    _write_features(tmp_path / "ref.txt", G)
    _write_features(tmp_path / "qry.txt", Q)
    np.savetxt(tmp_path / "ref_ids.txt", gid, fmt="%d")
    np.savetxt(tmp_path / "qry_ids.txt", qid, fmt="%d")
    r = subprocess.run([os.path.join(ROOT, "caffe_facade", "build", "rank_stats"), str(tmp_path / "ref.txt"),
                        str(tmp_path / "ref_ids.txt"), str(tmp_path / "qry.txt"), str(tmp_path / "qry_ids.txt"),
                        str(tmp_path / "stats.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict((ln.split(" = ")[0], float(ln.split(" = ")[1])) for ln in r.stdout.strip().split("\n") if " = " in ln)
    Gt, Qt = _read_features(tmp_path / "ref.txt"), _read_features(tmp_path / "qry.txt")
    d64 = ref.distances(Qt, Gt)
    eps = 4.0 * float(np.abs(ref.distances(Qt, Gt, np.float32).astype(np.float64) - d64).max())
    summary, best, ap, order = ref.rank_stats(d64, qid, gid)
    print(got, summary)
    assert list(got) == ["median_rank", "recall_at_1", "recall_at_5", "recall_at_10", "mean_ap"]
    assert got["median_rank"] == summary["median_rank"]
    for a, b in (("recall_at_1", "recall_1"), ("recall_at_5", "recall_5"), ("recall_at_10", "recall_10"), ("mean_ap", "mean_ap")):
        assert abs(got[a] - summary[b]) <= 1e-4, (a, got[a], summary[b])
    lines = (tmp_path / "stats.txt").read_text().strip().split("\n")
    assert lines[0] == "#item_id,rank,rec@1,rec@5,ret_id_1,ret_id_2,ret_id_3,ret_id_4,ret_id_5"        # :124-126
    assert len(lines) == 65
    for i, ln in enumerate(lines[1:]):
        f = ln.split(",")
        assert len(f) == 15
        ids5 = order[i, :5]
        _, r1, r5, _, _ = ref.ap_stats(gid[order[i]], qid[i])
        assert [int(f[0]), int(f[1]), int(f[2])] == [i, int(qid[i]), int(best[i])]
        assert float(f[3]) == float("%g" % r1) and float(f[4]) == float("%g" % r5)
        got5 = [int(x) for x in f[5:10]]
        if got5 != ids5.tolist():                                  # only as near ties
            assert np.abs(d64[i, got5] - d64[i, ids5]).max() <= eps
        for x, j in zip(f[10:15], got5):                           # distances as operator<<(float) prints them: 6 significant digits
            assert abs(float(x) - d64[i, j]) <= 5.1e-6 * max(1.0, abs(d64[i, j])) + eps
