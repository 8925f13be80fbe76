"""GPU tests of the class-level leave-one-out statistics (vv_gallery_pool_by_id, vv_gallery_class_stats, Gallery.class_stats, the
facade's RETRIEVAL_STATS layer with video_level_retrieval / stats_output_file and the class_stats tool) against
tests/class_stats_ref.py, the float64 restatement of the reference's RetrievalStatsLayer.

Tolerances.  Per-query AP: four times the largest |ap32 - ap64| that numpy's own float32 product shows on the same input (the
factor the gallery tests allow between two float32 summation orders); printed with the measured value.  Per-query acc1 / acc5
and top5_idx: equal to float64 except as NEAR TIES -- within eps = four times the largest |d32 - d64| of numpy's float32
product -- for at most 1 % of the scored queries.  mean_ap, hit_at_1, hit_at_5: 1e-4; n_scored exact; pooled rows: 1e-6."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import class_stats_ref as ref   # noqa: E402
from tests.test_class_stats_host import HAND, HAND_IDS, HAND_MAP, HAND_TOP5, HAND_X, INPUTS   # noqa: E402
from tests.test_facade_proto import pb   # noqa: E402,F401  (fixture)

import videovector_amd as vv   # noqa: E402
from videovector_amd.prototxt import train_net   # noqa: E402
from videovector_amd.synth import SyntheticVideos, init_weights, synthetic_windows   # noqa: E402

pytestmark = pytest.mark.gpu
BUILD = os.path.join(ROOT, "caffe_facade", "build")
_cache = {}


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def case(name):
    if name not in _cache:
        _cache[name] = ref.make_input(*INPUTS[name])
    return _cache[name]


def check_against(label, got, X, vid, m, exclude):
    """got = class_stats(..., per_query=True) of items X / vid against float64 with the module's tolerances."""
    vid = np.asarray(vid)
    d64 = ref.distances(X)
    d32 = ref.distances(X, np.float32).astype(np.float64)
    eps = 4.0 * float(np.abs(d32 - d64).max())
    s64, ap64, a1, a5, t5 = ref.class_stats(d64, vid, m, exclude)
    ap32 = ref.class_stats(d32, vid, m, exclude)[1]
    cls = ref.classes_of(vid, m)
    scored = cls >= 0
    ap_np = float(np.abs(ap32 - ap64)[scored].max())
    ap_got = float(np.abs(got["ap"] - ap64)[scored].max())
    print("%s exclude=%s: eps %.3g, largest |ap - ap64| %.3g (numpy float32: %.3g, bound %.3g), summary %s, float64 %s"
          % (label, exclude, eps, ap_got, ap_np, 4 * ap_np, {f: got[f] for f in s64}, s64))
    assert got["n_scored"] == s64["n_scored"]
    for f in ("mean_ap", "hit_at_1", "hit_at_5"):
        assert abs(got[f] - s64[f]) <= 1e-4, (f, got[f], s64[f])
    for f in ("ap", "acc1", "acc5"):
        assert np.isnan(got[f][~scored]).all() and not np.isnan(got[f][scored]).any()
    assert (got["top5_idx"][~scored] == -1).all()
    assert ap_got <= 4 * ap_np + 1e-7                                   # (1e-7: the float32 the per-query value is returned in)
    near = set()
    for i in np.flatnonzero(scored & ((got["acc1"] != a1) | (np.abs(got["acc5"] - a5) > 1e-6))):
        for k, g in ((1, got["acc1"][i]), (5, got["acc5"][i] * 5)):
            lo, hi = ref.acc_interval(d64[i], i, vid, cls, exclude, eps, k)
            assert lo <= round(float(g)) <= hi, (i, k, g, lo, hi)
        near.add(int(i))
    for i in np.flatnonzero(scored & (got["top5_idx"] != t5).any(axis=1)):
        g5, w5 = got["top5_idx"][i], t5[i]
        assert ((g5 >= 0) == (w5 >= 0)).all() and len(set(g5[g5 >= 0])) == (g5 >= 0).sum(), (i, g5, w5)
        assert (vid[g5[g5 >= 0]] != vid[i]).all()
        assert np.abs(d64[i, g5[g5 >= 0]] - d64[i, w5[w5 >= 0]]).max() <= eps, (i, g5, w5)
        near.add(int(i))
    print("%s: queries that use the near-tie exemption: %d of %d" % (label, len(near), int(scored.sum())))
    assert len(near) <= 0.01 * scored.sum()


def test_reference_known_answer(eng):
    """test_retrieval_stats_layer.cpp:34-39, 82-84."""
    X = np.array([[1, 0], [0, 1], [1, .06], [0, 1], [1, .1]], np.float32)
    g = eng.gallery(X, np.array([2, 3, 4, 5, 6], np.int32))
    s = g.class_stats({2: 1, 3: 2, 4: 1, 5: 2, 6: 2})
    g.close()
    assert abs(s["mean_ap"] - 0.7833333) <= 1e-6 and abs(s["hit_at_1"] - 0.60) <= 1e-6 and abs(s["hit_at_5"] - 0.32) <= 1e-6
    assert s["n_scored"] == 5


@pytest.mark.parametrize("exclude", [True, False])
def test_hand_worked_case(eng, exclude):
    """Two equal rows (2 and 3: the tie puts 2 first, so the positive 3 of query 4 has val 3), a query of class -1 (2), an id
    absent from the map (20: class 0), queries whose only class-mate shares their video (0 and 1), a class of one (5)."""
    g = eng.gallery(HAND_X, HAND_IDS)
    s = g.class_stats(HAND_MAP, exclude_same_video=exclude, per_query=True)
    g.close()
    h = HAND[exclude]
    assert np.allclose(s["ap"], np.array(h["ap"], np.float32), atol=1e-7, equal_nan=True), s["ap"]
    assert np.array_equal(s["acc1"], np.array(h["acc1"], np.float32), equal_nan=True), s["acc1"]
    assert np.array_equal(s["acc5"], np.array(h["acc5"], np.float32), equal_nan=True), s["acc5"]
    assert s["top5_idx"].tolist() == HAND_TOP5
    assert s["n_scored"] == 5
    for f in ("mean_ap", "hit_at_1", "hit_at_5"):
        assert abs(s[f] - h[f]) <= 1e-7, (f, s[f], h[f])


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("name", ["A", "B"])
def test_against_float64(eng, name, exclude):
    """Also several query blocks: the block holds at most 512 queries, these inputs have 4096 and 3001."""
    X, vid, m = case(name)
    g = eng.gallery(X, vid)
    got = g.class_stats(m, exclude_same_video=exclude, per_query=True)
    scratch, block, passes = g.scratch_bytes, int(g.get("query_block")), int(g.get("last_passes"))
    g.close()
    print("%s: scratch %d bytes, query block %d, passes %d" % (name, scratch, block, passes))
    assert 0 < scratch <= 1 << 30
    assert block < len(X)
    check_against(name, got, X, vid, m, exclude)


@pytest.mark.parametrize("name", ["A", "B"])
def test_video_level(eng, name):
    X, vid, m = case(name)
    g = eng.gallery(X, vid)
    p = g.pool_by_id()
    assert int(g.get("n_ids")) == len(np.unique(vid)) == p.n_ref
    rows = p.rows()
    got = p.class_stats(m, exclude_same_video=True, per_query=True)
    ids = p.ids
    p.close(); g.close()
    P64, pid = ref.pool_by_id(X, vid)
    assert np.array_equal(ids, pid) and (np.diff(ids) > 0).all()
    print("%s: %d videos, largest |pooled - float64| %.3g" % (name, len(pid), np.abs(rows - P64).max()))
    assert rows.shape == P64.shape and np.abs(rows - P64).max() <= 1e-6
    check_against(name + " video level", got, rows, pid, m, True)


def test_more_class_mates_than_one_pass_holds(eng):
    X, vid, m = ref.make_input(9000, 64, 120, 2, 1.0, 2.0, 13)
    g = eng.gallery(X, vid)
    got = g.class_stats(m, exclude_same_video=True, per_query=True)
    passes, chunk = int(g.get("last_passes")), int(g.get("positive_chunk"))
    g.close()
    cls = ref.classes_of(vid, m)
    most = max(int((cls == c).sum()) for c in set(cls.tolist()) if c >= 0)
    print("largest class %d items, chunk %d, passes %d" % (most, chunk, passes))
    assert most > chunk and passes == -(-most // chunk) and passes > 1
    check_against("two classes", got, X, vid, m, True)


def test_two_calls_are_bit_identical(eng):
    X, vid, m = case("B")
    g = eng.gallery(X, vid)
    a = g.class_stats(m, per_query=True)
    b = g.class_stats(m, per_query=True)
    c = g.class_stats(m, exclude_same_video=False, per_query=True)
    g.close()
    for f in ("ap", "acc1", "acc5", "top5_idx"):
        assert a[f].tobytes() == b[f].tobytes(), f
    for f in ("mean_ap", "hit_at_1", "hit_at_5", "n_scored"):
        assert a[f] == b[f]
    assert a["ap"].tobytes() != c["ap"].tobytes()


def test_gallery_from_table_equals_gallery_of_embeddings():
    ds = SyntheticVideos(seed=1701, n_videos=50)
    F, D = 128, 32
    W, b = init_weights(1, D, F, std=0.02)
    e = vv.Engine(0, "f16")
    e.table_synth(ds.seed, ds.n_rows, F)
    e.params_set(W, b)
    rng = np.random.default_rng(19)
    n = min(900, ds.n_rows)
    rows = rng.integers(0, ds.n_rows, (n, 3)).astype(np.int32)
    coeff = np.array([0.5, 0.25, 0.25], np.float32)
    ids = rng.integers(0, 30, n).astype(np.int32)
    m = {int(v): int(v % 4) - (v == 7) * 5 for v in range(30)}
    g1 = e.gallery(e.embed_mean(rows, coeff, relu=True, l2norm=True), ids)
    g2 = e.gallery_from_table(rows, ids, coeff=coeff, relu=True, l2norm=True)
    outs = []
    for g in (g1, g2):
        p = g.pool_by_id()
        outs.append((g.class_stats(m, per_query=True), p.class_stats(m, per_query=True), p.rows()))
        p.close(); g.close()
    e.close()
    for s1, s2 in ((outs[0][0], outs[1][0]), (outs[0][1], outs[1][1])):
        for f in ("ap", "acc1", "acc5", "top5_idx"):
            assert s1[f].tobytes() == s2[f].tobytes(), f
        assert [s1[f] for f in ("mean_ap", "hit_at_1", "hit_at_5", "n_scored")] == [s2[f] for f in ("mean_ap", "hit_at_1", "hit_at_5", "n_scored")]
    assert outs[0][2].tobytes() == outs[1][2].tobytes()


def test_errors_leave_the_engine_usable(eng):
    X, vid, m = ref.make_input(200, 16, 10, 3, 1.0, 1.0, 14)
    g = eng.gallery(X)                                    # no ids
    with pytest.raises(vv.VVError, match="error 1"):
        g.class_stats(m)
    with pytest.raises(vv.VVError, match="error 1"):
        g.pool_by_id()
    g.close()
    g = eng.gallery(X, vid)
    with pytest.raises(vv.VVError, match="error 1"):
        g.class_stats({})
    with pytest.raises(vv.VVError, match="error 1"):
        g.class_stats({int(v): -1 for v in np.unique(vid)})           # no scored query
    got = g.class_stats(m, per_query=True)
    g.close()
    check_against("after errors", got, X, vid, m, True)


# ---------------------------------------------------------------------------------------------- facade
def _write_features(path, X):
    with open(path, "w") as f:
        f.write("#features\n")
        for row in X:
            f.write("".join("%.6g," % v for v in row) + "\n")     # what operator<<(float) prints (extract_features.cpp)


def _read_features(path):
    return np.array([[float(x) for x in ln.rstrip(",\n").split(",")] for ln in open(path) if not ln.startswith("#")], np.float32)


def _tool(args, timeout=600):
    r = subprocess.run([os.path.join(BUILD, "class_stats")] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return [float(ln.split(" = ")[1]) for ln in r.stdout.strip().split("\n") if " = " in ln], r.stdout


def _tool_files(tmp_path, n=1500):
    X, vid, m = case("B")
    X, vid = X[:n], vid[:n]
    _write_features(tmp_path / "feat.txt", X)
    np.savetxt(tmp_path / "ids.txt", vid, fmt="%d")
    (tmp_path / "map.txt").write_text("".join("%d,%d\n" % kv for kv in m.items()))
    return _read_features(tmp_path / "feat.txt"), vid, m


@pytest.mark.parametrize("exclude", [True, False])
def test_class_stats_tool_and_stats_output_file(eng, tmp_path, exclude):
    Xt, vid, m = _tool_files(tmp_path)
    tops, out = _tool([tmp_path / "feat.txt", tmp_path / "ids.txt", tmp_path / "map.txt", tmp_path / "stats.txt"]
                      + ([] if exclude else ["--include_same_video"]))
    assert [ln.split(" = ")[0] for ln in out.strip().split("\n")] == ["test_map", "test_hit_at_1", "test_hit_at_5"]
    g = eng.gallery(Xt, vid)
    s = g.class_stats(m, exclude_same_video=exclude, per_query=True)
    g.close()
    assert [np.float32(t) for t in tops] == [np.float32(s[f]) for f in ("mean_ap", "hit_at_1", "hit_at_5")]
    lines = (tmp_path / "stats.txt").read_text().strip().split("\n")
    assert lines[0] == ("#video_id,class_id,ap,acc@1,acc@5,ret_id_1,ret_id_2,ret_id_3,ret_id_4,ret_id_5"
                        ",class_id_1,class_id_2,class_id_3,class_id_4,class_id_5")                  # :151-153
    cls = ref.classes_of(vid, m)
    scored = np.flatnonzero(cls >= 0)
    assert len(lines) == 1 + len(scored)
    for ln, i in zip(lines[1:], scored):
        f = ln.split(",")
        assert len(f) == 15
        assert [int(f[0]), int(f[1])] == [int(vid[i]), int(cls[i])]
        for x, v in zip(f[2:5], (s["ap"][i], s["acc1"][i], s["acc5"][i])):                          # operator<<(double): 6 digits
            assert float(x) == float("%g" % v), (i, x, v)
        t5 = [int(x) for x in f[5:10]]
        assert t5 == s["top5_idx"][i].tolist()
        assert [int(x) for x in f[10:15]] == [int(cls[j]) if j >= 0 else -1 for j in t5]


def test_class_stats_tool_video_level(eng, tmp_path):
    Xt, vid, m = _tool_files(tmp_path)
    tops, _ = _tool([tmp_path / "feat.txt", tmp_path / "ids.txt", tmp_path / "map.txt", "--video_level", tmp_path / "stats.txt"])
    g = eng.gallery(Xt, vid)
    p = g.pool_by_id()
    s = p.class_stats(m, per_query=True)
    ids = p.ids
    p.close(); g.close()
    assert [np.float32(t) for t in tops] == [np.float32(s[f]) for f in ("mean_ap", "hit_at_1", "hit_at_5")]
    lines = (tmp_path / "stats.txt").read_text().strip().split("\n")
    cls = ref.classes_of(ids, m)
    scored = np.flatnonzero(cls >= 0)
    assert lines[0].startswith("#video_id,class_id,ap,acc@1,acc@5,ret_id_1") and len(lines) == 1 + len(scored)
    for ln, i in zip(lines[1:], scored):
        f = ln.split(",")
        assert len(f) == 5 and [int(f[0]), int(f[1])] == [int(ids[i]), int(cls[i])]                 # :333-336
        for x, v in zip(f[2:5], (s["ap"][i], s["acc1"][i], s["acc5"][i])):
            assert float(x) == float("%g" % v)


@pytest.mark.parametrize("exclude", [True, False])
def test_layer_without_the_new_parameters_is_unchanged(eng, tmp_path, exclude):
    """The layer with neither video_level_retrieval nor stats_output_file makes the call it made before: its tops are those of
    Engine.retrieval_stats (vv_retrieval_stats) on the same features, bit for bit."""
    Xt, vid, m = _tool_files(tmp_path, 700)
    tops, _ = _tool([tmp_path / "feat.txt", tmp_path / "ids.txt", tmp_path / "map.txt", "--within_batch"]
                    + ([] if exclude else ["--include_same_video"]))
    want = eng.retrieval_stats(Xt, vid, m, exclude)
    assert [np.float32(t).tobytes() for t in tops] == [np.float32(w).tobytes() for w in want]


def _caffe_test(net_p, model, log, env):
    r = subprocess.run([os.path.join(BUILD, "caffe"), "test", "--model=%s" % net_p, "--weights=%s" % model, "--iterations=1",
                        "--log_file=%s" % log], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    text = open(log).read() if os.path.exists(log) else ""
    return r, text


def test_facade_video_level_under_both_executors(pb, tmp_path):   # noqa: F811
    from tests.test_gpu_facade import write_caffemodel
    B, C, Nn, F, D, V, NW = 16, 5, 3, 128, 64, 60, 90
    ds = SyntheticVideos(seed=9, n_videos=V)
    cls = {int(v): int(v % 5) + 1 for v in range(V)}
    (tmp_path / "id2class.txt").write_text("".join("%d,%d\n" % kv for kv in cls.items()))
    src = "synthetic://videos=%d;seed=9;features=%d" % (V, F)
    wsrc = "synthetic-windows://videos=%d;seed=9;features=%d;windows=%d;context=4;wseed=5" % (V, F, NW)
    _, vids = synthetic_windows(ds, NW, 4, 5)
    nvid = len(np.unique(vids))
    base = train_net(src, B, C, Nn, D, max_buffer=300, w_std=0.02, test_source=wsrc, test_batch=NW, test_frames=4,
                     id_to_class_file=str(tmp_path / "id2class.txt"))
    key = 'id_to_class_file: "%s"\n' % (tmp_path / "id2class.txt")
    assert base.count(key) == 1
    W0, b0 = init_weights(4, D, F, std=0.02)
    write_caffemodel(pb, str(tmp_path / "init.caffemodel"), W0, b0)
    tops = {}
    for name, env in (("fused", {}), ("seq", {"VV_FACADE_SEQUENTIAL": "1"})):
        stats = tmp_path / ("stats_%s.txt" % name)
        net_p = tmp_path / ("net_%s.prototxt" % name)
        net_p.write_text(base.replace(key, key + '    video_level_retrieval: true\n    max_num_videos: %d\n    stats_output_file: "%s"\n'
                                      % (nvid, stats)))
        r, log = _caffe_test(net_p, tmp_path / "init.caffemodel", str(tmp_path / (name + ".log")), env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert ("Fused videovec TEST plan" in log) == (name == "fused")
        tops[name] = [re.findall(r"Batch 0, %s = ([0-9.eE+-]+)" % t, log)[0] for t in ("test_map", "test_hit_at_1", "test_hit_at_5")]
        lines = stats.read_text().strip().split("\n")
        assert lines[0].startswith("#video_id,class_id,ap,acc@1,acc@5") and len(lines) == 1 + nvid
        assert [int(ln.split(",")[0]) for ln in lines[1:]] == sorted(set(int(v) for v in vids))
        assert all(len(ln.split(",")) == 5 for ln in lines[1:])
    assert tops["fused"] == tops["seq"], tops
    assert 0 < float(tops["fused"][0]) <= 1
    # the reference's CHECK_EQ(num_shots_per_video.size(), max_num_videos_) (:187)
    bad = tmp_path / "bad.prototxt"
    bad.write_text(base.replace(key, key + "    video_level_retrieval: true\n    max_num_videos: %d\n" % (nvid + 1)))
    r, log = _caffe_test(bad, tmp_path / "init.caffemodel", str(tmp_path / "bad.log"), {})
    assert r.returncode != 0
    assert re.search(r"Check failed: .*max_num_videos_.*\(%d vs\. %d\)" % (nvid, nvid + 1), r.stderr + log)
