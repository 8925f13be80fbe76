"""GPU tests of the kmeans tool: the feature file becomes a gallery, vv_gallery_kmeans runs on the device, and the tool's centroid file,
assignment file and printed lines are those the binding (Gallery.kmeans) gives on the same features -- values written with nine
digits read back as themselves, objectives are printed with seventeen.  A bad metric or a missing output exits 2."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "caffe_facade", "build", "kmeans")


def write_features(path, X):
    with open(path, "w") as f:
        f.write("#features\n")
        for row in X:
            f.write("".join("%.9g," % v for v in row) + "\n")


def read_features(path):
    rows = [ln for ln in open(path).read().splitlines() if ln and not ln.startswith("#")]
    return np.array([[np.float32(v) for v in ln.rstrip(",").split(",")] for ln in rows], np.float32)


def run(args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmeans")
    rng = np.random.default_rng(19)
    member = rng.integers(0, 4, 700)
    X = (4.0 * rng.choice([-1, 1], (4, 12))[member] + rng.standard_normal((700, 12))).astype(np.float32)
    write_features(d / "features.txt", X)
    return d, X


def expected_lines(r):
    lines = ["pass %d objective = %.17g moved = %d" % (t, o, m) for t, (o, m) in enumerate(zip(r.objective, r.moved))]
    rep = r.report
    return lines + ["empty = %d degenerate = %d nonfinite_rows = %d" % (rep["empty_last"], rep["degenerate_last"], rep["nonfinite_rows"])]


@pytest.mark.parametrize("metric", ["euclidean", "spherical"])
def test_tool_matches_the_binding(case, metric):
    d, X = case
    out = run([d / "features.txt", 5, "--iters", 4, "--metric", metric, "--seed", 3, "--out_centroids", d / "c.txt", "--out_assign", d / "a.txt"])
    assert out.returncode == 0, out.stderr
    eng = vv.Engine(0, "f16")
    try:
        g = eng.gallery(X)
        r = g.kmeans(5, iters=4, metric=metric, seed=3)
        g.close()
    finally:
        eng.close()
    assert out.stdout.splitlines() == expected_lines(r)
    cent = read_features(d / "c.txt")
    assert cent.shape == r.centroids.shape and np.array_equal(cent.view(np.uint32), r.centroids.view(np.uint32))
    assert np.array_equal(np.loadtxt(d / "a.txt", dtype=np.int32), r.assign)


def test_tool_starts_from_a_centroid_file(case):
    d, X = case
    write_features(d / "init.txt", X[[5, 50, 500]])
    out = run([d / "features.txt", 3, "--iters", 2, "--init", d / "init.txt", "--out_centroids", d / "c3.txt", "--out_assign", d / "a3.txt"])
    assert out.returncode == 0, out.stderr
    eng = vv.Engine(0, "f16")
    try:
        g = eng.gallery(X)
        r = g.kmeans(3, iters=2, init=X[[5, 50, 500]])
        g.close()
    finally:
        eng.close()
    assert out.stdout.splitlines() == expected_lines(r)
    assert np.array_equal(read_features(d / "c3.txt").view(np.uint32), r.centroids.view(np.uint32))
    assert np.array_equal(np.loadtxt(d / "a3.txt", dtype=np.int32), r.assign)


def test_usage_errors(case):
    d, _ = case
    for args in ([], [d / "features.txt", 3, "--out_centroids", d / "x.txt"],
                 [d / "features.txt", 3, "--metric", "cosine", "--out_centroids", d / "x.txt", "--out_assign", d / "y.txt"],
                 [d / "features.txt", 3, "--seed", 1, "--init", d / "features.txt", "--out_centroids", d / "x.txt", "--out_assign", d / "y.txt"]):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "", (args, out.stderr)
    assert not os.path.exists(d / "x.txt") and not os.path.exists(d / "y.txt")
