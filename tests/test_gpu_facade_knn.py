"""GPU tests of the classification_stats tool's --knn mode: the training items become a gallery, the class votes of every test item's K
nearest training items are counted on the device, and the tool prints the statistics the binding path (Gallery.knn_scores ->
Engine.classification_stats) gives for the same data, formatted with %.9g, behind one `kNN:` line.  A bad weighting exits 2."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "caffe_facade", "build", "classification_stats")


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.close()


def write_features(path, X):
    with open(path, "w") as f:
        f.write("#features\n")
        for row in X:
            f.write("".join("%.9g," % v for v in row) + "\n")          # nine digits: every fp32 value reads back as itself


def write_labels(path, labels):
    with open(path, "w") as f:
        f.write("".join("%d\n" % v for v in labels))


def expected_lines(acc, ap, rep):
    lines = ["accuracy_c%d = %.9g" % (k, v) for k, v in enumerate(acc)] + ["ap_c%d = %.9g" % (k, v) for k, v in enumerate(ap)]
    return lines + ["total_accuracy = %.9g" % rep["total_accuracy"], "mean_ap = %.9g" % rep["mean_ap"]]


def run(args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("knn")
    rng = np.random.default_rng(12)
    Cn, dim = 4, 20
    centres = 3 * rng.choice([-1, 1], (Cn, dim))
    tr_lab = rng.permutation(np.repeat(np.arange(Cn), 15)).astype(np.int32)
    train = (centres[tr_lab] + rng.standard_normal((60, dim))).astype(np.float32)
    te_lab = rng.integers(0, Cn, 150).astype(np.int32)
    test = (centres[te_lab] + 2 * rng.standard_normal((150, dim))).astype(np.float32)
    te_lab[::13] = (te_lab[::13] + 1) % Cn
    write_features(d / "train.txt", train)
    write_labels(d / "train_labels.txt", tr_lab)
    write_features(d / "test.txt", test)
    write_labels(d / "test_labels.txt", te_lab)
    return d, train, tr_lab, test, te_lab, Cn


def binding(eng, case, **kw):
    _, train, tr_lab, test, te_lab, Cn = case
    g = eng.gallery(train)
    try:
        buf = g.knn_scores(test, tr_lab, Cn, 5, **kw)
        acc, ap, _, rep = eng.classification_stats(buf, te_lab, Cn)
        buf.free()
    finally:
        g.close()
    return acc, ap, rep


def test_knn_run_prints_the_bindings_values(eng, case):
    d = case[0]
    acc, ap, rep = binding(eng, case)
    r = run([d / "test.txt", d / "test_labels.txt", "--knn", 5, d / "train.txt", d / "train_labels.txt"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["kNN: k = 5 weighting = uniform form = 1"] + expected_lines(acc, ap, rep)
    assert 0.5 < rep["total_accuracy"] < 1.0
    r2 = run([d / "test.txt", d / "test_labels.txt", "--knn", 5, d / "train.txt", d / "train_labels.txt", "--knn_weighting", "uniform"])
    assert r2.returncode == 0 and r2.stdout == r.stdout


def test_exp_weighting_prints_the_bindings_values(eng, case):
    d = case[0]
    acc, ap, rep = binding(eng, case, weighting="exp", temperature=0.5)
    r = run([d / "test.txt", d / "test_labels.txt", "--knn", 5, d / "train.txt", d / "train_labels.txt", "--knn_weighting", "exp",
             "--knn_temperature", 0.5])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["kNN: k = 5 weighting = exp form = 1"] + expected_lines(acc, ap, rep)


@pytest.mark.parametrize("flags", [["--knn_weighting", "gaussian"], ["--knn_temperature", "0"], ["--knn_temperature", "nan"]])
def test_a_bad_value_prints_the_usage(case, flags):
    d = case[0]
    r = run([d / "test.txt", d / "test_labels.txt", "--knn", 5, d / "train.txt", d / "train_labels.txt"] + flags)
    assert r.returncode == 2 and r.stderr.startswith("usage:") and "--knn K" in r.stderr and r.stdout == ""


def test_a_bad_k_prints_the_usage(case):
    d = case[0]
    for k in ("0", "2049", "five"):
        r = run([d / "test.txt", d / "test_labels.txt", "--knn", k, d / "train.txt", d / "train_labels.txt"])
        assert r.returncode == 2 and r.stderr.startswith("usage:") and r.stdout == ""
