"""GPU tests of the facade's CLASSIFICATION_STATS layer through the classification_stats tool: the lines it prints are the binding's
values formatted with %.9g (on a score file and on a --prototypes run, where the scores are made on the device by the gallery
calls); a prototxt that names the layer builds it; each of the layer's three shape CHECKs fires."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classification_ref as ref   # noqa: E402

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
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cls")
    scores, labels = ref.make_case(np.random.default_rng(3), 300, 5, "structured")
    write_features(d / "scores.txt", scores)
    write_labels(d / "labels.txt", labels)
    return d, scores, labels


def test_tool_prints_the_bindings_values(eng, files):
    d, scores, labels = files
    acc, ap, cnt, rep = eng.classification_stats(scores, labels, 5)
    r = run([d / "scores.txt", d / "labels.txt"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == expected_lines(acc, ap, rep)
    assert cnt[4] == 0 and "accuracy_c4 = 0" in r.stdout and "ap_c0 = 0" in r.stdout


def test_prototxt_with_the_layer_builds(eng, files):
    d, scores, labels = files
    net = d / "net.prototxt"
    net.write_text('name: "cls"\nlayers {\n  name: "stats" type: CLASSIFICATION_STATS\n  bottom: "scores" bottom: "label"\n'
                   '  top: "accuracy" top: "ap" top: "total_accuracy"\n  classification_stats_param { num_classes: 5 }\n}\n')
    acc, ap, _, rep = eng.classification_stats(scores, labels, 5)
    r = run([d / "scores.txt", d / "labels.txt", "--prototxt", net])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == expected_lines(acc, ap, rep)
    net.write_text(net.read_text().replace("num_classes: 5", "num_classes: 6"))          # the prototxt's own parameter is what is checked
    r = run([d / "scores.txt", d / "labels.txt", "--prototxt", net])
    assert r.returncode != 0 and "The input score count should be equal to number of classes." in r.stderr


def test_the_three_shape_checks_fire(files):
    d, scores, labels = files
    write_labels(d / "short.txt", labels[:-1])
    r = run([d / "scores.txt", d / "short.txt"])
    assert r.returncode != 0 and "The data and label should have the same number." in r.stderr
    r = run([d / "scores.txt", d / "labels.txt", "--num_classes", 4])
    assert r.returncode != 0 and "The input score count should be equal to number of classes." in r.stderr
    r = run([d / "scores.txt", d / "labels.txt", "--label_channels", 2])
    assert r.returncode != 0 and "bottom[1]->channels()" in r.stderr and "(2 vs. 1)" in r.stderr


def test_prototypes_run_scores_on_the_device(eng, tmp_path):
    rng = np.random.default_rng(11)
    Cn, dim = 4, 20
    centres = 3 * rng.choice([-1, 1], (Cn, dim))
    tr_lab = rng.permutation(np.repeat(np.arange(Cn), 10)).astype(np.int32)
    train = (centres[tr_lab] + rng.standard_normal((40, dim))).astype(np.float32)
    te_lab = rng.integers(0, Cn, 150).astype(np.int32)
    test = (centres[te_lab] + 2 * rng.standard_normal((150, dim))).astype(np.float32)
    te_lab[::13] = (te_lab[::13] + 1) % Cn
    write_features(tmp_path / "train.txt", train)
    write_labels(tmp_path / "train_labels.txt", tr_lab)
    write_features(tmp_path / "test.txt", test)
    write_labels(tmp_path / "test_labels.txt", te_lab)
    items = eng.gallery(train, tr_lab)
    protos = items.pool_by_id()
    try:
        buf = protos.scores(test)
        acc, ap, _, rep = eng.classification_stats(buf, te_lab, Cn)
        buf.free()
    finally:
        protos.close()
        items.close()
    r = run([tmp_path / "test.txt", tmp_path / "test_labels.txt", "--prototypes", tmp_path / "train.txt", tmp_path / "train_labels.txt"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == expected_lines(acc, ap, rep)
    assert 0.5 < rep["total_accuracy"] < 1.0
