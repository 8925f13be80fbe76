"""The classification_stats tool's --linear mode under --loss hinge: for both norms its `Linear fit:` line and its statistics are the
binding's fit -> scores -> classification_stats on the same files, equal as printed (%.9g).  Without the flags, and with --loss softmax,
it prints the binding's softmax path: what it printed before the flags existed.  A bad --loss or --hinge_norm prints the usage and exits
non-zero."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "caffe_facade", "build", "classification_stats")
FIT = dict(iters=30, batch=16, lr=0.05, momentum=0.5, weight_decay=0.001)
FIT_FLAGS = ["--iters", 30, "--batch", 16, "--lr", 0.05, "--momentum", 0.5, "--weight_decay", 0.001]


def write_features(path, X):
    with open(path, "w") as f:
        f.write("#features\n")
        for row in X:
            f.write("".join("%.9g," % v for v in row) + "\n")          # nine digits: every fp32 value reads back as itself


def write_labels(path, labels):
    with open(path, "w") as f:
        f.write("".join("%d\n" % v for v in labels))


def expected_lines(fit, acc, ap, rep):
    lines = ["Linear fit: steps = 30 loss = %.9g -> %.9g" % (fit["loss_first"], fit["loss_last"])]
    lines += ["accuracy_c%d = %.9g" % (k, v) for k, v in enumerate(acc)] + ["ap_c%d = %.9g" % (k, v) for k, v in enumerate(ap)]
    return lines + ["total_accuracy = %.9g" % rep["total_accuracy"], "mean_ap = %.9g" % rep["mean_ap"]]


def run(args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("hinge_tool")
    rng = np.random.default_rng(11)
    Cn, dim = 4, 20
    centres = 3 * rng.choice([-1, 1], (Cn, dim))
    tr_lab = rng.permutation(np.repeat(np.arange(Cn), 10)).astype(np.int32)
    train = (centres[tr_lab] + rng.standard_normal((40, dim))).astype(np.float32)
    te_lab = rng.integers(0, Cn, 150).astype(np.int32)
    test = (centres[te_lab] + 2 * rng.standard_normal((150, dim))).astype(np.float32)
    te_lab[::13] = (te_lab[::13] + 1) % Cn
    write_features(d / "train.txt", train)
    write_labels(d / "train_labels.txt", tr_lab)
    write_features(d / "test.txt", test)
    write_labels(d / "test_labels.txt", te_lab)
    want = {}
    eng = vv.Engine(0, "f16")
    try:
        items = eng.gallery(train, tr_lab)
        for key, kw in (("softmax", {}), ("L1", dict(loss="hinge", norm="L1")), ("L2", dict(loss="hinge", norm="L2"))):
            lin = eng.linear(dim, Cn)
            _, fit = lin.fit(items, tr_lab, **dict(FIT, **kw))
            acc, ap, _, rep = eng.classification_stats(lin.scores(test), te_lab, Cn)
            want[key] = expected_lines(fit, acc, ap, rep)
            assert fit["loss_last"] < fit["loss_first"] and rep["total_accuracy"] > 0.5
            lin.close()
    finally:
        eng.close()
    files = [d / "test.txt", d / "test_labels.txt", "--linear", d / "train.txt", d / "train_labels.txt"] + FIT_FLAGS
    return files, want


@pytest.mark.parametrize("norm", ["L1", "L2"])
def test_hinge_prints_the_bindings_numbers(case, norm):
    files, want = case
    r = run(files + ["--loss", "hinge", "--hinge_norm", norm])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == want[norm]
    assert want[norm] != want["softmax"] and want["L1"] != want["L2"]


def test_the_default_norm_is_l2_and_the_default_loss_is_softmax(case):
    files, want = case
    r = run(files + ["--loss", "hinge"])
    assert r.returncode == 0 and r.stdout.splitlines() == want["L2"]
    plain, named = run(files), run(files + ["--loss", "softmax"])
    assert plain.returncode == 0 and named.returncode == 0
    assert plain.stdout.splitlines() == want["softmax"] and named.stdout == plain.stdout
    assert run(files + ["--hinge_norm", "L1"]).stdout == plain.stdout      # the norm is read under hinge only


@pytest.mark.parametrize("flags", [["--loss", "logistic"], ["--loss", "hinge", "--hinge_norm", "L3"], ["--loss", "Hinge"]])
def test_a_bad_value_prints_the_usage(case, flags):
    files, _ = case
    r = run(files + flags)
    assert r.returncode != 0 and "usage: classification_stats" in r.stderr and "--loss softmax|hinge" in r.stderr and r.stdout == ""
