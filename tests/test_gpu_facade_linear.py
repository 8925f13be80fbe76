"""The classification_stats tool's --linear mode: a softmax linear classifier trained on one feature file and scored on another,
everything on the device.  Its `total_accuracy` / `ap_c<k>` lines are the binding's numbers for the same configuration formatted with
%.9g, its `Linear fit:` line the fit's report; the --prototypes output on the same files still equals the binding's
nearest-class-mean path line for line (what the tool printed before --linear existed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "caffe_facade", "build", "classification_stats")


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


def test_linear_and_prototypes_modes(tmp_path):
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
    files = [tmp_path / "test.txt", tmp_path / "test_labels.txt"]
    trainf = [tmp_path / "train.txt", tmp_path / "train_labels.txt"]
    eng = vv.Engine(0, "f16")
    try:
        items = eng.gallery(train, tr_lab)
        lin = eng.linear(dim, Cn)
        trace, fit = lin.fit(items, tr_lab, iters=30, batch=16, lr=0.05, momentum=0.5, weight_decay=0.001)
        buf = lin.scores(test)
        acc, ap, _, rep = eng.classification_stats(buf, te_lab, Cn)
        protos = items.pool_by_id()
        pbuf = protos.scores(test)
        pacc, pap, _, prep = eng.classification_stats(pbuf, te_lab, Cn)
    finally:
        eng.close()
    r = run(files + ["--linear"] + trainf + ["--iters", 30, "--batch", 16, "--lr", 0.05, "--momentum", 0.5, "--weight_decay", 0.001])
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[0] == "Linear fit: steps = 30 loss = %.9g -> %.9g" % (fit["loss_first"], fit["loss_last"])
    assert out[1:] == expected_lines(acc, ap, rep)
    assert fit["loss_last"] < fit["loss_first"] and rep["total_accuracy"] > 0.5
    r = run(files + ["--prototypes"] + trainf)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == expected_lines(pacc, pap, prep)
