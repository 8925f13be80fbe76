"""The classification_stats tool's row-list flags: --shuffle SEED --epochs E trains on vv_rows_shuffled's list and, with --dump_rows,
prints statistics equal to the binding's when the binding fits on the dumped list; --folds K --weight_decay a,b,c prints the fold means
Linear.cross_validate computes and chooses what it chooses; without the new flags the tool's output is the wording it had before they
existed (the strings tests/test_gpu_facade_linear.py expects, restated here)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import videovector_amd as vv   # noqa: E402

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "caffe_facade", "build", "classification_stats")
HP = dict(iters=30, batch=16, lr=0.05, momentum=0.5)
FLAGS = ["--iters", 30, "--batch", 16, "--lr", 0.05, "--momentum", 0.5]


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


def fit_line(fit):
    return "Linear fit: steps = %d loss = %.9g -> %.9g" % (fit["steps"], fit["loss_first"], fit["loss_last"])


def run(args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Training items in class order (as extract_features writes a gallery, video by video), noisy test items."""
    tmp = tmp_path_factory.mktemp("rows")
    rng = np.random.default_rng(11)
    Cn, dim = 4, 20
    centres = 3 * rng.choice([-1, 1], (Cn, dim))
    tr_lab = np.repeat(np.arange(Cn), 15).astype(np.int32)
    train = (centres[tr_lab] + 1.5 * rng.standard_normal((60, dim))).astype(np.float32)
    te_lab = rng.integers(0, Cn, 150).astype(np.int32)
    test = (centres[te_lab] + 2 * rng.standard_normal((150, dim))).astype(np.float32)
    te_lab[::13] = (te_lab[::13] + 1) % Cn
    write_features(tmp / "train.txt", train)
    write_labels(tmp / "train_labels.txt", tr_lab)
    write_features(tmp / "test.txt", test)
    write_labels(tmp / "test_labels.txt", te_lab)
    return dict(tmp=tmp, Cn=Cn, dim=dim, train=train, tr_lab=tr_lab, test=test, te_lab=te_lab,
                files=[tmp / "test.txt", tmp / "test_labels.txt"], trainf=[tmp / "train.txt", tmp / "train_labels.txt"])


def read_dump(path):
    """{name: [indices]} of a --dump_rows file, in file order."""
    out, name = {}, None
    for line in open(path).read().splitlines():
        if line.startswith("#"):
            name = line[1:].strip()
            out[name] = []
        else:
            out[name].append(int(line))
    return out


def test_shuffled_epochs_equal_the_binding_on_the_dumped_list(case):
    dump = case["tmp"] / "rows.txt"
    r = run(case["files"] + ["--linear"] + case["trainf"] + FLAGS + ["--weight_decay", 0.001, "--shuffle", 7, "--epochs", 2, "--dump_rows", dump])
    assert r.returncode == 0, r.stderr
    lists = read_dump(dump)
    assert list(lists) == ["shuffled"]
    rows = np.array(lists["shuffled"], np.int32)
    assert rows.tolist() == vv.rows_shuffled(7, 60, 2).tolist()
    eng = vv.Engine(0, "f16")
    try:
        items = eng.gallery(case["train"], case["tr_lab"])
        lin = eng.linear(case["dim"], case["Cn"])
        _, fit = lin.fit(items, case["tr_lab"], rows=rows, weight_decay=0.001, **HP)
        acc, ap, _, rep = eng.classification_stats(lin.scores(case["test"]), case["te_lab"], case["Cn"])
        plain = eng.linear(case["dim"], case["Cn"])
        _, plain_fit = plain.fit(items, case["tr_lab"], weight_decay=0.001, **HP)
    finally:
        eng.close()
    out = r.stdout.splitlines()
    assert out[0] == fit_line(fit) and out[1:] == expected_lines(acc, ap, rep)
    assert fit_line(plain_fit) != out[0]                                  # the order of the items matters: the flag did something


def test_folds_choose_what_cross_validate_chooses(case):
    decays = (0.5, 0.001, 0.05)
    dump = case["tmp"] / "folds.txt"
    r = run(case["files"] + ["--linear"] + case["trainf"] + FLAGS + ["--loss", "hinge", "--folds", 3, "--weight_decay", "0.5,0.001,0.05", "--cv_seed", 5,
                                                                     "--dump_rows", dump])
    assert r.returncode == 0, r.stderr
    eng = vv.Engine(0, "f16")
    try:
        items = eng.gallery(case["train"], case["tr_lab"])
        lin = eng.linear(case["dim"], case["Cn"])
        lin.set_loss("hinge", "L2")
        cv = lin.cross_validate(items, case["tr_lab"], 3, decays, seed=5, **HP)
        lin.put(W=np.zeros((case["Cn"], case["dim"]), np.float32), b=np.zeros(case["Cn"], np.float32), hW=np.zeros((case["Cn"], case["dim"]), np.float32),
                hb=np.zeros(case["Cn"], np.float32), steps=0)
        _, fit = lin.fit(items, case["tr_lab"], weight_decay=cv["best"], **HP)
        acc, ap, _, rep = eng.classification_stats(lin.scores(case["test"]), case["te_lab"], case["Cn"])
    finally:
        eng.close()
    out = r.stdout.splitlines()
    want = ["cv weight_decay = %.9g mean_ap = %.9g total_accuracy = %.9g" % (np.float32(x["weight_decay"]), x["mean_ap_mean"], x["total_accuracy_mean"])
            for x in cv["results"]]
    assert out[:3] == want
    assert out[3] == "cv chosen weight_decay = %.9g" % np.float32(cv["best"])
    assert out[4] == fit_line(fit) and out[5:] == expected_lines(acc, ap, rep)
    lists = read_dump(dump)
    assert list(lists) == [x for f in range(3) for x in ("fold %d train" % f, "fold %d held" % f)]
    for f in range(3):
        train, held = vv.rows_fold(5, 60, 3, f)
        assert lists["fold %d train" % f] == train.tolist() and lists["fold %d held" % f] == held.tolist()


def test_without_the_new_flags_the_output_is_the_parents_wording(case):
    eng = vv.Engine(0, "f16")
    try:
        items = eng.gallery(case["train"], case["tr_lab"])
        lin = eng.linear(case["dim"], case["Cn"])
        _, fit = lin.fit(items, case["tr_lab"], weight_decay=0.001, **HP)
        acc, ap, _, rep = eng.classification_stats(lin.scores(case["test"]), case["te_lab"], case["Cn"])
    finally:
        eng.close()
    r = run(case["files"] + ["--linear"] + case["trainf"] + FLAGS + ["--weight_decay", 0.001])
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[0] == "Linear fit: steps = 30 loss = %.9g -> %.9g" % (fit["loss_first"], fit["loss_last"])
    assert out[1:] == expected_lines(acc, ap, rep)
    # the new flags without what they need, or without --linear: the usage, exit 2
    for bad in (["--shuffle", 3], ["--epochs", 2], ["--folds", 3]):
        r = run(case["files"] + ["--linear"] + case["trainf"] + bad)
        assert r.returncode == 2 and r.stderr.startswith("usage:")
    r = run(case["files"] + ["--prototypes"] + case["trainf"] + ["--shuffle", 3, "--epochs", 1])
    assert r.returncode == 2
