"""CPU tests of the classification statistics: the numpy restatement the GPU tests compare against (tests/classification_ref.py)
is held against tests/classification_pin.cpp -- the layer's procedure run with the real libstdc++ (n dummies, push_back, std::sort
with std::greater<pair<float, bool>>, the walk over the first n, float accumulation) -- on random cases with forced ties, exact
zeros, -0.0, all-negative columns, absent classes and +-Inf; against the literal float64 form of the same procedure; and against the
hand-checkable case.  Counts and accuracies are integers behind one fp32 division: equal with ==.  The pin's ap is a serial fp32
chain of count_c divisions and additions of terms in (0, 1]: its first-order error bound is (count_c + 1) 2^-24 relative to the
sum, and the final division adds one more half ulp; the test allows that doubled, (count_c + 2) 2^-23 relative.

Also without a GPU: include/videovec.h, the built library's exports and the ctypes binding agree on the two new entry points,
sizeof(vv_classification_report) is what a C probe says, the facade's protobuf stand-in parses classification_stats_param, and the
tool is built."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classification_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402
from videovector_amd import engine as vve   # noqa: E402

NEW_SYMBOLS = ["vv_classification_stats", "vv_gallery_scores"]
CASES = [(1, 1, "random"), (4, 2, "ties"), (63, 3, "ties"), (257, 5, "random"), (300, 4, "structured"), (200, 3, "inf"),
         (129, 2, "one_class"), (500, 7, "ties"), (1000, 3, "structured")]


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pin") / "classification_pin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "classification_pin.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "videovector_amd", "csrc"), "-s", "-j4"], check=True)
    subprocess.run(["make", "-C", os.path.join(ROOT, "caffe_facade"), "-s", "-j4"], check=True)
    return os.path.join(ROOT, "caffe_facade", "build")


def run_pin(exe, scores, labels, tmp_path, threads=1):
    n, Cn = scores.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n, Cn], np.int32).tobytes() + np.ascontiguousarray(scores, np.float32).tobytes() + np.ascontiguousarray(labels, np.int32).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(threads)], check=True)
    raw = (tmp_path / "out.bin").read_bytes()
    count = np.frombuffer(raw, np.int32, Cn, 0)
    acc = np.frombuffer(raw, np.float32, Cn, 4 * Cn)
    ap = np.frombuffer(raw, np.float32, Cn, 8 * Cn)
    total = np.frombuffer(raw, np.float32, 1, 12 * Cn)[0]
    return count, acc, ap, total


def test_hand_checkable_case():
    scores = np.array([[0.5, 0], [0.7, 0], [-0.1, 0], [0.0, 0]], np.float32)
    r = ref.classification_stats(scores, [0, 1, 0, 1], 2)
    assert r["ap64"][0] == 0.25 and r["count"].tolist() == [2, 2]
    # column 1 is all zeros: both positives are visited, ahead of the zero non-positives and the dummies: (1/1 + 2/2) / 2
    assert r["ap64"][1] == 1.0
    # predictions: column 0 for rows 0, 1 and 3 (row 3: the first of two equal maxima), column 1 for row 2
    assert r["correct"].tolist() == [1, 0] and r["accuracy"].tolist() == [0.5, 0.0] and r["total_accuracy"] == np.float32(0.25)
    assert np.array_equal(ref.by_sorting(scores, [0, 1, 0, 1], 2), r["ap64"])


def test_negative_zero_is_visited_and_negative_is_not():
    scores = np.array([[-0.0], [0.0], [-1e-30], [1.0]], np.float32)
    lab = [0, 0, 0, 0]
    r = ref.classification_stats(scores, lab, 1)
    # 1.0: 1/1; -0.0 and 0.0 tie, item order: 2/2, 3/3; the negative one is never reached; divisor 4
    assert r["ap64"][0] == 3 / 4
    assert np.array_equal(ref.by_sorting(scores, lab, 1), r["ap64"])


@pytest.mark.parametrize("n,Cn,kind", CASES)
def test_restatement_against_the_pin_and_the_literal_form(pin, tmp_path, n, Cn, kind):
    rng = np.random.default_rng(1000 * n + Cn)
    scores, labels = ref.make_case(rng, n, Cn, kind)
    r = ref.classification_stats(scores, labels, Cn)
    count, acc, ap, total = run_pin(pin, scores, labels, tmp_path)
    assert np.array_equal(count, r["count"])
    assert np.array_equal(acc, r["accuracy"]) and total == r["total_accuracy"]
    lit = ref.by_sorting(scores, labels, Cn)
    err = np.abs(lit - r["ap64"])
    print("counting form vs literal float64 form: max abs", err.max())
    assert (err <= 1e-12).all()
    bound = (r["count"] + 2) * 2.0 ** -23 * np.abs(ap.astype(np.float64))
    d = np.abs(r["ap64"] - ap.astype(np.float64))
    print("restatement vs pin: max abs", d.max(), "bound", bound.max())
    assert (d <= bound).all(), (d, bound)
    if kind == "structured":
        assert r["ap64"][0] == 0.0 and r["count"][0] > 0 and ap[0] == 0.0


def test_pin_threads_do_not_change_its_output(pin, tmp_path):
    rng = np.random.default_rng(5)
    scores, labels = ref.make_case(rng, 400, 6, "ties")
    a = run_pin(pin, scores, labels, tmp_path, 1)
    b = run_pin(pin, scores, labels, tmp_path, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_header_binding_and_exports_agree(built):
    hdr = open(os.path.join(ROOT, "include", "videovec.h")).read()
    assert "classification_stats_layer.cpp:13-95" in hdr and "2^24" in hdr
    nocomment = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", nocomment))
    out = subprocess.run(["nm", "-D", "--defined-only", vv.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[-1].startswith("vv_")}
    assert set(NEW_SYMBOLS) <= declared and exported == declared, (sorted(exported - declared), sorted(declared - exported))
    L = vv.load_library()
    assert len(L.vv_classification_stats.argtypes) == 10 and len(L.vv_gallery_scores.argtypes) == 5
    assert hasattr(vv.Engine, "classification_stats") and hasattr(vv.Gallery, "scores")


def test_report_struct_matches_a_c_probe(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "videovec.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(vv_classification_report), offsetof(vv_classification_report, mean_ap), '
                   'offsetof(vv_classification_report, classes_present), offsetof(vv_classification_report, n)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_map, o_cls, o_n = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    R = vve._ClassificationReport
    assert (size, o_map, o_cls, o_n) == (C.sizeof(R), R.mean_ap.offset, R.classes_present.offset, R.n.offset) == (24, 4, 8, 16)


def test_proto_parses_the_layer_parameter(built, tmp_path):
    net = tmp_path / "net.prototxt"
    net.write_text('name: "cls"\nlayers {\n  name: "cls" type: CLASSIFICATION_STATS\n  bottom: "scores" bottom: "label"\n'
                   '  top: "acc" top: "ap" top: "total"\n  classification_stats_param { num_classes: 300 }\n}\n')
    tool = os.path.join(built, "proto_tool")
    subprocess.run([tool, "text2bin", "NetParameter", str(net), str(tmp_path / "net.bin")], check=True)
    subprocess.run([tool, "bin2text", "NetParameter", str(tmp_path / "net.bin"), str(tmp_path / "back.prototxt")], check=True)
    assert re.search(r"classification_stats_param\s*{\s*num_classes:\s*300\s*}", (tmp_path / "back.prototxt").read_text())
    # field 42 of LayerParameter (tag 42 << 3 | 2 = 0xd2 0x02), inside it field 1, varint 300
    assert b"\xd2\x02\x03\x08\xac\x02" in (tmp_path / "net.bin").read_bytes()
    bad = tmp_path / "bad.prototxt"
    bad.write_text(net.read_text().replace("num_classes: 300", "no_such_field: 1"))
    r = subprocess.run([tool, "text2bin", "NetParameter", str(bad), str(tmp_path / "bad.bin")], capture_output=True)
    assert b"ClassificationStatsParameter" in r.stderr      # parsed field by field, no longer opaque


def test_tool_is_built(built):
    assert os.access(os.path.join(built, "classification_stats"), os.X_OK)
