"""CPU tests of the k-NN classifier's plumbing: the header declares vv_gallery_knn_scores / vv_gallery_knn_scores_self and the two
weighting constants, the binding declares both, Gallery has the two methods, the built library exports them, and the
classification_stats tool's usage names --knn."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import videovector_amd as vv   # noqa: E402

NEW_SYMBOLS = ["vv_gallery_knn_scores", "vv_gallery_knn_scores_self"]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "videovector_amd", "csrc"), "-s", "-j4"], check=True)
    subprocess.run(["make", "-C", os.path.join(ROOT, "caffe_facade"), "-s", "-j4"], check=True)


def header():
    return open(os.path.join(ROOT, "include", "videovec.h")).read()


def test_header_declares_the_functions_and_the_constants():
    hdr = header()
    assert re.search(r"^#define VV_KNN_UNIFORM 0$", hdr, re.M) and re.search(r"^#define VV_KNN_EXP 1$", hdr, re.M)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", code))
    assert set(NEW_SYMBOLS) <= declared
    assert "HAS NO REFERENCE COUNTERPART" in hdr[hdr.index("k-nearest-neighbour classifier"):hdr.index("#define VV_KNN_UNIFORM")]


def test_binding_declares_the_new_symbols():
    L = vv.load_library()
    assert len(L.vv_gallery_knn_scores.argtypes) == 12 and len(L.vv_gallery_knn_scores_self.argtypes) == 10
    for m in ("knn_scores", "knn_scores_self"):
        assert callable(getattr(vv.Gallery, m))


def test_library_exports_the_new_entry_points(built):
    out = subprocess.run(["nm", "-D", "--defined-only", vv.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    assert set(NEW_SYMBOLS) <= exported


def test_tool_usage_names_knn(built):
    r = subprocess.run([os.path.join(ROOT, "caffe_facade", "build", "classification_stats")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == ""
    assert "--knn K train_features.txt train_labels.txt [--knn_weighting uniform|exp] [--knn_temperature T]" in r.stderr
