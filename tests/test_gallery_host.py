"""CPU tests of the gallery retrieval plumbing: the facade's protobuf stand-in parses RETRIEVAL_RANK_STATS_FIXED_REF with its
parameter message, the ctypes binding declares the new entry points, the built library exports exactly the functions
include/videovec.h declares, and the float64 restatement the GPU tests compare against gives the hand-derived known answer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gallery_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

GALLERY_SYMBOLS = ["vv_gallery_create", "vv_gallery_from_table", "vv_gallery_destroy", "vv_gallery_topk",
                   "vv_gallery_rank_stats", "vv_gallery_get"]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "videovector_amd", "csrc"), "-s", "-j4"], check=True)
    subprocess.run(["make", "-C", os.path.join(ROOT, "caffe_facade"), "-s", "-j4"], check=True)
    return os.path.join(ROOT, "caffe_facade", "build")


def test_reference_restatement_known_answer():
    """Derived by hand from the reference's code.  Query 0: order by (d, g) is g0, g4, g1, g3, g2, g5 with ids 9, 7, 7, 9, 7, 5;
    positives at ranks 2, 3, 5; AP = (1/2 + 2/3 + 3/5) / 3."""
    Q = np.array([[1, 0], [0, 1], [.6, .8], [1, 0]], np.float32)
    qid = np.array([7, 7, 9, 3], np.int32)
    G = np.array([[1, 0], [.8, .6], [0, 1], [.6, .8], [1, 0], [-1, 0]], np.float32)
    gid = np.array([9, 7, 7, 9, 7, 5], np.int32)
    s, best, ap, order = ref.rank_stats(ref.distances(Q, G, np.float32), qid, gid)
    assert order[:, :5].tolist() == [[0, 4, 1, 3, 2], [2, 3, 1, 0, 4], [3, 1, 2, 0, 4], [0, 4, 1, 3, 2]]
    assert best.tolist() == [2, 1, 1, 10000]
    assert np.abs(ap - np.array([0.588889, 0.755556, 0.75, 0])).max() <= 1e-6
    assert s["median_rank"] == 1.5
    for f, v in (("recall_1", 0.5), ("recall_5", 0.75), ("recall_10", 0.75), ("mean_ap", 0.523611)):
        assert abs(s[f] - v) <= 1e-6


def test_proto_parses_the_layer_with_all_parameter_fields(built, tmp_path):
    net = tmp_path / "net.prototxt"
    net.write_text('''name: "rank"
layers {
  name: "stats" type: RETRIEVAL_RANK_STATS_FIXED_REF
  bottom: "q" bottom: "qid" bottom: "r" bottom: "rid"
  top: "median_rank" top: "recall1" top: "recall5" top: "recall10" top: "map"
  retrieval_rank_stats_fixed_ref_param { stats_output_file: "out/stats.txt" num_reference_points: 1234 source: "ref_db" }
}
''')
    tool = os.path.join(built, "proto_tool")
    subprocess.run([tool, "text2bin", "NetParameter", str(net), str(tmp_path / "net.bin")], check=True)
    subprocess.run([tool, "bin2text", "NetParameter", str(tmp_path / "net.bin"), str(tmp_path / "back.prototxt")], check=True)
    back = (tmp_path / "back.prototxt").read_text()
    assert "RETRIEVAL_RANK_STATS_FIXED_REF" in back
    assert re.search(r'retrieval_rank_stats_fixed_ref_param\s*{[^}]*stats_output_file:\s*"out/stats.txt"', back)
    assert re.search(r"num_reference_points:\s*1234", back) and re.search(r'source:\s*"ref_db"', back)
    # field 52 of LayerParameter, fields 1 (string), 2 (varint), 3 (string) inside it (caffe.proto:950-954)
    raw = (tmp_path / "net.bin").read_bytes()
    assert b"\xa2\x03\x1a" + b"\x0a\x0dout/stats.txt\x10\xd2\x09\x1a\x06ref_db" in raw      # tag (52 << 3 | 2) = 0xa2 0x03, 26 bytes
    bad = tmp_path / "bad.prototxt"
    bad.write_text(net.read_text().replace("num_reference_points: 1234", "no_such_field: 1"))
    r = subprocess.run([tool, "text2bin", "NetParameter", str(bad), str(tmp_path / "bad.bin")], capture_output=True)
    assert b"RetrievalRankStatsFixedRefParameter" in r.stderr     # parsed field by field, no longer opaque: the stranger is named


def test_rank_stats_tool_is_built(built):
    assert os.access(os.path.join(built, "rank_stats"), os.X_OK)


def test_binding_declares_the_gallery_symbols():
    L = vv.load_library()
    for n in GALLERY_SYMBOLS:
        fn = getattr(L, n)
        assert fn.argtypes is not None and len(fn.argtypes) >= 2, n
    assert hasattr(vv.Engine, "gallery") and hasattr(vv.Engine, "gallery_from_table")
    for m in ("topk", "rank_stats", "close"):
        assert hasattr(vv.Gallery, m)


def test_library_exports_exactly_the_header(built):
    hdr = open(os.path.join(ROOT, "include", "videovec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", vv.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[-1].startswith("vv_")}
    assert set(GALLERY_SYMBOLS) <= declared
    assert len(declared) >= 74 + len(GALLERY_SYMBOLS)
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
