"""CPU tests of the class-level retrieval statistics: the float64 restatement the GPU tests compare against reproduces the
issue's figures, the reference's known answer and a hand-worked case; the facade's protobuf stand-in round-trips the three
RetrievalStatsParameter fields the new path reads; the library exports what include/videovec.h declares, the two new entry
points among them; the class_stats tool is built."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import class_stats_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

NEW_SYMBOLS = ["vv_gallery_pool_by_id", "vv_gallery_class_stats"]

INPUTS = {"A": (4096, 512, 300, 15, 3.0, 6.0, 11), "B": (3001, 96, 211, 7, 1.5, 2.5, 12)}
# float64: (mAP, hit@1, hit@5) with exclude on, with exclude off, scored queries; video level: videos, scored, (mAP, hit@1, hit@5)
EXPECT64 = {"A": ((0.115255, 0.2784, 0.2441), (0.186506, 1.0000, 0.9968), 3923, 300, 286, (0.527669, 0.8182, 0.7189)),
            "B": ((0.369015, 0.7065, 0.6756), (0.409285, 0.9651, 0.9273), 2869, 211, 201, (0.874791, 0.9900, 0.9761))}

# the hand-worked case: classes 1, 1, -1, 0 (id 20 is absent from the map), 0, 2; rows 2 and 3 are equal
HAND_X = np.array([[1, 0], [.8, .6], [0, 1], [0, 1], [.6, .8], [-1, 0]], np.float32)
HAND_IDS = np.array([10, 10, 30, 20, 40, 50], np.int32)
HAND_MAP = {10: 1, 30: -1, 40: 0, 50: 2}
NAN = float("nan")
HAND = {True: dict(ap=[0, 0, NAN, .5, 1 / 3, 0], acc1=[0, 0, NAN, 0, 0, 0], acc5=[0, 0, NAN, .2, .2, 0],
                   mean_ap=(.5 + 1 / 3) / 5, hit_at_1=0.0, hit_at_5=.08),
        False: dict(ap=[1, .5, NAN, .5, 1 / 3, 0], acc1=[1, 0, NAN, 0, 0, 0], acc5=[.2, .2, NAN, .2, .2, 0],
                    mean_ap=(2 + 1 / 3) / 5, hit_at_1=.2, hit_at_5=.16)}
HAND_TOP5 = [[4, 2, 3, 5, -1], [4, 2, 3, 5, -1], [-1] * 5, [2, 4, 1, 0, 5], [1, 2, 3, 0, 5], [2, 3, 4, 1, 0]]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "videovector_amd", "csrc"), "-s", "-j4"], check=True)
    subprocess.run(["make", "-C", os.path.join(ROOT, "caffe_facade"), "-s", "-j4"], check=True)
    return os.path.join(ROOT, "caffe_facade", "build")


def close(got, want, tol):
    return all(abs(g - w) <= tol for g, w in zip(got, want))


@pytest.mark.parametrize("name", ["A", "B"])
def test_float64_reference_figures(name):
    X, vid, m = ref.make_input(*INPUTS[name])
    on, off, scored, nvid, vscored, vlevel = EXPECT64[name]
    d = ref.distances(X)
    for exclude, want in ((True, on), (False, off)):
        s = ref.class_stats(d, vid, m, exclude)[0]
        print(name, exclude, s)
        assert s["n_scored"] == scored
        assert abs(s["mean_ap"] - want[0]) <= 6e-5 and close((s["hit_at_1"], s["hit_at_5"]), want[1:], 6e-4), (s, want)
    P, pid = ref.pool_by_id(X, vid)
    assert len(pid) == nvid and (np.diff(pid) > 0).all()
    s = ref.class_stats(ref.distances(P), pid, m, True)[0]
    print(name, "video level", s)
    assert s["n_scored"] == vscored
    assert abs(s["mean_ap"] - vlevel[0]) <= 6e-5 and close((s["hit_at_1"], s["hit_at_5"]), vlevel[1:], 6e-4), (s, vlevel)


def test_reference_known_answer():
    """test_retrieval_stats_layer.cpp:34-39, 82-84."""
    X = np.array([[1, 0], [0, 1], [1, .06], [0, 1], [1, .1]], np.float32)
    s = ref.class_stats(ref.distances(X), np.array([2, 3, 4, 5, 6]), {2: 1, 3: 2, 4: 1, 5: 2, 6: 2}, True)[0]
    assert abs(s["mean_ap"] - 0.7833333) <= 1e-6 and abs(s["hit_at_1"] - 0.60) <= 1e-9 and abs(s["hit_at_5"] - 0.32) <= 1e-9


@pytest.mark.parametrize("exclude", [True, False])
def test_hand_worked_case(exclude):
    s, ap, a1, a5, t5 = ref.class_stats(ref.distances(HAND_X), HAND_IDS, HAND_MAP, exclude)
    h = HAND[exclude]
    assert np.allclose(ap, h["ap"], atol=1e-12, equal_nan=True)
    assert np.array_equal(a1, h["acc1"], equal_nan=True) and np.allclose(a5, h["acc5"], atol=1e-12, equal_nan=True)
    assert t5.tolist() == HAND_TOP5
    assert s["n_scored"] == 5
    for f in ("mean_ap", "hit_at_1", "hit_at_5"):
        assert abs(s[f] - h[f]) <= 1e-12, f


def test_proto_round_trips_the_layer_parameters(built, tmp_path):
    net = tmp_path / "net.prototxt"
    net.write_text('''name: "stats"
layers {
  name: "stats" type: RETRIEVAL_STATS
  bottom: "x" bottom: "ids"
  top: "test_map" top: "test_hit_at_1" top: "test_hit_at_5"
  retrieval_stats_param { id_to_class_file: "map.txt" stats_output_file: "out/stats.txt" exclude_same_video_shots: false
                          video_level_retrieval: true max_num_videos: 1234 }
}
''')
    tool = os.path.join(built, "proto_tool")
    subprocess.run([tool, "text2bin", "NetParameter", str(net), str(tmp_path / "net.bin")], check=True)
    subprocess.run([tool, "bin2text", "NetParameter", str(tmp_path / "net.bin"), str(tmp_path / "back.prototxt")], check=True)
    back = (tmp_path / "back.prototxt").read_text()
    block = re.search(r"retrieval_stats_param\s*{([^}]*)}", back).group(1)
    assert re.search(r'stats_output_file:\s*"out/stats.txt"', block) and re.search(r"video_level_retrieval:\s*true", block)
    assert re.search(r"max_num_videos:\s*1234", block) and re.search(r"exclude_same_video_shots:\s*false", block)
    # field 47 of LayerParameter; inside it 1, 2 (strings), 3, 4 (bools), 5 (varint 1234) (caffe.proto:955-966)
    raw = (tmp_path / "net.bin").read_bytes()
    assert b"\x0a\x07map.txt\x12\x0dout/stats.txt\x18\x00\x20\x01\x28\xd2\x09" in raw


def test_tools_are_built(built):
    assert os.access(os.path.join(built, "class_stats"), os.X_OK) and os.access(os.path.join(built, "rank_stats"), os.X_OK)


def test_binding_declares_the_new_symbols():
    L = vv.load_library()
    for n in NEW_SYMBOLS:
        fn = getattr(L, n)
        assert fn.argtypes is not None and len(fn.argtypes) >= 3, n
    for m in ("pool_by_id", "class_stats", "rows"):
        assert hasattr(vv.Gallery, m)


def test_library_exports_the_header_with_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "videovec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", vv.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[-1].startswith("vv_")}
    assert set(NEW_SYMBOLS) <= declared
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    print(len(exported), "exports")
