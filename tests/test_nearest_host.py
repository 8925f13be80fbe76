"""CPU tests of the nearest-neighbour lists: the numpy restatement the GPU tests compare against gives the hand-worked lists of a
4 x 6 case and agrees with a brute-force loop on the exclusion input; the exact inputs have integer distances; the binding
declares the two new entry points and the built library exports them."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nearest_ref as ref   # noqa: E402

import videovector_amd as vv   # noqa: E402

NEW_SYMBOLS = ["vv_gallery_nearest", "vv_gallery_nearest_self"]

# the vectors of test_gpu_gallery.py::test_known_answer
Q = np.array([[1, 0], [0, 1], [.6, .8], [1, 0]], np.float32)
QID = np.array([7, 7, 9, 3], np.int32)
G = np.array([[1, 0], [.8, .6], [0, 1], [.6, .8], [1, 0], [-1, 0]], np.float32)
GID = np.array([9, 7, 7, 9, 7, 5], np.int32)
# d = -2 Q G^T:  row 0 / 3: -2 -1.6 0 -1.2 -2 2;  row 1: 0 -1.2 -2 -1.6 0 0;  row 2: -1.2 -1.92 -1.6 -2 -1.2 1.2
HAND_ALL = [[0, 4, 1, 3, 2, 5, -1], [2, 3, 1, 0, 4, 5, -1], [3, 1, 2, 0, 4, 5, -1], [0, 4, 1, 3, 2, 5, -1]]
HAND_ALL_D = [[-2, -2, -1.6, -1.2, 0, 2, 0], [-2, -1.6, -1.2, 0, 0, 0, 0], [-2, -1.92, -1.6, -1.2, -1.2, 1.2, 0],
              [-2, -2, -1.6, -1.2, 0, 2, 0]]
# items of another id only: query 0 / 1 (id 7) may list items 0, 3, 5; query 2 (id 9) items 1, 2, 4, 5; query 3 (id 3) all
HAND_OTHER = [[0, 3, 5, -1], [3, 0, 5, -1], [1, 2, 4, 5], [0, 4, 1, 3]]
HAND_OTHER_D = [[-2, -1.2, 2, 0], [-1.6, 0, 0, 0], [-1.92, -1.6, -1.2, 1.2], [-2, -2, -1.6, -1.2]]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "videovector_amd", "csrc"), "-s", "-j4"], check=True)


def test_hand_worked_case():
    d = ref.distances32(Q, G)
    assert not np.signbit(d).any() or (d[np.signbit(d)] != 0).all()            # no -0 is left
    idx, dist = ref.nearest(d, None, 7)
    assert idx.tolist() == HAND_ALL
    assert np.abs(dist - np.array(HAND_ALL_D)).max() <= 1e-6
    idx, dist = ref.nearest(d, GID[None, :] != QID[:, None], 4)
    assert idx.tolist() == HAND_OTHER
    assert np.abs(dist - np.array(HAND_OTHER_D)).max() <= 1e-6
    idx, dist = ref.nearest(d, None, 2)
    assert idx.tolist() == [r[:2] for r in HAND_ALL]


def test_restatement_against_brute_force_on_the_exclusion_input():
    """The input of the GPU tests' exclusion case, cut to a size a Python loop walks: 50 ids, then one id that owns all but 10."""
    Qx, qid, Gx, gid = ref.exact_input(64, 50001, 50, 21)
    Qx, qid, Gx, gid = Qx[:6], qid[:6], Gx[:3000], gid[:3000]
    d = ref.distances32(Qx, Gx)
    assert (d == np.round(d)).all() and d.dtype == np.float32
    for ids, q_ids in ((gid, qid), (ref.one_id_owns_all_but(gid, 50, 10, 22), np.array([50, 50, 3, 50, 7, 50], np.int32))):
        el = ids[None, :] != q_ids[:, None]
        a = ref.nearest(d, el, 64)
        b = ref.nearest_brute_force(d, el, 64)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert (a[0][0, :10] >= 0).all() and (a[0][0, 10:] == -1).all() and (a[1][0, 10:] == 0).all()


def test_exact_inputs_have_integer_distances():
    for args in ((64, 50001, 50, 21), (1, 3000, 60, 23)):
        Qx, _, Gx, _ = ref.exact_input(*args)
        d = ref.distances32(Qx, Gx)
        assert d.dtype == np.float32 and (d == np.round(d)).all() and np.abs(d).max() <= 2 * 9 * 40
        assert np.array_equal(d, -2.0 * (Qx.astype(np.float64) @ Gx.astype(np.float64).T) + 0.0)
        assert len(np.unique(d)) <= 1441


def test_binding_declares_the_new_symbols():
    L = vv.load_library()
    for n in NEW_SYMBOLS:
        fn = getattr(L, n)
        assert fn.argtypes is not None and len(fn.argtypes) >= 6, n
    for m in ("nearest", "nearest_self"):
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
