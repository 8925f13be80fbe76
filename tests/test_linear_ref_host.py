"""Host tests of the softmax linear classifier's restatement (tests/linear_ref.py) and of the new symbols' plumbing: the float64
gradient against central differences of its own loss, the softmax's invariants, the cursor, and that header, library, ctypes
structs (against the compiler's sizeof of the header's typedefs) and binding agree.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linear_ref as ref   # noqa: E402

from videovector_amd import engine   # noqa: E402

NEW = ["vv_linear_create", "vv_linear_destroy", "vv_linear_get", "vv_linear_put", "vv_linear_cfg_default", "vv_linear_fit",
       "vv_linear_grad", "vv_linear_scores", "vv_op_softmax_loss", "vv_op_gemm_tn"]


def test_gradient_matches_central_differences():
    rs = np.random.RandomState(1)
    X, y = ref.blobs(n=24, C=3, dim=5, seed=2)
    st = ref.State(5, 3)
    st.W, st.b = rs.randn(3, 5), rs.randn(3)
    dW, db, _, _ = ref.gradient(st, X, y, loss_weight=0.25)
    h = 1e-6

    def loss_at(W, b):
        s = ref.State(5, 3)
        s.W, s.b = W, b
        return ref.gradient(s, X, y, loss_weight=0.25)[2]
    for c in range(3):
        for d in range(5):
            Wp, Wm = st.W.copy(), st.W.copy()
            Wp[c, d] += h
            Wm[c, d] -= h
            assert abs((loss_at(Wp, st.b) - loss_at(Wm, st.b)) / (2 * h) - dW[c, d]) < 1e-8
        bp, bm = st.b.copy(), st.b.copy()
        bp[c] += h
        bm[c] -= h
        assert abs((loss_at(st.W, bp) - loss_at(st.W, bm)) / (2 * h) - db[c]) < 1e-8


def test_softmax_rows_sum_to_one_and_ties_take_the_first_maximum():
    z = np.array([[1.0, 3.0, 3.0, -2.0], [0.0, 0.0, 0.0, 0.0], [5.0, -1.0, 5.0, 5.0]])
    p, dz, _, correct = ref.softmax_loss(z, np.array([2, 0, 0]))
    assert np.allclose(p.sum(axis=1), 1.0, atol=1e-15)
    assert list(ref.first_max(z)) == [1, 0, 0]
    assert correct == 2                                  # row 0's label 2 ties the maximum but column 1 comes first
    assert np.allclose(dz.sum(axis=1), 0.0, atol=1e-16)
    p32, _, _, c32 = ref.softmax_loss_f32(z, np.array([2, 0, 0]))
    assert c32 == 2 and np.allclose(p32.sum(axis=1), 1.0, atol=4e-7)
    assert list(ref.first_max(np.array([[np.nan, 1.0, 1.0], [np.nan, np.nan, np.nan]]))) == [1, 0]


def test_flt_min_clamp():
    z = np.array([[0.0, -200.0]])
    for fn in (ref.softmax_loss, ref.softmax_loss_f32):
        _, _, loss, _ = fn(z, np.array([1]))
        assert abs(float(loss) - (-np.log(float(ref.FLT_MIN)))) < 1e-5      # 87.3365..., not 200 and not inf


def test_cursor_sequence():
    plan, cursor = ref.batches(10, 4, 5)
    assert [c for _, c in plan] == [4, 4, 2, 4, 4] and [f for f, _ in plan] == [0, 4, 8, 0, 4] and cursor == 8
    plan, cursor = ref.batches(10, 4, 2, cursor=cursor)
    assert plan == [(8, 2), (0, 4)] and cursor == 4
    assert ref.batches(10, 0, 2) == ([(0, 10), (0, 10)], 0)
    assert [c for _, c in ref.batches(256, 100, 4)[0]] == [100, 100, 56, 100]


def test_blob_fit_reaches_the_stated_figures():
    X, y = ref.blobs()
    for batch in (0, 64, 100):
        st = ref.State(8, 4)
        trace, _ = ref.fit(st, X, y, 60, batch=batch, lr=0.5, momentum=0.9, weight_decay=1e-4)
        z = X.astype(np.float64) @ st.W.T + st.b
        assert (np.argmax(z, axis=1) == y).all()
        srt = np.sort(z, axis=1)
        assert (srt[:, -1] - srt[:, -2]).min() > 4.1 and trace[-1] < 1e-4
        s32 = ref.State(8, 4, np.float32)
        ref.fit(s32, X, y, 60, batch=batch, lr=0.5, momentum=0.9, weight_decay=1e-4)
        assert np.abs(s32.W - st.W).max() < 5e-6


def test_header_library_and_binding_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "videovec.h")).read()
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared
    lib = engine.lib_path()
    assert os.path.exists(lib), "build the library first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vv_[a-z0-9_]+)$", out, re.M))
    assert set(NEW) <= exported
    L = engine.load_library()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
    for name in ("fit", "grad", "scores", "get", "put", "close"):
        assert callable(getattr(engine.Linear, name))
    for name in ("linear", "op_softmax_loss", "op_gemm_tn"):
        assert callable(getattr(engine.Engine, name))


def test_ctypes_structs_have_the_headers_sizes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.fail("no C compiler to take the structs' sizes from the header")
    src, exe = tmp_path / "sz.c", tmp_path / "sz"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "videovec.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(vv_linear_cfg), offsetof(vv_linear_cfg, loss_weight), '
                   'sizeof(vv_linear_report), offsetof(vv_linear_report, accuracy_last), offsetof(vv_linear_report, steps), '
                   'offsetof(vv_linear_report, nonfinite_rows)); return 0; }\n')
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    Cf, R = engine._LinearCfg, engine._LinearReport
    assert got == [C.sizeof(Cf), Cf.loss_weight.offset, C.sizeof(R), R.accuracy_last.offset, R.steps.offset, R.nonfinite_rows.offset], got
