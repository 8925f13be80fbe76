"""The forward-only pass's surface without a GPU: include/videovec.h declares vv_forward, vv_eval_reset, vv_eval_stats and
vv_eval_report; the built library exports the three; engine.py binds them; the ctypes struct has the header's size (checked against a C
compiler's sizeof of the header's own typedef)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "videovec.h")
EXPORTS = ("vv_forward", "vv_eval_reset", "vv_eval_stats")


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_three_functions_and_the_struct():
    h = re.sub(r"\s+", " ", header_text())
    assert "int vv_forward(vv_ctx* ctx, const vv_step_cfg* cfg, const int32_t* idx, int idx_on_device);" in h
    assert "int vv_eval_reset(vv_ctx* ctx);" in h
    assert "int vv_eval_stats(vv_ctx* ctx, vv_eval_report* out);" in h
    m = re.search(r"typedef struct \{([^}]*)\} vv_eval_report;", h)
    assert m, "vv_eval_report is not declared"
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int64_t passes", "int64_t terms", "double loss_sum, viol_sum", "float last_loss, last_violations",
                      "float mean_loss, mean_violations"], fields
    assert "Net::Forward" in h                                            # the reference interface the entry replaces is named


def test_library_exports_them():
    from videovector_amd.engine import lib_path
    lib = C.CDLL(lib_path())
    for name in EXPORTS:
        assert hasattr(lib, name), "%s is not exported" % name


def test_engine_binds_them():
    import videovector_amd as vv
    from videovector_amd import engine
    L = vv.load_library()
    assert L.vv_forward.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] and L.vv_forward.restype is C.c_int
    assert L.vv_eval_reset.argtypes == [C.c_void_p]
    assert L.vv_eval_stats.argtypes == [C.c_void_p, C.POINTER(engine._EvalReport)]
    for name in ("forward", "eval_reset", "eval_stats"):
        assert callable(getattr(vv.Engine, name))


def test_ctypes_struct_has_the_headers_size(tmp_path):
    from videovector_amd import engine
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.fail("no C compiler to take sizeof(vv_eval_report) from the header")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "videovec.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(vv_eval_report), offsetof(vv_eval_report, loss_sum), '
                   'offsetof(vv_eval_report, last_loss), offsetof(vv_eval_report, mean_violations)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    R = engine._EvalReport
    assert got == [C.sizeof(R), R.loss_sum.offset, R.last_loss.offset, R.mean_violations.offset], got


def test_prototxt_writes_the_held_out_branch_only_when_asked():
    from videovector_amd.prototxt import solver, train_net
    src = "synthetic://videos=50;seed=1701;features=128"
    plain = train_net(src, 32, 5, 2, 32, max_buffer=500, dropout=0.5)
    assert "phase: TEST" not in plain and "held_out" not in plain
    held = train_net(src, 32, 5, 2, 32, max_buffer=500, dropout=0.5, held_out_source="synthetic://videos=40;seed=99;features=128", held_out_batch=24)
    assert held.count("type: VIDEO_SAMPLED_SHOTS_DATA") == 2 and "batch_size: 24" in held and "videos=40;seed=99" in held
    # every layer behind the data layers that was TRAIN-only runs in both phases; the data layers stay one per phase
    n_train = plain.count("include: { phase: TRAIN }")
    assert held.count("include: { phase: TRAIN }") == n_train and held.count("include: { phase: TEST }") == n_train
    assert held.replace("  include: { phase: TEST }\n", "").count("layers {") == plain.count("layers {") + 1
    with pytest.raises(ValueError):
        train_net(src, 32, 5, 2, 32, held_out_source=src, test_source=src, id_to_class_file="x")
    assert "test_compute_loss" not in solver("net.prototxt", test_iter=3, test_interval=2)
    assert "test_compute_loss: true" in solver("net.prototxt", test_iter=3, test_interval=2, test_compute_loss=True)
