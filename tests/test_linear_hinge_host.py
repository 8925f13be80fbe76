"""Plumbing of the hinge loss's symbols: the header's prototypes, the library's exports and the ctypes binding agree; the enum values
the binding and tests/hinge_ref.py use are the header's (taken from the compiler); every new entry point cites hinge_loss_layer.cpp by
line.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hinge_ref as hr   # noqa: E402

from videovector_amd import engine   # noqa: E402

NEW = {"vv_linear_loss_set": 4, "vv_linear_loss_get": 4, "vv_op_hinge_loss": 11}      # name: parameters
HDR = open(os.path.join(ROOT, "include", "videovec.h")).read()


def test_header_library_and_binding_agree():
    lib = engine.lib_path()
    assert os.path.exists(lib), "build the library first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vv_[a-z0-9_]+)$", out, re.M))
    L = engine.load_library()
    for name, nargs in NEW.items():
        proto = re.search(r"^int %s\(([^;]*)\);" % name, HDR, re.M | re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == nargs, name
        assert name in exported, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    assert list(L.vv_op_hinge_loss.argtypes) == [vp, vp, i64, i32, i64, vp, i32, f32, vp, C.POINTER(f32), C.POINTER(i64)]
    assert list(L.vv_linear_loss_set.argtypes) == [vp, vp, i32, i32]
    for name in ("set_loss", "loss", "fit", "grad"):
        assert hasattr(engine.Linear, name)
    assert isinstance(engine.Linear.loss, property) and callable(engine.Engine.op_hinge_loss)
    import inspect
    assert {"loss", "norm"} <= set(inspect.signature(engine.Linear.fit).parameters)


def test_enum_values_are_the_headers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.fail("no C compiler to take the enum values from the header")
    src, exe = tmp_path / "en.c", tmp_path / "en"
    src.write_text('#include <stdio.h>\n#include "videovec.h"\n'
                   'int main(void) { printf("%d %d %d %d\\n", VV_LIN_LOSS_SOFTMAX, VV_LIN_LOSS_HINGE, VV_NORM_L1, VV_NORM_L2); return 0; }\n')
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [0, 1, 1, 2]
    assert got == [engine.LIN_LOSS_SOFTMAX, engine.LIN_LOSS_HINGE, engine.NORM_L1, engine.NORM_L2]
    assert got == [hr.SOFTMAX, hr.HINGE, hr.L1, hr.L2]


def test_every_new_entry_point_cites_the_reference_by_line():
    start = HDR.index("under HINGE_LOSS")
    block = HDR[HDR.rindex("/*", 0, start):HDR.index("*/", start)]
    for name in NEW:
        m = re.search(r"%s \(hinge_loss_layer\.cpp:\d+" % name, block)
        assert m, "%s carries no hinge_loss_layer.cpp:<line> cite" % name
    assert "src/caffe/layers/hinge_loss_layer.cpp:13-77" in block
    kern = open(os.path.join(ROOT, "videovector_amd", "csrc", "kernels_linear.hip")).read()
    assert "k_hinge" in kern and "hinge_loss_layer.cpp:13-77" in kern


def test_the_grid_constants_of_the_restatement_are_the_kernels():
    internal = open(os.path.join(ROOT, "videovector_amd", "csrc", "vv_internal.h")).read()
    assert int(re.search(r"constexpr int LIN_SM_BLOCKS = (\d+);", internal).group(1)) == hr.GRID_BLOCKS
    assert "dim3(LIN_SM_BLOCKS), dim3(256)" in open(os.path.join(ROOT, "videovector_amd", "csrc", "kernels_linear.hip")).read().split("void launch_hinge")[1]
    assert hr.WAVES == 256 // 64
