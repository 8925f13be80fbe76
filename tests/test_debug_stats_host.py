"""Host side of the magnitude statistics (the reference's SolverParameter.debug_info, caffe.proto field 23; net.cpp:580-636): the header
declares vv_op_asum, vv_debug_stats_queue, vv_debug_mark_update, vv_debug_stats_get, the record and the enum; the built library exports
the entry points; the binding's record has the header's size and the binding's names are the enum's, in order; debug_info parses from a
solver prototxt.  No GPU.  Without the feature the header has none of this: every case but the parse fails."""
import ctypes
import os
import re
import subprocess

import videovector_amd as vv
from videovector_amd import engine, prototxt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vv_op_asum", "vv_debug_stats_queue", "vv_debug_mark_update", "vv_debug_stats_get")
ENUM = ("VV_STAT_W", "VV_STAT_B", "VV_STAT_HIST_W", "VV_STAT_HIST_B", "VV_STAT_DW", "VV_STAT_DB", "VV_STAT_TARGET_SCORE",
        "VV_STAT_NEGATIVE_SCORES", "VV_STAT_UPD_W", "VV_STAT_UPD_B", "VV_STAT_N")


def header():
    return open(os.path.join(ROOT, "include", "videovec.h")).read()


def code_of(hdr):
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_entry_points_the_struct_and_the_enum():
    code = code_of(header())
    flat = " ".join(code.split())
    for proto in ("int vv_op_asum(vv_ctx* ctx, const float* x_dev, int64_t n, vv_abs_stat* out);",
                  "int vv_debug_stats_queue(vv_ctx* ctx, uint32_t mask);",
                  "int vv_debug_mark_update(vv_ctx* ctx);",
                  "int vv_debug_stats_get(vv_ctx* ctx, vv_abs_stat out[VV_STAT_N]);"):
        assert proto in flat, proto
    assert "typedef struct { double asum; float amax; int32_t reserved_; int64_t count, nonfinite; } vv_abs_stat;" in flat
    m = re.search(r"enum\s*\{([^}]*VV_STAT_N[^}]*)\}", code)
    assert m, "no enum with VV_STAT_N"
    assert tuple(x.strip() for x in m.group(1).split(",") if x.strip()) == ENUM


def test_header_comments_cite_the_reference():
    """each entry point's comment names net.cpp:580-636 and blob.cpp:138-165"""
    hdr = header()
    for name in ENTRY_POINTS:
        at = hdr.index("int %s(" % name)
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "net.cpp:580-636" in comment and "blob.cpp:138-165" in comment, name
    at = hdr.index("int vv_debug_mark_update(")
    assert "ONE fp32 subtraction per element" in hdr[hdr.rindex("/*", 0, at):at]


def test_library_exports_the_entry_points():
    L = vv.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is ctypes.c_int


def test_binding_record_matches_the_header(tmp_path):
    """sizeof and the field offsets as a C compiler lays out the header's struct"""
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "videovec.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(vv_abs_stat), offsetof(vv_abs_stat, asum), '
                   'offsetof(vv_abs_stat, amax), offsetof(vv_abs_stat, count), offsetof(vv_abs_stat, nonfinite), (int)VV_STAT_N); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_asum, o_amax, o_count, o_nf, n = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    S = engine._AbsStat
    assert (ctypes.sizeof(S), S.asum.offset, S.amax.offset, S.count.offset, S.nonfinite.offset) == (size, o_asum, o_amax, o_count, o_nf)
    assert size == 32
    assert len(engine.STAT_NAMES) == n and tuple("VV_STAT_" + s for s in engine.STAT_NAMES) == ENUM[:-1]


def test_debug_info_parses_from_a_solver_prototxt(tmp_path):
    tool = os.path.join(ROOT, "caffe_facade", "build", "proto_tool")
    assert os.path.exists(tool), "build() makes caffe_facade/build/proto_tool"
    for on in (True, False):
        txt = tmp_path / ("solver_%d.prototxt" % on)
        txt.write_text(prototxt.solver("net.prototxt", display=1, max_iter=3, debug_info=on))
        assert ("debug_info: true" in txt.read_text()) == on
        subprocess.run([tool, "text2bin", "SolverParameter", str(txt), str(tmp_path / "s.bin")], check=True)
        subprocess.run([tool, "bin2text", "SolverParameter", str(tmp_path / "s.bin"), str(tmp_path / "s.txt")], check=True)
        back = (tmp_path / "s.txt").read_text()
        assert ("debug_info: true" in back) == on, back
