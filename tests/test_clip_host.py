"""Non-GPU checks of the gradient-clipping plumbing: include/videovec.h declares the three entry points and says where the semantics come
from, the built library exports them, the ctypes binding declares them; the facade's SolverParameter parses clip_gradients from text (by
name, as a BVLC solver file writes it), round-trips it on the wire with its documented number (135: BVLC's 35 is taken in this fork) and
defaults to -1; the prototxt writer emits it only when asked."""
import os
import re
import subprocess

import ctypes as C

import videovector_amd as vv
from tests.test_facade_proto import tool  # noqa: F401  (fixture)
from tests.test_solver_ext_host import fields
from videovector_amd import engine
from videovector_amd.prototxt import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vv_clip_gradients_set": 2, "vv_clip_gradients_get": 2, "vv_clip_stats": 2}
FIELD = 135


def test_header_binding_and_exports_agree(tool):  # noqa: F811  (the fixture builds the library)
    hdr = open(os.path.join(ROOT, "include", "videovec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", vv.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    L = vv.load_library()
    for name, nargs in NEW.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in exported, name + " is not exported"
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int
    assert re.search(r"float\s+clip\b", re.search(r"vv_clip_gradients_set\s*\(([^)]*)\)", code).group(1))
    for phrase in ("SGDSolver::ClipGradients", "BVLC", "clip_gradients", "the reference tree has no such function", "sync schedule", "VV_ERR_STATE"):
        assert phrase in hdr, phrase
    m = re.search(r"typedef struct \{([^{}]*)\}\s*vv_clip_report;", code)
    assert m and [w for w in re.findall(r"\b(norm|scale|clipped|updates|clipped_updates)\b", m.group(1))] == ["norm", "scale", "clipped", "updates", "clipped_updates"]
    assert C.sizeof(engine._ClipReport) == 32
    for meth in ("clip_gradients_set", "clip_gradients_get", "clip_stats"):
        assert hasattr(vv.Engine, meth), meth
    cfg = vv.StepConfig(4, 3, 2, clip_gradients=35)
    assert cfg.clip_gradients == 35.0 and vv.StepConfig(4, 3, 2).clip_gradients is None
    assert C.sizeof(engine._StepCfg) == C.sizeof(type(vv.StepConfig(1, 2, 1).c))          # (the struct keeps its layout: nothing was added)


def test_solver_parameter_clip_gradients(tool, tmp_path):  # noqa: F811
    txt = tmp_path / "s.prototxt"
    txt.write_text(solver("net.prototxt", clip_gradients=35))
    assert "clip_gradients: 35.0" in txt.read_text()
    subprocess.run([tool, "text2bin", "SolverParameter", str(txt), str(tmp_path / "s.bin")], check=True)
    f = fields((tmp_path / "s.bin").read_bytes())
    assert (FIELD, 5, 35.0) in f, f
    assert not [x for x in f if x[0] == 35], "35 is snapshot_vis_truncate_len in this fork"
    subprocess.run([tool, "bin2text", "SolverParameter", str(tmp_path / "s.bin"), str(tmp_path / "s.txt")], check=True)
    assert re.search(r"clip_gradients:\s*35\b", (tmp_path / "s.txt").read_text())
    subprocess.run([tool, "text2bin", "SolverParameter", str(tmp_path / "s.txt"), str(tmp_path / "s2.bin")], check=True)
    assert (tmp_path / "s2.bin").read_bytes() == (tmp_path / "s.bin").read_bytes()
    # a BVLC solver file as it is: the field by name beside the fork's own field 35
    both = tmp_path / "both.prototxt"
    both.write_text(solver("net.prototxt") + "clip_gradients: 10\nsnapshot_vis_truncate_len: 7\n")
    subprocess.run([tool, "text2bin", "SolverParameter", str(both), str(tmp_path / "both.bin")], check=True)
    f = fields((tmp_path / "both.bin").read_bytes())
    assert (FIELD, 5, 10.0) in f and (35, 0, 7) in f
    # absent: not written, and the default is -1
    plain = solver("net.prototxt")
    assert "clip_gradients" not in plain, "the field is written only when asked"
    (tmp_path / "p.prototxt").write_text(plain)
    subprocess.run([tool, "text2bin", "SolverParameter", str(tmp_path / "p.prototxt"), str(tmp_path / "p.bin")], check=True)
    assert not [x for x in fields((tmp_path / "p.bin").read_bytes()) if x[0] == FIELD]
    src = open(os.path.join(ROOT, "caffe_facade", "src", "proto_lite.cpp")).read()
    assert re.search(r'OPTD\(%d,\s*"clip_gradients",\s*T_FLOAT,\s*"-1"\)' % FIELD, src), "the default is -1"
    assert "clip_gradients" in open(os.path.join(ROOT, "INTEGRATION.md")).read() and str(FIELD) in open(os.path.join(ROOT, "INTEGRATION.md")).read()
