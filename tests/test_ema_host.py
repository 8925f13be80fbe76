"""Non-GPU checks of the moving average's plumbing: include/videovec.h declares the entry points and says that the semantics are this
project's own, the built library exports them, the ctypes binding declares them with the record's layout; the facade's SolverParameter
parses ema_decay and test_with_ema from text, round-trips them on the wire with their documented numbers (137 and 138, behind 135 / 136)
and defaults to -1 / false; an old solver file parses to the same bytes as before; the prototxt writer emits the fields only when asked."""
import contextlib
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
NEW = {"vv_ema_set": 2, "vv_ema_get_decay": 2, "vv_ema_get": 3, "vv_ema_put": 3, "vv_ema_use": 2, "vv_ema_stats": 2}
F_DECAY, F_TEST = 137, 138


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
    assert re.search(r"float\s+decay\b", re.search(r"vv_ema_set\s*\(([^)]*)\)", code).group(1))
    for phrase in ("Neither the reference tree nor BVLC Caffe", "this project's own", "om = 1.0f - decay", "k_ema", "sync schedule", "VV_ERR_STATE",
                   "vv_params_set(vv_ema_get())"):
        assert phrase in hdr, phrase
    m = re.search(r"typedef struct \{([^{}]*)\}\s*vv_ema_report;", code)
    assert m and re.findall(r"\b(updates|decay|in_use)\b", m.group(1)) == ["updates", "decay", "in_use"]
    assert C.sizeof(engine._EmaReport) == 16 and [f for f, _ in engine._EmaReport._fields_] == ["updates", "decay", "in_use"]
    for meth in ("ema_set", "ema_get", "ema_put", "ema_use", "ema_stats", "ema"):
        assert hasattr(vv.Engine, meth), meth
    assert isinstance(vv.Engine.ema(object.__new__(vv.Engine)), contextlib.AbstractContextManager)


def test_solver_parameter_ema_fields(tool, tmp_path):  # noqa: F811
    txt = tmp_path / "s.prototxt"
    txt.write_text(solver("net.prototxt", ema_decay=0.999, test_with_ema=True))
    assert "ema_decay: 0.999" in txt.read_text() and "test_with_ema: true" in txt.read_text()
    subprocess.run([tool, "text2bin", "SolverParameter", str(txt), str(tmp_path / "s.bin")], check=True)
    f = fields((tmp_path / "s.bin").read_bytes())
    assert [x for x in f if x[0] == F_DECAY] == [(F_DECAY, 5, C.c_float(0.999).value)], f
    assert (F_TEST, 0, 1) in f, f
    subprocess.run([tool, "bin2text", "SolverParameter", str(tmp_path / "s.bin"), str(tmp_path / "s.txt")], check=True)
    back = (tmp_path / "s.txt").read_text()
    assert re.search(r"ema_decay:\s*0\.999", back) and re.search(r"test_with_ema:\s*true", back)
    subprocess.run([tool, "text2bin", "SolverParameter", str(tmp_path / "s.txt"), str(tmp_path / "s2.bin")], check=True)
    assert (tmp_path / "s2.bin").read_bytes() == (tmp_path / "s.bin").read_bytes()
    # an old solver file: the fields are not written, nothing of them on the wire, the bytes those of the file with the clipping and
    # accumulation fields beside it (135 / 136 keep their numbers)
    plain = solver("net.prototxt")
    assert "ema" not in plain, "the fields are written only when asked"
    assert "test_with_ema: false" in solver("net.prototxt", test_with_ema=False)
    (tmp_path / "p.prototxt").write_text(plain)
    subprocess.run([tool, "text2bin", "SolverParameter", str(tmp_path / "p.prototxt"), str(tmp_path / "p.bin")], check=True)
    assert not [x for x in fields((tmp_path / "p.bin").read_bytes()) if x[0] in (F_DECAY, F_TEST)]
    (tmp_path / "old.prototxt").write_text(solver("net.prototxt", clip_gradients=35, iter_size=2))
    subprocess.run([tool, "text2bin", "SolverParameter", str(tmp_path / "old.prototxt"), str(tmp_path / "old.bin")], check=True)
    f = fields((tmp_path / "old.bin").read_bytes())
    assert (135, 5, 35.0) in f and (136, 0, 2) in f and not [x for x in f if x[0] in (F_DECAY, F_TEST)]
    src = open(os.path.join(ROOT, "caffe_facade", "src", "proto_lite.cpp")).read()
    assert re.search(r'OPTD\(%d,\s*"ema_decay",\s*T_FLOAT,\s*"-1"\)' % F_DECAY, src), "the default is -1"
    assert re.search(r'OPTD\(%d,\s*"test_with_ema",\s*T_BOOL,\s*"false"\)' % F_TEST, src), "the default is false"
    assert len(re.findall(r"\b(?:OPTD|OPT|REP|OENUM|OMSG|RMSG)\((?:%d|%d)," % (F_DECAY, F_TEST), src.split('{"SolverParameter"')[1].split('{"SolverState"')[0])) == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ema_decay" in doc and "test_with_ema" in doc and str(F_DECAY) in doc and str(F_TEST) in doc
