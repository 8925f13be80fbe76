"""Non-GPU checks of the RMSProp / Adam plumbing: include/videovec.h declares the new entry points and solver types and says where the
rules come from, the built library exports them, the ctypes binding declares them; the facade's SolverParameter parses BVLC Caffe's
rms_decay (38) and momentum2 (39) and the three new SolverType values through text and wire; the prototxt writer emits the two fields
only when asked."""
import os
import re
import struct
import subprocess

import ctypes as C

import videovector_amd as vv
from tests.test_facade_proto import tool  # noqa: F401  (fixture)
from videovector_amd import engine
from videovector_amd.prototxt import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vv_solver_ext_set": 3, "vv_solver_ext_get": 3, "vv_solver_iter_set": 2, "vv_solver_iter_get": 2, "vv_history2_set": 3, "vv_history2_get": 3}


def header():
    return open(os.path.join(ROOT, "include", "videovec.h")).read()


def test_header_binding_and_exports_agree(tool):  # noqa: F811  (the fixture builds the library)
    hdr = header()
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
    assert re.search(r"VV_SOLVER_RMSPROP\s*=\s*3\b", code) and re.search(r"VV_SOLVER_ADAM\s*=\s*5\b", code)
    for phrase in ("RMSPropSolver", "AdamSolver", "BVLC", "momentum2", "rms_decay", "0.999", "0.99", "iter + 1", "not implemented"):
        assert phrase in hdr, phrase
    assert engine.SOLVER_TYPES == {"SGD": 0, "NESTEROV": 1, "ADAGRAD": 2, "RMSPROP": 3, "ADAM": 5}
    for meth in ("history2_set", "history2_get", "solver_iter", "solver_ext_set", "solver_ext_get"):
        assert hasattr(vv.Engine, meth), meth
    cfg = vv.StepConfig(4, 3, 2, solver_type="ADAM", momentum2=0.98, rms_decay=0.9)
    assert cfg.c.solver_type == 5 and cfg.momentum2 == 0.98 and cfg.rms_decay == 0.9
    assert vv.StepConfig(4, 3, 2, solver_type="RMSPROP").c.solver_type == 3 and vv.StepConfig(4, 3, 2).momentum2 is None
    assert C.sizeof(engine._StepCfg) == C.sizeof(type(vv.StepConfig(1, 2, 1).c))          # (the struct keeps its layout: nothing was added)


def fields(buf):
    """(field number, wire type, value) of a flat protobuf message"""
    i, out = 0, []
    def varint():
        nonlocal i
        v, s = 0, 0
        while True:
            b = buf[i]; i += 1
            v |= (b & 0x7F) << s; s += 7
            if not b & 0x80:
                return v
    while i < len(buf):
        key = varint()
        num, wt = key >> 3, key & 7
        if wt == 0: out.append((num, wt, varint()))
        elif wt == 5: out.append((num, wt, struct.unpack("<f", buf[i:i + 4])[0])); i += 4
        elif wt == 1: out.append((num, wt, struct.unpack("<d", buf[i:i + 8])[0])); i += 8
        elif wt == 2:
            n = varint(); out.append((num, wt, bytes(buf[i:i + n]))); i += n
        else: raise AssertionError("wire type %d" % wt)
    return out


def test_solver_parameter_fields_parse_and_round_trip(tool, tmp_path):  # noqa: F811
    for stype, num in (("RMSPROP", 3), ("ADADELTA", 4), ("ADAM", 5)):
        txt = tmp_path / ("s_%s.prototxt" % stype)
        txt.write_text(solver("net.prototxt", solver_type=stype, momentum2=0.98, rms_decay=0.9, delta=1e-6))
        subprocess.run([tool, "text2bin", "SolverParameter", str(txt), str(tmp_path / "s.bin")], check=True)
        f = fields((tmp_path / "s.bin").read_bytes())
        assert (30, 0, num) in f, (stype, f)
        assert (38, 5, struct.unpack("<f", struct.pack("<f", 0.9))[0]) in f and (39, 5, struct.unpack("<f", struct.pack("<f", 0.98))[0]) in f
        subprocess.run([tool, "bin2text", "SolverParameter", str(tmp_path / "s.bin"), str(tmp_path / "s.txt")], check=True)
        back = (tmp_path / "s.txt").read_text()
        assert re.search(r"solver_type:\s*%s\b" % stype, back) and re.search(r"rms_decay:\s*0\.9\b", back) and re.search(r"momentum2:\s*0\.98\b", back)
        subprocess.run([tool, "text2bin", "SolverParameter", str(tmp_path / "s.txt"), str(tmp_path / "s2.bin")], check=True)
        assert (tmp_path / "s2.bin").read_bytes() == (tmp_path / "s.bin").read_bytes()
    plain = solver("net.prototxt", solver_type="ADAM")
    assert "momentum2" not in plain and "rms_decay" not in plain, "the two fields are written only when asked"
    (tmp_path / "p.prototxt").write_text(plain)
    subprocess.run([tool, "text2bin", "SolverParameter", str(tmp_path / "p.prototxt"), str(tmp_path / "p.bin")], check=True)
    assert not [x for x in fields((tmp_path / "p.bin").read_bytes()) if x[0] in (38, 39)]
