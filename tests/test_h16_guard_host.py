"""Non-GPU checks of the f16 rows' range guard: include/videovec.h declares vv_h16_stats and its report, documents the option's three values,
the two counts and the lag; the built library exports the function; the ctypes binding mirrors the struct."""
import ctypes as C
import os
import re
import subprocess

import pytest

import videovector_amd as vv
from videovector_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("saturated", 8), ("faint_rows", 8), ("flagged_steps", 8), ("first_flagged_step", 8), ("fallback", 4), ("rows_f16", 4)]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "videovector_amd", "csrc"), "-s", "-j4"], check=True)


def header():
    return open(os.path.join(ROOT, "include", "videovec.h")).read()


def test_header_declares_the_report_and_documents_the_guard():
    hdr = header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+vv_h16_stats\s*\(\s*vv_ctx\s*\*\s*\w+\s*,\s*vv_h16_report\s*\*\s*\w+\s*\)\s*;", code)
    m = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*vv_h16_report\s*;", code, flags=re.S)
    assert m, "vv_h16_report is not declared"
    names = re.findall(r"\b(?:int64_t|int32_t)\b([^;]*);", m.group(1))
    assert [n.strip() for grp in names for n in grp.split(",")] == [n for n, _ in FIELDS]
    for phrase in ('"h16_guard" (VV_H16_GUARD, 1)', '"last_h16"', "65504", "2^-14", "[65488, 65504)", "step s + 4", "bf16"):
        assert phrase in hdr, phrase


def test_binding_mirrors_the_report():
    assert [(n, C.sizeof(t)) for n, t in engine._H16Report._fields_] == FIELDS
    assert C.sizeof(engine._H16Report) == 40
    L = vv.load_library()
    assert L.vv_h16_stats.argtypes is not None and len(L.vv_h16_stats.argtypes) == 2
    assert hasattr(vv.Engine, "h16_stats")


def test_library_exports_vv_h16_stats(built):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", code))
    out = subprocess.run(["nm", "-D", "--defined-only", vv.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[-1].startswith("vv_")}
    assert "vv_h16_stats" in declared and "vv_h16_stats" in exported
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
