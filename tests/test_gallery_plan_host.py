"""The gallery scratch's sizes of videovector_amd/csrc/vv_gallery_plan.h on the host: builds tools/gallery_plan_check.cc with g++ (the
header includes no HIP header), runs it -- one line per combination of the edge shapes, query counts and the class / selection flags
-- and compares every line with the arithmetic as restated in tests/gallery_plan_ref.py from the entry points' own former sums."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovector_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gallery_plan_ref as ref   # noqa: E402

IN_KEYS = ("n_ref", "dim", "n_q", "cls", "sel")
OUT_KEYS = ("Dp", "pitch", "seg", "S", "qb_max", "row_bytes", "block_rows")
# where behaviour can change: the 64-float pitch; 64 * 16384 items, where seg leaves its floor; 503808, the largest pitch that still
# allows 512-row blocks under the distances' share of the limit, and the first that does not; 2^30 items, of which not one row fits
N_REF = (1, 63, 64, 65, 16384, 16385, 1048576, 1048577, 503808, 503809, 1 << 30)
DIM = (1, 32, 33, 512, 8192)
N_Q = (1, 511, 512, 513)


def test_gallery_plan_every_case(tmp_path):
    build = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", CSRC, "-s", "gallery_plan_check", "BUILD=" + build], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "gallery_plan_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = []
    for line in r.stdout.splitlines():
        left, right = line.split(" -> ")
        i = {k: int(v) for k, v in (f.split("=") for f in left.split())}
        o = {k: int(v) for k, v in (f.split("=") for f in right.split())}
        assert tuple(i) == IN_KEYS and tuple(o) == OUT_KEYS, line
        sh = ref.shape(i["n_ref"], i["dim"])
        want = dict(sh, row_bytes=ref.row_bytes(sh, i["cls"], i["sel"]), block_rows=ref.block_rows(sh, i["n_q"], i["cls"], i["sel"]))
        assert o == want, "%s\n  the former sums say %s" % (line, want)
        # what the three hand-written sums were protecting: a block never passes the scratch limit
        assert o["block_rows"] * o["row_bytes"] <= 2 ** 30, line
        # without a flag the limit over the row bytes never binds (the distances' share leaves 40 MiB for the rest): one formula serves
        if not i["cls"] and not i["sel"]:
            assert o["block_rows"] == min(i["n_q"], o["qb_max"]), line
        seen.append(tuple(i.values()))
    want_cases = {(n, d, q, c, s) for n in N_REF for d in DIM for q in N_Q for c in (0, 1) for s in (0, 1)}
    assert len(seen) == len(want_cases) and set(seen) == want_cases          # every case, once
    # the cases reach what they are there for: a gallery that fits no row, one whose blocks the per-row limit sets, not qb_max
    assert any(n == 1 << 30 for n, *_ in seen)
    sh = ref.shape(503808, 8192)
    assert sh["qb_max"] == 512 and ref.block_rows(sh, 512, 0, 1) < 512 and ref.shape(503809, 1)["qb_max"] == 511


def _code_lines(name):
    with open(os.path.join(CSRC, name)) as f:
        for n, line in enumerate(f, 1):
            yield n, line.split("//")[0]


def _sources():
    return [name for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h", ".cc"))]


def test_sizes_defined_once():
    """The limits, the RT_* sizes the arithmetic needs and the accumulator's size: one definition each in the tree, in the plan's header."""
    for const in ("GALLERY_SCRATCH_MAX", "GALLERY_DIST_MAX", "GALLERY_QB_MAX", "GALLERY_SEG_MAX", "GALLERY_ACC_BYTES", "RT_BK", "RT_CHUNK",
                  "RT_MAX_K", "RT_SEL_BINS", "RT_SEL_LAST_BINS"):
        # a definition: the name, then an initialiser ('=' but not '=='), or a macro of that name
        defs = [(name, n) for name in _sources() for n, code in _code_lines(name)
                if re.search(r"\b%s\s*=[^=]|#\s*define\s+%s\b" % (const, const), code)]
        assert len(defs) == 1 and defs[0][0] == "vv_gallery_plan.h", "%s: %s" % (const, defs)
    assert not any("LIN_SCRATCH_MAX" in code for name in _sources() for _, code in _code_lines(name))


def test_row_bytes_summed_in_the_header_only():
    """No .hip file adds up the bytes of a scratch row by itself: the partial keys' RT_MAX_K * 8 bytes, which every former sum carried,
    appear in the header's sum alone."""
    for name in _sources():
        if name.endswith(".hip"):
            for n, code in _code_lines(name):
                assert not re.search(r"RT_MAX_K\s*\*\s*8\b", code), "%s:%d sums scratch row bytes outside vv_gallery_plan.h: %s" % (name, n, code.strip())
    assert any(re.search(r"RT_MAX_K\s*\*\s*8\b", code) for _, code in _code_lines("vv_gallery_plan.h"))
