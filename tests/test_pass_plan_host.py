"""The pass plan of videovector_amd/csrc/vv_pass_plan.h on the host: builds tools/pass_plan_check.cc with g++ (the header includes no HIP
header), runs it -- one line per combination of the options, dropout, forward-only, ablation and the edge shapes -- and compares every
line with the rules as restated below."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovector_amd", "csrc")

IN_KEYS = ("dedup", "seg_bwd", "drop_dedup", "h16", "h16_fallback", "v16", "ablate", "D", "C", "Nn", "dropout", "fwd_only")
OUT_KEYS = ("drop_on", "dd", "drop_rides_dd", "seg", "h16", "v16")


def expected(i):
    """The rules in words, from the comments of the step: k_seg_bwd holds a row of 512 or 1024 columns, so the segment-wise pair exists at
    those two widths, for de-duplicated batches, under option seg_bwd.  Dropout keeps a batch dense unless the pair carries the masks for
    its shape: drop_dedup 1 -- the register-resident score kernel's shapes only (D = 512, at most 6 context rows, at most 56 target /
    negative rows); 2 -- every shape of the pair; 0 -- none.  Ablation runs dense with fp32 rows.  f16 rows exist only where the pair
    reads them, and not once the guard has fallen back.  f16 per-item vectors: f16 rows at D = 1024 without dropout, and never in a
    forward-only pass, which writes none."""
    pair_shape = i["D"] in (512, 1024)
    resident_shape = i["D"] == 512 and i["C"] - 1 <= 6 and 1 + i["Nn"] <= 56
    masks_carried = bool(i["seg_bwd"]) and {0: False, 1: resident_shape, 2: pair_shape}[i["drop_dedup"]]
    o = {"drop_on": bool(i["dropout"])}
    o["dd"] = bool(i["dedup"]) and not i["ablate"] and (masks_carried if i["dropout"] else True)
    o["drop_rides_dd"] = o["dd"] and o["drop_on"]
    o["seg"] = o["dd"] and bool(i["seg_bwd"]) and pair_shape
    o["h16"] = o["seg"] and bool(i["h16"]) and not i["h16_fallback"]
    o["v16"] = o["h16"] and bool(i["v16"]) and i["D"] == 1024 and not i["dropout"] and not i["fwd_only"]
    return o


def test_pass_plan_every_case(tmp_path):
    build = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", CSRC, "-s", "pass_plan_check", "BUILD=" + build], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "pass_plan_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = set()
    for line in r.stdout.splitlines():
        left, right = line.split(" -> ")
        i = {k: int(v) for k, v in (f.split("=") for f in left.split())}
        o = {k: int(v) for k, v in (f.split("=") for f in right.split())}
        assert tuple(i) == IN_KEYS and tuple(o) == OUT_KEYS, line
        want = expected(i)
        assert {k: bool(v) for k, v in o.items()} == want, "%s\n  the rules say %s" % (line, want)
        seen.add(tuple(i.values()))
    # every combination, once: 8 on/off inputs, drop_dedup 0 / 1 / 2, and shapes on both sides of the register-resident kernel's limits
    # (C - 1 <= 6, 1 + Nn <= 56)
    want_cases = {(de, sb, dd, h, fb, v, ab, D, C, Nn, dr, fo)
                  for de in (0, 1) for sb in (0, 1) for dd in (0, 1, 2) for h in (0, 1) for fb in (0, 1) for v in (0, 1) for ab in (0, 1)
                  for D in (256, 512, 1024) for C in (2, 7, 8) for Nn in (1, 55, 56) for dr in (0, 1) for fo in (0, 1)}
    assert seen == want_cases and len(r.stdout.splitlines()) == len(want_cases)


def _code_lines(name):
    with open(os.path.join(CSRC, name)) as f:
        for n, line in enumerate(f, 1):
            yield n, line.split("//")[0]


def test_shape_rules_defined_once():
    """score_fwd_supported / score_fwd_dropout_supported: one definition each in the tree, in the plan's header."""
    for fn in ("score_fwd_supported", "score_fwd_dropout_supported"):
        defs = [(name, n) for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h", ".cc"))
                for n, code in _code_lines(name) if re.search(r"\bbool\s+%s\s*\(" % fn, code)]
        assert len(defs) == 1 and defs[0][0] == "vv_pass_plan.h", "%s: %s" % (fn, defs)


def test_plan_computed_through_the_header_only():
    """Neither pass.hip (the two passes, whose code left api.hip) nor ops.hip decides dd, seg or h16 from the options itself, or asks the shape
    predicates: both go through pass_plan (api.hip, solver.hip, retrieval.hip and classify.hip run no pass)."""
    old = re.compile(r"c->dedup\s*&&|c->seg_bwd\s*&&|c->h16\s*&&|&&\s*c->(dedup|seg_bwd|h16)\b|\bscore_fwd_(dropout_)?supported\s*\(")
    for name in ("api.hip", "pass.hip", "solver.hip", "ops.hip", "retrieval.hip", "classify.hip"):
        for n, code in _code_lines(name):
            assert not old.search(code), "%s:%d decides the pass's execution outside vv_pass_plan.h: %s" % (name, n, code.strip())
