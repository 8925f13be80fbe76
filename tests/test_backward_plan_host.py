"""The backward half's host decisions (videovector_amd/csrc/vv_backward_plan.h) on the host: builds tools/backward_plan_check.cc with g++
(the header includes no HIP header), runs it -- one line per case of split_k_plan, chunk_plan and backward_plan -- and compares every
line with the rules as restated in tests/backward_plan_ref.py.  Then two readings of the sources: the options the plan combines are
combined nowhere else, and the host's spin-wait is written once."""
import itertools
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovector_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import backward_plan_ref as ref   # noqa: E402

IN_KEYS = ("world", "comm_sharded", "comm_overlap", "D", "F", "Dp", "Fp", "Rp", "B", "S", "grads_own", "grads_exposed", "fuse_update",
           "wgrad_update", "slab16", "wgrad_lean", "guard_proactive", "fuse_keep_grads", "can_fuse_update", "hinted", "hint_adam", "hint_clip",
           "f16", "dd", "seg", "table_rows", "wmax_slots")
OUT_KEYS = ("shard_rows", "sharded", "chunked", "lazy", "fuse_w", "slab16", "lean", "proactive", "n_rounds", "n_of0", "n_of1")
BASE = dict(world=0, comm_sharded=0, comm_overlap=0, D=256, F=256, Dp=256, Fp=256, Rp=512, B=64, S=8, grads_own=1, grads_exposed=0,
            fuse_update=1, wgrad_update=1, slab16=1, wgrad_lean=1, guard_proactive=1, fuse_keep_grads=0, can_fuse_update=1, hinted=0,
            hint_adam=0, hint_clip=0, f16=1, dd=1, seg=1, table_rows=2049, wmax_slots=2048)
F_SET, D_SET, S_SET, WORLDS = (252, 254, 256, 260, 4096), (256, 258, 4096), (1, 2, 8, 9), (0, 1, 2, 3, 8)
NK_SET = (1, 7, 8, 15, 16, 31, 32, 64, 65)


def _case(group, **kw):
    c = dict(BASE, **kw)
    if "D" in kw:
        c["Dp"] = ref.pad(c["D"])
    if "F" in kw and "Fp" not in kw:
        c["Fp"] = ref.pad(c["F"])
    return (group,) + tuple(c[k] for k in IN_KEYS)


def intended_cases():
    """The case set of the tool's header, group by group."""
    bools = lambda n: itertools.product((0, 1), repeat=n)   # noqa: E731
    want = set()
    for world, (sh, ov, own, ex, fu), F, D, S, wmax in itertools.product(WORLDS, bools(5), F_SET, D_SET, S_SET, (2048, 1023)):
        want.add(_case("dest", world=world, comm_sharded=sh, comm_overlap=ov, grads_own=own, grads_exposed=ex, fuse_update=fu, F=F, D=D, S=S,
                       wmax_slots=wmax))
    for b, S, F, (D, wmax) in itertools.product(bools(11), S_SET, F_SET, ((256, 2048), (4096, 2048), (4096, 255))):
        want.add(_case("fuse", hinted=b[0], wgrad_update=b[1], can_fuse_update=b[2], fuse_keep_grads=b[3], hint_adam=b[4], hint_clip=b[5],
                       slab16=b[6], fuse_update=b[7], world=b[8], grads_exposed=b[9], grads_own=b[10], S=S, F=F, D=D, wmax_slots=wmax))
    for lean, rows, Fp in itertools.product((0, 1), (255, 256, 257, 8388591, 8388592, 16777215, 16777216), (64, 256, 8388352, 8388608)):
        want.add(_case("lean", wgrad_lean=lean, table_rows=rows, F=Fp, Fp=Fp))
    for (f16, dd, seg, pro), B, Rp in itertools.product(bools(4), (64, 65), (512, 768)):
        want.add(_case("guard", f16=f16, dd=dd, seg=seg, guard_proactive=pro, B=B, Rp=Rp))
    return want


def _run_tool(tmp, san=""):
    build = str(tmp / ("build_san" if san else "build"))
    r = subprocess.run(["make", "-C", CSRC, "-s", "backward_plan_check", "BUILD=" + build] + (["SAN=" + san] if san else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "backward_plan_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def _parse(line):
    left, right = line.split(" -> ")
    i = dict(f.split("=") for f in left.split())
    fn, group = i.pop("fn"), i.pop("group", None)
    return fn, group, {k: int(v) for k, v in i.items()}, {k: int(v) for k, v in (f.split("=") for f in right.split())}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    return _run_tool(tmp_path_factory.mktemp("backward_plan"))


def test_backward_plan_every_case(lines):
    seen, n_lines = set(), 0
    values = {k: set() for k in OUT_KEYS}
    split_seen, chunk_seen = set(), set()
    for line in lines:
        fn, group, i, o = _parse(line)
        if fn == "backward_plan":
            assert tuple(i) == IN_KEYS and tuple(o) == OUT_KEYS, line
            want = ref.backward(i, i["wmax_slots"])
            assert o == want, "%s\n  the rules say %s" % (line, want)
            seen.add((group,) + tuple(i.values()))
            n_lines += 1
            for k in OUT_KEYS:
                values[k].add(o[k])
        elif fn == "split_k_plan":
            assert (o["S"], o["kps"]) == ref.split_k(i["Dp"], i["Fp"], i["Rp"]), line
            assert 1 <= o["S"] <= max(1, i["Rp"] // ref.BK) and o["S"] * o["kps"] >= i["Rp"] // ref.BK, line      # every K-step is somebody's
            split_seen.add(tuple(i.values()))
        else:
            assert fn == "chunk_plan", line
            n = o["n"]
            kt = [o["kt%d" % k] for k in range(n + 1)]
            assert kt == ref.chunks(i["nk"], i["n_chunks"]), line
            # the stated properties, directly
            assert 1 <= n <= i["n_chunks"], line
            assert kt[0] == 0 and kt[-1] == i["nk"], line
            assert all(k % 2 == 0 for k in kt[:-1]), line                      # (the last boundary is the end of F, whatever its parity)
            widths = [b - a for a, b in zip(kt, kt[1:])]
            assert n == 1 or all(w >= 4 for w in widths), line
            assert all(a >= b for a, b in zip(widths, widths[1:])), line
            chunk_seen.add(tuple(i.values()))
    want_cases = intended_cases()
    assert seen == want_cases and n_lines == len(want_cases)
    assert split_seen == set(itertools.product((256, 512, 4096), (256, 512, 4096), (256, 512, 768, 8192)))
    assert chunk_seen == set(itertools.product(NK_SET, (1, 2, 3, 4)))
    assert len(lines) == len(want_cases) + len(split_seen) + len(chunk_seen)
    # no output's expression loses a side: every output takes at least two values over the cases
    assert all(len(v) >= 2 for v in values.values()), values


def test_backward_plan_tool_under_sanitizers(lines, tmp_path):
    """The stand-alone tool built with AddressSanitizer + UBSan (chunk_plan writes kt[0 .. n] of a 5-element array): runs clean, same output."""
    assert _run_tool(tmp_path, "-fsanitize=address,undefined") == lines


def _code_lines(name):
    with open(os.path.join(CSRC, name)) as f:
        for n, line in enumerate(f, 1):
            yield n, line.split("//")[0]


def test_backward_options_combined_in_the_plan_only():
    """c->grads_exposed, c->fuse_update, c->comm_sharded, c->comm_overlap and c->slab16 are not combined with && anywhere in pass.hip, api.hip
    or ops.hip: plan_backward copies them into BackwardPlanIn (plain assignments) and the header decides.  (solver.hip's schedule refusals
    combine the two comm_* flags with || and are not meant.)"""
    flag = r"c->(grads_exposed|fuse_update|comm_sharded|comm_overlap|slab16)\b"
    old = re.compile(r"%s\s*&&|&&\s*!?\s*%s" % (flag, flag))
    for name in ("pass.hip", "api.hip", "ops.hip"):
        for n, code in _code_lines(name):
            assert not old.search(code), "%s:%d combines a backward-plan option outside vv_backward_plan.h: %s" % (name, n, code.strip())
    filled = [n for n, code in _code_lines("pass.hip") if re.search(r"\bin\.\w+\s*=\s*" + flag, code)]
    assert filled, "plan_backward no longer fills BackwardPlanIn from the context"


def test_host_spin_wait_written_once():
    hits = [(name, n) for name in ("api.hip", "pass.hip") for n, code in _code_lines(name) if "nanosleep" in code]
    assert len(hits) == 1 and hits[0][0] == "pass.hip", hits
