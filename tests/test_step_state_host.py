"""The gradient / update-sync states of videovector_amd/csrc/vv_step_state.h on the host: builds tools/step_state_check.cc with g++ (the
header includes no HIP header) and runs it -- every (state, transition) pair, the whole resulting state, the guard's answers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovector_amd", "csrc")


def test_step_state_transitions(tmp_path):
    build = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", CSRC, "-s", "step_state_check", "BUILD=" + build], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "step_state_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout, r.stdout


def test_state_written_through_transitions_only():
    """No raw assignment to the two states outside the header: api.hip, pass.hip (the pass) and solver.hip (the update), whose code left api.hip, and ops.hip go
    through its transitions (retrieval.hip and classify.hip, whose code left api.hip too, touch neither state)."""
    import re
    raw = re.compile(r"(->|\.)(grad(\.(at|buf(\.\w+)?))?|upd_sync)\s*(=[^=]|\+\+|--)")
    for name in ("api.hip", "pass.hip", "solver.hip", "ops.hip", "comm.hip", "retrieval.hip", "classify.hip"):
        with open(os.path.join(CSRC, name)) as f:
            for n, line in enumerate(f, 1):
                assert not raw.search(line.split("//")[0]), "%s:%d assigns to the state directly: %s" % (name, n, line.strip())
