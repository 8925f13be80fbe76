"""The option table of csrc/api.hip (kOptions) on the host: every name of the option surface that tests/test_gpu_options.py carries is
written once in the library's sources -- one row, no second list of read-only names, no chain of comparisons beside it.  The labels
of vv_profile_get's timed launches (the second argument of PROFILED) are names of another kind -- one of them, "dedup", is also an
option's -- and are left out of the count."""
import glob
import os
import re

from tests.test_gpu_options import LAB, READ_ONLY, RETIRED, SETTABLE

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "videovector_amd", "csrc")


def test_every_option_name_is_one_string_literal():
    code = ""
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        # a // comment starts outside a string literal: drop it, keep the literals
        code += "\n".join(re.match(r'((?:[^"/]|"(?:[^"\\]|\\.)*"|/(?!/))*)', line).group(1) for line in text.split("\n")) + "\n"
    code = re.sub(r'\bPROFILED\(c, "\w+"', "PROFILED(c, label", code)
    names = list(SETTABLE) + list(READ_ONLY) + list(RETIRED) + list(LAB)
    assert len(names) == len(set(names)) == 55
    for name in names:
        assert len(re.findall('"%s"' % re.escape(name), code)) == 1, name
