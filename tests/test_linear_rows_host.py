"""The row lists' plumbing and their definition, without a GPU: the header's prototypes, the library's exports and the ctypes binding
agree on the five new functions; a pure-Python restatement of videovector_amd/csrc/vv_rows.h's rule (splitmix64, Fisher-Yates from the
top, j = the high 64 bits of next() * (i + 1)) reproduces vv_rows_shuffled and vv_rows_fold; the argument errors; tools/rows_check.cc
builds with the host sanitizers, as a program of its own, and exits 0."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovector_amd", "csrc")

import videovector_amd as vv   # noqa: E402
from videovector_amd import engine   # noqa: E402

NEW = {"vv_linear_fit_rows": 10, "vv_linear_grad_rows": 10, "vv_linear_scores_rows": 6, "vv_rows_shuffled": 4, "vv_rows_fold": 8}   # name: parameters
HDR = open(os.path.join(ROOT, "include", "videovec.h")).read()
M64 = (1 << 64) - 1


def test_header_library_and_binding_agree():
    lib = engine.lib_path()
    assert os.path.exists(lib), "build the library first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vv_[a-z0-9_]+)$", out, re.M))
    L = engine.load_library()
    for name, nargs in NEW.items():
        proto = re.search(r"^int %s\(([^;]*)\);" % name, HDR, re.M | re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == nargs, name
        assert name in exported, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    assert list(L.vv_linear_scores_rows.argtypes) == [vp, vp, vp, vp, i64, vp]
    assert list(L.vv_linear_grad_rows.argtypes) == [vp, vp, vp, vp, vp, i64, f32, vp, vp, C.POINTER(f32)]
    assert list(L.vv_rows_shuffled.argtypes) == [C.c_uint64, i32, i32, vp]
    assert list(L.vv_rows_fold.argtypes) == [C.c_uint64, i32, i32, i32, vp, C.POINTER(i64), vp, C.POINTER(i64)]
    assert {"rows", "epochs", "shuffle_seed"} <= set(inspect.signature(engine.Linear.fit).parameters)
    assert "rows" in inspect.signature(engine.Linear.grad).parameters and "rows" in inspect.signature(engine.Linear.scores).parameters
    assert callable(engine.Linear.cross_validate) and vv.rows_shuffled is engine.rows_shuffled and vv.rows_fold is engine.rows_fold
    # the option is read-only and the header names it; the data-order cite is data_layer.cpp's cursor
    assert '"last_lin_gather"' in HDR and re.search(r"data_layer\.cpp:\d+", HDR) and "this project's own" in HDR


# ---- the rule, restated from the header's comment
def splitmix64(seed):
    state = seed & M64
    while True:
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        yield z ^ (z >> 31)


def shuffled(seed, n, epochs):
    rng, out = splitmix64(seed), []
    for _ in range(epochs):
        p = list(range(n))
        for i in range(n - 1, 0, -1):
            j = (next(rng) * (i + 1)) >> 64
            p[i], p[j] = p[j], p[i]
        out += p
    return out


def fold(seed, n, folds, f):
    perm = shuffled(seed, n, 1)
    lo, hi = f * n // folds, (f + 1) * n // folds
    return perm[:lo] + perm[hi:], perm[lo:hi]


def test_the_constants_are_the_headers():
    text = open(os.path.join(CSRC, "vv_rows.h")).read()
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert text.count(const) >= 2                                     # the stated rule and the code
    assert next(splitmix64(0)) == 0xE220A8397B1DCDAF                      # splitmix64's published first output for seed 0


@pytest.mark.parametrize("seed", [0, 1, 7, 2 ** 63 + 5, M64])
def test_python_restatement_reproduces_the_lists(seed):
    for n, epochs in ((1, 1), (1, 3), (2, 1), (2, 4), (3, 2), (17, 3), (300, 2), (1000, 1)):
        got = vv.rows_shuffled(seed, n, epochs)
        assert got.dtype == np.int32 and got.tolist() == shuffled(seed, n, epochs), (n, epochs)
        for e in range(epochs):
            assert sorted(got[e * n:(e + 1) * n].tolist()) == list(range(n))
    for n, folds in ((2, 2), (3, 2), (3, 3), (10, 3), (10, 10), (17, 5), (300, 7)):   # folds = n included
        seen = []
        for f in range(folds):
            train, held = vv.rows_fold(seed, n, folds, f)
            want_train, want_held = fold(seed, n, folds, f)
            assert train.tolist() == want_train and held.tolist() == want_held, (n, folds, f)
            assert len(held) >= 1 and sorted(train.tolist() + held.tolist()) == list(range(n))
            seen += held.tolist()
        assert sorted(seen) == list(range(n))                             # the folds partition the items


def test_argument_errors():
    buf = np.full(8, -9, np.int32)
    L = engine.load_library()
    nt, nh = C.c_int64(-9), C.c_int64(-9)
    p = engine._ptr(buf)
    bad = [lambda: L.vv_rows_shuffled(1, 0, 1, p), lambda: L.vv_rows_shuffled(1, -1, 1, p), lambda: L.vv_rows_shuffled(1, 4, 0, p),
           lambda: L.vv_rows_shuffled(1, 4, 1, None),
           lambda: L.vv_rows_fold(1, 0, 2, 0, p, C.byref(nt), p, C.byref(nh)), lambda: L.vv_rows_fold(1, 4, 1, 0, p, C.byref(nt), p, C.byref(nh)),
           lambda: L.vv_rows_fold(1, 4, 5, 0, p, C.byref(nt), p, C.byref(nh)), lambda: L.vv_rows_fold(1, 4, 2, 2, p, C.byref(nt), p, C.byref(nh)),
           lambda: L.vv_rows_fold(1, 4, 2, -1, p, C.byref(nt), p, C.byref(nh)), lambda: L.vv_rows_fold(1, 4, 2, 0, None, C.byref(nt), p, C.byref(nh))]
    for call in bad:
        assert call() == 1                                                # VV_ERR_ARG
        assert L.vv_last_error().startswith(b"vv_rows_")
    assert (buf == -9).all() and nt.value == -9 and nh.value == -9        # a refused call wrote nothing
    for call in (lambda: vv.rows_shuffled(1, 0, 1), lambda: vv.rows_shuffled(1, 5, 0), lambda: vv.rows_fold(1, 5, 1, 0),
                 lambda: vv.rows_fold(1, 5, 6, 0), lambda: vv.rows_fold(1, 5, 2, 2)):
        with pytest.raises(vv.VVError) as e:
            call()
        assert e.value.code == 1


def test_rows_check_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (its own main) built with -fsanitize=address,undefined and run on the CPU; nothing loaded into Python is
    instrumented."""
    build = str(tmp_path / "build")
    san = "SAN=-fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan"      # (the runtimes inside the program)
    r = subprocess.run(["make", "-C", CSRC, "-s", "rows_check", "BUILD=" + build, san], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "rows_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^\d+ cases, 0 failed$", r.stdout.strip(), re.M) and "runtime error" not in r.stderr
