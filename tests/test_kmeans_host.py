"""k-means' plumbing and its block plan, without a GPU: the header's prototypes, the library's exports and the ctypes binding agree on
the new functions and structures; vv_kmeans_init_rows is the head of vv_rows_shuffled's one epoch and refuses what it must;
videovector_amd/csrc/vv_kmeans_plan.h builds with the host compiler alone, under the host sanitizers, as a program of its own
(tools/kmeans_plan_check.cc), and every line it prints equals the restatement below."""
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

NEW = {"vv_gallery_kmeans": 11, "vv_kmeans_init_rows": 4, "vv_kmeans_cfg_default": 1}     # name: parameters
HDR = open(os.path.join(ROOT, "include", "videovec.h")).read()


def test_header_library_and_binding_agree():
    lib = engine.lib_path()
    assert os.path.exists(lib), "build the library first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vv_[a-z0-9_]+)$", out, re.M))
    L = engine.load_library()
    for name, nargs in NEW.items():
        proto = re.search(r"^(int|void) %s\(([^;]*)\);" % name, HDR, re.M | re.S)
        assert proto, name
        assert len(proto.group(2).split(",")) == nargs, name
        assert name in exported, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert fn.restype is (None if proto.group(1) == "void" else C.c_int), name
    assert re.search(r"enum \{ VV_KMEANS_EUCLIDEAN = 0, VV_KMEANS_SPHERICAL = 1 \};", HDR)
    assert engine.KMEANS_METRICS == {"euclidean": 0, "spherical": 1}
    block = HDR[HDR.index("k-means clustering of a gallery"):HDR.index("enum { VV_KMEANS_EUCLIDEAN")]
    assert "HAS NO REFERENCE COUNTERPART" in block
    for opt in ("km_block_rows", "last_km_blocks", "last_km_chunks", "last_km_assign_form", "last_km_sim_ms", "last_km_assign_ms",
                "last_km_group_ms", "last_km_update_ms"):
        assert '"%s"' % opt in block, opt
        assert open(os.path.join(CSRC, "api.hip")).read().count('"%s"' % opt) == 1, opt
    # the structures: the header's fields in the header's order and widths
    assert [f for f, _ in engine._KmeansCfg._fields_] == ["num_clusters", "iters", "metric", "reserved_"] and C.sizeof(engine._KmeansCfg) == 16
    assert [f for f, _ in engine._KmeansReport._fields_] == ["n", "num_clusters", "iters", "empty_last", "degenerate_last", "moved_last",
                                                             "objective_last", "nonfinite_rows"]
    assert C.sizeof(engine._KmeansReport) == 48 and engine._KmeansReport.moved_last.offset == 24
    assert list(inspect.signature(engine.Gallery.kmeans).parameters) == ["self", "num_clusters", "iters", "metric", "init", "seed"]
    assert vv.kmeans_init_rows is engine.kmeans_init_rows and callable(engine.KMeansResult.gallery)
    cfg = engine._KmeansCfg(7, 7, 7, 7)
    L.vv_kmeans_cfg_default(C.byref(cfg))
    assert (cfg.num_clusters, cfg.iters, cfg.metric, cfg.reserved_) == (0, 20, 0, 0)


@pytest.mark.parametrize("seed,n,k", [(0, 1, 1), (5, 10, 10), (2 ** 63 + 9, 1000, 37), (77, 70001, 4096)])
def test_init_rows_are_the_head_of_one_shuffled_epoch(seed, n, k):
    rows = vv.kmeans_init_rows(seed, n, k)
    assert rows.dtype == np.int32 and np.array_equal(rows, vv.rows_shuffled(seed, n, 1)[:k])
    assert len(set(rows.tolist())) == k and rows.min() >= 0 and rows.max() < n


def test_init_rows_refusals_write_nothing():
    L = engine.load_library()
    out = np.full(8, -9, np.int32)
    for n, k in [(0, 1), (-1, 1), (5, 0), (5, 6), (5, -2)]:
        assert L.vv_kmeans_init_rows(1, n, k, out.ctypes.data_as(C.c_void_p)) == 1
        assert b"vv_kmeans_init_rows" in L.vv_last_error() and (out == -9).all()
    assert L.vv_kmeans_init_rows(1, 5, 2, None) == 1


# ---- the plan, restated
CHUNK, SLOT, TILE, SLICE, MAX_C = 256, 64, 1024, 512, 4096
LIMIT, TARGET = 1 << 30, 64 << 20


def plan(n, dim, Cn, force):
    zero = dict(ok=0, Dp=0, block_rows=0, blocks=0, tiles=0, slots=0, max_chunks=0, slices=0, score=0, item=0, partial=0, total=0)
    if n < 1 or dim < 1 or Cn < 1 or Cn > MAX_C:
        return zero
    p = dict(zero)
    p["Dp"] = -(-dim // 32) * 32
    p["tiles"], p["slots"] = -(-n // TILE), -(-n // SLOT)
    p["max_chunks"] = n // CHUNK + min(Cn, n)
    p["slices"] = -(-p["Dp"] // SLICE)
    p["item"] = n * 8 + p["tiles"] * Cn * 4 + p["slots"] * 8 + Cn * p["Dp"] * 4 + Cn * 24 + p["max_chunks"] * 16 + 4096
    p["partial"] = p["max_chunks"] * p["Dp"] * 4
    fixed, row = p["item"] + p["partial"], Cn * 4
    if fixed + row * SLOT > LIMIT:
        return p
    rows = -(-force // SLOT) * SLOT if force > 0 else TARGET // row // SLOT * SLOT
    rows = min(max(rows, SLOT), -(-n // SLOT) * SLOT, (LIMIT - fixed) // row // SLOT * SLOT, 1 << 24)
    p.update(ok=1, block_rows=rows, blocks=-(-n // rows), score=rows * row, total=fixed + rows * row)
    return p


def test_plan_every_case(tmp_path):
    build = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", CSRC, "-s", "kmeans_plan_check", "BUILD=" + build, "SAN=-fsanitize=address,undefined"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "kmeans_plan_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 17 * 5 * 6 * 6
    seen_fail = seen_cut = seen_many = 0
    for line in lines:
        left, right = line.split(" -> ")
        i = {k: int(v) for k, v in (f.split("=") for f in left.split())}
        o = {k: int(v) for k, v in (f.split("=") for f in right.split())}
        want = plan(i["n"], i["dim"], i["C"], i["force"])
        assert o == want, "%s\n  restated: %s" % (line, want)
        if o["ok"]:
            # what the plan is for: everything together within the limit, whole slots, every item in exactly one block
            assert o["total"] <= LIMIT and o["block_rows"] % SLOT == 0 and (o["blocks"] - 1) * o["block_rows"] < i["n"] <= o["blocks"] * o["block_rows"]
            seen_many += o["blocks"] > 1
            seen_cut += o["score"] < min(TARGET // (i["C"] * 4 * SLOT) * SLOT, -(-i["n"] // SLOT) * SLOT) * i["C"] * 4 and i["force"] == 0
        else:
            seen_fail += i["C"] <= MAX_C
    assert seen_fail and seen_cut and seen_many          # the cases reach a refusal, a block the limit cut, and several blocks
    assert plan(1000, 40, 6, 64)["blocks"] == 16 and plan(1000, 40, 6, 0)["blocks"] == 1      # (tests/test_gpu_kmeans.py leans on these)
    big = plan(1000000, 512, 4096, 0)
    assert big["ok"] and big["block_rows"] == 4096 and big["total"] < LIMIT // 4
