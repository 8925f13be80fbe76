"""The inverted-file index's plumbing and its block plan, without a GPU: the header's prototypes, the library's exports and the ctypes
binding agree on the new functions; videovector_amd/csrc/vv_ivf_plan.h builds with the host compiler alone, under the host sanitizers,
as a program of its own (tools/ivf_plan_check.cc), and every line it prints equals the restatement below."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovector_amd", "csrc")

import videovector_amd as vv   # noqa: E402
from videovector_amd import engine   # noqa: E402

NEW = {"vv_ivf_create": 7, "vv_ivf_destroy": 2, "vv_ivf_search": 9, "vv_ivf_get": 3, "vv_ivf_lists": 4}     # name: parameters
HDR = open(os.path.join(ROOT, "include", "videovec.h")).read()
GET_NAMES = ["n_ref", "dim", "num_clusters", "metric", "largest_list", "empty_lists", "last_blocks", "last_tiles", "last_candidates",
             "last_grid_wgs", "last_probe_ms", "last_group_ms", "last_sim_ms", "last_select_ms", "last_device_ms"]


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
        assert fn.restype is C.c_int, name
    assert "typedef struct vv_ivf vv_ivf;" in HDR
    block = HDR[HDR.index("inverted-file (IVF) index on a gallery"):HDR.index("typedef struct vv_ivf vv_ivf;")]
    assert "HAS NO REFERENCE COUNTERPART" in block
    # the index's own file and the coarse index's, which answers the names every index shares, together: every documented name compared
    # exactly once, nothing else compared; this index's own names in its own getter and in neither other file
    ivf_src, shared_src, pq_src = (open(os.path.join(CSRC, f)).read() for f in ("ivf.hip", "ivf_coarse.hip", "pq.hip"))
    for name in GET_NAMES:
        assert '"%s"' % name in block, name
        assert (ivf_src + shared_src).count('n == "%s"' % name) == 1, name
    assert sorted(re.findall(r'n == "([^"]*)"', ivf_src + shared_src)) == sorted(GET_NAMES)
    getter = ivf_src[ivf_src.index("int vv_ivf_get("):]
    getter = getter[:getter.index("\n}\n")]
    for name in ("last_tiles", "last_grid_wgs", "last_group_ms", "last_sim_ms"):
        assert getter.count('n == "%s"' % name) == 1 and '"%s"' % name not in shared_src + pq_src, name
    for opt in ("ivf_block_rows", "ivf_grid_wgs"):
        assert '"%s"' % opt in block, opt
        assert open(os.path.join(CSRC, "api.hip")).read().count('"%s"' % opt) == 1, opt
    assert list(inspect.signature(engine.Engine.ivf).parameters) == ["self", "items", "centroids", "metric", "assign"]
    assert inspect.signature(engine.Engine.ivf).parameters["metric"].default == "euclidean"
    assert list(inspect.signature(engine.KMeansResult.ivf).parameters) == ["self", "items"]
    assert list(inspect.signature(engine.IVFIndex.search).parameters) == ["self", "q", "k", "nprobe"]
    assert vv.IVFIndex is engine.IVFIndex and all(callable(getattr(engine.IVFIndex, f)) for f in ("lists", "get", "close"))
    # without a context nothing runs: the NULL checks come first and name the argument
    assert L.vv_ivf_create(None, None, None, 1, 0, None, None) == 1 and b"ctx is NULL" in L.vv_last_error()
    assert L.vv_ivf_search(None, None, None, 1, 1, 1, None, None, None) == 1 and b"ctx is NULL" in L.vv_last_error()
    v = C.c_double(-3.0)
    assert L.vv_ivf_get(None, b"n_ref", C.byref(v)) == 1 and v.value == -3.0
    assert L.vv_ivf_lists(None, None, None, None) == 1 and L.vv_ivf_destroy(None, None) == 1


# ---- the plan, restated
TILE, KM_TILE, KM_CHUNK, MAX_C, MAX_PROBE, MAX_K = 128, 1024, 256, 4096, 64, 32
LIMIT, GRID, GRID_MAX, ROWS_MAX, BUFFERS, ALIGN = 1 << 30, 512, 65535, 65536, 20, 256
TAIL = 40 + 16 + 8 + BUFFERS * ALIGN                 # the k-means record, the call's record, two counters, the buffers' alignment


def cdiv(a, b):
    return -(-a // b)


def tile_cap(rows, pitch, pairs, n, Cn):
    return cdiv(rows * pitch, TILE * TILE) + cdiv(pairs, TILE) + cdiv(n, TILE) + min(Cn, pairs)


def block_bytes(rows, pitch, Dp, Cn, nprobe, n):
    pairs = rows * nprobe
    return (rows * (Cn * 4 + Dp * 4 + pitch * 4 + 4 + MAX_K * 8) + pairs * 12 + cdiv(pairs, KM_TILE) * Cn * 4 +
            (pairs // KM_CHUNK + min(Cn, pairs)) * 16 + (3 * Cn + 2) * 4 + tile_cap(rows, pitch, pairs, n, Cn) * 16 + TAIL)


def plan(n, dim, Cn, nprobe, nq, items, force, grid):
    zero = dict(ok=0, Dp=0, pitch=0, block_rows=0, blocks=0, pairs=0, pair_tiles=0, max_chunks=0, tile_cap=0, grid_wgs=0, total=0)
    if n < 1 or dim < 1 or Cn < 1 or Cn > MAX_C or nq < 1 or items < 0 or items > n:
        return zero
    if nprobe < 1 or nprobe > Cn or (nprobe > MAX_PROBE and nprobe != Cn):
        return zero
    p = dict(zero)
    p["Dp"] = cdiv(dim, 32) * 32
    pitch = p["pitch"] = max(cdiv(items, 4) * 4, 4)
    p["grid_wgs"] = min(grid, GRID_MAX) if grid > 0 else GRID
    per_row = (Cn * 4 + p["Dp"] * 4 + pitch * 4 + 4 + MAX_K * 8 + nprobe * 12 + cdiv(nprobe * Cn * 4, KM_TILE) + cdiv(nprobe * 16, KM_CHUNK) +
               cdiv(pitch * 16, TILE * TILE) + cdiv(nprobe * 16, TILE))
    fixed = Cn * 4 + Cn * 16 + (3 * Cn + 2) * 4 + (cdiv(n, TILE) + 2 + Cn) * 16 + TAIL
    if fixed + per_row > LIMIT:
        return p
    rows = (LIMIT - fixed) // per_row
    if 0 < force < rows:
        rows = force
    rows = min(rows, ROWS_MAX, nq)
    pairs = rows * nprobe
    p.update(ok=1, block_rows=rows, blocks=cdiv(nq, rows), pairs=pairs, pair_tiles=cdiv(pairs, KM_TILE),
             max_chunks=pairs // KM_CHUNK + min(Cn, pairs), tile_cap=tile_cap(rows, pitch, pairs, n, Cn),
             total=block_bytes(rows, pitch, p["Dp"], Cn, nprobe, n))
    return p


def test_plan_every_case(tmp_path):
    build = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", CSRC, "-s", "ivf_plan_check", "BUILD=" + build, "SAN=-fsanitize=address,undefined"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "ivf_plan_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 8 * 3 * 6 * 5 * 4 * 4 * 4 + 4
    assert lines[-4:] == ["pitch_items nprobe=1 -> 300", "pitch_items nprobe=2 -> 429", "pitch_items nprobe=7 -> 700", "pitch_items nprobe=8 -> 700"]
    seen_fail = seen_cut = seen_many = seen_forced = 0
    for line in lines[:-4]:
        left, right = line.split(" -> ")
        i = {k: int(v) for k, v in (f.split("=") for f in left.split())}
        o = {k: int(v) for k, v in (f.split("=") for f in right.split())}
        want = plan(i["n"], i["dim"], i["C"], i["nprobe"], i["nq"], i["items"], i["force"], i["grid"])
        assert o == want, "%s\n  restated: %s" % (line, want)
        if o["ok"]:
            # what the plan is for: everything together within the limit, every query in exactly one block, a candidate row that holds
            # the nprobe largest lists on a 16-byte pitch, pairs that fit an int, a grid within its limit
            assert o["total"] <= LIMIT and (o["blocks"] - 1) * o["block_rows"] < i["nq"] <= o["blocks"] * o["block_rows"]
            assert o["pitch"] >= max(i["items"], 4) and o["pitch"] % 4 == 0 and o["pairs"] < 1 << 31 and 1 <= o["grid_wgs"] <= GRID_MAX
            assert o["tile_cap"] < 1 << 31 and o["tile_cap"] * TILE * TILE >= o["block_rows"] * i["items"]
            seen_many += o["blocks"] > 1
            seen_cut += o["block_rows"] < min(i["nq"], ROWS_MAX) and i["force"] == 0
            seen_forced += o["block_rows"] == i["force"]
        else:
            seen_fail += o["Dp"] > 0
    assert seen_fail and seen_cut and seen_many and seen_forced      # a row that does not fit, a block the limit cut, several blocks, a forced one
    # the shapes the GPU tests and the benchmark lean on
    assert plan(700, 64, 8, 2, 300, 429, 64, 0)["blocks"] == 5 and plan(700, 64, 8, 2, 300, 429, 0, 0)["blocks"] == 1
    big = plan(1000000, 512, 4096, 32, 4096, 32 * 1000, 0, 0)
    assert big["ok"] and big["blocks"] == 1 and big["total"] > LIMIT // 2
