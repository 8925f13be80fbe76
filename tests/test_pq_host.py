"""Product quantisation's plumbing, limits and block plan, without a GPU: the header's prototypes, the library's exports and the ctypes
binding agree on the new functions; videovector_amd/csrc/vv_pq_plan.h builds with the host compiler alone, under the host sanitizers,
as a program of its own (tools/pq_plan_check.cc), and every line it prints equals the restatement below."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovector_amd", "csrc")

import videovector_amd as vv   # noqa: E402
from videovector_amd import engine   # noqa: E402

NEW = {"vv_pq_train": 8, "vv_pq_encode": 6, "vv_ivfpq_create": 10, "vv_ivfpq_destroy": 2, "vv_ivfpq_search": 9, "vv_ivfpq_get": 3,
       "vv_ivfpq_lists": 4, "vv_ivfpq_codes": 3}     # name: parameters
HDR = open(os.path.join(ROOT, "include", "videovec.h")).read()
GET_NAMES = ["n_ref", "dim", "num_clusters", "metric", "M", "ksub", "largest_list", "empty_lists", "index_bytes", "last_blocks",
             "last_candidates", "last_scan_form", "last_probe_ms", "last_lut_ms", "last_scan_ms", "last_select_ms", "last_device_ms"]


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
    assert "vv_kmeans_rows" not in exported                       # the factored k-means body stays internal
    assert "typedef struct vv_ivfpq vv_ivfpq;" in HDR
    ivf_end = HDR.index("int vv_ivf_lists(")
    block = HDR[HDR.index("product-quantised lists (IVF-PQ)"):HDR.index("typedef struct vv_ivfpq vv_ivfpq;")]
    assert HDR.index("product-quantised lists (IVF-PQ)") > ivf_end           # the block follows the IVF block
    assert "HAS NO REFERENCE COUNTERPART" in block
    # the arithmetic is stated: the table's store, the chain's start, both chains, the limits, what is out of scope
    for phrase in ("-2.0f * s + 0.0f", "+0.0f", "rounded on its own", "acc = lut(i, 0, code[g][0])", "acc = acc + lut(i, m, code[g][m])",
                   "vv_kmeans_init_rows(seed + m, n_ref, ksub)", "iters = 0", "1 <= M <= 64", "dim % M == 0", "2 <= ksub <= 256",
                   "M * ksub * 4 <= 65536", "Not residual", "k_pq_lut", "ascending g"):
        assert phrase in block, phrase
    # the index's own file and the coarse index's, which answers the names every index shares, together: every documented name compared
    # exactly once, nothing else compared; this index's own names in its own getter and in neither other file
    pq_src, shared_src, ivf_src = (open(os.path.join(CSRC, f)).read() for f in ("pq.hip", "ivf_coarse.hip", "ivf.hip"))
    for name in GET_NAMES:
        assert '"%s"' % name in block, name
        assert (pq_src + shared_src).count('n == "%s"' % name) == 1, name
    assert (pq_src + shared_src).count('n == "') == len(GET_NAMES)
    assert sorted(re.findall(r'n == "([^"]*)"', pq_src + shared_src)) == sorted(GET_NAMES)
    getter = pq_src[pq_src.index("int vv_ivfpq_get("):]
    getter = getter[:getter.index("\n}\n")]
    for name in ("M", "ksub", "index_bytes", "last_scan_form", "last_lut_ms", "last_scan_ms"):
        assert getter.count('n == "%s"' % name) == 1 and '"%s"' % name not in shared_src + ivf_src, name
    assert '"ivf_block_rows"' in block
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(BUILD)/kernels_pq.o" in mk and "$(BUILD)/pq.o" in mk and "vv_pq_plan.h" in mk
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert sig(engine.Engine.pq_train) == ["self", "items", "M", "ksub", "iters", "seed"]
    assert sig(engine.Engine.pq_encode) == ["self", "items", "codebooks"]
    assert sig(engine.Engine.ivfpq) == ["self", "items", "centroids", "codebooks", "metric", "assign"]
    assert inspect.signature(engine.Engine.ivfpq).parameters["metric"].default == "euclidean"
    assert sig(engine.KMeansResult.ivfpq) == ["self", "items", "codebooks"]
    assert sig(engine.IVFPQIndex.search) == ["self", "q", "k", "nprobe"]
    assert vv.IVFPQIndex is engine.IVFPQIndex and all(callable(getattr(engine.IVFPQIndex, f)) for f in ("lists", "codes", "get", "close"))
    # without a context nothing runs: the NULL checks come first and name the argument
    assert L.vv_pq_train(None, None, 1, 2, 0, 0, None, None) == 1 and b"ctx is NULL" in L.vv_last_error()
    assert L.vv_pq_encode(None, None, None, 1, 2, None) == 1 and b"ctx is NULL" in L.vv_last_error()
    assert L.vv_ivfpq_create(None, None, None, 1, 0, None, None, 1, 2, None) == 1 and b"ctx is NULL" in L.vv_last_error()
    assert L.vv_ivfpq_search(None, None, None, 1, 1, 1, None, None, None) == 1 and b"ctx is NULL" in L.vv_last_error()
    v = C.c_double(-3.0)
    assert L.vv_ivfpq_get(None, b"n_ref", C.byref(v)) == 1 and v.value == -3.0
    assert L.vv_ivfpq_lists(None, None, None, None) == 1 and L.vv_ivfpq_codes(None, None, None) == 1 and L.vv_ivfpq_destroy(None, None) == 1


# ---- the limits and the plan, restated
MAX_M, MAX_KSUB, LDS, MAX_C, MAX_PROBE, MAX_K = 64, 256, 65536, 4096, 64, 32
LIMIT, ROWS_MAX, BUFFERS, ALIGN, REC = 1 << 30, 65536, 12, 256, 16


def cdiv(a, b):
    return -(-a // b)


def shape_error(dim, M, ksub):
    if M < 1 or M > MAX_M:
        return 1
    if dim < 1 or dim % M:
        return 2
    if ksub < 2 or ksub > MAX_KSUB:
        return 3
    if M * ksub * 4 > LDS:
        return 4
    return 0


def form(M):
    return 1 if M % 16 == 0 else 2 if M % 4 == 0 else 3


def block_bytes(rows, pitch, Dp, Cn, nprobe, table):
    # per row: probe scores, padded query, table, candidates, m, the k <= 32 results (idx and dist), the pairs' cluster and offset
    return rows * (Cn * 4 + Dp * 4 + table * 4 + pitch * 4 + 4 + MAX_K * 8 + nprobe * 8) + Cn * 4 + REC + BUFFERS * ALIGN


def plan(n, dim, Cn, nprobe, nq, items, M, ksub, force):
    zero = dict(ok=0, Dp=0, dsub=0, form=0, table=0, pitch=0, block_rows=0, blocks=0, pairs=0, total=0)
    if n < 1 or dim < 1 or Cn < 1 or Cn > MAX_C or nq < 1 or items < 0 or items > n:
        return zero
    if nprobe < 1 or nprobe > Cn or (nprobe > MAX_PROBE and nprobe != Cn):
        return zero
    if shape_error(dim, M, ksub):
        return zero
    p = dict(zero)
    p.update(Dp=cdiv(dim, 32) * 32, dsub=dim // M, form=form(M), table=cdiv(M * ksub, 4) * 4, pitch=max(cdiv(items, 4) * 4, 4))
    fixed = block_bytes(0, p["pitch"], p["Dp"], Cn, nprobe, p["table"])
    per_row = block_bytes(1, p["pitch"], p["Dp"], Cn, nprobe, p["table"]) - fixed
    if fixed + per_row > LIMIT:
        return p
    rows = (LIMIT - fixed) // per_row
    if 0 < force < rows:
        rows = force
    rows = min(rows, ROWS_MAX, nq)
    p.update(ok=1, block_rows=rows, blocks=cdiv(nq, rows), pairs=rows * nprobe,
             total=block_bytes(rows, p["pitch"], p["Dp"], Cn, nprobe, p["table"]))
    return p


def test_plan_every_case(tmp_path):
    build = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", CSRC, "-s", "pq_plan_check", "BUILD=" + build, "SAN=-fsanitize=address,undefined"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(build, "pq_plan_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    shapes = 7 * 6 * 4
    assert len(lines) == shapes * (1 + 3 * 4 * 5 * 4 * 4)
    errors, forms = set(), set()
    seen_fail = seen_cut = seen_many = seen_forced = seen_full = 0
    for line in lines:
        left, right = line.split(" -> ")
        if left.startswith("shape "):
            i = {k: int(v) for k, v in (f.split("=") for f in left.split()[1:])}
            o = {k: int(v) for k, v in (f.split("=") for f in right.split())}
            err = shape_error(i["dim"], i["M"], i["ksub"])
            assert o["error"] == err, line
            if i["M"] > 0:
                assert o["form"] == form(i["M"]) and o["row"] == i["M"] and o["row"] % {1: 16, 2: 4, 3: 1}[o["form"]] == 0, line
            if not err:
                # what the limits are for: a whole table in LDS on a 16-byte pitch, a code in one byte
                assert o["table"] == cdiv(i["M"] * i["ksub"], 4) * 4 and o["table"] * 4 <= LDS and i["ksub"] - 1 <= 255, line
                forms.add(o["form"])
                seen_full += o["table"] * 4 == LDS
            errors.add(err)
            continue
        i = {k: int(v) for k, v in (f.split("=") for f in left.split())}
        o = {k: int(v) for k, v in (f.split("=") for f in right.split())}
        want = plan(i["n"], i["dim"], i["C"], i["nprobe"], i["nq"], i["items"], i["M"], i["ksub"], i["force"])
        assert o == want, "%s\n  restated: %s" % (line, want)
        if o["ok"]:
            assert o["total"] <= LIMIT and (o["blocks"] - 1) * o["block_rows"] < i["nq"] <= o["blocks"] * o["block_rows"]
            assert o["pitch"] >= max(i["items"], 4) and o["pitch"] % 4 == 0 and o["pairs"] < 1 << 31 and o["dsub"] * i["M"] == i["dim"]
            seen_many += o["blocks"] > 1
            seen_cut += o["block_rows"] < min(i["nq"], ROWS_MAX) and i["force"] == 0
            seen_forced += o["block_rows"] == i["force"]
        else:
            seen_fail += o["Dp"] > 0
    # every kind of refusal but the LDS one, which the limits of M and ksub leave nothing to reach (64 * 256 * 4 is the limit itself: seen_full),
    # every form, a row that does not fit, a block the limit cut, several blocks, a forced one
    assert errors == {0, 1, 2, 3} and forms == {1, 2, 3} and seen_full
    assert seen_fail and seen_cut and seen_many and seen_forced
    assert shape_error(512, 64, 256) == 0 and MAX_M * MAX_KSUB * 4 == LDS
    # the shapes the GPU tests and the benchmark lean on
    assert plan(1475, 48, 7, 3, 70, 1475, 16, 16, 64)["blocks"] == 2 and plan(1475, 48, 7, 3, 70, 1475, 16, 16, 0)["blocks"] == 1
    big = plan(1000000, 512, 4096, 32, 4096, 32 * 1000, 64, 256, 0)
    assert big["ok"] and big["blocks"] == 1 and big["form"] == 1
