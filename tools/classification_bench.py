#!/usr/bin/env python3
"""Times vv_classification_stats on device scores against the reference's procedure on the host, prints ONE JSON line and writes
it to profiles/classification_<n>x<C>.json (--out: elsewhere).

  python tools/classification_bench.py --n 200000 --classes 100 [--reps 5] [--warmup 1] [--host-threads 16] [--no-host]

Device: the scores are uploaded once (vv_dev_alloc); every call is Engine.classification_stats on that buffer.  Per call the host
wall time (label lists, allocations, launches, the synchronising download) and the library's own device events: "last_cls_row_ms"
(row pass + column pack) and "last_cls_count_ms" (counting + final pass), with the segments, launches and column blocks it ran.
Host: tests/classification_pin.cpp -- n dummies + n pairs per class, std::sort, the walk -- compiled with g++ -O2 and run on the same
data with --host-threads threads over the classes; its own timer excludes the file I/O.  The two results are compared (counts and
accuracies equal, ap within the pin's fp32 chain bound) before any time is reported.

Scores: a class signal of +1 in the row's own column under unit normal noise, rounded to 1/64 so that ties occur; labels uniform."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import videovector_amd as vv   # noqa: E402


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, Cn = a.n, a.classes
    rng = np.random.default_rng(9)
    labels = rng.integers(0, Cn, n).astype(np.int32)
    scores = rng.standard_normal((n, Cn), dtype=np.float32)
    scores[np.arange(n), labels] += 1.0
    scores = np.round(scores * 64) / 64

    eng = vv.Engine(0, "f16")
    buf = eng.dev(scores)
    wall, row_ms, count_ms = [], [], []
    got = None
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        got = eng.classification_stats(buf, labels, Cn)
        t1 = time.perf_counter()
        if r >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            row_ms.append(eng.get_option("last_cls_row_ms"))
            count_ms.append(eng.get_option("last_cls_count_ms"))
    out = dict(n=n, classes=Cn, reps=a.reps, device_wall_ms=stats(wall), row_pass_ms=stats(row_ms), counting_pass_ms=stats(count_ms),
               segments=int(eng.get_option("last_cls_segments")), counting_launches=int(eng.get_option("last_cls_passes")),
               column_blocks=int(eng.get_option("last_cls_blocks")), pair_comparisons=float(n) * n,
               total_accuracy=float(got[3]["total_accuracy"]), mean_ap=float(got[3]["mean_ap"]))
    buf.free()
    eng.close()

    if not a.no_host:
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "pin")
            subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "classification_pin.cpp"), "-o", exe], check=True)
            with open(os.path.join(d, "in.bin"), "wb") as f:
                f.write(np.array([n, Cn], np.int32).tobytes())
                f.write(scores.tobytes())
                f.write(labels.tobytes())
            secs = []
            for _ in range(max(1, min(a.reps, 3))):
                subprocess.run([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin"), str(a.host_threads)], check=True)
                raw = open(os.path.join(d, "out.bin"), "rb").read()
                secs.append(float(np.frombuffer(raw, np.float64, 1, 12 * Cn + 4)[0]) * 1e3)
            cnt = np.frombuffer(raw, np.int32, Cn, 0)
            acc = np.frombuffer(raw, np.float32, Cn, 4 * Cn)
            pap = np.frombuffer(raw, np.float32, Cn, 8 * Cn).astype(np.float64)
        assert np.array_equal(cnt, got[2]) and np.array_equal(acc, got[0]), "device and host disagree on the counts"
        d_ap = np.abs(got[1].astype(np.float64) - pap)
        assert (d_ap <= (cnt + 3) * 2.0 ** -23 * pap).all(), "device and host disagree on ap beyond the pin's fp32 chain bound"
        out.update(host_threads=a.host_threads, host_sort_ms=stats(secs), ap_max_abs_diff_vs_host=float(d_ap.max()),
                   host_over_device_wall=stats(secs)["median"] / stats(wall)["median"])
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, "profiles", "classification_%dx%d.json" % (n, Cn))
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
