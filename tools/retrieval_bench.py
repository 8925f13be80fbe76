#!/usr/bin/env python3
"""Times gallery retrieval on one GPU and prints ONE JSON line.

  python tools/retrieval_bench.py --nq 4096 --ng 1000000 --dim 512 --k 10 [--reps 20] [--warmup 3]
      top-k and rank statistics of nq queries against ng reference items: milliseconds per call (device events inside the
      library: "last_device_ms" of vv_gallery_get, uploads of the query blocks included), the similarity kernels' share of it
      and their achieved TFLOP/s (2 nq ng dim / similarity time), and the bytes of device scratch held.
  python tools/retrieval_bench.py --versus-within-batch --n 8192 --dim 512 [--reps 5]
      the parent's only retrieval path, vv_retrieval_stats (Gram kernel, download, one host sort per row), against
      vv_gallery_rank_stats with the same n rows as queries and as gallery; host wall time of both calls, alternating.
  python tools/retrieval_bench.py --class-stats --n 8192 --dim 512 [--classes 15] [--videos 600] [--reps 10] [--no-within-batch]
      class-level leave-one-out statistics (vv_gallery_class_stats) of n items: host wall time of gallery creation + class_stats
      against vv_retrieval_stats on the same rows, alternating in one process (skipped with --no-within-batch: n^2 floats no
      longer fit), and the device time of class_stats alone, its similarity share, passes and scratch bytes.  Input: make_input
      of tests/class_stats_ref.py (noise 3.0 / 6.0, seed 11).

Inputs are seeded: unit rows around `nid` random centres, ids = the centre's index (the generator of tests/gallery_ref.py, drawn in
float32 blocks so that a million rows need no float64 copy)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import videovector_amd as vv   # noqa: E402


def make(n, dim, nid, noise, seed, cen=None):
    rng = np.random.default_rng(seed)
    if cen is None:
        cen = rng.standard_normal((nid, dim), dtype=np.float32)
    ids = rng.integers(0, nid, n).astype(np.int32)
    X = np.empty((n, dim), np.float32)
    for a in range(0, n, 65536):
        b = min(n, a + 65536)
        blk = cen[ids[a:b]] + noise * rng.standard_normal((b - a, dim), dtype=np.float32)
        X[a:b] = blk / np.linalg.norm(blk, axis=1, keepdims=True)
    return X, ids, cen


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--ng", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nid", type=int, default=20000)
    ap.add_argument("--noise", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--versus-within-batch", action="store_true")
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--class-stats", action="store_true")
    ap.add_argument("--classes", type=int, default=15)
    ap.add_argument("--videos", type=int, default=600)
    ap.add_argument("--no-within-batch", action="store_true")
    a = ap.parse_args()
    eng = vv.Engine(0, "f16")
    if a.class_stats:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from class_stats_ref import make_input
        X, ids, id2class = make_input(a.n, a.dim, a.videos, a.classes, 3.0, 6.0, 11)
        old, new, dev, sim = [], [], [], []
        res = ref = None
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            if not a.no_within_batch:
                ref = eng.retrieval_stats(X, ids, id2class, exclude_same_video=True)
            t1 = time.perf_counter()
            g = eng.gallery(X, ids)
            res = g.class_stats(id2class, exclude_same_video=True)
            t2 = time.perf_counter()
            if r >= a.warmup:
                old.append((t1 - t0) * 1e3); new.append((t2 - t1) * 1e3)
                dev.append(g.get("last_device_ms")); sim.append(g.get("last_sim_ms"))
            passes, scratch, block = int(g.get("last_passes")), g.scratch_bytes, int(g.get("query_block"))
            g.close()
        flop = 2.0 * a.n * a.n * a.dim
        out = dict(bench="class_stats", n=a.n, dim=a.dim, classes=a.classes, videos=a.videos, reps=a.reps, warmup=a.warmup,
                   gallery_plus_class_stats_ms=stats(new), class_stats_device_ms=stats(dev), similarity_ms=stats(sim),
                   similarity_tflops=flop / (stats(sim)["median"] * 1e-3) / 1e12, passes=passes, scratch_bytes=scratch,
                   query_block=block, result={k: float(v) for k, v in res.items()},
                   timer="host wall clock around the blocking calls; device events for *_device_ms / similarity_ms")
        if not a.no_within_batch:
            out.update(retrieval_stats_ms=stats(old), ratio_of_medians=stats(old)["median"] / stats(new)["median"],
                       retrieval_stats_result=[float(v) for v in ref])
    elif a.versus_within_batch:
        X, ids, _ = make(a.n, a.dim, max(a.n // 8, 1), a.noise, 7)
        id2class = {int(i): int(i) for i in np.unique(ids)}
        g = eng.gallery(X, ids)
        old, new = [], []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            eng.retrieval_stats(X, ids, id2class, exclude_same_video=False)
            t1 = time.perf_counter()
            g.rank_stats(X, ids)
            t2 = time.perf_counter()
            if r >= a.warmup:
                old.append((t1 - t0) * 1e3); new.append((t2 - t1) * 1e3)
        out = dict(bench="within_batch_vs_gallery", n=a.n, dim=a.dim, reps=a.reps, warmup=a.warmup,
                   retrieval_stats_ms=stats(old), gallery_rank_stats_ms=stats(new),
                   ratio_of_medians=stats(old)["median"] / stats(new)["median"], timer="host wall clock around each blocking call")
        g.close()
    else:
        G, gid, cen = make(a.ng, a.dim, a.nid, a.noise, 5)
        Q, qid, _ = make(a.nq, a.dim, a.nid, a.noise, 6, cen)
        g = eng.gallery(G, gid)
        flop = 2.0 * a.nq * a.ng * a.dim
        res = {}
        for name, call in (("topk", lambda: g.topk(Q, a.k)), ("rank_stats", lambda: g.rank_stats(Q, qid))):
            dev, sim = [], []
            for r in range(a.warmup + a.reps):
                call()
                if r >= a.warmup:
                    dev.append(g.get("last_device_ms")); sim.append(g.get("last_sim_ms"))
            res[name + "_ms"] = stats(dev)
            res[name + "_similarity_ms"] = stats(sim)
            res[name + "_similarity_tflops"] = flop / (stats(sim)["median"] * 1e-3) / 1e12
            res[name + "_end_to_end_tflops"] = flop / (stats(dev)["median"] * 1e-3) / 1e12
        out = dict(bench="gallery", nq=a.nq, ng=a.ng, dim=a.dim, k=a.k, reps=a.reps, warmup=a.warmup,
                   scratch_bytes=g.scratch_bytes, query_block=int(g.get("query_block")), passes=int(g.get("last_passes")),
                   timer="device events", **res)
        g.close()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
