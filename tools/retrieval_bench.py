#!/usr/bin/env python3
"""Times gallery retrieval on one GPU and prints ONE JSON line.

  python tools/retrieval_bench.py --nq 4096 --ng 1000000 --dim 512 --k 10 [--reps 20] [--warmup 3]
      top-k and rank statistics of nq queries against ng reference items: milliseconds per call (device events inside the
      library: "last_device_ms" of vv_gallery_get, uploads of the query blocks included), the similarity kernels' share of it
      and their achieved TFLOP/s (2 nq ng dim / similarity time), and the bytes of device scratch held.
  python tools/retrieval_bench.py --versus-within-batch --n 8192 --dim 512 [--reps 5]
      the parent's only retrieval path, vv_retrieval_stats (Gram kernel, download, one host sort per row), against
      vv_gallery_rank_stats with the same n rows as queries and as gallery; host wall time of both calls, alternating.

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
    a = ap.parse_args()
    eng = vv.Engine(0, "f16")
    if a.versus_within_batch:
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
