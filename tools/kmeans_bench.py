#!/usr/bin/env python3
"""Times vv_gallery_kmeans on a device gallery against the similarity product alone on the same shape, prints ONE JSON line and writes
it to profiles/kmeans_<n>x<dim>x<C>.json (--out: elsewhere).

  python tools/kmeans_bench.py --n 200000 --dim 512 --clusters 1024 [--iters 10] [--rounds 4] [--metric euclidean] [--no-host]

Two legs alternate, --rounds times (K S K S ...: what drifts reaches both alike), each with a box probe (Engine.box_probe) in front:
  K  one Gallery.kmeans call of --iters iterations from kmeans_init_rows(1, n, C), timed on the host around the call (it synchronises
     once, at its end): iters + 1 assignment passes and iters updates.  The four legs' device time in the call's last iteration comes
     from the library's own events ("last_km_sim_ms", "last_km_assign_ms", "last_km_group_ms", "last_km_update_ms").
  S  the yardstick: the similarity kernel alone on the same product, C rows against the n items in dim columns -- Gallery.topk(k = 1) of
     C query rows against the item gallery, of which only "last_sim_ms" (the k_sim_f32 launches' device time) is read.  An iteration
     cannot be faster than its product.
Reported: per-iteration time (wall / iters, and the last iteration's four legs added up), each leg's share of that iteration, the
ratio of the iteration to the similarity-only leg, and the similarity leg's own round-to-round spread beside the three other kernels'
time.  Medians over the rounds.  No ratio is asserted.
Host, for context only: ONE Lloyd iteration (keys in row blocks, argmin, per-cluster means) in numpy float32 on --host-threads threads.

Embeddings: C class means 3 e_(c mod dim) + 0.2 c / C under 0.5 N(0, 1) noise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def host_iteration(X, cent, block=16384):
    n, Cn = X.shape[0], cent.shape[0]
    nn = (cent * cent).sum(1)
    a = np.empty(n, np.int64)
    for r0 in range(0, n, block):
        a[r0:r0 + block] = (-2.0 * (X[r0:r0 + block] @ cent.T) + nn[None, :]).argmin(1)
    order = np.argsort(a, kind="stable")
    counts = np.bincount(a, minlength=Cn)
    sums = np.add.reduceat(X[order], np.concatenate([[0], np.cumsum(counts)[:-1]]).clip(max=n - 1), axis=0)
    return np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], cent).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--metric", choices=("euclidean", "spherical"), default="euclidean")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(a.host_threads))
    import videovector_amd as vv

    rs = np.random.RandomState(1)
    member = np.arange(a.n) % a.clusters
    X = (0.5 * rs.standard_normal((a.n, a.dim))).astype(np.float32)
    X[np.arange(a.n), member % a.dim] += 3.0
    X[:, 0] += (0.2 * member / a.clusters).astype(np.float32)
    rows = vv.kmeans_init_rows(1, a.n, a.clusters)
    eng = vv.Engine(0, "f16")
    gal = eng.gallery(X)
    gal.kmeans(a.clusters, iters=1, metric=a.metric, init=rows)              # warm-up: first use of every kernel
    gal.topk(X[rows], 1)
    wall, legs, sim_only, probes, res = [], [], [], [], None
    for _ in range(a.rounds):
        probes.append(eng.box_probe())
        t0 = time.perf_counter()
        res = gal.kmeans(a.clusters, iters=a.iters, metric=a.metric, init=rows)
        wall.append((time.perf_counter() - t0) * 1e3)
        legs.append([eng.get_option("last_km_%s_ms" % k) for k in ("sim", "assign", "group", "update")])
        probes.append(eng.box_probe())
        gal.topk(X[rows], 1)
        sim_only.append(gal.get("last_sim_ms"))
    names = ("sim", "assign", "group", "update")
    leg = {k: stats([l[i] for l in legs]) for i, k in enumerate(names)}
    it_ms = sum(leg[k]["median"] for k in names)
    so = stats(sim_only)
    Dp = -(-a.dim // 32) * 32
    flop = 2.0 * a.n * a.clusters * Dp
    out = dict(shape=[a.n, a.dim, a.clusters], iters=a.iters, metric=a.metric, rounds=a.rounds,
               call_ms=stats(wall), per_iteration_ms=stats([w / max(a.iters, 1) for w in wall]),
               legs_ms_last_iteration=leg, last_iteration_ms=it_ms, shares={k: leg[k]["median"] / it_ms for k in names},
               similarity_only_ms=so, similarity_only_spread_ms=so["max"] - so["min"],
               non_similarity_ms=it_ms - leg["sim"]["median"],
               ratio_iteration_to_similarity_only=it_ms / so["median"],
               ratio_call_to_similarity_only=stats(wall)["median"] / ((a.iters + 1) * so["median"]),
               model=dict(product_flop=flop, sim_tflops_in_call=flop / (leg["sim"]["median"] * 1e-3) / 1e12,
                          sim_tflops_alone=flop / (so["median"] * 1e-3) / 1e12),
               blocks=int(eng.get_option("last_km_blocks")), chunks=int(eng.get_option("last_km_chunks")),
               assign_form=int(eng.get_option("last_km_assign_form")),
               objective=[float(v) for v in res.objective], moved=[int(v) for v in res.moved], report=res.report,
               box_probe=probes)
    if not a.no_host:
        t0 = time.perf_counter()
        host_iteration(X, X[rows])
        out["host_numpy_f32_iteration_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_threads"] = a.host_threads
    gal.close()
    eng.close()
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, "profiles", "kmeans_%dx%dx%d.json" % (a.n, a.dim, a.clusters))
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
