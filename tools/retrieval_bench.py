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
  python tools/retrieval_bench.py --nearest 33,256,2048 [--nq 4096 --ng 1000000 --dim 512] [--self-n 8192,200000] [--out FILE]
      nearest-neighbour lists (vv_gallery_nearest): topk(32), the yardstick, and nearest(K) alternate call by call in one process,
      for every K given; per call the library's device events ("last_device_ms", "last_sim_ms"), and the selection's own share,
      last_device_ms - last_sim_ms (uploads of the query blocks and downloads of the lists included), next to top-k's.  Then
      nearest_self(64) on galleries of the --self-n sizes (the class-level benchmark's two).  Writes the JSON it prints to
      profiles/nearest_<nq>x<ng>x<dim>.json (--out: elsewhere) as well.
  python tools/retrieval_bench.py --knn 32,256,2048 [--nq 4096 --ng 1000000 --dim 512] [--classes 15] [--out FILE]
      the k-NN classifier (vv_gallery_knn_scores, uniform weights, labels = id % classes): nearest(K), the yardstick, and
      knn_scores(K) alternate call by call in one process on the shape and with the box probes of --nearest; per call the library's
      device events, the vote launches' own time ("last_knn_vote_ms") and, as the host sees it, the wall time around each blocking
      call (nearest returns the lists to the host, knn_scores leaves the scores on the device).  Writes the JSON it prints to
      profiles/knn_<nq>x<ng>x<dim>.json (--out: elsewhere) as well.
  python tools/retrieval_bench.py --ivf 4096:32,1024:8 [--nq 4096 --ng 1000000 --dim 512] [--rounds 4] [--out FILE]
      the inverted-file index (vv_ivf_search): for every C:nprobe the index is built on Gallery.kmeans(C, iters=10), then
      IVFIndex.search(k = 32) and Gallery.topk(32), the yardstick, alternate call by call for --rounds rounds behind one warm-up round;
      per call the library's device events and the host's wall clock, the search's four legs (vv_ivf_get), recall@1 and recall@32
      against the exact lists of the same invocation, and the share of the tiles' area that is padding (tiles x 128^2 against the
      candidates).  The condition: the search's median below top-k's by more than the two spreads (max - min) together.  Writes the JSON
      it prints to profiles/ivf_<nq>x<ng>x<dim>.json (--out: elsewhere) as well.
  python tools/retrieval_bench.py --ivfpq 64,16 [--nq 4096 --ng 1000000 --dim 512] [--pq-c 4096 --pq-nprobe 32 --ksub 256] [--rounds 4] [--out FILE]
      product-quantised lists (vv_ivfpq_search) against the fp32 index (vv_ivf_search), both built on the same Gallery.kmeans(C, iters=10)
      centroids and assignment: for every M the codebooks are Engine.pq_train(M, ksub, iters = --pq-iters), then the two searches (k = 32)
      alternate call by call for --rounds rounds behind one warm-up round; per call the library's device events and the host's wall
      clock, the four legs of either search -- "ivfpq_scan_ms" is k_pq_scan's own device time, "ivf_sim_ms" the grouped similarity's --,
      index_bytes beside the fp32 index's n_ref Dp 4 bytes of rows, and recall@1 / recall@32 against vv_ivf_search at the same nprobe
      (the quantisation's loss alone) and against topk(32).  Run on two inputs: the generator below as the other legs use it (noise 4.0
      on unit-scale centres: an item's neighbours are all but random, so recall there says little) and the same generator with
      --clustered-noise (0.05, well below the centres' scale).  Writes the JSON it prints to profiles/ivfpq_<nq>x<ng>x<dim>.json as well.

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


def nearest_bench(eng, a):
    ks = [int(x) for x in a.nearest.split(",")]
    G, gid, cen = make(a.ng, a.dim, a.nid, a.noise, 5)
    Q, qid, _ = make(a.nq, a.dim, a.nid, a.noise, 6, cen)
    g = eng.gallery(G, gid)
    box = {"before": eng.box_probe()}
    res = []
    for k in ks:
        t = dict(topk=dict(dev=[], sim=[]), nearest=dict(dev=[], sim=[]))
        form = scratch = None
        for r in range(a.warmup + a.reps):
            for name, call in (("topk", lambda: g.topk(Q, 32)), ("nearest", lambda: g.nearest(Q, k))):
                got = call()
                if r >= a.warmup:
                    t[name]["dev"].append(g.get("last_device_ms")); t[name]["sim"].append(g.get("last_sim_ms"))
                if name == "topk":
                    head = got
                else:
                    form, scratch = int(g.get("last_nearest_form")), g.scratch_bytes
                    same = bool(np.array_equal(got[0][:, :32], head[0]) and np.array_equal(got[1][:, :32].view(np.uint32), head[1].view(np.uint32)))
        e = dict(k=k, form=form, scratch_bytes=scratch, first_32_equal_topk_32=same)
        for name in ("topk", "nearest"):
            dev, sim = t[name]["dev"], t[name]["sim"]
            e[name + "_ms"] = stats(dev); e[name + "_similarity_ms"] = stats(sim)
            e[name + "_other_ms"] = stats([d - s for d, s in zip(dev, sim)])
        e["nearest_over_topk"] = e["nearest_ms"]["median"] / e["topk_ms"]["median"]
        res.append(e)
    blocks = -(-a.nq // int(g.get("query_block")))
    g.close()
    del G, Q
    selfs = []
    for n in [int(x) for x in a.self_n.split(",") if x]:
        X, ids, _ = make(n, a.dim, max(n // 8, 1), a.noise, 7)
        gs = eng.gallery(X, ids)
        e = dict(n=n, k=64)
        for name, excl in (("nearest_self", False), ("nearest_self_other_id", True)):
            dev, sim = [], []
            for r in range(1 + a.self_reps):
                gs.nearest_self(64, excl)
                if r >= 1:
                    dev.append(gs.get("last_device_ms")); sim.append(gs.get("last_sim_ms"))
            e[name + "_ms"] = stats(dev); e[name + "_similarity_ms"] = stats(sim)
            e[name + "_other_ms"] = stats([d - s for d, s in zip(dev, sim)])
        e.update(form=int(gs.get("last_nearest_form")), scratch_bytes=gs.scratch_bytes)
        gs.close()
        selfs.append(e)
    box["after"] = eng.box_probe()
    out = dict(bench="nearest", nq=a.nq, ng=a.ng, dim=a.dim, reps=a.reps, warmup=a.warmup, self_reps=a.self_reps, query_blocks=blocks,
               yardstick="vv_gallery_topk at k = 32, alternating call by call with vv_gallery_nearest in one process",
               timer="device events inside the library (last_device_ms, last_sim_ms); *_other_ms = device - similarity per call",
               lists=res, self_lists=selfs, box=box)
    path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                 "nearest_%dx%dx%d.json" % (a.nq, a.ng, a.dim))
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return out


def knn_bench(eng, a):
    ks = [int(x) for x in a.knn.split(",")]
    G, gid, cen = make(a.ng, a.dim, a.nid, a.noise, 5)
    Q, qid, _ = make(a.nq, a.dim, a.nid, a.noise, 6, cen)
    lab = (gid % a.classes).astype(np.int32)
    g = eng.gallery(G, gid)
    buf = vv.engine.DevBuf(eng, (a.nq, a.classes))
    box = {"before": eng.box_probe()}
    res = []
    for k in ks:
        t = dict(nearest=dict(dev=[], sim=[], wall=[]), knn=dict(dev=[], sim=[], wall=[], vote=[]))
        for r in range(a.warmup + a.reps):
            for name, call in (("nearest", lambda: g.nearest(Q, k)), ("knn", lambda: g.knn_scores(Q, lab, a.classes, k, out=buf))):
                t0 = time.perf_counter()
                got = call()
                wall = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    t[name]["dev"].append(g.get("last_device_ms")); t[name]["sim"].append(g.get("last_sim_ms")); t[name]["wall"].append(wall)
                    if name == "knn":
                        t[name]["vote"].append(g.get("last_knn_vote_ms"))
                if name == "nearest":
                    lists = got
        # the last pair of calls: the device's votes against the lists the yardstick returned
        votes = np.stack([np.bincount(lab[row], minlength=a.classes) for row in lists[0]]).astype(np.float32) / np.float32(k)
        e = dict(k=k, form=int(g.get("last_nearest_form")), store_form=int(eng.get_option("last_knn_form")), scratch_bytes=g.scratch_bytes,
                 scores_equal_votes_of_nearest=bool(np.array_equal(buf.get(), votes)))
        for name in ("nearest", "knn"):
            dev, sim = t[name]["dev"], t[name]["sim"]
            e[name + "_ms"] = stats(dev); e[name + "_similarity_ms"] = stats(sim); e[name + "_wall_ms"] = stats(t[name]["wall"])
            e[name + "_other_ms"] = stats([d - s for d, s in zip(dev, sim)])
        e["knn_vote_ms"] = stats(t["knn"]["vote"])
        e["knn_over_nearest"] = e["knn_ms"]["median"] / e["nearest_ms"]["median"]
        e["knn_over_nearest_wall"] = e["knn_wall_ms"]["median"] / e["nearest_wall_ms"]["median"]
        res.append(e)
    blocks = -(-a.nq // int(g.get("query_block")))
    buf.free()
    g.close()
    box["after"] = eng.box_probe()
    out = dict(bench="knn", nq=a.nq, ng=a.ng, dim=a.dim, classes=a.classes, weighting="uniform", reps=a.reps, warmup=a.warmup, query_blocks=blocks,
               yardstick="vv_gallery_nearest at the same k, alternating call by call with vv_gallery_knn_scores in one process",
               timer="device events inside the library (last_device_ms, last_sim_ms, last_knn_vote_ms); *_other_ms = device - similarity "
                     "per call; *_wall_ms: host wall clock around the blocking call",
               votes=res, box=box)
    path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                 "knn_%dx%dx%d.json" % (a.nq, a.ng, a.dim))
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return out


def ivf_bench(eng, a):
    G, gid, cen = make(a.ng, a.dim, a.nid, a.noise, 5)
    Q, qid, _ = make(a.nq, a.dim, a.nid, a.noise, 6, cen)
    g = eng.gallery(G, gid)
    box = {"before": eng.box_probe()}
    res = []
    for spec in a.ivf.split(","):
        Cn, nprobe = (int(x) for x in spec.split(":"))
        t0 = time.perf_counter()
        km = g.kmeans(Cn, iters=10)
        t1 = time.perf_counter()
        ix = km.ivf(g)
        t2 = time.perf_counter()
        t = dict(topk=dict(dev=[], wall=[]), ivf=dict(dev=[], wall=[], probe=[], group=[], sim=[], select=[]))
        for r in range(1 + a.rounds):
            for name, call in (("topk", lambda: g.topk(Q, 32)), ("ivf", lambda: ix.search(Q, 32, nprobe))):
                w0 = time.perf_counter()
                got = call()
                wall = (time.perf_counter() - w0) * 1e3
                if name == "topk":
                    exact = got
                if r >= 1:
                    t[name]["wall"].append(wall)
                    t[name]["dev"].append(g.get("last_device_ms") if name == "topk" else ix.get("last_device_ms"))
                    if name == "ivf":
                        for leg in ("probe", "group", "sim", "select"):
                            t[name][leg].append(ix.get("last_%s_ms" % leg))
        idx, dist, m = got
        hit1 = float((idx[:, 0] == exact[0][:, 0]).mean())
        hit32 = float(np.mean([len(np.intersect1d(u, v)) for u, v in zip(idx, exact[0])]) / 32.0)
        tiles, cands = ix.get("last_tiles"), ix.get("last_candidates")
        e = dict(num_clusters=Cn, nprobe=nprobe, k=32, kmeans_iters=10, kmeans_wall_ms=(t1 - t0) * 1e3, index_build_wall_ms=(t2 - t1) * 1e3,
                 largest_list=int(ix.get("largest_list")), empty_lists=int(ix.get("empty_lists")), blocks=int(ix.get("last_blocks")),
                 grid_wgs=int(ix.get("last_grid_wgs")), tiles=int(tiles), candidates=int(cands),
                 mean_candidates_per_query=cands / a.nq, share_of_gallery_met=cands / (float(a.nq) * a.ng),
                 padded_tile_area_share=1.0 - cands / (tiles * 128.0 * 128.0) if tiles else 0.0,
                 recall_at_1=hit1, recall_at_32=hit32)
        for name in ("topk", "ivf"):
            e[name + "_ms"] = stats(t[name]["dev"]); e[name + "_wall_ms"] = stats(t[name]["wall"])
        for leg in ("probe", "group", "sim", "select"):
            e["ivf_%s_ms" % leg] = stats(t["ivf"][leg])
        for kind in ("_ms", "_wall_ms"):
            tk, iv = e["topk" + kind], e["ivf" + kind]
            e["topk_over_ivf" + kind.replace("_ms", "")] = tk["median"] / iv["median"]
            e["condition_met" + kind.replace("_ms", "")] = bool(tk["median"] - iv["median"] > (tk["max"] - tk["min"]) + (iv["max"] - iv["min"]))
        res.append(e)
        ix.close()
    g.close()
    box["after"] = eng.box_probe()
    out = dict(bench="ivf", nq=a.nq, ng=a.ng, dim=a.dim, rounds=a.rounds, warmup_rounds=1,
               yardstick="vv_gallery_topk at k = 32, alternating call by call with vv_ivf_search in one process",
               timer="device events inside the library (last_device_ms of either call; the legs of vv_ivf_get); *_wall_ms: host wall clock "
                     "around the blocking call",
               condition="median(topk) - median(ivf) > (max - min)(topk) + (max - min)(ivf)", searches=res, box=box)
    path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                 "ivf_%dx%dx%d.json" % (a.nq, a.ng, a.dim))
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return out


def recall(idx, want, at):
    """the share of want's first `at` items (its -1 slots apart) found in idx's first `at`"""
    hit = total = 0
    for u, v in zip(idx, want):
        v = v[:at][v[:at] >= 0]
        hit += len(np.intersect1d(u[:at], v)); total += len(v)
    return hit / float(max(total, 1))


def ivfpq_bench(eng, a):
    Ms = [int(x) for x in a.ivfpq.split(",")]
    Cn, nprobe, ksub = a.pq_c, a.pq_nprobe, a.ksub
    box = {"before": eng.box_probe()}
    inputs = []
    for gen, noise in (("bench", a.noise), ("clustered", a.clustered_noise)):
        G, gid, cen = make(a.ng, a.dim, a.nid, noise, 5)
        Q, qid, _ = make(a.nq, a.dim, a.nid, noise, 6, cen)
        g = eng.gallery(G, gid)
        print("ivfpq: %s input on the device" % gen, file=sys.stderr, flush=True)
        km = g.kmeans(Cn, iters=10)
        flat = eng.ivf(g, km.centroids, metric=km.metric, assign=km.assign)
        exact = g.topk(Q, 32)
        res = []
        for M in Ms:
            print("ivfpq: %s M = %d" % (gen, M), file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            cb, obj = eng.pq_train(g, M, ksub, iters=a.pq_iters, seed=1)
            t1 = time.perf_counter()
            pq = eng.ivfpq(g, km.centroids, cb, metric=km.metric, assign=km.assign)
            t2 = time.perf_counter()
            legs = dict(ivf=("probe", "group", "sim", "select"), ivfpq=("probe", "lut", "scan", "select"))
            t = {name: dict(dev=[], wall=[], **{leg: [] for leg in legs[name]}) for name in legs}
            got = {}
            for r in range(1 + a.rounds):
                for name, ix in (("ivf", flat), ("ivfpq", pq)):
                    w0 = time.perf_counter()
                    got[name] = ix.search(Q, 32, nprobe)
                    wall = (time.perf_counter() - w0) * 1e3
                    if r >= 1:
                        t[name]["wall"].append(wall); t[name]["dev"].append(ix.get("last_device_ms"))
                        for leg in legs[name]:
                            t[name][leg].append(ix.get("last_%s_ms" % leg))
            Dp = -(-a.dim // 32) * 32
            e = dict(M=M, ksub=ksub, dsub=a.dim // M, pq_train_iters=a.pq_iters, pq_train_wall_ms=(t1 - t0) * 1e3, index_build_wall_ms=(t2 - t1) * 1e3,
                     pq_objective_sum=float(obj.sum()), scan_form=int(pq.get("last_scan_form")), blocks=int(pq.get("last_blocks")),
                     candidates=int(pq.get("last_candidates")), same_candidates_as_ivf=bool(np.array_equal(got["ivf"][2], got["ivfpq"][2])),
                     index_bytes=int(pq.get("index_bytes")), ivf_row_bytes=a.ng * Dp * 4,
                     rows_over_index_bytes=a.ng * Dp * 4 / pq.get("index_bytes"),
                     recall_at_1_vs_ivf=recall(got["ivfpq"][0], got["ivf"][0], 1), recall_at_32_vs_ivf=recall(got["ivfpq"][0], got["ivf"][0], 32),
                     recall_at_1_vs_topk=recall(got["ivfpq"][0], exact[0], 1), recall_at_32_vs_topk=recall(got["ivfpq"][0], exact[0], 32),
                     ivf_recall_at_1_vs_topk=recall(got["ivf"][0], exact[0], 1), ivf_recall_at_32_vs_topk=recall(got["ivf"][0], exact[0], 32))
            for name in legs:
                e[name + "_ms"] = stats(t[name]["dev"]); e[name + "_wall_ms"] = stats(t[name]["wall"])
                for leg in legs[name]:
                    e["%s_%s_ms" % (name, leg)] = stats(t[name][leg])
            e["ivf_over_ivfpq"] = e["ivf_ms"]["median"] / e["ivfpq_ms"]["median"]
            e["ivf_sim_over_ivfpq_scan"] = e["ivf_sim_ms"]["median"] / e["ivfpq_scan_ms"]["median"]
            res.append(e)
            pq.close()
        inputs.append(dict(generator=gen, noise=noise, nid=a.nid, largest_list=int(flat.get("largest_list")), empty_lists=int(flat.get("empty_lists")),
                           searches=res))
        flat.close(); g.close()
        del G, Q
    box["after"] = eng.box_probe()
    out = dict(bench="ivfpq", nq=a.nq, ng=a.ng, dim=a.dim, num_clusters=Cn, nprobe=nprobe, k=32, kmeans_iters=10, rounds=a.rounds, warmup_rounds=1,
               yardstick="vv_ivf_search on the same centroids and assignment, alternating call by call with vv_ivfpq_search in one process",
               timer="device events inside the library (last_device_ms and the legs of vv_ivf_get / vv_ivfpq_get); *_wall_ms: host wall clock "
                     "around the blocking call", inputs=inputs, box=box)
    path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                 "ivfpq_%dx%dx%d.json" % (a.nq, a.ng, a.dim))
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return out


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
    ap.add_argument("--nearest", type=str, default=None, metavar="K[,K...]")
    ap.add_argument("--knn", type=str, default=None, metavar="K[,K...]")
    ap.add_argument("--self-n", type=str, default="8192,200000")
    ap.add_argument("--self-reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--ivf", type=str, default=None, metavar="C:NPROBE[,C:NPROBE...]")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--ivfpq", type=str, default=None, metavar="M[,M...]")
    ap.add_argument("--pq-c", type=int, default=4096)
    ap.add_argument("--pq-nprobe", type=int, default=32)
    ap.add_argument("--ksub", type=int, default=256)
    ap.add_argument("--pq-iters", type=int, default=5)
    ap.add_argument("--clustered-noise", type=float, default=0.05)
    a = ap.parse_args()
    eng = vv.Engine(0, "f16")
    if a.ivfpq:
        out = ivfpq_bench(eng, a)
    elif a.ivf:
        out = ivf_bench(eng, a)
    elif a.nearest:
        out = nearest_bench(eng, a)
    elif a.knn:
        if not 1 <= a.classes <= 4096:
            ap.error("--classes must be 1 .. 4096 with --knn")
        out = knn_bench(eng, a)
    elif a.class_stats:
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
