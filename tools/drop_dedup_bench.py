#!/usr/bin/env python3
"""What option "drop_dedup" = 2 is worth on the shapes it adds: a training step under dropout 0.9 (counter mask) with the de-duplicated
execution (value 2: k_score_stream / k_seg_bwd carry the per-instance masks) against value 1, which runs these shapes dense.

One engine per value on the same synthetic table and batch; the two alternate in rounds (A B A B ...), each leg >= 200 steps after warm-up,
timed with a host clock around work that ends in a device synchronise.  Reported per shape: the median over the rounds and every round's
figure (their spread is the yardstick for the difference), per-kernel times from vv_profile_get (a separate, untimed pass), rows / distinct
rows, the box probe.  One JSON file per shape: profiles/drop_dedup_<shape>.json.

  python tools/drop_dedup_bench.py [--shapes cfg5_rank,b1024_nn70,b1024_c9] [--steps 200] [--rounds 4] [--out profiles]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name: (B, C, Nn, F, D, global batch the items are drawn with, global_count)
SHAPES = {
    "cfg5_rank": (512, 5, 200, 4096, 1024, 4096, 4096 * 200),       # one rank's batch of BASELINE configs[4]
    "b1024_nn70": (1024, 5, 70, 4096, 512, 1024, 0),                # D = 512 past the register-resident kernel's 55 negatives
    "b1024_c9": (1024, 9, 50, 4096, 512, 1024, 0),                  # ... past its 6 context rows
}
KERNELS = ("dedup", "fwd_gemm", "score_loss", "segsum", "guard", "wgrad_gemm", "reduce", "sgd", "reduce_sgd")


def make_engine(vv, ds, W, b, F, value):
    eng = vv.Engine(0, "f16")
    eng.set_option("drop_dedup", value)
    eng.table_synth(ds.seed, ds.n_rows, F)
    eng.params_set(W, b)
    return eng


def leg(eng, cfg, idx, steps):
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step(cfg, idx)
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_us(eng, cfg, idx, steps):
    eng.profile_select(None)
    eng.profile_enable(1)
    for _ in range(steps):
        eng.step(cfg, idx)
    eng.synchronize()
    out = {}
    for k in KERNELS:
        ms, n = eng.profile_get(k)              # (the mean over its n timed launches)
        if n:
            out[k] = round(ms * 1e3, 2)
    eng.profile_enable(False)
    return out


def run_shape(vv, name, steps, rounds, warmup):
    from videovector_amd.synth import SyntheticVideos, init_weights
    B, C, Nn, F, D, GB, gcount = SHAPES[name]
    ds = SyntheticVideos(seed=1701, n_videos=2048)
    smp = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=GB, context_size=C, num_negative_samples=Nn,
                     max_buffer_size=5000, negative_swap_percentage=50)
    idx = np.ascontiguousarray(smp.next()[:B])
    smp.close()
    W, b = init_weights(5, D, F)
    cfg = vv.StepConfig(B, C, Nn, lr=1e-3, dropout_ratio=0.9, dropout_seed=4242, global_count=gcount)
    engines = {v: make_engine(vv, ds, W, b, F, v) for v in (1, 2)}
    res = {"shape": dict(name=name, B=B, C=C, Nn=Nn, F=F, D=D, global_count=gcount, dropout_ratio=0.9, mask="counter"),
           "steps_per_leg": steps, "rounds": rounds, "warmup": warmup, "box_probe_before": engines[1].box_probe()}
    for v, eng in engines.items():
        for _ in range(warmup):
            eng.step(cfg, idx)
        eng.synchronize()
        rows, uniq = eng.dedup_stats()
        res["value_%d" % v] = dict(rows=rows, distinct_rows=uniq, last_score_form=int(eng.get_option("last_score_form")), loss=eng.loss()[0])
    legs = {1: [], 2: []}
    for _ in range(rounds):                       # A B A B: what drifts (clocks, neighbours) reaches both alike
        for v in (1, 2):
            legs[v].append(leg(engines[v], cfg, idx, steps))
    for v in (1, 2):
        r = res["value_%d" % v]
        r["ms_per_step_rounds"] = [round(x, 4) for x in legs[v]]
        r["ms_per_step"] = round(statistics.median(legs[v]), 4)
        r["kernel_us"] = kernel_us(engines[v], cfg, idx, 20)
    res["box_probe_after"] = engines[1].box_probe()
    spread = max(max(legs[v]) - min(legs[v]) for v in (1, 2))
    gain = res["value_1"]["ms_per_step"] - res["value_2"]["ms_per_step"]
    res["value_2_gain_ms"] = round(gain, 4)
    res["rounds_spread_ms"] = round(spread, 4)
    res["value_2_faster_beyond_spread"] = bool(gain > spread)
    for eng in engines.values():
        eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.steps < 200:
        print("note: fewer than 200 steps per leg -- a rehearsal, not a measurement", file=sys.stderr)
    import videovector_amd as vv
    os.makedirs(a.out, exist_ok=True)
    for name in a.shapes.split(","):
        res = run_shape(vv, name, a.steps, a.rounds, a.warmup)
        path = os.path.join(a.out, "drop_dedup_%s.json" % name)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("%s: value 1 %.4f ms (%d / %d rows distinct), value 2 %.4f ms (%d / %d), gain %.4f ms, spread %.4f ms -> %s" % (
            name, res["value_1"]["ms_per_step"], res["value_1"]["distinct_rows"], res["value_1"]["rows"], res["value_2"]["ms_per_step"],
            res["value_2"]["distinct_rows"], res["value_2"]["rows"], res["value_2_gain_ms"], res["rounds_spread_ms"], path), flush=True)


if __name__ == "__main__":
    main()
