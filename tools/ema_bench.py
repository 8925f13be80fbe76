#!/usr/bin/env python3
"""What the moving average of the parameters (vv_ema_set) costs a step, measured against the PARENT commit's library.

Three legs at cfg 2 (B 1024, C 5, Nn 50, 4096 -> 512) -- the parent's library; this library with the average off (vv_ema_set never
called); with the average on at decay 0.999 (k_ema behind every update) -- alternate as child processes of this script (P F N P F N ...:
what drifts, clocks or neighbours, reaches all alike).  Every child creates one engine on the same synthetic table and batch, warms up,
times one leg of >= 200 steps with a host clock around work that ends in a device synchronise, takes a box probe and prints one JSON
line; it runs under its own time limit and the chain stops at the first child that fails.  A further, untimed child per leg of this
library reads the kernels' own durations (vv_profile_get: "reduce_sgd", and "ema" -- k_ema's own -- for the active leg).  Reported:
every round's figure, the medians, the parent's spread (max - min of its rounds: the yardstick) and the verdict of the condition to
report:

  the off leg's median <= the parent's median + the parent's spread.

The on leg's step time and k_ema's duration are reported, not bounded: k_ema moves 12 D F bytes per update (25 MB here).

The parent's library comes from a git worktree of the parent commit built into a scratch directory (--parent-root: that checkout, built
with `make -C videovector_amd/csrc`; its own Python package is imported with its library named by VV_LIB).  Without --parent-root the
script makes the worktree of HEAD~1 under --scratch and builds it.

  python tools/ema_bench.py [--parent-root DIR] [--steps 200] [--rounds 4] [--out profiles]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (B, C, Nn, F, D, global batch the items are drawn with, global_count)
SHAPES = {"cfg2": (1024, 5, 50, 4096, 512, 1024, 0)}               # BASELINE configs[1]
# leg: (whose library and package, the decay or None for "never called")
LEGS = {
    "parent": ("parent", None),
    "off": ("new", None),
    "on": ("new", 0.999),
}
KERNELS = ("reduce_sgd", "ema")
CHILD_LIMIT_S = 240
TAG = "EMA_BENCH "


def child(a):
    """One leg in a process of its own: prints one JSON line."""
    sys.path.insert(0, a.pkg_root)
    import numpy as np
    import videovector_amd as vv
    from videovector_amd.synth import SyntheticVideos, init_weights
    B, C, Nn, F, D, GB, gcount = SHAPES[a.shape]
    ds = SyntheticVideos(seed=1701, n_videos=2048)
    smp = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=GB, context_size=C, num_negative_samples=Nn,
                     max_buffer_size=5000, negative_swap_percentage=50)
    idx = np.ascontiguousarray(smp.next()[:B])
    smp.close()
    W, b = init_weights(5, D, F)
    eng = vv.Engine(0, "f16")
    eng.table_synth(ds.seed, ds.n_rows, F)
    eng.params_set(W, b)
    decay = LEGS[a.leg][1]
    if decay is not None:
        eng.ema_set(decay)
    cfg = vv.StepConfig(B, C, Nn, lr=1e-3, momentum=0.9, global_count=gcount)
    for _ in range(a.warmup):
        eng.step(cfg, idx)
    eng.synchronize()
    out = dict(leg=a.leg, lib=vv.lib_path())
    if a.profile:
        eng.profile_select(None)
        eng.profile_enable(1)
        for _ in range(a.steps):
            eng.step(cfg, idx)
        eng.synchronize()
        out["kernel_us"] = {}
        for k in KERNELS:
            ms, n = eng.profile_get(k)
            if n:
                out["kernel_us"][k] = round(ms * 1e3, 3)
    else:
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.step(cfg, idx)
        eng.synchronize()
        out["ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / a.steps, 5)
    if decay is not None:
        s = eng.ema_stats()
        out["ema_stats"] = dict(updates=int(s["updates"]), decay=float(s["decay"]), in_use=bool(s["in_use"]))
    out.update(last_update_form=int(eng.get_option("last_update_form")), last_wgrad_splits=int(eng.get_option("last_wgrad_splits")),
               loss=eng.loss()[0], box_probe=eng.box_probe())
    eng.close()
    print(TAG + json.dumps(out), flush=True)


def run_child(a, shape, leg, parent_root, profile):
    root = parent_root if LEGS[leg][0] == "parent" else ROOT
    env = dict(os.environ, VV_LIB=os.path.join(root, "videovector_amd", "lib", "libvideovec.so"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", shape, "--leg", leg, "--pkg-root", root,
           "--steps", str(20 if profile else a.steps), "--warmup", str(a.warmup)]
    if profile:
        cmd.append("--profile")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
    if r.returncode != 0 or not lines:
        raise SystemExit("the %s leg of %s failed (exit %d): the chain stops here\n%s" % (leg, shape, r.returncode, r.stderr[-2000:]))
    return json.loads(lines[-1][len(TAG):])


def build_parent(scratch):
    root = os.path.join(scratch, "parent")
    if not os.path.isdir(root):
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", root, "HEAD~1"], check=True)
    subprocess.run(["make", "-C", os.path.join(root, "videovector_amd", "csrc"), "-s", "-j8"], check=True)
    return root


def run_shape(a, shape, parent_root):
    B, C, Nn, F, D, GB, gcount = SHAPES[shape]
    res = {"shape": dict(name=shape, B=B, C=C, Nn=Nn, F=F, D=D, global_count=gcount), "steps_per_leg": a.steps, "rounds": a.rounds,
           "warmup": a.warmup, "k_ema_bytes": 12 * (D * F + D),
           "legs": {leg: {"ms_per_step_rounds": [], "box_probe_rounds": []} for leg in LEGS}}
    for _ in range(a.rounds):
        for leg in LEGS:
            o = run_child(a, shape, leg, parent_root, False)
            L = res["legs"][leg]
            L["ms_per_step_rounds"].append(o["ms_per_step"])
            L["box_probe_rounds"].append(o["box_probe"])
            L.update({k: o[k] for k in ("last_update_form", "last_wgrad_splits", "loss", "ema_stats") if k in o})
    for leg in LEGS:
        res["legs"][leg]["kernel_us"] = run_child(a, shape, leg, parent_root, True)["kernel_us"]
        res["legs"][leg]["ms_per_step"] = round(statistics.median(res["legs"][leg]["ms_per_step_rounds"]), 5)
    p = res["legs"]["parent"]
    spread = max(p["ms_per_step_rounds"]) - min(p["ms_per_step_rounds"])
    res["parent_spread_ms"] = round(spread, 5)
    for leg in ("off", "on"):
        res[leg + "_minus_parent_ms"] = round(res["legs"][leg]["ms_per_step"] - p["ms_per_step"], 5)
    res["k_ema_us"] = res["legs"]["on"]["kernel_us"].get("ema")
    res["off_within_condition"] = bool(res["off_minus_parent_ms"] <= spread)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--shape"); ap.add_argument("--leg"); ap.add_argument("--pkg-root")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.steps < 200:
        print("note: fewer than 200 steps per leg -- a rehearsal, not a measurement", file=sys.stderr)
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else build_parent(a.scratch or tempfile.mkdtemp(prefix="ema_bench_parent_"))
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for shape in a.shapes.split(","):
        res = run_shape(a, shape, parent_root)
        path = os.path.join(a.out, "ema_%s.json" % shape)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        ok = ok and res["off_within_condition"]
        print("%s: parent %.4f ms (spread %.4f), average off %+.4f ms, on %+.4f ms, k_ema %s us -> %s" % (
            shape, res["legs"]["parent"]["ms_per_step"], res["parent_spread_ms"], res["off_minus_parent_ms"],
            res["on_minus_parent_ms"], res["k_ema_us"], path), flush=True)
    print("condition (the off leg within the parent's spread) %s" % ("met" if ok else "MISSED"), flush=True)


if __name__ == "__main__":
    main()
