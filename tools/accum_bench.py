#!/usr/bin/env python3
"""What gradient accumulation (vv_grads_bank; BVLC iter_size) costs, measured against the PARENT commit's library.

Three legs at cfg 2 (B 1024, C 5, Nn 50, 4096 -> 512) -- the parent's library; this library with nothing banked (the plain vv_step);
iter_size 4 (four forward_backward + grads_bank, one apply_update: reported per micro-batch and per update) -- alternate as child
processes of this script (P N A P N A ...: what drifts, clocks or neighbours, reaches all alike).  Every child creates one engine on the
same synthetic table and batch, warms up, times one leg of >= 200 steps with a host clock around work that ends in a device synchronise,
takes a box probe and prints one JSON line; it runs under its own time limit and the chain stops at the first child that fails.  A
further, untimed child per leg of this library reads the kernels' own durations (vv_profile_get: "reduce_sgd" for the plain leg;
"reduce", "grad_bank", "sgd" for the accumulating one).  Reported: every round's figure, the medians, the parent's spread (max - min of
its rounds: the yardstick) and the verdict of the condition to report:

  the nothing-banked leg's median <= the parent's median + the parent's spread.

The accumulating leg's times are reported, not bounded: each of its passes runs k_reduce + k_grad_bank where a plain step runs the fused
update, and its one update adds the closing pass over the 8.4 MB gradient.

The parent's library comes from a git worktree of the parent commit built into a scratch directory (--parent-root: that checkout, built
with `make -C videovector_amd/csrc`; its own Python package is imported with its library named by VV_LIB).  Without --parent-root the
script makes the worktree of HEAD~1 under --scratch and builds it.

  python tools/accum_bench.py [--parent-root DIR] [--steps 200] [--rounds 4] [--out profiles]
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
# leg: (whose library and package, micro-batches banked per update; 0: the plain vv_step, no bank call)
LEGS = {
    "parent": ("parent", 0),
    "nothing_banked": ("new", 0),
    "iter_size_4": ("new", 4),
}
KERNELS = ("reduce_sgd", "reduce", "grad_bank", "sgd")
CHILD_LIMIT_S = 240
TAG = "ACCUM_BENCH "


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
    m = LEGS[a.leg][1]
    cfg = vv.StepConfig(B, C, Nn, lr=1e-3, momentum=0.9, global_count=gcount)

    def step():
        """one update: the plain vv_step, or m banked passes and their update"""
        if m == 0:
            eng.step(cfg, idx)
            return
        for _ in range(m):
            eng.forward_backward(cfg, idx)
            eng.grads_bank()
        eng.apply_update(cfg)

    for _ in range(a.warmup):
        step()
    eng.synchronize()
    out = dict(leg=a.leg, lib=vv.lib_path())
    if a.profile:
        eng.profile_select(None)
        eng.profile_enable(1)
        for _ in range(a.steps):
            step()
        eng.synchronize()
        out["kernel_us"] = {}
        for k in KERNELS:
            ms, n = eng.profile_get(k)
            if n:
                out["kernel_us"][k] = round(ms * 1e3, 3)
    else:
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        eng.synchronize()
        out["ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / a.steps, 5)          # per UPDATE
    if m:
        out["accum_stats"] = {k: (float(v) if k.startswith("last_mean") else int(v)) for k, v in eng.accum_stats().items()}
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
           "warmup": a.warmup, "gradient_bytes": 4 * (D * F + D),
           "legs": {leg: {"ms_per_step_rounds": [], "box_probe_rounds": []} for leg in LEGS}}
    for _ in range(a.rounds):
        for leg in LEGS:
            o = run_child(a, shape, leg, parent_root, False)
            L = res["legs"][leg]
            L["ms_per_step_rounds"].append(o["ms_per_step"])
            L["box_probe_rounds"].append(o["box_probe"])
            L.update({k: o[k] for k in ("last_update_form", "last_wgrad_splits", "loss", "accum_stats") if k in o})
    for leg in LEGS:
        res["legs"][leg]["kernel_us"] = run_child(a, shape, leg, parent_root, True)["kernel_us"]
        res["legs"][leg]["ms_per_step"] = round(statistics.median(res["legs"][leg]["ms_per_step_rounds"]), 5)
    p = res["legs"]["parent"]
    spread = max(p["ms_per_step_rounds"]) - min(p["ms_per_step_rounds"])
    res["parent_spread_ms"] = round(spread, 5)
    res["nothing_banked_minus_parent_ms"] = round(res["legs"]["nothing_banked"]["ms_per_step"] - p["ms_per_step"], 5)
    res["nothing_banked_within_condition"] = bool(res["nothing_banked_minus_parent_ms"] <= spread)
    acc, m = res["legs"]["iter_size_4"], LEGS["iter_size_4"][1]
    acc["ms_per_update"] = acc["ms_per_step"]
    acc["ms_per_micro_batch"] = round(acc["ms_per_step"] / m, 5)
    res["micro_batch_minus_parent_step_ms"] = round(acc["ms_per_micro_batch"] - p["ms_per_step"], 5)
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
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else build_parent(a.scratch or tempfile.mkdtemp(prefix="accum_bench_parent_"))
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for shape in a.shapes.split(","):
        res = run_shape(a, shape, parent_root)
        path = os.path.join(a.out, "accum_%s.json" % shape)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        ok = ok and res["nothing_banked_within_condition"]
        acc = res["legs"]["iter_size_4"]
        print("%s: parent %.4f ms (spread %.4f), nothing banked %+.4f ms, iter_size 4: %.4f ms per update, %.4f ms per micro-batch -> %s" % (
            shape, res["legs"]["parent"]["ms_per_step"], res["parent_spread_ms"], res["nothing_banked_minus_parent_ms"],
            acc["ms_per_update"], acc["ms_per_micro_batch"], path), flush=True)
    print("condition (the nothing-banked leg within the parent's spread) %s" % ("met" if ok else "MISSED"), flush=True)


if __name__ == "__main__":
    main()
