#!/usr/bin/env python3
"""What option "h16_guard" costs a training step, measured against the PARENT commit's library (never against this library's own value 0).

Three legs -- the parent's library, this library with h16_guard 1, this library with h16_guard 0 -- alternate as child processes of this
script (P 1 0 P 1 0 ...: what drifts, clocks or neighbours, reaches all alike).  Every child creates one engine on the same synthetic table and
batch, warms up, times one leg of >= 200 steps with a host clock around work that ends in a device synchronise, takes a box probe and prints
one JSON line; it runs under its own time limit and the chain stops at the first child that fails.  A further, untimed child per leg reads the
segment-wise backward's own duration (vv_profile_get "segsum": k_seg_bwd / k_seg_bwd_cnt).  Reported per shape: every round's figure, the
medians, the parent's spread (max - min of its rounds: the yardstick) and the verdict of DESIGN.md 3.6's condition for default 1:

  guard 1's median <= the parent's median + the parent's spread, and guard 0's median within the parent's spread of the parent's median.

The parent's library comes from a git worktree of the parent commit built into a scratch directory (--parent-root: that checkout, built with
`make -C videovector_amd/csrc`; its own Python package is imported with its library named by VV_LIB).  Without --parent-root the script
makes the worktree of HEAD~1 under --scratch and builds it.

  python tools/h16_guard_bench.py [--parent-root DIR] [--shapes cfg2,cfg5_rank] [--steps 200] [--rounds 4] [--out profiles]
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
SHAPES = {
    "cfg2": (1024, 5, 50, 4096, 512, 1024, 0),                      # BASELINE configs[1]
    "cfg5_rank": (512, 5, 200, 4096, 1024, 4096, 4096 * 200),       # one rank's batch of BASELINE configs[4]
}
LEGS = ("parent", "guard1", "guard0")
CHILD_LIMIT_S = 240


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
    if a.guard >= 0:
        eng.set_option("h16_guard", a.guard)
    eng.table_synth(ds.seed, ds.n_rows, F)
    eng.params_set(W, b)
    cfg = vv.StepConfig(B, C, Nn, lr=1e-3, global_count=gcount)
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
        ms, n = eng.profile_get("segsum")
        out.update(seg_bwd_us=round(ms * 1e3, 3), seg_bwd_launches=int(n))
    else:
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.step(cfg, idx)
        eng.synchronize()
        out["ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / a.steps, 5)
    rows, uniq = eng.dedup_stats()
    out.update(rows=rows, distinct_rows=uniq, last_score_form=int(eng.get_option("last_score_form")), loss=eng.loss()[0],
               box_probe=eng.box_probe())
    if a.guard >= 0:
        out["last_h16"] = int(eng.get_option("last_h16"))
        out["h16_stats"] = eng.h16_stats()
    eng.close()
    print("H16_GUARD_BENCH " + json.dumps(out), flush=True)


def run_child(a, shape, leg, parent_root, profile):
    root = parent_root if leg == "parent" else ROOT
    env = dict(os.environ, VV_LIB=os.path.join(root, "videovector_amd", "lib", "libvideovec.so"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", shape, "--leg", leg, "--pkg-root", root,
           "--guard", {"parent": "-1", "guard1": "1", "guard0": "0"}[leg], "--steps", str(20 if profile else a.steps), "--warmup", str(a.warmup)]
    if profile:
        cmd.append("--profile")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("H16_GUARD_BENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the %s leg of %s failed (exit %d): the chain stops here\n%s" % (leg, shape, r.returncode, r.stderr[-2000:]))
    return json.loads(lines[-1][len("H16_GUARD_BENCH "):])


def build_parent(scratch):
    root = os.path.join(scratch, "parent")
    if not os.path.isdir(root):
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", root, "HEAD~1"], check=True)
    subprocess.run(["make", "-C", os.path.join(root, "videovector_amd", "csrc"), "-s", "-j8"], check=True)
    return root


def run_shape(a, shape, parent_root):
    B, C, Nn, F, D, GB, gcount = SHAPES[shape]
    res = {"shape": dict(name=shape, B=B, C=C, Nn=Nn, F=F, D=D, global_count=gcount), "steps_per_leg": a.steps, "rounds": a.rounds,
           "warmup": a.warmup, "legs": {leg: {"ms_per_step_rounds": [], "box_probe_rounds": []} for leg in LEGS}}
    for _ in range(a.rounds):
        for leg in LEGS:
            o = run_child(a, shape, leg, parent_root, False)
            L = res["legs"][leg]
            L["ms_per_step_rounds"].append(o["ms_per_step"])
            L["box_probe_rounds"].append(o["box_probe"])
            L.update({k: o[k] for k in ("rows", "distinct_rows", "last_score_form", "loss", "last_h16", "h16_stats") if k in o})
    for leg in LEGS:
        o = run_child(a, shape, leg, parent_root, True)
        res["legs"][leg].update(seg_bwd_us=o["seg_bwd_us"], seg_bwd_launches=o["seg_bwd_launches"])
        res["legs"][leg]["ms_per_step"] = round(statistics.median(res["legs"][leg]["ms_per_step_rounds"]), 5)
    p = res["legs"]["parent"]
    spread = max(p["ms_per_step_rounds"]) - min(p["ms_per_step_rounds"])
    res["parent_spread_ms"] = round(spread, 5)
    res["guard1_minus_parent_ms"] = round(res["legs"]["guard1"]["ms_per_step"] - p["ms_per_step"], 5)
    res["guard0_minus_parent_ms"] = round(res["legs"]["guard0"]["ms_per_step"] - p["ms_per_step"], 5)
    res["guard1_within_condition"] = bool(res["guard1_minus_parent_ms"] <= spread)
    res["guard0_within_parent_spread"] = bool(abs(res["guard0_minus_parent_ms"]) <= spread)
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
    ap.add_argument("--shape"); ap.add_argument("--leg"); ap.add_argument("--pkg-root"); ap.add_argument("--guard", type=int, default=-1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.steps < 200:
        print("note: fewer than 200 steps per leg -- a rehearsal, not a measurement", file=sys.stderr)
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else build_parent(a.scratch or tempfile.mkdtemp(prefix="h16_guard_parent_"))
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for shape in a.shapes.split(","):
        res = run_shape(a, shape, parent_root)
        path = os.path.join(a.out, "h16_guard_%s.json" % shape)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        L = res["legs"]
        ok = ok and res["guard1_within_condition"] and res["guard0_within_parent_spread"]
        print("%s: parent %.4f ms (spread %.4f), guard 1 %+.4f ms, guard 0 %+.4f ms; k_seg_bwd %.2f / %.2f / %.2f us -> %s" % (
            shape, L["parent"]["ms_per_step"], res["parent_spread_ms"], res["guard1_minus_parent_ms"], res["guard0_minus_parent_ms"],
            L["parent"]["seg_bwd_us"], L["guard1"]["seg_bwd_us"], L["guard0"]["seg_bwd_us"], path), flush=True)
    print("condition for default 1 %s" % ("met on every shape" if ok else "MISSED"), flush=True)


if __name__ == "__main__":
    main()
