#!/usr/bin/env python3
"""What the forward-only pass (vv_forward) costs, and whether its plumbing costs the training step anything, measured against the PARENT
commit's library.

Three legs at cfg 2 (B 1024, C 5, Nn 50, 4096 -> 512) -- the parent's training step; this library's training step with vv_forward never
called; vv_forward alone -- alternate as child processes of this script (P T F P T F ...: what drifts, clocks or neighbours, reaches
all alike).  Every child creates one engine on the same synthetic table and batch, warms up, times one leg of >= 200 steps with a host
clock around work that ends in a device synchronise, takes a box probe and prints one JSON line; it runs under its own time limit and the
chain stops at the first child that fails.  A further, untimed child per leg reads the kernels' own durations (vv_profile_get:
"score_loss" and "fwd_gemm" of a training step; "eval_score", "eval_fwd_gemm" and "eval_loss" of the forward-only pass).  Two results:

  * the verdict of the condition to report: the training leg's median <= the parent's median + the parent's spread
    (max - min of its rounds: the yardstick);
  * the forward-only pass's time beside the training step's, and the score kernel's own duration in both (reported, not bounded).

The parent's library comes from a git worktree of the parent commit built into a scratch directory (--parent-root: that checkout, built
with `make -C videovector_amd/csrc`; its own Python package is imported with its library named by VV_LIB).  Without --parent-root the
script makes the worktree of HEAD~1 under --scratch and builds it.

  python tools/eval_bench.py [--parent-root DIR] [--steps 200] [--rounds 4] [--out profiles]
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
# leg: (whose library and package, what a step is: "train" the plain vv_step, "forward" one vv_forward)
LEGS = {
    "parent": ("parent", "train"),
    "train_no_forward": ("new", "train"),
    "forward_only": ("new", "forward"),
}
KERNELS = ("fwd_gemm", "score_loss", "segsum", "wgrad_gemm", "reduce_sgd", "eval_fwd_gemm", "eval_score", "eval_loss")
CHILD_LIMIT_S = 240
TAG = "EVAL_BENCH "


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
    fwd = LEGS[a.leg][1] == "forward"
    cfg = vv.StepConfig(B, C, Nn, lr=1e-3, momentum=0.9, global_count=gcount)

    def step():
        """one training step, or one forward-only pass"""
        if fwd:
            eng.forward(cfg, idx)
        else:
            eng.step(cfg, idx)

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
        out["ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / a.steps, 5)
    if fwd:
        st = eng.eval_stats()
        out.update(passes=st.passes, loss=float(st.last_loss))
    else:
        out.update(last_update_form=int(eng.get_option("last_update_form")), loss=eng.loss()[0])
    out.update(last_score_form=int(eng.get_option("last_score_form")), box_probe=eng.box_probe())
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
           "warmup": a.warmup,
           "legs": {leg: {"ms_per_step_rounds": [], "box_probe_rounds": []} for leg in LEGS}}
    for _ in range(a.rounds):
        for leg in LEGS:
            o = run_child(a, shape, leg, parent_root, False)
            L = res["legs"][leg]
            L["ms_per_step_rounds"].append(o["ms_per_step"])
            L["box_probe_rounds"].append(o["box_probe"])
            L.update({k: o[k] for k in ("last_update_form", "last_score_form", "loss", "passes") if k in o})
    for leg in LEGS:
        res["legs"][leg]["kernel_us"] = run_child(a, shape, leg, parent_root, True)["kernel_us"]
        res["legs"][leg]["ms_per_step"] = round(statistics.median(res["legs"][leg]["ms_per_step_rounds"]), 5)
    p = res["legs"]["parent"]
    spread = max(p["ms_per_step_rounds"]) - min(p["ms_per_step_rounds"])
    res["parent_spread_ms"] = round(spread, 5)
    tr, fw = res["legs"]["train_no_forward"], res["legs"]["forward_only"]
    res["train_minus_parent_ms"] = round(tr["ms_per_step"] - p["ms_per_step"], 5)
    res["train_within_condition"] = bool(res["train_minus_parent_ms"] <= spread)
    res["forward_only_over_train_step"] = round(fw["ms_per_step"] / tr["ms_per_step"], 4)
    res["score_kernel_us"] = {"parent_train": p["kernel_us"].get("score_loss"), "train": tr["kernel_us"].get("score_loss"),
                              "forward_only": fw["kernel_us"].get("eval_score")}
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
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else build_parent(a.scratch or tempfile.mkdtemp(prefix="eval_bench_parent_"))
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for shape in a.shapes.split(","):
        res = run_shape(a, shape, parent_root)
        path = os.path.join(a.out, "eval_%s.json" % shape)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        ok = ok and res["train_within_condition"]
        print("%s: parent %.4f ms (spread %.4f), training step with vv_forward never called %+.4f ms, vv_forward alone %.4f ms (%.2f of a step); "
              "score kernel %s us -> %s" % (shape, res["legs"]["parent"]["ms_per_step"], res["parent_spread_ms"], res["train_minus_parent_ms"],
                                            res["legs"]["forward_only"]["ms_per_step"], res["forward_only_over_train_step"], res["score_kernel_us"], path), flush=True)
    print("condition (the training leg within the parent's spread) %s" % ("met" if ok else "MISSED"), flush=True)


if __name__ == "__main__":
    main()
