#!/usr/bin/env python3
"""Times vv_linear_fit on a device gallery against the same step in numpy float32 on the host, prints ONE JSON line and writes it
to profiles/linear_<n>x<dim>x<C>[_b<batch>].json (--out: elsewhere).

  python tools/linear_bench.py --n 200000 --dim 512 --classes 100 [--batch 4096] [--steps 50] [--reps 5] [--warmup 1] [--no-host]

Device: the gallery is uploaded once; every repetition is one fit of --steps steps from zero weights, timed on the host around the
call (one synchronisation at its end), so per step = wall / steps; the four legs' device time in the fit's last step comes from the
library's own events ("last_lin_fwd_ms", "last_lin_softmax_ms", "last_lin_wgrad_ms", "last_lin_update_ms"), with the splits and row
blocks it ran.  A box probe (Engine.box_probe) is taken in front of and behind the fits.  The model per full-batch step: X is read
twice (2 n Dp 4 bytes), the forward and the weight-gradient products are 2 n Dp Cp FLOP each.
Host: the same step (logits, softmax, dz^T X, the rule) in numpy float32 on --host-threads threads: the outside yardstick.

--loss hinge [--norm L1|L2] times the same fit under the one-vs-rest hinge loss (vv_linear_loss_set): the second leg is then k_hinge's
device time (it is reported in the "softmax" slot: "last_lin_softmax_ms" is the loss kernel's leg), the file is
profiles/linear_hinge_<n>x<dim>x<C>[_b<batch>].json, the streaming model of that kernel -- the logits read once and dz written once,
2 count Cp 4 bytes, at the box probe's copy rate of this run -- is recorded beside it, and the host yardstick is left out.

--compare PARENT_ROOT (a checkout of the parent commit with its library built) alternates three legs as child processes of this script,
--rounds times (P S H P S H ...: what drifts reaches all alike): the PARENT's library under the softmax loss, this library under the
softmax loss, this library under the hinge loss.  Every child is one run as above (no host yardstick) with its own box probe and its own
time limit, and the chain stops at the first child that fails.  Written to profiles/linear_hinge_<shape>.json: every round's figures, the
medians, the parent's spread (max - min of its rounds' loss-kernel legs), k_hinge's leg against the parent's k_softmax_xent leg and against
the streaming model, and the condition that this library's softmax leg lies within the parent's spread.

--rows PARENT_ROOT alternates four legs the same way (P C I S P C I S ..., --rounds times), all under the softmax loss: the PARENT's
library, contiguous fit; this library, contiguous fit; this library, vv_linear_fit_rows over the identity list; vv_linear_fit_rows over one
shuffled epoch (vv_rows_shuffled, seed 1).  A child runs a row-list leg with --fit-rows identity|shuffled.  Written to
profiles/linear_rows_<shape>.json: every round's forward and weight-gradient legs and step time, the medians, the parent's spread per leg
(max - min of its rounds), the condition that this library's contiguous legs lie within it, the identity and shuffled legs as ratios to
this library's contiguous legs, and the index traffic beside them: count 4 bytes of indices per product against count Dp 4 bytes of rows.

Embeddings: class means 3 e_(c mod dim) under 0.5 N(0, 1) noise; labels i mod C."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--loss", choices=("softmax", "hinge"), default="softmax")
    ap.add_argument("--norm", choices=("L1", "L2"), default="L2")
    ap.add_argument("--compare", default=None, metavar="PARENT_ROOT")
    ap.add_argument("--rows", default=None, metavar="PARENT_ROOT")
    ap.add_argument("--fit-rows", choices=("identity", "shuffled"), default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pkg-root", default=ROOT)
    a = ap.parse_args()
    if a.compare:
        return compare(a)
    if a.rows:
        return compare_rows(a)
    if a.pkg_root != ROOT:
        sys.path.insert(0, a.pkg_root)
    os.environ.setdefault("OMP_NUM_THREADS", str(a.host_threads))
    import linear_ref as ref
    import videovector_amd as vv

    rs = np.random.RandomState(1)
    y = (np.arange(a.n) % a.classes).astype(np.int32)
    X = (0.5 * rs.standard_normal((a.n, a.dim))).astype(np.float32)
    X[np.arange(a.n), y % a.dim] += 3.0
    hp = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)
    eng = vv.Engine(0, "f16")
    gal = eng.gallery(X)
    rows = None
    if a.fit_rows:
        rows = np.arange(a.n, dtype=np.int32) if a.fit_rows == "identity" else vv.rows_shuffled(1, a.n, 1)
    probe0 = eng.box_probe()
    wall, legs, rep = [], [], None
    for r in range(a.warmup + a.reps):
        lin = eng.linear(a.dim, a.classes)
        if a.loss == "hinge":
            lin.set_loss("hinge", a.norm)
        t0 = time.perf_counter()
        _, rep = lin.fit(gal, y, iters=a.steps, batch=a.batch, **hp) if rows is None else lin.fit(gal, y, iters=a.steps, batch=a.batch, rows=rows, **hp)
        t1 = time.perf_counter()
        lin.close()
        if r >= a.warmup:
            wall.append((t1 - t0) * 1e3 / a.steps)
            legs.append([eng.get_option("last_lin_%s_ms" % k) for k in ("fwd", "softmax", "wgrad", "update")])
    probe1 = eng.box_probe()
    count = a.n if a.batch == 0 else min(a.batch, a.n)
    Dp, Cp = -(-a.dim // 32) * 32, -(-a.classes // 32) * 32
    leg = {k: stats([l[i] for l in legs]) for i, k in enumerate(("fwd", "softmax", "wgrad", "update"))}
    flop = 2.0 * count * Dp * Cp
    out = dict(shape=[a.n, a.dim, a.classes], batch=a.batch, steps=a.steps, step_ms=stats(wall), legs_ms_last_step=leg,
               splits=eng.get_option("last_lin_splits"), row_blocks=eng.get_option("last_lin_blocks"),
               loss_first=float(rep["loss_first"]), loss_last=float(rep["loss_last"]), accuracy_last=float(rep["accuracy_last"]),
               model=dict(x_bytes_per_step=2.0 * count * Dp * 4, product_flop=flop,
                          fwd_tflops=flop / (leg["fwd"]["median"] * 1e-3) / 1e12, wgrad_tflops=flop / (leg["wgrad"]["median"] * 1e-3) / 1e12,
                          fwd_yardstick_tflops=85.0),
               box_probe=[probe0, probe1], lib=vv.lib_path())
    if a.fit_rows:
        out["fit_rows"], out["last_lin_gather"] = a.fit_rows, int(eng.get_option("last_lin_gather"))
    if a.loss == "hinge":
        out["loss"], out["norm"], out["last_hinge_form"] = "hinge", a.norm, int(eng.get_option("last_hinge_form"))
        out["model"]["hinge_stream_bytes"] = 2.0 * count * Cp * 4
    if not a.no_host and a.loss == "softmax":
        st = ref.State(a.dim, a.classes, np.float32)
        t = []
        for _ in range(a.host_steps):
            t0 = time.perf_counter()
            ref.step(st, X[:count], y[:count], **hp)
            t.append((time.perf_counter() - t0) * 1e3)
        out["host_numpy_f32_step_ms"] = stats(t)
        out["host_threads"] = a.host_threads
    line = json.dumps(out)
    print(line)
    name = "linear_%s%dx%dx%d%s.json" % ("hinge_" if a.loss == "hinge" else "", a.n, a.dim, a.classes, "_b%d" % a.batch if a.batch else "")
    path = a.out or os.path.join(ROOT, "profiles", name)
    with open(path, "w") as f:
        f.write(line + "\n")


LEGS = {"parent_softmax": ("parent", "softmax"), "softmax": ("new", "softmax"), "hinge": ("new", "hinge")}
CHILD_LIMIT_S = 240


def copy_rate(probe):
    """The box probe's streaming-copy rate in bytes / s."""
    return float(probe["copy_tbs"]) * 1e12


def compare(a):
    parent = os.path.abspath(a.compare)
    shape = "%dx%dx%d%s" % (a.n, a.dim, a.classes, "_b%d" % a.batch if a.batch else "")
    res = dict(shape=[a.n, a.dim, a.classes], batch=a.batch, steps=a.steps, reps=a.reps, rounds=a.rounds, norm=a.norm,
               legs={k: dict(loss_leg_ms_rounds=[], step_ms_rounds=[], box_probe_rounds=[]) for k in LEGS})
    tmp = os.path.join(ROOT, "profiles", ".linear_bench_child.json")
    for _ in range(a.rounds):
        for leg, (whose, loss) in LEGS.items():
            root = parent if whose == "parent" else ROOT
            env = dict(os.environ, VV_LIB=os.path.join(root, "videovector_amd", "lib", "libvideovec.so"))
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--dim", str(a.dim), "--classes", str(a.classes), "--batch", str(a.batch),
                   "--steps", str(a.steps), "--reps", str(a.reps), "--warmup", str(a.warmup), "--no-host", "--out", tmp, "--pkg-root", root]
            if loss == "hinge":
                cmd += ["--loss", "hinge", "--norm", a.norm]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S, env=env)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                raise SystemExit("the %s leg failed (exit %d): the chain stops here\n%s" % (leg, r.returncode, r.stderr[-2000:]))
            o = json.loads(lines[-1])
            L = res["legs"][leg]
            L["loss_leg_ms_rounds"].append(o["legs_ms_last_step"]["softmax"]["median"])
            L["step_ms_rounds"].append(o["step_ms"]["median"])
            L["box_probe_rounds"].append(o["box_probe"])
            L["library"] = "the parent commit's" if whose == "parent" else "this commit's"
            L["last"] = {k: o[k] for k in ("legs_ms_last_step", "splits", "row_blocks", "loss_first", "loss_last", "accuracy_last", "model") if k in o}
    if os.path.exists(tmp):
        os.remove(tmp)
    for L in res["legs"].values():
        L["loss_leg_ms"] = statistics.median(L["loss_leg_ms_rounds"])
        L["step_ms"] = statistics.median(L["step_ms_rounds"])
    p = res["legs"]["parent_softmax"]
    res["parent_spread_ms"] = max(p["loss_leg_ms_rounds"]) - min(p["loss_leg_ms_rounds"])
    res["softmax_minus_parent_ms"] = res["legs"]["softmax"]["loss_leg_ms"] - p["loss_leg_ms"]
    res["softmax_within_parent_spread"] = bool(abs(res["softmax_minus_parent_ms"]) <= res["parent_spread_ms"])
    res["hinge_over_parent_softmax"] = res["legs"]["hinge"]["loss_leg_ms"] / p["loss_leg_ms"]
    rates = [copy_rate(pr) for pair in res["legs"]["hinge"]["box_probe_rounds"] for pr in pair]
    if rates:
        count = a.n if a.batch == 0 else min(a.batch, a.n)
        model_ms = 2.0 * count * (-(-a.classes // 32) * 32) * 4 / statistics.median(rates) * 1e3
        res["hinge_stream_model_ms"], res["hinge_over_stream_model"] = model_ms, res["legs"]["hinge"]["loss_leg_ms"] / model_ms
    path = os.path.join(ROOT, "profiles", "linear_hinge_%s.json" % shape) if a.out is None else a.out
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("%s: parent softmax %.4f ms (spread %.4f), softmax %+.4f ms, hinge %.4f ms = %.3f x parent's softmax, %s x the streaming model -> %s" % (
        shape, p["loss_leg_ms"], res["parent_spread_ms"], res["softmax_minus_parent_ms"], res["legs"]["hinge"]["loss_leg_ms"],
        res["hinge_over_parent_softmax"], "%.2f" % res["hinge_over_stream_model"] if rates else "?", path), flush=True)


ROW_LEGS = {"parent": ("parent", None), "contiguous": ("new", None), "identity": ("new", "identity"), "shuffled": ("new", "shuffled")}


def compare_rows(a):
    parent = os.path.abspath(a.rows)
    shape = "%dx%dx%d%s" % (a.n, a.dim, a.classes, "_b%d" % a.batch if a.batch else "")
    kinds = ("fwd", "wgrad")
    res = dict(shape=[a.n, a.dim, a.classes], batch=a.batch, steps=a.steps, reps=a.reps, rounds=a.rounds,
               legs={k: dict(fwd_ms_rounds=[], wgrad_ms_rounds=[], step_ms_rounds=[], box_probe_rounds=[]) for k in ROW_LEGS})
    tmp = os.path.join(ROOT, "profiles", ".linear_bench_child.json")
    for _ in range(a.rounds):
        for leg, (whose, fit_rows) in ROW_LEGS.items():
            root = parent if whose == "parent" else ROOT
            env = dict(os.environ, VV_LIB=os.path.join(root, "videovector_amd", "lib", "libvideovec.so"))
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--dim", str(a.dim), "--classes", str(a.classes), "--batch", str(a.batch),
                   "--steps", str(a.steps), "--reps", str(a.reps), "--warmup", str(a.warmup), "--no-host", "--out", tmp, "--pkg-root", root]
            if fit_rows:
                cmd += ["--fit-rows", fit_rows]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S, env=env)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                raise SystemExit("the %s leg failed (exit %d): the chain stops here\n%s" % (leg, r.returncode, r.stderr[-2000:]))
            o = json.loads(lines[-1])
            if fit_rows and o.get("last_lin_gather") != 2:
                raise SystemExit("the %s leg did not run the gathered form" % leg)
            L = res["legs"][leg]
            for k in kinds:
                L["%s_ms_rounds" % k].append(o["legs_ms_last_step"][k]["median"])
            L["step_ms_rounds"].append(o["step_ms"]["median"])
            L["box_probe_rounds"].append(o["box_probe"])
            L["library"] = "the parent commit's" if whose == "parent" else "this commit's"
            L["last"] = {k: o[k] for k in ("legs_ms_last_step", "splits", "row_blocks", "loss_first", "loss_last", "accuracy_last", "model") if k in o}
    if os.path.exists(tmp):
        os.remove(tmp)
    for L in res["legs"].values():
        for k in kinds + ("step",):
            L["%s_ms" % k] = statistics.median(L["%s_ms_rounds" % k])
    p, c = res["legs"]["parent"], res["legs"]["contiguous"]
    for k in kinds:
        spread = max(p["%s_ms_rounds" % k]) - min(p["%s_ms_rounds" % k])
        res["parent_%s_spread_ms" % k] = spread
        res["contiguous_%s_minus_parent_ms" % k] = c["%s_ms" % k] - p["%s_ms" % k]
        res["contiguous_%s_within_parent_spread" % k] = bool(abs(c["%s_ms" % k] - p["%s_ms" % k]) <= spread)
        for leg in ("identity", "shuffled"):
            res["%s_%s_over_contiguous" % (leg, k)] = res["legs"][leg]["%s_ms" % k] / c["%s_ms" % k]
    for leg in ("identity", "shuffled"):
        res["%s_step_over_contiguous" % leg] = res["legs"][leg]["step_ms"] / c["step_ms"]
    # the same traces, or the legs did not compute the same fit (identity == contiguous bit for bit is the tests' business)
    res["identity_loss_last_equals_contiguous"] = bool(res["legs"]["identity"]["last"]["loss_last"] == c["last"]["loss_last"])
    count, Dp = (a.n if a.batch == 0 else min(a.batch, a.n)), -(-a.dim // 32) * 32
    res["index_traffic_model"] = dict(index_bytes_per_product=count * 4, row_bytes_per_product=count * Dp * 4, ratio=1.0 / Dp)
    path = os.path.join(ROOT, "profiles", "linear_rows_%s.json" % shape) if a.out is None else a.out
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("%s: fwd parent %.4f (spread %.4f) contiguous %+.4f -> %s; identity x%.3f shuffled x%.3f | wgrad parent %.4f (spread %.4f) contiguous %+.4f -> %s; "
          "identity x%.3f shuffled x%.3f | step: identity x%.3f shuffled x%.3f -> %s" % (
              shape, p["fwd_ms"], res["parent_fwd_spread_ms"], res["contiguous_fwd_minus_parent_ms"], res["contiguous_fwd_within_parent_spread"],
              res["identity_fwd_over_contiguous"], res["shuffled_fwd_over_contiguous"], p["wgrad_ms"], res["parent_wgrad_spread_ms"],
              res["contiguous_wgrad_minus_parent_ms"], res["contiguous_wgrad_within_parent_spread"], res["identity_wgrad_over_contiguous"],
              res["shuffled_wgrad_over_contiguous"], res["identity_step_over_contiguous"], res["shuffled_step_over_contiguous"], path), flush=True)


if __name__ == "__main__":
    main()
