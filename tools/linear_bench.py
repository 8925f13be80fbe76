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

Embeddings: class means 3 e_(c mod dim) under 0.5 N(0, 1) noise; labels i mod C."""
import argparse
import json
import os
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
    a = ap.parse_args()
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
    probe0 = eng.box_probe()
    wall, legs, rep = [], [], None
    for r in range(a.warmup + a.reps):
        lin = eng.linear(a.dim, a.classes)
        t0 = time.perf_counter()
        _, rep = lin.fit(gal, y, iters=a.steps, batch=a.batch, **hp)
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
               box_probe=[probe0, probe1])
    if not a.no_host:
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
    name = "linear_%dx%dx%d%s.json" % (a.n, a.dim, a.classes, "_b%d" % a.batch if a.batch else "")
    path = a.out or os.path.join(ROOT, "profiles", name)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
