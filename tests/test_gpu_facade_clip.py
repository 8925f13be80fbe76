"""`caffe train` with SolverParameter.clip_gradients (BVLC Caffe's field, read by name; SGDSolver::ClipGradients) on the smallest facade
fixture, the one tests/test_gpu_facade_adam.py uses: with a threshold far below the first step's norm BVLC's line appears on the display
iterations and the totals line at the end, the final caffemodel differs from an unclipped run's and equals, bit for bit, the engine
driven through Python with the same threshold; with clip_gradients: -1 or with the field absent the caffemodel is byte-identical and the
log is line for line the same once each line's time stamp, process id and source line number are taken off (the parent commit's binary
is not available to a test: "today's run" is represented by the run without the field, whose weights must in turn equal the engine's
without any clipping call, bit for bit)."""
import re

import numpy as np
import pytest

from tests.test_facade_proto import pb, tool  # noqa: F401  (fixtures)
from tests.test_gpu_facade import read_caffemodel, run_caffe, write_caffemodel
from videovector_amd.prototxt import solver, train_net
from videovector_amd.synth import SyntheticVideos, init_weights

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, V, ITERS = 32, 5, 2, 128, 32, 50, 3
ENV = {"VV_DEDUP": "0", "VV_SLAB16": "0"}
CLIP = 1e-3
LINE = r"Gradient clipping: scaling down gradients \(L2 norm ([0-9.eE+-]+) > ([0-9.eE+-]+)\) by scale factor ([0-9.eE+-]+)"


def caffe_run(pb, tmp_path, name, **extra):  # noqa: F811
    d = tmp_path / name
    d.mkdir()
    net_p, sol_p = d / "net.prototxt", d / "solver.prototxt"
    net_p.write_text(train_net("synthetic://videos=%d;seed=1701;features=%d" % (V, F), B, C, Nn, D, max_buffer=500, w_std=0.02))
    sol_p.write_text(solver(str(net_p), base_lr=0.01, momentum=0.9, max_iter=ITERS, display=1, lr_policy="fixed",
                            snapshot_prefix=str(d / "snap"), **extra))
    W0, b0 = init_weights(3, D, F, std=0.02)
    write_caffemodel(pb, str(d / "init.caffemodel"), W0, b0)
    log = run_caffe(["train", "--solver=%s" % sol_p, "--weights=%s" % (d / "init.caffemodel")], str(d / "train.log"), ENV)
    model = (d / ("snap_iter_%d.caffemodel" % ITERS)).read_bytes()
    W, b, _ = read_caffemodel(pb, str(d / ("snap_iter_%d.caffemodel" % ITERS)))
    # each line without its time stamp, process id and source line; the run's own directory by one name
    lines = [re.sub(r"^[IWEF]\d{4} \d\d:\d\d:\d\d\.\d{6} +\d+ ([\w.]+):\d+\] ", r"\1] ", ln).replace(str(d), "<dir>") for ln in log.splitlines()]
    return log, lines, model, W, b


def engine_run(clip):
    import videovector_amd as vv
    ds = SyntheticVideos(seed=1701, n_videos=V)
    smp = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=B, context_size=C, num_negative_samples=Nn, max_buffer_size=500,
                     negative_swap_percentage=50)
    W0, b0 = init_weights(3, D, F, std=0.02)
    eng = vv.Engine(0, "f16")
    try:
        eng.set_dedup(False); eng.set_option("slab16", 0)
        eng.table_synth(ds.seed, ds.n_rows, F)
        eng.params_set(W0, b0)
        cfg = vv.StepConfig(B, C, Nn, lr=0.01, momentum=0.9, clip_gradients=clip)
        stats = []
        for _ in range(ITERS):                             # as Solver::Step on a display iteration: hint, pass, the loss, the update
            eng.update_hint(cfg)
            eng.forward_backward(cfg, smp.next())
            eng.loss()
            eng.apply_update(cfg)
            stats.append(eng.clip_stats())
        W, b, _, _ = eng.params_get()
        return W, b, stats
    finally:
        eng.close()
        smp.close()


def test_caffe_train_clip_gradients(tool, pb, tmp_path):  # noqa: F811
    log0, lines0, model0, W_plain, b_plain = caffe_run(pb, tmp_path, "absent")
    log1, lines1, model1, _, _ = caffe_run(pb, tmp_path, "minus_one", clip_gradients=-1)
    logc, _, modelc, W_clip, b_clip = caffe_run(pb, tmp_path, "clipped", clip_gradients=CLIP)

    # clipped: BVLC's line on every display iteration, the totals at the end, another model
    found = re.findall(LINE, logc)
    assert len(found) == ITERS, logc[-3000:]
    assert ("Gradient clipping: %d of %d updates were scaled down" % (ITERS, ITERS)) in logc
    assert modelc != model0 and not np.array_equal(W_clip, W_plain)
    We, be, stats = engine_run(CLIP)
    assert all(s["clipped"] == 1 for s in stats) and stats[-1]["clipped_updates"] == ITERS
    for (norm, thr, scale), s in zip(found, stats):
        assert float(thr) == float("%g" % CLIP) and float(norm) == float("%g" % s["norm"]) and float(scale) == float("%g" % s["scale"])
        assert float(norm) > 100 * CLIP, "the threshold is not far below the norm: the inputs are wrong"
    assert np.array_equal(W_clip, We) and np.array_equal(b_clip, be), "caffe train with clip_gradients differs from the engine with the same threshold"

    # disabled or absent: nothing of it in the log, byte-identical models, the same log, the engine's unclipped weights
    assert not [ln for ln in lines0 if "clip" in ln.lower()]          # (lines0: the run's own directory, named after this test, taken out)
    assert model1 == model0
    assert [ln for ln in lines1 if not re.match(r"^(\S+\] )?clip_gradients: -1$", ln)] == lines0
    assert "Gradient clipping" not in log1
    Wp, bp, stats = engine_run(None)
    assert stats[-1]["updates"] == 0
    assert np.array_equal(W_plain, Wp) and np.array_equal(b_plain, bp)
