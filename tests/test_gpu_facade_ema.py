"""`caffe train` with SolverParameter.ema_decay / test_with_ema (this project's own fields) on the smallest facade fixture, the one
tests/test_gpu_facade_clip.py and tests/test_gpu_facade_eval.py use (a held-out branch on a second source, test_interval 2, test_iter 3).

  * ema_decay 0.9: beside every snapshot there is <prefix>_iter_<N>.ema.caffemodel with the ordinary model's layer and blob names; its
    values equal, bit for bit, ema_get of the engine driven through Python over the same sampler stream, and the ordinary caffemodels
    are bit for bit those of the run without the fields (training is untouched);
  * test_with_ema: every `Test loss` / `Test net output` value printed equals, to the printed digits, the binding's eval_stats means
    under ema_use on an engine that holds that iteration's average (ema_put of the run's own .ema.caffemodel) -- and differs from the
    means on the ordinary weights;
  * a resumed run takes the average from the .ema.caffemodel beside the restored model, or, with that file gone, starts it from the
    restored weights, and says which: after one more update the new average is decay * e + om * W' in float32 for that e and the run's
    own new weights W';
  * without the fields no .ema.caffemodel is written and the log names none of it; with ema_decay: -1 the models are byte-identical to
    those and the log is line for line the same (the parent commit's binary is not available to a test: "today's run" is represented
    by the run without the fields, as tests/test_gpu_facade_clip.py does)."""
import os
import re

import numpy as np
import pytest

from tests.test_facade_proto import pb, tool  # noqa: F401  (fixtures)
from tests.test_gpu_facade import read_caffemodel, run_caffe, write_caffemodel
from videovector_amd.prototxt import solver, train_net
from videovector_amd.synth import SyntheticVideos, init_weights

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, V = 32, 5, 2, 128, 32, 50
HB, HV, HSEED = 24, 40, 99
ENV = {"VV_DEDUP": "0", "VV_SLAB16": "0"}
ITERS, TEST_ITER, TEST_INTERVAL = 4, 3, 2
DECAY = 0.9
TRAIN_SRC = "synthetic://videos=%d;seed=1701;features=%d" % (V, F)
HELD_SRC = "synthetic://videos=%d;seed=%d;features=%d" % (HV, HSEED, F)


def job(pb, d, held_out=True, max_iter=ITERS, resume=None, prefix="snap", **extra):  # noqa: F811
    d.mkdir(exist_ok=True)
    net_p, sol_p = d / ("net_%s.prototxt" % prefix), d / ("solver_%s.prototxt" % prefix)
    kw = dict(held_out_source=HELD_SRC, held_out_batch=HB) if held_out else {}
    net_p.write_text(train_net(TRAIN_SRC, B, C, Nn, D, max_buffer=500, w_std=0.02, **kw))
    tkw = dict(test_iter=TEST_ITER, test_interval=TEST_INTERVAL, test_compute_loss=True) if held_out else {}
    sol_p.write_text(solver(str(net_p), display=1, lr_policy="fixed", base_lr=0.01, momentum=0.9, max_iter=max_iter, snapshot=TEST_INTERVAL,
                            snapshot_prefix=str(d / prefix), **tkw, **extra))
    W0, b0 = init_weights(3, D, F, std=0.02)
    write_caffemodel(pb, str(d / "init.caffemodel"), W0, b0)
    how = ["--snapshot=%s" % resume] if resume else ["--weights=%s" % (d / "init.caffemodel")]
    log = run_caffe(["train", "--solver=%s" % sol_p] + how, str(d / ("train_%s.log" % prefix)), ENV)
    lines = [re.sub(r"^[IWEF]\d{4} \d\d:\d\d:\d\d\.\d{6} +\d+ ([\w.]+):\d+\] ", r"\1] ", ln).replace(str(d), "<dir>") for ln in log.splitlines()]
    return log, lines, W0, b0


def model(pb, d, it, ema=False, prefix="snap"):  # noqa: F811
    return read_caffemodel(pb, str(d / ("%s_iter_%d%s.caffemodel" % (prefix, it, ".ema" if ema else ""))))


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ema_ref(e, w):
    d = np.float32(DECAY)
    return d * e + (np.float32(1.0) - d) * w


def printed_tests(log):
    parts = re.split(r"Iteration (\d+), Testing net \(#0\)", log)[1:]
    out = []
    for body in parts[1::2]:
        tl = re.search(r"Test loss: (\S+)", body)
        lo = re.search(r"Test net output #0: loss_output = (\S+) \(\* 1 = (\S+) loss\)", body)
        vi = re.search(r"Test net output #1: train_violations = (\S+)", body)
        assert tl and lo and vi, body[:2000]
        out.append((float(tl.group(1)), float(lo.group(1)), float(vi.group(1))))
    return [int(x) for x in parts[0::2]], out


def test_caffe_train_with_a_moving_average(tool, pb, tmp_path):  # noqa: F811
    import videovector_amd as vv
    d = tmp_path / "ema"
    log, _, W0, b0 = job(pb, d, ema_decay=DECAY, test_with_ema=True)
    assert "ema_decay: 0.9 -- a moving average" in log and "Held-out branch" in log
    for it in (TEST_INTERVAL, ITERS):
        assert ("Snapshotting the moving average to %s" % (d / ("snap_iter_%d.ema.caffemodel" % it))) in log

    # ---- the engine over the same sampler stream: the weights and the average after every update
    ds = SyntheticVideos(seed=1701, n_videos=V)
    smp = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=B, context_size=C, num_negative_samples=Nn, max_buffer_size=500,
                     negative_swap_percentage=50)
    eng = vv.Engine(0, "f16")
    avg = {0: (W0, b0)}
    try:
        eng.set_dedup(False); eng.set_option("slab16", 0)
        eng.table_synth(ds.seed, ds.n_rows, F)
        eng.params_set(W0, b0)
        eng.ema_set(DECAY)
        cfg = vv.StepConfig(B, C, Nn, lr=0.01, momentum=0.9)
        for it in range(1, ITERS + 1):                     # as Solver::Step on a display iteration: hint, pass, the loss, the update
            eng.update_hint(cfg)
            eng.forward_backward(cfg, smp.next())
            eng.loss()
            eng.apply_update(cfg)
            if it in (TEST_INTERVAL, ITERS):
                avg[it] = eng.ema_get()
                We, be, _, _ = eng.params_get()
                Wm, bm, net = model(pb, d, it)
                Wa, ba, neta = model(pb, d, it, ema=True)
                assert bits(Wm, We) and bits(bm, be), "iteration %d: the caffemodel differs from the engine's weights" % it
                assert bits(Wa, avg[it][0]) and bits(ba, avg[it][1]), "iteration %d: the .ema.caffemodel differs from the engine's ema_get" % it
                assert not bits(Wa, Wm)
                assert [(l.name, l.type, len(l.blobs)) for l in neta.layers] == [(l.name, l.type, len(l.blobs)) for l in net.layers] and neta.name == net.name
    finally:
        eng.close()
        smp.close()

    # ---- test_with_ema: the printed means are the binding's under ema_use, on the held-out stream
    at, printed = printed_tests(log)
    assert at == [0, TEST_INTERVAL, ITERS], at
    assert log.count("Testing on the moving average of the parameters (ema_decay 0.9)") == 3
    hs = SyntheticVideos(seed=HSEED, n_videos=HV)

    def held_out_means(use_ema):
        s = vv.Sampler(hs.video_id, hs.n_shots, hs.row_base, batch_size=HB, context_size=C, num_negative_samples=Nn, max_buffer_size=500,
                       negative_swap_percentage=50)
        ev = vv.Engine(0, "f16")
        out = []
        try:
            ev.set_dedup(False); ev.set_option("slab16", 0)
            ev.table_synth(hs.seed, hs.n_rows, F)
            hcfg = vv.StepConfig(HB, C, Nn)
            for it in at:
                ev.params_set(*((W0, b0) if it == 0 else model(pb, d, it)[:2]))      # the last iterate ...
                ev.ema_set(DECAY)
                ev.ema_put(*avg[it])                                                    # ... and that iteration's average beside it
                ev.ema_use(use_ema)
                ev.eval_reset()
                for _ in range(TEST_ITER):
                    ev.forward(hcfg, s.next())
                st = ev.eval_stats()
                ev.ema_use(False)
                ev.ema_set(-1)
                assert st.passes == TEST_ITER
                out.append((float("%g" % st.mean_loss), float("%g" % st.mean_loss), float("%g" % st.mean_violations)))
        finally:
            ev.close()
            s.close()
        return out

    want, last_iterate = held_out_means(True), held_out_means(False)
    print("FACADE-EMA printed %r, under ema_use %r, on the last iterate %r" % (printed, want, last_iterate))
    assert printed == want
    assert want[0] == last_iterate[0] and want[1:] != last_iterate[1:]       # (at iteration 0 the average is the weights)

    # ---- resumed from iteration 2, one more update: with the averaged model beside the restored one, and without it
    state = str(d / ("snap_iter_%d.solverstate" % TEST_INTERVAL))
    W2, b2, _ = model(pb, d, TEST_INTERVAL)
    e2 = model(pb, d, TEST_INTERVAL, ema=True)[:2]
    logr, _, _, _ = job(pb, d, held_out=False, max_iter=TEST_INTERVAL + 1, resume=state, prefix="with", ema_decay=DECAY)
    assert ("Restoring the moving average from %s" % (d / ("snap_iter_%d.ema.caffemodel" % TEST_INTERVAL))) in logr
    os.unlink(str(d / ("snap_iter_%d.ema.caffemodel" % TEST_INTERVAL)))
    logn, _, _, _ = job(pb, d, held_out=False, max_iter=TEST_INTERVAL + 1, resume=state, prefix="without", ema_decay=DECAY)
    assert "the moving average starts from the restored weights" in logn and "Restoring the moving average" not in logn
    for prefix, (eW, eb) in (("with", e2), ("without", (W2, b2))):
        W3, b3, _ = model(pb, d, TEST_INTERVAL + 1, prefix=prefix)
        Wa, ba, _ = model(pb, d, TEST_INTERVAL + 1, ema=True, prefix=prefix)
        assert (W3 != W2).mean() > 0.99
        assert bits(Wa, ema_ref(eW, W3)) and bits(ba, ema_ref(eb, b3)), "resumed %s the averaged model: the next average is not decay * e + om * W'" % prefix
    assert not bits(model(pb, d, TEST_INTERVAL + 1, ema=True, prefix="with")[0], model(pb, d, TEST_INTERVAL + 1, ema=True, prefix="without")[0])

    # ---- without the fields: no averaged model, nothing of it in the log; ema_decay: -1 is that run
    p = tmp_path / "plain"
    log0, lines0, _, _ = job(pb, p)
    m = tmp_path / "minus_one"
    log1, lines1, _, _ = job(pb, m, ema_decay=-1)
    for q in (p, m):
        assert not [f for f in os.listdir(str(q)) if ".ema." in f]
    assert not [ln for ln in lines0 if re.search(r"\bema\b|ema_decay|moving average", ln)]
    assert [ln for ln in lines1 if not re.match(r"^(\S+\] )?ema_decay: -1$", ln)] == lines0
    for it in (TEST_INTERVAL, ITERS):
        name = "snap_iter_%d.caffemodel" % it
        assert (p / name).read_bytes() == (m / name).read_bytes(), name
        Wp, bp, _ = model(pb, p, it)
        Wm, bm, _ = model(pb, d, it)
        assert bits(Wp, Wm) and bits(bp, bm), "iteration %d: training with the average is not the training without it" % it
    assert printed_tests(log0)[1] == last_iterate                            # (the run without the fields tests on the last iterate)
