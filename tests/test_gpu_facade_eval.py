"""`caffe train` with a held-out branch (videovector_amd.prototxt.train_net(held_out_source=...): the TRAIN graph under
include { phase: TEST } on a second data source), test_interval 2, test_iter 3, test_compute_loss, on the smallest facade fixture (the one
tests/test_gpu_facade_accum.py uses).  The TEST-phase net is matched to the fused plan and Net::Forward runs the library's forward-only
pass; Solver::Test averages its loss and train_violations tops over the three passes.

  * every `Test loss` and `Test net output` value printed (at iterations 0, 2 and 4) equals, to the printed digits, the binding's
    eval_stats means: the engine driven with the same weights (the run's own caffemodels) and the same sampler stream, three passes
    per test in the order the solver runs them;
  * the training log lines (loss, Train net output, lr) and the final caffemodel are bit-equal to a run of the same solver on the same
    net without the held-out branch."""
import re

import numpy as np
import pytest

from tests.test_facade_proto import pb, tool  # noqa: F401  (fixtures)
from tests.test_gpu_facade import read_caffemodel, run_caffe, write_caffemodel
from videovector_amd.prototxt import solver, train_net
from videovector_amd.synth import SyntheticVideos, init_weights

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, V = 32, 5, 2, 128, 32, 50
HB, HV, HSEED = 24, 40, 99              # the held-out source: other videos, another batch size
ENV = {"VV_DEDUP": "0", "VV_SLAB16": "0"}
ITERS, TEST_ITER, TEST_INTERVAL = 4, 3, 2
TRAIN_SRC = "synthetic://videos=%d;seed=1701;features=%d" % (V, F)
HELD_SRC = "synthetic://videos=%d;seed=%d;features=%d" % (HV, HSEED, F)


def write_job(pb, d, held_out):  # noqa: F811
    d.mkdir(exist_ok=True)
    net_p, sol_p = d / "net.prototxt", d / "solver.prototxt"
    kw = dict(held_out_source=HELD_SRC, held_out_batch=HB) if held_out else {}
    net_p.write_text(train_net(TRAIN_SRC, B, C, Nn, D, max_buffer=500, w_std=0.02, dropout=0.5, **kw))
    tkw = dict(test_iter=TEST_ITER, test_interval=TEST_INTERVAL, test_compute_loss=True) if held_out else {}
    sol_p.write_text(solver(str(net_p), display=1, lr_policy="fixed", base_lr=0.01, momentum=0.9, max_iter=ITERS, snapshot=TEST_INTERVAL,
                            snapshot_prefix=str(d / "snap"), random_seed=7, **tkw))
    W0, b0 = init_weights(3, D, F, std=0.02)
    write_caffemodel(pb, str(d / "init.caffemodel"), W0, b0)
    log = run_caffe(["train", "--solver=%s" % sol_p, "--weights=%s" % (d / "init.caffemodel")], str(d / "train.log"), ENV)
    return log, W0, b0


def train_lines(log):
    """what a training iteration logs: loss, outputs, rate (without the glog prefix)"""
    out = []
    for line in log.splitlines():
        m = re.search(r"(Iteration \d+, (?:loss|lr) = \S+|Train net output #\d+: .*)$", line)
        if m:
            out.append(m.group(1))
    return out


def test_caffe_train_with_a_held_out_branch(tool, pb, tmp_path):  # noqa: F811
    log, W0, b0 = write_job(pb, tmp_path / "held", True)
    assert "phase: TEST" in (tmp_path / "held" / "net.prototxt").read_text()
    assert "Held-out branch" in log and "Not the fused videovec pattern" not in log
    # ---- what Solver::Test printed, test by test
    tests = re.split(r"Iteration (\d+), Testing net \(#0\)", log)[1:]
    at = [int(x) for x in tests[0::2]]
    assert at == [0, TEST_INTERVAL, ITERS], at
    printed = []
    for body in tests[1::2]:
        tl = re.search(r"Test loss: (\S+)", body)
        lo = re.search(r"Test net output #0: loss_output = (\S+) \(\* 1 = (\S+) loss\)", body)
        vi = re.search(r"Test net output #1: train_violations = (\S+)", body)
        assert tl and lo and vi, body[:2000]
        printed.append((float(tl.group(1)), float(lo.group(1)), float(vi.group(1))))
    # ---- the binding on the same weights and the same sampler stream
    import videovector_amd as vv
    ds = SyntheticVideos(seed=HSEED, n_videos=HV)
    smp = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=HB, context_size=C, num_negative_samples=Nn,
                     max_buffer_size=500, negative_swap_percentage=50)
    eng = vv.Engine(0, "f16")
    try:
        eng.set_dedup(False); eng.set_option("slab16", 0)
        eng.table_synth(ds.seed, ds.n_rows, F)
        cfg = vv.StepConfig(HB, C, Nn)                                      # dropout_ratio 0: the TEST phase
        for k, it in enumerate(at):
            W, b = (W0, b0) if it == 0 else read_caffemodel(pb, str(tmp_path / "held" / ("snap_iter_%d.caffemodel" % it)))[:2]
            eng.params_set(W, b)
            eng.eval_reset()
            for _ in range(TEST_ITER):
                eng.forward(cfg, smp.next())
            st = eng.eval_stats()
            assert st.passes == TEST_ITER and st.terms == TEST_ITER * HB * Nn
            print("FACADE-EVAL iteration %d: printed %r, binding mean loss %r violations %r" % (it, printed[k], st.mean_loss, st.mean_violations))
            assert printed[k][0] == float("%g" % st.mean_loss), (it, printed[k], st)
            assert printed[k][1] == float("%g" % st.mean_loss) and printed[k][2] == float("%g" % st.mean_violations), (it, printed[k], st)
    finally:
        eng.close()
        smp.close()
    assert printed[0] != printed[1] != printed[2]
    # ---- the same solver without the held-out branch: the training run is the same run
    log0, _, _ = write_job(pb, tmp_path / "plain", False)
    assert "Testing net" not in log0
    a, b_ = train_lines(log), train_lines(log0)
    assert len(a) >= 3 * ITERS and a == b_, "the training log lines differ from the run without the held-out branch"
    for it in (TEST_INTERVAL, ITERS):
        Wh, bh, _ = read_caffemodel(pb, str(tmp_path / "held" / ("snap_iter_%d.caffemodel" % it)))
        Wp, bp, _ = read_caffemodel(pb, str(tmp_path / "plain" / ("snap_iter_%d.caffemodel" % it)))
        assert np.array_equal(Wh.view(np.uint32), Wp.view(np.uint32)) and np.array_equal(bh.view(np.uint32), bp.view(np.uint32)), \
            "the caffemodel of iteration %d differs from the run without the held-out branch" % it
    assert (Wh != W0).mean() > 0.99
