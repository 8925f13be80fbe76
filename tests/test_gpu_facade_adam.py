"""`caffe train` with solver_type: ADAM (and RMSPROP) on the smallest facade fixture: the solverstate holds four history blobs in BVLC
AdamSolver's order (m of W, m of b, v of W, v of b); a restore writes them back bit for bit and continues the bias correction at
t = iter + 1 -- one resumed iteration must equal, bit for bit, the same update made through the Python binding from the snapshot's
state with vv_solver_iter_set(iter) (a resumed data layer starts over, as the reference's, so the resumed iteration reads the run's
first batch); an Adam run refuses a two-blob state; ADADELTA fails with one clear line.  (These need the device: the facade's solver
creates its context when it is constructed.)"""
import re
import subprocess

import numpy as np
import pytest

from tests.test_facade_proto import pb, tool  # noqa: F401  (fixtures)
from tests.test_gpu_facade import CAFFE, read_caffemodel, run_caffe, write_caffemodel
from videovector_amd.prototxt import solver, train_net
from videovector_amd.synth import SyntheticVideos, init_weights

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, V = 32, 5, 2, 128, 32, 50
ENV = {"VV_DEDUP": "0", "VV_SLAB16": "0"}


def state_of(pb, path):  # noqa: F811
    st = pb["SolverState"]()
    st.ParseFromString(open(path, "rb").read())
    return st


def hist(st, i):
    return np.array(st.history[i].data, np.float32)


def test_caffe_train_adam_snapshot_and_resume(tool, pb, tmp_path):  # noqa: F811
    import videovector_amd as vv
    net_p, sol_p = tmp_path / "net.prototxt", tmp_path / "solver.prototxt"
    net_p.write_text(train_net("synthetic://videos=%d;seed=1701;features=%d" % (V, F), B, C, Nn, D, max_buffer=500, w_std=0.02))
    kw = dict(base_lr=0.001, momentum=0.9, momentum2=0.99, max_iter=4, display=1, lr_policy="fixed", solver_type="ADAM", delta=1e-8,
              snapshot_prefix=str(tmp_path / "snap"))
    sol_p.write_text(solver(str(net_p), **kw))
    W0, b0 = init_weights(3, D, F, std=0.02)
    write_caffemodel(pb, str(tmp_path / "init.caffemodel"), W0, b0)
    log = run_caffe(["train", "--solver=%s" % sol_p, "--weights=%s" % (tmp_path / "init.caffemodel")], str(tmp_path / "train.log"), ENV)
    losses = [float(x) for x in re.findall(r"Iteration \d+, loss = ([0-9.eE+-]+)", log)]
    assert len(losses) == 5 and all(np.isfinite(losses))
    st = state_of(pb, tmp_path / "snap_iter_4.solverstate")
    assert st.iter == 4 and len(st.history) == 4, "an Adam solverstate holds four history blobs"
    shapes = [(h.height, h.width) for h in st.history]
    assert shapes == [(D, F), (1, D), (D, F), (1, D)], shapes
    m, v = hist(st, 0), hist(st, 2)
    assert (m < 0).any() and (m > 0).any() and (v >= 0).all() and (v > 0).mean() > 0.9, "the order is m of W, m of b, v of W, v of b"
    assert (hist(st, 3) >= 0).all() and hist(st, 3).max() > 0
    W4, b4, _ = read_caffemodel(pb, str(tmp_path / "snap_iter_4.caffemodel"))
    assert (W4 != W0).mean() > 0.99

    # resume for ONE more iteration
    sol2 = tmp_path / "solver2.prototxt"
    sol2.write_text(solver(str(net_p), **dict(kw, max_iter=5, snapshot_prefix=str(tmp_path / "re"))))
    log2 = run_caffe(["train", "--solver=%s" % sol2, "--snapshot=%s" % (tmp_path / "snap_iter_4.solverstate")], str(tmp_path / "resume.log"), ENV)
    assert "Restoring previous solver status" in log2 and "AdamSolver: restoring history" in log2
    loss_r = [float(x) for x in re.findall(r"Iteration 4, loss = ([0-9.eE+-]+)", log2)][0]
    W5, b5, _ = read_caffemodel(pb, str(tmp_path / "re_iter_5.caffemodel"))
    st5 = state_of(pb, tmp_path / "re_iter_5.solverstate")
    assert st5.iter == 5 and len(st5.history) == 4

    # the same update through the binding: the snapshot's state, t = 4 updates made, the run's first batch
    ds = SyntheticVideos(seed=1701, n_videos=V)
    idx = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=B, context_size=C, num_negative_samples=Nn, max_buffer_size=500,
                     negative_swap_percentage=50).next()
    eng = vv.Engine(0, "f16")
    try:
        eng.set_dedup(False); eng.set_option("slab16", 0)
        eng.table_synth(ds.seed, ds.n_rows, F)
        eng.params_set(W4, b4, hist(st, 0).reshape(D, F), hist(st, 1))
        eng.history2_set(hist(st, 2).reshape(D, F), hist(st, 3))
        eng.solver_iter = 4
        cfg = vv.StepConfig(B, C, Nn, lr=0.001, momentum=0.9, momentum2=0.99, solver_type="ADAM", delta=1e-8)
        eng.step(cfg, idx)
        loss_e = eng.loss()[0]
        We, be, mWe, mbe = eng.params_get()
        vWe, vbe = eng.history2_get()
        # ... and with t NOT restored the result is far away (the check below can tell)
        eng.params_set(W4, b4, hist(st, 0).reshape(D, F), hist(st, 1))
        eng.history2_set(hist(st, 2).reshape(D, F), hist(st, 3))
        eng.step(cfg, idx)
        assert not np.array_equal(eng.params_get()[0], We)
    finally:
        eng.close()
    assert loss_r == float("%g" % loss_e), "the logged loss of the resumed iteration (%r) is not the binding's (%r)" % (loss_r, loss_e)
    for name, a, e in (("W", W5, We), ("b", b5, be), ("m of W", hist(st5, 0), mWe.ravel()), ("m of b", hist(st5, 1), mbe),
                       ("v of W", hist(st5, 2), vWe.ravel()), ("v of b", hist(st5, 3), vbe)):
        assert np.array_equal(np.asarray(a).ravel(), np.asarray(e).ravel()), "%s after the resumed iteration differs from the update at t = 5" % name

    # an Adam run refuses a two-blob state; ADADELTA is one clear line
    sgd = tmp_path / "sgd.prototxt"
    sgd.write_text(solver(str(net_p), base_lr=0.001, max_iter=1, display=1, lr_policy="fixed", snapshot_prefix=str(tmp_path / "sgd")))
    run_caffe(["train", "--solver=%s" % sgd, "--weights=%s" % (tmp_path / "init.caffemodel")], str(tmp_path / "sgd.log"), ENV)
    assert len(state_of(pb, tmp_path / "sgd_iter_1.solverstate").history) == 2
    r = subprocess.run([CAFFE, "train", "--solver=%s" % sol2, "--snapshot=%s" % (tmp_path / "sgd_iter_1.solverstate")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "Incorrect length of history blobs" in (r.stderr + r.stdout)
    bad = tmp_path / "adadelta.prototxt"
    bad.write_text(solver(str(net_p), max_iter=1, solver_type="ADADELTA"))
    r = subprocess.run([CAFFE, "train", "--solver=%s" % bad], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ADADELTA is not implemented" in (r.stderr + r.stdout)


def test_caffe_train_rmsprop(tool, pb, tmp_path):  # noqa: F811
    net_p, sol_p = tmp_path / "net.prototxt", tmp_path / "solver.prototxt"
    net_p.write_text(train_net("synthetic://videos=%d;seed=1701;features=%d" % (V, F), B, C, Nn, D, max_buffer=500, w_std=0.02))
    kw = dict(base_lr=0.001, momentum=0.0, rms_decay=0.95, max_iter=2, display=1, lr_policy="fixed", solver_type="RMSPROP", delta=1e-8,
              snapshot_prefix=str(tmp_path / "snap"))
    sol_p.write_text(solver(str(net_p), **kw))
    W0, b0 = init_weights(3, D, F, std=0.02)
    write_caffemodel(pb, str(tmp_path / "init.caffemodel"), W0, b0)
    run_caffe(["train", "--solver=%s" % sol_p, "--weights=%s" % (tmp_path / "init.caffemodel")], str(tmp_path / "train.log"), ENV)
    st = state_of(pb, tmp_path / "snap_iter_2.solverstate")
    assert len(st.history) == 2 and (hist(st, 0) >= 0).all() and hist(st, 0).max() > 0
    W2, _, _ = read_caffemodel(pb, str(tmp_path / "snap_iter_2.caffemodel"))
    assert np.isfinite(W2).all() and (W2 != W0).mean() > 0.99
    bad = tmp_path / "bad.prototxt"
    bad.write_text(solver(str(net_p), **dict(kw, momentum=0.9)))
    r = subprocess.run([CAFFE, "train", "--solver=%s" % bad], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Momentum cannot be used with RMSProp" in (r.stderr + r.stdout)
