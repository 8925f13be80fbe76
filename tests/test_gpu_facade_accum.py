"""`caffe train` with SolverParameter.iter_size (BVLC Caffe's field, read by name; Solver::Step and SGDSolver::Normalize) on the smallest
facade fixture, the one tests/test_gpu_facade_clip.py uses.  iter_size: 2, max_iter: 3 -- six batches in the sampler's usual order, three
updates: the final caffemodel equals, bit for bit, the engine driven through the binding over the same six batches (two banked per
update), and the loss logged for each iteration is that cycle's mean as the library forms it (float32: the sum in pass order times
1.0f / iter_size).  With solver_type: ADAM the solverstate after two iterations says iter 2, and ONE resumed iteration equals the
binding's cycle from the snapshot's state at t = 2 (a resumed data layer starts over, as the reference's: the run's first two batches):
iterations, snapshots and Adam's t count updates, not passes."""
import re

import numpy as np
import pytest

from tests.test_facade_proto import pb, tool  # noqa: F401  (fixtures)
from tests.test_gpu_facade import read_caffemodel, run_caffe, write_caffemodel
from tests.test_gpu_facade_adam import hist, state_of
from videovector_amd.prototxt import solver, train_net
from videovector_amd.synth import SyntheticVideos, init_weights

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, V = 32, 5, 2, 128, 32, 50
ENV = {"VV_DEDUP": "0", "VV_SLAB16": "0"}
ITER_SIZE = 2


def write_nets(pb, d, **kw):  # noqa: F811
    net_p, sol_p = d / "net.prototxt", d / "solver.prototxt"
    net_p.write_text(train_net("synthetic://videos=%d;seed=1701;features=%d" % (V, F), B, C, Nn, D, max_buffer=500, w_std=0.02))
    sol_p.write_text(solver(str(net_p), display=1, lr_policy="fixed", iter_size=ITER_SIZE, **kw))
    W0, b0 = init_weights(3, D, F, std=0.02)
    write_caffemodel(pb, str(d / "init.caffemodel"), W0, b0)
    return net_p, sol_p, W0, b0


class Binding:
    """the engine and the sampler the facade's run is restated with"""

    def __init__(self):
        import videovector_amd as vv
        self.vv = vv
        ds = SyntheticVideos(seed=1701, n_videos=V)
        self.smp = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=B, context_size=C, num_negative_samples=Nn,
                              max_buffer_size=500, negative_swap_percentage=50)
        self.eng = vv.Engine(0, "f16")
        self.eng.set_dedup(False); self.eng.set_option("slab16", 0)
        self.eng.table_synth(ds.seed, ds.n_rows, F)

    def cycle(self, cfg):
        """one iteration of Solver::Step with iter_size passes -> the mean loss in float32"""
        total = None
        for _ in range(ITER_SIZE):
            self.eng.forward_backward(cfg, self.smp.next())
            l = np.float32(self.eng.loss()[0])
            total = l if total is None else total + l
            self.eng.grads_bank()
        self.eng.apply_update(cfg)
        assert int(self.eng.get_option("last_update_form")) == 1
        return total * (np.float32(1) / np.float32(ITER_SIZE))

    def close(self):
        self.eng.close()
        self.smp.close()


def test_caffe_train_iter_size(tool, pb, tmp_path):  # noqa: F811
    iters = 3
    _, sol_p, W0, b0 = write_nets(pb, tmp_path, base_lr=0.01, momentum=0.9, max_iter=iters, snapshot_prefix=str(tmp_path / "snap"))
    assert "iter_size: 2" in sol_p.read_text()
    log = run_caffe(["train", "--solver=%s" % sol_p, "--weights=%s" % (tmp_path / "init.caffemodel")], str(tmp_path / "train.log"), ENV)
    W, b, _ = read_caffemodel(pb, str(tmp_path / ("snap_iter_%d.caffemodel" % iters)))
    assert state_of(pb, tmp_path / ("snap_iter_%d.solverstate" % iters)).iter == iters
    logged = dict((int(i), float(x)) for i, x in re.findall(r"Iteration (\d+), loss = ([0-9.eE+-]+)", log))
    assert sorted(logged) == list(range(iters + 1)), log[-3000:]
    assert len(re.findall(r"Iteration \d+, lr = ", log)) == iters, "the learning-rate policy advances once per update"
    bd = Binding()
    try:
        bd.eng.params_set(W0, b0)
        cfg = bd.vv.StepConfig(B, C, Nn, lr=0.01, momentum=0.9)
        means = [bd.cycle(cfg) for _ in range(iters)]
        We, be, _, _ = bd.eng.params_get()
        s = bd.eng.accum_stats()
        assert (s["last_count"], s["updates"]) == (ITER_SIZE, iters) and s["last_mean_loss"] == means[-1]
    finally:
        bd.close()
    assert (W != W0).mean() > 0.99
    assert np.array_equal(W.view(np.uint32), We.view(np.uint32)) and np.array_equal(b.view(np.uint32), be.view(np.uint32)), \
        "caffe train with iter_size: 2 differs from the engine banking the same six batches"
    for k, mean in enumerate(means):
        assert logged[k] == float("%g" % mean), "iteration %d: the logged loss %r is not the cycle's mean %r" % (k, logged[k], float(mean))


def test_caffe_train_iter_size_adam_resume(tool, pb, tmp_path):  # noqa: F811
    kw = dict(base_lr=0.001, momentum=0.9, momentum2=0.99, solver_type="ADAM", delta=1e-8)
    net_p, sol_p, W0, b0 = write_nets(pb, tmp_path, max_iter=2, snapshot_prefix=str(tmp_path / "snap"), **kw)
    run_caffe(["train", "--solver=%s" % sol_p, "--weights=%s" % (tmp_path / "init.caffemodel")], str(tmp_path / "train.log"), ENV)
    st = state_of(pb, tmp_path / "snap_iter_2.solverstate")
    assert st.iter == 2 and len(st.history) == 4
    W2, b2, _ = read_caffemodel(pb, str(tmp_path / "snap_iter_2.caffemodel"))
    sol2 = tmp_path / "solver2.prototxt"
    sol2.write_text(solver(str(net_p), display=1, lr_policy="fixed", iter_size=ITER_SIZE, max_iter=3, snapshot_prefix=str(tmp_path / "re"), **kw))
    log2 = run_caffe(["train", "--solver=%s" % sol2, "--snapshot=%s" % (tmp_path / "snap_iter_2.solverstate")], str(tmp_path / "resume.log"), ENV)
    assert "AdamSolver: restoring history" in log2
    loss_r = [float(x) for x in re.findall(r"Iteration 2, loss = ([0-9.eE+-]+)", log2)][0]
    W3, b3, _ = read_caffemodel(pb, str(tmp_path / "re_iter_3.caffemodel"))
    st3 = state_of(pb, tmp_path / "re_iter_3.solverstate")
    assert st3.iter == 3 and len(st3.history) == 4
    bd = Binding()
    try:
        eng = bd.eng
        eng.params_set(W2, b2, hist(st, 0).reshape(D, F), hist(st, 1))
        eng.history2_set(hist(st, 2).reshape(D, F), hist(st, 3))
        eng.solver_iter = 2                                 # two UPDATES made (four passes)
        cfg = bd.vv.StepConfig(B, C, Nn, lr=0.001, momentum=0.9, momentum2=0.99, solver_type="ADAM", delta=1e-8)
        mean = bd.cycle(cfg)
        assert eng.solver_iter == 3
        We, be, mWe, mbe = eng.params_get()
        vWe, vbe = eng.history2_get()
    finally:
        bd.close()
    assert loss_r == float("%g" % mean)
    for name, a, e in (("W", W3, We), ("b", b3, be), ("m of W", hist(st3, 0), mWe), ("m of b", hist(st3, 1), mbe),
                       ("v of W", hist(st3, 2), vWe), ("v of b", hist(st3, 3), vbe)):
        assert np.array_equal(np.asarray(a, np.float32).ravel().view(np.uint32), np.asarray(e, np.float32).ravel().view(np.uint32)), \
            "%s after the resumed iteration differs from the binding's cycle at t = 3" % name
