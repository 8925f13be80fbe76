"""`caffe train --snapshot=...` with SolverParameter.snapshot_data_state: the resumed run is, bit for bit, the run that was never
interrupted -- and with the field off (the default) nothing changes: no file, and a resumed data layer starts over, as the reference's.

A small net (max_same_video_negs > 0: the general sampler path with quirk Q1's persistent slots; dropout 0.9: the counter mask; a
held-out branch with test_interval 2: a second sampler whose "Test loss" lines must continue too), max_iter 8, snapshot 4, once with SGD
and once with ADAM.  Run A goes straight through, run B resumes from _iter_4.solverstate."""
import os
import re

import numpy as np
import pytest

from tests.test_facade_proto import pb, tool  # noqa: F401  (fixtures)
from tests.test_gpu_facade import read_caffemodel, run_caffe, write_caffemodel
from tests.test_gpu_facade_adam import hist, state_of
from videovector_amd.prototxt import solver, train_net
from videovector_amd.synth import init_weights

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, V = 32, 5, 4, 128, 32, 50
HB, HV, HSEED = 24, 40, 99
TRAIN_SRC = "synthetic://videos=%d;seed=1701;features=%d" % (V, F)
HELD_SRC = "synthetic://videos=%d;seed=%d;features=%d" % (HV, HSEED, F)
SOLVERS = {"SGD": dict(base_lr=0.01, momentum=0.9),
           "ADAM": dict(base_lr=0.001, momentum=0.9, momentum2=0.99, solver_type="ADAM", delta=1e-8)}


def job(pb, d, kind, data_state, max_iter=8, resume_from=None, prefix="snap"):  # noqa: F811
    d.mkdir(exist_ok=True)
    net_p, sol_p = d / "net.prototxt", d / ("solver_%s.prototxt" % prefix)
    net_p.write_text(train_net(TRAIN_SRC, B, C, Nn, D, max_buffer=500, w_std=0.02, dropout=0.9, max_same=2,
                               held_out_source=HELD_SRC, held_out_batch=HB))
    sol_p.write_text(solver(str(net_p), display=1, lr_policy="fixed", max_iter=max_iter, snapshot=4, snapshot_prefix=str(d / prefix),
                            random_seed=7, test_iter=3, test_interval=2, test_compute_loss=True,
                            snapshot_data_state=True if data_state else None, **SOLVERS[kind]))
    if resume_from is None:
        W0, b0 = init_weights(3, D, F, std=0.02)
        write_caffemodel(pb, str(d / "init.caffemodel"), W0, b0)
        start = "--weights=%s" % (d / "init.caffemodel")
    else:
        start = "--snapshot=%s" % resume_from
    return run_caffe(["train", "--solver=%s" % sol_p, start], str(d / ("%s.log" % prefix)))


def lines_from(log, first_iter):
    """the loss, Train net output and Test loss lines from iteration first_iter on, without the glog prefix"""
    out, on = [], False
    for line in log.splitlines():
        m = re.search(r"(Iteration (\d+), (?:loss = \S+|Testing net.*)|Train net output #\d+: .*|Test loss: .*|Test net output #\d+: .*)$", line)
        if not m:
            continue
        if m.group(2) is not None:
            on = int(m.group(2)) >= first_iter
        if on:
            out.append(m.group(1))
    return out


@pytest.mark.parametrize("kind", ["SGD", "ADAM"])
def test_resumed_run_continues_the_same_run(tool, pb, tmp_path, kind):  # noqa: F811
    d = tmp_path / kind
    log_a = job(pb, d, kind, True)
    assert os.path.exists(d / "snap_iter_4.datastate") and "Snapshotting data state to" in log_a
    log_b = job(pb, d, kind, True, resume_from=d / "snap_iter_4.solverstate", prefix="re")
    assert "Restoring data state from" in log_b
    a, b = lines_from(log_a, 4), lines_from(log_b, 4)
    print("\n".join("A %s\nB %s" % (x, y) for x, y in zip(a, b)))
    assert sum("loss = " in x for x in a) == 5 and sum(x.startswith("Test loss") for x in a) == 3, a
    assert a == b
    Wa, ba, _ = read_caffemodel(pb, str(d / "snap_iter_8.caffemodel"))
    Wb, bb, _ = read_caffemodel(pb, str(d / "re_iter_8.caffemodel"))
    assert np.array_equal(Wa.view(np.uint32), Wb.view(np.uint32)) and np.array_equal(ba.view(np.uint32), bb.view(np.uint32))
    sa, sb = state_of(pb, d / "snap_iter_8.solverstate"), state_of(pb, d / "re_iter_8.solverstate")
    assert len(sa.history) == len(sb.history) == (4 if kind == "ADAM" else 2)
    for i in range(len(sa.history)):
        assert np.array_equal(hist(sa, i).view(np.uint32), hist(sb, i).view(np.uint32)), "history %d" % i


def test_field_off_changes_nothing_and_a_missing_file_starts_over(tool, pb, tmp_path):  # noqa: F811
    on, off = tmp_path / "on", tmp_path / "off"
    log_on = job(pb, on, "SGD", True, max_iter=4)
    log_off = job(pb, off, "SGD", False, max_iter=4)
    assert not [f for f in os.listdir(off) if f.endswith(".datastate")] and "data state" not in log_off
    for f in ("snap_iter_4.caffemodel",):          # (the solverstate names its model file by path: compared through its fields below)
        assert open(on / f, "rb").read() == open(off / f, "rb").read(), f
    s_on, s_off = state_of(pb, on / "snap_iter_4.solverstate"), state_of(pb, off / "snap_iter_4.solverstate")
    assert s_on.iter == s_off.iter == 4 and all(np.array_equal(hist(s_on, i), hist(s_off, i)) for i in range(2))
    assert lines_from(log_on, 0) == lines_from(log_off, 0)
    # field off: the resumed data layer starts over -- the resumed iteration reads the run's first batch.  Dropout's counter starts over
    # too, so iteration 4 of the resumed run is the update of the run's FIRST batch and mask on the snapshot's weights: the same lines as
    # a resume with the field on whose .datastate has been deleted, which must say so in one line
    log_r_off = job(pb, off, "SGD", False, max_iter=5, resume_from=off / "snap_iter_4.solverstate", prefix="re")
    assert "data state" not in log_r_off
    os.remove(on / "snap_iter_4.datastate")
    log_r_on = job(pb, on, "SGD", True, max_iter=5, resume_from=on / "snap_iter_4.solverstate", prefix="re")
    assert len(re.findall(r"No data state beside the restored solver state", log_r_on)) == 1 and "start over" in log_r_on
    assert lines_from(log_r_on, 4) == lines_from(log_r_off, 4)
    W_on = read_caffemodel(pb, str(on / "re_iter_5.caffemodel"))[0]
    W_off = read_caffemodel(pb, str(off / "re_iter_5.caffemodel"))[0]
    assert np.array_equal(W_on.view(np.uint32), W_off.view(np.uint32))
    # ... and that iteration is NOT the uninterrupted run's fifth (which a resume with the data state reproduces, above)
    log_5 = job(pb, tmp_path / "straight", "SGD", False, max_iter=5)
    it4 = lambda log: [x for x in lines_from(log, 4) if x.startswith("Iteration 4, loss")]
    assert len(it4(log_5)) == len(it4(log_r_off)) == 1 and it4(log_5) != it4(log_r_off)


def test_field_off_resumed_iteration_reads_the_first_batch(tool, pb, tmp_path):  # noqa: F811
    """The default resume keeps the parent's semantics, asserted as tests/test_gpu_facade_adam.py does: the one resumed iteration equals,
    bit for bit, the update made through the binding from the snapshot's state on the run's FIRST batch."""
    import videovector_amd as vv
    from videovector_amd.synth import SyntheticVideos
    env = {"VV_DEDUP": "0", "VV_SLAB16": "0"}
    nn = 2
    net_p = tmp_path / "net.prototxt"
    net_p.write_text(train_net(TRAIN_SRC, B, C, nn, D, max_buffer=500, w_std=0.02))
    kw = dict(base_lr=0.01, momentum=0.9, display=1, lr_policy="fixed")
    W0, b0 = init_weights(3, D, F, std=0.02)
    write_caffemodel(pb, str(tmp_path / "init.caffemodel"), W0, b0)
    sol = tmp_path / "solver.prototxt"
    sol.write_text(solver(str(net_p), max_iter=4, snapshot_prefix=str(tmp_path / "snap"), **kw))
    run_caffe(["train", "--solver=%s" % sol, "--weights=%s" % (tmp_path / "init.caffemodel")], str(tmp_path / "train.log"), env)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".datastate")]
    sol2 = tmp_path / "solver2.prototxt"
    sol2.write_text(solver(str(net_p), max_iter=5, snapshot_prefix=str(tmp_path / "re"), **kw))
    run_caffe(["train", "--solver=%s" % sol2, "--snapshot=%s" % (tmp_path / "snap_iter_4.solverstate")], str(tmp_path / "resume.log"), env)
    st = state_of(pb, tmp_path / "snap_iter_4.solverstate")
    W4, b4, _ = read_caffemodel(pb, str(tmp_path / "snap_iter_4.caffemodel"))
    W5, b5, _ = read_caffemodel(pb, str(tmp_path / "re_iter_5.caffemodel"))
    ds = SyntheticVideos(seed=1701, n_videos=V)
    idx = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=B, context_size=C, num_negative_samples=nn, max_buffer_size=500,
                     negative_swap_percentage=50).next()
    eng = vv.Engine(0, "f16")
    try:
        eng.set_dedup(False); eng.set_option("slab16", 0)
        eng.table_synth(ds.seed, ds.n_rows, F)
        eng.params_set(W4, b4, hist(st, 0).reshape(D, F), hist(st, 1))
        eng.step(vv.StepConfig(B, C, nn, lr=0.01, momentum=0.9), idx)
        We, be, _, _ = eng.params_get()
    finally:
        eng.close()
    assert np.array_equal(np.asarray(W5).ravel(), We.ravel()) and np.array_equal(np.asarray(b5).ravel(), be.ravel())
