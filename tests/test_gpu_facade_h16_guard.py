"""`caffe train` on a net whose fc7 bias is past f16's range: the Solver runs its engine with "h16_guard" 2, so the job switches to fp32 rows
of ip2 four iterations after the first saturated step, says so in ONE warning line naming the iteration and both counts, and finishes.
VV_H16_GUARD=1 in the environment keeps the library's report-only value: no switch, no line."""
import re

import numpy as np
import pytest

from tests.test_facade_proto import pb, tool  # noqa: F401  (fixtures)
from tests.test_gpu_facade import run_caffe, write_caffemodel
from videovector_amd.prototxt import solver, train_net
from videovector_amd.synth import init_weights

pytestmark = pytest.mark.gpu

LINE = r"Iteration (\d+), ip2 left f16's range: (\d+) saturated elements, (\d+) faint rows"


@pytest.mark.parametrize("guard_env", [None, "1"])
def test_caffe_train_warns_once_at_the_fallback_and_finishes(tool, pb, tmp_path, guard_env):  # noqa: F811
    B, C, Nn, F, D, V, iters = 16, 5, 10, 128, 512, 50, 8
    net_p, sol_p = tmp_path / "net.prototxt", tmp_path / "solver.prototxt"
    net_p.write_text(train_net("synthetic://videos=%d;seed=1701;features=%d" % (V, F), B, C, Nn, D, max_buffer=500, w_std=0.02))
    sol_p.write_text(solver(str(net_p), base_lr=0.001, max_iter=iters, display=1, snapshot=0, snapshot_prefix=str(tmp_path / "snap")))
    W0, b0 = init_weights(3, D, F, std=0.02)
    b0[:] = 0
    b0[7] = 131072.0                                   # every distinct row of every step saturates in column 7
    write_caffemodel(pb, str(tmp_path / "init.caffemodel"), W0, b0)
    env = {} if guard_env is None else {"VV_H16_GUARD": guard_env}
    log = run_caffe(["train", "--solver=%s" % sol_p, "--weights=%s" % (tmp_path / "init.caffemodel")], str(tmp_path / "train.log"), env)
    losses = [float(x) for x in re.findall(r"Iteration \d+, loss = ([0-9.eE+-]+)", log)]
    assert len(losses) == iters + 1 and np.isfinite(losses).all(), losses
    assert "Optimization Done." in log
    hits = re.findall(LINE, log)
    if guard_env == "1":
        assert hits == [], hits
        return
    assert len(hits) == 1, hits
    it, sat, faint = (int(v) for v in hits[0])
    assert it == 4 and 0 < sat <= B * (C + Nn) and faint == 0, hits      # one saturated element per distinct row of iteration 0
