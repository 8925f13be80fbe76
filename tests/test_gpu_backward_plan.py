"""The backward plan (videovector_amd/csrc/vv_backward_plan.h) from outside: after one forward_backward + apply_update on an f16 engine,
options "last_wgrad_splits" and "last_update_form" say which split of K the weight-gradient GEMM ran with and which form of the update
the gradient's place led to.  Expected values come from tests/backward_plan_ref.py fed with the same inputs -- the rules restated, not read
from the library -- and the shapes are the smallest on both sides of the edges a small shape reaches:

  the S <= 8 edge        D = F = 256 is one 256 x 256 tile, so S is the number of 64-row K-steps: B = 64 gives 512 rows, S = 8 (the gradient
                         stays in the slabs: form 3 / 4); B = 65 gives 520 rows padded to 768, S = 12 (reduced at once: k_sgd, form 1)
  F % 8 and F % 4        F = 256 (f16 slabs: form 4), 260 (fp32 slabs: 3), 254 (no 16-byte groups: the flat buffer, element-wise k_sgd: 2)
  options at the base    slab16 0 (form 3), fuse_update 0 (form 1), a grads_device() call before the step (form 1)

No parameter value is compared here: the exact tests own those.  The one-split epilogue form (S = 1, form 5) needs D = F = 4096 and stays
with tests/test_gpu_step_state.py."""
import os
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import vv  # noqa: F401  (fixture)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_plan_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS, D, C, NN = 2048, 256, 3, 5

# (id, B, F, options set before the step, grads_device() before the step)
CASES = [
    ("base", 64, 256, {}, False),
    ("twelve_k_steps", 65, 256, {}, False),
    ("F260", 64, 260, {}, False),
    ("F254", 64, 254, {}, False),
    ("slab16_off", 64, 256, {"slab16": 0}, False),
    ("fuse_update_off", 64, 256, {"fuse_update": 0}, False),
    ("grads_exposed", 64, 256, {}, True),
]


def expected(B, F, opts, exposed):
    Dp, Fp, Rp = ref.pad(D), ref.pad(F), ref.pad(B * (C + NN))
    S, _ = ref.split_k(Dp, Fp, Rp)
    plan = ref.backward(dict(world=0, comm_sharded=0, comm_overlap=0, D=D, F=F, Dp=Dp, Fp=Fp, Rp=Rp, B=B, S=S, grads_own=1,
                             grads_exposed=int(exposed), fuse_update=opts.get("fuse_update", 1), wgrad_update=1, slab16=opts.get("slab16", 1),
                             wgrad_lean=1, guard_proactive=1, fuse_keep_grads=0, can_fuse_update=1, hinted=0, hint_adam=0, hint_clip=0,
                             f16=1, dd=1, seg=0, table_rows=N_ROWS + 1))
    return S, ref.update_form(plan, F)


def test_the_cases_sit_on_both_sides_of_their_edges():
    """(needs no GPU work of its own: the reference alone) the shapes are what the docstring says they are"""
    got = {name: expected(B, F, opts, exposed) for name, B, F, opts, exposed in CASES}
    assert got == {"base": (8, 4), "twelve_k_steps": (12, 1), "F260": (8, 3), "F254": (8, 2), "slab16_off": (8, 3), "fuse_update_off": (8, 1),
                   "grads_exposed": (8, 1)}


@pytest.mark.parametrize("name,B,F,opts,exposed", CASES, ids=[c[0] for c in CASES])
def test_splits_and_update_form(vv, name, B, F, opts, exposed):  # noqa: F811
    from videovector_amd.synth import init_weights
    eng = vv.Engine(0, "f16")
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.table_synth(1701, N_ROWS, F)
    W, b = init_weights(1, D, F, std=0.02)
    eng.params_set(W, b)
    if exposed:
        eng.grads_device()
    idx = np.ascontiguousarray(np.random.default_rng(7).integers(0, N_ROWS, size=(B, C + NN), dtype=np.int32))
    cfg = vv.StepConfig(B, C, NN, lr=0.01, momentum=0.9, weight_decay=5e-4)
    eng.forward_backward(cfg, idx)
    eng.apply_update(cfg)
    loss, _ = eng.loss()
    assert np.isfinite(loss)
    got = (int(eng.get_option("last_wgrad_splits")), int(eng.get_option("last_update_form")))
    print("%s: splits, form = %s; the rules say %s" % (name, got, expected(B, F, opts, exposed)))
    assert got == expected(B, F, opts, exposed)
