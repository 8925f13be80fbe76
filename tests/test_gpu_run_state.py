"""The step's carried state (vv_run_state_*; Engine.run_state / set_run_state) with the sampler's (Sampler.state / set_state): a run
resumed into a fresh context and a fresh sampler is, bit for bit, the run that was never interrupted.

Run A: eight steps.  Run B: four steps; then parameters, histories, Adam's t, the run state and the sampler state are read and put -- in
the documented order: params_set, history2_set, solver_iter, set_run_state -- into a fresh Engine and a fresh Sampler, which run four
more.  Every step's loss and violations, the final W, b, histories and a vv_forward loss (it reads the 16-bit copy of W) must be equal
as bits.  Control: the same without set_run_state must differ under counter dropout (the counter restarts), which shows the test can tell.

Shape: the exact-update tests' small one (B = 8, a few negatives, D = 512: the de-duplicated segment-wise path with f16 rows and f16
slabs, the defaults), counter dropout 0.5, and a large learning rate in the SGD cases, so that the weights -- and with them the
16-bit scales, which follow max |W| one update late -- move from step to step."""
import numpy as np
import pytest

from videovector_amd.engine import VVError
from videovector_amd.synth import SyntheticVideos, init_weights

pytestmark = pytest.mark.gpu

VV_ERR_ARG, VV_ERR_STATE = 1, 3
B, CTX, NN, F, D = 8, 5, 3, 256, 512
DS = SyntheticVideos(seed=4242, n_videos=40)
SAMPLER_KW = dict(batch_size=B, context_size=CTX, num_negative_samples=NN, max_buffer_size=40, negative_swap_percentage=50)
EVAL_IDX = np.random.default_rng(5).integers(0, DS.n_rows, size=(B, CTX + NN)).astype(np.int32)

CASES = {
    # name: (solver keywords, hinted vv_step?, options)
    "sgd_step": (dict(solver_type="SGD", lr=0.5, momentum=0.9), True, {}),
    "adam_fb_update": (dict(solver_type="ADAM", lr=0.01, momentum=0.9, momentum2=0.999, delta=1e-8), False, {}),
    "h16_guard2": (dict(solver_type="SGD", lr=0.5, momentum=0.9), True, {"h16_guard": 2}),
    "dense": (dict(solver_type="SGD", lr=0.5, momentum=0.9), True, {"dedup": 0}),
}


def new_engine(vv, options):
    eng = vv.Engine(0, "f16")
    for k, v in options.items():
        eng.set_option(k, v)
    eng.table_synth(DS.seed, DS.n_rows, F)
    return eng


def new_sampler(vv):
    return vv.Sampler(DS.video_id, DS.n_shots, DS.row_base, **SAMPLER_KW)


def cfg_of(vv, solver_kw):
    return vv.StepConfig(B, CTX, NN, dropout_ratio=0.5, dropout_seed=77, weight_decay=5e-4, **solver_kw)


def run_steps(eng, smp, cfg, hinted, n):
    out = []
    for _ in range(n):
        idx = smp.next()
        if hinted:
            eng.step(cfg, idx)
        else:
            eng.forward_backward(cfg, idx)
            eng.apply_update(cfg)
        out.append(eng.loss())
    return out


def final_state(vv, eng, adam):
    W, b, hW, hb = eng.params_get()
    h2 = eng.history2_get() if adam else ()
    ev = vv.StepConfig(B, CTX, NN)
    eng.eval_reset()
    eng.forward(ev, EVAL_IDX)
    return [W, b, hW, hb, *h2, np.float32(eng.eval_stats().last_loss)]


def resume(vv, case, with_run_state):
    solver_kw, hinted, options = CASES[case]
    adam = solver_kw["solver_type"] == "ADAM"
    W0, b0 = init_weights(3, D, F, std=0.02)
    eng, smp, cfg = new_engine(vv, options), new_sampler(vv), cfg_of(vv, solver_kw)
    eng.params_set(W0, b0)
    losses = run_steps(eng, smp, cfg, hinted, 4)
    W, b, hW, hb = eng.params_get()
    h2 = eng.history2_get() if adam else None
    t = eng.solver_iter
    run_blob, smp_blob = eng.run_state(), smp.state()
    eng.close(), smp.close()
    eng2, smp2 = new_engine(vv, options), new_sampler(vv)
    eng2.params_set(W, b, hW, hb)
    if adam:
        eng2.history2_set(*h2)
    eng2.solver_iter = t
    if with_run_state:
        eng2.set_run_state(run_blob)
    smp2.set_state(smp_blob)
    losses += run_steps(eng2, smp2, cfg_of(vv, solver_kw), hinted, 4)
    fin = final_state(vv, eng2, adam)
    eng2.close(), smp2.close()
    return losses, fin


@pytest.fixture(scope="module")
def vv():
    import videovector_amd
    return videovector_amd


@pytest.mark.parametrize("case", sorted(CASES))
def test_resumed_run_is_the_uninterrupted_one(vv, case):
    solver_kw, hinted, options = CASES[case]
    adam = solver_kw["solver_type"] == "ADAM"
    W0, b0 = init_weights(3, D, F, std=0.02)
    eng, smp, cfg = new_engine(vv, options), new_sampler(vv), cfg_of(vv, solver_kw)
    eng.params_set(W0, b0)
    want_losses = run_steps(eng, smp, cfg, hinted, 8)
    want = final_state(vv, eng, adam)
    eng.close(), smp.close()
    got_losses, got = resume(vv, case, True)
    print(case, "losses A", want_losses, "B", got_losses, "forward loss A", want[-1], "B", got[-1])
    assert got_losses == want_losses
    for name, a, g in zip(("W", "b", "hW", "hb", "vW", "vb") if adam else ("W", "b", "hW", "hb"), want, got):
        assert np.array_equal(a.view(np.uint32), g.view(np.uint32)), name
    assert np.float32(want[-1]).tobytes() == np.float32(got[-1]).tobytes()
    if case == "sgd_step":          # the control: without the run state the dropout counter restarts and the run is another one
        ctl_losses, ctl = resume(vv, case, False)
        assert ctl_losses[:4] == want_losses[:4]
        assert ctl_losses[4:] != want_losses[4:] and not np.array_equal(ctl[0], want[0])


def test_refusals(vv):
    solver_kw, _, _ = CASES["sgd_step"]
    cfg = cfg_of(vv, solver_kw)
    W0, b0 = init_weights(3, D, F, std=0.02)
    eng, smp = new_engine(vv, {}), new_sampler(vv)

    def refused(fn, code):
        with pytest.raises(VVError) as e:
            fn()
        assert e.value.code == code, str(e.value)

    refused(eng.run_state, VV_ERR_STATE)                                   # no parameters
    eng.params_set(W0, b0)
    fresh = eng.run_state()
    eng.step(cfg, smp.next())
    blob = eng.run_state()
    assert blob != fresh and eng.run_state() == blob
    # a gradient is held: a backward pass waits for its update (get), any gradient at all (put)
    eng.forward_backward(cfg, smp.next())
    refused(eng.run_state, VV_ERR_STATE)
    refused(lambda: eng.set_run_state(blob), VV_ERR_STATE)
    eng.apply_update(cfg)
    eng.run_state()
    refused(lambda: eng.set_run_state(blob), VV_ERR_STATE)                 # (the consumed gradient is still held)
    # gradients are banked
    eng.forward_backward(cfg, smp.next())
    eng.grads_bank()
    refused(eng.run_state, VV_ERR_STATE)
    eng.grads_bank_reset()
    W, b, hW, hb = eng.params_get()
    eng.params_set(W, b, hW, hb)
    # the average is in use
    eng.ema_set(0.5)
    eng.ema_use(True)
    refused(eng.run_state, VV_ERR_STATE)
    refused(lambda: eng.set_run_state(blob), VV_ERR_STATE)
    eng.ema_use(False)
    eng.ema_set(-1.0)
    # the overlapped and the sharded schedule
    for schedule in (1, 2):
        eng.L.vv_comm_schedule(eng.h, schedule)
        refused(eng.run_state, VV_ERR_STATE)
        refused(lambda: eng.set_run_state(blob), VV_ERR_STATE)
        eng.L.vv_comm_schedule(eng.h, 0)
    # the blob itself: truncated, over-long, a wrong version, D, F
    eng.set_run_state(blob)
    bad_version = bytearray(blob); bad_version[8] ^= 0x02
    for bad in (blob[:-1], blob[:64], b"", blob + b"\0", bytes(bad_version)):
        refused(lambda: eng.set_run_state(bad), VV_ERR_ARG)
    other = new_engine(vv, {})
    other.params_set(*init_weights(3, 1024, F, std=0.02))
    refused(lambda: other.set_run_state(blob), VV_ERR_ARG)                 # another D
    other.close()
    other = vv.Engine(0, "f16")
    other.table_synth(DS.seed, DS.n_rows, 128)
    other.params_set(*init_weights(3, D, 128, std=0.02))
    refused(lambda: other.set_run_state(blob), VV_ERR_ARG)                 # another F
    other.close()
    eng.close(), smp.close()
