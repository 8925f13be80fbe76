"""The forward-only pass under the three data-parallel schedules (vv_comm_overlap 0 / 1, vv_comm_schedule sharded), world 2 on the
shared-memory transport: every rank runs fb; apply_update; forward(held-out); fb; apply_update.  The pass orders itself behind an update
still in flight and is local to the rank, so its loss is bit-equal across the three schedules, and the final parameters (with the 16-bit
copy the next forward pass reads) are bit-equal to the same run without the pass.  Follows tests/test_gpu_comm_adam.py (two processes
sharing the one GPU, the same time limits)."""
import multiprocessing as mp
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, C, Nn, F, D = 32, 5, 4, 512, 256


def _rank_main(rank, world, id_path, schedule, with_forward, q):
    import videovector_amd as vv
    from videovector_amd.synth import SyntheticVideos, init_weights
    ds = SyntheticVideos(seed=21, n_videos=300)
    W, b = init_weights(21, D, F, std=0.02)
    s = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=world * B, context_size=C, num_negative_samples=Nn,
                   max_buffer_size=1000, negative_swap_percentage=50)
    batches = [s.next() for _ in range(3)]
    s.close()
    eng = vv.Engine(0, "f16")
    eng.table_synth(ds.seed, ds.n_rows, F)
    eng.params_set(W, b)
    eng.comm_init(world, rank, id_path, "shm")
    if schedule == "sharded": eng.comm_schedule("sharded")
    else: eng.comm_overlap(schedule == "overlap")
    cfg = vv.StepConfig(B, C, Nn, global_count=world * B * Nn, lr=1e-2)
    mine = lambda g: g[rank * B:(rank + 1) * B]
    eng.forward_backward(cfg, mine(batches[0]))
    eng.apply_update(cfg)
    ev = None
    if with_forward:
        eng.forward(vv.StepConfig(B, C, Nn, global_count=world * B * Nn), mine(batches[2]))      # the held-out batch
        st = eng.eval_stats()
        ev = (st.passes, st.last_loss, st.last_violations)
    eng.forward_backward(cfg, mine(batches[1]))
    eng.apply_update(cfg)
    loss = eng.loss()
    Wn, bn, hW, hb = eng.params_get()              # (sharded schedule: collectives -- every rank is here)
    I, Y = eng.dev(np.eye(F, dtype=np.float32)), eng.dev((F, D))
    eng.op("inner_product", I, F, Y)               # the 16-bit copy as a forward pass reads it (+ the bias)
    copy = Y.get()
    I.free(); Y.free()
    eng.comm_destroy()
    q.put((rank, Wn, bn, hW, hb, copy, np.float32(loss[0]), np.float32(loss[1]), ev))


def _run_world(world, schedule, with_forward):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    id_path = os.path.join(tempfile.gettempdir(), "vv_comm_eval_%d_%d_%s_%d" % (os.getpid(), world, schedule, with_forward))
    if os.path.exists(id_path):
        os.unlink(id_path)
    procs = [ctx.Process(target=_rank_main, args=(r, world, id_path, schedule, with_forward, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = q.get(timeout=300)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


NAMES = ("W", "b", "history of W", "history of b", "the 16-bit copy", "the last training loss", "the last training violations")


def test_forward_only_pass_between_two_updates():
    """Four runs: the synchronous schedule without the pass, and every schedule with it.  The three schedules apply bit-identical updates
    (tests/test_gpu_comm.py, tests/test_gpu_comm_adam.py), so the synchronous run without the pass is every schedule's twin."""
    plain = _run_world(2, "sync", False)
    ev = {}
    for schedule in ("sync", "overlap", "sharded"):
        held = _run_world(2, schedule, True)
        for r in range(2):
            assert held[r][7][0] == 1 and np.isfinite(held[r][7][1]) and held[r][7][1] > 0
            for k, name in enumerate(NAMES):
                assert np.array_equal(held[r][k], plain[r][k]), "%s: %s of rank %d differs from the run without the forward-only pass" % (schedule, name, r)
        ev[schedule] = [held[r][7] for r in range(2)]
        print("COMM-EVAL %s: held-out loss / violations per rank %r" % (schedule, ev[schedule]))
    assert ev["overlap"] == ev["sync"] and ev["sharded"] == ev["sync"], ev
    assert ev["sync"][0] != ev["sync"][1]                                  # local to the rank: each rank's own items
