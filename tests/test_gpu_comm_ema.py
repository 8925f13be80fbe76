"""The moving average of the parameters under data parallelism (two ranks over the shared-memory transport, started as
tests/test_gpu_comm_clip.py starts its ranks): on the sync schedule every rank applies the same update to identical parameters and runs
k_ema behind it, so after three updates the averages are bit-identical across the ranks, and on each rank they are the numpy-float32
restatement (decay * e + om * w, every operation rounded) driven by that rank's own W and b after each update.  Selecting the overlapped
or the sharded schedule while the average is active, or activating it while one of them is selected, is VV_ERR_STATE."""
import multiprocessing as mp
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, C, Nn, F, D = 32, 5, 4, 512, 256
VV_ERR_STATE = 3
DECAY = 0.9


def _rank_main(rank, world, id_path, q):
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
    eng.comm_overlap(False)
    cfg = vv.StepConfig(B, C, Nn, global_count=world * B * Nn, lr=0.01, momentum=0.9)
    refused = []

    def state_error(fn):
        try:
            fn()
        except vv.VVError as e:
            refused.append("videovec error %d" % VV_ERR_STATE in str(e) and "sync" in str(e))
        else:
            refused.append(False)

    eng.ema_set(DECAY)
    state_error(lambda: eng.comm_schedule("overlap"))
    state_error(lambda: eng.comm_schedule("sharded"))
    state_error(lambda: eng.comm_overlap(True))
    d = np.float32(DECAY)
    om = np.float32(1.0) - d
    rW, rb = W.copy(), b.copy()
    for k in range(3):
        eng.forward_backward(cfg, batches[k][rank * B:(rank + 1) * B])
        eng.apply_update(cfg)
        Wn, bn, _, _ = eng.params_get()
        rW, rb = d * rW + om * Wn, d * rb + om * bn
    eW, eb = eng.ema_get()
    updates = eng.ema_stats()["updates"]
    # the reverse order of the two calls
    eng.ema_set(-1.0)
    for sched in ("overlap", "sharded"):
        eng.comm_schedule(sched)
        state_error(lambda: eng.ema_set(DECAY))
        eng.ema_set(-1.0)                                  # (turning it off is always allowed)
    eng.comm_schedule("sync")
    eng.ema_set(DECAY)
    eng.comm_destroy()
    q.put((rank, eW, eb, rW, rb, Wn, updates, refused))


def test_two_ranks_average_identically_on_the_sync_schedule():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    id_path = os.path.join(tempfile.gettempdir(), "vv_comm_ema_%d" % os.getpid())
    if os.path.exists(id_path):
        os.unlink(id_path)
    procs = [ctx.Process(target=_rank_main, args=(r, world, id_path, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = q.get(timeout=300)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        eW, eb, rW, rb, Wn, updates, refused = res[r]
        assert updates == 3
        assert refused == [True] * 5, "rank %d: schedule 1 / 2 against the active average, in both orders: %r" % (r, refused)
        assert rW.dtype == np.float32 and np.array_equal(eW, rW) and np.array_equal(eb, rb), "rank %d: the average differs from its float32 restatement" % r
        assert np.isfinite(eW).all() and not np.array_equal(eW, Wn)
    for k, name in enumerate(("eW", "eb")):
        assert np.array_equal(res[0][k], res[1][k]), "the ranks diverged in %s" % name
    assert np.array_equal(res[0][4], res[1][4]), "the ranks diverged in W"
