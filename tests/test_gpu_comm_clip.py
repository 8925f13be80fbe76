"""Gradient clipping under data parallelism (two ranks over the shared-memory transport, started as tests/test_gpu_comm_adam.py starts
its ranks): on the sync schedule the all-reduce finishes, then every rank runs the same two kernels on identical buffers -- both ranks
must end with bit-identical W and read the identical norm.  tests/test_gpu_comm_adam.py holds no comparison of a two-rank run against a
single process at the global batch, so there is no tolerance to take over: this file checks the two-rank equality only, plus that the
norm is the norm of the summed gradient both ranks read back (1 ulp, as tests/test_gpu_clip_gradients.py derives).  Selecting the
overlapped or the sharded schedule while clipping is active, or activating clipping while one of them is selected, is VV_ERR_STATE."""
import multiprocessing as mp
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, C, Nn, F, D = 32, 5, 4, 512, 256
VV_ERR_STATE = 3


def _rank_main(rank, world, id_path, q):
    import videovector_amd as vv
    from videovector_amd.synth import SyntheticVideos, init_weights
    ds = SyntheticVideos(seed=21, n_videos=300)
    W, b = init_weights(21, D, F, std=0.02)
    s = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=world * B, context_size=C, num_negative_samples=Nn,
                   max_buffer_size=1000, negative_swap_percentage=50)
    batches = [s.next() for _ in range(2)]
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

    # the first step unclipped: the norm of the summed gradient, read back by both ranks
    eng.forward_backward(cfg, batches[0][rank * B:(rank + 1) * B])
    eng.apply_update(cfg)
    dW, db = eng.grads()
    n0 = float(np.sqrt((dW.astype(np.float64) ** 2).sum() + (db.astype(np.float64) ** 2).sum()))
    # the second step with a threshold far below any norm: the scale comes from the norm the kernels compute on each rank
    eng.clip_gradients_set(n0 / 64.0)
    state_error(lambda: eng.comm_schedule("overlap"))
    state_error(lambda: eng.comm_schedule("sharded"))
    state_error(lambda: eng.comm_overlap(True))
    eng.forward_backward(cfg, batches[1][rank * B:(rank + 1) * B])
    eng.apply_update(cfg)
    st = eng.clip_stats()
    gW, gb = eng.grads()
    form = int(eng.get_option("last_update_form"))
    Wn, bn, hW, hb = eng.params_get()
    # the reverse order of the two calls
    eng.clip_gradients_set(-1.0)
    for sched in ("overlap", "sharded"):
        eng.comm_schedule(sched)
        state_error(lambda: eng.clip_gradients_set(1.0))
        eng.clip_gradients_set(-1.0)                       # (disabling is always allowed)
    eng.comm_schedule("sync")
    eng.clip_gradients_set(1.0)
    eng.comm_destroy()
    q.put((rank, Wn, bn, hW, hb, gW, gb, st, form, refused))


def test_two_ranks_clip_identically_on_the_sync_schedule():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    id_path = os.path.join(tempfile.gettempdir(), "vv_comm_clip_%d" % os.getpid())
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
        st, form, refused = res[r][6], res[r][7], res[r][8]
        assert form == 1
        assert st["clipped"] == 1 and st["updates"] == 1 and st["clipped_updates"] == 1 and 0 < st["scale"] < 1
        assert refused == [True] * 5, "rank %d: schedule 1 / 2 against active clipping, in both orders: %r" % (r, refused)
    for k, name in enumerate(("W", "b", "hW", "hb", "the clipped dW", "the clipped db")):
        assert np.array_equal(res[0][k], res[1][k]), "the ranks diverged in %s" % name
    assert res[0][6]["norm"] == res[1][6]["norm"] and res[0][6]["scale"] == res[1][6]["scale"]
    # the gradient read back is g * scale: its norm is clip within the rounding of the n products (relative 2^-24 each)
    gW, gb, st = res[0][4], res[0][5], res[0][6]
    back = np.sqrt((gW.astype(np.float64) ** 2).sum() + (gb.astype(np.float64) ** 2).sum())
    assert abs(back / (float(st["norm"]) * float(st["scale"])) - 1.0) < 2.0 ** -22
    assert np.isfinite(res[0][0]).all()
