"""Adam under the three data-parallel schedules (vv_comm_overlap 0 / 1, vv_comm_schedule sharded): every schedule updates through k_sgd's
two-history instantiation -- the whole matrix, F-chunk by F-chunk, or this rank's rows, whose shard then owns its rows of v -- so at world 2
on the shared-memory transport the three must agree bit for bit after two updates: W, b, m, v (gathered by the collective vv_params_get /
vv_history2_get) and the 16-bit copy the next forward pass reads.  Follows tests/test_gpu_comm.py's schedule-equality tests (two
processes sharing the one GPU, the same time limits)."""
import multiprocessing as mp
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, UPDATES = 32, 5, 4, 512, 256, 2


def _rank_main(rank, world, id_path, schedule, q):
    import videovector_amd as vv
    from videovector_amd.synth import SyntheticVideos, init_weights
    ds = SyntheticVideos(seed=21, n_videos=300)
    W, b = init_weights(21, D, F, std=0.02)
    s = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=world * B, context_size=C, num_negative_samples=Nn,
                   max_buffer_size=1000, negative_swap_percentage=50)
    batches = [s.next() for _ in range(UPDATES)]
    s.close()
    eng = vv.Engine(0, "f16")
    eng.table_synth(ds.seed, ds.n_rows, F)
    eng.params_set(W, b)
    eng.comm_init(world, rank, id_path, "shm")
    if schedule == "sharded": eng.comm_schedule("sharded")
    else: eng.comm_overlap(schedule == "overlap")
    cfg = vv.StepConfig(B, C, Nn, global_count=world * B * Nn, lr=1e-3, solver_type="ADAM", momentum=0.9, momentum2=0.999)
    for g in batches:
        eng.forward_backward(cfg, g[rank * B:(rank + 1) * B])
        eng.apply_update(cfg)
    form, t = int(eng.get_option("last_update_form")), eng.solver_iter
    Wn, bn, mW, mb = eng.params_get()              # (sharded schedule: collectives -- every rank is here)
    vW, vb = eng.history2_get()
    I, Y = eng.dev(np.eye(F, dtype=np.float32)), eng.dev((F, D))
    eng.op("inner_product", I, F, Y)               # the 16-bit copy as a forward pass reads it (+ the bias)
    copy = Y.get()
    I.free(); Y.free()
    eng.comm_destroy()
    q.put((rank, Wn, bn, mW, mb, vW, vb, copy, form, t))


def _run_world(world, schedule):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    id_path = os.path.join(tempfile.gettempdir(), "vv_comm_adam_%d_%d_%s" % (os.getpid(), world, schedule))
    if os.path.exists(id_path):
        os.unlink(id_path)
    procs = [ctx.Process(target=_rank_main, args=(r, world, id_path, schedule, q)) for r in range(world)]
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


def test_adam_three_schedules_agree_bit_for_bit():
    names = ("W", "b", "m of W", "m of b", "v of W", "v of b", "the 16-bit copy")
    sync = _run_world(2, "sync")
    assert sync[0][7] == 1 and sync[0][8] == UPDATES
    assert np.isfinite(sync[0][0]).all() and sync[0][4].max() > 0 and (sync[0][4] >= 0).all(), "v was not updated"
    assert (sync[0][4] > 0).mean() > 0.99
    for schedule in ("overlap", "sharded"):
        other = _run_world(2, schedule)
        for r in range(2):
            assert other[r][7] == 1 and other[r][8] == UPDATES
            for k, name in enumerate(names):
                assert np.array_equal(other[r][k], sync[0][k]), "%s: %s of rank %d differs from the synchronous schedule's" % (schedule, name, r)
    for k, name in enumerate(names):
        assert np.array_equal(sync[1][k], sync[0][k]), "sync: ranks diverged in %s" % name
