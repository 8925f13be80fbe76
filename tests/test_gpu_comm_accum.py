"""Gradient accumulation under data parallelism (two ranks over the shared-memory transport, started as tests/test_gpu_comm_clip.py
starts its ranks), sync schedule, m = 3: every rank banks its own three gradients, vv_apply_update writes the bank into the buffer, ONE
all-reduce sums the two banks, every element is multiplied by 1.0f / 3 and the plain k_sgd runs.  Both ranks must end bit-identical in
W, b and the histories -- and bit-identical to a single-process restatement of those steps, made by rank 0 behind the exchange with an
engine that has no communicator: each rank's bank as acc = g1; acc = acc + gk in float32 from that rank's gradients (dense execution is
deterministic: the engine reproduces them bit for bit, which the test asserts for rank 0's own), the sum over the ranks bank_0 + bank_1
(two ranks: one float32 add per element, the same in either order of the transport), times float32(1) / float32(3); that buffer, bound
as the engine's gradient, through vv_apply_update.  Banking while schedule 1 or 2 is selected, and selecting one while the bank is
non-empty, is VV_ERR_STATE.  Two processes."""
import multiprocessing as mp
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, C, Nn, F, D, M = 32, 5, 4, 512, 256, 3
VV_ERR_STATE = 3


def _rank_main(rank, world, id_path, q):
    try:
        _rank_body(rank, world, id_path, q)
    except BaseException as e:                             # (the parent fails at once instead of waiting for its queue)
        q.put((rank, "error", repr(e)))
        raise


def _rank_body(rank, world, id_path, q):
    import videovector_amd as vv
    from videovector_amd.synth import SyntheticVideos, init_weights
    ds = SyntheticVideos(seed=21, n_videos=300)
    W, b = init_weights(21, D, F, std=0.02)
    s = vv.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=world * B, context_size=C, num_negative_samples=Nn,
                   max_buffer_size=1000, negative_swap_percentage=50)
    batches = [s.next() for _ in range(M)]
    s.close()
    cfg = vv.StepConfig(B, C, Nn, global_count=world * B * Nn, lr=0.01, momentum=0.9)

    def engine():
        e = vv.Engine(0, "f16")
        e.set_dedup(False)
        e.set_option("fuse_update", 0)
        e.table_synth(ds.seed, ds.n_rows, F)
        e.params_set(W, b)
        return e

    eng = engine()
    eng.comm_init(world, rank, id_path, "shm")
    eng.comm_overlap(False)
    refused = []

    def state_error(fn):
        try:
            fn()
        except vv.VVError as e:
            refused.append("videovec error %d" % VV_ERR_STATE in str(e) and "sync" in str(e))
        else:
            refused.append(False)

    mine = lambda k, r=rank: batches[k][r * B:(r + 1) * B]
    own = []
    for k in range(M):
        eng.forward_backward(cfg, mine(k))
        own.append(eng.grads())
        eng.grads_bank()
        if k == 0:                                         # selecting one while the bank is non-empty
            state_error(lambda: eng.comm_schedule("overlap"))
            state_error(lambda: eng.comm_schedule("sharded"))
            state_error(lambda: eng.comm_overlap(True))
    eng.apply_update(cfg)
    gW, gb = eng.grads()
    form = int(eng.get_option("last_update_form"))
    st = eng.accum_stats()
    Wn, bn, hW, hb = eng.params_get()
    for sched in ("overlap", "sharded"):                   # banking while schedule 1 or 2 is selected
        eng.comm_schedule(sched)
        eng.forward_backward(cfg, mine(0))
        state_error(eng.grads_bank)
    eng.comm_schedule("sync")
    eng.comm_destroy()
    eng.close()
    restated = None
    if rank == 0:                                          # the single-process restatement
        banks = []
        for r in range(world):                             # (a fresh engine per rank: the same history of steps as that rank's own engine)
            ref = engine()
            acc = None
            for k in range(M):
                ref.forward_backward(cfg, mine(k, r))
                g = ref.grads()
                if r == 0:
                    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(g, own[k])), "the engines' gradients differ: the premise of the restatement"
                acc = g if acc is None else (acc[0] + g[0], acc[1] + g[1])
            banks.append(acc)
            ref.close()
        ref = engine()
        inv = np.float32(1) / np.float32(M)
        nW, nb = (banks[0][0] + banks[1][0]) * inv, (banks[0][1] + banks[1][1]) * inv
        assert nW.dtype == np.float32 and nb.dtype == np.float32
        buf = ref.dev((D * F + D,))
        ref.grads_bind(buf.ptr.value)
        ref.forward_backward(cfg, mine(0))                 # (a gradient exists; the buffer is then overwritten with the restated one)
        ref.loss()                                         # (synchronises: the pass has written the buffer)
        buf.set(np.concatenate([nW.ravel(), nb]))
        ref.apply_update(cfg)
        restated = (nW, nb) + tuple(ref.params_get()) + (int(ref.get_option("last_update_form")),)
        ref.grads_bind(0)
        buf.free()
        ref.close()
    q.put((rank, Wn, bn, hW, hb, gW, gb, st, form, refused, restated))


def test_two_ranks_accumulate_identically_on_the_sync_schedule():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    id_path = os.path.join(tempfile.gettempdir(), "vv_comm_accum_%d" % os.getpid())
    if os.path.exists(id_path):
        os.unlink(id_path)
    procs = [ctx.Process(target=_rank_main, args=(r, world, id_path, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = q.get(timeout=300)
        assert not isinstance(r[1], str), "rank %d: %s" % (r[0], r[-1])
        res[r[0]] = r[1:]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        st, form, refused = res[r][6], res[r][7], res[r][8]
        assert form == 1
        assert (st["banked"], st["last_count"], st["updates"]) == (0, M, 1)
        assert sorted(refused) == [True] * 5, "rank %d: schedule 1 / 2 against the bank, in both orders: %r" % (r, refused)
    names = ("W", "b", "hW", "hb", "the normalised dW", "the normalised db")
    for k, name in enumerate(names):
        assert np.array_equal(res[0][k].view(np.uint32), res[1][k].view(np.uint32)), "the ranks diverged in %s" % name
    nW, nb, Wr, br, hWr, hbr, form_r = res[0][9]
    assert form_r == 1
    for name, a, e in zip(names, res[0][:6], (Wr, br, hWr, hbr, nW, nb)):
        assert np.array_equal(a.view(np.uint32), e.view(np.uint32)), "%s differs from the single-process restatement" % name
    from videovector_amd.synth import init_weights
    W0, _ = init_weights(21, D, F, std=0.02)
    assert np.isfinite(res[0][0]).all() and (res[0][0] != W0).mean() > 0.99
