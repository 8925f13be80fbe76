"""BASELINE config 2 (B 1024, C 5, Nn 50, 4096 -> 512) on the GPU: parity against the oracle on a
shard the CPU finishes in seconds, and size-independent properties at the full size."""
import numpy as np
import pytest

from videovector_amd.synth import SyntheticVideos, init_weights

pytestmark = pytest.mark.gpu

B, C, Nn, F, D = 1024, 5, 50, 4096, 512


@pytest.fixture(scope="module")
def setup(oracle):
    import videovector_amd as vv
    ds = SyntheticVideos(seed=1701, n_videos=2048)
    smp = oracle.Sampler(ds.video_id, ds.n_shots, ds.row_base, batch_size=B, context_size=C,
                         num_negative_samples=Nn, max_buffer_size=5000, negative_swap_percentage=50)
    idx, _, _ = smp.next()
    W, b = init_weights(1701, D, F)
    eng = vv.Engine(0, "f16")
    eng.table_synth(ds.seed, ds.n_rows, F)
    eng.params_set(W, b)
    return vv, ds, idx, W, b, eng


def test_full_size_properties(setup):
    vv, ds, idx, W, b, eng = setup
    cfg = vv.StepConfig(B, C, Nn)
    eng.forward_backward(cfg, idx)
    l1, v1 = eng.loss()
    blobs = eng.blobs(cfg, ip1_diff=True)
    dW, db = eng.grads()
    assert np.isfinite(l1) and 0 < l1 < 16 and 0 <= v1 <= B * Nn
    # idempotence: same inputs, same bits (fixed summation orders everywhere)
    eng.forward_backward(cfg, idx)
    dW2, db2 = eng.grads()
    assert eng.loss() == (l1, v1) and np.array_equal(dW, dW2) and np.array_equal(db, db2)
    # loss recomputed on the host from the returned scores
    d = blobs["target_score"] - blobs["negative_scores"]
    h = np.maximum(0, 2.0 - d.astype(np.float64))
    assert abs((h * h).mean() - l1) <= 1e-5 * l1 and (d < 0).sum() == v1
    # db is the column sum of the ip1_nonorm diff; dW probed with random vectors:
    # u^T dW v == sum_r (dY_r . u)(X_r . v)
    dY = blobs["ip1_diff"].astype(np.float64)
    assert np.abs(dY.sum(0) - db).max() <= 2e-3 * np.abs(db).max()
    rng = np.random.default_rng(0)
    u, v = rng.standard_normal(D), rng.standard_normal(F)
    rows = idx.T.reshape(-1)                        # reference row order ch*B + b
    uniq, inv = np.unique(rows, return_inverse=True)
    xv = (ds.table(F, uniq).astype(np.float64) @ v)[inv]
    lhs, rhs = u @ dW.astype(np.float64) @ v, ((dY @ u) * xv).sum()
    assert abs(lhs - rhs) <= 2e-3 * max(abs(lhs), abs(rhs), 1e-12)
    # linearity of the gradient in loss_weight
    eng.forward_backward(vv.StepConfig(B, C, Nn, loss_weight=0.5), idx)
    dWh, _ = eng.grads()
    assert np.abs(dWh - 0.5 * dW).max() <= 1e-3 * np.abs(dW).max()


def test_shard_of_full_batch_matches_oracle(setup, oracle):
    # data-parallel semantics: a 64-item shard with the GLOBAL loss count equals the oracle's shard
    vv, ds, idx, W, b, eng = setup
    sh = idx[128:192]
    uniq, inv = np.unique(sh.reshape(-1), return_inverse=True)
    table = ds.table(F, uniq)
    idx_local = inv.reshape(sh.shape).astype(np.int32)
    ref = oracle.forward_backward(table, idx_local, W, b, C_=C, Nn=Nn, global_count=B * Nn,
                                  want=("H", "s_true", "s_bogus", "dW", "db"))
    cfg = vv.StepConfig(64, C, Nn, global_count=B * Nn)
    eng.forward_backward(cfg, sh)
    got = eng.blobs(cfg)
    dW, db = eng.grads()
    rel = lambda a, r: np.linalg.norm(a - r) / np.linalg.norm(r)
    e_emb = (np.linalg.norm(got["ip2"] - ref["H"], axis=1) / np.linalg.norm(ref["H"], axis=1)).max()
    print("FULLSIZE shard emb=%.3e dW=%.3e db=%.3e loss=%.6f/%.6f" %
          (e_emb, rel(dW, ref["dW"]), rel(db, ref["db"]), eng.loss()[0], ref["loss"]))
    assert e_emb <= 1e-3
    assert abs(eng.loss()[0] - ref["loss"]) <= 1e-3 * ref["loss"]
    assert np.abs(got["negative_scores"] - ref["s_bogus"]).max() <= 1e-3
    # Gradients: at this initialisation every embedding shares a large common component (the
    # features are non-negative), cos(context, target) ~ 0.9+, so d(loss)/dH is a small difference
    # of nearly parallel vectors and amplifies ANY perturbation of H ~100x -- including the 2^-12
    # rounding of the f16 weight copy.  So (a) against the oracle evaluated AT the f16-rounded
    # weights the HIP gradients must agree tightly (kernel math), and (b) against the fp32-weight
    # oracle only as well as the problem's conditioning allows.
    sw = 2.0 ** (12 - np.frexp(np.abs(W).max())[1])
    Wq = (W * sw).astype(np.float16).astype(np.float32) / sw
    refq = oracle.forward_backward(table, idx_local, Wq, b, C_=C, Nn=Nn, global_count=B * Nn,
                                   want=("dW", "db"))
    print("FULLSIZE shard vs oracle@f16(W): dW=%.3e db=%.3e ; oracle(W) vs oracle(f16 W): dW=%.3e" %
          (rel(dW, refq["dW"]), rel(db, refq["db"]), rel(refq["dW"], ref["dW"])))
    assert rel(dW, refq["dW"]) <= 2e-3 and rel(db, refq["db"]) <= 2e-3
    assert rel(dW, ref["dW"]) <= 5e-2 and rel(db, ref["db"]) <= 5e-2


def test_sibling_lead_forward_kernel_is_bit_identical(setup, monkeypatch):
    """The default forward GEMM of a single-round launch lets the column-half siblings of a row tile ask for different A half-tiles
    a K-tile early (odd column tiles with their halves swapped, a ring of four LDS slots, the loop unrolled by four: a different
    issue order and LDS layout, the same MFMA order).  VV_FWD_LEAD=0 selects the plain kernel: every output bit must agree.
    (The second call of each engine is the one compared: the tile plan -- and with it the lead -- follows the PREVIOUS step's
    distinct-row count.)"""
    vv, ds, idx, W, b, eng = setup
    cfg = vv.StepConfig(B, C, Nn)
    eng.forward_backward(cfg, idx)
    eng.forward_backward(cfg, idx)
    ip2 = eng.blobs(cfg)["ip2"].copy()
    dW, db = eng.grads()
    try:
        monkeypatch.setenv("VV_FWD_LEAD", "0")
        e2 = vv.Engine(0, "f16")                      # (the switch is read when a context is created)
        e2.table_synth(ds.seed, ds.n_rows, F)
        e2.params_set(W, b)
        e2.forward_backward(cfg, idx)
        e2.forward_backward(cfg, idx)
        ip2_l = e2.blobs(cfg)["ip2"]
        dW_l, db_l = e2.grads()
        assert np.array_equal(ip2, ip2_l) and np.array_equal(dW, dW_l) and np.array_equal(db, db_l)
        del e2
    finally:
        monkeypatch.setenv("VV_FWD_LEAD", "1")
        vv.Engine(0, "f16")                           # back to the default kernel for the tests that follow


def test_full_size_dropout_on_the_deduplicated_path(setup, oracle, fp32_ip2):
    """The shipped dropout ratio 0.9 at the benchmark's size: the de-duplicated execution (the mask per instance on the shared projection) and
    the dense one (the mask in the forward GEMM's epilogue) drop the same elements and agree; a shard of the batch against the oracle with
    the same explicit mask."""
    vv, ds, idx, W, b, _ = setup
    out = {}
    for dd in (1, 0):
        eng = vv.Engine(0, "f16")
        eng.set_option("drop_dedup", dd)
        eng.table_synth(ds.seed, ds.n_rows, F); eng.params_set(W, b)
        cfg = vv.StepConfig(B, C, Nn, dropout_ratio=0.9, dropout_seed=1701)
        eng.forward_backward(cfg, idx)
        dW, db = eng.grads()
        out[dd] = (eng.dedup_stats(), eng.loss(), dW.copy(), db.copy())
        eng.forward_backward(cfg, idx)                           # idempotence under the same seed and iteration count: not expected (the
        del eng                                                  # stream advances with the iteration); only that a second step runs
    (st1, l1, dW1, db1), (st0, l0, dW0, db0) = out[1], out[0]
    assert st1[1] < st1[0] == B * (C + Nn) and st0[1] == st0[0]
    assert abs(l1[0] - l0[0]) <= 2e-6 * l0[0] and l1[1] == l0[1]
    e = float(np.linalg.norm(dW1 - dW0) / np.linalg.norm(dW0))
    print("FULLSIZE dropout 0.9: %d rows, %d distinct; loss %.6f / %.6f; dW dedup vs dense %.2e" % (st1 + (l1[0], l0[0], e)))
    assert e <= 2e-3 and np.linalg.norm(db1 - db0) <= 1e-4 * np.linalg.norm(db0)
    # a shard against the oracle, explicit mask
    sh = idx[200:232]
    Bs = sh.shape[0]
    uniq, inv = np.unique(sh.reshape(-1), return_inverse=True)
    table = ds.table(F, uniq)
    il = inv.reshape(sh.shape).astype(np.int32)
    mask = (np.random.default_rng(9).random(((C + Nn) * Bs, D)) > 0.9).astype(np.uint8)
    ref = oracle.forward_backward(table, il, W, b, C_=C, Nn=Nn, dropout_ratio=0.9, dropout_mask=mask, global_count=B * Nn,
                                  want=("H", "s_true", "s_bogus", "dW"))
    eng = vv.Engine(0, "f16")
    eng.table_synth(ds.seed, ds.n_rows, F); eng.params_set(W, b)
    cfg = vv.StepConfig(Bs, C, Nn, dropout_ratio=0.9, dropout_mask=mask, global_count=B * Nn)
    eng.forward_backward(cfg, sh)
    rows, nu = eng.dedup_stats()
    assert nu == len(uniq) < rows
    got = eng.blobs(cfg)
    nz = np.linalg.norm(ref["H"], axis=1) > 0
    e_emb = (np.linalg.norm(got["ip2"] - ref["H"], axis=1)[nz] / np.linalg.norm(ref["H"], axis=1)[nz]).max()
    assert e_emb <= 1e-3 and abs(eng.loss()[0] - ref["loss"]) <= 1e-3 * ref["loss"]
    assert np.abs(got["negative_scores"] - ref["s_bogus"]).max() <= 1e-3
    assert np.linalg.norm(eng.grads()[0] - ref["dW"]) <= 5e-2 * np.linalg.norm(ref["dW"])


def _local(ds, idx):
    """The batch's distinct table rows as a compact fp32 table for the oracle + the batch re-indexed into it."""
    uniq, inv = np.unique(idx.reshape(-1), return_inverse=True)
    return ds.table(F, uniq), inv.reshape(idx.shape).astype(np.int32), len(uniq)


@pytest.mark.parametrize("dropout,h16,slab16", [(0.0, 0, 0), (0.9, 0, 0), (0.0, 1, 0), (0.9, 1, 0), (0.0, 1, 1), (0.9, 1, 1)])
def test_the_whole_benchmark_batch_against_the_oracle(setup, oracle, dropout, h16, slab16):
    """not a shard -- ALL 56 320 rows of the BASELINE configs[1] batch, on the engine state bench.py times (de-duplication
    on; the SECOND call of an engine, whose forward GEMM is planned from the previous step's distinct-row count: 192-row tiles, ~216
    workgroups, sibling lead), against oracle.forward_backward on the same batch: every ip2 row, every score, the loss, the violations,
    dW / db against the oracle on the same rounded operands, and W / history after one vv_apply_update against oracle.sgd_update.
    dropout 0.9 (the shipped ratio) with an explicit mask: the mask per instance on the shared projection."""
    vv, ds, idx, W, b, _ = setup
    table, il, nu = _local(ds, idx)
    mask = None
    kw = {}
    if dropout > 0:
        mask = (np.random.default_rng(11).random(((C + Nn) * B, D)) > dropout).astype(np.uint8)
        kw = dict(dropout_ratio=dropout, dropout_mask=mask)
    lr = 0.01
    eng = vv.Engine(0, "f16")
    eng.set_option("h16", h16)                    # (round 6: ip2 as f16 between the forward GEMM and the segment-wise pair -- the same bounds)
    eng.set_option("slab16", slab16)              # (round 6: the split-K partial products of dW as f16 x a power of two per tile)
    eng.table_synth(ds.seed, ds.n_rows, F); eng.params_set(W, b)
    cfg = vv.StepConfig(B, C, Nn, lr=lr, **kw)
    eng.forward_backward(cfg, idx)
    eng.forward_backward(cfg, idx)                # the plan of a running job (the first call sized its tiles for 56 320 rows)
    rows, u = eng.dedup_stats()
    assert rows == B * (C + Nn) and u == nu < rows
    got = eng.blobs(cfg)
    loss, viol = eng.loss()
    dW, db = eng.grads()
    want = ("H", "s_true", "s_bogus", "dW", "db")
    ref = oracle.forward_backward(table, il, W, b, C_=C, Nn=Nn, want=want, **kw)
    # -- forward: every row, every score
    nr = np.linalg.norm(ref["H"], axis=1)
    nz = nr > 0
    e_rows = np.linalg.norm(got["ip2"] - ref["H"], axis=1)[nz] / nr[nz]
    assert nz.sum() >= 0.999 * len(nr) and np.all(got["ip2"][~nz] == 0)
    e_s = max(np.abs(got["target_score"] - ref["s_true"]).max(), np.abs(got["negative_scores"] - ref["s_bogus"]).max())
    print("FULLBATCH dropout %.1f h16 %d slab16 %d: %d rows (%d distinct): ip2 rows max %.2e mean %.2e, scores %.2e, loss %.7f / %.7f, violations %d / %d"
          % (dropout, h16, slab16, rows, u, e_rows.max(), e_rows.mean(), e_s, loss, ref["loss"], viol, ref["violations"]))
    assert e_rows.max() <= 1e-3
    assert e_s <= 1e-3
    assert abs(loss - ref["loss"]) <= 1e-3 * ref["loss"]
    assert abs(viol - ref["violations"]) <= max(2e-3 * ref["violations"], 2)
    # -- backward: the kernels' arithmetic against the oracle on the SAME rounded operands (module docstring of test_gpu_parity.py)
    sw = 2.0 ** (12 - np.frexp(np.abs(W).max())[1])
    Wq = (W * sw).astype(np.float16).astype(np.float32) / sw
    refq = oracle.forward_backward(table, il, Wq, b, C_=C, Nn=Nn, want=("dW", "db"), **kw)
    rel = lambda a, r: float(np.linalg.norm(a - r) / np.linalg.norm(r))
    print("FULLBATCH dropout %.1f h16 %d slab16 %d: dW %.2e db %.2e vs the oracle at f16(W); %.2e vs the fp32-operand oracle"
          % (dropout, h16, slab16, rel(dW, refq["dW"]), rel(db, refq["db"]), rel(dW, ref["dW"])))
    assert rel(dW, refq["dW"]) <= 2e-3 and rel(db, refq["db"]) <= 2e-3
    assert rel(dW, ref["dW"]) <= 5e-2
    # -- the update (solver.cpp:485-576): the solver's rule on the oracle's own gradient, and -- the rule alone -- on the engine's
    eng.apply_update(cfg)
    Wn, bn, hW, hb = eng.params_get()
    for g_w, g_b, tol in ((refq["dW"], refq["db"], 2e-3), (dW, db, 2e-6)):
        Wo, bo, hWo, hbo = W.copy(), b.copy(), np.zeros_like(W), np.zeros_like(b)
        oracle.sgd_update(Wo, g_w.copy(), hWo, lr, 1.0, 0.9, 5e-4, 1.0)
        oracle.sgd_update(bo, g_b.copy(), hbo, lr, 2.0, 0.9, 5e-4, 0.0)
        assert rel(hW, hWo) <= tol and rel(hb, hbo) <= tol, (tol, rel(hW, hWo), rel(hb, hbo))
        assert rel(Wn - W, Wo - W) <= tol and rel(bn - b, bo - b) <= tol
    assert np.linalg.norm(Wn - W) > 0

