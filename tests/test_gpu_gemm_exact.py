"""The two GEMMs of the step, element for element against float64, at every tile height and split plan.

The other GPU tests bound a norm over a whole batch (rel_rows / rel_fro): one wrong element, one K-tile dropped in one tile or one
row of a ragged last tile written to the wrong place disappears in such a bound.  Here the operands are chosen so that EVERY value on
the path is exactly representable, the expected output is the float64 product itself and the comparison is np.array_equal:

  features / X   integers 0 .. 3, about half of them zero          (exact in f16 and bf16; the table keeps scale 1)
  W, b           integers -8 .. 8 times 2^-6                       (exact after the f16 range scaling and in bf16's 8-bit mantissa)
  dY             integers -2 .. 2                                  (the power-of-two gradient scale keeps them exact)
  dropout 0.5    the factor 2, ip_regularization 0.5 the factor 1.25

so every fp32 accumulation is an integer count of 2^-6 units far below 2^24, whatever its order.  The tests assert that themselves
on the CPU (operands_exact / checked_ref): a failure there means a wrong input, not a wrong kernel.  No element is exempt.

Every case also asserts the FORM it was written for -- the forward GEMM's tile height ("last_fwd_tile_rows") or the weight-gradient
GEMM's split count ("last_wgrad_splits"), read back from the context after the launch.  This file holds no copy of the launchers'
rules: if a shape lands in another band after a change of the cost table, the assertion fails and the shape has to move.

A mismatch reports the first differing (row, column), the tile it lies in and both values.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import round_operand, round_table, vv  # noqa: F401  (vv: fixture)

pytestmark = pytest.mark.gpu

PRECS = ["f16", "bf16"]
SENTINEL = np.float32(-12345.0)          # no product of these operands: |Y| <= (3 * 8 * F + 8) / 64
_REFS = {}                               # float64 references, computed once per shape and never modified


# ------------------------------------------------------------------------------- operands
def features(seed, n, F):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 4, size=(n, F)) * (rng.random((n, F)) < 0.5)).astype(np.float32)


def weights(D, F):
    rng = np.random.default_rng(7 * D + F)
    W = (rng.integers(-8, 9, size=(D, F)) / 64.0).astype(np.float32)
    b = (rng.integers(-8, 9, size=D) / 64.0).astype(np.float32)
    return W, b


def gradients(seed, R, D):
    return np.random.default_rng(seed).integers(-2, 3, size=(R, D)).astype(np.float32)


def operands_exact(prec, X=None, W=None, dY=None):
    """The values the MFMA reads are the values given (a failure here is a wrong input, not a wrong kernel)."""
    if X is not None:
        assert np.array_equal(round_table(X, prec), X)
    if W is not None:
        assert np.array_equal(round_operand(W, prec), W)
    if dY is not None:
        assert np.array_equal(round_operand(dY, prec), dY)


def checked_ref(key, make):
    """The float64 reference of a shape, once: an integer count of 2^-6 units below 2^24 -- exact in fp32 in any summation order."""
    if key not in _REFS:
        ref = make()
        assert ref.dtype == np.float64
        units = ref * 64.0
        assert np.array_equal(units, np.rint(units)), "the reference is not a multiple of 2^-6: the inputs are wrong"
        assert np.abs(units).max() < 2 ** 24, "the reference leaves fp32's exact integers: the inputs are wrong"
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def assert_exact(got, ref, what, tile_rows, tile_cols=256):
    if np.array_equal(got, ref):
        return
    bad = np.argwhere(~(got == ref))
    r, c = (int(v) for v in bad[0])
    tiles = {(int(i) // tile_rows, int(j) // tile_cols) for i, j in bad[:100000]}
    msg = ("%s: %d of %d elements differ, in %s%d tile(s) of %d x %d; first at (row %d, column %d) = tile (%d, %d), row %d and column %d "
           "inside it: got %r, expected %r" % (what, len(bad), ref.size, "at least " if len(bad) > 100000 else "", len(tiles), tile_rows,
                                               tile_cols, r, c, r // tile_rows, c // tile_cols, r % tile_rows, c % tile_cols,
                                               float(got[r, c]), float(ref[r, c])))
    print(msg)
    pytest.fail(msg)


# ------------------------------------------------------------------------------- engines
@pytest.fixture(scope="module")
def engines(vv):  # noqa: F811
    """engines(prec, D, F, n_rows) -> (engine, table, W, b): one engine per key for the whole module, closed at its end."""
    made = {}

    def get(prec, D, F, n_rows=500):
        key = (prec, D, F, n_rows)
        if key not in made:
            T = features(1000 + F, n_rows, F)
            W, b = weights(D, F)
            operands_exact(prec, X=T, W=W)
            eng = vv.Engine(0, prec)
            assert eng.get_option("last_fwd_tile_rows") == 0 and eng.get_option("last_wgrad_splits") == 0     # before any launch
            eng.table_set(T)
            eng.params_set(W, b)
            assert np.array_equal(eng.table_get(n=n_rows), T)
            made[key] = (eng, T, W, b)
        return made[key]

    yield get
    for eng, _, _, _ in made.values():
        eng.close()


def fwd_tile(eng):
    return int(eng.get_option("last_fwd_tile_rows"))


def test_launch_records_are_read_only(vv):  # noqa: F811
    eng = vv.Engine(0, "f16")
    for name in ("last_fwd_tile_rows", "last_wgrad_splits", "last_update_form", "last_grad_shift", "last_grad_shift_round1", "last_grad_repeat"):
        assert eng.get_option(name) == 0
        with pytest.raises(vv.VVError, match="videovec error 1: .*read-only"):          # VV_ERR_ARG
            eng.set_option(name, 128)
        assert eng.get_option(name) == 0
    eng.close()


# ------------------------------------------------------------------------------- forward: vv_op_inner_product
# (D, F, R, tile rows the case is written for, fwd_lead).  D = 4096 has 16 column tiles.  R fills the tiles exactly (2048 = 16 x 128,
# 3072 = 16 x 192, 4096 = 16 x 256) or leaves a ragged last tile: one row (1025, 3073), just over half (2049 = 10 x 192 + 129),
# a few rows (2500 = 13 x 192 + 4), most of it (3500 = 13 x 256 + 172).  D = 4090: D % 4 = 2, the scalar-store epilogue under 16 column
# tiles; D = 250: the same with ONE column tile (no sibling lead there).  fwd_lead 0 / 1: both exact, hence bit-identical; the 256-row
# form has no lead and runs under the default.  F = 320 pads to eight K-tiles of which the last three are all zero: the F = 512 cases make
# every K-tile count, the last ones -- where the stream of half-tiles runs out -- included.
IP_CASES = [(4096, 512, 1025, 128, 1), (4096, 512, 2049, 192, 1), (4096, 512, 2049, 192, 0), (4096, 512, 3073, 256, 1),
            (4096, 320, 2048, 128, 1), (4096, 320, 1025, 128, 1), (4096, 320, 1025, 128, 0),
            (4096, 320, 3072, 192, 1), (4096, 320, 2049, 192, 1), (4096, 320, 2049, 192, 0),
            (4096, 320, 4096, 256, 1), (4096, 320, 3073, 256, 1),
            (4090, 320, 2500, 192, 1), (4090, 320, 3500, 256, 1), (250, 100, 130, 128, 1)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("D,F,R,tile,lead", IP_CASES)
def test_inner_product_exact_at_every_tile_height(engines, prec, D, F, R, tile, lead):
    eng, _, W, b = engines(prec, D, F)
    X = features(R, R, F)
    operands_exact(prec, X=X)
    ref = checked_ref(("ip", D, F, R), lambda: X.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64))
    assert (ref < 0).any() and (ref > 0).any()                 # no ReLU here: negative outputs are compared too
    Xd = eng.dev(X)
    Yd = eng.dev(np.full((R + 256, D), SENTINEL, np.float32))  # 256 rows past R: a whole tallest tile of slack
    assert eng.get_option("fwd_lead") == 1                     # the default
    eng.set_option("fwd_lead", lead)
    try:
        eng.op("inner_product", Xd, R, Yd)
        got_tile = fwd_tile(eng)
        y = Yd.get()
    finally:
        eng.set_option("fwd_lead", 1)
        Xd.free(); Yd.free()
    assert got_tile == tile, "R = %d at D = %d ran %d-row tiles, the case is written for %d: move R" % (R, D, got_tile, tile)
    assert_exact(y[:R], ref, "Y = X W^T + b (%s, D %d, F %d, R %d, lead %d)" % (prec, D, F, R, lead), tile)
    assert np.array_equal(y[R:], np.full((256, D), SENTINEL, np.float32)), "rows past R were written"


# ------------------------------------------------------------------------------- forward: vv_embed (gather + ReLU)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n,tile", [(2600, 192), (3300, 256)])
def test_embed_gathered_rows_exact_in_tall_tiles(engines, prec, n, tile):
    D, F = 4096, 320
    eng, T, W, b = engines(prec, D, F)
    rows = np.random.default_rng(n).integers(0, 40, size=n).astype(np.int32) * 13 % len(T)      # heavy repetition: 40 distinct rows
    rows[[0, n // 2, n - 1]] = len(T) - 1                                                        # the table's last row: first, middle, last
    rows[[1, n // 3, n - 2]] = 0                                                                 # ... and its first
    ref = checked_ref(("embed", n), lambda: np.maximum(T[rows].astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64), 0.0))
    e = eng.embed(rows, relu=True, l2norm=False)
    assert fwd_tile(eng) == tile, "n = %d ran %d-row tiles, the case is written for %d: move n" % (n, fwd_tile(eng), tile)
    assert_exact(e, ref, "vv_embed (%s, n %d)" % (prec, n), tile)


# ------------------------------------------------------------------------------- forward: the dense step, dropout in the epilogue
def step_case(B, C, Nn, T, W, b):
    """idx with empty slots (-1), some of them in the last row tile, and the float64 ip2 before dropout in the blob's row order
    (row = ch * B + b, as tests/test_gpu_parity.py reads it)."""
    CN = C + Nn
    idx = np.random.default_rng(B).integers(0, len(T), size=(B, CN)).astype(np.int32)
    for bb, ch in ((0, 2), (B // 2, 4), (B - 1, 0), (B - 1, CN - 1), (B - 2, 1)):      # (the GEMM's row is b * CN + ch: b = B - 1 is its last tile)
        idx[bb, ch] = -1
    Tz = np.concatenate([T, np.zeros((1, T.shape[1]), np.float32)])
    flat = np.where(idx < 0, len(T), idx).T.reshape(-1)
    h0 = checked_ref(("step", B, W.shape[0]), lambda: np.maximum(Tz[flat].astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64), 0.0))
    return idx, h0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", ["plain", "mask", "hash"])
@pytest.mark.parametrize("B,tile", [(320, 192), (500, 256)])
def test_dense_step_ip2_exact_with_empty_slots_and_dropout(vv, engines, prec, mode, B, tile):  # noqa: F811
    D, F, C, Nn = 4096, 320, 3, 5
    eng, T, W, b = engines(prec, D, F)
    idx, h0 = step_case(B, C, Nn, T, W, b)
    kw = {}
    if mode == "mask":
        mask = (np.random.default_rng(B + 1).random(((C + Nn) * B, D)) > 0.5).astype(np.uint8)
        kw = dict(dropout_ratio=0.5, dropout_mask=mask)
    elif mode == "hash":
        kw = dict(dropout_ratio=0.5, dropout_seed=4242)
    cfg = vv.StepConfig(B, C, Nn, **kw)
    eng.set_dedup(False)
    try:
        eng.forward_backward(cfg, idx)
        got_tile = fwd_tile(eng)
        assert eng.dedup_stats() == (B * (C + Nn), B * (C + Nn))
        ip2 = eng.blobs(cfg, scores=False)["ip2"]
    finally:
        eng.set_dedup(True)
    assert got_tile == tile, "B = %d ran %d-row tiles, the case is written for %d: move B" % (B, got_tile, tile)
    what = "ip2 of the dense step (%s, B %d, %s)" % (prec, B, mode)
    if mode == "plain":
        assert_exact(ip2, h0, what, tile)
    elif mode == "mask":
        ref = checked_ref(("step-mask", B), lambda: mask.astype(np.float64) * 2.0 * h0)
        assert_exact(ip2, ref, what, tile)
    else:
        h2 = checked_ref(("step-x2", B), lambda: 2.0 * h0)
        live = h2 != 0
        kept = ip2 != 0
        assert_exact(np.where(kept, ip2, h2), h2, what + ": a kept element is twice the reference", tile)      # every element: 0 or exactly 2 x
        assert not (kept & ~live).any(), "an element whose reference is zero came out non-zero"
        n, k = int(live.sum()), int((kept & live).sum())
        print("counter-hash dropout: %d of %d live elements kept (%.5f)" % (k, n, k / n))
        assert abs(k - 0.5 * n) <= 4.0 * np.sqrt(0.25 * n)


# ------------------------------------------------------------------------------- forward: de-duplicated steps (n_dev, R_hint)
@pytest.mark.parametrize("prec", PRECS)
def test_dedup_steps_ip2_exact_under_a_right_and_a_wrong_hint(vv, engines, prec):  # noqa: F811
    """Step 1 has no hint: the tile is chosen for all R rows (256-row band) although few are distinct.  Step 2 is planned from step 1's
    distinct count: 128-row tiles.  Step 3's indices are all distinct, planned from step 2's count: the hint is ten times too small, the
    grid still covers every row.  D = 4096 keeps fp32 rows (h16 applies at D = 512 / 1024 only).  No update: W stays exact.

    The launcher reads the host-mapped distinct count when it gets there: a step whose grouping has ALREADY finished on the second stream is
    planned from its own count, not the previous step's -- on an idle GPU that is a race the host usually loses.  The test decides it: the
    indices are device memory produced on the context's stream (idx_on_device = 1: the grouping waits for that stream) and a few
    milliseconds of copy kernels are queued there first, so every launch is planned long before its own grouping can start.  For that the
    steps must not synchronise on their way: a small de-duplicated step first (it allocates the grouping's tables), then a dense step
    of the batch shape (it allocates the batch and leaves the hint at 0)."""
    D, F, B, C, Nn = 4096, 320, 400, 3, 5
    CN, R = C + Nn, B * (C + Nn)
    eng, T, W, b = engines(prec, D, F, n_rows=3300)
    rng = np.random.default_rng(6)
    batches = [(rng.integers(0, 300, size=(B, CN)), 256), (rng.integers(300, 600, size=(B, CN)), 128),
               (rng.permutation(len(T))[:R].reshape(B, CN), 128)]

    def ref_of(key, idx):
        flat = idx.T.reshape(-1)
        return checked_ref(key, lambda: np.maximum(T[flat].astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64), 0.0))

    cfg = vv.StepConfig(B, C, Nn)
    small = vv.StepConfig(8, C, Nn)
    eng.forward_backward(small, np.zeros((8, CN), np.int32))
    assert eng.dedup_stats() == (8 * CN, 1)
    idx0 = batches[2][0].astype(np.int32)
    eng.set_dedup(False)
    try:
        eng.forward_backward(cfg, idx0)                        # the dense execution of step 3's batch, while we are here
        assert fwd_tile(eng) == 256 and eng.dedup_stats() == (R, R)
        assert_exact(eng.blobs(cfg, scores=False)["ip2"], ref_of(("dedup", 3), idx0), "ip2 of the dense step (%s)" % prec, 256)
    finally:
        eng.set_dedup(True)
    ballast = eng.dev((1 << 28,))                              # 1 GiB: one y = x + 0 y over it keeps the stream busy for most of a millisecond
    idx_dev = eng.dev(idx0)
    try:
        for step, (idx, tile) in enumerate(batches, 1):
            idx = idx.astype(np.int32)
            ref = ref_of(("dedup", step), idx)
            idx_dev.set(idx)
            eng.synchronize()
            for _ in range(8):
                eng.op("axpby", 1 << 28, 1.0, ballast, 0.0, ballast)
            eng.forward_backward(cfg, idx_dev_ptr=idx_dev.ptr.value)
            got_tile = fwd_tile(eng)
            rows, uniq = eng.dedup_stats()
            ip2 = eng.blobs(cfg, scores=False)["ip2"]
            assert (rows, uniq) == (R, len(np.unique(idx))), "the de-duplicated path did not run"
            assert got_tile == tile, "step %d (%d distinct rows of %d) ran %d-row tiles, written for %d" % (step, uniq, R, got_tile, tile)
            assert_exact(ip2, ref, "ip2 of de-duplicated step %d (%s, %d distinct rows)" % (step, prec, uniq), tile)
    finally:
        ballast.free(); idx_dev.free()


# ------------------------------------------------------------------------------- weight gradient: vv_op_inner_product_bwd
# (D, F, R of the first call, R of the call under test, S, K-tiles per split, splits that work, K-tiles of the last working split).
# S is what "last_wgrad_splits" must report; the other three follow from it by the kernel's own arithmetic (Rp / 64 K-tiles dealt out
# ceil(total / S) at a time) and say what the case is FOR:
#   D = F = 256           one K-tile per split (R = 1: three of the four K-tiles are padding)
#   512 x 768, R 3000     two per split, and 19 splits that get nothing yet must leave zero slabs
#   768 x 768, R 5000     three per split (odd), the last working split shorter (2), two empty splits
#   4096 x 4096, R 700    one split holds the whole K loop
#   30 x 100              D % 4 != 0 and a padded F
# The first call runs MORE rows on the same engine, so the 16-bit scratch copies of X and dY hold stale rows past R in the second.
WGRAD_CASES = [(256, 256, 300, 1, 4, 1, 4, 1), (256, 256, 600, 257, 8, 1, 8, 1), (256, 256, 600, 300, 8, 1, 8, 1),
               (512, 768, 3500, 3000, 43, 2, 24, 2), (768, 768, 5500, 5000, 29, 3, 27, 2),
               (4096, 4096, 900, 700, 1, 12, 1, 12), (30, 100, 400, 200, 4, 1, 4, 1)]


def wgrad_ref(D, F, R):
    X, dY = features(R + F, R, F), gradients(1000003 + R + D, R, D)
    dW = checked_ref(("dW", D, F, R), lambda: dY.astype(np.float64).T @ X.astype(np.float64))
    dW125 = checked_ref(("dW125", D, F, R), lambda: 1.25 * dW)
    db = checked_ref(("db", D, F, R), lambda: dY.astype(np.float64).sum(0))
    return X, dY, dW, dW125, db


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tr", [1, 0])
@pytest.mark.parametrize("D,F,R_first,R,S,kps,working,last", WGRAD_CASES)
def test_weight_gradient_exact_split_by_split(engines, prec, tr, D, F, R_first, R, S, kps, working, last):
    eng, _, _, _ = engines(prec, D, F)
    eng.set_option("wgrad_tr", tr)
    try:
        for rows, under_test in ((R_first, False), (R, True)):
            X, dY, dW_ref, dW125_ref, db_ref = wgrad_ref(D, F, rows)
            operands_exact(prec, X=X, dY=dY)
            Xd, Yd, dYd = eng.dev(X), eng.dev((rows, D)), eng.dev(dY)
            try:
                eng.op("inner_product", Xd, rows, Yd)
                eng.op("inner_product_bwd", dYd, rows, 0.0)
                got_S = int(eng.get_option("last_wgrad_splits"))
                dW, db = eng.grads()
                what = "(%s, wgrad_tr %d, D %d, F %d, R %d, S %d)" % (prec, tr, D, F, rows, got_S)
                if under_test:
                    total = -(-rows // 256) * 256 // 64                  # Rp / 64 K-tiles
                    got_kps = -(-total // got_S)
                    got_working = -(-total // got_kps)
                    assert (got_S, got_kps, got_working, total - (got_working - 1) * got_kps) == (S, kps, working, last), \
                        "R = %d at %d x %d ran another split plan than the case is written for: move R" % (rows, D, F)
                assert_exact(dW, dW_ref, "dW = dY^T X " + what, 256)
                assert np.array_equal(db, db_ref), "db " + what
                if under_test:
                    eng.op("inner_product_bwd", dYd, rows, 0.5)         # ip_regularization 0.5: exactly 1.25 x dW, db unchanged
                    assert int(eng.get_option("last_wgrad_splits")) == S
                    dW, db = eng.grads()
                    assert_exact(dW, dW125_ref, "1.25 dW " + what, 256)
                    assert np.array_equal(db, db_ref), "db under ip_regularization " + what
            finally:
                Xd.free(); Yd.free(); dYd.free()
    finally:
        eng.set_option("wgrad_tr", 1)
