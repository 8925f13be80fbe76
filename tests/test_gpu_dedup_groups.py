"""The de-duplication grouping and the segment sums, array by array and bit for bit (videovector_amd/csrc/kernels_dedup.hip).

Every benchmarked step decides through k_dd_claim, k_dd_leaders, k_dd_map, k_dd_segstart (and k_dd_pos) which table row the forward GEMM
projects for each slot and which gradient rows k_segsum adds into which row of the weight-gradient GEMM's operand.  The other tests see
that stage only through dedup_stats()[1] and norms of dW.  Here Engine.dedup_groups() (vv_dedup_groups_get) returns the arrays themselves
and they are held to a numpy restatement (tests/pyref.py: dedup_groups_expected / dedup_groups_check; the checker itself is tested on the
CPU in tests/test_dedup_groups_host.py).  It is integer bookkeeping and exact arithmetic: no tolerance anywhere in this file.

GROUPING.  F = 64, D = 64, f16, a random table of 3100 rows.  The single-pass scans work in blocks of DD_BLOCK = 1024, so R (k_dd_claim,
k_dd_leaders) and the distinct count U (k_dd_segstart) are put at 1023, 1024, 1025, at multiples of 1024 -- where the total seg_start[U]
is written by thread 0 of a block past the data -- and at 3072 = U for three full blocks of look-back.  Empty (-1) and invalid indices
share the zero row's slot; slots are numbered by first appearance, not by row number; vv_forward_backward_q1 CAN take the de-duplicated
path (without dropout it always does), so one case puts composite rows past n_rows.

SEGMENT SUMS.  k_segsum is exact by construction: a float64 sum of at most 2^13 16-bit addends (order-independent), rounded to float,
then to 16 bits.  On the row-writing path (every D but 512 / 1024; at D = 512 with VV_SEG_BWD=0) the addends come back through
blobs(ip1_diff=True); the test first asserts that ip1_diff * scale is exactly representable in the 16-bit type, then compares dyu[:U]
with np.array_equal and requires zeros in rows U .. ceil(U / 64) * 64 (the weight-gradient K loop reads whole 64-row steps).  Every case
runs a batch of all-distinct rows first, so those rows hold stale sums that have to be cleared.  Dp is D rounded up to 256: D = 64 gives
Dp = 256 (half a 512-column chunk: lanes 32 .. 63 idle), D = 320 gives Dp = 512 (one chunk, 192 padding columns), and D = 768 (Dp = 768)
is added so that the chunk loop runs a second, partial time.

STATE.  Epoch-tagged key / aggregate words that are never reset, four rotating array sets, the distinct-row hint that sizes the next
forward GEMM and the dYu rows between U and the next multiple of 64 all outlive a step.  One context runs nine steps over batches of
U = 2050, 2, 1025, 1024 (more than two rotations; a shrinking and a growing U), a second alternates R = 1025 and R = 2050 (the arrays are
reallocated, key table and epoch survive); after EVERY step the arrays are checked and dW, db, loss, ip2 and dyu compared bit for bit
with a fresh context that ran only that batch.  In f16 the gradient scale is state too, by design: from the fifth step on the host moves
it when a reported max |dY| lies outside [2^5, 2^13) scaled units (api.hip, fb_impl).  A fresh context cannot be given another scale, so
the f16 runs use a loss_weight that keeps every batch's maxima inside that window and ASSERT that the scale stayed (the test fails
there, loudly, if it ever moves); bf16 has no scale and covers the same state without that condition.
"""
import os

import numpy as np
import pytest

from tests.pyref import dedup_groups_check, dedup_groups_expected
from tests.test_gpu_parity import round_operand, vv  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PRECS = ["f16", "bf16"]
N_ROWS, F = 3100, 64
SHAPE = {3: (1, 2, 1), 1023: (33, 5, 26), 1024: (64, 4, 12), 1025: (41, 5, 20), 2048: (128, 4, 12), 2050: (41, 5, 45), 3072: (192, 4, 12),
         800: (16, 5, 45)}        # R -> (B, C, Nn)
# f16, see STATE above: an INPUT of the tests, not a bound -- nothing is compared with it.  At loss_weight 1 the scaled maxima of the state
# tests' batches (rows and sums) lie between 2^4 and 2^5.3 (snapshot() prints them); 16 puts them at 2^8 .. 2^9.3, the middle of the window
# [2^5, 2^13), four binades from either end.  Should they ever leave it the tests fail at the scale assertion, they do not pass wrongly.
LOSS_WEIGHT = 16.0


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20)
    table = rng.random((N_ROWS, F), dtype=np.float32)
    params = {}
    for D in (64, 320, 512, 768):
        r = np.random.default_rng(100 + D)
        params[D] = ((r.standard_normal((D, F)) * 0.1).astype(np.float32), (r.standard_normal(D) * 0.1).astype(np.float32))
    return table, params


def engine(vv, world, prec="f16", D=64, seg_bwd=None):  # noqa: F811
    table, params = world
    if seg_bwd is not None:
        os.environ["VV_SEG_BWD"] = "1" if seg_bwd else "0"
    try:
        eng = vv.Engine(0, prec)
    finally:
        os.environ.pop("VV_SEG_BWD", None)
    eng.table_set(table)
    eng.params_set(*params[D])
    return eng


def cfg_of(vv, R, **kw):  # noqa: F811
    B, C, Nn = SHAPE[R]
    assert B * (C + Nn) == R
    return vv.StepConfig(B, C, Nn, **kw)


def shaped(flat, R):
    B, C, Nn = SHAPE[R]
    return np.asarray(flat, np.int32).reshape(B, C + Nn)


def batch_random(R, seed, n_pool=300):
    """Random indices over about n_pool rows spread over the whole table."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(N_ROWS, n_pool, replace=False)
    return shaped(pool[rng.integers(0, n_pool, R)], R)


def batch_with_u(R, U, seed):
    """U distinct rows, each placed once, the rest filled from them, shuffled."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(N_ROWS, U, replace=False)
    flat = np.concatenate([pool, pool[rng.integers(0, U, R - U)]])
    rng.shuffle(flat)
    assert len(np.unique(flat)) == U
    return shaped(flat, R)


def step_and_check(eng, cfg, idx, n_rows=N_ROWS, dyu=False, **fb):
    if fb:
        eng.forward_backward(cfg, **fb)
    else:
        eng.forward_backward(cfg, idx)
    got = eng.dedup_groups(dyu=dyu)
    exp = dedup_groups_expected(idx, n_rows)
    dedup_groups_check(got, exp)
    assert eng.dedup_stats() == (exp["R"], exp["U"])
    return got, exp


# ------------------------------------------------------------------------------- the accessor's contract
def test_accessor_refuses_without_a_deduplicated_pass(vv, world):  # noqa: F811
    eng = engine(vv, world)
    with pytest.raises(vv.VVError, match="no forward pass"):
        eng._chk(eng.L.vv_dedup_groups_get(eng.h, *([None] * 9)))
    idx = batch_random(3, 1)
    eng.set_dedup(False)
    eng.forward_backward(cfg_of(vv, 3), idx)
    with pytest.raises(vv.VVError, match="dense"):
        eng._chk(eng.L.vv_dedup_groups_get(eng.h, *([None] * 9)))
    eng.set_dedup(True)
    eng.forward_backward(cfg_of(vv, 3), idx)
    eng._chk(eng.L.vv_dedup_groups_get(eng.h, *([None] * 9)))          # every output is optional
    dW = eng.grads()[0].copy()
    eng.dedup_groups()
    assert np.array_equal(eng.grads()[0], dW)                           # read-only
    eng.close()


# ------------------------------------------------------------------------------- grouping: boundaries of R and U
@pytest.mark.parametrize("R", [3, 1023, 1024, 1025, 2048, 2050])
def test_grouping_at_the_boundaries_of_R(vv, world, R):  # noqa: F811
    eng = engine(vv, world)
    got, exp = step_and_check(eng, cfg_of(vv, R), batch_random(R, seed=R))
    assert exp["Rp"] == {3: 256, 1023: 1024, 1024: 1024, 1025: 1280, 2048: 2048, 2050: 2304}[R]
    assert 1 < exp["U"] <= 300
    eng.close()


@pytest.mark.parametrize("R,U", [(2050, 1), (2050, 2), (2050, 1023), (2050, 1024), (2050, 1025), (2050, 2048), (2050, 2050),
                                 (3072, 3072), (1024, 1024)])
def test_grouping_at_the_boundaries_of_U(vv, world, R, U):  # noqa: F811
    eng = engine(vv, world)
    got, exp = step_and_check(eng, cfg_of(vv, R), batch_with_u(R, U, seed=7 * R + U))
    assert exp["U"] == U and got["seg_start"][U] == R
    if U == R:
        assert np.array_equal(got["map"], np.arange(R)) and (got["cnt"][:U] == 1).all() and (got["ord"] == 0).all()
    eng.close()


# ------------------------------------------------------------------------------- grouping: empty, invalid, order, composite rows
def test_empty_slots_form_one_slot_of_the_zero_row(vv, world):  # noqa: F811
    R = 2050
    idx = batch_random(R, seed=11)
    flat = idx.reshape(-1)
    flat[np.random.default_rng(12).random(R) < 0.05] = -1
    flat[0] = 17                                                        # (slot 0 is a table row here; the next test has the other case)
    eng = engine(vv, world)
    got, exp = step_and_check(eng, cfg_of(vv, R), idx)
    n_empty = int((flat == -1).sum())
    assert 50 < n_empty < 200
    z = np.flatnonzero(got["uniq_rows"][:exp["U"]] == N_ROWS)
    assert len(z) == 1 and got["cnt"][z[0]] == n_empty
    eng.close()


def test_invalid_device_indices_share_the_zero_rows_slot(vv, world):  # noqa: F811
    import torch
    R = 1025
    idx = batch_random(R, seed=13)
    flat = idx.reshape(-1)
    flat[5], flat[77], flat[600], flat[1024] = -7, N_ROWS, 10 ** 9, -1
    t = torch.from_numpy(idx).to("cuda:0")
    torch.cuda.synchronize()
    eng = engine(vv, world)
    got, exp = step_and_check(eng, cfg_of(vv, R), idx, idx_dev_ptr=t.data_ptr())
    z = int(got["map"][5])
    assert got["uniq_rows"][z] == N_ROWS and got["cnt"][z] == 4 and (got["map"][[77, 600, 1024]] == z).all()
    eng.close()


def test_first_instance_empty_makes_slot_zero_the_zero_row(vv, world):  # noqa: F811
    R = 1025
    idx = batch_random(R, seed=14)
    idx.reshape(-1)[[0, 900]] = -1
    eng = engine(vv, world)
    got, exp = step_and_check(eng, cfg_of(vv, R), idx)
    assert got["uniq_rows"][0] == N_ROWS and got["map"][0] == 0 and got["map"][900] == 0 and got["cnt"][0] == 2
    eng.close()


def test_slots_follow_first_appearance_not_row_number(vv, world):  # noqa: F811
    R = 1025
    idx = shaped(3000 - np.arange(R) // 2, R)                           # every row twice, first appearances in DESCENDING row number
    eng = engine(vv, world)
    got, exp = step_and_check(eng, cfg_of(vv, R), idx)
    U = exp["U"]
    assert U == 513 and np.array_equal(got["uniq_rows"][:U], 3000 - np.arange(U)) and (np.diff(got["uniq_rows"][:U]) < 0).all()
    eng.close()


def test_q1_composite_rows_lie_past_the_table(vv, world):  # noqa: F811
    """vv_forward_backward_q1 takes the de-duplicated path whenever vv_forward_backward would (no dropout): every slot whose last feature
    comes from another row becomes a scratch row n_rows + 1 + p, p in instance order, and each of those is a distinct row of its own."""
    R = 1025
    idx = batch_random(R, seed=15)
    flat = idx.reshape(-1)
    flat[[3, 500]] = -1
    last = idx.copy()
    lf = last.reshape(-1)
    rng = np.random.default_rng(16)
    q1 = np.sort(rng.choice(R, 120, replace=False))
    lf[q1] = rng.integers(-1, N_ROWS, len(q1))
    lf[3] = 9                                                           # an empty slot is never composite
    patched = flat.astype(np.int64).copy()
    comp = np.flatnonzero((flat != lf) & (flat >= 0))
    patched[comp] = N_ROWS + 1 + np.arange(len(comp))
    assert 100 <= len(comp) <= 121
    eng = engine(vv, world)
    cfg = cfg_of(vv, R)
    eng.forward_backward_q1(cfg, idx, last)
    got = eng.dedup_groups(dyu=False)
    exp = dedup_groups_expected(patched, N_ROWS, row_limit=N_ROWS + 1 + len(comp))
    dedup_groups_check(got, exp)
    assert eng.dedup_stats() == (R, exp["U"]) and (got["rows"][comp] > N_ROWS).all() and (got["cnt"][got["map"][comp]] == 1).all()
    # and the plain entry point right after it, in the same context: the scratch rows are gone from the grouping
    step_and_check(eng, cfg, idx)
    eng.close()


# ------------------------------------------------------------------------------- k_segsum, exactly
def to16(x32, prec):
    """fp32 -> the 16-bit type (round to nearest even) -> fp32"""
    x32 = np.ascontiguousarray(x32, np.float32)
    return x32.astype(np.float16).astype(np.float32) if prec == "f16" else round_operand(x32, "bf16")


def instance_rows(ip1_diff, cfg):
    """blobs()'s [ch * B + b] rows as instance rows r = b (C + Nn) + ch"""
    B, CN = cfg.c.B, cfg.c.C + cfg.c.Nn
    return np.ascontiguousarray(ip1_diff.reshape(CN, B, -1).transpose(1, 0, 2)).reshape(B * CN, -1)


def check_segsum(eng, cfg, got, exp, prec, tag):
    U, D = exp["U"], eng.D
    scale = np.float32(got["scale"])
    assert scale > 0 and np.frexp(scale)[0] == 0.5 and (prec == "f16" or scale == 1.0)       # a power of two
    dy = instance_rows(eng.blobs(cfg, ip2=False, scores=False, ip1_diff=True)["ip1_diff"], cfg).astype(np.float64) * np.float64(scale)
    # the inputs' exactness: what the test sums is what the kernel read
    assert np.array_equal(dy.astype(np.float32).astype(np.float64), dy), "ip1_diff * scale is not exact in fp32"
    assert np.array_equal(to16(dy.astype(np.float32), prec).astype(np.float64), dy), "ip1_diff * scale is not exact in " + prec
    m = exp["map"].astype(np.int64)
    s64, absum = np.zeros((U, D)), np.zeros((U, D))
    np.add.at(s64, m, dy)
    np.add.at(absum, m, np.abs(dy))
    # Order independence of the float64 sum, per element.  (a) Every addend is a multiple of q = the smallest unit in the last place among
    # them (p significant bits: 2^(e - p) for an addend in [2^(e-1), 2^e)); while sum |x| < 2^53 q every partial sum, in any order, is a
    # multiple of q that float64 holds exactly.  f16 sums of up to 2^13 addends always are ((a) must hold everywhere); bf16 addends can span
    # more binades, and then (b): a float64 sum of n terms in any order lies within n 2^-53 sum |x| of the true one, two orders within
    # twice that, and the float that interval rounds to must not depend on where in it the sum lies.
    p = 11 if prec == "f16" else 8
    ulp = np.where(dy != 0, np.ldexp(1.0, np.frexp(dy)[1] - p), np.inf)
    q = np.full((U, D), np.inf)
    np.minimum.at(q, m, ulp)
    exact = absum < 2.0 ** 53 * q                                       # (an all-zero element: 0 < inf)
    bound = 2.0 * exp["cnt"][:U, None] * 2.0 ** -53 * absum
    stable = (s64 - bound).astype(np.float32) == (s64 + bound).astype(np.float32)
    assert (exact if prec == "f16" else exact | stable).all(), "the float64 sums depend on the order of the addends: the inputs are wrong"
    want = to16(s64.astype(np.float32), prec) / scale                    # the kernel's two-step rounding, then the accessor's 1 / scale
    dyu = got["dyu"]
    assert dyu.shape == (exp["Rp"], D) and np.abs(dyu).max() > 0 and np.abs(want).max() > 0
    once = to16_once(s64, prec) / scale
    print("SEGSUM %s: U %d, longest segment %d, scale %g, max |sum| %.3e scaled; %d of %d elements differ from ONE rounding float64 -> %s" % (
        tag, U, exp["cnt"].max(), scale, np.abs(s64).max(), int((once != want).sum()), want.size, prec))
    if not np.array_equal(dyu[:U], want):
        bad = np.argwhere(dyu[:U] != want)
        u, d = bad[0]
        raise AssertionError("%s: %d elements of dyu differ in %d slots; first: slot %d (%d instances) column %d: got %r, expected %r" % (
            tag, len(bad), len(np.unique(bad[:, 0])), u, exp["cnt"][u], d, dyu[u, d], want[u, d]))
    Uk = (U + 63) // 64 * 64
    assert not dyu[U:Uk].any(), "%s: rows U .. ceil(U / 64) * 64 of dYu are not zero (%d nonzero elements)" % (tag, np.count_nonzero(dyu[U:Uk]))


def to16_once(x64, prec):
    """float64 -> the 16-bit type in ONE rounding (informational)"""
    if prec == "f16":
        return x64.astype(np.float16).astype(np.float32)
    u = np.ascontiguousarray(x64, np.float64).view(np.uint64)
    drop = np.uint64(52 - 7)                                            # bf16 keeps 7 of float64's 52 fraction bits
    one = np.uint64(1)
    r = ((u + ((one << (drop - one)) - one) + ((u >> drop) & one)) >> drop) << drop
    return r.view(np.float64).astype(np.float32)                        # (exponents of gradient sums are far inside bf16's range)


def segsum_case(vv, world, prec, D, R, idx, seg_bwd=None, tag=""):  # noqa: F811
    eng = engine(vv, world, prec, D, seg_bwd)
    # the form this case is written for: per-instance 16-bit rows + k_segsum.  D = 512 / 1024 take it only with the segment-wise backward off
    assert D not in (512, 1024) or eng.get_option("seg_bwd") == 0, "VV_SEG_BWD=0 was not honoured: k_seg_bwd would form the sums"
    cfg = cfg_of(vv, R, loss_weight=LOSS_WEIGHT)
    step_and_check(eng, cfg, batch_with_u(R, min(R, 2050), seed=99))   # all distinct first: every row of dYu up to R holds a sum
    got, exp = step_and_check(eng, cfg, idx, dyu=True)
    check_segsum(eng, cfg, got, exp, prec, "%s %s D %d" % (tag, prec, D))
    eng.close()
    return got, exp


@pytest.mark.parametrize("prec", PRECS)
def test_segment_sums_exact_d64_u1025(vv, world, prec):  # noqa: F811
    got, exp = segsum_case(vv, world, prec, 64, 2050, batch_with_u(2050, 1025, seed=31), tag="R 2050 U 1025")
    assert exp["U"] == 1025


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("D", [320, 768])
def test_segment_sums_exact_over_the_chunk_loop(vv, world, prec, D):  # noqa: F811
    got, exp = segsum_case(vv, world, prec, D, 1025, batch_random(1025, seed=32), tag="R 1025")
    assert 200 < exp["U"] <= 300


@pytest.mark.parametrize("prec", PRECS)
def test_segment_sums_exact_d512_long_segments(vv, world, prec):  # noqa: F811
    """One row held by 600 instances, one by 65, one by 64, one by 1 (and 70 more instances over 30 rows); D = 512 takes the row-writing
    path only with VV_SEG_BWD=0."""
    R = 800
    rng = np.random.default_rng(33)
    pool = rng.choice(N_ROWS, 34, replace=False)
    flat = np.concatenate([np.repeat(pool[:4], [600, 65, 64, 1]), pool[4 + rng.integers(0, 30, 70)]])
    rng.shuffle(flat)
    got, exp = segsum_case(vv, world, prec, 512, R, shaped(flat, R), seg_bwd=False, tag="R 800 long")
    counts = sorted(exp["cnt"][:exp["U"]].tolist())
    assert counts[-3:] == [64, 65, 600] and counts[0] == 1


# ------------------------------------------------------------------------------- state across steps
def snapshot(eng, cfg, idx):
    """One step in eng: the grouping checked against numpy, and everything a later consumer reads"""
    got, exp = step_and_check(eng, cfg, idx, dyu=True)
    Uk = (exp["U"] + 63) // 64 * 64
    dW, db = eng.grads()
    print("STATE %s R %d U %d: scale %g, max |dyu| %.4g scaled" % (eng.prec, exp["R"], exp["U"], got["scale"], np.abs(got["dyu"][:exp["U"]]).max() * got["scale"]))
    return dict(U=exp["U"], dW=dW, db=db, loss=eng.loss(), ip2=eng.blobs(cfg, scores=False)["ip2"], dyu=got["dyu"][:Uk].copy(),
                scale=got["scale"], tile=int(eng.get_option("last_fwd_tile_rows")))


def same_as_fresh(s, f, tag):
    assert s["scale"] == f["scale"], "%s: the gradient scale moved (%g, fresh %g): not comparable with a fresh context" % (tag, s["scale"], f["scale"])
    for k in ("ip2", "dyu", "dW", "db"):
        assert np.array_equal(s[k], f[k]), "%s: %s differs from a fresh context's in %d elements" % (tag, k, int((s[k] != f[k]).sum()))
    assert s["loss"] == f["loss"], tag
    # The step's forward GEMM is planned from the distinct-row hint the previous step's grouping left (or this step's, if it has landed:
    # the launcher reads it late), a fresh context's from no hint.  At D = 64 (one column of tiles) and R <= 2304 no hint changes the
    # plan: 256-, 192- and 128-row tiles all fit one round of workgroups and the 128-row tile is the cheapest round, so both contexts
    # must have run that form.  (At a shape whose plan did depend on the hint only ip2's equality above could be asserted.)
    assert s["tile"] == f["tile"] == 128, (tag, s["tile"], f["tile"])


@pytest.fixture(scope="module")
def fresh(vv, world):  # noqa: F811
    """(prec, batch) -> the snapshot of a fresh context that ran only that batch; computed once, shared, never modified"""
    cache = {}

    def get(prec, R, idx):
        assert idx.size == R
        key = (prec, idx.shape, idx.tobytes())
        if key not in cache:
            eng = engine(vv, world, prec)
            cache[key] = snapshot(eng, cfg_of(vv, R, loss_weight=LOSS_WEIGHT), idx)
            eng.close()
        return cache[key]
    return get


BATCHES_2050 = [("u2050", 2050), ("u2", 2), ("u1025", 1025), ("u1024", 1024)]


@pytest.mark.parametrize("prec", PRECS)
def test_nine_steps_in_one_context_equal_fresh_contexts(vv, world, fresh, prec):  # noqa: F811
    R = 2050
    batches = [(name, batch_with_u(R, U, seed=40 + i)) for i, (name, U) in enumerate(BATCHES_2050)]
    eng = engine(vv, world, prec)
    cfg = cfg_of(vv, R, loss_weight=LOSS_WEIGHT)
    prev_u = 0
    for call in range(9):
        name, idx = batches[call % 4]
        s = snapshot(eng, cfg, idx)
        same_as_fresh(s, fresh(prec, R, idx), "%s call %d (%s after U %d)" % (prec, call, name, prev_u))
        prev_u = s["U"]
    assert eng.grad_scale_stats()[0] == 0                               # no step's gradients had to be produced again at another scale
    eng.close()


@pytest.mark.parametrize("prec", PRECS)
def test_alternating_shapes_in_one_context_equal_fresh_contexts(vv, world, fresh, prec):  # noqa: F811
    seq = [(1025, "r1025", batch_random(1025, seed=50)), (2050, "u1025", batch_with_u(2050, 1025, seed=42)),
           (1025, "r1025b", batch_with_u(1025, 1025, seed=51)), (2050, "u2", batch_with_u(2050, 2, seed=41))]
    eng = engine(vv, world, prec)
    for call in range(9):
        R, name, idx = seq[call % 4]
        s = snapshot(eng, cfg_of(vv, R, loss_weight=LOSS_WEIGHT), idx)
        same_as_fresh(s, fresh(prec, R, idx), "%s call %d (R %d %s)" % (prec, call, R, name))
    assert eng.grad_scale_stats()[0] == 0
    eng.close()
