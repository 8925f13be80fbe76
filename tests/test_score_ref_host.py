"""tests/score_ref.py checked on the CPU: against the fp32 oracle on its own ip2, its gradient against central finite differences of its
own float64 loss, and the degenerate batches.  (The GPU comparison that uses it: tests/test_gpu_score_seg_exact.py.)"""
import numpy as np
import pytest

from tests.score_ref import instance_order, score_ref, ulp16, v16_term


def small_case(seed, B, C, Nn, F, D, n_rows=40):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((n_rows, F)).astype(np.float32)
    W = (rng.standard_normal((D, F)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(D) * 0.1).astype(np.float32)
    idx = rng.integers(0, n_rows, (B, C + Nn)).astype(np.int32)
    return table, idx, W, b


@pytest.mark.parametrize("case", ["plain", "weighted_l1", "dropout_coeff_global"])
def test_against_the_oracle(oracle, case):
    B, C, Nn, F, D = 6, 4, 5, 24, 32
    table, idx, W, b = small_case(3, B, C, Nn, F, D)
    idx[1, 2] = idx[4, 0]                                               # repeats across items: slots with several instances
    rng = np.random.default_rng(4)
    kw = {"plain": dict(),
          "weighted_l1": dict(norm=1, margin=0.5, item_weight=(1 + np.arange(B) % 3).astype(np.float32), loss_weight=2.0),
          "dropout_coeff_global": dict(ctx_coeff=[0.2, 0.3, 0.5], global_count=4 * B * Nn, dropout_ratio=0.5,
                                       dropout_mask=(rng.random((B * (C + Nn), D)) < 0.5).astype(np.uint8))}[case]
    o = oracle.forward_backward(table, idx, W, b, C_=C, Nn=Nn, want=("H", "s_true", "s_bogus", "dY"), **kw)
    rkw = {k: v for k, v in kw.items() if k != "dropout_mask"}
    r = score_ref(o["H"], idx, len(table), C, Nn, **rkw)
    # the oracle computes in fp32: its distance from float64 is a few units of 2^-24 of the largest term of each sum
    assert np.abs(o["s_true"][:, 0] - r["target_score"]).max() <= 4e-7 and np.abs(o["s_bogus"] - r["negative_scores"]).max() <= 4e-7
    assert abs(o["loss"] - r["loss"]) <= 2e-6 * r["loss"] and o["violations"] == r["violations"]
    dY = instance_order(o["dY"], B)
    assert np.abs(r["dY"]).max() > 0
    assert np.abs(dY - r["dY"]).max() <= 2e-5 * np.abs(r["dY"]).max()
    # the per-slot sums against a plain loop over a dictionary of rows
    slots = {}
    for i, row in enumerate(idx.reshape(-1)):
        slots.setdefault(int(row), []).append(i)
    assert len(slots) == r["groups"]["U"] < idx.size
    for u, (row, inst) in enumerate(slots.items()):                     # (dict order = order of first appearance = slot order)
        assert np.allclose(r["dyu"][u], r["dY"][inst].sum(0), rtol=0, atol=1e-15)


@pytest.mark.parametrize("norm", [2, 1])
def test_gradient_against_finite_differences(norm):
    B, C, Nn, D = 3, 3, 4, 16
    rng = np.random.default_rng(10 + norm)
    ip2 = (rng.random((B * (C + Nn), D)) + 0.05).astype(np.float32)      # all positive: ReLU's mask is 1 everywhere
    idx = np.arange(B * (C + Nn), dtype=np.int32).reshape(B, C + Nn)
    kw = dict(margin=0.05 if norm == 1 else 2.0, norm=norm, item_weight=np.array([1.0, 2.0, 0.5], np.float32), ctx_coeff=[0.25, 0.75],
              loss_weight=1.5)
    r = score_ref(ip2, idx, 1000, C, Nn, **kw)
    if norm == 1:
        assert 0 < (r["d"] < 0.05).sum() < B * Nn and np.abs(0.05 - r["d"]).min() > 1e-3       # both hinge states, none at the kink
    # score_ref takes float32 rows; a step of 2^-10 on values in [0.05, 1.05) is exact in float32
    step = 2.0 ** -10
    fd = np.zeros((B * (C + Nn), D))
    for i in range(ip2.shape[0]):
        for d in range(D):
            p, m = ip2.copy(), ip2.copy()
            p[i, d] += step; m[i, d] -= step
            fd[i, d] = (score_ref(p, idx, 1000, C, Nn, **kw)["loss"] - score_ref(m, idx, 1000, C, Nn, **kw)["loss"]) / (2 * step)
    fd = instance_order(fd, B)
    # central differences: error ~ step^2 |f'''| / 6 ~ 1e-6 of the gradient's size here
    assert np.abs(fd - r["dY"]).max() <= 2e-5 * np.abs(r["dY"]).max(), np.abs(fd - r["dY"]).max() / np.abs(r["dY"]).max()
    # an element at 0 takes no gradient (ReLU / dropout backward) and moves nobody else's
    z = ip2.copy()
    z[2, 5] = 0
    rz = score_ref(z, idx, 1000, C, Nn, **kw)
    zi = instance_order(np.arange(z.shape[0])[:, None], B).reshape(-1).tolist().index(2)
    assert rz["dY"][zi, 5] == 0 and (rz["dY"][zi, :5] != 0).all()


def test_degenerate_batches():
    B, C, Nn, D = 4, 3, 5, 16
    rng = np.random.default_rng(20)
    idx = rng.integers(0, 12, (B, C + Nn)).astype(np.int32)
    # all rows equal: s Ah - t x = 0 for every instance
    same = np.tile((rng.random(D) + 0.1).astype(np.float32), (B * (C + Nn), 1))
    r = score_ref(same, idx, 12, C, Nn)
    assert np.abs(r["dY"]).max() <= 1e-15 and np.abs(r["d"]).max() <= 1e-15 and abs(r["loss"] - 4.0) <= 1e-12
    # a zero row (a negative of item 1): score 0 / (0 + eps) = 0, finite everywhere, no gradient into the row
    ip2 = (rng.random((B * (C + Nn), D)) + 0.05).astype(np.float32)
    ip2[(C + 1) * B + 1] = 0
    r = score_ref(ip2, idx, 12, C, Nn)
    assert r["negative_scores"][1, 1] == 0 and np.isfinite(r["dY"]).all() and np.isfinite(r["dyu"]).all()
    assert not r["dY"][1 * (C + Nn) + C + 1].any()
    # an item whose every slot is -1: its rows are the zero row's projection, all equal -> no gradient from it; its instances share ONE slot
    idx2 = idx.copy()
    idx2[2] = -1
    ip3 = ip2.copy()
    ip3[np.arange(C + Nn) * B + 2] = same[0]
    r = score_ref(ip3, idx2, 12, C, Nn)
    g = r["groups"]
    u = g["map"][2 * (C + Nn)]
    assert g["uniq_rows"][u] == 12 and g["cnt"][u] == C + Nn
    assert np.abs(r["dY"][2 * (C + Nn):3 * (C + Nn)]).max() <= 1e-15 and np.abs(r["dyu"][u]).max() <= 1e-15
    assert np.abs(r["dyu"]).max() > 1e-3


def test_float32_twin_and_the_rounding_helpers():
    B, C, Nn, D = 4, 3, 5, 64
    rng = np.random.default_rng(30)
    idx = rng.integers(0, 12, (B, C + Nn)).astype(np.int32)
    ip2 = np.maximum(rng.standard_normal((B * (C + Nn), D)), 0).astype(np.float16).astype(np.float32)
    r64 = score_ref(ip2, idx, 12, C, Nn, h16=True)
    r32 = score_ref(ip2, idx, 12, C, Nn, h16=True, dtype=np.float32)
    assert r32["dyu"].dtype == np.float32 and r32["negative_scores"].dtype == np.float32
    e = np.abs(r32["dyu"] - r64["dyu"]).max()
    assert 0 < e <= 1e-5 * np.abs(r64["dyu"]).max()
    with pytest.raises(AssertionError, match="f16 row"):
        score_ref(ip2 + np.float32(1e-4), idx, 12, C, Nn, h16=True)
    x = np.array([0.0, 2.0 ** -25, 2.0 ** -14, 1.0, 1.5, 2.0, 65504.0])
    assert np.array_equal(ulp16(x, "f16"), 2.0 ** np.array([-24, -24, -24, -10, -10, -9, 5.0]))
    assert np.array_equal(ulp16(x[3:6], "bf16"), 2.0 ** np.array([-7, -7, -6.0]))
    f = np.float16(1.0)
    assert np.nextafter(f, np.float16(2)) - f == ulp16(1.0, "f16")
    t = v16_term(r64, B, C, Nn)
    assert t.shape == r64["dyu"].shape and (t >= 0).all() and 0 < t.max() <= 2.0 ** -11 * 4 * np.abs(r64["alpha"]).max() * (B * (C + Nn))
