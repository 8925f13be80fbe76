"""Everything between ip2 and the weight-gradient GEMM's operand, restated in numpy (float64; tests only): the score / loss forward
and the segment-wise backward of videovector_amd/csrc/kernels_score.hip (k_score_fwd / k_score_stream + k_seg_bwd / k_seg_bwd_cnt, and the
per-instance kernels k_score_loss / k_score_loss_reg), from the math stated at the head of that file:

    A = sum_j c_j H[j],  Ah = A / (|A| + eps)
    per q in {0, C..}: n_q = |H[q]|, t_q = Ah . H[q], score_q = t_q / (n_q + eps)
    d_k = s+ - s-_k, h = max(0, margin - d), loss += w_b h^2 (L2) or w_b |h| (L1), violations += d < 0
    g_k = grad_scale w_b (2 h | [h > 0]);  c_0 = -sum_k g_k, c_{C+k} = g_k
    dAh = sum_q c_q H[q] / (n_q + eps);   dH[q] = c_q (n_q^2 Ah - H[q] t_q) / (n_q^3 + eps)
    dA  = (sA dAh - A (A . dAh)) / (sA^1.5 + eps), dH[j] = c_j dA
    dY_i = dH_i drop_scale [ip2_i > 0]                 (the instance's own row carries its dropout mask)
    dyu[u] = sum of dY_i over the instances i of slot u  (the grouping: tests/pyref.py dedup_groups_expected, not the engine's)

The input is ip2 as Engine.blobs() returns it -- one row per instance, after ReLU and dropout -- so the forward GEMM that produced it
(held exactly by tests/test_gpu_gemm_exact.py) is outside: what is compared is these kernels alone.  dtype=np.float32 gives the same
function in float32 in numpy's own summation order; the GPU tests use the distance between the two to size their tolerances, never as a
reference.  Checked on the CPU by tests/test_score_ref_host.py.
"""
import numpy as np

from tests.pyref import dedup_groups_expected

EPS = 1e-10


def instance_order(x, B):
    """blobs()'s rows [ch * B + b] as instance rows r = b (C + Nn) + ch"""
    x = np.asarray(x)
    CN = x.shape[0] // B
    return np.ascontiguousarray(x.reshape(CN, B, -1).transpose(1, 0, 2)).reshape(B * CN, -1)


def score_ref(ip2, idx, n_rows, C, Nn, margin=2.0, norm=2, loss_weight=1.0, item_weight=None, ctx_coeff=None, global_count=0,
              dropout_ratio=0.0, h16=False, dtype=np.float64):
    """ip2 [(C+Nn) B][D] in blobs()'s row order (row ch * B + b), idx [B][C+Nn], n_rows the table's (its zero row is row n_rows).
    h16: the rows were stored as f16 -- asserted.  Returns a dict: target_score [B], negative_scores [B][Nn], d [B][Nn], loss, violations,
    sens (sum of |dloss / dd_k|), dY [R][D] (instance order r = b (C+Nn) + ch), dyu [U][D], groups (dedup_groups_expected), and the
    per-item pieces Ah [B][D], dA [B][D], alpha [R] (dY_i = alpha_i V - beta_i x: the factor of Ah_b or dA_b in instance i's gradient), pos [R][D] = ip2_i > 0."""
    T = dtype
    idx = np.asarray(idx)
    B, CN = idx.shape
    assert CN == C + Nn and ip2.shape[0] == B * CN
    D = ip2.shape[1]
    ip2 = np.asarray(ip2, np.float32)
    ds = T(1.0 / (1.0 - dropout_ratio)) if dropout_ratio > 0 else T(1.0)
    if h16:
        stored = ip2 / np.float32(ds)                                  # (1 / (1 - ratio) a power of two in the tests: exact)
        assert np.array_equal(stored.astype(np.float16).astype(np.float32), stored), "ip2 is not what an f16 row holds"
    eps = T(EPS)
    H = ip2.astype(T).reshape(CN, B, D)
    coeff = (np.full(C - 1, 1.0 / (C - 1), np.float32) if ctx_coeff is None else np.asarray(ctx_coeff, np.float32)).astype(T)
    w = (np.ones(B, np.float32) if item_weight is None else np.asarray(item_weight, np.float32)).astype(T)
    A = np.tensordot(coeff, H[1:C], axes=(0, 0))                       # [B][D]
    sA = (A * A).sum(1)
    Ah = A / (np.sqrt(sA) + eps)[:, None]
    P = np.concatenate([H[0:1], H[C:]], 0)                             # [1+Nn][B][D]
    n2 = (P * P).sum(2)
    n = np.sqrt(n2)
    t = (P * Ah[None]).sum(2)
    s = t / (n + eps)
    sp, sn = s[0], s[1:].T
    d = sp[:, None] - sn
    h = np.maximum(T(0), T(margin) - d)
    count = B * Nn
    gcount = global_count if global_count else count
    per = w[:, None] * (h * h if norm == 2 else np.abs(h))
    loss = T(np.float32(loss_weight)) / T(count) * per.sum()
    gs = T(np.float32(loss_weight)) / T(gcount)
    g = gs * w[:, None] * (2 * h if norm == 2 else (h > 0).astype(T))
    sens = (T(np.float32(loss_weight)) / T(count) * w[:, None] * (2 * h if norm == 2 else (h > 0).astype(T))).sum()
    c = np.concatenate([-g.sum(1)[None], g.T], 0)                      # [1+Nn][B]
    dAh = (c[:, :, None] * P / (n + eps)[:, :, None]).sum(0)
    cd = c / (n2 * n + eps)
    alpha_q, beta_q = cd * n2, cd * t
    dP = alpha_q[:, :, None] * Ah[None] - beta_q[:, :, None] * P
    dA = (sA[:, None] * dAh - A * (A * dAh).sum(1)[:, None]) / (sA * np.sqrt(sA) + eps)[:, None]
    dE = np.empty_like(H)
    dE[0], dE[C:] = dP[0], dP[1:]
    alpha = np.empty((CN, B), T)
    alpha[0], alpha[C:] = alpha_q[0], alpha_q[1:]
    for j in range(1, C):
        dE[j] = coeff[j - 1] * dA
        alpha[j] = coeff[j - 1]
    dY = instance_order((dE * ds * (H > 0)).reshape(CN * B, D), B)
    pos = instance_order((H > 0).reshape(CN * B, D), B)
    groups = dedup_groups_expected(idx, n_rows)
    dyu = np.zeros((groups["U"], D), T)
    np.add.at(dyu, groups["map"].astype(np.int64), dY)
    return dict(target_score=sp, negative_scores=sn, d=d, loss=loss, violations=float((d < 0).sum()), sens=sens, dY=dY, dyu=dyu,
                groups=groups, Ah=Ah, dA=dA, pos=pos, alpha=np.ascontiguousarray((alpha * ds).T).reshape(-1))


def ulp16(x, prec):
    """Spacing of the 16-bit type at |x| (float64 array): f16 2^(e-11) for |x| in [2^(e-1), 2^e), 2^-24 below 2^-14 (subnormals) and at 0;
    bf16 2^(e-8), 2^-133 below 2^-126 and at 0."""
    x = np.abs(np.asarray(x, np.float64))
    e = np.where(x > 0, np.frexp(x)[1], -2000).astype(np.float64)       # (frexp(0) reports exponent 0)
    if prec == "f16":
        return np.ldexp(1.0, (np.maximum(e, -13) - 11).astype(np.int64))
    return np.ldexp(1.0, (np.maximum(e, -125) - 8).astype(np.int64))


def v16_term(ref, B, C, Nn):
    """The half-ulps of the V16 form's own roundings (k_score_stream<.., V16>: Ah_b leaves as f16; dA_b as f16 times the power of two sc_b
    that puts its largest magnitude in [2^13, 2^14), at most 2^126), carried linearly through dY_i = alpha_i V[vec_i] - beta_i x_u to every element of
    dyu, in unscaled units [U][D]:
        target / negative instance i of item b:  |alpha_i| ulp16(Ah_b[d]) / 2
        context instance j of item b:            |coeff_j drop_scale| ulp16(dA_b[d] sc_b) / (2 sc_b)
    summed over the instances of the slot whose own ip2 element is positive, all from the float64 reference's values."""
    CN = C + Nn
    Ah, dA = ref["Ah"], ref["dA"]
    m = np.abs(dA).max(1)
    sc = np.where(m > 0, np.ldexp(1.0, np.minimum(14 - np.frexp(m)[1], 126)), 1.0)[:, None]      # (the kernel's exponent stops at 126)
    hA = ulp16(Ah, "f16") / 2
    hD = ulp16(dA * sc, "f16") / 2 / sc
    is_ctx = np.tile((np.arange(CN) >= 1) & (np.arange(CN) < C), B)
    item = np.repeat(np.arange(B), CN)
    per = np.abs(ref["alpha"])[:, None] * np.where(is_ctx[:, None], hD[item], hA[item]) * ref["pos"]
    out = np.zeros_like(ref["dyu"])
    np.add.at(out, ref["groups"]["map"].astype(np.int64), per)
    return out
