"""A numpy restatement of vv_ivfpq_search's own arithmetic (include/videovec.h states it), for the tests: the table chain, the ADC chain,
and the selection -- which is ivf_ref.search fed the approximate distances in place of d_items.  It computes NO k-means and NO centroid
distance of its own: the codes are given (the tests take them from Gallery(items[:, cols]).kmeans(iters=0, init=cb[m]).assign), and
d_cent / nn / the lists come as tests/ivf_ref.py takes them.  Every numpy operation below is one fp32 operation on fp32 operands, so
each product and each sum is rounded on its own, in the order written."""
import numpy as np

import ivf_ref

F32 = np.float32


def table(q, cb):
    """lut [n_q][M][ksub]: -2.0f * s + 0.0f, s the serial chain over sub-space m's columns in ascending order from +0.0f.
    q: [n_q][M * dsub], cb: [M][ksub][dsub]."""
    q, cb = np.asarray(q, F32), np.asarray(cb, F32)
    M, ksub, dsub = cb.shape
    assert q.shape[1] == M * dsub
    s = np.zeros((q.shape[0], M, ksub), F32)
    for col in range(dsub):
        prod = (q[:, col::dsub][:, :M, None] * cb[None, :, :, col]).astype(F32)      # q[i][m dsub + col] * cb[m][j][col]
        s = (s + prod).astype(F32)
    return (F32(-2.0) * s + F32(0.0)).astype(F32)


def adc(lut, codes):
    """a [n_q][n]: acc = lut[i][0][code[g][0]], then acc = acc + lut[i][m][code[g][m]] for m = 1 .. M - 1.  codes: [n][M], item order."""
    lut, codes = np.asarray(lut, F32), np.asarray(codes, np.int64)
    acc = lut[:, 0, codes[:, 0]]
    for m in range(1, codes.shape[1]):
        acc = (acc + lut[:, m, codes[:, m]]).astype(F32)
    return acc.astype(F32)


def search(q, cb, codes, d_cent, nn, metric, start, lst, nprobe, k):
    """ivf_ref.search's dict with the approximate distances as the items' distances: idx, dist, n_candidates, probes, candidates."""
    return ivf_ref.search(adc(table(q, cb), codes), d_cent, nn, metric, start, lst, nprobe, k)
