"""vv_op_gemm_tn (k_lin_wgrad and its slab reduction) element for element against float64.  The operands are small integers, so
every partial sum is an integer below 2^24 and any correct order gives the same float: np.array_equal, no tolerance.  Shapes walk
the tile's edges (m, n below, at and above 32 / 128), the K step's (k = 1, 2, 63, 64, 65), one split +- 1 (the library's plan takes
128 rows per split at these sizes), three splits + 1, and two row blocks under lin_split_rows = 2 (a row block holds 128 splits).
lda / ldb exceed m / n, once by odd pads (the element-wise loads) and once on 16-byte rows (the vector loads and, where a tile is
full, the loop without column tests); the padding holds NaN, which must not leak.  Each case asserts the splits it expects."""
import numpy as np
import pytest

import videovector_amd as vv
from videovector_amd.engine import DevBuf

pytestmark = pytest.mark.gpu

MS, NS = (1, 31, 32, 33, 100, 129), (1, 32, 33, 96, 512)
# (k, lin_split_rows, splits expected, row blocks expected)
KS = [(1, 0, 1, 1), (2, 0, 1, 1), (63, 0, 1, 1), (64, 0, 1, 1), (65, 0, 1, 1), (127, 0, 1, 1), (128, 0, 1, 1), (129, 0, 2, 1),
      (385, 0, 4, 1), (257, 2, 128, 2), (200, 64, 4, 1)]


@pytest.fixture(scope="module")
def eng():
    e = vv.Engine(0, "f16")
    yield e
    e.set_option("lin_split_rows", 0)
    e.close()


def padded(rs, k, cols, ld):
    a = np.full((k, ld), np.nan, np.float32)
    a[:, :cols] = rs.randint(-3, 4, size=(k, cols))
    return a


@pytest.mark.parametrize("k,split_rows,splits,blocks", KS)
def test_gemm_tn_is_exact(eng, k, split_rows, splits, blocks):
    rs = np.random.RandomState(k)
    eng.set_option("lin_split_rows", split_rows)
    for m in MS:
        for n in NS:
            for pa, pb in ((3, 5), (-m % 4 + 4, -n % 4 + 4)):
                A, B = padded(rs, k, m, m + pa), padded(rs, k, n, n + pb)
                dA, dB, out = DevBuf(eng, A), DevBuf(eng, B), DevBuf(eng, np.full((m, n), np.nan, np.float32))
                eng.op_gemm_tn(dA, m + pa, dB, n + pb, k, m, n, out)
                want = A[:, :m].astype(np.float64).T @ B[:, :n].astype(np.float64)
                assert np.array_equal(out.get().astype(np.float64), want), (k, m, n, pa, pb)
                assert (eng.get_option("last_lin_splits"), eng.get_option("last_lin_blocks")) == (splits, blocks), (k, m, n)
                for d in (dA, dB, out):
                    d.free()


def test_gemm_tn_asymmetric_identity(eng):
    """A = I picks rows of an asymmetric B: a swapped output map would show."""
    eng.set_option("lin_split_rows", 0)
    k = m = 70
    n = 45
    A = np.eye(k, dtype=np.float32)
    B = (np.arange(k)[:, None] * 64 + np.arange(n)[None, :]).astype(np.float32)
    dA, dB, out = DevBuf(eng, A), DevBuf(eng, B), DevBuf(eng, (m, n))
    eng.op_gemm_tn(dA, m, dB, n, k, m, n, out)
    assert np.array_equal(out.get(), B)


@pytest.mark.parametrize("kw", [dict(k=0), dict(m=0), dict(n=0), dict(lda=3), dict(ldb=3)])
def test_gemm_tn_refuses_bad_shapes(eng, kw):
    a = dict(k=4, m=4, n=4, lda=4, ldb=4)
    a.update(kw)
    buf = DevBuf(eng, (16,))
    with pytest.raises(vv.VVError):
        eng.op_gemm_tn(buf, a["lda"], buf, a["ldb"], a["k"], a["m"], a["n"], buf)
