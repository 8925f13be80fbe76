"""Inputs, float64 references, comparisons and deliberately wrong models for the evaluation head (k_mean_rows, k_row_normalize,
k_gram, vv_retrieval_stats), shared by tests/test_gpu_eval_head_exact.py and its host self-check tests/test_eval_head_ref_host.py.

Every input is chosen so that the values on the path are exactly representable; the functions here assert that on the CPU before they
return a reference: a failure in this file means a wrong input, not a wrong kernel.

  table           integers 0 .. 3, about half of them zero, N_ROWS rows, three of them all zero    (exact in f16 and bf16, scale 1)
  W, b            the first D rows of the F x F identity, 0: the layer reads the 16-bit mean row out unchanged
  coefficients    1 / k for k in {1, 2, 4}, or distinct powers of two
  Gram operands   integers -3 .. 3
"""
import numpy as np

from tests.class_stats_ref import class_stats, distances
from tests.test_gpu_parity import round_operand, round_table

U = 2.0 ** -24                     # fp32 unit roundoff
N_ROWS = 200
ZERO_ROWS = (5, 6, 150)            # all-zero table rows ("a sample of zero features")
PRECS = ["f16", "bf16"]
TIE_P = {"f16": 10, "bf16": 7}     # x0 + x1 2^-p, x0 in {2, 3}, x1 odd: half an ulp of the 16-bit format above a representable value
RANGE_SCALE = 2.0 ** 16            # the range-scale case: the f16 table leaves scale 1 (max |x| = 3 x 2^16 > 2^14)
RANGE_SX = 2.0 ** -10              # ... for the power of two that moves 3 x 2^16 to [2^7, 2^8)


# ------------------------------------------------------------------------------- part 1: the window mean
def table(F, scale=1.0):
    rng = np.random.default_rng(1000 + F)
    T = (rng.integers(1, 4, size=(N_ROWS, F)) * (rng.random((N_ROWS, F)) < 0.5)).astype(np.float32)
    T[list(ZERO_ROWS)] = 0
    assert T[0].any() and T[N_ROWS - 1].any()
    return T * np.float32(scale)


def identity_layer(D, F, prec):
    W = np.eye(F, dtype=np.float32)[:D].copy()
    assert np.array_equal(round_operand(W, prec), W)
    return W, np.zeros(D, np.float32)


def window_rows(n, k, seed=0):
    """[n][k] table rows.  Sample 0 starts with the table's first row and (k > 1) ends with its last; with k = 1 the last row is sample 3
    (n >= 4) or takes the first row's place.  With room for them (n >= 3), sample 1 has one row in every slot and sample 2 a window of
    all-zero rows."""
    rows = np.random.default_rng(100003 * n + 17 * k + seed).integers(0, N_ROWS, size=(n, k)).astype(np.int32)
    if n >= 3:
        rows[1, :] = 123
        rows[2, :] = [ZERO_ROWS[j % len(ZERO_ROWS)] for j in range(k)]
    rows[0, 0] = 0
    rows[(0, k - 1) if k > 1 or n < 4 else (3, 0)] = N_ROWS - 1
    return rows


def coefficients(k, kind, prec="f16"):
    """'uniform': None (the product's 1 / k, dyadic for k in {1, 2, 4});  'distinct': 2^-1 .. 2^-k, all different, so a swapped or
    dropped slot changes the sum;  'tie' (k = 2): [1, 2^-p]."""
    if kind == "uniform":
        assert k in (1, 2, 4)
        return None
    if kind == "distinct":
        return (2.0 ** -np.arange(1, k + 1)).astype(np.float32)
    assert kind == "tie" and k == 2
    return np.array([1.0, 2.0 ** -TIE_P[prec]], np.float32)


def mean64(T, rows, coeff):
    """sum_j coeff[j] T[rows[i, j]] in float64, after asserting that every term is an integer count of one power-of-two unit and the sum
    of magnitudes stays below 2^24 units: every partial sum is then exact in fp32, in any order, fused or not."""
    k = rows.shape[1]
    c = np.full(k, 1.0 / k) if coeff is None else np.asarray(coeff, np.float64)
    terms = c[None, :, None] * T[rows].astype(np.float64)
    nz = np.abs(terms[terms != 0])
    unit = 2.0 ** np.floor(np.log2(nz.min())) if nz.size else 1.0
    while not np.array_equal(terms / unit, np.rint(terms / unit)):
        unit /= 2.0
        assert unit > 2.0 ** -40, "the terms share no power-of-two unit: the inputs are wrong"
    assert np.abs(terms).sum(1).max() / unit < 2 ** 24, "a partial sum can leave fp32's exact integers: the inputs are wrong"
    m = terms.sum(1)
    assert np.array_equal(m.astype(np.float32).astype(np.float64), m)
    return m


def round_rows(m, prec, sx=1.0):
    """What k_mean_rows stores for the fp32 mean m (table units: m * sx), read back: round-to-nearest-even to 16 bits."""
    s = np.float32(sx)
    return (round_table((m.astype(np.float32) * s).astype(np.float32), prec) / s).astype(np.float64)


def truncate_rows(m, prec):
    """The wrong model: the mean chopped to 16 bits (toward zero) instead of rounded."""
    x = m.astype(np.float32)
    if prec == "bf16":
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)


def mean_ref(T, rows, coeff, prec, D, sx=1.0):
    """The exact expected output of embed_mean(rows, coeff, relu=False, l2norm=False) through the identity layer."""
    ref = round_rows(mean64(T, rows, coeff), prec, sx)[:, :D]
    ref.setflags(write=False)
    return ref


def tie_inventory(T, rows, prec):
    """(down, up): masks [n][F] of the elements of the 'tie' case whose mean lies exactly half-way between two 16-bit values and that
    round-to-nearest-even resolves downwards / upwards."""
    m = mean64(T, rows, coefficients(2, "tie", prec))
    x0, x1 = T[rows[:, 0]], T[rows[:, 1]]
    tie = (x0 >= 2) & (x1 % 2 == 1)
    r, t = round_rows(m, prec), truncate_rows(m, prec)
    ulp = 2.0 ** -9 if prec == "f16" else 2.0 ** -6              # of a 16-bit value in [2, 4)
    assert np.array_equal((m - t)[tie], np.full(int(tie.sum()), ulp / 2)), "not half-way: the inputs are wrong"
    assert np.array_equal(r[~tie], m[~tie]) and np.array_equal(t[~tie], m[~tie])       # every other element is exact in 16 bits
    return tie & (r < m), tie & (r > m)


# wrong models of k_mean_rows, as float64 means to be passed through round_rows
def mean_last_slot_dropped(T, rows, coeff):
    k = rows.shape[1]
    c = np.full(k, 1.0 / k) if coeff is None else np.asarray(coeff, np.float64).copy()
    c[k - 1] = 0.0
    return (c[None, :, None] * T[rows].astype(np.float64)).sum(1)


def mean_last_column_from_slot0(T, rows, coeff):
    k = rows.shape[1]
    c = np.full(k, 1.0 / k) if coeff is None else np.asarray(coeff, np.float64)
    m = (c[None, :, None] * T[rows].astype(np.float64)).sum(1)
    m[:, -1] = c[0] * T[rows[:, 0], -1]
    return m


# ------------------------------------------------------------------------------- part 2: the L2 normalisation
def norm_rows(n):
    """n table rows for embed(..., l2norm=True); with n >= 3, row 1 is an all-zero row."""
    rows = np.random.default_rng(7 * n + 1).integers(0, N_ROWS, size=n).astype(np.int32)
    if n >= 3:
        rows[1] = ZERO_ROWS[0]
    return rows


def normalize_ref(e):
    """float64 e / (sqrt(sum e^2) + 1e-10) for the exact un-normalised rows e, after asserting that sum e^2 is an integer count of 1 / 16
    far below 2^24 (e is a multiple of 1 / 4 at most 3): exact in fp32 in any order."""
    e = np.asarray(e, np.float64)
    assert np.array_equal(e * 4, np.rint(e * 4)) and e.min() >= 0 and e.max() <= 3
    s = (e * e).sum(1)
    assert np.array_equal(s * 16, np.rint(s * 16)) and (s * 16).max() < 2 ** 20
    return e / (np.sqrt(s) + 1e-10)[:, None]


def within_normalize_bound(got, ref):
    """|got - ref| <= 4.5 x 2^-24 |ref| element-wise: the roundings of sqrt, of the add, of the reciprocal and of the product, 2^-24
    relative each (all four correctly rounded: the library is built without fast-math), plus second-order terms."""
    got = np.asarray(got, np.float64)
    return bool((np.abs(got - ref) <= 4.5 * U * np.abs(ref)).all())


def normalize_fp32_model(e):
    """k_row_normalize's four roundings in numpy's (correctly rounded) fp32."""
    e = np.asarray(e, np.float32)
    s = (e.astype(np.float64) ** 2).sum(1).astype(np.float32)               # exact, see normalize_ref
    inv = np.float32(1.0) / (np.sqrt(s) + np.float32(1e-10))
    return e * inv[:, None]


# ------------------------------------------------------------------------------- part 3: the Gram matrix
GRAM_N = [1, 2, 63, 64, 65, 130]
GRAM_DIM = [1, 15, 16, 17, 96, 100]
GRAM_CASES = [(n, d) for n in GRAM_N for d in (17, 96)] + [(65, d) for d in GRAM_DIM if d not in (17, 96)]


def gram_operand(n, dim):
    return np.random.default_rng(31 * n + dim).integers(-3, 4, size=(n, dim)).astype(np.float32)


def gram_ref(X, alpha=-2.0):
    """float64 alpha X X^T of integer X, after asserting that it is integer-valued and below 2^24."""
    assert alpha == -2.0
    ref = distances(X)
    assert ref.dtype == np.float64 and np.array_equal(ref, np.rint(ref))
    assert 2.0 * (np.abs(X.astype(np.float64)) @ np.abs(X.astype(np.float64)).T).max() < 2 ** 24
    ref.setflags(write=False)
    return ref


def gram_bound(X):
    """(dim + 2) 2^-24 x 2 sum_d |x_id x_jd|: the dot product of dim terms in any order, fused or not, plus the product with alpha."""
    A = np.abs(X.astype(np.float64))
    return (X.shape[1] + 2) * U * 2.0 * (A @ A.T)


def gram_last_ktile_dropped(X, alpha=-2.0):
    dim = X.shape[1]
    keep = (dim - 1) // 16 * 16
    Xk = X[:, :keep].astype(np.float64)
    return alpha * (Xk @ Xk.T)


def gram_edge_tile_shifted(X, alpha=-2.0):
    """The last row tile's rows written one row further down (its last row is lost, its first row keeps what was there: zero)."""
    n = X.shape[0]
    G = np.array(gram_ref(X, alpha))
    i0 = (n - 1) // 64 * 64
    out = G.copy()
    out[i0] = 0.0
    out[i0 + 1:] = G[i0:n - 1]
    return out


# ------------------------------------------------------------------------------- part 4: the retrieval statistics
STAT_KEYS = ("mean_ap", "hit_at_1", "hit_at_5")


def stats_case(n=130, dim=17):
    """Integer features (exact distances: ties are real ties), 12 video ids in 4 classes, two ids mapped to a negative class (skipped
    as queries, still ranked as items), two ids absent from the map (class 0), ten feature rows duplicated into items of other videos
    and classes, and one query -- the only item of the only video of class 3 -- without any positive."""
    rng = np.random.default_rng(2024)
    X = rng.integers(-3, 4, size=(n, dim)).astype(np.float32)
    ids = 500 + 3 * np.arange(12)
    vid = ids[rng.integers(0, 11, n)]                    # ids[11] is given to one item only, below
    id2class = {int(ids[0]): 0, int(ids[1]): 1, int(ids[2]): 2, int(ids[3]): 1, int(ids[4]): -1, int(ids[5]): 2,
                int(ids[6]): 0, int(ids[7]): -4, int(ids[8]): 1, int(ids[11]): 3}       # ids[9], ids[10]: absent -> class 0
    lonely = 77
    vid[lonely] = ids[11]
    cls = np.array([id2class.get(int(v), 0) for v in vid])
    done = 0
    for dst in range(n - 1, 0, -1):                      # duplicates: a low-index source copied to a high-index item of another video and class
        src = (7 * done + 3) % 40
        if done < 10 and dst != lonely and src != lonely and vid[src] != vid[dst] and cls[src] != cls[dst]:
            X[dst] = X[src]
            done += 1
    assert done == 10
    return X, vid.astype(np.int32), id2class, lonely


def stats_ref(X, vid, id2class, exclude, descending_ties=False):
    """The three float64 figures by the documented rule -- ascending (distance, index), the query removed whatever its distance -- or,
    descending_ties, the wrong model that breaks ties by descending index (the same ranking of the items in reversed order)."""
    assert np.array_equal(X, np.rint(X))
    d = distances(X)
    if descending_ties:
        d, vid = d[::-1, ::-1], vid[::-1]
    s = class_stats(d, vid, id2class, exclude)[0]
    return {k: float(s[k]) for k in STAT_KEYS}


def stats_query_ap(X, vid, id2class, exclude):
    """Every query's float64 average precision (NaN for a skipped query)."""
    return class_stats(distances(X), vid, id2class, exclude)[1]


def within_one_ulp(got, ref):
    """got (fp32, cast once from a double sum) within one fp32 ulp of the float64 figure."""
    return abs(float(got) - ref) <= float(np.spacing(np.float32(abs(ref))))
