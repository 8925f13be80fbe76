"""A numpy-float32 restatement of vv_gallery_kmeans' arithmetic (include/videovec.h states it), for the tests.  Every sum is an explicit
serial chain in the order the header gives -- nothing here calls np.sum on floats.  scores_fn(centroids) -> d [n][C] float32 supplies
the distances, so the restatement can be fed exact host products (operands whose products are exact in any order) or the library's
own stored floats (Gallery.scores x -2 on a gallery made of the centroids).

step() is one pass: it returns the pass's assignment, counts, selected keys and objective; update() is one centroid update; run() is
the whole call and keeps every pass's values."""
import numpy as np

F32 = np.float32
CHUNK = 256          # csrc/vv_kmeans_plan.h: KM_CHUNK
SLOT = 64            # KM_SLOT_ROWS


def exact_scores(x):
    """scores_fn for operands whose dot products are exact in float32 whatever the order (small integers): d = -2 x . c, -0 as +0."""
    x64 = np.asarray(x, np.float64)

    def fn(cent):
        d = (-2.0 * (x64 @ np.asarray(cent, np.float64).T)).astype(F32)
        return d + F32(0.0)
    return fn


def chain_sq(rows):
    """rows [m][dim] float32 -> [m]: the serial chain of row[col]^2 in ascending column from +0, product and sum rounded apart."""
    rows = np.asarray(rows, F32)
    q = np.zeros(rows.shape[0], F32)
    for col in range(rows.shape[1]):
        q = (q + (rows[:, col] * rows[:, col]).astype(F32)).astype(F32)
    return q


def keys_of(d, cent, metric):
    d = np.asarray(d, F32)
    if metric == "spherical":
        return d
    return (d + chain_sq(cent)[None, :]).astype(F32)


def assign_of(key):
    """The cluster of the smallest (key, c) of every row, a NaN key never selected; a row of NaN: cluster 0."""
    valid = ~np.isnan(key)
    kk = np.where(valid, key, np.inf).astype(F32)
    m = kk.min(axis=1)
    return np.argmax(valid & (kk == m[:, None]), axis=1).astype(np.int32)


def objective_of(sel):
    """Slots of 64 consecutive items folded by x[i] += x[i + o], o = 32 .. 1 (absent items +0.0), then added in ascending slot from +0.0."""
    n = len(sel)
    v = np.zeros((n + SLOT - 1) // SLOT * SLOT, np.float64)
    v[:n] = np.asarray(sel, np.float64)
    v = v.reshape(-1, SLOT)
    o = SLOT // 2
    while o >= 1:
        v[:, :o] = v[:, :o] + v[:, o:2 * o]
        o //= 2
    acc = 0.0
    for s in v[:, 0]:
        acc = acc + float(s)
    return acc


def step(d, cent, metric, prev_assign):
    key = keys_of(d, cent, metric)
    a = assign_of(key)
    sel = key[np.arange(len(a)), a]
    counts = np.bincount(a, minlength=cent.shape[0]).astype(np.int32)
    moved = len(a) if prev_assign is None else int((a != prev_assign).sum())
    nonfinite = int((~np.isfinite(sel)).sum())
    return dict(assign=a, counts=counts, moved=moved, objective=objective_of(sel), sel=sel, nonfinite=nonfinite)


def cluster_sum(x, items):
    """items ascending: chunks of 256 list entries, each a serial chain from its first row; the partials added in ascending chunk order
    from the first."""
    s = None
    for b in range(0, len(items), CHUNK):
        rows = x[items[b:b + CHUNK]]
        acc = rows[0].copy()
        for r in rows[1:]:
            acc = (acc + r).astype(F32)
        s = acc if s is None else (s + acc).astype(F32)
    return s


def update(x, a, cent, metric):
    """-> (new centroids, empty, degenerate)"""
    x = np.asarray(x, F32)
    new = np.array(cent, F32, copy=True)
    empty = degenerate = 0
    order = np.argsort(a, kind="stable")
    counts = np.bincount(a, minlength=cent.shape[0])
    starts = np.concatenate([[0], np.cumsum(counts)])
    for c in range(cent.shape[0]):
        if counts[c] == 0:
            empty += 1
            continue
        s = cluster_sum(x, order[starts[c]:starts[c + 1]])
        if metric == "spherical":
            q = chain_sq(s[None, :])[0]
            if q == 0 or not np.isfinite(q):
                degenerate += 1
                continue
            new[c] = (s / np.sqrt(q, dtype=F32)).astype(F32)
        else:
            inv = F32(1.0) / F32(counts[c])
            new[c] = (s * inv).astype(F32)
    return new, empty, degenerate


def run(x, cent0, iters, metric, scores_fn):
    """-> dict(passes=[step dicts, each with the `centroids` it was assigned against], centroids, empty_last, degenerate_last)"""
    x = np.asarray(x, F32)
    cent = np.array(cent0, F32, copy=True)
    prev, passes = None, []
    empty = degenerate = 0
    for t in range(iters + 1):
        st = step(scores_fn(cent), cent, metric, prev)
        st["centroids"] = cent.copy()
        passes.append(st)
        prev = st["assign"]
        if t == iters:
            break
        cent, empty, degenerate = update(x, prev, cent, metric)
    return dict(passes=passes, centroids=cent, empty_last=empty, degenerate_last=degenerate)
