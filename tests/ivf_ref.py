"""A numpy restatement of vv_ivf_search (include/videovec.h states it), for the tests.  It computes NO dot product of its own: d_items
[n_q][n_ref] and d_cent [n_q][C] are the stored floats (Gallery.scores(q) x -2 on the items, the same on a gallery made of the
centroids), nn [C] comes from kmeans_ref.chain_sq, and the lists are given (start [C + 1], lst [n_ref]).  From these it derives the
probe order, every query's candidate set and count, the k smallest (d, g), and the tile and candidate totals the index reports."""
import numpy as np

F32 = np.float32
TILE = 128           # csrc/vv_ivf_plan.h: IVF_TILE


def lists_of(assign, C):
    """(start, lst): every cluster's items in ascending item index -- a stable sort of the items by cluster."""
    assign = np.asarray(assign, np.int64)
    lst = np.argsort(assign, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=C))]).astype(np.int32)
    return start, lst


def probe_keys(d_cent, nn, metric):
    d = np.asarray(d_cent, F32)
    if metric == "spherical":
        return d
    return (d + np.asarray(nn, F32)[None, :]).astype(F32)


def probe_order(key_row, nprobe):
    """The nprobe smallest (key, c) ascending, lowest cluster at a tie, -0 == +0; NaN keys below nothing: the slots left take the lowest
    unused clusters.  nprobe == C: every cluster in ascending index."""
    C = len(key_row)
    if nprobe == C:
        return list(range(C))
    num = [c for c in range(C) if not np.isnan(key_row[c])]
    num.sort(key=lambda c: (float(key_row[c]) + 0.0, c))
    chosen = num[:nprobe]
    if len(chosen) < nprobe:
        chosen += [c for c in range(C) if np.isnan(key_row[c])][:nprobe - len(chosen)]
    return chosen


def search(d_items, d_cent, nn, metric, start, lst, nprobe, k, block_rows=None):
    """-> dict(idx [n_q][k], dist [n_q][k], n_candidates [n_q], probes (list of lists), tiles, candidates).  block_rows: the query rows of
    one block (None: all in one) -- tiles are counted per block, as the index lists them."""
    d_items, start, lst = np.asarray(d_items, F32), np.asarray(start, np.int64), np.asarray(lst, np.int64)
    n_q, C = d_items.shape[0], len(start) - 1
    key = probe_keys(d_cent, nn, metric)
    idx = np.full((n_q, k), -1, np.int32)
    dist = np.zeros((n_q, k), F32)
    m = np.zeros(n_q, np.int32)
    probes = []
    for i in range(n_q):
        pr = probe_order(key[i], nprobe)
        probes.append(pr)
        cand = np.concatenate([lst[start[c]:start[c + 1]] for c in pr]) if pr else np.zeros(0, np.int64)
        m[i] = len(cand)
        dd = d_items[i, cand]
        # ascending (d, g): d compared as floats after -0 -> +0 (the stored floats carry no -0), g the item index
        order = np.lexsort((cand, dd))[:k]
        idx[i, :len(order)] = cand[order]
        dist[i, :len(order)] = dd[order]
    rows = n_q if block_rows is None else block_rows
    tiles = 0
    for b0 in range(0, n_q, rows):
        per = np.zeros(C, np.int64)
        for pr in probes[b0:b0 + rows]:
            per[pr] += 1
        size = start[1:] - start[:-1]
        tiles += int((-(-per // TILE) * -(-size // TILE))[(per > 0) & (size > 0)].sum())
    return dict(idx=idx, dist=dist, n_candidates=m, probes=probes, tiles=tiles, candidates=int(m.sum()))


def recall(idx, exact_idx, at):
    """The share of the exact lists' first `at` items found in idx's first `at`, over all queries."""
    hit = sum(len(set(a[:at].tolist()) & set(b[:at].tolist())) for a, b in zip(idx, exact_idx))
    return hit / float(len(idx) * at)
