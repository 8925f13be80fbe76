"""Numpy restatement of the nearest-neighbour lists of vv_gallery_nearest / vv_gallery_nearest_self for the tests: given the
distances, who is eligible and k, every row's eligible items in ascending (distance, gallery index), cut at k and padded with
index -1 / distance 0.  Also the exact inputs the GPU tests use: small integers, so that every float32 dot product is exact in
any summation order and lists can be compared bit for bit."""
import numpy as np


def distances32(Q, G):
    """-2 Q G^T in float32, -0 folded into +0 as the similarity kernel stores it."""
    return np.float32(-2.0) * (Q.astype(np.float32) @ G.astype(np.float32).T) + np.float32(0.0)


def nearest(d, eligible, k):
    """d [n_q][n_ref]; eligible: bool [n_q][n_ref] or None (everything).  Returns (idx int32 [n_q][k], dist d.dtype [n_q][k])."""
    nq, ng = d.shape
    idx = np.full((nq, k), -1, np.int32)
    dist = np.zeros((nq, k), d.dtype)
    every = np.arange(ng)
    for i in range(nq):
        g = every if eligible is None else np.flatnonzero(eligible[i])
        g = g[np.lexsort((g, d[i, g]))][:k]
        idx[i, :len(g)] = g
        dist[i, :len(g)] = d[i, g]
    return idx, dist


def nearest_brute_force(d, eligible, k):
    """The same by a plain Python loop: sorted() over (distance, index) tuples."""
    nq, ng = d.shape
    idx = np.full((nq, k), -1, np.int32)
    dist = np.zeros((nq, k), d.dtype)
    for i in range(nq):
        pairs = sorted((d[i, g], g) for g in range(ng) if eligible is None or eligible[i, g])[:k]
        for j, (v, g) in enumerate(pairs):
            idx[i, j], dist[i, j] = g, v
    return idx, dist


def exact_input(nq, ng, nid, seed, dim=40):
    """Integer features in [-3, 3]: |dot| <= 9 dim, every float32 distance exact.  Returns Q, q_ids, G, g_ids."""
    rng = np.random.default_rng(seed)
    G = rng.integers(-3, 4, (ng, dim)).astype(np.float32)
    Q = rng.integers(-3, 4, (nq, dim)).astype(np.float32)
    gid = rng.integers(0, nid, ng).astype(np.int32)
    qid = rng.integers(0, nid, nq).astype(np.int32)
    return Q, qid, G, gid


def one_id_owns_all_but(gid, big_id, keep, seed):
    """ids in which `big_id` owns every item except `keep` of them, which retain their id of gid."""
    rng = np.random.default_rng(seed)
    out = np.full_like(gid, big_id)
    rest = rng.permutation(len(gid))[:keep]
    out[rest] = gid[rest]
    return out
