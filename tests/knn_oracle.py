"""Float64 restatement of cross-set kNN label transfer (harmonypy_amd.knn_predict / knn_query) -- TEST INFRASTRUCTURE.

``knn_cross``: brute force over every (query, reference) pair, distances from direct differences (the square root, as
sklearn's ``kneighbors`` reports it), nearest first, ties by the smaller reference index.
``vote``: per query the category with the most votes among its neighbours' labels; tied categories go to the one whose
nearest member ranks first; the share is votes / k.
"""
import numpy as np


def knn_cross(Q, R, k, chunk=512):
    """Sorted distances and indices (n_q x k) of the k reference rows nearest to every query row."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    nq, nr = Q.shape[0], R.shape[0]
    if k > nr:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {nr}")
    dist = np.empty((nq, k))
    idx = np.empty((nq, k), dtype=np.int64)
    ref = np.arange(nr)
    for i in range(nq):
        diff = R - Q[i]
        dd = np.sqrt((diff * diff).sum(1))
        o = np.lexsort((ref, dd))[:k]
        dist[i] = dd[o]
        idx[i] = o
    return dist, idx


def vote(idx, codes):
    """(pred, prob) of every query row: idx n_q x k neighbour indices (nearest first), codes the reference's label codes."""
    nq, k = idx.shape
    pred = np.empty(nq, dtype=np.int64)
    prob = np.empty(nq, dtype=np.float64)
    for i in range(nq):
        lab = codes[idx[i]]
        best, best_n, best_rank = -1, 0, k
        for c in np.unique(lab):
            hit = np.flatnonzero(lab == c)
            n, first = hit.size, hit[0]
            if n > best_n or (n == best_n and first < best_rank):
                best, best_n, best_rank = c, n, first
        pred[i] = best
        prob[i] = best_n / k
    return pred, prob
