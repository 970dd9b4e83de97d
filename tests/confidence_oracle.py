"""Float64 NumPy restatement of the mapping-confidence scores (Symphony's per-cell and per-cluster mapping metrics,
Kang et al., Nat. Commun. 12, 5890, 2021), the yardstick of ``ClusterMoments`` / ``mapping_score`` /
``cluster_mapping_score``.  Dense and direct: one cluster at a time, ``np.linalg.cholesky`` and ``np.linalg.solve``
on the differences themselves -- no whitening matrices, no tiling, no shared code with the library.

Cells are rows here (N x d, N x K), as the Python interface hands them out.
"""
import numpy as np


def code_weights(codes, n_groups):
    """Hard group codes (N ints in [0, n_groups)) as a G x N matrix of 0 / 1 weights."""
    codes = np.asarray(codes)
    W = np.zeros((n_groups, codes.shape[0]))
    W[codes, np.arange(codes.shape[0])] = 1.0
    return W


def cluster_moments(W, Z):
    """(mass G, mass_sq G, mean G x d, cov G x d x d) of the cells Z (N x d) under the weights W (G x N): the unbiased
    weighted covariance, centred before it is squared.  A group without mass has NaN mean and covariance."""
    W = np.asarray(W, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    G, d = W.shape[0], Z.shape[1]
    mass = W.sum(axis=1)
    mass_sq = (W * W).sum(axis=1)
    mean = np.full((G, d), np.nan)
    cov = np.full((G, d, d), np.nan)
    for g in range(G):
        if not mass[g] > 0:
            continue
        mean[g] = (W[g] @ Z) / mass[g]
        C = Z - mean[g]
        with np.errstate(divide="ignore", invalid="ignore"):
            cov[g] = (C.T * W[g]) @ C / mass[g] / (1.0 - mass_sq[g] / mass[g] ** 2)
    return mass, mass_sq, mean, cov


def regularised(cov, ridge):
    """cov + ridge * (tr cov / d) * I."""
    d = cov.shape[0]
    return cov + ridge * (np.trace(cov) / d) * np.eye(d)


def cholesky_or_none(A):
    """The lower Cholesky factor of A, or None when A is not finite or a pivot is not positive."""
    if not np.all(np.isfinite(A)):
        return None
    try:
        return np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None


def invalid_clusters(cov, ridge=0.0):
    """Indices of the covariances whose regularised Cholesky factorisation fails."""
    return [k for k in range(cov.shape[0]) if cholesky_or_none(regularised(cov[k], ridge)) is None]


def distances(X, mean, cov, ridge=0.0):
    """D[k, j] = sqrt((x_j - mean_k)^T (cov_k + ridge tr(cov_k)/d I)^-1 (x_j - mean_k)); a row of NaN for an invalid k."""
    X = np.asarray(X, dtype=np.float64)
    K = mean.shape[0]
    D = np.full((K, X.shape[0]), np.nan)
    for k in range(K):
        L = cholesky_or_none(regularised(cov[k], ridge))
        if L is None:
            continue
        y = np.linalg.solve(L, (X - mean[k]).T)            # d x N: L y = delta
        D[k] = np.sqrt((y * y).sum(axis=0))
    return D


def per_cell_score(Rq, X, mean, cov, ridge=0.0):
    """score[j] = sum_k Rq[j, k] D[k, j] (Rq: N x K)."""
    bad = invalid_clusters(cov, ridge)
    if bad:
        raise ValueError(f"invalid clusters {bad}")
    return (np.asarray(Rq, dtype=np.float64).T * distances(X, mean, cov, ridge)).sum(axis=0)


def per_cluster_score(Rq, X, codes, n_groups, ref_mean, ridge=0.0, min_cells_per_dim=2):
    """(n_cells G, score G): the reference's cluster means measured in each query group's own covariance, weighted by
    the group's mean soft assignment.  NaN for a group of fewer than min_cells_per_dim * d cells or an invalid one."""
    Rq = np.asarray(Rq, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    codes = np.asarray(codes)
    d = X.shape[1]
    n = np.bincount(codes, minlength=n_groups)[:n_groups]
    score = np.full(n_groups, np.nan)
    for g in range(n_groups):
        if n[g] < min_cells_per_dim * d or n[g] < 2:
            continue
        Xg = X[codes == g]
        mq = Xg.mean(axis=0)
        cq = np.cov(Xg.T, ddof=1).reshape(d, d)
        L = cholesky_or_none(regularised(cq, ridge))
        if L is None:
            continue
        y = np.linalg.solve(L, (ref_mean - mq).T)          # d x K
        rbar = Rq[codes == g].mean(axis=0)
        score[g] = float(rbar @ np.sqrt((y * y).sum(axis=0)))
    return n, score
