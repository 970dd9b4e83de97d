"""The data sets of the mapping-confidence tests, shared by the CPU conditioning checks (test_confidence_cpu.py) and the
GPU accuracy tests (test_confidence_gpu.py), and the conditioning measure itself."""
import numpy as np
import pandas as pd

import confidence_oracle as CO

# name -> (reference cells, query cells, PCs, clusters, batches, seed)
SYNTHETIC = {
    "c3": (20000, 20000, 50, 100, 8, 11),        # the C3 shape of the benchmark: 50 PCs, K = 100
    "wide": (12000, 3000, 20, 120, 3, 5),        # K > 112: the wide kernels of the engine
    "d100": (6000, 3000, 100, 30, 4, 7),         # more than 64 PCs
    "d10": (3000, 1000, 10, 12, 2, 13),          # at most 16 PCs: the one-tile instances of the tuned kernels
    "d40": (8000, 2000, 40, 40, 3, 17),          # 33..48 PCs: the three-tile instances
}


def synthetic(name):
    """(Z_ref, meta_ref, X_q, meta_q, centres K x d): K anisotropic Gaussian clusters around random centres, every batch
    shifted a little; float32 as a user would pass them."""
    N_ref, N_q, d, K, B, seed = SYNTHETIC[name]
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, d)) * 3
    scale = 0.3 * (0.5 + rng.random(size=(K, d)))              # per-cluster, per-axis spread: no two axes alike
    shift = rng.normal(size=(B, d)) * 0.15

    def draw(n):
        lab = rng.integers(0, K, size=n)
        b = rng.integers(0, B, size=n)
        X = centres[lab] + rng.normal(size=(n, d)) * scale[lab] + shift[b]
        return X.astype(np.float32), pd.DataFrame({"batch": [f"b{i}" for i in b]})
    Zr, mr = draw(N_ref)
    Xq, mq = draw(N_q)
    return Zr, mr, Xq, mq, centres


def soft_assignment(X, centres, sigma=0.1):
    """cells x K: the engine's initial assignment formula on unit-length rows (a CPU stand-in for a finished run's R)."""
    Xc = X / np.linalg.norm(X, axis=1, keepdims=True)
    Y = centres / np.linalg.norm(centres, axis=1, keepdims=True)
    R = np.exp(-2.0 * (1.0 - Xc @ Y.T) / sigma)
    return R / R.sum(axis=1, keepdims=True)


def conditioning(R_ref, Z_ref, R_q, X_q, ridge=0.0):
    """(invalid reference clusters, largest relative difference of the per-cell scores between the oracle run on the
    cells as given and on the cells in reversed order -- reference and query both).  Small means the inputs themselves
    leave no room for disagreement beyond the summation order."""
    R_ref, Z_ref = np.asarray(R_ref, np.float64), np.asarray(Z_ref, np.float64)
    R_q, X_q = np.asarray(R_q, np.float64), np.asarray(X_q, np.float64)
    _, _, mean, cov = CO.cluster_moments(R_ref.T, Z_ref)
    invalid = CO.invalid_clusters(cov, ridge)
    if invalid:
        return invalid, np.inf
    fwd = CO.per_cell_score(R_q, X_q, mean, cov, ridge)
    _, _, mean_r, cov_r = CO.cluster_moments(R_ref[::-1].T, Z_ref[::-1])
    if CO.invalid_clusters(cov_r, ridge):
        return invalid, np.inf
    rev = CO.per_cell_score(R_q[::-1], X_q[::-1], mean_r, cov_r, ridge)[::-1]
    return invalid, float(np.max(np.abs(fwd - rev) / np.abs(fwd)))


def gaussian_reference(d=20, K=6, n_per=1500, n_query_per=400, n_novel=300, seed=3):
    """A reference of K Gaussian clusters with known covariances, far apart; a query of fresh draws from the same
    clusters (labels 0..K-1) and a population the reference does not contain (label K), many within-cluster standard
    deviations from every reference cluster.  (Z_ref, labels_ref, X_q, labels_q)."""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(K + 1, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    centres = dirs * 30.0                                        # centres 30 apart from the origin, ~40 from each other
    A = [np.linalg.qr(rng.normal(size=(d, d)))[0] * (0.6 + 0.8 * rng.random(d)) for _ in range(K + 1)]   # sd 0.6 .. 1.4

    def draw(k, n):
        return centres[k] + rng.normal(size=(n, d)) @ A[k].T
    Zr = np.concatenate([draw(k, n_per) for k in range(K)])
    lr = np.repeat(np.arange(K), n_per)
    Xq = np.concatenate([draw(k, n_query_per) for k in range(K)] + [draw(K, n_novel)])
    lq = np.concatenate([np.repeat(np.arange(K), n_query_per), np.full(n_novel, K)])
    pr, pq = rng.permutation(len(lr)), rng.permutation(len(lq))
    return Zr[pr].astype(np.float32), lr[pr], Xq[pq].astype(np.float32), lq[pq]
