"""Float64 NumPy restatement of reference mapping (harmonypy_amd.map_query, include/hmx_map.h): the checker of the tests.

Written in harmonypy's orientation (cells are columns: Z is d x N, R is K x N, Phi is B x N) with a dense
``np.linalg.solve`` per cluster, not the arrowhead elimination the solve kernels use.  Line numbers cite harmonypy's
harmony.py.
"""
import numpy as np

F64 = np.float64


def reference_summary(R, Z_corr):
    """R (K x N), Z_corr (d x N) -> (cluster_sums K x d, cluster_mass K)."""
    R = np.asarray(R, F64)
    return R @ np.asarray(Z_corr, F64).T, R.sum(axis=1)


def centroids(cluster_sums):
    """The reference's clusters in the corrected space, unit rows (K x d)."""
    S = np.asarray(cluster_sums, F64)
    return S / np.linalg.norm(S, axis=1, keepdims=True)


def assign(X, Y, sigma):
    """harmony.py:379-386 with the centroids Y (K x d): R (K x N) of the query X (d x N); no diversity penalty."""
    X = np.asarray(X, F64)
    Xh = X / np.linalg.norm(X, axis=0, keepdims=True)                 # :238
    dist = 2.0 * (1.0 - np.asarray(Y, F64) @ Xh)                       # :380
    R = np.exp(-dist / np.asarray(sigma, F64)[:, None])                # :383-384
    return R / R.sum(axis=0, keepdims=True)                            # :385


def lambdas(R, Pr_b, lamb, lambda_estimation, alpha):
    """K x (B+1) ridge penalties: ``lamb`` for every cluster, or harmony.py:587-591 from E = T (x) Pr_b."""
    K = R.shape[0]
    if not lambda_estimation:
        return np.tile(np.asarray(lamb, F64), (K, 1))
    E = np.outer(R.sum(axis=1), np.asarray(Pr_b, F64))                 # :388
    return np.concatenate([np.zeros((K, 1)), alpha * E], axis=1)


def correct(X, R, Phi, lam, cluster_sums=None, cluster_mass=None):
    """harmony.py:535-569 with the reference in the intercept: X (d x N), R (K x N), Phi (B x N), lam (K x (B+1)).
    Returns (X_corr, X_cos, W K x (B+1) x d).  Zero / None reference terms: the plain ridge."""
    X = np.asarray(X, F64)
    R = np.asarray(R, F64)
    K, N = R.shape
    Phi_moe = np.concatenate([np.ones((1, N)), np.asarray(Phi, F64)], axis=0)     # :255-256
    X_corr = X.copy()
    W_all = np.zeros((K, Phi_moe.shape[0], X.shape[0]))
    for k in range(K):
        Phi_k = Phi_moe * R[k]                                          # :547
        A = Phi_k @ Phi_moe.T + np.diag(lam[k])                         # :550
        b = Phi_k @ X.T                                                 # :556-563
        if cluster_mass is not None:
            A[0, 0] += cluster_mass[k]
            b[0] += cluster_sums[k]
        W = np.linalg.solve(A, b)
        W[0, :] = 0                                                     # :565
        W_all[k] = W
        X_corr -= W.T @ Phi_k                                           # :566
    return X_corr, X_corr / np.linalg.norm(X_corr, axis=0, keepdims=True), W_all   # :569


def map_query(X, Phi, Pr_b, cluster_sums, cluster_mass, sigma, lamb, lambda_estimation=False, alpha=0.2):
    """The whole mapping of a query X (d x N) with batch design Phi (B x N): (R, X_corr, X_cos)."""
    R = assign(X, centroids(cluster_sums), sigma)
    lam = lambdas(R, Pr_b, lamb, lambda_estimation, alpha)
    X_corr, X_cos, _ = correct(X, R, Phi, lam, np.asarray(cluster_sums, F64), np.asarray(cluster_mass, F64))
    return R, X_corr, X_cos


def arrowhead_v1(S, O, lam, ref_sum, ref_mass):
    """What k_ridge_solve_v1 evaluates for one cluster and one batch variable: S (B x d) per-batch sums, O (B) per-batch
    masses, lam (B+1).  Returns W ((B+1) x d) with row 0 zero."""
    c = lam[1:] / (O + lam[1:])
    w0 = (c @ S + ref_sum) / (lam[0] + ref_mass + c @ O)
    W = np.zeros((len(O) + 1, S.shape[1]))
    W[1:] = (S - O[:, None] * w0[None, :]) / (O + lam[1:])[:, None]
    return W


def general_system(S_g, O_g, group_cols, B, lam, ref_sum, ref_mass):
    """The augmented system k_ridge_solve_general assembles from group tables (S_g G x d, O_g G, group_cols G x V) with
    the reference terms; solved densely here.  Returns W ((B+1) x d) with row 0 zero."""
    n = B + 1
    d = S_g.shape[1]
    M = np.zeros((n, n))
    rhs = np.zeros((n, d))
    for g in range(len(O_g)):
        rows = [0] + [int(c) + 1 for c in group_cols[g]]
        for a in rows:
            rhs[a] += S_g[g]
            for b in rows:
                M[a, b] += O_g[g]
    M[0, 0] += ref_mass
    rhs[0] += ref_sum
    M += np.diag(lam)
    W = np.linalg.solve(M, rhs)
    W[0] = 0
    return W
