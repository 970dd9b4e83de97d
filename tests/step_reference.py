"""The three steps of a Harmony iteration in float64.  TEST INFRASTRUCTURE: plain NumPy, no engine calls.

Every function takes exactly what the engine holds at the start of the step -- its fp32 arrays, widened -- in the
engine's public orientation (cells x PCs, cells x clusters, PCs x clusters) and evaluates the step in float64
throughout.  A test feeds each step the ENGINE's own input to it (Y from the R before the round, the new R from the
engine's Y of that round, Z_corr from the engine's R), so one kernel family's error never enters another's check.

  centroids  harmony.py:443-444            sweep  harmony.py:464-513 + the objective :394-417
  ridge      harmony.py:535-569

The oracle (oracle/harmony_oracle.py) states the same algorithm in the reference's fp32; tests/test_instance_grid_cpu.py
holds the two against each other.
"""
import numpy as np

F64 = np.float64


def device_perm_source(N, seed):
    """The engine's device-side update order as the permutation stream the oracle consumes
    (harmony.py:471): position p of round r holds the cell whose keyed-bijection position is p."""
    from oracle.device_order import positions
    state = {"counter": 0}

    def perm(n):
        assert n == N
        pos = positions(np.arange(N), N, seed, state["counter"])
        state["counter"] += 1
        return np.argsort(pos, kind="stable")
    return perm


def blocks_of(order, block_size):
    """harmony.py:474-484: the update order cut into ceil(1 / block_size) blocks, the last one takes the rest."""
    N = len(order)
    n_blocks = int(np.ceil(1.0 / block_size))
    per_block = int(N * block_size)
    return [order[b * per_block:(N if b == n_blocks - 1 else (b + 1) * per_block)] for b in range(n_blocks)]


def _one_hot(batch, B):
    phi = np.zeros((len(batch), B), F64)
    phi[np.arange(len(batch)), batch] = 1.0
    return phi


def centroids(Z_cos, R):
    """Unit columns of Z_cos^T . R (harmony.py:443-444): d x K."""
    Y = np.asarray(Z_cos, F64).T @ np.asarray(R, F64)
    return Y / np.sqrt((Y * Y).sum(axis=0))


def sweep(Z_cos, Y, R, batch, Pr_b, theta, sigma, blocks, scale=None):
    """update_R block by block (harmony.py:464-513) and the objective of the new state (:394-417).

    Z_cos N x d, Y d x K (this round's centroids), R N x K (before the sweep), batch: N batch codes of ONE batch
    variable, Pr_b / theta: B, sigma: K, blocks: index arrays in update order.  O and E at the start are those of R
    (O = R^T Phi, E = mass x Pr_b: what the engine carries in fp64).  Returns a dict: R (N x K), O (K x B), mass (K),
    dist / entropy / cross (the three sums of :399, :402, :411, not yet scaled by 2000 / N).  `scale` (N x K) replaces the softmax of
    :466-468 by one evaluated elsewhere (the anchors below); everything after it stays float64."""
    Z_cos, Y, R = np.asarray(Z_cos, F64), np.asarray(Y, F64), np.array(R, F64)
    Pr_b, theta, sigma = np.asarray(Pr_b, F64), np.asarray(theta, F64), np.asarray(sigma, F64)
    B = len(Pr_b)
    phi = _one_hot(batch, B)
    dist = 2.0 * (1.0 - Z_cos @ Y)                                      # N x K (:447)
    if scale is None:
        scale = np.exp(-dist / sigma[None, :])                          # :466-467
        scale /= scale.sum(axis=1, keepdims=True)                       # :468
    scale = np.asarray(scale, F64)
    O = R.T @ phi                                                       # K x B
    E = np.outer(R.sum(axis=0), Pr_b)
    for idx in blocks:
        R_b, phi_b = R[idx], phi[idx]
        E = E - np.outer(R_b.sum(axis=0), Pr_b)                         # :491
        O = O - R_b.T @ phi_b                                           # :492
        OE = np.maximum(O + E, 1e-8)                                    # :495-503
        ratio = np.clip(E / OE, 1e-8, 1.0)
        ratio_pow = ratio ** theta[None, :]
        R_new = scale[idx] * (phi_b @ ratio_pow.T)
        R_new /= np.maximum(R_new.sum(axis=1, keepdims=True), 1e-8)
        E = E + np.outer(R_new.sum(axis=0), Pr_b)                       # :506
        O = O + R_new.T @ phi_b                                         # :507
        R[idx] = R_new                                                  # :509
    with np.errstate(divide="ignore", invalid="ignore"):
        xlogx = R * np.log(R)
    xlogx[~np.isfinite(xlogx)] = 0.0                                    # :572-576
    O_c, E_c = np.maximum(O, 1e-8), np.maximum(E, 1e-8)                 # :407-408
    theta_log = theta[None, :] * np.log((O_c + E_c) / E_c)              # K x B (:409-410)
    return dict(R=R, O=O, mass=R.sum(axis=0),
                dist=float((R * dist).sum()), entropy=float((xlogx * sigma[None, :]).sum()),
                cross=float((R * sigma[None, :] * (phi @ theta_log.T)).sum()))


def ridge_weights(Z_orig, R, batch, lamb):
    """W (K x (B + 1) x d) of harmony.py:547-565 for one batch variable: per cluster the (B + 1)-square solve."""
    Z_orig, R, lamb = np.asarray(Z_orig, F64), np.asarray(R, F64), np.asarray(lamb, F64)
    K, B = R.shape[1], len(lamb) - 1
    mass = np.zeros((K, B), F64)
    rhs = np.zeros((K, B, Z_orig.shape[1]), F64)
    for b in range(B):
        idx = np.flatnonzero(batch == b)
        mass[:, b] = R[idx].sum(axis=0)
        rhs[:, b] = R[idx].T @ Z_orig[idx]
    W = np.zeros((K, B + 1, Z_orig.shape[1]), F64)
    for k in range(K):
        cov = np.diag(np.concatenate([[mass[k].sum()], mass[k]]) + lamb)            # Phi_moe diag(R_k) Phi_moe^T + diag(lamb) (:550)
        cov[0, 1:] = cov[1:, 0] = mass[k]
        W[k] = np.linalg.solve(cov, np.concatenate([rhs[k].sum(axis=0, keepdims=True), rhs[k]]))   # :553-563
    W[:, 0, :] = 0.0                                                                # :565
    return W


def ridge_apply(Z_orig, R, batch, W):
    """Z_corr = Z_orig - sum_k R_ik W_k[batch_i] (harmony.py:566) and its unit rows Z_cos (:569), in W's and R's type."""
    Z_corr = np.array(Z_orig, dtype=W.dtype)
    R = np.asarray(R, W.dtype)
    for b in range(W.shape[1] - 1):
        idx = np.flatnonzero(batch == b)
        Z_corr[idx] -= R[idx] @ W[:, b + 1, :]
    return Z_corr, Z_corr / np.sqrt((Z_corr * Z_corr).sum(axis=1, keepdims=True))


def ridge(Z_orig, R, batch, lamb):
    """moe_correct_ridge (harmony.py:535-569) with the fixed ridge penalties `lamb` (B + 1, the intercept's first):
    (Z_corr, Z_cos), both N x d."""
    return ridge_apply(np.asarray(Z_orig, F64), R, batch, ridge_weights(Z_orig, R, batch, lamb))


def errors(x, ref):
    """(relative Frobenius error, max-abs error over max |ref|) of x against the float64 reference."""
    x, ref = np.asarray(x, F64), np.asarray(ref, F64)
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref)), float(np.abs(x - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------------
# Anchors: the same steps in the arithmetic a kernel is DESIGNED to have, evaluated on the CPU.  A kernel's error against
# the float64 step is measured in units of its anchor's error (tests/test_instance_grid_gpu.py); a single product dropped
# from the six of the bf16 pipe moves the anchor by a known factor (tests/test_instance_grid_cpu.py).
# ---------------------------------------------------------------------------------------------------------------------
ANCHOR_CHUNK = 1024     # cells a workgroup of the R^T.Z pass accumulates in fp32 before its slab is summed in fp64


def _gemm_emulations():
    from test_split_gemm import SIX, bf16_mfma, f32_mfma, split3
    return SIX, bf16_mfma, f32_mfma, split3


def anchor_scale(Z_cos, Y, sigma, products="six"):
    """The softmax of the sweep (harmony.py:447, 466-468) as the kernels evaluate it: exp2 of the distance GEMM against
    the centroids scaled by c = 2 log2(e) / sigma, accumulated from -c in fp32 -- `products`: 'six' (the bf16 pipe: every
    operand as three bf16 terms), a list of (centroid term, cell term) pairs (a mutation), or None (the f32-input
    matrix instruction) -- normalised in fp32.  N x K, float32."""
    SIX, bf16_mfma, f32_mfma, _ = _gemm_emulations()
    Z = np.ascontiguousarray(Z_cos, np.float32)
    c = np.float32(2.0 * np.log2(np.e) / float(sigma[0]))
    assert np.all(np.asarray(sigma) == sigma[0])
    Ys = (np.ascontiguousarray(np.asarray(Y, np.float32).T) * c).astype(np.float32)      # K x d
    acc = f32_mfma(Z, Ys, c) if products is None else bf16_mfma(Z, Ys, c, SIX if products == "six" else products)
    r = np.exp2(acc.astype(np.float32))
    return (r / r.sum(axis=1, dtype=np.float32, keepdims=True)).astype(np.float32)


def anchor_rtz(R, Z, products="six"):
    """R^T . Z (K x d, float64) with the products of ANCHOR_CHUNK cells accumulated in fp32 the way the matrix
    instructions do (k-steps of 32 cells on the bf16 pipe, of 4 for f32 inputs; one rounding per instruction) and the
    chunks summed in float64."""
    SIX, _, _, split3 = _gemm_emulations()
    R, Z = np.asarray(R, np.float32), np.asarray(Z, np.float32)
    N, K, d = R.shape[0], R.shape[1], Z.shape[1]
    nch = -(-N // ANCHOR_CHUNK)
    Rp = np.zeros((nch * ANCHOR_CHUNK, K), np.float32); Rp[:N] = R
    Zp = np.zeros((nch * ANCHOR_CHUNK, d), np.float32); Zp[:N] = Z
    if products is None:
        step, terms = 4, [(Rp.reshape(nch, ANCHOR_CHUNK, K), Zp.reshape(nch, ANCHOR_CHUNK, d))]
    else:
        r = dict(zip("hml", (x.reshape(nch, ANCHOR_CHUNK, K) for x in split3(Rp))))
        z = dict(zip("hml", (x.reshape(nch, ANCHOR_CHUNK, d) for x in split3(Zp))))
        step, terms = 32, [(r[pr], z[pz]) for pr, pz in (_gemm_emulations()[0] if products == "six" else products)]
    acc = np.zeros((nch, K, d), np.float32)
    for s in range(0, ANCHOR_CHUNK, step):
        for a, b in terms:
            acc = (acc.astype(F64) + np.matmul(a[:, s:s + step].transpose(0, 2, 1).astype(F64), b[:, s:s + step].astype(F64))).astype(np.float32)
    return acc.astype(F64).sum(axis=0)


def anchor_centroids(Z_cos, R, products="six"):
    """centroids() from anchor_rtz: the fp64 sums rounded to fp32, normalised in fp32 (k_rtz3_finish).  d x K, float32."""
    Y = anchor_rtz(R, Z_cos, products).astype(np.float32).T
    return (Y / np.sqrt((Y * Y).sum(axis=0, dtype=np.float32), dtype=np.float32)).astype(np.float32)


def anchor_ridge(Z_orig, R, batch, lamb):
    """ridge() with W from the float64 solve rounded to fp32 and Z_orig - R . W, the row norms and the division evaluated
    in fp32 NumPy."""
    W = ridge_weights(Z_orig, R, batch, lamb).astype(np.float32)
    return ridge_apply(np.asarray(Z_orig, np.float32), np.asarray(R, np.float32), batch, W)
