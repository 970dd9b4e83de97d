/* hmx_map.h -- reference mapping in libhmx.so: new query cells are placed onto a finished Harmony reference without a new
 * run on the union, as in Symphony (Kang et al., Nat. Commun. 12, 5890, 2021).  The reference is compressed into
 * per-cluster sums (K x (d + 1) numbers); the query is soft-assigned to the reference's corrected-space centroids and
 * moved by one mixture-of-experts ridge step whose intercept carries the reference's mass, so the query moves and the
 * reference does not.  Part of the same C ABI as hmx.h (HMX_ABI_VERSION 8: added symbols only), kept in its own header so
 * that hmx.h's declared set stays what its C clients were written against.  Line numbers cite harmonypy's harmony.py.
 */
#ifndef HMX_MAP_H
#define HMX_MAP_H

#include "hmx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference summary of a clustered engine (hmx_init_cluster has run; normally a finished harmonize() loop), from its
 * current soft assignment R and corrected embedding Z_corr (after the last ridge, harmony.py:566):
 *     cluster_mass_out[k]          = sum_i R[k,i]                 (K, the O of harmony.py:550 summed over batches)
 *     cluster_sums_out[k * d + j]  = sum_i R[k,i] Z_corr[j,i]     (K x d row-major, the right-hand side of :556-559
 *                                                                  with Z_corr in place of Z_orig)
 * One R^T.Z pass over the cells (the ridge's statistics kernels fed Z_corr), per batch group tables summed in float64 on
 * the host.  In a sharded job every rank receives the sums over all ranks (a collective: every rank must call).  The
 * engine's state is unchanged: later hmx_cluster / hmx_moe_correct_ridge calls give what they would have given. */
int hmx_reference_summary(hmx_engine* e, double* cluster_sums_out, double* cluster_mass_out);

/* Map the uploaded query (hmx_upload / hmx_upload_device: the query's cells, batch design, lamb and the reference's sigma;
 * theta is not used) onto a reference given by its summary (K x d sums, K masses, as hmx_reference_summary writes them):
 *   1. centroids Y[k] = cluster_sums[k] / |cluster_sums[k]| (rounded to fp32 first; harmony.py:377, k_y_normalize);
 *   2. R[k,j] = exp(-2 (1 - Y[k] . x_j / |x_j|) / sigma_k), normalised over k -- the init assignment of harmony.py:379-389
 *      (no diversity penalty), which also sets O and E; the engine is clustered afterwards;
 *   3. the ridge statistics of the query over Z_orig (harmony.py:547-563);
 *   4. per cluster the ridge solve of harmony.py:550-565 with the reference in the intercept row:
 *          A_k = Phi_k Phi^T + diag(lambda) + cluster_mass[k] e0 e0^T,   b_k = Phi_k X^T + e0 cluster_sums[k],
 *          W_k = A_k^-1 b_k,  W_k[0,:] = 0;
 *   5. Z_corr = Z_orig - sum_k W_k^T Phi_k (:566) and Z_cos (:569).
 * With lambda estimation (hmx_config.lambda_estimation) lambda comes from the query's own E.  The reference terms hold
 * for this call only: a later hmx_moe_correct_ridge is the plain Harmony ridge.  HMX_ERR_ARG for null pointers,
 * non-finite terms or a zero row of cluster_sums; HMX_ERR_STATE before an upload. */
int hmx_map_query(hmx_engine* e, const double* cluster_sums, const double* cluster_mass);

#ifdef __cplusplus
}
#endif
#endif /* HMX_MAP_H */
