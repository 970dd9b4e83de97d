/* hmx_score.h -- mapping confidence in libhmx.so: second moments of an engine's cells per soft cluster (or per hard
 * group) and the per-cell Mahalanobis mapping score of a mapped query, as Symphony's mapping metrics (Kang et al., Nat.
 * Commun. 12, 5890, 2021).  Part of the same C ABI as hmx.h (HMX_ABI_VERSION 8: added symbols only), kept in its own
 * header so that the declared set of the earlier headers stays what their C clients were written against.
 */
#ifndef HMX_SCORE_H
#define HMX_SCORE_H

#include "hmx_device_io.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weighted moments of the cells of a clustered engine (a finished Harmony run or a mapped query) in the embedding which_Z
 * (HMX_Z_ORIG or HMX_Z_CORR), z_i = the fp32 row of cell i converted to float64 exactly:
 *     mass[g]    = sum_i w[g,i]                        mass_sq[g] = sum_i w[g,i]^2
 *     mean[g]    = sum_i w[g,i] z_i / mass[g]          (n_groups x d, row-major)
 *     cov[g]     = sum_i w[g,i] (z_i - mean[g]) (z_i - mean[g])^T / mass[g] / (1 - mass_sq[g] / mass[g]^2)
 *                                                      (n_groups x d x d, row-major, exactly symmetric)
 * codes == NULL: w is the engine's soft assignment R and n_groups must be n_clusters.  Otherwise codes holds n_cells
 * group codes in [0, n_groups), n_groups in [1, 4096], in the CALLER's cell order (the order of the upload) and
 * w[g,i] = [codes[i] == g].  All sums are float64 and the second moments are accumulated about mean[g] (two passes over
 * the cells), in a summation order that depends on the shapes only.  A group without mass gets NaN mean and covariance; a
 * group whose unbiased normalisation is 0 / 0 (one cell) a NaN covariance.  All outputs are HOST arrays.
 * Cost and memory: transient device buffers of up to 64 + 256 MiB for the per-chunk partial sums, plus the covariance
 * tiles, n_groups * dt * (dt + 1) / 2 * 2 KiB with dt = ceil(n_pcs / 16), held once more on the device and once on the host;
 * that figure may not exceed 1 GiB (HMX_ERR_ARG: e.g. 4096 groups up to 240 PCs, 2496 groups at 320).  With codes every
 * group reads all n_cells codes (the products of other groups' cells are skipped), so the second pass costs about
 * n_groups * n_cells code reads on top of one pass over the cells' rows: meant for hundreds of groups, not for one per cell.
 * The engine's state is not touched: later hmx_cluster / hmx_moe_correct_ridge calls give bit for bit what they would have
 * given.  HMX_ERR_STATE before an upload, before clustering, and on an engine that is one shard of a sharded job. */
int hmx_cluster_moments(hmx_engine* e, int which_Z, const int32_t* codes, int32_t n_groups,
                        double* mass, double* mass_sq, double* mean, double* cov);

/* The per-cell mapping score of a clustered engine's cells against per-cluster whitening transforms:
 *     score[j] = sum_k R[k,j] * || T_k x_j - t_k ||_2 ,      x_j = cell j's row of which_Z (HMX_Z_ORIG or HMX_Z_CORR)
 * whitening: n_clusters x d x d float64, row-major, T_k LOWER triangular (the inverse of the Cholesky factor of the
 * cluster's regularised covariance; entries above the diagonal are not read); offsets: n_clusters x d, t_k = T_k mean_k.
 * Both HOST arrays, all entries finite.  The distance is the root of a sum of squares of float64 differences; the quadratic
 * form is never expanded.  score_host (HOST, n_cells float64) or score_device (DEVICE memory of the engine's GPU, n_cells
 * contiguous float64), exactly one of them non-null, receives the scores in the CALLER's cell order; with score_device the
 * work is ordered behind what was queued on stream (the caller's hipStream_t, NULL = the null stream), and later work on
 * that stream sees the result.  The call returns once the scores are written.  The engine's state is not touched.
 * HMX_ERR_STATE as for hmx_cluster_moments, and when the upload's source_row was not a permutation of the cells. */
int hmx_mapping_score(hmx_engine* e, int which_Z, const double* whitening, const double* offsets,
                      double* score_host, void* score_device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMX_SCORE_H */
