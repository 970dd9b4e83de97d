/* hmx_knn.h -- label transfer in libhmx.so: the exact k nearest reference cells of every query cell, and a majority vote
 * on the reference's labels, as Symphony's knnPredict does after mapQuery (Kang et al., Nat. Commun. 12, 5890, 2021).
 * Part of the same C ABI as hmx.h (HMX_ABI_VERSION 8: added symbols only), kept in its own header so that hmx.h's declared
 * set stays what its C clients were written against.
 */
#ifndef HMX_KNN_H
#define HMX_KNN_H

#include "hmx_device_io.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cross-set kNN and vote on GPU device_id.  Q (n_q query cells) and R (n_r reference cells, n_r < 2^31 - 256) are DEVICE
 * matrices of that GPU with the same d features, d in [1, HMX_MAX_PCS], of type q_dtype / r_dtype (HMX_DTYPE_*): element
 * (cell i, feature c) at Q + i * q_stride_cell + c * q_stride_col, strides in elements, any non-negative values.  Every
 * element is converted to float64 exactly.
 *
 * Neighbours: for every query cell the k reference cells nearest in Euclidean distance, nearest first, ties by the
 * smaller reference index; the distance itself (the square root) of float64 direct differences.  1 <= k <= n_r and
 * k <= 2040 (the candidate lists hold 256 / 1024 / 4096 entries for k <= 120 / 504 / 2040).
 *
 * Vote, per label column L: ref_label_codes (HOST, n_labels x n_r, row-major, codes in [0, 2^31)) gives every reference
 * cell a category; pred_out[i * n_labels + L] is the category with the most votes among query i's k neighbours and
 * prob_out[i * n_labels + L] its votes / k.  Tied categories go to the one whose nearest member ranks first.
 *
 * slices: how many parts the reference is cut into, each searched against the whole query set with lists of its own,
 * the survivors of all parts ranked together (the result does not depend on it); 0 = automatic, which cuts the
 * reference only when the query alone cannot fill the GPU.  At most one part per 16 reference cells is used.
 *
 * pred_out / prob_out (n_q x n_labels int32 / float64): DEVICE pointers, NULL iff n_labels == 0 (a plain kNN search).
 * knn_dist_out / knn_idx_out (n_q x k float64 / int32): DEVICE pointers, both or neither.  stream: the caller's
 * hipStream_t (NULL = the null stream); the work runs there, behind what was queued before it, and the call returns once
 * it has completed.  HMX_ERR_ARG for every bad argument, with the reason in hmx_last_error(). */
int hmx_knn_predict(int32_t device_id,
                    const void* Q, int q_dtype, int64_t n_q, int64_t q_stride_cell, int64_t q_stride_col,
                    const void* R, int r_dtype, int64_t n_r, int64_t r_stride_cell, int64_t r_stride_col,
                    int32_t d, int32_t k, int32_t slices, void* stream,
                    const int32_t* ref_label_codes, int32_t n_labels,
                    int32_t* pred_out, double* prob_out,
                    double* knn_dist_out, int32_t* knn_idx_out);

/* The number of reference slices hmx_knn_predict's automatic choice (slices = 0) uses for these sizes on GPU device_id
 * (>= 1), or a negative HMX_ERR_* for arguments hmx_knn_predict would refuse. */
int hmx_knn_slices(int32_t device_id, int64_t n_q, int64_t n_r, int32_t d, int32_t k);

#ifdef __cplusplus
}
#endif
#endif /* HMX_KNN_H */
