/* hmx_device_io.h -- the device I/O path of libhmx.so: an embedding that already lives on the GPU goes in without a
 * host copy, and the N-sized results come back into a caller's device tensor.  Part of the same C ABI as hmx.h
 * (HMX_ABI_VERSION 8: added symbols only), kept in its own header so that hmx.h's declared set stays what its C
 * clients were written against.  Device pointers and streams are those of the engine's GPU (hmx_config.device_id).
 */
#ifndef HMX_DEVICE_IO_H
#define HMX_DEVICE_IO_H

#include "hmx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Element types of a caller's device tensor (hmx_upload_device, hmx_compute_lisi_device). */
#define HMX_DTYPE_F32 0
#define HMX_DTYPE_F16 1
#define HMX_DTYPE_BF16 2
#define HMX_DTYPE_F64 3

/* hmx_upload with Z in device memory of the engine's GPU (harmony.py:234-238: the reference builds Z_corr / Z_orig
 * with torch.tensor(Z, dtype=float32, device=device) and divides by the column norms).  Z holds N cells x d features
 * of type dtype (HMX_DTYPE_*): element (cell n, feature f) at Z + n * stride_cell + f * stride_pc, strides in elements,
 * any non-negative values (row-major N x d, the reference's d x N, transposed views, column slices).  Values are
 * rounded to fp32 to nearest; the device state is byte-identical to hmx_upload's on the same fp32 values.  stream:
 * the caller's hipStream_t (NULL = the null stream) -- the engine waits for an event recorded there before it reads Z,
 * and returns once its reads have completed.  The remaining arguments are hmx_upload's; source_row must be a
 * permutation here.  The cell map stays resident for hmx_copy_out_device (hmx_upload keeps it too). */
int hmx_upload_device(hmx_engine* e, const void* Z, int dtype, int64_t stride_cell, int64_t stride_pc, void* stream,
                      const int32_t* static_cells, int64_t n_static_pos, const int32_t* static_tile_group, int32_t n_static_tiles,
                      const int32_t* group_cols, const float* Pr_b, const float* theta, const float* sigma, const float* lamb,
                      const int32_t* global_id, const int32_t* source_row);

/* Property getters of harmony.py:288-303 (Z_corr / Z_orig / Z_cos / R) into device memory of the engine's GPU: which is
 * HMX_Z_ORIG, HMX_Z_COS, HMX_Z_CORR or HMX_R; dst receives fp32 N cells x cols (d, or K for R) in the caller's cell
 * order (the cell map of the upload), element (cell n, column c) at dst + n * stride_cell + c * stride_col, strides in
 * elements and >= 1; nothing else of dst is written.  Asynchronous: the engine's stream waits for an event recorded on
 * stream (the caller's hipStream_t, NULL = the null stream) before it writes, and stream waits for the copy. */
int hmx_copy_out_device(hmx_engine* e, int which, void* dst, int64_t stride_cell, int64_t stride_col, void* stream);

/* hmx_compute_lisi of hmx.h with X in device memory of GPU device_id: n cells x d features (d in [1, HMX_MAX_PCS]) of
 * type dtype (HMX_DTYPE_*), element (cell r, feature c) at X + r * stride_cell + c * stride_col, strides in elements,
 * any non-negative values (row-major, .T of a d x n tensor, column slices, row-strided views).  Every element is
 * converted to float64 exactly, so the results equal hmx_compute_lisi's on the same values.  label_codes stays in
 * HOST memory (n_labels x n, as for hmx_compute_lisi).  lisi_out (n x n_labels float64) and knn_dist_out / knn_idx_out
 * (n x (nn-1) float64 / int32, both or neither, may be NULL) are DEVICE pointers of that GPU, row-major, written by the
 * kernels in place.  stream: the caller's hipStream_t (NULL = the null stream); the work runs there, behind what was
 * queued before it, and the call returns once it has completed. */
int hmx_compute_lisi_device(int32_t device_id, const void* X, int dtype, int64_t n, int32_t d, int64_t stride_cell,
                            int64_t stride_col, void* stream, const int32_t* label_codes, int32_t n_labels, double perplexity,
                            double* lisi_out, double* knn_dist_out, int32_t* knn_idx_out);

#ifdef __cplusplus
}
#endif
#endif /* HMX_DEVICE_IO_H */
