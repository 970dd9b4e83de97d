// hmx_score_kernels.h -- argument blocks and launchers of the mapping-confidence kernels (hmx_score.hip), shared with the
// C ABI host code (hmx_capi.cpp: hmx_cluster_moments, hmx_mapping_score).  Not part of the public interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define HMX_MOM_TPW 10   /* output tiles (16 x 16 float64) one wave of k_mom_cov accumulates: 80 accumulator registers */
#define HMX_MSCORE_CT 2  /* 16-cell tiles one wave of k_mscore carries through the clusters */

// Weights of both moment passes: the soft assignment (R non-null) or hard codes in the caller's cell order.
struct MomArgs {
    const float* R;        // N x Kp, or null: code mode
    const int* codes;      // N codes in the caller's order (code mode)
    const int* map;        // internal row -> caller row, or null (identity)
    const float* Z;        // N x dp
    int64_t N, chunk;      // cells; cells per chunk (a multiple of 8)
    int nchunks;
    int Kp, dp, d, dt;     // dt = ceil(d / 16) column tiles
    int G, G16;            // groups, rounded up to 16
    // first pass: slab1[chunk][G16][ld1] = sum w z (dp16 columns), then mass and mass_sq; folded into sums / mean
    double* slab1;
    int ld1;               // 16 * dt + 2
    double* sums;          // G16 x ld1
    double* mean;          // G16 x 16 dt (0 / 0 = NaN for a group without mass)
    // second pass: slab2[chunk][G][nt][256] accumulator tiles of the upper triangle (tile rows <= tile columns), folded into tiles
    double* slab2;
    int nt;                // dt (dt + 1) / 2
    double* tiles;         // G x nt x 256, element [reg * 64 + lane] = (row (lane >> 4) + 4 reg, column lane & 15) of the tile
};
void launch_mom_sums(const MomArgs& a, hipStream_t s);   // first pass and its fold
void launch_mom_cov(const MomArgs& a, hipStream_t s);    // second pass and its fold

struct MScoreArgs {
    const float* R;        // N x Kp
    const float* Z;        // N x dp
    const int* map;        // internal row -> caller row, or null
    const double* T;       // K x mscore_frag_doubles(dt): T_k as the A fragments of its lower-triangular tiles
    const double* off;     // K x 16 dt: t_k, zero padded
    double* out;           // N scores, caller order
    int64_t N;
    int K, Kp, dp, d, dt;
};
// doubles of one cluster's fragments: tile row ti holds 4 (ti + 1) k-steps of 64 lanes,
// element [lane] of step kc = T[16 ti + (lane & 15)][4 kc + (lane >> 4)]
__host__ __device__ inline size_t mscore_frag_doubles(int dt) { return (size_t)128 * dt * (dt + 1); }
__host__ __device__ inline size_t mscore_frag_offset(int ti) { return (size_t)128 * ti * (ti + 1); }
void launch_mscore(const MScoreArgs& a, hipStream_t s);
