// hmx_score.hip -- mapping confidence (include/hmx_score.h): per-cluster second moments of an engine's cells and the
// per-cell Mahalanobis mapping score of a mapped query.  Everything is float64 on v_mfma_f64_16x16x4_f64: every fp32
// element of Z and R converts exactly, so the only rounding is that of the float64 sums.
//
// Fragment maps of the f64 MFMA (one wave, lane l, li = l & 15, q = l >> 4): A[row li][k q], B[k q][col li], one double
// each; C/D four doubles per lane, register r = (row q + 4 r, col li) -- NOT the map of the f32 forms.
//
//   k_mom_sums   pass 1: per chunk of cells, sum_i w[g,i] z_i for a tile of 16 groups (A = w^T, B = Z) plus mass and
//                mass_sq from the A operands themselves.
//   k_mom_fold1  chunks summed in order: sums, and mean = sums / mass.
//   k_mom_cov    pass 2, centred: per (chunk, group), up to HMX_MOM_TPW tiles of the upper triangle of
//                sum_i w (z_i - mean)(z_i - mean)^T (A = w (z - mean) of the tile's rows, B = z - mean of its columns).
//                Steps of four cells without weight are skipped (hard codes: almost all of them).
//                d <= 64: k_mom_cov_t<DT>, the whole triangle (<= 10 tiles) in one wave, one load per column tile.
//   k_mom_fold2  chunks summed in order.
//   k_mscore     per wave HMX_MSCORE_CT tiles of 16 cells, all clusters in turn: y = T_k x - t_k by tile rows of the lower
//                triangle (A = T_k's fragments as the host packed them, B = x, C starts at -t_k), D^2 = sum y^2 folded over
//                the four lane groups, score += R D.  One wave owns a cell's whole sum, so the order over k is fixed.
//                d <= 64: k_mscore_t<DT>, the cells held in registers across the clusters.
// No kernel writes outside its own slab / output rows; cells behind N and columns behind d are read as zero weight / zero.
#include "hmx_score_kernels.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// weight of internal cell c (valid) for group g
__device__ __forceinline__ double mom_weight(const MomArgs& a, int64_t c, int g, int code) {
    if (a.R) return g < a.G ? (double)a.R[(size_t)c * a.Kp + g] : 0.0;
    return code == g ? 1.0 : 0.0;
}
__device__ __forceinline__ int mom_code(const MomArgs& a, int64_t c) {
    if (a.R) return -1;
    return a.codes[a.map ? a.map[c] : c];
}

// grid (chunk, group tile, block of 4 column tiles), one wave
__global__ __launch_bounds__(64) void k_mom_sums(MomArgs a) {
    const int l = threadIdx.x, li = l & 15, q = l >> 4;
    const int chunk = blockIdx.x, gt = blockIdx.y, cb = blockIdx.z;
    const int64_t c0 = (int64_t)chunk * a.chunk, cend = c0 + a.chunk < a.N ? c0 + a.chunk : a.N;
    const int g = 16 * gt + li;
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double m1 = 0.0, m2 = 0.0;
    int col[4];
    bool colok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        col[t] = 16 * (4 * cb + t) + li;
        colok[t] = col[t] < a.d;
        if (!colok[t]) col[t] = 0;
    }
    for (int64_t cs = c0; cs < cend; cs += 4) {
        const int64_t c = cs + q;
        const bool valid = c < cend;
        const int64_t ci = valid ? c : c0;
        const double w = valid ? mom_weight(a, ci, g, mom_code(a, ci)) : 0.0;
        if (!__any(w != 0.0)) continue;
        m1 += w;
        m2 += w * w;
        const float* z = a.Z + (size_t)ci * a.dp;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (4 * cb + t < a.dt) {
                const double b = valid && colok[t] ? (double)z[col[t]] : 0.0;
                acc[t] = MFMA64(w, b, acc[t]);
            }
        }
    }
    double* out = a.slab1 + ((size_t)chunk * a.G16 + 16 * gt) * a.ld1;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (4 * cb + t < a.dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(q + 4 * r) * a.ld1 + 16 * (4 * cb + t) + li] = acc[t][r];
    if (cb == 0) {
        m1 += __shfl_xor(m1, 16); m1 += __shfl_xor(m1, 32);
        m2 += __shfl_xor(m2, 16); m2 += __shfl_xor(m2, 32);
        if (q == 0) {
            out[(size_t)li * a.ld1 + 16 * a.dt] = m1;
            out[(size_t)li * a.ld1 + 16 * a.dt + 1] = m2;
        }
    }
}

// one thread per entry of sums (G16 x ld1): the chunks in order; the mean beside it
__global__ __launch_bounds__(256) void k_mom_fold1(MomArgs a) {
    const size_t n = (size_t)a.G16 * a.ld1, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = (int)(i / a.ld1), c = (int)(i % a.ld1);
    double v = 0.0, m = 0.0;
    for (int ch = 0; ch < a.nchunks; ++ch) {
        const double* s = a.slab1 + ((size_t)ch * a.G16 + g) * a.ld1;
        v += s[c];
        m += s[16 * a.dt];
    }
    a.sums[i] = v;
    if (c < 16 * a.dt) a.mean[(size_t)g * 16 * a.dt + c] = v / m;
}

// grid (chunk, group, block of HMX_MOM_TPW tiles of the upper triangle), one wave
__global__ __launch_bounds__(64) void k_mom_cov(MomArgs a) {
    const int l = threadIdx.x, li = l & 15, q = l >> 4;
    const int chunk = blockIdx.x, g = blockIdx.y, t0 = blockIdx.z * HMX_MOM_TPW;
    const int64_t c0 = (int64_t)chunk * a.chunk, cend = c0 + a.chunk < a.N ? c0 + a.chunk : a.N;
    const int ntile = a.nt - t0 < HMX_MOM_TPW ? a.nt - t0 : HMX_MOM_TPW;
    // tile t of the triangle in row-major order of (ti <= tj): walk to t0, then on
    int ti = 0, tj = 0;
    for (int t = 0; t < t0; ++t)
        if (++tj == a.dt) { ++ti; tj = ti; }
    int ci_[HMX_MOM_TPW], cj_[HMX_MOM_TPW];
    bool oki[HMX_MOM_TPW], okj[HMX_MOM_TPW];
    double mi[HMX_MOM_TPW], mj[HMX_MOM_TPW];
    f64x4 acc[HMX_MOM_TPW];
    const double* mean = a.mean + (size_t)g * 16 * a.dt;
#pragma unroll
    for (int t = 0; t < HMX_MOM_TPW; ++t) {
        acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        const int ri = 16 * ti + li, rj = 16 * tj + li;
        oki[t] = t < ntile && ri < a.d;
        okj[t] = t < ntile && rj < a.d;
        ci_[t] = oki[t] ? ri : 0;
        cj_[t] = okj[t] ? rj : 0;
        mi[t] = mean[ci_[t]];
        mj[t] = mean[cj_[t]];
        if (++tj == a.dt) { ++ti; tj = ti; }
    }
    for (int64_t cs = c0; cs < cend; cs += 4) {
        const int64_t c = cs + q;
        const bool valid = c < cend;
        const int64_t ci = valid ? c : c0;
        const double w = valid ? mom_weight(a, ci, g, mom_code(a, ci)) : 0.0;
        if (!__any(w != 0.0)) continue;
        const float* z = a.Z + (size_t)ci * a.dp;
#pragma unroll
        for (int t = 0; t < HMX_MOM_TPW; ++t) {
            if (t < ntile) {
                const double zi = valid && oki[t] ? (double)z[ci_[t]] - mi[t] : 0.0;
                const double zj = valid && okj[t] ? (double)z[cj_[t]] - mj[t] : 0.0;
                acc[t] = MFMA64(w * zi, zj, acc[t]);
            }
        }
    }
    double* out = a.slab2 + (((size_t)chunk * a.G + g) * a.nt + t0) * 256;
#pragma unroll
    for (int t = 0; t < HMX_MOM_TPW; ++t)
        if (t < ntile)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)t * 256 + r * 64 + l] = acc[t][r];
}

// d <= 64 (DT = ceil(d / 16) <= 4): the whole upper triangle in one wave, one load per column tile shared by the tiles that use it,
// two steps of four cells per iteration: the loads of both steps are issued together, then their 2 x NT MFMAs (an iteration still
// waits for its own loads; nothing is fetched ahead for the next one).  Same products in the same order as k_mom_cov.
// grid (chunk, group), one wave
template <int DT>
__global__ __launch_bounds__(64) void k_mom_cov_t(MomArgs a) {
    constexpr int NT = DT * (DT + 1) / 2;
    const int l = threadIdx.x, li = l & 15, q = l >> 4;
    const int chunk = blockIdx.x, g = blockIdx.y;
    const int64_t c0 = (int64_t)chunk * a.chunk, cend = c0 + a.chunk < a.N ? c0 + a.chunk : a.N;
    int col[DT];
    bool ok[DT];
    double mu[DT];
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        ok[t] = 16 * t + li < a.d;
        col[t] = ok[t] ? 16 * t + li : 0;
        mu[t] = a.mean[(size_t)g * 16 * DT + col[t]];
    }
    for (int64_t cs = c0; cs < cend; cs += 8) {
        double w[2], zc[2][DT];
        bool valid[2];
        const float* z[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t c = cs + 4 * h + q;
            valid[h] = c < cend;
            const int64_t ci = valid[h] ? c : c0;
            w[h] = valid[h] ? mom_weight(a, ci, g, mom_code(a, ci)) : 0.0;
            z[h] = a.Z + (size_t)ci * a.dp;
        }
        if (!__any(w[0] != 0.0 || w[1] != 0.0)) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int t = 0; t < DT; ++t) zc[h][t] = valid[h] && ok[t] ? (double)z[h][col[t]] - mu[t] : 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int idx = 0;
#pragma unroll
            for (int ti = 0; ti < DT; ++ti) {
                const double aw = w[h] * zc[h][ti];
#pragma unroll
                for (int tj = ti; tj < DT; ++tj, ++idx) acc[idx] = MFMA64(aw, zc[h][tj], acc[idx]);
            }
        }
    }
    double* out = a.slab2 + ((size_t)chunk * a.G + g) * NT * 256;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)t * 256 + r * 64 + l] = acc[t][r];
}

__global__ __launch_bounds__(256) void k_mom_fold2(MomArgs a) {
    const size_t n = (size_t)a.G * a.nt * 256, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = 0.0;
    for (int ch = 0; ch < a.nchunks; ++ch) v += a.slab2[(size_t)ch * n + i];
    a.tiles[i] = v;
}

// one wave per HMX_MSCORE_CT x 16 cells
__global__ __launch_bounds__(64) void k_mscore(MScoreArgs a) {
    constexpr int CT = HMX_MSCORE_CT;
    const int l = threadIdx.x, li = l & 15, q = l >> 4;
    const int64_t base = (int64_t)blockIdx.x * (16 * CT);
    const float* zrow[CT];
    const float* rrow[CT];
    int64_t cell[CT];
    double score[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        cell[ct] = base + 16 * ct + li;
        const int64_t ci = cell[ct] < a.N ? cell[ct] : a.N - 1;   // cells behind N: computed on a copy of the last cell, never stored
        zrow[ct] = a.Z + (size_t)ci * a.dp;
        rrow[ct] = a.R + (size_t)ci * a.Kp;
        score[ct] = 0.0;
    }
    const int dp16 = 16 * a.dt;
    for (int k = 0; k < a.K; ++k) {
        const double* Tk = a.T + (size_t)k * mscore_frag_doubles(a.dt);
        const double* tk = a.off + (size_t)k * dp16;
        double d2[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) d2[ct] = 0.0;
        for (int ti = 0; ti < a.dt; ++ti) {
            f64x4 acc[CT];
            {
                f64x4 t;
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] = -tk[16 * ti + q + 4 * r];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = t;
            }
            const double* frag = Tk + mscore_frag_offset(ti) + l;
            // 4 (ti + 1) k-steps, four at a time: the loads of a group are issued before its MFMAs (features behind d: T holds
            // zeros there and x is read as zero)
            for (int kc = 0; kc < 4 * (ti + 1); kc += 4) {
                double av[4], x[4][CT];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    av[u] = frag[(size_t)(kc + u) * 64];
                    const int f = 4 * (kc + u) + q;
                    const bool fok = f < a.d;
                    const int fi = fok ? f : 0;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) x[u][ct] = fok ? (double)zrow[ct][fi] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) acc[ct] = MFMA64(av[u], x[u][ct], acc[ct]);
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) d2[ct] += acc[ct][r] * acc[ct][r];
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            double v = d2[ct];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            score[ct] += (double)rrow[ct][k] * sqrt(v);
        }
    }
    if (q == 0) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
            if (cell[ct] < a.N) a.out[a.map ? a.map[cell[ct]] : cell[ct]] = score[ct];
    }
}

// d <= 64 (DT <= 4): the wave's cells stay in registers as B operands for all clusters, so the loop over the clusters loads T_k's
// fragments only.  Same products in the same order as k_mscore.
template <int DT>
__global__ __launch_bounds__(64) void k_mscore_t(MScoreArgs a) {
    constexpr int CT = HMX_MSCORE_CT, NK = 4 * DT;
    const int l = threadIdx.x, li = l & 15, q = l >> 4;
    const int64_t base = (int64_t)blockIdx.x * (16 * CT);
    const float* rrow[CT];
    int64_t cell[CT];
    double score[CT], xr[NK][CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        cell[ct] = base + 16 * ct + li;
        const int64_t ci = cell[ct] < a.N ? cell[ct] : a.N - 1;   // cells behind N: computed on a copy of the last cell, never stored
        const float* zrow = a.Z + (size_t)ci * a.dp;
        rrow[ct] = a.R + (size_t)ci * a.Kp;
        score[ct] = 0.0;
#pragma unroll
        for (int u = 0; u < NK; ++u) {
            const int f = 4 * u + q;
            xr[u][ct] = f < a.d ? (double)zrow[f < a.d ? f : 0] : 0.0;
        }
    }
    for (int k = 0; k < a.K; ++k) {
        const double* Tk = a.T + (size_t)k * mscore_frag_doubles(DT) + l;
        const double* tk = a.off + (size_t)k * 16 * DT;
        double d2[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) d2[ct] = 0.0;
#pragma unroll
        for (int ti = 0; ti < DT; ++ti) {
            f64x4 acc[CT];
            {
                f64x4 t;
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] = -tk[16 * ti + q + 4 * r];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = t;
            }
            const double* frag = Tk + mscore_frag_offset(ti);
#pragma unroll
            for (int kc = 0; kc < 4 * (ti + 1); ++kc) {
                const double av = frag[(size_t)kc * 64];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = MFMA64(av, xr[kc][ct], acc[ct]);
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) d2[ct] += acc[ct][r] * acc[ct][r];
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            double v = d2[ct];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            score[ct] += (double)rrow[ct][k] * sqrt(v);
        }
    }
    if (q == 0) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
            if (cell[ct] < a.N) a.out[a.map ? a.map[cell[ct]] : cell[ct]] = score[ct];
    }
}

}  // namespace

void launch_mom_sums(const MomArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_mom_sums, dim3(a.nchunks, a.G16 / 16, (a.dt + 3) / 4), dim3(64), 0, s, a);
    const size_t n = (size_t)a.G16 * a.ld1;
    hipLaunchKernelGGL(k_mom_fold1, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

void launch_mom_cov(const MomArgs& a, hipStream_t s) {
    const dim3 grid(a.nchunks, a.G);
    switch (a.dt) {   // d <= 64: the tuned instances; wider: blocks of tiles
        case 1: hipLaunchKernelGGL(k_mom_cov_t<1>, grid, dim3(64), 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_mom_cov_t<2>, grid, dim3(64), 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_mom_cov_t<3>, grid, dim3(64), 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_mom_cov_t<4>, grid, dim3(64), 0, s, a); break;
        default: hipLaunchKernelGGL(k_mom_cov, dim3(a.nchunks, a.G, (a.nt + HMX_MOM_TPW - 1) / HMX_MOM_TPW), dim3(64), 0, s, a);
    }
    const size_t n = (size_t)a.G * a.nt * 256;
    hipLaunchKernelGGL(k_mom_fold2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

void launch_mscore(const MScoreArgs& a, hipStream_t s) {
    const int64_t per = 16 * HMX_MSCORE_CT;
    const dim3 grid((unsigned)((a.N + per - 1) / per));
    switch (a.dt) {   // d <= 64: the cells stay in registers; wider: they are re-read per cluster
        case 1: hipLaunchKernelGGL(k_mscore_t<1>, grid, dim3(64), 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_mscore_t<2>, grid, dim3(64), 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_mscore_t<3>, grid, dim3(64), 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_mscore_t<4>, grid, dim3(64), 0, s, a); break;
        default: hipLaunchKernelGGL(k_mscore, grid, dim3(64), 0, s, a);
    }
}
