// hmx_io.hip -- the device I/O path: a caller's embedding in device memory straight into the engine's layout
// (hmx_upload_device), and the engine's N-sized arrays straight back into a caller's tensor (hmx_copy_out_device).
// They replace the host round trip of harmony.py:234-238 (Z uploaded, Z_cos formed) and of the property getters
// (harmony.py:288-351) for callers whose data already lives on the GPU.
//
//   k_io_load_rows<T>  : internal row r <- caller row map[r], converted to fp32, padded to dp with zeros.  With a
//                        feature stride of 1 every row is one contiguous read; with other strides it is element-wise.
//   k_io_load_slab<T>  : cell stride 1 (the reference's d x N orientation, or .T of a row-major matrix): S consecutive
//                        caller cells of every feature are read along the cells into an LDS tile, then written out as
//                        whole internal rows through the inverse map.
//   k_io_store_rows    : caller row map[r] <- internal row r (fp32), any strides.
//   k_io_store_slab    : cell stride 1: whole internal rows of S consecutive caller cells into the LDS tile, then every
//                        column written along the cells.
//   k_io_invert        : inverse of the cell map (caller row -> internal row), for the slab kernels.
//
// Every kernel is a single pass over HBM: no reuse, no arithmetic beyond the conversion.  The LDS tile is S x pitch
// floats with an odd pitch, so that the column accesses of a wave (one cell per lane) fall on distinct banks; S is the
// largest of 128 / 64 / 32 whose tile stays within 64 KB.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hmx_device_io.h"
#include "hmx_internal.h"

namespace {

constexpr int IO_THREADS = 256;
constexpr int IO_ROWS = 32;        // internal rows per workgroup of the row kernels

struct bf16_t { uint16_t u; };

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(double v) { return (float)v; }           // round to nearest even, as NumPy
__device__ __forceinline__ float to_f32(_Float16 v) { return (float)v; }          // exact
__device__ __forceinline__ float to_f32(bf16_t v) { return __uint_as_float((unsigned)v.u << 16); }   // exact

template <typename T>
__global__ __launch_bounds__(IO_THREADS) void k_io_load_rows(const T* __restrict__ src, int64_t s_cell, int64_t s_pc,
                                                             const int* __restrict__ map, float* __restrict__ dst,
                                                             int d, int dp, int64_t N) {
    const int64_t r0 = (int64_t)blockIdx.x * IO_ROWS;
    const int n = (int)min((int64_t)IO_ROWS, N - r0) * dp;
    float* out = dst + r0 * dp;
    for (int i = threadIdx.x; i < n; i += IO_THREADS) {
        const int j = (unsigned)i / (unsigned)dp, c = i - j * dp;
        const int64_t r = r0 + j;
        const int64_t sr = map ? (int64_t)map[r] : r;
        out[i] = c < d ? to_f32(src[sr * s_cell + (int64_t)c * s_pc]) : 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(IO_THREADS) void k_io_load_slab(const T* __restrict__ src, int64_t s_pc, const int* __restrict__ inv,
                                                             float* __restrict__ dst, int d, int dp, int pitch, int64_t N, int lg_s) {
    extern __shared__ float tile[];
    const int S = 1 << lg_s;
    const int64_t n0 = (int64_t)blockIdx.x << lg_s;
    const int ns = (int)min((int64_t)S, N - n0);
    for (int i = threadIdx.x; i < (d << lg_s); i += IO_THREADS) {
        const int f = i >> lg_s, j = i & (S - 1);
        if (j < ns) tile[j * pitch + f] = to_f32(src[(int64_t)f * s_pc + n0 + j]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ns * dp; i += IO_THREADS) {
        const int j = (unsigned)i / (unsigned)dp, c = i - j * dp;
        const int64_t r = inv ? (int64_t)inv[n0 + j] : n0 + j;
        dst[r * dp + c] = c < d ? tile[j * pitch + c] : 0.f;
    }
}

__global__ __launch_bounds__(IO_THREADS) void k_io_store_rows(const float* __restrict__ src, int ld, int cols, const int* __restrict__ map,
                                                              float* __restrict__ dst, int64_t s_cell, int64_t s_col, int64_t N) {
    const int64_t r0 = (int64_t)blockIdx.x * IO_ROWS;
    const int n = (int)min((int64_t)IO_ROWS, N - r0) * cols;
    for (int i = threadIdx.x; i < n; i += IO_THREADS) {
        const int j = (unsigned)i / (unsigned)cols, c = i - j * cols;
        const int64_t r = r0 + j;
        const int64_t dr = map ? (int64_t)map[r] : r;
        dst[dr * s_cell + (int64_t)c * s_col] = src[r * ld + c];
    }
}

__global__ __launch_bounds__(IO_THREADS) void k_io_store_slab(const float* __restrict__ src, int ld, int cols, const int* __restrict__ inv,
                                                              float* __restrict__ dst, int64_t s_col, int pitch, int64_t N, int lg_s) {
    extern __shared__ float tile[];
    const int S = 1 << lg_s;
    const int64_t n0 = (int64_t)blockIdx.x << lg_s;
    const int ns = (int)min((int64_t)S, N - n0);
    for (int i = threadIdx.x; i < ns * cols; i += IO_THREADS) {
        const int j = (unsigned)i / (unsigned)cols, c = i - j * cols;
        const int64_t r = inv ? (int64_t)inv[n0 + j] : n0 + j;
        tile[j * pitch + c] = src[r * ld + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (cols << lg_s); i += IO_THREADS) {
        const int f = i >> lg_s, j = i & (S - 1);
        if (j < ns) dst[(int64_t)f * s_col + n0 + j] = tile[j * pitch + f];
    }
}

__global__ __launch_bounds__(IO_THREADS) void k_io_invert(const int* __restrict__ map, int* __restrict__ inv, int64_t N) {
    const int64_t r = (int64_t)blockIdx.x * IO_THREADS + threadIdx.x;
    if (r < N) inv[map[r]] = (int)r;
}

int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

IoSlab io_slab(int cols) {
    IoSlab t;
    t.pitch = cols | 1;
    t.lg_s = t.pitch * 128 * 4 <= 65536 ? 7 : t.pitch * 64 * 4 <= 65536 ? 6 : 5;
    return t;
}

bool io_uses_slab(int64_t s_cell, int64_t s_feat) { return s_cell == 1 && s_feat != 1; }

void launch_io_invert(const int* map, int* inv, int64_t N, hipStream_t s) {
    if (N <= 0) return;
    hipLaunchKernelGGL(k_io_invert, dim3(cdiv64(N, IO_THREADS)), dim3(IO_THREADS), 0, s, map, inv, N);
}

template <typename T>
static void load_as(const void* src, int64_t s_cell, int64_t s_pc, const int* map, const int* inv, float* dst, int d, int dp,
                    int64_t N, hipStream_t s) {
    const T* p = static_cast<const T*>(src);
    if (io_uses_slab(s_cell, s_pc)) {
        const IoSlab t = io_slab(d);
        hipLaunchKernelGGL(k_io_load_slab<T>, dim3(cdiv64(N, (int64_t)1 << t.lg_s)), dim3(IO_THREADS),
                           ((size_t)t.pitch << t.lg_s) * sizeof(float), s, p, s_pc, inv, dst, d, dp, t.pitch, N, t.lg_s);
    } else {
        hipLaunchKernelGGL(k_io_load_rows<T>, dim3(cdiv64(N, IO_ROWS)), dim3(IO_THREADS), 0, s, p, s_cell, s_pc, map, dst, d, dp, N);
    }
}

int launch_io_load(const void* src, int dtype, int64_t s_cell, int64_t s_pc, const int* map, const int* inv, float* dst, int d,
                   int dp, int64_t N, hipStream_t s) {
    if (N <= 0) return 0;
    switch (dtype) {
        case HMX_DTYPE_F32: load_as<float>(src, s_cell, s_pc, map, inv, dst, d, dp, N, s); return 0;
        case HMX_DTYPE_F16: load_as<_Float16>(src, s_cell, s_pc, map, inv, dst, d, dp, N, s); return 0;
        case HMX_DTYPE_BF16: load_as<bf16_t>(src, s_cell, s_pc, map, inv, dst, d, dp, N, s); return 0;
        case HMX_DTYPE_F64: load_as<double>(src, s_cell, s_pc, map, inv, dst, d, dp, N, s); return 0;
        default: return 1;
    }
}

void launch_io_store(const float* src, int ld, int cols, const int* map, const int* inv, float* dst, int64_t s_cell, int64_t s_col,
                     int64_t N, hipStream_t s) {
    if (N <= 0) return;
    if (io_uses_slab(s_cell, s_col)) {
        const IoSlab t = io_slab(cols);
        hipLaunchKernelGGL(k_io_store_slab, dim3(cdiv64(N, (int64_t)1 << t.lg_s)), dim3(IO_THREADS),
                           ((size_t)t.pitch << t.lg_s) * sizeof(float), s, src, ld, cols, inv, dst, s_col, t.pitch, N, t.lg_s);
    } else {
        hipLaunchKernelGGL(k_io_store_rows, dim3(cdiv64(N, IO_ROWS)), dim3(IO_THREADS), 0, s, src, ld, cols, map, dst, s_cell, s_col, N);
    }
}
