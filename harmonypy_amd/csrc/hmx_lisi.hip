// LISI (Local Inverse Simpson Index) on gfx950 -- the integration metric of the reference
// (harmonypy/lisi.py:24-133): exact k nearest neighbours, a per-cell perplexity search, and the
// inverse Simpson index of the labels in the neighbourhood.
//
//   k_lisi_colsum / k_lisi_center : centre the float64 input, float32 copy padded to 16-float rows,
//                                   squared norms (padding rows get +inf and never qualify)
//   k_lisi_load<T>                : a caller's device tensor (float32 / float16 / bfloat16 / float64, any
//                                   strides) read in place into the float64 n x d matrix, converted exactly,
//                                   with k_lisi_colsum's column sums on the way (hmx_compute_lisi_device)
//   k_lisi_knn<KS16, QT>          : brute-force neighbour search.  A wave owns 16*QT queries whose
//                                   fragments stay in registers and streams every 16-candidate tile
//                                   (shared by the workgroup's waves through LDS) through f32 MFMA, turns them into
//                                   |c|^2 - 2 q.c, and appends the candidates below the query's
//                                   current threshold to the query's list in global memory (an LDS
//                                   counter hands out the slots).  A list that is nearly full is
//                                   sorted by the wave in LDS (bitonic, 256 keys), cut to the best
//                                   128, and the 128th key becomes the new threshold.
//   k_lisi_finish                 : one wave per cell: exact float64 distances to the 128 survivors
//                                   (float32 only preselects; 128 >= 3*perplexity leaves slack for
//                                   rank inversions of the approximation), exact ranking, first
//                                   column dropped (lisi.py:58-60), then compute_simpson
//                                   (lisi.py:83-132) in float64 and 1/simpson per label column.
//
// Label transfer (hmx_knn_predict, include/hmx_knn.h) reuses the search across two sets:
//   k_knn_center                  : k_lisi_center with the reference's column means, for both sets
//   k_knn_search<KS16, QT, CAP>   : k_lisi_knn's workgroup (knn_search_block) with queries from the query set and
//                                   candidate tiles from one slice of the reference set (grid y = slice)
//   k_knn_finish<KEEP, FW>        : one wave per query: the survivors of every slice ranked exactly in float64, the
//                                   k nearest written, and a majority vote per label column
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "hmx_device_io.h"
#include "hmx_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ unsigned long long ld_l2(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // past the CU's L1
}
// Ordering between the lanes of ONE wave through LDS: the DS pipe serves a wave's requests in order, so
// only the compiler has to be kept from moving LDS accesses across the hand-over points.
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// float -> unsigned with the same order (negative values included)
__device__ __forceinline__ unsigned order_bits(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_float(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// one thread per column (d may exceed the workgroup: up to HMX_MAX_PCS), 1024 rows per workgroup
__global__ __launch_bounds__(256) void k_lisi_colsum(const double* __restrict__ X, int64_t n, int d, double* __restrict__ sums) {
    const int64_t r0 = (int64_t)blockIdx.x * 1024, r1 = min(n, r0 + 1024);
    for (int c = threadIdx.x; c < d; c += 256) {
        double s = 0.0;
        for (int64_t r = r0; r < r1; ++r) s += X[r * d + c];
        atomicAdd(sums + c, s);
    }
}

struct bf16_t { uint16_t u; };
__device__ __forceinline__ double to_f64(double v) { return v; }
__device__ __forceinline__ double to_f64(float v) { return (double)v; }                                // every conversion exact
__device__ __forceinline__ double to_f64(_Float16 v) { return (double)(float)v; }
__device__ __forceinline__ double to_f64(bf16_t v) { return (double)__uint_as_float((unsigned)v.u << 16); }

// k_lisi_colsum's layout with the source read in place: element (row r, column c) at src + r * s_cell + c * s_col.
// A row-major source is read along the rows by the lanes of a wave; a d x n one (cell stride 1) along the cells by
// every lane, whose column stays in the cache for the next rows.  The float64 rows are written contiguously.
// LISI_LOAD_ROWS rows per workgroup; the row loop is unrolled so that several loads of a lane are in flight.
#define LISI_LOAD_ROWS 256
template <typename T>
__global__ __launch_bounds__(256) void k_lisi_load(const T* __restrict__ src, int64_t s_cell, int64_t s_col, int64_t n, int d,
                                                   double* __restrict__ X, double* __restrict__ sums) {
    const int64_t r0 = (int64_t)blockIdx.x * LISI_LOAD_ROWS, r1 = min(n, r0 + LISI_LOAD_ROWS);
    for (int c = threadIdx.x; c < d; c += 256) {
        const T* col = src + (int64_t)c * s_col;
        double s = 0.0;
#pragma unroll 8
        for (int64_t r = r0; r < r1; ++r) {
            const double v = to_f64(col[r * s_cell]);
            X[r * d + c] = v;
            s += v;
        }
        atomicAdd(sums + c, s);
    }
}

// 16 lanes per row; rows >= n are padding
__global__ __launch_bounds__(256) void k_lisi_center(const double* __restrict__ X, int64_t n, int64_t npad, int d, int dp,
                                                     const double* __restrict__ sums, float* __restrict__ X32, float* __restrict__ cn) {
    const int l16 = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (row >= npad) return;
    float ss = 0.f;
    for (int c = l16; c < dp; c += 16) {
        float v = 0.f;
        if (row < n && c < d) v = (float)(X[row * d + c] - sums[c] / (double)n);
        X32[row * dp + c] = v;
        ss += v * v;
    }
    for (int off = 8; off; off >>= 1) ss += __shfl_xor(ss, off);
    if (l16 == 0) cn[row] = row < n ? ss : __builtin_inff();
}

// ---- wave-level bitonic sort of N keys in LDS (ascending), N / 128 compare-exchanges per lane and step ---------
template <int N>
__device__ __forceinline__ void wave_sort(unsigned long long* scr, int lane) {
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int h = 0; h < N / 128; ++h) {
                const int p = lane + 64 * h;
                const int i = ((p / j) * 2 * j) + (p % j);
                const int l = i + j;
                const bool up = (i & k) == 0;
                const unsigned long long a = scr[i], b = scr[l];
                if ((a > b) == up) { scr[i] = b; scr[l] = a; }
            }
            wave_fence();
        }
    }
}

// Candidate lists come in three sizes (CAP entries, the best CAP / 2 kept by a compaction and ranked exactly afterwards):
// 256 for 3 * perplexity <= 120 neighbours (the reference's default is 90), 1024 up to 504, 4096 up to 2040.  The large
// sizes keep the sort scratch in dynamic LDS (32 KB / 128 KB per workgroup) and so run fewer workgroups per CU.
//
// Above 208 features (KS16 14..20, QT 1) two things change, both by constexpr so that the instances up to 208 are
// compiled as before:
//  - registers: the query fragments alone are 4 * KS16 VGPRs (80 at 320 features), the tile fragments as many again,
//    plus the prefetch pieces (8 * NPC) -- 192 at KS16 = 20, more than the 168 of three waves per SIMD.  The 256-entry
//    lists there ask for two (256 registers; KS16 14..16 still fit in 168), the larger lists keep asking for one;
//  - LDS: the sort scratch of the 4096-entry lists (4 waves x 32 KB) plus two staging buffers of 16 x (16 * KS16 + 4)
//    floats exceed the CU's 160 KB from KS16 = 16 on.  Those instances stage through ONE buffer and take a second
//    barrier per tile, between the fragment reads of tile t and the store of tile t+1 (every wave has multiplied by
//    then).  Fewer waves per workgroup would keep the single barrier but multiply the workgroup's global / L2 reads
//    of every candidate tile; halving the feature dimension would split the query fragments across two passes.  The
//    4096-entry lists (3 * perplexity > 504) are dominated by their compaction sorts anyway.
template <int KS16, int QT, int CAP>
constexpr int knn_stage_buffers() {
    constexpr size_t fixed = (size_t)LISI_KNN_WAVES * CAP * 8 + (size_t)LISI_KNN_WAVES * 16 * QT * 4 * 2;   // scratch, cnt, tau
    return fixed + 2 * 16 * (16 * KS16 + 4) * 4 <= 160 * 1024 ? 2 : 1;
}

// k_knn_search: queries per wave as k_lisi_knn, and workgroups per CU as there except at the 50-feature shape (KS16 4),
// whose k_lisi_knn instance spills at three workgroups per CU
constexpr int knn_search_min_blocks(int KS16, int CAP) { return CAP == 256 ? (KS16 <= 13 && KS16 != 4 ? 3 : 2) : 1; }

// The search of one workgroup, shared by k_lisi_knn (a set against itself) and k_knn_search (the query set against one
// slice of the reference set): queries are rows qbase.. of Xq (qbase from blockIdx.x), candidates the 16-row tiles
// tile0 .. tile0 + ntiles - 1 of Xc with norms cn (candidate index = row of Xc), query row i's list at lists + i * CAP and
// its final length in counts[i] for i < nq.
template <int KS16, int QT, int CAP>
__device__ __forceinline__ void knn_search_block(const float* Xq, const float* Xc, const float* cn, int tile0, int ntiles, int dp,
                                                 unsigned long long* lists, int* counts, int64_t nq, unsigned long long* prof) {
    constexpr int KEEP = CAP / 2;
    constexpr int NSTAGE = knn_stage_buffers<KS16, QT, CAP>();
    extern __shared__ __attribute__((aligned(16))) unsigned long long scr_all[];   // waves x CAP
    __shared__ int cnt_all[LISI_KNN_WAVES][16 * QT];
    __shared__ float tau_all[LISI_KNN_WAVES][16 * QT];
    constexpr int LDW = 16 * KS16 + 4;                       // padded row: conflict-free 16-byte fragment reads
    __shared__ __attribute__((aligned(16))) float stage[NSTAGE][16 * LDW];
    static_assert((size_t)LISI_KNN_WAVES * CAP * 8 + sizeof(cnt_all) + sizeof(tau_all) + sizeof(stage) <= 160 * 1024,
                  "knn_search_block: LDS over the CU's 160 KB");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c16 = lane & 15, q = lane >> 4;
    unsigned long long* scr = scr_all + (size_t)wv * CAP;
    int* cnt = cnt_all[wv];
    float* tau = tau_all[wv];
    const int64_t qbase = ((int64_t)blockIdx.x * LISI_KNN_WAVES + wv) * (16 * QT);   // < npad: npad is a multiple of 256
    for (int i = lane; i < 16 * QT; i += 64) { cnt[i] = 0; tau[i] = __builtin_inff(); }
    wave_fence();

    f32x4 bq[QT][KS16];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int m = 0; m < KS16; ++m) bq[t][m] = ld4(Xq + (size_t)(qbase + 16 * t + c16) * dp + 16 * m + 4 * q);
    float th[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) th[t] = __builtin_inff();

    // sort one query's list, keep the best KEEP, tighten its threshold
    auto compact = [&](int slot) {
        const int c = cnt[slot];
        unsigned long long* lst = lists + (size_t)(qbase + slot) * CAP;
#pragma unroll 4
        for (int h = 0; h < CAP / 64; ++h) { const int i = lane + 64 * h; scr[i] = i < c ? ld_l2(lst + i) : ~0ull; }
        wave_fence();
        wave_sort<CAP>(scr, lane);
        const int keep = min(c, KEEP);
#pragma unroll 4
        for (int h = 0; h < KEEP / 64; ++h) { const int i = lane + 64 * h; if (i < keep) lst[i] = scr[i]; }
        if (lane == 0) {
            cnt[slot] = keep;
            if (c >= KEEP) tau[slot] = order_float((unsigned)(scr[KEEP - 1] >> 32));
        }
        wave_fence();
    };

    // Software pipeline over the candidate tiles.  The workgroup's four waves share every tile
    // through LDS (one global read per workgroup instead of one per wave: the float32 matrix is
    // streamed by every workgroup, so the reuse decides whether the loop is L2/MALL- or MFMA-bound):
    //   iteration t:  issue the global loads of tile t+2's pieces  ->  fragments of tile t from
    //   LDS, MFMAs of tile t  ->  pieces of tile t+1 (issued an iteration ago) into the other LDS
    //   buffer  ->  tile t-1's products into keys, the qualifying ones appended to the
    //   lists  ->  barrier.
    // The list stores are issued from inline assembly on purpose: with ordinary stores in the loop the
    // compiler waits for vmcnt(0) before every use of a loaded value (it cannot bound a counter that
    // loads and stores leave out of order).  Its "at most as many outstanding as loads issued after
    // the wanted one" is still sufficient: loads return in order among themselves, so while a wanted
    // load is outstanding every younger load is too and the counter stays above the bound; a store
    // in flight can only lengthen the wait.
    constexpr int NPC = (64 * KS16 + 64 * LISI_KNN_WAVES - 1) / (64 * LISI_KNN_WAVES);   // 16-byte pieces per thread
    f32x4 pre[2][NPC], af[KS16], acc[2][QT];
    auto fetch_pieces = [&](int ps, int tile) {
#pragma unroll
        for (int j = 0; j < NPC; ++j) {
            const int i = tid + 64 * LISI_KNN_WAVES * j;
            const int row = i / (4 * KS16), c4 = i - row * (4 * KS16);
            if (i < 64 * KS16) pre[ps][j] = ld4(Xc + (size_t)(16 * tile + row) * dp + 4 * c4);
        }
    };
    auto store_pieces = [&](int ps, int sb) {
        if constexpr (NSTAGE == 1) sb = 0;
#pragma unroll
        for (int j = 0; j < NPC; ++j) {
            const int i = tid + 64 * LISI_KNN_WAVES * j;
            const int row = i / (4 * KS16), c4 = i - row * (4 * KS16);
            if (i < 64 * KS16) *reinterpret_cast<f32x4*>(&stage[sb][row * LDW + 4 * c4]) = pre[ps][j];
        }
    };
    auto read_fragments = [&](int sb) {
        if constexpr (NSTAGE == 1) sb = 0;
#pragma unroll
        for (int m = 0; m < KS16; ++m) af[m] = *reinterpret_cast<const f32x4*>(&stage[sb][c16 * LDW + 16 * m + 4 * q]);
    };
    auto multiply = [&](int p) {
#pragma unroll
        for (int t = 0; t < QT; ++t) acc[p][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < KS16; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < QT; ++t) acc[p][t] = MFMA16(af[m][r], bq[t][m][r], acc[p][t]);
    };
    // Tile products -> keys -> list entries.  Most tiles add nothing once the thresholds are tight: one
    // wave-wide test leaves early.  A qualifying value takes its list position from the query's LDS
    // counter and is stored from inline assembly (see below); the positions handed out tell whether a
    // list is about to overflow, so the counters are not read back.
    auto append = [&](int p, const f32x4 cn4, int tile) {
        bool any = false;
        float key[QT][4];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                key[t][r] = cn4[r] - 2.f * acc[p][t][r];                 // |c|^2 - 2 q.c (+inf for padding rows)
                any |= key[t][r] < th[t];
            }
        if (!__any(any)) return;                                        // the common case once the thresholds are tight
        // Qualifying values are few and scattered: every lane walks the set bits of its own 16-value
        // mask, so the wave loops as often as its busiest lane has entries (once, typically) instead
        // of branching around sixteen value slots.
        unsigned mask = 0;
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) mask |= (key[t][r] < th[t]) ? (1u << (4 * t + r)) : 0u;
        bool full = false;
        while (__any(mask != 0)) {
            if (mask != 0) {
                const int j = __ffs(mask) - 1;
                mask &= mask - 1;
                float kv = key[0][0];
#pragma unroll
                for (int jj = 1; jj < 4 * QT; ++jj) kv = (j == jj) ? key[jj >> 2][jj & 3] : kv;
                const int t = j >> 2, r = j & 3;
                const int slot = atomicAdd(&cnt[16 * t + c16], 1);
                const unsigned long long ent = ((unsigned long long)order_bits(kv) << 32) | (unsigned)(16 * tile + 4 * q + r);
                unsigned long long* dst = lists + (size_t)(qbase + 16 * t + c16) * CAP + slot;
                asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(dst), "v"(ent) : "memory");
                full |= slot >= CAP - 16;                          // the list now holds more than CAP-16 entries
            }
        }
        if (__any(full)) {
            wave_fence();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the list entries are in L2
            for (int slot = 0; slot < 16 * QT; ++slot)
                if (cnt[slot] > CAP - 16) compact(slot);           // wave-uniform
#pragma unroll
            for (int t = 0; t < QT; ++t) th[t] = tau[16 * t + c16];
        }
    };
    // the query fragments must have landed before the loop: a wait for them left inside the loop
    // would also wait for the prefetches issued there
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int m = 0; m < KS16; ++m) asm volatile("" ::"v"(bq[t][m][3]));
    fetch_pieces(0, tile0);
    store_pieces(0, 0);
    if (ntiles > 1) fetch_pieces(1, tile0 + 1);
    __syncthreads();
#ifdef LISI_PROF   // cycle stamps per phase segment (timing experiments only)
    unsigned long long pf[6] = {0, 0, 0, 0, 0, 0}, pt = __builtin_amdgcn_s_memtime();
#define LISI_STAMP(k) { const unsigned long long now = __builtin_amdgcn_s_memtime(); pf[k] += now - pt; pt = now; }
#else
#define LISI_STAMP(k)
#endif
    for (int ct = 0; ct < ntiles; ct += 2) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int t = ct + p;
            if (t < ntiles) {                                           // workgroup-uniform
                const bool more = t + 1 < ntiles;
                // addresses of both loads first, in registers of their own: the compiler otherwise recycles
                // the first load's address registers for the second and waits for the first load to return
                int cn_off = 16 * (tile0 + (t > 0 ? t - 1 : 0)) + 4 * q;
                asm volatile("" : "+v"(cn_off));
                if (t + 2 < ntiles) fetch_pieces(p, tile0 + t + 2);             // two tiles ahead: a round trip can exceed one MFMA phase
                const f32x4 cn_prev = ld4(cn + cn_off);               // norms of the tile appended below
                __builtin_amdgcn_sched_barrier(0);                      // loads first: their latency runs under the MFMAs
                LISI_STAMP(0)
                read_fragments(p);
                multiply(p);
                __builtin_amdgcn_sched_barrier(0);
                LISI_STAMP(1)
                if constexpr (NSTAGE == 1) __syncthreads();             // one buffer: every wave has read tile t
                if (more) store_pieces(p ^ 1, p ^ 1);
                __builtin_amdgcn_sched_barrier(0);
                LISI_STAMP(2)
                if (t > 0) append(p ^ 1, cn_prev, tile0 + t - 1);
                LISI_STAMP(3)
                __syncthreads();
                LISI_STAMP(4)
            }
        }
    }
#ifdef LISI_PROF
    if (lane == 0 && prof) for (int k = 0; k < 6; ++k) atomicAdd(prof + k, pf[k]);
#endif
    {
        const f32x4 cn_last = ld4(cn + 16 * (tile0 + ntiles - 1) + 4 * q);
        if ((ntiles - 1) & 1) append(1, cn_last, tile0 + ntiles - 1);
        else append(0, cn_last, tile0 + ntiles - 1);
    }
    wave_fence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int slot = 0; slot < 16 * QT; ++slot) {
        compact(slot);
        if (lane == 0 && qbase + slot < nq) counts[qbase + slot] = cnt[slot];
    }
}

template <int KS16, int QT, int CAP>
__global__ __launch_bounds__(64 * LISI_KNN_WAVES, CAP == 256 ? (KS16 <= 13 ? 3 : 2) : 1) void k_lisi_knn(LisiKnnArgs a) {
    knn_search_block<KS16, QT, CAP>(a.X, a.X, a.cn, 0, (int)((a.n + 15) / 16), a.dp, a.lists, a.counts, a.n, a.prof);
}

// The cross-set search: the query blocks along x, the reference slices along y.  Slice s streams the reference tiles
// s * tiles_per_slice .. (at least one) into lists and counts of its own.
template <int KS16, int QT, int CAP>
__global__ __launch_bounds__(64 * LISI_KNN_WAVES, knn_search_min_blocks(KS16, CAP)) void k_knn_search(KnnSearchArgs a) {
    const int s = blockIdx.y;
    const int t0 = s * a.tiles_per_slice;
    knn_search_block<KS16, QT, CAP>(a.Xq, a.Xr, a.cn, t0, min(a.ntiles - t0, a.tiles_per_slice), a.dp,
                                    a.lists + (size_t)s * a.nq_pad * CAP, a.counts + (size_t)s * a.nq, a.nq, nullptr);
}

// ---- exact ranking + compute_simpson ------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int KEEP, int FW>
__global__ __launch_bounds__(64 * FW) void k_lisi_finish(LisiFinishArgs a) {
    constexpr int NH = KEEP / 64;                                       // list positions per lane
    __shared__ unsigned long long key_all[FW][KEEP];
    __shared__ int idx_all[FW][KEEP];
    __shared__ double p_all[FW][KEEP];
    __shared__ int lab_all[FW][KEEP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cell = (int64_t)blockIdx.x * FW + wv;
    if (cell >= a.n) return;
    unsigned long long* key = key_all[wv];
    int* idx = idx_all[wv];
    double* P = p_all[wv];
    int* lab = lab_all[wv];
    const int c = a.counts[cell];
    const unsigned long long* lst = a.lists + (size_t)cell * (2 * KEEP);
    const double* xq = a.X + (size_t)cell * a.d;
    // exact squared distances to the survivors, float64 from direct differences
#pragma unroll 2
    for (int h = 0; h < NH; ++h) {
        const int i = lane + 64 * h;
        unsigned long long kb = ~0ull;
        int id = 0x7FFFFFFF;
        if (i < c) {
            id = (int)(unsigned)(lst[i] & 0xFFFFFFFFull);
            const double* xc = a.X + (size_t)id * a.d;
            double s = 0.0;
            for (int k = 0; k < a.d; ++k) { const double df = xc[k] - xq[k]; s += df * df; }
            kb = (unsigned long long)__double_as_longlong(s);           // s >= 0: bit order = value order
        }
        key[i] = kb; idx[i] = id;
    }
    wave_fence();
    // bitonic sort of the KEEP (distance, index) pairs, ties by index
    for (int k = 2; k <= KEEP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int h = 0; h < KEEP / 128; ++h) {
                const int p = lane + 64 * h;
                const int i = ((p / j) * 2 * j) + (p % j);
                const int l = i + j;
                const bool up = (i & k) == 0;
                const unsigned long long ka = key[i], kb = key[l];
                const int ia = idx[i], ib = idx[l];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == up) { key[i] = kb; key[l] = ka; idx[i] = ib; idx[l] = ia; }
            }
            wave_fence();
        }
    }
    // neighbours = ranks 1 .. nn-1 (the first column is dropped, lisi.py:58-60)
    const int M = a.nn - 1;
    double D[NH];
    int nid[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int j = lane + 64 * h;
        D[h] = j < M ? sqrt(__longlong_as_double((long long)key[j + 1])) : 0.0;
        nid[h] = j < M ? idx[j + 1] : 0;
        if (j < M && a.knn_dist) { a.knn_dist[(size_t)cell * M + j] = D[h]; a.knn_idx[(size_t)cell * M + j] = nid[h]; }
    }
    // lisi.py:83-119: search beta so that the entropy of P = exp(-beta D) is log(perplexity)
    const double logU = log(a.perplexity);
    double beta = 1.0, betamin = -__builtin_inf(), betamax = __builtin_inf();
    double H = 0.0, Pn[NH];
    auto entropy = [&]() {
        double p[NH], s = 0.0, sd = 0.0;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            p[h] = (lane + 64 * h) < M ? exp(-D[h] * beta) : 0.0;
            s += p[h];
            sd += D[h] * p[h];
        }
        s = wave_sum(s);
        sd = wave_sum(sd);
        if (s == 0.0) {
            H = 0.0;
#pragma unroll
            for (int h = 0; h < NH; ++h) Pn[h] = 0.0;
        } else {
            H = log(s) + beta * sd / s;
#pragma unroll
            for (int h = 0; h < NH; ++h) Pn[h] = p[h] / s;
        }
    };
    entropy();
    double Hdiff = H - logU;
    for (int t = 0; t < 50; ++t) {
        if (fabs(Hdiff) < a.tol) break;
        if (Hdiff > 0) {
            betamin = beta;
            beta = isinf(betamax) ? beta * 2.0 : (beta + betamax) / 2.0;
        } else {
            betamax = beta;
            beta = isinf(betamin) ? beta / 2.0 : (beta + betamin) / 2.0;
        }
        entropy();
        Hdiff = H - logU;
    }
    // lisi.py:120-132: squared probability mass per category = sum_j P_j * (mass of j's category)
#pragma unroll
    for (int h = 0; h < NH; ++h) { const int j = lane + 64 * h; P[j] = j < M ? Pn[h] : 0.0; }
    wave_fence();
    for (int L = 0; L < a.n_labels; ++L) {
#pragma unroll
        for (int h = 0; h < NH; ++h) { const int j = lane + 64 * h; if (j < M) lab[j] = a.labels[(size_t)L * a.n + nid[h]]; }
        wave_fence();
        double part = 0.0;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int j = lane + 64 * h;
            if (j < M) {
                const int mine = lab[j];
                double mass = 0.0;
                for (int m2 = 0; m2 < M; ++m2) mass += (lab[m2] == mine) ? P[m2] : 0.0;
                part += Pn[h] * mass;
            }
        }
        double simpson = wave_sum(part);
        if (H == 0.0) simpson += -1.0;
        if (lane == 0) a.out[(size_t)cell * a.n_labels + L] = 1.0 / simpson;
        wave_fence();
    }
}

// ---- cross-set kNN (hmx_knn_predict): centring by the reference's means, exact ranking of the slices' survivors, vote ----

// k_lisi_center with the means of another set (the reference's column sums over n_ref rows); cn may be null (queries)
__global__ __launch_bounds__(256) void k_knn_center(const double* __restrict__ X, int64_t n, int64_t npad, int d, int dp,
                                                    const double* __restrict__ ref_sums, int64_t n_ref, float* __restrict__ X32,
                                                    float* __restrict__ cn) {
    const int l16 = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (row >= npad) return;
    float ss = 0.f;
    for (int c = l16; c < dp; c += 16) {
        float v = 0.f;
        if (row < n && c < d) v = (float)(X[row * d + c] - ref_sums[c] / (double)n_ref);
        X32[row * dp + c] = v;
        ss += v * v;
    }
    for (int off = 8; off; off >>= 1) ss += __shfl_xor(ss, off);
    if (cn && l16 == 0) cn[row] = row < n ? ss : __builtin_inff();
}

// (distance bits, index) pairs of one wave in LDS, ascending, ties by the smaller index
__device__ __forceinline__ void cswap_pair(unsigned long long* key, int* idx, int i, int l) {
    const unsigned long long ka = key[i], kb = key[l];
    const int ia = idx[i], ib = idx[l];
    if (ka > kb || (ka == kb && ia > ib)) { key[i] = kb; key[l] = ka; idx[i] = ib; idx[l] = ia; }
}
template <int N>
__device__ __forceinline__ void wave_sort_pairs(unsigned long long* key, int* idx, int lane) {
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int h = 0; h < N / 128; ++h) {
                const int p = lane + 64 * h;
                const int i = ((p / j) * 2 * j) + (p % j);
                if ((i & k) == 0) cswap_pair(key, idx, i, i + j);
                else cswap_pair(key, idx, i + j, i);
            }
            wave_fence();
        }
    }
}
// [0, N) and [N, 2N) sorted ascending -> [0, N) holds the N smallest of both, sorted: the first compare-exchange of a
// bitonic merge against the reversed second half leaves them in the first half as a bitonic sequence, which is merged.
template <int N>
__device__ __forceinline__ void wave_merge_lower(unsigned long long* key, int* idx, int lane) {
#pragma unroll
    for (int h = 0; h < N / 64; ++h) { const int p = lane + 64 * h; cswap_pair(key, idx, p, 2 * N - 1 - p); }
    wave_fence();
    for (int j = N >> 1; j > 0; j >>= 1) {
#pragma unroll
        for (int h = 0; h < N / 128; ++h) {
            const int p = lane + 64 * h;
            const int i = ((p / j) * 2 * j) + (p % j);
            cswap_pair(key, idx, i, i + j);
        }
        wave_fence();
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// One wave per query: exact float64 distances to the survivors of every slice (KEEP per slice at most), merged into the
// best KEEP by (distance, index); the k nearest written out, then the vote of every label column.  The vote sorts the k
// (label << 32 | rank) pairs in LDS, so any number of categories works: a run of equal labels is one category, its
// length the votes and its first entry the category's nearest member.  Winner: most votes, then the nearest member.
template <int KEEP, int FW>
__global__ __launch_bounds__(64 * FW) void k_knn_finish(KnnFinishArgs a) {
    constexpr int NH = KEEP / 64;                                       // list positions per lane
    __shared__ unsigned long long key_all[FW][2 * KEEP];
    __shared__ int idx_all[FW][2 * KEEP];
    __shared__ unsigned long long start_all[FW][NH];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t qi = (int64_t)blockIdx.x * FW + wv;
    if (qi >= a.nq) return;
    unsigned long long* key = key_all[wv];
    int* idx = idx_all[wv];
    unsigned long long* starts = start_all[wv];
    const double* xq = a.Q + (size_t)qi * a.d;
    for (int s = 0; s < a.slices; ++s) {
        const int c = a.counts[(size_t)s * a.nq + qi];
        const unsigned long long* lst = a.lists + ((size_t)s * a.nq_pad + qi) * (2 * KEEP);
        unsigned long long* kd = key + (s ? KEEP : 0);                  // slice 0 straight into the result half
        int* id = idx + (s ? KEEP : 0);
#pragma unroll 2
        for (int h = 0; h < NH; ++h) {
            const int i = lane + 64 * h;
            unsigned long long kb = ~0ull;
            int r = 0x7FFFFFFF;                                         // no entry: sorts last, never read
            if (i < c) {
                r = (int)(unsigned)(lst[i] & 0xFFFFFFFFull);
                const double* xc = a.R + (size_t)r * a.d;
                double sq = 0.0;
                for (int k = 0; k < a.d; ++k) { const double df = xc[k] - xq[k]; sq += df * df; }
                kb = (unsigned long long)__double_as_longlong(sq);     // sq >= 0: bit order = value order
            }
            kd[i] = kb; id[i] = r;
        }
        wave_fence();
        wave_sort_pairs<KEEP>(kd, id, lane);
        if (s) wave_merge_lower<KEEP>(key, idx, lane);
    }
    // the k nearest (fewer only where the input holds NaN: those ranks keep index 0x7FFFFFFF and are left out)
    int m = 0;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int j = lane + 64 * h;
        const bool ok = j < a.k && idx[j] != 0x7FFFFFFF;
        m += __popcll(__ballot(ok));
        if (j < a.k && a.dist) {
            a.dist[(size_t)qi * a.k + j] = ok ? sqrt(__longlong_as_double((long long)key[j])) : __builtin_nan("");
            a.idx[(size_t)qi * a.k + j] = ok ? idx[j] : -1;
        }
    }
    unsigned long long* sk = key + KEEP;                                // free now
    for (int L = 0; L < a.n_labels; ++L) {
        const int* lab = a.labels + (size_t)L * a.nr;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int j = lane + 64 * h;
            sk[j] = j < m ? ((unsigned long long)(unsigned)lab[idx[j]] << 32) | (unsigned)j : ~0ull;
        }
        wave_fence();
        wave_sort<KEEP>(sk, lane);
        bool st[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int j = lane + 64 * h;
            st[h] = j < m && (j == 0 || (sk[j - 1] >> 32) != (sk[j] >> 32));          // a run of one label starts here
            const unsigned long long w = __ballot(st[h]);
            if (lane == 0) starts[h] = w;
        }
        wave_fence();
        unsigned long long best = 0;                                    // votes << 32 | ~(rank of the nearest member)
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            if (!st[h]) continue;
            const int j = lane + 64 * h;
            unsigned long long w = lane == 63 ? 0ull : starts[h] & (~0ull << (lane + 1));
            int hh = h;
            while (!w && ++hh < NH) w = starts[hh];
            const int next = w ? min(m, 64 * hh + __ffsll((long long)w) - 1) : m;
            const unsigned long long sc = ((unsigned long long)(next - j) << 32) | (0xFFFFFFFFu - (unsigned)sk[j]);
            best = sc > best ? sc : best;
        }
        best = wave_max_u64(best);
        if (lane == 0) {
            const size_t o = (size_t)qi * a.n_labels + L;
            if (m > 0) {
                a.pred[o] = lab[idx[0xFFFFFFFFu - (unsigned)best]];
                a.prob[o] = (double)(best >> 32) / (double)a.k;
            } else {
                a.pred[o] = -1;
                a.prob[o] = 0.0;
            }
        }
        wave_fence();
    }
}

template <int KS16, int CAP>
void launch_knn_cap(const LisiKnnArgs& a, hipStream_t s) {
    constexpr int QT = KS16 <= 4 ? 4 : KS16 <= 8 ? 2 : 1;
    const int64_t waves = (a.npad + 16 * QT - 1) / (16 * QT);
    const int wgs = (int)((waves + LISI_KNN_WAVES - 1) / LISI_KNN_WAVES);
    const size_t sm = (size_t)LISI_KNN_WAVES * CAP * sizeof(unsigned long long);
    static bool attr_done = false;
    if (!attr_done && sm > 48 * 1024) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lisi_knn<KS16, QT, CAP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
        attr_done = true;
    }
    hipLaunchKernelGGL((k_lisi_knn<KS16, QT, CAP>), dim3(wgs), dim3(64 * LISI_KNN_WAVES), sm, s, a);
}
template <int KS16>
void launch_knn_qt(const LisiKnnArgs& a, hipStream_t s) {
    if (a.cap <= 256) launch_knn_cap<KS16, 256>(a, s);
    else if (a.cap <= 1024) launch_knn_cap<KS16, 1024>(a, s);
    else launch_knn_cap<KS16, 4096>(a, s);
}

}  // namespace

void launch_lisi_prepare(const double* X, int64_t n, int64_t npad, int d, int dp, double* sums, float* X32, float* cn, hipStream_t s) {
    (void)hipMemsetAsync(sums, 0, sizeof(double) * d, s);
    hipLaunchKernelGGL(k_lisi_colsum, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, X, n, d, sums);
    hipLaunchKernelGGL(k_lisi_center, dim3((unsigned)(npad / 16)), dim3(256), 0, s, X, n, npad, d, dp, sums, X32, cn);
}

namespace {
template <typename T>
void load_as(const void* src, int64_t s_cell, int64_t s_col, int64_t n, int d, double* X, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_lisi_load<T>, dim3((unsigned)((n + LISI_LOAD_ROWS - 1) / LISI_LOAD_ROWS)), dim3(256), 0, s,
                       static_cast<const T*>(src), s_cell, s_col, n, d, X, sums);
}
}  // namespace

int launch_lisi_prepare_device(const void* src, int dtype, int64_t s_cell, int64_t s_col, int64_t n, int64_t npad, int d, int dp,
                               double* X, double* sums, float* X32, float* cn, hipStream_t s) {
    (void)hipMemsetAsync(sums, 0, sizeof(double) * d, s);
    switch (dtype) {
        case HMX_DTYPE_F32: load_as<float>(src, s_cell, s_col, n, d, X, sums, s); break;
        case HMX_DTYPE_F16: load_as<_Float16>(src, s_cell, s_col, n, d, X, sums, s); break;
        case HMX_DTYPE_BF16: load_as<bf16_t>(src, s_cell, s_col, n, d, X, sums, s); break;
        case HMX_DTYPE_F64: load_as<double>(src, s_cell, s_col, n, d, X, sums, s); break;
        default: return 1;
    }
    hipLaunchKernelGGL(k_lisi_center, dim3((unsigned)(npad / 16)), dim3(256), 0, s, X, n, npad, d, dp, sums, X32, cn);
    return 0;
}

int launch_lisi_knn(const LisiKnnArgs& a, hipStream_t s) {
    switch (a.dp / 16) {
        case 1: launch_knn_qt<1>(a, s); break;
        case 2: launch_knn_qt<2>(a, s); break;
        case 3: launch_knn_qt<3>(a, s); break;
        case 4: launch_knn_qt<4>(a, s); break;
        case 5: launch_knn_qt<5>(a, s); break;
        case 6: launch_knn_qt<6>(a, s); break;
        case 7: launch_knn_qt<7>(a, s); break;
        case 8: launch_knn_qt<8>(a, s); break;
        case 9: launch_knn_qt<9>(a, s); break;
        case 10: launch_knn_qt<10>(a, s); break;
        case 11: launch_knn_qt<11>(a, s); break;
        case 12: launch_knn_qt<12>(a, s); break;
        case 13: launch_knn_qt<13>(a, s); break;
        case 14: launch_knn_qt<14>(a, s); break;
        case 15: launch_knn_qt<15>(a, s); break;
        case 16: launch_knn_qt<16>(a, s); break;
        case 17: launch_knn_qt<17>(a, s); break;
        case 18: launch_knn_qt<18>(a, s); break;
        case 19: launch_knn_qt<19>(a, s); break;
        case 20: launch_knn_qt<20>(a, s); break;
        default: return 1;
    }
    return 0;
}

void launch_lisi_finish(const LisiFinishArgs& a, hipStream_t s) {
    if (a.cap <= 256) hipLaunchKernelGGL((k_lisi_finish<128, 4>), dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, s, a);
    else if (a.cap <= 1024) hipLaunchKernelGGL((k_lisi_finish<512, 4>), dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_lisi_finish<2048, 1>), dim3((unsigned)a.n), dim3(64), 0, s, a);
}

int lisi_list_cap(int nn) { return nn <= 128 - 8 ? 256 : nn <= 512 - 8 ? 1024 : nn <= 2048 - 8 ? 4096 : 0; }

// ---- cross-set kNN -----------------------------------------------------------------------------------------------------
int launch_knn_load(const void* src, int dtype, int64_t s_cell, int64_t s_col, int64_t n, int d, double* X, double* sums, hipStream_t s) {
    (void)hipMemsetAsync(sums, 0, sizeof(double) * d, s);
    switch (dtype) {
        case HMX_DTYPE_F32: load_as<float>(src, s_cell, s_col, n, d, X, sums, s); break;
        case HMX_DTYPE_F16: load_as<_Float16>(src, s_cell, s_col, n, d, X, sums, s); break;
        case HMX_DTYPE_BF16: load_as<bf16_t>(src, s_cell, s_col, n, d, X, sums, s); break;
        case HMX_DTYPE_F64: load_as<double>(src, s_cell, s_col, n, d, X, sums, s); break;
        default: return 1;
    }
    return 0;
}

void launch_knn_center(const double* X, int64_t n, int64_t npad, int d, int dp, const double* ref_sums, int64_t n_ref, float* X32,
                       float* cn, hipStream_t s) {
    hipLaunchKernelGGL(k_knn_center, dim3((unsigned)(npad / 16)), dim3(256), 0, s, X, n, npad, d, dp, ref_sums, n_ref, X32, cn);
}

int knn_queries_per_workgroup(int dp) {
    const int ks16 = dp / 16;
    return LISI_KNN_WAVES * 16 * (ks16 <= 4 ? 4 : ks16 <= 8 ? 2 : 1);
}

namespace {
// fn(std::integral_constant<int, KS16>) for KS16 = dp / 16 in 1..20; 1 for another dp
template <typename Fn>
int with_ks16(int dp, Fn&& fn) {
    switch (dp / 16) {
        case 1: fn(std::integral_constant<int, 1>{}); break;
        case 2: fn(std::integral_constant<int, 2>{}); break;
        case 3: fn(std::integral_constant<int, 3>{}); break;
        case 4: fn(std::integral_constant<int, 4>{}); break;
        case 5: fn(std::integral_constant<int, 5>{}); break;
        case 6: fn(std::integral_constant<int, 6>{}); break;
        case 7: fn(std::integral_constant<int, 7>{}); break;
        case 8: fn(std::integral_constant<int, 8>{}); break;
        case 9: fn(std::integral_constant<int, 9>{}); break;
        case 10: fn(std::integral_constant<int, 10>{}); break;
        case 11: fn(std::integral_constant<int, 11>{}); break;
        case 12: fn(std::integral_constant<int, 12>{}); break;
        case 13: fn(std::integral_constant<int, 13>{}); break;
        case 14: fn(std::integral_constant<int, 14>{}); break;
        case 15: fn(std::integral_constant<int, 15>{}); break;
        case 16: fn(std::integral_constant<int, 16>{}); break;
        case 17: fn(std::integral_constant<int, 17>{}); break;
        case 18: fn(std::integral_constant<int, 18>{}); break;
        case 19: fn(std::integral_constant<int, 19>{}); break;
        case 20: fn(std::integral_constant<int, 20>{}); break;
        default: return 1;
    }
    return 0;
}
// fn(k_knn_search<KS16, QT, CAP> instance, QT, dynamic LDS bytes) for the list size of cap
template <int KS16, typename Fn>
void with_search_instance(int cap, Fn&& fn) {
    constexpr int QT = KS16 <= 4 ? 4 : KS16 <= 8 ? 2 : 1;
    auto one = [&](auto kernel, int c) {
        const size_t sm = (size_t)LISI_KNN_WAVES * c * sizeof(unsigned long long);
        if (sm > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
        fn(kernel, QT, sm);
    };
    if (cap <= 256) one(k_knn_search<KS16, QT, 256>, 256);
    else if (cap <= 1024) one(k_knn_search<KS16, QT, 1024>, 1024);
    else one(k_knn_search<KS16, QT, 4096>, 4096);
}
}  // namespace

int knn_search_workgroups_per_cu(int dp, int cap) {
    int n = 1;
    with_ks16(dp, [&](auto ks) {
        with_search_instance<decltype(ks)::value>(cap, [&](auto kernel, int, size_t sm) {
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64 * LISI_KNN_WAVES, sm) == hipSuccess && per_cu > 0) n = per_cu;
        });
    });
    return n;
}

int launch_knn_search(const KnnSearchArgs& a, hipStream_t s) {
    return with_ks16(a.dp, [&](auto ks) {
        with_search_instance<decltype(ks)::value>(a.cap, [&](auto kernel, int qt, size_t sm) {
            const int wgs = (int)(a.nq_pad / (LISI_KNN_WAVES * 16 * qt));
            const int slices = (a.ntiles + a.tiles_per_slice - 1) / a.tiles_per_slice;
            hipLaunchKernelGGL(kernel, dim3(wgs, slices), dim3(64 * LISI_KNN_WAVES), sm, s, a);
        });
    });
}

void launch_knn_finish(const KnnFinishArgs& a, hipStream_t s) {
    if (a.cap <= 256) hipLaunchKernelGGL((k_knn_finish<128, 4>), dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s, a);
    else if (a.cap <= 1024) hipLaunchKernelGGL((k_knn_finish<512, 4>), dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_knn_finish<2048, 1>), dim3((unsigned)a.nq), dim3(64), 0, s, a);
}
