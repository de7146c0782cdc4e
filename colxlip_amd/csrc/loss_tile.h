// The exact-fp32 logits-tile engine of the three fused contrastive losses (loss_fused.hip: ClipLoss, loss_sigmoid.hip:
// SigLipLoss, loss_distill.hip: DistillClipLoss).  None of them holds a logits matrix: 64x64 tiles of z = X . Y^T are
// recomputed from the features on v_mfma_f32_16x16x4_f32 (== an fmaf chain); each loss file keeps its own statistics,
// its d(logits) formula and its ABI functions.
//   forward   lt_tile_to_lds: one 64x64 tile on 2x2 waves into an LDS matrix, reduced by the loss's own epilogue.
//   backward  a block owns 64 rows of one operand and walks its share (lt_split_range) of the other side's 64-row tiles:
//             lt_slab recomputes the wave's 16 x 64 slice of a tile, the loss writes d(logits) to dZs, lt_product adds
//             dZ . Q_tile into 16 x E registers per wave and lt_store_part writes the block's split partial of dP.
//             lt_split_sum adds the splits in split order and lt_sum_parts_kernel the block partials in index order
//             (no atomics: the same result every run).
// Three translation units include this header: its kernels are static.
#pragma once
#include <type_traits>
#include "kernels.h"

constexpr int LT_T = 64;            // tile edge (rows of P x rows of Q)
constexpr int LT_BK = 64;           // k-depth of one staged chunk (16 was latency-bound: two barriers + an L2 round trip per 16-deep chunk)
constexpr int LT_LD = LT_T + 16;    // LDS row stride of the k-major operand images (as gemm_f32.hip)

// columns of Q staged per chunk of the product (NE = E / 16 accumulator tiles per wave; NE == 0: no product)
constexpr int lt_ec(int NE) { return NE >= 4 ? 64 : (NE > 0 ? 16 * NE : 16); }

// stage rows [r0, r0+64) x columns [k0, k0+64) of a row-major [n, E] matrix into the k-major LDS image S[k][row]
// (16-byte loads, four per thread, all issued before the first LDS write; rows >= n and columns >= E read as zero)
__device__ __forceinline__ void lt_stage(float (&S)[LT_BK][LT_LD], const float* __restrict__ src, int r0, int n, int E, int k0,
                                         int tid) {
    const int k4 = (tid & 15) * 4;
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = (tid >> 4) + 16 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + m < n && k0 + k4 < E) v[i] = load4(src + (long)(r0 + m) * E + k0 + k4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = (tid >> 4) + 16 * i;
        S[k4][m] = v[i].x; S[k4 + 1][m] = v[i].y; S[k4 + 2][m] = v[i].z; S[k4 + 3][m] = v[i].w;
    }
}

// ---------------------------------------------------------------------------------------------- forward
// 64x64 tile of X @ Y^T (depth E) into the LDS matrix Z (256 threads; 2x2 waves of 32x32).  No barrier after the Z writes.
__device__ __forceinline__ void lt_tile_to_lds(float (&Xs)[LT_BK][LT_LD], float (&Ys)[LT_BK][LT_LD], float (&Z)[LT_T][LT_T + 1],
                                               const float* __restrict__ X, const float* __restrict__ Y, int p0, int np, int q0,
                                               int nq, int E, int tid) {
    const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += LT_BK) {
        lt_stage(Xs, X, p0, np, E, k0, tid);
        lt_stage(Ys, Y, q0, nq, E, k0, tid);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < LT_BK / 4; ++ks) {
            const float a0 = Xs[ks * 4 + g][wm * 32 + c], a1 = Xs[ks * 4 + g][wm * 32 + 16 + c];
            const float b0 = Ys[ks * 4 + g][wn * 32 + c], b1 = Ys[ks * 4 + g][wn * 32 + 16 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of the 16x16 MFMA: col = lane & 15, row = 4*(lane >> 4) + reg
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) Z[wm * 32 + 16 * i + 4 * g + r][wn * 32 + 16 * j + c] = acc[i][j][r];
}

// ---------------------------------------------------------------------------------------------- backward walk
// the [jt0, jt1) share of the other side's 64-row tiles that split blockIdx.y of gridDim.y walks
__device__ __forceinline__ void lt_split_range(int nq, int& jt0, int& jt1) {
    const int ntq = (nq + LT_T - 1) / LT_T;
    const int per = (ntq + gridDim.y - 1) / gridDim.y;
    jt0 = blockIdx.y * per;
    jt1 = min(ntq, jt0 + per);
}

// this wave's 16 x 64 slice of the tile at (p0, q0), depth E: wave w owns rows 16w..16w+15 against the tile's four 16-column
// groups, z[t] in the C/D map (col = lane & 15, row = 4*(lane >> 4) + reg).  The caller's lane coordinates are passed in.
__device__ __forceinline__ void lt_slab(f32x4 (&z)[4], float (&Xs)[LT_BK][LT_LD], float (&Ys)[LT_BK][LT_LD],
                                        const float* __restrict__ X, const float* __restrict__ Y, int p0, int np, int q0, int nq,
                                        int E, int tid, int wave, int g, int c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) z[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += LT_BK) {
        lt_stage(Xs, X, p0, np, E, k0, tid);
        lt_stage(Ys, Y, q0, nq, E, k0, tid);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < LT_BK / 4; ++ks) {
            const float a = Xs[ks * 4 + g][16 * wave + c];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                z[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Ys[ks * 4 + g][16 * t + c], z[t], 0, 0, 0);
        }
        __syncthreads();
    }
}

// product: acc[16 rows x E] += dZ[16 x 64] . Q_tile[64 x E] for this wave's rows of dZs, Q staged EC columns at a time through
// Qe.  dZs has stride 66 (the A-operand read, row = lane & 15, k = lane >> 4, is conflict-free), Qe a stride == 16 (mod 32) as
// the k-major operand images.  Ends on a barrier: dZs and Qe are free again.
template <int NE>
__device__ __forceinline__ void lt_product(f32x4 (&acc)[NE], const float (&dZs)[LT_T][LT_T + 2], float (&Qe)[LT_T][lt_ec(NE) + 16],
                                           const float* __restrict__ Q, int q0, int nq, int tid, int wave, int g, int c) {
    constexpr int E = 16 * NE, EC = lt_ec(NE), TC = EC / 16;    // TC: accumulator tiles per chunk
#pragma unroll
    for (int ec = 0; ec < NE / TC; ++ec) {
        __syncthreads();                            // Qe free (previous chunk consumed); dZs rows of this wave written
        for (int i = tid; i < LT_T * (EC / 4); i += 256) {
            const int row = i / (EC / 4), c4 = (i % (EC / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q0 + row < nq) v = load4(Q + (long)(q0 + row) * E + ec * EC + c4);
            Qe[row][c4] = v.x; Qe[row][c4 + 1] = v.y; Qe[row][c4 + 2] = v.z; Qe[row][c4 + 3] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int kc = 0; kc < LT_T / 4; ++kc) {
            const float a = dZs[16 * wave + c][4 * kc + g];
#pragma unroll
            for (int t = 0; t < TC; ++t)
                acc[ec * TC + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Qe[4 * kc + g][16 * t + c], acc[ec * TC + t], 0, 0, 0);
        }
    }
    __syncthreads();
}

// this block's share of dP (the walk over q tiles is split over gridDim.y blocks): dP_part[blockIdx.y][p][e] = osc * acc for
// the lane's rows prow[] < np, summed over the splits by lt_split_sum
template <int NE>
__device__ __forceinline__ void lt_store_part(float* __restrict__ dP_part, const f32x4 (&acc)[NE], const int (&prow)[4], int np,
                                              float osc, int c) {
#pragma unroll
    for (int t = 0; t < NE; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = prow[r];
            if (p < np) dP_part[((long)blockIdx.y * np + p) * (16 * NE) + 16 * t + c] = osc * acc[t][r];
        }
}

// block partials -> 4 waves -> one float (fixed order)
__device__ __forceinline__ float lt_block_sum(float v, float* red, int wave, int lane) {
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// blocks over the q tiles of one row tile, about `target` blocks in all (768: ~3 blocks per CU in flight for the walks with a product)
static inline int lt_split(int np, int nq, int target) {
    const int tp = cdiv(np, LT_T), tq = cdiv(nq, LT_T);
    int split = cdiv(target, tp);
    if (split > tq) split = tq;
    if (split < 1) split = 1;
    return split;
}

// ---------------------------------------------------------------------------------------------- fixed-order sums
// out[j] = (accumulate ? out[j] : 0) + m * sum_k part[k*n + j], k in order; m = the product of *mul_dev and *mul2_dev where
// given (1 when neither is)
static __global__ __launch_bounds__(256) void lt_split_sum_kernel(int nsplit, long n, const float* __restrict__ part,
                                                                  const float* __restrict__ mul_dev,
                                                                  const float* __restrict__ mul2_dev, int accumulate,
                                                                  float* __restrict__ out) {
    float m = 1.f;
    if (mul_dev) m *= mul_dev[0];
    if (mul2_dev) m *= mul2_dev[0];
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        float s = 0.f;
        for (int k = 0; k < nsplit; ++k) s += part[k * n + j];
        out[j] = accumulate ? out[j] + m * s : m * s;
    }
}

static inline void lt_split_sum(int nsplit, long n, const float* part, const float* mul_dev, const float* mul2_dev,
                                int accumulate, float* out, hipStream_t stream) {
    int grid = cdiv(n, 256);
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(lt_split_sum_kernel, dim3(grid), dim3(256), 0, stream, nsplit, n, part, mul_dev, mul2_dev, accumulate, out);
}

// out[k] += (sum_i part[i*K + k], i in order) [/ *div_dev] for the K interleaved sums of n block partials: launch K blocks of
// one thread (k = blockIdx.x keeps the loads scalar)
static __global__ void lt_sum_parts_kernel(int n, int K, const float* __restrict__ part, const float* __restrict__ div_dev,
                                           float* __restrict__ out) {
    const int k = blockIdx.x;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += part[i * K + k];
    out[k] += div_dev ? s / div_dev[0] : s;
}

// ---------------------------------------------------------------------------------------------- embed dims
// The fused kernels are instantiated for E = 16 * NE over this list; colxlip_amd/ops.py FUSED_CE_DIMS names the same dims and
// sends every other one to the materialised paths.
template <int... NE> struct lt_dims {};
using lt_fused_dims = lt_dims<1, 2, 4, 8, 16, 32, 40, 48, 64>;
#define LT_FUSED_DIMS_STR "16, 32, 64, 128, 256, 512, 640, 768, 1024"

template <class F, int... NE>
static int lt_dim_dispatch(int E, F& launch, lt_dims<NE...>) {
    return ((E == 16 * NE && (launch(std::integral_constant<int, NE>{}), true)) || ...) ? 0 : -1;
}

// launch(std::integral_constant<int, NE>{}) for the NE with E == 16 * NE; 0, or -1 when E is not a fused dim
template <class F>
static int fused_dim_dispatch(int E, F&& launch) { return lt_dim_dispatch(E, launch, lt_fused_dims{}); }

static inline bool is_fused_dim(int E) { return fused_dim_dispatch(E, [](auto) {}) == 0; }
