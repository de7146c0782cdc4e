// Eight-wave PING-PONG bf16 NT GEMM:  y[M,N] = epi(x[M,K] . w[N,K]^T), 256x256 tile, K % 64 == 0.
//
// The schedule, its hazard argument, the tile walk and the launch geometry are the engine's (gemm_nt_pp.h).  This file supplies
// what is bf16 about it: a k-step is 64 elements, a C segment is 2 x 32 v_mfma_f32_16x16x32_bf16 (the MFMA of gemm_bf16_nt.hip),
// and a tile ends in that kernel's epilogue (gemm_nt_epilogue.h) or in the MaxSim reduction (gemm_nt_maxsim.h).
#include "gemm_nt_pp.h"
#include "gemm_nt_epilogue.h"
#include "gemm_nt_maxsim.h"

struct PpBf16 {
    typedef bf16_t elem;
    typedef bf16x8 frag;
    // slice ks of a k-step is k 32 ks .. 32 ks + 31; lane group g holds k 8 g .. 8 g + 7 of it
    static __device__ __forceinline__ int chunk(int ks, int g) { return ks * 4 + g; }
    // fragments of slice s: F[12 s + i] = w-tile i (i < 4), F[12 s + 4 + j] = x-tile j
    template <bool FIRST>
    static __device__ __forceinline__ void mfma(f32x4 (&acc)[4][8], frag (&F)[24]) {
        static_for<0, 8>([&](auto jc) {
            constexpr int j_ = decltype(jc)::value;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (FIRST)
                    acc[i][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[i], F[4 + j_], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                else
                    acc[i][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[i], F[4 + j_], acc[i][j_], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        static_for<0, 8>([&](auto jc) {
            constexpr int j_ = decltype(jc)::value;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[12 + i], F[12 + 4 + j_], acc[i][j_], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
    }
};

#ifdef PP_PROFILE
// per wave: [0] total [1] epilogue [2] L segment [3] wait before the post-L barrier .. [4] C segment [5] vmcnt wait [6] barrier
// after C [7] k-steps
__device__ unsigned long long g_pp_dbg[64];
extern "C" int clipx_debug_nt8p(unsigned long long* out, int reset) {
    if (reset) {
        unsigned long long z[64] = {0};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_pp_dbg), z, sizeof(z));
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pp_dbg), 64 * sizeof(unsigned long long));
}
struct PpProbe {
    long t0 = clock64(), last = 0, sum[8] = {0, 0, 0, 0, 0, 0, 0, 1};
    __device__ __forceinline__ void tick() { last = clock64(); }
    template <int I>
    __device__ __forceinline__ void lap() {
        const long t = clock64();
        sum[I] += t - last;
        last = t;
        if constexpr (I == PP_T_VMCNT) ++sum[7];      // one counted wait per k-step
    }
    __device__ __forceinline__ void flush(int wave, int lane) {
        sum[0] = clock64() - t0;
        if (lane == 0)
            for (int i = 0; i < 8; ++i) atomicAdd(&g_pp_dbg[wave * 8 + i], (unsigned long long)sum[i]);
    }
};
#else
typedef PpNoProbe PpProbe;
#endif

template <typename OUT_T, int FL, int ACT>
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt8p_kernel(int M, int N, int K, const bf16_t* __restrict__ X,
                                                                const bf16_t* __restrict__ W, EpiB16 epi,
                                                                OUT_T* __restrict__ out, int tiles_m, int tiles_n, int gm) {
    pp_gemm_nt<PpBf16>(M, N, K, X, W, tiles_m, tiles_n, gm,
                       [&](f32x4 (&acc)[4][8], int m0, int n0, int wm, int wn, int lane) {
                           if constexpr ((FL & F_MAXSIM_SEG) != 0)
                               nt_maxsim_seg_epilogue<8>(acc, epi, M, N, m0, n0, wm, wn, lane);
                           else if constexpr ((FL & F_MAXSIM) != 0)
                               nt_maxsim_epilogue<8>(acc, epi, M, N, m0, n0, wm, wn, lane);
                           else
                               (void)nt_tile_epilogue<OUT_T, 8, FL, ACT>(acc, epi, out, M, N, m0, n0, wm, wn, lane);
                       },
                       PpProbe());
}

template <int FL, int ACT>
static int launch_pp(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, bf16_t* out, int n_cu,
                     hipStream_t stream) {
    return pp_launch<gemm_bf16_nt8p_kernel<bf16_t, FL, ACT>>(M, N, K, X, W, epi, out, n_cu, stream);
}

// S = X . W^T reduced on the fly to per-(row, slot, segment) maxima, per-(row, image, half) below 64 tokens per image
// (gemm_nt_maxsim.h); nothing else is written
int launch_gemm_bf16_nt8p_maxsim(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, hipStream_t stream) {
    if (K % 64 != 0 || K < 128 || (long)256 * K * 2 >= (1l << 31) || epi.ms_q < 16 || epi.ms_q > 65535) return 1;
    if (epi.ms_q < 64)
        return launch_pp<F_MAXSIM | F_MAXSIM_SEG, CLIPX_ACT_NONE>(M, N, K, X, W, epi, nullptr, clipx_num_cu(false), stream);
    return launch_pp<F_MAXSIM, CLIPX_ACT_NONE>(M, N, K, X, W, epi, nullptr, clipx_num_cu(false), stream);
}

// 1 = this kernel does not apply (the caller falls back to the one-barrier kernel)
int launch_gemm_bf16_nt8p(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, void* out, int out_dtype,
                          int n_cu, hipStream_t stream) {
    if (K % 64 != 0 || K < 128 || out_dtype != CLIPX_BF16) return 1;
    if ((long)256 * K * 2 >= (1l << 31)) return 1;
    int fl, act;
    if (!nt_epi_flags(epi, fl, act)) return 1;
#define PP_CASE(FLV, ACTV) \
    if (fl == (FLV) && act == (ACTV)) return launch_pp<(FLV), (ACTV)>(M, N, K, X, W, epi, (bf16_t*)out, n_cu, stream)
    NT_EPI_CASES(PP_CASE)
#undef PP_CASE
    return 1;
}
