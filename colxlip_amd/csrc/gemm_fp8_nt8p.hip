// fp8 (OCP e4m3) x fp8 NT GEMM on v_mfma_f32_16x16x128_f8f6f4 -- the CDNA4 matrix instruction that runs at twice the bf16 rate:
//     y[M,N] (bf16) = epi( 2^(xe[m] + we[n]) * sum_k x8[m,k] * w8[n,k] )
// x8 / w8: e4m3 bytes with one power-of-two exponent per row (activations: clipx_quant_rows_e4m3; weights:
// clipx_quant_weight_e4m3), products and sums exact / fp32 in the MFMA.  BASELINE.json config 5 ("fp8 weights, CDNA4 fp8 MFMA").
//
// The kernel is an instance of the eight-wave ping-pong engine (gemm_nt_pp.h: schedule, hazard argument, tile walk, launch
// geometry), as gemm_bf16_nt8p.hip is.  What is fp8 about it: a k-step is 128 elements, i.e. the SAME 128-byte rows, LDS image,
// rings and LDS-DMA pieces; a lane's MFMA operand is 32 consecutive k of one row = the two 16-byte chunks 2g, 2g+1 of the row (two
// ds_read_b128 into one 8-VGPR tuple), so a C segment is 32 MFMAs of 32 cycles: the same 1024 cycles as 64 bf16 MFMAs, for
// twice the K; and the row exponents are applied to the accumulators before the tile epilogue.
//
// The MaxSim instances (F_MAXSIM, F_MAXSIM_SEG) end a tile in the reductions of gemm_nt_maxsim.h instead: x8 = packed text rows,
// w8 = image tokens.  The column exponent we[n] differs per image token and therefore decides which token wins, so it has to be
// on the accumulators BEFORE the maximum; the row exponent is a positive factor and could follow it, but one scaling loop
// serves both.  The partial arrays are those of the bf16 instances, value for value in layout and tie rules.
#include "gemm_nt_pp.h"
#include "gemm_nt_epilogue.h"
#include "gemm_nt_maxsim.h"

typedef __attribute__((ext_vector_type(4))) int f8x16;      // 16 fp8 bytes
typedef __attribute__((ext_vector_type(8))) int f8x32;      // one lane's MFMA operand: 32 fp8 bytes

struct PpFp8 {
    typedef unsigned char elem;
    typedef f8x16 frag;
    // half ks (k 0..15 / 16..31 of the lane's 32) of lane group g: chunks 2g, 2g+1 = k 32g .. 32g+31
    static __device__ __forceinline__ int chunk(int ks, int g) { return 2 * g + ks; }
    // fragments of half h: F[12 h + i] = w-tile i (i < 4), F[12 h + 4 + j] = x-tile j
    template <bool FIRST>
    static __device__ __forceinline__ void mfma(f32x4 (&acc)[4][8], frag (&F)[24]) {
        static_for<0, 8>([&](auto jc) {
            constexpr int j_ = decltype(jc)::value;
            const f8x32 xb = __builtin_shufflevector(F[4 + j_], F[12 + 4 + j_], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f8x32 wa_ = __builtin_shufflevector(F[i], F[12 + i], 0, 1, 2, 3, 4, 5, 6, 7);
                if constexpr (FIRST)
                    acc[i][j_] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa_, xb, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0, 0, 0);
                else
                    acc[i][j_] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa_, xb, acc[i][j_], 0, 0, 0, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
};

struct F8Scales {
    const int* xe;      // [M] row exponents of x8
    const int* we;      // [N] row exponents of w8
};

template <typename OUT_T, int FL, int ACT>
__global__ __launch_bounds__(512, 2) void gemm_fp8_nt8p_kernel(int M, int N, int K, const unsigned char* __restrict__ X,
                                                                const unsigned char* __restrict__ W, EpiB16 epi,
                                                                OUT_T* __restrict__ out, int tiles_m, int tiles_n, int gm,
                                                               F8Scales sc) {
    pp_gemm_nt<PpFp8>(M, N, K, X, W, tiles_m, tiles_n, gm, [&](f32x4 (&acc)[4][8], int m0, int n0, int wm, int wn, int lane) {
        // the row exponents: acc[n-tile i][m-tile j][q] belongs to row 16j + c, column 16i + 4g + q of the wave's 128 x 64
        const int g = lane >> 4, c = lane & 15;
        const int m_base = m0 + wm * 128 + c, n_base = n0 + wn * 64 + 4 * g;
        if constexpr ((FL & F_MAXSIM) != 0) {
            // the same factors in two passes, columns then rows, read through buffer descriptors: one 32-bit offset per operand
            // instead of twelve 64-bit addresses beside the 128 accumulators (the form below spilled two VGPRs here), and an index
            // past the end reads exponent 0 without a clamp.  Powers of two, so the order of the factors changes no value.
            const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc((void*)sc.xe, 0, M * 4, 0x00020000);
            const __amdgpu_buffer_rsrc_t ce = __builtin_amdgcn_make_buffer_rsrc((void*)sc.we, 0, N * 4, 0x00020000);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float sq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    sq[q] = __builtin_ldexpf(1.0f, __builtin_amdgcn_raw_buffer_load_b32(ce, 4 * n_base + 4 * (16 * i + q), 0, 0));
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[i][j][q] *= sq[q];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float sr = __builtin_ldexpf(1.0f, __builtin_amdgcn_raw_buffer_load_b32(re, 4 * m_base + 64 * j, 0, 0));
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[i][j][q] *= sr;
            }
            if constexpr ((FL & F_MAXSIM_SEG) != 0)
                nt_maxsim_seg_epilogue<8>(acc, epi, M, N, m0, n0, wm, wn, lane);
            else
                nt_maxsim_epilogue<8>(acc, epi, M, N, m0, n0, wm, wn, lane);
            return;
        }
        float sr[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sr[j] = __builtin_ldexpf(1.0f, sc.xe[min(m_base + 16 * j, M - 1)]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float sq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) sq[q] = __builtin_ldexpf(1.0f, sc.we[min(n_base + 16 * i + q, N - 1)]);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][j][q] *= sr[j] * sq[q];
        }
        (void)nt_tile_epilogue<OUT_T, 8, FL, ACT>(acc, epi, out, M, N, m0, n0, wm, wn, lane);
    });
}

// S = 2^(xe[m] + we[n]) * X8 . W8^T reduced on the fly to the MaxSim partials (gemm_nt_maxsim.h), as
// launch_gemm_bf16_nt8p_maxsim does for bf16 operands; nothing else is written.  1 = this kernel does not apply.
int launch_gemm_fp8_nt8p_maxsim(int M, int N, int K, const unsigned char* X, const int* xe, const unsigned char* W, const int* we,
                                const EpiB16& epi, hipStream_t stream) {
    if (K % 128 != 0 || K < 256 || (long)256 * K >= (1l << 31) || epi.ms_q < 16 || epi.ms_q > 65535 || N % 8 != 0) return 1;
    if (((uintptr_t)X % 16 != 0) || ((uintptr_t)W % 16 != 0)) return 1;
    if (M <= 0 || N <= 0) return 0;
    const F8Scales sc{xe, we};
    if (epi.ms_q < 64)
        return pp_launch<gemm_fp8_nt8p_kernel<bf16_t, F_MAXSIM | F_MAXSIM_SEG, CLIPX_ACT_NONE>>(
            M, N, K, X, W, epi, (bf16_t*)nullptr, clipx_num_cu(false), stream, sc);
    return pp_launch<gemm_fp8_nt8p_kernel<bf16_t, F_MAXSIM, CLIPX_ACT_NONE>>(M, N, K, X, W, epi, (bf16_t*)nullptr,
                                                                             clipx_num_cu(false), stream, sc);
}

// y = epi(x8 . w8^T) for e4m3 operands with per-row exponents; bf16 output.  Needs K % 128 == 0.
int launch_gemm_fp8_nt(int M, int N, int K, const unsigned char* X, const int* xe, const unsigned char* W, const int* we,
                       const EpiB16& epi, bf16_t* out, hipStream_t stream) {
    CLIPX_CHECK(K % 128 == 0 && K >= 256 && N % 8 == 0, "fp8 NT GEMM needs K %% 128 == 0, K >= 256, N %% 8 == 0 (K=%d N=%d)", K, N);
    CLIPX_CHECK(((uintptr_t)X % 16 == 0) && ((uintptr_t)W % 16 == 0) && ((uintptr_t)out % 16 == 0),
                "fp8 NT GEMM: operands must be 16-B aligned");
    CLIPX_CHECK((long)256 * K < (1l << 31), "fp8 NT GEMM: K too large");
    if (M <= 0 || N <= 0) return 0;
    const int n_cu = clipx_num_cu(false);
    const F8Scales sc{xe, we};
    int fl, act;
    CLIPX_CHECK(nt_epi_flags(epi, fl, act), "fp8 NT GEMM: act and act_u are mutually exclusive");
    CLIPX_CHECK(!epi.ms_max, "fp8 NT GEMM: the MaxSim epilogue has its own launch (launch_gemm_fp8_nt8p_maxsim)");
#define F8_CASE(FLV, ACTV)             \
    if (fl == (FLV) && act == (ACTV)) \
    return pp_launch<gemm_fp8_nt8p_kernel<bf16_t, (FLV), (ACTV)>>(M, N, K, X, W, epi, out, n_cu, stream, sc)
    NT_EPI_CASES(F8_CASE)
#undef F8_CASE
    clipx_set_error("fp8 NT GEMM: epilogue combination not built (flags %d, act %d)", fl, act);
    return -1;
}
