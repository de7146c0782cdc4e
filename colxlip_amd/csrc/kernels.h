// Internal launch prototypes shared between translation units of libclipx_hip.so.
#pragma once
#include "common.h"

struct EpiF32 {
    const float* bias;      // [N] added before act
    int act;                // activation applied to (acc+bias)
    float* preact;          // optional store of (acc+bias), ldc layout
    const float* act_u;     // optional: multiply by act'(act_u[m,n]) (fused GELU backward)
    int act_u_kind;
    const float* residual;  // optional add, ldc layout
    float alpha, beta;
};
struct EpiB16 {
    const float* bias;        // [N] fp32
    int act;
    bf16_t* preact;           // optional [M,N]
    const bf16_t* act_u;      // optional [M,N]: multiply by act'(u)
    int act_u_kind;
    const bf16_t* residual;   // optional [M,N]
    // MaxSim epilogue (gemm_nt_maxsim.h): no output tile; per (row, 64-column slot, segment) maximum + index inside the image
    // (per (row, image, slot half) below 64 tokens per image)
    float* ms_max;            // [2 * slots, ms_ld]   (ms_q < 64: [2 * images, ms_ld])
    unsigned short* ms_idx;   // the same shape
    int ms_q, ms_ld;          // tokens per image (>= 16), row stride of the two arrays
    // GELU'(pre-activation) on eight bits (gemm_epi.h, G8_*): written by the c_fc epilogue, read by the c_proj dgrad epilogue
    unsigned char* pre8;          // optional [M,N]
    const unsigned char* actu8;   // optional [M,N]
};

int launch_gemm_f32(int M, int N, int K, const float* A, long a_rs, long a_cs, const float* B, long b_rs, long b_cs,
                    float* C, long ldc, const EpiF32& epi, hipStream_t stream);
int launch_gemm_bf16_nt(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, void* out,
                        int out_dtype, hipStream_t stream);
int launch_gemm_bf16_nt5(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, bf16_t* out, int n_cu,
                         hipStream_t stream);   // 1 = does not apply
int launch_gemm_bf16_nt8p(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, void* out, int out_dtype,
                          int n_cu, hipStream_t stream);   // 1 = does not apply
int launch_gemm_bf16_nt8p_maxsim(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, hipStream_t stream);
int launch_gemm_fp8_nt(int M, int N, int K, const unsigned char* X, const int* xe, const unsigned char* W, const int* we,
                       const EpiB16& epi, bf16_t* out, hipStream_t stream);
int launch_gemm_fp8_nt8p_maxsim(int M, int N, int K, const unsigned char* X, const int* xe, const unsigned char* W, const int* we,
                                const EpiB16& epi, hipStream_t stream);   // 1 = does not apply
int launch_gemm_bf16_tn(int M, int N, int K, const bf16_t* DY, const bf16_t* X, float* dw, float beta, float* db,
                        float beta_b, void* ws, size_t ws_bytes, hipStream_t stream);
size_t gemm_bf16_tn_ws_bytes(int M, int N, int K);
// grouped wgrad (up to 4 problems over the same M rows as one grid); launch returns 1 when the grouped kernel does not apply
size_t gemm_bf16_tn_group_ws_bytes(int M, int nprob, const int* N, const int* K);
int launch_gemm_bf16_tn_group(int M, int nprob, const int* N, const int* K, const bf16_t* const* DY, const bf16_t* const* X,
                              float* const* dw, const float* beta, float* const* db, const float* beta_b, void* ws,
                              size_t ws_bytes, hipStream_t stream);

// ---- LDS / MFMA fragment helpers (device) ------------------------------------------------
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((const GLOBAL_PTR(void))gsrc, (LDS_PTR(void))lds_dst, 16, 0, 0);
}
// one LDS-DMA piece through a buffer descriptor (a plain __device__ function: inside a kernel's nested generic lambdas the
// builtin silently suppressed the HOST-side instantiation of the whole kernel template -- undefined stubs at load time)
__device__ __forceinline__ void lds_dma_piece(__amdgpu_buffer_rsrc_t rsrc, char* lds_dst, unsigned voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (LDS_PTR(void))lds_dst, 16, voff, soff, 0, 0);
}

__device__ __forceinline__ bf16x8 lds_read8(const char* p) { return *reinterpret_cast<const bf16x8*>(p); }

__device__ __forceinline__ bf16x8 lds_tr8(const char* p0, const char* p1) {
    // two transposed 4-row reads -> the 8 reduction-index elements of a 16x16x32 operand
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))p0);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))p1);
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo;
    u.s.b = hi;
    return u.v;
}

