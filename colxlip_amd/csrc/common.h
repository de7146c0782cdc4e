// Shared device/host helpers for libclipx_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/clipx.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

#define LDS_PTR(T) __attribute__((address_space(3))) T*
#define GLOBAL_PTR(T) __attribute__((address_space(1))) T*

void clipx_set_error(const char* fmt, ...);

#define CLIPX_CHECK(cond, ...)                 \
    do {                                       \
        if (!(cond)) {                         \
            clipx_set_error(__VA_ARGS__);      \
            return -1;                         \
        }                                      \
    } while (0)

#define CLIPX_LAUNCH_CHECK()                                                   \
    do {                                                                       \
        hipError_t e_ = hipGetLastError();                                     \
        if (e_ != hipSuccess) {                                                \
            clipx_set_error("%s:%d launch failed: %s", __FILE__, __LINE__,     \
                            hipGetErrorString(e_));                            \
            return -2;                                                         \
        }                                                                      \
    } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// CUs the persistent GEMM grids are sized by: the device's count (256 when HIP cannot say), rounded down to a multiple of 8
// (blocks are dealt round-robin over the 8 XCDs), at least 8.  honour_switch: the experiment CLIPX_GEMM_CUS=<n>, persistent
// grids of fewer blocks than CUs, applies.
static inline int clipx_num_cu(bool honour_switch) {
    static int cached[2] = {0, 0};
    int& n_cu = cached[honour_switch ? 1 : 0];
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
        if (n_cu <= 0) n_cu = 256;
        n_cu = (n_cu / 8) * 8;
        if (n_cu < 8) n_cu = 8;
        const char* e = honour_switch ? getenv("CLIPX_GEMM_CUS") : nullptr;
        if (e && atoi(e) >= 8 && atoi(e) < n_cu) n_cu = (atoi(e) / 8) * 8;
    }
    return n_cu;
}

// ---- element access: T in {float, bf16_t}; math always in fp32 -----------------------
template <typename T> __device__ __forceinline__ float to_f(T v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f(float v) { return (T)v; }

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const bf16_t* p) {
    bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void store4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void store4(bf16_t* p, float4 v) {
    bf16x4 o;
    o[0] = (bf16_t)v.x; o[1] = (bf16_t)v.y; o[2] = (bf16_t)v.z; o[3] = (bf16_t)v.w;
    *reinterpret_cast<bf16x4*>(p) = o;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// activations (transformer.py:32-35 QuickGELU; nn.GELU = exact erf form)
__device__ __forceinline__ float act_fwd(int act, float x) {
    if (act == CLIPX_ACT_GELU) return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
    if (act == CLIPX_ACT_QUICKGELU) return x / (1.0f + __expf(-1.702f * x));
    return x;
}
__device__ __forceinline__ float act_bwd(int act, float x) {
    if (act == CLIPX_ACT_GELU) {
        float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
        float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
        return cdf + x * pdf;
    }
    if (act == CLIPX_ACT_QUICKGELU) {
        float s = 1.0f / (1.0f + __expf(-1.702f * x));
        return s * (1.0f + 1.702f * x * (1.0f - s));
    }
    return 1.0f;
}

// Fast GELU for the bf16 kernels: erf by Abramowitz-Stegun 7.1.26 (|error| < 1.5e-7, far below bf16 resolution),
// one v_exp + one v_rcp + 6 FMAs instead of libm erff; exp(-x^2/2) is shared with the Gaussian pdf of GELU'.
__device__ __forceinline__ void gelu_cdf_pdf(float x, float& cdf, float& pdf) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
    const float e = __expf(-z * z);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float erf_abs = 1.0f - poly * e;
    cdf = 0.5f * (1.0f + copysignf(erf_abs, x));
    pdf = 0.39894228040143267794f * e;
}
__device__ __forceinline__ float act_fwd_fast(int act, float x) {
    if (act == CLIPX_ACT_GELU) {
        float cdf, pdf;
        gelu_cdf_pdf(x, cdf, pdf);
        return x * cdf;
    }
    if (act == CLIPX_ACT_QUICKGELU) return x * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x));
    return x;
}
__device__ __forceinline__ float act_bwd_fast(int act, float x) {
    if (act == CLIPX_ACT_GELU) {
        float cdf, pdf;
        gelu_cdf_pdf(x, cdf, pdf);
        return cdf + x * pdf;
    }
    if (act == CLIPX_ACT_QUICKGELU) {
        const float s = __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x));
        return s * (1.0f + 1.702f * x * (1.0f - s));
    }
    return 1.0f;
}
// Polynomial GELU for the GEMM epilogues (two values per packed-fp32 instruction, no transcendental):
//   Phi(x) - 0.5 = xc * Q(s),  GELU'(x) - 0.5 = xc * R(s),  xc = clamp(x, -4.5, 4.5), s = xc^2,
// Q, R degree 9 in s (scripts/fit_gelu.py: max abs error 8e-5 for GELU, 2.6e-4 for GELU' in fp32 Horner form).  The exp + rcp
// forms above cost ~2.5x the VALU time.
// Round 4, measured and REJECTED: polynomials "fitted to the bf16 output" -- Q degree 6 clamped at 3.80 (2.5e-4), R degree 7 at 4.00
// (2.7e-4); -DCLIPX_GELU_LOWDEG=1 builds them.  (a) They buy 1.5-2 % on the two GELU GEMMs, not the 20 % their share of the
// epilogue's VALU instructions suggests: the polynomial is a quarter of what those epilogues cost, the pre-activation's store and
// read-back are the rest (scripts/bench_epi.py: fc bias 0.896 ms, + GELU 0.939, + pre-activation store 1.051) -- see G8_* in
// gemm_epi.h for what was done about THAT.  (b) An approximation error is not rounding noise: it is the same function of u in every
// layer.  On ViT-L/14-336 (24 blocks) the first-layer gradient norms moved from 0.7 % to 4.4-4.6 % off the reference
// (profiles/r04_ablation_gelu.txt), outside the 3 % the bf16 parity tests allow; ViT-B/32's 12 blocks stayed inside.  Scalar
// v_fma_f32 instead of v_pk_fma_f32 (-DCLIPX_GELU_UNPACK=1; the packed form is an anti-lever BESIDE MFMAs, but both waves of a
// SIMD are in their epilogues at once here) measured 1-3 % slower.
typedef __attribute__((ext_vector_type(2))) float f32x2;
#ifndef CLIPX_GELU_LOWDEG
#define CLIPX_GELU_LOWDEG 0
#endif
#ifndef CLIPX_GELU_UNPACK
#define CLIPX_GELU_UNPACK 0
#endif
#if !CLIPX_GELU_LOWDEG
#define CLIPX_GELU_QD 9
#define CLIPX_GELU_RD 9
#define CLIPX_GELU_QX0 4.5f
#define CLIPX_GELU_RX0 4.5f
#define CLIPX_GELU_Q {3.989246741e-01f, -6.642068731e-02f, 9.891780975e-03f, -1.142718240e-03f, 1.017347828e-04f, \
                      -6.813823852e-06f, 3.279000976e-07f, -1.056747898e-08f, 2.022538949e-10f, -1.726437751e-12f}
#define CLIPX_GELU_R {7.976261673e-01f, -2.649257722e-01f, 5.860940169e-02f, -8.815904631e-03f, 9.405530695e-04f, \
                      -7.122351675e-05f, 3.722063937e-06f, -1.268116212e-07f, 2.521483450e-09f, -2.210983774e-11f}
#else
#define CLIPX_GELU_QD 6
#define CLIPX_GELU_RD 7
#define CLIPX_GELU_QX0 3.8f
#define CLIPX_GELU_RX0 4.0f
#define CLIPX_GELU_Q {3.986767257e-01f, -6.571974143e-02f, 9.316605391e-03f, -9.315394851e-04f, 6.068374521e-05f, \
                      -2.272396882e-06f, 3.665624856e-08f}
#define CLIPX_GELU_R {7.967215709e-01f, -2.620296498e-01f, 5.591467279e-02f, -7.687389655e-03f, 6.876364868e-04f, \
                      -3.845875696e-05f, 1.213768810e-06f, -1.641910750e-08f}
#endif
// N pairs at once with the Horner steps of the independent pairs interleaved: back-to-back DEPENDENT packed-fp32 ops
// cost a wait state each on gfx950 (the compiler emits s_nop between them).
template <int NP, int D>
__device__ __forceinline__ void gelu_poly_core(const f32x2 (&x)[NP], const float (&c)[D + 1], float x0, f32x2 (&xc)[NP], f32x2 (&r)[NP]) {
    f32x2 s[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        xc[p][0] = __builtin_amdgcn_fmed3f(x[p][0], -x0, x0);
        xc[p][1] = __builtin_amdgcn_fmed3f(x[p][1], -x0, x0);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) s[p] = xc[p] * xc[p];
#if CLIPX_GELU_UNPACK
    // scalar FMAs, kept scalar: the optimiser would SLP-pack two adjacent fmaf into one v_pk_fma_f32 again
#pragma unroll
    for (int p = 0; p < NP; ++p) r[p] = (f32x2){c[D], c[D]};
#pragma unroll
    for (int k = D - 1; k >= 0; --k)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float a = r[p][0], b = r[p][1];
            asm("v_fma_f32 %0, %1, %2, %3" : "=v"(a) : "v"(a), "v"(s[p][0]), "v"(c[k]));
            asm("v_fma_f32 %0, %1, %2, %3" : "=v"(b) : "v"(b), "v"(s[p][1]), "v"(c[k]));
            r[p][0] = a;
            r[p][1] = b;
        }
#else
#pragma unroll
    for (int p = 0; p < NP; ++p) r[p] = (f32x2){c[D], c[D]};
#pragma unroll
    for (int k = D - 1; k >= 0; --k)
#pragma unroll
        for (int p = 0; p < NP; ++p) r[p] = r[p] * s[p] + (f32x2){c[k], c[k]};
#endif
}
// x[p] <- GELU(x[p])
template <int NP>
__device__ __forceinline__ void gelu_fwd_polyN(f32x2 (&x)[NP]) {
    const float q[CLIPX_GELU_QD + 1] = CLIPX_GELU_Q;
    f32x2 xc[NP], r[NP];
    gelu_poly_core<NP, CLIPX_GELU_QD>(x, q, CLIPX_GELU_QX0, xc, r);
#pragma unroll
    for (int p = 0; p < NP; ++p) x[p] = x[p] * (xc[p] * r[p] + (f32x2){0.5f, 0.5f});
}
// u[p] <- GELU'(u[p])
template <int NP>
__device__ __forceinline__ void gelu_bwd_polyN(f32x2 (&u)[NP]) {
    const float q[CLIPX_GELU_RD + 1] = CLIPX_GELU_R;
    f32x2 xc[NP], r[NP];
    gelu_poly_core<NP, CLIPX_GELU_RD>(u, q, CLIPX_GELU_RX0, xc, r);
#pragma unroll
    for (int p = 0; p < NP; ++p) u[p] = xc[p] * r[p] + (f32x2){0.5f, 0.5f};
}
// u[p] <- A * GELU'(u[p]) + B with A folded into the coefficients (the 8-bit quantiser of gemm_epi.h: no separate scaling pass)
template <int NP>
__device__ __forceinline__ void gelu_bwd_polyN_affine(f32x2 (&u)[NP], float a, float b) {
    const float q0[CLIPX_GELU_RD + 1] = CLIPX_GELU_R;
    float q[CLIPX_GELU_RD + 1];
#pragma unroll
    for (int k = 0; k <= CLIPX_GELU_RD; ++k) q[k] = q0[k] * a;
    f32x2 xc[NP], r[NP];
    gelu_poly_core<NP, CLIPX_GELU_RD>(u, q, CLIPX_GELU_RX0, xc, r);
    const float off = 0.5f * a + b;
#pragma unroll
    for (int p = 0; p < NP; ++p) u[p] = xc[p] * r[p] + (f32x2){off, off};
}
// activation / activation derivative of two accumulator quads at once (bf16 kernels)
__device__ __forceinline__ void act_fwd_quads(int act, float4& a, float4& b) {
    if (act == CLIPX_ACT_GELU) {
        f32x2 x[4] = {{a.x, a.y}, {a.z, a.w}, {b.x, b.y}, {b.z, b.w}};
        gelu_fwd_polyN<4>(x);
        a = make_float4(x[0][0], x[0][1], x[1][0], x[1][1]);
        b = make_float4(x[2][0], x[2][1], x[3][0], x[3][1]);
    } else {
        a.x = act_fwd_fast(act, a.x); a.y = act_fwd_fast(act, a.y); a.z = act_fwd_fast(act, a.z); a.w = act_fwd_fast(act, a.w);
        b.x = act_fwd_fast(act, b.x); b.y = act_fwd_fast(act, b.y); b.z = act_fwd_fast(act, b.z); b.w = act_fwd_fast(act, b.w);
    }
}
__device__ __forceinline__ void act_bwd_quads(int act, float4& ua, float4& ub) {   // u -> act'(u), in place
    if (act == CLIPX_ACT_GELU) {
        f32x2 x[4] = {{ua.x, ua.y}, {ua.z, ua.w}, {ub.x, ub.y}, {ub.z, ub.w}};
        gelu_bwd_polyN<4>(x);
        ua = make_float4(x[0][0], x[0][1], x[1][0], x[1][1]);
        ub = make_float4(x[2][0], x[2][1], x[3][0], x[3][1]);
    } else {
        ua.x = act_bwd_fast(act, ua.x); ua.y = act_bwd_fast(act, ua.y); ua.z = act_bwd_fast(act, ua.z); ua.w = act_bwd_fast(act, ua.w);
        ub.x = act_bwd_fast(act, ub.x); ub.y = act_bwd_fast(act, ub.y); ub.z = act_bwd_fast(act, ub.z); ub.w = act_bwd_fast(act, ub.w);
    }
}

template <typename T> __device__ __forceinline__ float act_bwd_t(int act, float x);
template <> __device__ __forceinline__ float act_bwd_t<float>(int act, float x) { return act_bwd(act, x); }
template <> __device__ __forceinline__ float act_bwd_t<bf16_t>(int act, float x) { return act_bwd_fast(act, x); }
