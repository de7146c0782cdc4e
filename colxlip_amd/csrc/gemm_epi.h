// Pieces shared by the bf16 NT GEMM kernels: epilogue flags, bf16 pack/unpack, the compile-time-specialised epilogue
// arithmetic, static_for.
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "kernels.h"

enum { F_BIAS = 1, F_RES = 2, F_ACTU = 4, F_ACT = 8, F_PRE = 16, F_MAXSIM = 32, F_PRE8 = 64, F_ACTU8 = 128,
       F_MAXSIM_SEG = 256 };   // with F_MAXSIM: the per-image form for fewer than 64 tokens per image (gemm_nt_maxsim.h)

// GELU'(u) on EIGHT bits (round 4).  What the c_fc epilogue costs beyond its bias form is not the polynomial but the second
// store -- fc bias 0.896 ms, + GELU 0.939, + bf16 pre-activation store 1.051 (scripts/bench_epi.py, ViT-B/32 vision shape at
// b = 4096) -- and what the c_proj dgrad costs beyond its plain form is reading that tensor back.  The backward needs the
// pre-activation for one thing only: the factor GELU'(u) in [-0.129, 1.129].  So the forward epilogue evaluates that factor
// itself (from the fp32 accumulator + bias, not from a bf16-rounded u) and stores it as a byte, b = round((g - LO) / STEP),
// STEP = 0.005: absolute error <= 0.0025, what bf16 has at g ~ 0.6 and half of what it has at g ~ 1, where most of the
// gradient's mass is; the dgrad epilogue multiplies by LO + STEP b and evaluates nothing.  Half the bytes both ways, one
// polynomial less in the backward, one byte per element less kept per block.
// LO and STEP put the two values the factor SATURATES at on the grid: 0 = byte 26, 1 = byte 226 (max 1.145).  With the first choice
// (STEP = 1.26 / 255) a saturated 1 decoded to 1.0015 and a saturated 0 to -0.0015 -- a +0.15 % bias on most of the gradient's
// mass in every layer: ViT-L/14-336's first-layer gradient norms came out 4.8 % off after 24 layers (1.8 % with bf16 u).
#define G8_LO (-0.13f)
#define G8_STEP (0.005f)
#define G8_INV (200.0f)
// t = (g - LO) / STEP per value -> four bytes (byte e = column e).  v_cvt_pk_u8_f32 rounds to nearest and saturates (measured:
// with + 0.5 in front of it the decoded factor was off by up to a whole step).
__device__ __forceinline__ unsigned g8_pack_scaled(const float4& t) {
    unsigned w = 0;
    w = __builtin_amdgcn_cvt_pk_u8_f32(t.x, 0, w);
    w = __builtin_amdgcn_cvt_pk_u8_f32(t.y, 1, w);
    w = __builtin_amdgcn_cvt_pk_u8_f32(t.z, 2, w);
    w = __builtin_amdgcn_cvt_pk_u8_f32(t.w, 3, w);
    return w;
}
__device__ __forceinline__ float4 g8_unpack(unsigned w) {
    return make_float4(fmaf((float)(w & 0xffu), G8_STEP, G8_LO), fmaf((float)((w >> 8) & 0xffu), G8_STEP, G8_LO),
                       fmaf((float)((w >> 16) & 0xffu), G8_STEP, G8_LO), fmaf((float)(w >> 24), G8_STEP, G8_LO));
}

typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;


__device__ __forceinline__ unsigned pack2(float a, float b) {
    union { __attribute__((ext_vector_type(2))) bf16_t v; unsigned u; } x;
    x.v[0] = (bf16_t)a;
    x.v[1] = (bf16_t)b;
    return x.u;
}
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }


// 16-byte store of output-tile data.  NT_STORE_SC1: `sc1` stores do not leave the written line in the XCD's L2
// (MI355X_MICROARCH.md, stores of each flavour), so a tile's 128 KiB of output does not evict the weight / activation
// lines the XCD's other tiles are about to re-read.  The asm form is one VMEM store like the plain one: the counted
// s_waitcnt vmcnt(N) bookkeeping of the k-loops is unchanged.
#ifndef NT_STORE_SC1
#define NT_STORE_SC1 0
#endif
__device__ __forceinline__ void nt_store16(void* p, const u32x4& v) {
#if NT_STORE_SC1
    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
#else
    *reinterpret_cast<u32x4*>(p) = v;
#endif
}

// m-panels per walk block of the NT kernels' tile order (see `coords` there): an XCD walks gm m-panels x all n-tiles at a time,
// n-tile by n-tile, so a weight tile is fetched once per gm panels.  Measured twice.  With the one-barrier kernels
// (profiles/r02_ablation_tile_order_stores.txt) gm = 8 moved FETCH_SIZE (c_fc -20 %, other shapes +7..+20 %) but not the time
// (0.982 vs 0.983 ms): those kernels were not bound by that traffic.  With the ping-pong kernel (profiles/
// r02_ablation_pingpong.txt (7)) the loads are closer to the critical path and gm = 4 / 8 is 1.4 % faster over the 16 NT
// shapes (8.63 vs 8.75 ms; c_fc forward 1100 -> 1146 TFLOP/s, c_proj dgrad 1120 -> 1165): default 4 when there are enough
// m-panels to walk.  CLIPX_NT_GM=<n> selects another block height.
static inline int nt_pick_gm(int N, int K, int tiles_m = 1 << 30) {
    static int forced = -1;
    if (forced < 0) { const char* e = getenv("CLIPX_NT_GM"); forced = e ? atoi(e) : 0; }
    (void)N; (void)K;
    if (forced >= 1 && forced <= 32) return forced;
    return tiles_m >= 64 ? 4 : 1;
}

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// the epilogue arithmetic on TWO accumulator quads (4 consecutive n of one m each), flags known at compile time
// (F_PRE8: pre_lo[h] receives the four GELU' bytes of quad h; F_ACTU8: u_lo[h] holds them)
template <int FL, int ACT>
__device__ __forceinline__ void epi_math2(float4 (&v)[2], const float4 (&b)[2], const unsigned (&u_lo)[2],
                                          const unsigned (&u_hi)[2], const unsigned (&r_lo)[2], const unsigned (&r_hi)[2],
                                          unsigned (&pre_lo)[2], unsigned (&pre_hi)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if constexpr ((FL & F_BIAS) != 0) { v[h].x += b[h].x; v[h].y += b[h].y; v[h].z += b[h].z; v[h].w += b[h].w; }
        if constexpr ((FL & F_PRE) != 0) {
            pre_lo[h] = pack2(v[h].x, v[h].y);
            pre_hi[h] = pack2(v[h].z, v[h].w);
        }
    }
    if constexpr ((FL & F_PRE8) != 0) {
        static_assert(ACT == CLIPX_ACT_GELU, "the 8-bit derivative is built for GELU");
        f32x2 x[4] = {{v[0].x, v[0].y}, {v[0].z, v[0].w}, {v[1].x, v[1].y}, {v[1].z, v[1].w}};
        gelu_bwd_polyN_affine<4>(x, G8_INV, -G8_LO * G8_INV);        // (GELU'(v) - LO) / STEP, the scale inside the coefficients
        pre_lo[0] = g8_pack_scaled(make_float4(x[0][0], x[0][1], x[1][0], x[1][1]));
        pre_lo[1] = g8_pack_scaled(make_float4(x[2][0], x[2][1], x[3][0], x[3][1]));
    }
    if constexpr ((FL & F_ACTU8) != 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 d = g8_unpack(u_lo[h]);
            v[h].x *= d.x; v[h].y *= d.y; v[h].z *= d.z; v[h].w *= d.w;
        }
    }
    if constexpr ((FL & F_ACT) != 0) act_fwd_quads(ACT, v[0], v[1]);
    if constexpr ((FL & F_ACTU) != 0) {
        float4 d0 = make_float4(bf_lo(u_lo[0]), bf_hi(u_lo[0]), bf_lo(u_hi[0]), bf_hi(u_hi[0]));
        float4 d1 = make_float4(bf_lo(u_lo[1]), bf_hi(u_lo[1]), bf_lo(u_hi[1]), bf_hi(u_hi[1]));
        act_bwd_quads(ACT, d0, d1);
        v[0].x *= d0.x; v[0].y *= d0.y; v[0].z *= d0.z; v[0].w *= d0.w;
        v[1].x *= d1.x; v[1].y *= d1.y; v[1].z *= d1.z; v[1].w *= d1.w;
    }
    if constexpr ((FL & F_RES) != 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v[h].x += bf_lo(r_lo[h]); v[h].y += bf_hi(r_lo[h]);
            v[h].z += bf_lo(r_hi[h]); v[h].w += bf_hi(r_hi[h]);
        }
    }
}

