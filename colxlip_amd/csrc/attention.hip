// Attention core of nn.MultiheadAttention (reference transformer.py:253-255, mask :960-966).
// Sequences here are short (50 / 77 / 197 tokens): one workgroup owns one (sample, head) with the
// whole sequence resident in LDS, so scores never touch HBM and the kernels are HBM-bound on
// qkv / dout / dqkv traffic.
//
// bf16 kernels (head dim 64, L <= 128; longer sequences and head dim 80 on the online-softmax kernels further down): all products
// on v_mfma_f32_16x16x32_bf16, arranged so that no computed tile ever moves between lanes:
//   S^T = K.Q^T       (key rows in registers, query on the lane)  -> softmax is lane-local + 2 shuffles
//   O^T = V^T.P^T     A operand = V read through ds_read_b64_tr_b16, B operand = the S^T accumulator itself
// and in backward the same trick in both orientations (dQ from S^T/dP^T tiles, dK/dV from S/dP tiles).
// LDS image of a [rows][64] bf16 operand: 128-B rows, 16-B chunk c stored at c ^ (((row>>1)&3)<<1):
// conflict-free for both the row reads (ds_read_b128) and the transposed reads.
// fp32 kernels (parity mode): one thread per query / key row, exact expf, any head dim in {32,64,80}.
#include <stdlib.h>
#include "kernels.h"

// =============================================================================== fp32 parity kernels
template <int HD>
__global__ __launch_bounds__(128) void attn_f32_fwd_kernel(int L, int heads, int causal,
                                                           const float* __restrict__ qkv, float* __restrict__ out,
    const int* __restrict__ seq_ids, const int* __restrict__ cu_rows) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    long row0 = (long)b * L;
    if (cu_rows) {           // packed rows: this block's sequence starts at cu_rows[s] and has cu_rows[s+1]-cu_rows[s] rows
        const int s_ = seq_ids ? seq_ids[b] : b;
        row0 = cu_rows[s_];
        L = cu_rows[s_ + 1] - cu_rows[s_];
    }
    float* Ks = sm;
    float* Vs = sm + (size_t)L * HD;
    const int d = heads * HD;
    const float* base = qkv + row0 * 3 * d + h * HD;
    for (int i = threadIdx.x; i < L * HD; i += blockDim.x) {
        const int r = i / HD, cc = i % HD;
        Ks[i] = base[(long)r * 3 * d + d + cc];
        Vs[i] = base[(long)r * 3 * d + 2 * d + cc];
    }
    __syncthreads();
    const float scale = rsqrtf((float)HD);
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        float q[HD], o[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) { q[k] = base[(long)i * 3 * d + k]; o[k] = 0.f; }
        float m = -INFINITY, l = 0.f;
        const int jend = causal ? i + 1 : L;
        for (int j = 0; j < jend; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < HD; ++k) s += q[k] * Ks[j * HD + k];
            s *= scale;
            const float mn = fmaxf(m, s);
            const float a = expf(m - mn), p = expf(s - mn);
            l = l * a + p;
#pragma unroll
            for (int k = 0; k < HD; ++k) o[k] = o[k] * a + p * Vs[j * HD + k];
            m = mn;
        }
        const float inv = 1.0f / l;
        float* orow = out + (row0 + i) * d + h * HD;
#pragma unroll
        for (int k = 0; k < HD; ++k) orow[k] = o[k] * inv;
    }
}

template <int HD>
__global__ __launch_bounds__(128) void attn_f32_bwd_kernel(int L, int heads, int causal,
                                                           const float* __restrict__ qkv,
                                                           const float* __restrict__ dout,
                                                           float* __restrict__ dqkv,
    const int* __restrict__ seq_ids, const int* __restrict__ cu_rows) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    long row0 = (long)b * L;
    if (cu_rows) {           // packed rows: this block's sequence starts at cu_rows[s] and has cu_rows[s+1]-cu_rows[s] rows
        const int s_ = seq_ids ? seq_ids[b] : b;
        row0 = cu_rows[s_];
        L = cu_rows[s_ + 1] - cu_rows[s_];
    }
    float* A = sm;                         // phase 1: K      phase 2: Q
    float* B = sm + (size_t)L * HD;        // phase 1: V      phase 2: dO
    float* lse = B + (size_t)L * HD;
    float* delta = lse + L;
    const int d = heads * HD;
    const float* base = qkv + row0 * 3 * d + h * HD;
    const float* dob = dout + row0 * d + h * HD;
    float* dbase = dqkv + row0 * 3 * d + h * HD;
    const float scale = rsqrtf((float)HD);
    for (int i = threadIdx.x; i < L * HD; i += blockDim.x) {
        const int r = i / HD, cc = i % HD;
        A[i] = base[(long)r * 3 * d + d + cc];
        B[i] = base[(long)r * 3 * d + 2 * d + cc];
    }
    __syncthreads();
    // phase 1: per query row -> lse, delta, dq
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        float q[HD], go[HD], dq[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) { q[k] = base[(long)i * 3 * d + k]; go[k] = dob[(long)i * d + k]; dq[k] = 0.f; }
        const int jend = causal ? i + 1 : L;
        float m = -INFINITY, l = 0.f;
        for (int j = 0; j < jend; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < HD; ++k) s += q[k] * A[j * HD + k];
            s *= scale;
            const float mn = fmaxf(m, s);
            l = l * expf(m - mn) + expf(s - mn);
            m = mn;
        }
        const float ls = m + logf(l);
        float dl = 0.f;
        for (int j = 0; j < jend; ++j) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int k = 0; k < HD; ++k) { s += q[k] * A[j * HD + k]; dp += go[k] * B[j * HD + k]; }
            dl += expf(s * scale - ls) * dp;
        }
        for (int j = 0; j < jend; ++j) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int k = 0; k < HD; ++k) { s += q[k] * A[j * HD + k]; dp += go[k] * B[j * HD + k]; }
            const float ds = expf(s * scale - ls) * (dp - dl) * scale;
#pragma unroll
            for (int k = 0; k < HD; ++k) dq[k] += ds * A[j * HD + k];
        }
        lse[i] = ls;
        delta[i] = dl;
#pragma unroll
        for (int k = 0; k < HD; ++k) dbase[(long)i * 3 * d + k] = dq[k];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L * HD; i += blockDim.x) {
        const int r = i / HD, cc = i % HD;
        A[i] = base[(long)r * 3 * d + cc];
        B[i] = dob[(long)r * d + cc];
    }
    __syncthreads();
    // phase 2: per key row -> dv, then dk
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        float kk[HD], acc[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) { kk[k] = base[(long)j * 3 * d + d + k]; acc[k] = 0.f; }
        const int ibeg = causal ? j : 0;
        for (int i = ibeg; i < L; ++i) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < HD; ++k) s += A[i * HD + k] * kk[k];
            const float p = expf(s * scale - lse[i]);
#pragma unroll
            for (int k = 0; k < HD; ++k) acc[k] += p * B[i * HD + k];
        }
#pragma unroll
        for (int k = 0; k < HD; ++k) { dbase[(long)j * 3 * d + 2 * d + k] = acc[k]; acc[k] = 0.f; }
        float vv[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) vv[k] = base[(long)j * 3 * d + 2 * d + k];
        for (int i = ibeg; i < L; ++i) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int k = 0; k < HD; ++k) { s += A[i * HD + k] * kk[k]; dp += B[i * HD + k] * vv[k]; }
            const float ds = expf(s * scale - lse[i]) * (dp - delta[i]) * scale;
#pragma unroll
            for (int k = 0; k < HD; ++k) acc[k] += ds * A[i * HD + k];
        }
#pragma unroll
        for (int k = 0; k < HD; ++k) dbase[(long)j * 3 * d + d + k] = acc[k];
    }
}

// =============================================================================== bf16 MFMA kernels
// minimum waves per SIMD asked of the compiler (caps VGPRs): whole blocks must fit
#ifndef AT_MINW_S
#define AT_MINW_S 4      // NT <= 4 (blocks of <= 4 waves)
#endif
#ifndef AT_MINW_M
#define AT_MINW_M 3      // NT 5..8 (170 VGPRs: no spills in the backward; L=77 backward 686 -> 650 us vs 4 / 128 VGPRs)
#endif
#define AT_MINW(NT) ((NT) <= 4 ? AT_MINW_S : AT_MINW_M)

// ---- LDS image of an operand and its MFMA fragments, for every bf16 kernel below.  Per head dim:
//   HD = 64: 128-byte rows;
//   HD = 80: rows padded to 128 elements = 256 bytes (dims 80..127 zero), three 32-deep k-slices, five 16-column output tiles.
template <int HD> struct AtCfg {
    static constexpr int ROWB = HD <= 64 ? 128 : 256;      // LDS row bytes
    static constexpr int KS = (HD + 31) / 32;              // 32-deep k-slices of the QK^T reduction
    static constexpr int DT = (HD + 15) / 16;              // 16-column tiles of the head dim
    static constexpr int CHUNKS = HD / 8;                  // valid 16-byte chunks per row
    static constexpr int MAXW_F = HD <= 64 ? 16 : 12;      // online-softmax kernels: waves per block, forward (head dim 80 with the fast path: > 128 VGPRs)
    static constexpr int MAXW_B = HD <= 64 ? 16 : 12;      // backward: head dim 80 needs 168 VGPRs -> three waves per SIMD
    static constexpr int STAGE_U = HD <= 64 ? 5 : 6;       // online-softmax kernels: unroll of at_stage2 (see there)
};
constexpr int AT_HD = 64;                                   // the whole-sequence kernels' head dim and LDS row bytes
constexpr int AT_ROWB = AtCfg<AT_HD>::ROWB;

__device__ __forceinline__ bf16x8 pack_pair(const f32x4& a, const f32x4& b) {
    bf16x8 r;
    r[0] = (bf16_t)a[0]; r[1] = (bf16_t)a[1]; r[2] = (bf16_t)a[2]; r[3] = (bf16_t)a[3];
    r[4] = (bf16_t)b[0]; r[5] = (bf16_t)b[1]; r[6] = (bf16_t)b[2]; r[7] = (bf16_t)b[3];
    return r;
}
__device__ __forceinline__ float group_max(float v) {   // across the 4 lane groups (same lane&15)
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
// Swizzle of the 16-byte chunks of a row.  A 16-lane group of ds_read_b128 (rows c, chunk 4ks+g) and a 32-lane group of
// ds_read_b64_tr_b16 (eight consecutive rows, 32 bytes each) must land on 256 distinct bytes of the 64 banks:
//   128-byte rows: odd rows already sit in the other half of the banks; xor with 2 * ((row >> 1) & 3) inside the 8 chunks
//   256-byte rows: every row starts on bank 0, so the xor needs three row bits: 2 * (row & 7) inside the 16 chunks
//                  (with the 128-byte rule rows 2i and 2i+1 collided: every fragment read of the head-dim-80 kernels 2-way)
template <int ROWB>
__device__ __forceinline__ int at_off(int row, int chunk) {
    if constexpr (ROWB == 256) return row * ROWB + ((chunk ^ ((row & 7) << 1)) << 4);
    return row * ROWB + ((chunk ^ (((row >> 1) & 3) << 1)) << 4);
}
// stage rows [0, LP) of two operands (row stride `ld` elements in HBM) into their LDS images; rows >= L -> 0.
// Both operands of a phase at once, loads first: the plain loop (load, wait, write LDS, next chunk) was a chain of HBM
// latencies per thread -- 4 chunks x 2 operands with 3-wave blocks; here U x 2 loads per thread are in flight.
// U = 4 in the whole-sequence kernels.  The online-softmax kernels take 5 (head dim 64) or 6 (80): with a full block (16 x 64
// threads at head dim 64, 12 x 64 at 80) ONE batch covers both operand images, i.e. one HBM round trip per staging instead of two
// or three (nothing else runs on the CU meanwhile: the images of one (sample, head) fill its LDS)
template <int HD, int U>
__device__ __forceinline__ void at_stage2(char* ldsA, const bf16_t* srcA, long ldA, char* ldsB, const bf16_t* srcB, long ldB,
                                          int L, int LP) {
    constexpr int RC = AtCfg<HD>::ROWB / 16;
    const int total = LP * RC, step = blockDim.x;
    for (int base = threadIdx.x; base < total; base += U * step) {
        uint4 va[U], vb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int id = base + u * step, row = id / RC, ch = id % RC;
            va[u] = make_uint4(0u, 0u, 0u, 0u);
            vb[u] = make_uint4(0u, 0u, 0u, 0u);
            if (id < total && row < L && ch < AtCfg<HD>::CHUNKS) {
                va[u] = *reinterpret_cast<const uint4*>(srcA + (long)row * ldA + ch * 8);
                vb[u] = *reinterpret_cast<const uint4*>(srcB + (long)row * ldB + ch * 8);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int id = base + u * step, row = id / RC, ch = id % RC;
            if (id < total) {
                *reinterpret_cast<uint4*>(ldsA + at_off<AtCfg<HD>::ROWB>(row, ch)) = va[u];
                *reinterpret_cast<uint4*>(ldsB + at_off<AtCfg<HD>::ROWB>(row, ch)) = vb[u];
            }
        }
    }
}
// row-read fragment: rows 16*tile + c, reduction chunk 4*ks + g
template <int HD>
__device__ __forceinline__ bf16x8 at_row_frag(const char* img, int tile, int ks, int g, int c) {
    return lds_read8(img + at_off<AtCfg<HD>::ROWB>(16 * tile + c, 4 * ks + g));
}
// transposed fragment: reduction rows 32*s + {4g+q, 16+4g+q}, columns of 16-wide tile dt
template <int HD>
__device__ __forceinline__ bf16x8 at_tr_frag(const char* img, int s, int dt, int g, int q, int p) {
    const int r0 = 32 * s + 4 * g + q, r1 = r0 + 16;
    const int ch = 2 * dt + (p >> 1), hb = (p & 1) * 8;
    return lds_tr8(img + at_off<AtCfg<HD>::ROWB>(r0, ch) + hb, img + at_off<AtCfg<HD>::ROWB>(r1, ch) + hb);
}
// fragment straight from HBM/L2 (an operand tile that only this wave reads): rows 16*tile + c, chunk 4*ks + g
template <int HD>
__device__ __forceinline__ bf16x8 at_global_frag(const bf16_t* src, long ld, int L, int tile, int ks, int g, int c) {
    const int row = 16 * tile + c, ch = 4 * ks + g;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < L && ch < AtCfg<HD>::CHUNKS) v = *reinterpret_cast<const uint4*>(src + (long)row * ld + ch * 8);
    union { uint4 u; bf16x8 f; } x;
    x.u = v;
    return x.f;
}

// Store one 16-row x 64-column fp32 accumulator tile (lane (g,c): row c, columns 16*dt + 4*g + 0..3 in o[dt]) as bf16,
// coalesced: in the accumulator layout neighbouring lanes are neighbouring ROWS and each holds 8 bytes per 16-column
// tile, i.e. four 8-byte stores whose lanes all hit different cache lines (measured for the GEMM epilogue,
// scripts/ubench_store.hip: 13.7 B/clk per CU for such 16-byte stores, 50 B/clk when four neighbouring lanes cover 64
// contiguous bytes).  v_permlane16_swap pairs two 16-column tiles into 16-byte chunks, ds_bpermute (crossbar only) moves
// lane 16*g + c to lane 4*c + chunk: two 16-byte stores, each 16 rows x 64 contiguous bytes.  A fifth 16-column tile (HD = 80)
// goes out with 8-byte stores.
typedef unsigned at_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned at_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned at_pack2(float a, float b) {
    union { __attribute__((ext_vector_type(2))) __bf16 h; unsigned u; } x;
    x.h[0] = (bf16_t)a;
    x.h[1] = (bf16_t)b;
    return x.u;
}
template <int HD>
__device__ __forceinline__ void at_store_tile(bf16_t* dst, long ld, int L, int row0, const f32x4 (&o)[AtCfg<HD>::DT], float mul,
                                              int lane) {
    const int srow = lane >> 2, sch = lane & 3;
    const int bp_src = 4 * (16 * (((sch & 1) << 1) | (sch >> 1)) + srow);
    unsigned lo[4], hi[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        lo[dt] = at_pack2(o[dt][0] * mul, o[dt][1] * mul);
        hi[dt] = at_pack2(o[dt][2] * mul, o[dt][3] * mul);
    }
#pragma unroll
    for (int ip = 0; ip < 2; ++ip) {
        const at_u32x2 a = __builtin_amdgcn_permlane16_swap(lo[2 * ip], lo[2 * ip + 1], false, false);
        const at_u32x2 b = __builtin_amdgcn_permlane16_swap(hi[2 * ip], hi[2 * ip + 1], false, false);
        const unsigned q[4] = {a[0], b[0], a[1], b[1]};
        at_u32x4 t;
#pragma unroll
        for (int d = 0; d < 4; ++d) t[d] = (unsigned)__builtin_amdgcn_ds_bpermute(bp_src, (int)q[d]);
        if (row0 + srow < L) *reinterpret_cast<at_u32x4*>(dst + (long)(row0 + srow) * ld + 8 * sch + 32 * ip) = t;
    }
    if constexpr (AtCfg<HD>::DT > 4) {
        const int g = lane >> 4, c = lane & 15;
        if (row0 + c < L)
            store4(dst + (long)(row0 + c) * ld + 64 + 4 * g, make_float4(o[4][0] * mul, o[4][1] * mul, o[4][2] * mul, o[4][3] * mul));
    }
}

// ---- whole-sequence kernels: head dim 64, L <= 128 (NT = 2, 4, 6 or 8 tiles of 16 rows)
// CAUSAL / PACKED as in attn_bf16_bwd4_kernel below (round 4): key masks only in the tile that holds rows behind L and in the
// diagonal tile of a causal sequence, tiles above the diagonal skipped whole, the scale inside the exponent's packed FMA.
template <int NT, bool CAUSAL, bool PACKED>
__global__ __launch_bounds__(64 * NT, AT_MINW(NT)) void attn_bf16_fwd_kernel(int L, int heads,
                                                            const bf16_t* __restrict__ qkv,
                                                            bf16_t* __restrict__ out,
    const int* __restrict__ seq_ids, const int* __restrict__ cu_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int LP = 16 * NT;
    // K and V are shared by all query tiles and live in LDS; a wave's Q tile is read by that wave only, so its two
    // fragments come straight from memory (issued before the staging so they are in flight during it): one third less
    // LDS per (sample, head) = more resident blocks per CU
    char* Ks = smem;
    char* Vs = smem + LP * AT_ROWB;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    long row0 = (long)b * L;
    if (cu_rows) {           // packed rows: this block's sequence starts at cu_rows[s] and has cu_rows[s+1]-cu_rows[s] rows
        const int s_ = seq_ids ? seq_ids[b] : b;
        row0 = cu_rows[s_];
        L = cu_rows[s_ + 1] - cu_rows[s_];
    }
    const int d = heads * AT_HD;
    const bf16_t* base = qkv + row0 * 3 * d + h * AT_HD;
    bf16x8 qpre0, qpre1;
    {
        const int lane0 = threadIdx.x & 63, w0 = threadIdx.x >> 6;
        qpre0 = at_global_frag<AT_HD>(base, 3 * d, L, w0, 0, lane0 >> 4, lane0 & 15);
        qpre1 = at_global_frag<AT_HD>(base, 3 * d, L, w0, 1, lane0 >> 4, lane0 & 15);
    }
    at_stage2<AT_HD, 4>(Ks, base + d, 3 * d, Vs, base + 2 * d, 3 * d, L, LP);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c = lane & 15, q = c >> 2, p = c & 3;
    const float sc2 = rsqrtf((float)AT_HD) * 1.44269504088896340736f;
    const f32x2 sc22 = {sc2, sc2};
    const int ntq = PACKED ? (L + 15) >> 4 : NT;
    const bool ragged = (L & 15) != 0;
    const int kq0 = at_off<AT_ROWB>(c, g), kq1 = at_off<AT_ROWB>(c, 4 + g);
    int vt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vt[dt] = at_off<AT_ROWB>(4 * g + q, 2 * dt + (p >> 1)) + (p & 1) * 8;

    const int nwaves = blockDim.x >> 6;
    for (int qt = wave; qt < ntq; qt += nwaves) {
        const int query = 16 * qt + c;
        bf16x8 qf0 = qpre0, qf1 = qpre1;
        if (qt != wave) {      // only when a block has fewer waves than query tiles
            qf0 = at_global_frag<AT_HD>(base, 3 * d, L, qt, 0, g, c);
            qf1 = at_global_frag<AT_HD>(base, 3 * d, L, qt, 1, g, c);
        }
        f32x4 s[NT];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            s[kt] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if ((!PACKED || kt < ntq) && !(CAUSAL && kt > qt)) {
                f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Ks + kt * 2048 + kq0), qf0, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Ks + kt * 2048 + kq1), qf1, a, 0, 0, 0);
                if ((ragged && kt == ntq - 1) || (CAUSAL && kt == qt)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = 16 * kt + 4 * g + r;
                        if (key >= L || (CAUSAL && key > query)) a[r] = -INFINITY;
                    }
                }
                s[kt] = a;
                m = fmaxf(fmaxf(m, fmaxf(a[0], a[1])), fmaxf(a[2], a[3]));
            }
        }
        m = group_max(m);                                      // finite: key 0 is visible to every query
        const float m2 = m * sc2;
        const f32x2 nm2 = {-m2, -m2};
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const f32x2 t = __builtin_elementwise_fma((f32x2){s[kt][2 * h2], s[kt][2 * h2 + 1]}, sc22, nm2);
                const float e0 = __builtin_amdgcn_exp2f(t[0]), e1 = __builtin_amdgcn_exp2f(t[1]);
                s[kt][2 * h2] = e0;
                s[kt][2 * h2 + 1] = e1;
                l += e0 + e1;
            }
        l = group_sum(l);
        const float inv_l = 1.0f / l;
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sp = 0; sp < NT / 2; ++sp) {
            if ((!PACKED || 2 * sp < ntq) && !(CAUSAL && 2 * sp > qt)) {
                const bf16x8 pf = pack_pair(s[2 * sp], s[2 * sp + 1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        lds_tr8(Vs + sp * 4096 + vt[dt], Vs + sp * 4096 + 2048 + vt[dt]), pf, o[dt], 0, 0, 0);
            }
        }
        at_store_tile<AT_HD>(out + row0 * d + h * AT_HD, d, L, 16 * qt, o, inv_l, lane);
    }
}

// Backward with ALL FOUR operands of a (sample, head) resident in LDS: every operand is read from memory once (8 x 16 B per
// thread, all in flight together), both phases take their fragments from the LDS images, and one barrier separates them:
//   A  wave = one 16-query tile: S^T, dP^T -> lse, delta, dQ
//   B  wave = one 16-key tile:   S, dP -> dV, dK
// Costs 4 x LP x 128 B of LDS per block (32.5 KiB at LP = 64).  It replaced (round 3) a backward that kept two images -- K, V in
// phase A, then Q, dO restaged over them for phase B -- and took the other pair of each phase as per-wave fragments from memory.
// PMC on that kernel (profiles/r03_pmc_attention.txt): FETCH_SIZE = 2.0x the algorithmic reads -- Q, K, V and dO each travelled
// from the fabric TWICE, because the eight (sample, head) blocks a CU keeps in flight per XCD-L2 share outlive a 4-MiB L2 -- and
// with the dqkv write it moved 3.45 GB in 578 us = 6.0 TB/s: bandwidth-bound, on traffic it did not need.
// Round 4: templated on the causal flag, and the arithmetic of both phases cut down (the kernel proved bound by its vector work,
// not by bytes in flight -- a prefetching persistent form was slower, profiles/r04_attention_long.txt): fragment addresses are
// per-lane constants + immediates; key masks only in the one tile that holds rows behind L (and the diagonal tile of a causal
// sequence; tiles above the diagonal are skipped whole, MFMAs included); the scale folded into the exponent's packed FMA;
// phase A leaves -lse and -delta * scale in LDS (padded queries: -1e30, i.e. P = 0 by arithmetic) so that phase B is two packed
// FMAs, an exponential and a packed multiply per pair of scores.
// PACKED: the items are variable-length sequences of a packed batch (cu_rows), which may use fewer than NT tiles; a dense batch
// always uses all NT and needs no tile guards.
template <int NT, bool CAUSAL, bool PACKED>
__global__ __launch_bounds__(64 * NT, AT_MINW(NT)) void attn_bf16_bwd4_kernel(
    int L, int heads, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
    bf16_t* __restrict__ dqkv, const int* __restrict__ seq_ids, const int* __restrict__ cu_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int LP = 16 * NT;
    char* Kl = smem;
    char* Vl = smem + LP * AT_ROWB;
    char* Ql = smem + 2 * LP * AT_ROWB;
    char* Gl = smem + 3 * LP * AT_ROWB;
    float* lse2 = reinterpret_cast<float*>(smem + 4 * LP * AT_ROWB);
    float* delta = lse2 + LP;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    long row0 = (long)b * L;
    if (cu_rows) {
        const int s_ = seq_ids ? seq_ids[b] : b;
        row0 = cu_rows[s_];
        L = cu_rows[s_ + 1] - cu_rows[s_];
    }
    const int d = heads * AT_HD;
    const long ld3 = 3 * d;
    const bf16_t* qbase = qkv + row0 * ld3 + h * AT_HD;
    const bf16_t* gbase = dout + row0 * d + h * AT_HD;
    bf16_t* dbase = dqkv + row0 * ld3 + h * AT_HD;
    {   // all four images: loads first (4 operands x U chunks per thread in flight), then the LDS writes; rows >= L -> 0
        constexpr int U = 2;
        const int total = LP * 8, step = blockDim.x;
        for (int base = threadIdx.x; base < total; base += U * step) {
            uint4 v[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int id = base + u * step, row = id >> 3, ch = id & 7;
#pragma unroll
                for (int o = 0; o < 4; ++o) v[u][o] = make_uint4(0u, 0u, 0u, 0u);
                if (id < total && row < L) {
                    const bf16_t* pq = qbase + (long)row * ld3 + ch * 8;
                    v[u][0] = *reinterpret_cast<const uint4*>(pq + d);
                    v[u][1] = *reinterpret_cast<const uint4*>(pq + 2 * d);
                    v[u][2] = *reinterpret_cast<const uint4*>(pq);
                    v[u][3] = *reinterpret_cast<const uint4*>(gbase + (long)row * d + ch * 8);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int id = base + u * step, row = id >> 3, ch = id & 7;
                if (id < total) {
                    const int off = at_off<AT_ROWB>(row, ch);
                    *reinterpret_cast<uint4*>(Kl + off) = v[u][0];
                    *reinterpret_cast<uint4*>(Vl + off) = v[u][1];
                    *reinterpret_cast<uint4*>(Ql + off) = v[u][2];
                    *reinterpret_cast<uint4*>(Gl + off) = v[u][3];
                }
            }
        }
    }
    for (int i = threadIdx.x; i < LP; i += blockDim.x) { lse2[i] = -1e30f; delta[i] = 0.f; }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int g = lane >> 4, c = lane & 15, q = c >> 2, p = c & 3;
    const float scale = rsqrtf((float)AT_HD);
    const float sc2 = scale * 1.44269504088896340736f;
    const f32x2 sc22 = {sc2, sc2}, scale2 = {scale, scale};
    const int nt_used = PACKED ? (L + 15) >> 4 : NT;
    const bool ragged = (L & 15) != 0;                       // the last tile holds rows behind L
    // fragment offsets of tile 0 / slice 0: tiles are 2 KiB apart, the swizzle only depends on the row inside the tile
    const int kq0 = at_off<AT_ROWB>(c, g), kq1 = at_off<AT_ROWB>(c, 4 + g);
    int vt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vt[dt] = at_off<AT_ROWB>(4 * g + q, 2 * dt + (p >> 1)) + (p & 1) * 8;

    // ---- phase A: wave = one 16-query tile: S^T, dP^T -> lse, delta, dQ
    for (int qt = wave; qt < nt_used; qt += nwaves) {
        const int query = 16 * qt + c;
        const bf16x8 qf0 = lds_read8(Ql + qt * 2048 + kq0), qf1 = lds_read8(Ql + qt * 2048 + kq1);
        const bf16x8 gf0 = lds_read8(Gl + qt * 2048 + kq0), gf1 = lds_read8(Gl + qt * 2048 + kq1);
        f32x4 s[NT], dp[NT];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            s[kt] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            dp[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if ((!PACKED || kt < nt_used) && !(CAUSAL && kt > qt)) {       // (tiles behind L or above the diagonal: nothing to compute)
                f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kl + kt * 2048 + kq0), qf0, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kl + kt * 2048 + kq1), qf1, a, 0, 0, 0);
                f32x4 e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Vl + kt * 2048 + kq0), gf0, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Vl + kt * 2048 + kq1), gf1, e, 0, 0, 0);
                if ((ragged && kt == nt_used - 1) || (CAUSAL && kt == qt)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = 16 * kt + 4 * g + r;
                        if (key >= L || (CAUSAL && key > query)) a[r] = -INFINITY;
                    }
                }
                s[kt] = a;
                dp[kt] = e;
                m = fmaxf(fmaxf(m, fmaxf(a[0], a[1])), fmaxf(a[2], a[3]));
            }
            __builtin_amdgcn_sched_barrier(0);               // (a scheduling window over all tiles spills: 228 bytes per lane at NT = 4)
        }
        m = group_max(m);                                      // finite: key 0 is visible to every query
        const float m2 = m * sc2;
        const f32x2 nm2 = {-m2, -m2};
        float l = 0.f, num = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x2 t = __builtin_elementwise_fma((f32x2){s[kt][2 * h], s[kt][2 * h + 1]}, sc22, nm2);
                const float e0 = __builtin_amdgcn_exp2f(t[0]), e1 = __builtin_amdgcn_exp2f(t[1]);
                s[kt][2 * h] = e0;
                s[kt][2 * h + 1] = e1;
                l += e0 + e1;
                num = __builtin_fmaf(e0, dp[kt][2 * h], num);
                num = __builtin_fmaf(e1, dp[kt][2 * h + 1], num);
            }
        l = group_sum(l);
        num = group_sum(num);
        const float inv_l = 1.0f / l;
        const float dl = num * inv_l;                          // delta = sum_k P dP
        if (g == 0 && query < L) {
            lse2[query] = -(m2 + log2f(l));
            delta[query] = -dl * scale;
        }
        const float pscale = inv_l * scale;
        const f32x2 ps2 = {pscale, pscale}, ndl2 = {-dl, -dl};
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x2 pe = (f32x2){s[kt][2 * h], s[kt][2 * h + 1]} * ps2;
                const f32x2 ds = pe * ((f32x2){dp[kt][2 * h], dp[kt][2 * h + 1]} + ndl2);    // dS^T = P (dP - delta) scale
                s[kt][2 * h] = ds[0];
                s[kt][2 * h + 1] = ds[1];
            }
        f32x4 dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sp = 0; sp < NT / 2; ++sp) {
            if ((!PACKED || 2 * sp < nt_used) && !(CAUSAL && 2 * sp > qt)) {
                const bf16x8 df = pack_pair(s[2 * sp], s[2 * sp + 1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        lds_tr8(Kl + sp * 4096 + vt[dt], Kl + sp * 4096 + 2048 + vt[dt]), df, dq[dt], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        at_store_tile<AT_HD>(dbase, ld3, L, 16 * qt, dq, 1.0f, lane);
    }
    __syncthreads();                           // -lse / -delta * scale of every query tile are complete

    // ---- phase B: wave = one 16-key tile: S, dP -> dV, dK
    for (int kt = wave; kt < nt_used; kt += nwaves) {
        const int key = 16 * kt + c;
        const bf16x8 kf0 = lds_read8(Kl + kt * 2048 + kq0), kf1 = lds_read8(Kl + kt * 2048 + kq1);
        const bf16x8 vf0 = lds_read8(Vl + kt * 2048 + kq0), vf1 = lds_read8(Vl + kt * 2048 + kq1);
        f32x4 dv[4], dk[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int sp = 0; sp < NT / 2; ++sp) {
            // query tiles 2 sp, 2 sp + 1; causal: a query tile before the key tile sees none of its keys
            if ((!PACKED || 2 * sp < nt_used) && !(CAUSAL && 2 * sp + 1 < kt)) {
                f32x4 pt[2], dst[2];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int qt = 2 * sp + hh;
                    pt[hh] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    dst[hh] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if ((!PACKED || qt < nt_used) && !(CAUSAL && qt < kt)) {
                        f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Ql + qt * 2048 + kq0), kf0, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Ql + qt * 2048 + kq1), kf1, a, 0, 0, 0);
                        f32x4 e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Gl + qt * 2048 + kq0), vf0, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                        e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Gl + qt * 2048 + kq1), vf1, e, 0, 0, 0);
                        const f32x4 nls = *reinterpret_cast<const f32x4*>(lse2 + 16 * qt + 4 * g);     // -lse (padded queries: -1e30)
                        const f32x4 ndl = *reinterpret_cast<const f32x4*>(delta + 16 * qt + 4 * g);    // -delta * scale
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const f32x2 t = __builtin_elementwise_fma((f32x2){a[2 * h], a[2 * h + 1]}, sc22, (f32x2){nls[2 * h], nls[2 * h + 1]});
                            const f32x2 u = __builtin_elementwise_fma((f32x2){e[2 * h], e[2 * h + 1]}, scale2, (f32x2){ndl[2 * h], ndl[2 * h + 1]});
                            const f32x2 pr = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
                            const f32x2 ds = pr * u;
                            a[2 * h] = pr[0];
                            a[2 * h + 1] = pr[1];
                            e[2 * h] = ds[0];
                            e[2 * h + 1] = ds[1];
                        }
                        // columns of keys behind L: their dK / dV rows are never stored, but P there is exp2(0 - lse), which
                        // overflows for very negative scores -- cut them (and, causal, the keys above the diagonal)
                        if ((ragged && kt == nt_used - 1) || (CAUSAL && qt == kt)) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (key >= L || (CAUSAL && key > 16 * qt + 4 * g + r)) { a[r] = 0.f; e[r] = 0.f; }
                        }
                        pt[hh] = a;
                        dst[hh] = e;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                const bf16x8 pf = pack_pair(pt[0], pt[1]);
                const bf16x8 df = pack_pair(dst[0], dst[1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr8(Gl + sp * 4096 + vt[dt], Gl + sp * 4096 + 2048 + vt[dt]), pf, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr8(Ql + sp * 4096 + vt[dt], Ql + sp * 4096 + 2048 + vt[dt]), df, dk[dt], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        at_store_tile<AT_HD>(dbase + d, ld3, L, 16 * kt, dk, 1.0f, lane);
        at_store_tile<AT_HD>(dbase + 2 * d, ld3, L, 16 * kt, dv, 1.0f, lane);
    }
}

// =============================================================================== long sequences / head dim 80
// Same data flow as above (whole K, V of one (sample, head) in LDS, one block of up to 16 waves per CU), but a query
// tile's scores no longer fit registers, so the softmax runs ONLINE over chunks of key tiles: running row maximum m,
// rescaled row sum l and rescaled accumulators, as in flash attention.  Templated on the head dim:
//   HD = 64: 128 < L <= 608 (ViT-B/16: 197 tokens; ViT-L/14-336: 577 tokens; 2 x 608 x 128 B = 152 KiB);
//   HD = 80: L <= 288 (ViT-H/14: 257 tokens; 2 x 288 x 256 B = 144 KiB).
// Backward: two phases that reuse the same two LDS images (so a (sample, head) needs 2 x LP x ROWB, and each phase's registers
// are dead in the other):
//   A  K, V in LDS; wave = one 16-query tile (Q, dO fragments straight from memory): S^T, dP^T -> lse, delta, dQ
//   B  Q, dO in LDS; wave = one 16-key tile (K, V fragments from memory, L2-warm), query tiles walked in pairs: S, dP -> dV, dK
// Phase A makes two sweeps over the keys: sweep 1 gets log-sum-exp and delta = sum_k P dP with the same online rescaling (so
// the forward output is not needed), sweep 2 recomputes S, dP chunk-wise for dS and dQ.
#define ATL_CH 8      // key tiles per chunk (forward)
#define ATL_CHB 4     // backward phase A keeps S and dP of a chunk: half the chunk to stay within 128 VGPRs at 16 waves

__device__ __forceinline__ int atl_lp(int L) { return ((L + 31) >> 5) << 5; }

template <int HD, bool CAUSAL>
__global__ __launch_bounds__(AtCfg<HD>::MAXW_F * 64) void attn_bf16_long_fwd_kernel(int L, int heads, const bf16_t* __restrict__ qkv,
                                                                  bf16_t* __restrict__ out, float* __restrict__ lse_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ROWB = AtCfg<HD>::ROWB, KS = AtCfg<HD>::KS, DT = AtCfg<HD>::DT;
    const int LP = atl_lp(L);
    char* Ks = smem;
    char* Vs = smem + LP * ROWB;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int d = heads * HD;
    const bf16_t* base = qkv + (long)b * L * 3 * d + h * HD;
    at_stage2<HD, AtCfg<HD>::STAGE_U>(Ks, base + d, 3 * d, Vs, base + 2 * d, 3 * d, L, LP);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int g = lane >> 4, c = lane & 15, q = c >> 2, p = c & 3;
    const float sc2 = rsqrtf((float)HD) * 1.44269504088896340736f;
    const int nt = (L + 15) >> 4, np = LP >> 5;
    // per-lane byte offsets of the fragments of key tile 0 / key slice 0 (the swizzle is periodic in 8 rows, tiles are 16)
    int kq[KS], vt0[DT];          // (the transposed fragment's second half sits 16 rows further: same swizzle, + 16 * ROWB)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kq[ks] = at_off<ROWB>(c, 4 * ks + g);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vt0[dt] = at_off<ROWB>(4 * g + q, 2 * dt + (p >> 1)) + (p & 1) * 8;
    // all-ones A fragment: o-style MFMA of it with the packed probabilities = their column sums, i.e. the softmax denominator
    // of the lane's query in every output row -- the 32 row-sum adds per chunk leave the vector pipe, which is what bounds this
    // loop (per 128-key chunk and wave: 32 v_exp_f32 at quarter rate = 512 issue cycles + ~100 full-rate instructions, against
    // 36 MFMAs of 16 cycles)
    union { uint4 u; bf16x8 f; } ones_u;
    ones_u.u = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);
    const bf16x8 ones = ones_u.f;
    for (int qt = wave; qt < nt; qt += nwaves) {
        const int query = 16 * qt + c;
        bf16x8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = at_global_frag<HD>(base, 3 * d, L, qt, ks, g, c);
        float m2 = -INFINITY;
        f32x4 o[DT], lsum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // One full chunk of eight key tiles that hold real, unmasked keys only: no guards, the scale folded into the exponent's
        // (packed) FMA, accumulators started inside the first MFMA, fragment addresses = per-lane constants + immediates.
        auto chunk = [&](int pc) {
            const char* Kc = Ks + pc * 32 * ROWB;
            const char* Vc = Vs + pc * 32 * ROWB;
            f32x4 s[ATL_CH];
#pragma unroll
            for (int j = 0; j < ATL_CH; ++j) {
                f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kc + j * 16 * ROWB + kq[0]), qf[0],
                                                                  (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int ks = 1; ks < KS; ++ks)
                    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kc + j * 16 * ROWB + kq[ks]), qf[ks], a, 0, 0, 0);
                s[j] = a;
            }
            float cm = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
            for (int j = 1; j < ATL_CH; ++j) cm = fmaxf(fmaxf(cm, fmaxf(s[j][0], s[j][1])), fmaxf(s[j][2], s[j][3]));
            cm = group_max(cm);
            const float mn = fmaxf(m2, cm * sc2);                  // finite: key 32 pc is real
            const float alpha = __builtin_amdgcn_exp2f(m2 - mn);
            lsum *= alpha;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
            const f32x2 sc22 = {sc2, sc2}, nmn2 = {-mn, -mn};
#pragma unroll
            for (int j = 0; j < ATL_CH; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x2 t = __builtin_elementwise_fma((f32x2){s[j][2 * h], s[j][2 * h + 1]}, sc22, nmn2);   // v_pk_fma_f32
                    s[j][2 * h] = __builtin_amdgcn_exp2f(t[0]);
                    s[j][2 * h + 1] = __builtin_amdgcn_exp2f(t[1]);
                }
#pragma unroll
            for (int jp = 0; jp < ATL_CH / 2; ++jp) {
                const bf16x8 pf = pack_pair(s[2 * jp], s[2 * jp + 1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        lds_tr8(Vc + jp * 32 * ROWB + vt0[dt], Vc + (jp * 32 + 16) * ROWB + vt0[dt]), pf, o[dt], 0, 0, 0);
                lsum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, lsum, 0, 0, 0);
            }
            m2 = mn;
        };
        for (int pc = 0; pc < np; pc += ATL_CH / 2) {
            if (CAUSAL && 32 * pc > 16 * qt + 15) break;        // every key of this and later chunks is masked for the tile
            const int key_end = 32 * pc + 16 * ATL_CH;          // one past the chunk's last key
            if (key_end <= L && (!CAUSAL || key_end - 1 <= 16 * qt)) {
                chunk(pc);
                continue;
            }
            if constexpr (!CAUSAL) {
                // the keys behind the last full chunk, 32 at a time (one slice of the PV reduction per turn of a ROLLED loop: a
                // tail of one key -- L = 16 k + 1, the ViT shapes -- costs a quarter of a chunk, not a masked whole one)
                for (int sp = pc; sp < np; ++sp) {
                    const char* Kc = Ks + sp * 32 * ROWB;
                    const char* Vc = Vs + sp * 32 * ROWB;
                    f32x4 s2[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kc + j * 16 * ROWB + kq[0]), qf[0],
                                                                          (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                        for (int ks = 1; ks < KS; ++ks)
                            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kc + j * 16 * ROWB + kq[ks]), qf[ks], a, 0, 0, 0);
                        s2[j] = a;
                    }
                    if (32 * sp + 32 > L) {                       // rows behind L (zeros in LDS) must not count
#pragma unroll
                        for (int j = 0; j < 2; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (32 * sp + 16 * j + 4 * g + r >= L) s2[j][r] = -INFINITY;
                    }
                    float cm = fmaxf(fmaxf(fmaxf(s2[0][0], s2[0][1]), fmaxf(s2[0][2], s2[0][3])),
                                     fmaxf(fmaxf(s2[1][0], s2[1][1]), fmaxf(s2[1][2], s2[1][3])));
                    cm = group_max(cm);
                    const float mn = fmaxf(m2, cm * sc2);          // finite: key 32 sp is real
                    const float alpha = __builtin_amdgcn_exp2f(m2 - mn);
                    lsum *= alpha;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
                    const f32x2 sc22 = {sc2, sc2}, nmn2 = {-mn, -mn};
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const f32x2 t = __builtin_elementwise_fma((f32x2){s2[j][2 * h], s2[j][2 * h + 1]}, sc22, nmn2);
                            s2[j][2 * h] = __builtin_amdgcn_exp2f(t[0]);
                            s2[j][2 * h + 1] = __builtin_amdgcn_exp2f(t[1]);
                        }
                    const bf16x8 pf = pack_pair(s2[0], s2[1]);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr8(Vc + vt0[dt], Vc + 16 * ROWB + vt0[dt]), pf, o[dt], 0, 0, 0);
                    lsum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, lsum, 0, 0, 0);
                    m2 = mn;
                }
                break;
            } else {
            // causal chunks on or above the diagonal: per-score masks
            f32x4 s[ATL_CH];
            float cm = -INFINITY;
#pragma unroll
            for (int j = 0; j < ATL_CH; ++j) {
                const int kt = 2 * pc + j;
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                if (kt < nt) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_row_frag<HD>(Ks, kt, ks, g, c), qf[ks], a, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 16 * kt + 4 * g + r;
                    const bool ok = key < L && key <= query;
                    a[r] = ok ? a[r] * sc2 : -INFINITY;
                    cm = fmaxf(cm, a[r]);
                }
                s[j] = a;
            }
            cm = group_max(cm);
            const float mn = fmaxf(m2, cm);                       // finite: key 0 is visible to every query
            const float alpha = __builtin_amdgcn_exp2f(m2 - mn);
            lsum *= alpha;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
#pragma unroll
            for (int j = 0; j < ATL_CH; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[j][r] = __builtin_amdgcn_exp2f(s[j][r] - mn);
                }
#pragma unroll
            for (int jp = 0; jp < ATL_CH / 2; ++jp) {
                const int sp = pc + jp;
                if (sp < np) {
                    const bf16x8 pf = pack_pair(s[2 * jp], s[2 * jp + 1]);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_tr_frag<HD>(Vs, sp, dt, g, q, p), pf, o[dt], 0, 0, 0);
                    lsum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, lsum, 0, 0, 0);
                }
            }
            m2 = mn;
            }
        }
        const float l = lsum[0];                                  // every output row of the ones tile holds the query's sum
        at_store_tile<HD>(out + (long)b * L * d + h * HD, d, L, 16 * qt, o, 1.0f / l, lane);
        // log-sum-exp of the scaled scores in the log2 domain (what the backward's P = exp2(s - lse) needs): kept by callers that
        // will run clipx_attention_bwd_lse, whose phase A then needs no sweep of its own for it
        if (lse_out != nullptr && g == 0 && query < L) lse_out[(long)blockIdx.x * L + query] = m2 + log2f(l);
    }
}

// FAST = the forward handed over its log-sum-exp and output, no causal mask (every vision tower): no per-score masks at all --
// padded queries carry -lse = -1e30 (P = 0), padded key rows are zero in LDS and are cut from dS / P in the one chunk or key
// tile that holds them -- scale and subtraction folded into packed FMAs (-lse and -delta * scale are what phase A leaves in
// LDS), fragment addresses = per-lane constants + immediates.  Was ~13 vector instructions per score and phase, is ~6.
template <int HD, bool HAVE_LSE, bool CAUSAL>
__global__ __launch_bounds__(AtCfg<HD>::MAXW_B * 64) void attn_bf16_long_bwd_kernel(int L, int heads, const bf16_t* __restrict__ qkv,
                                                                  const bf16_t* __restrict__ dout, bf16_t* __restrict__ dqkv,
                                                                  const bf16_t* __restrict__ fwd_out, const float* __restrict__ lse_in) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ROWB = AtCfg<HD>::ROWB, KS = AtCfg<HD>::KS, DT = AtCfg<HD>::DT;
    const int LP = atl_lp(L);
    char* R0 = smem;                          // phase A: K      phase B: Q
    char* R1 = smem + LP * ROWB;              // phase A: V      phase B: dO
    float* lse2 = reinterpret_cast<float*>(smem + 2 * LP * ROWB);
    float* delta = lse2 + LP;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int d = heads * HD;
    const long ld3 = 3 * d;
    const bf16_t* qbase = qkv + (long)b * L * ld3 + h * HD;
    const bf16_t* gbase = dout + (long)b * L * d + h * HD;
    bf16_t* dbase = dqkv + (long)b * L * ld3 + h * HD;
    at_stage2<HD, AtCfg<HD>::STAGE_U>(R0, qbase + d, ld3, R1, qbase + 2 * d, ld3, L, LP);
    constexpr bool FAST = HAVE_LSE && !CAUSAL;
    constexpr bool causal = CAUSAL;
    for (int i = threadIdx.x; i < LP; i += blockDim.x) { lse2[i] = FAST ? -1e30f : 1e30f; delta[i] = 0.f; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int g = lane >> 4, c = lane & 15, q = c >> 2, p = c & 3;
    const float scale = rsqrtf((float)HD);
    const float sc2 = scale * 1.44269504088896340736f;
    const int nt = (L + 15) >> 4, np = LP >> 5;
    // per-lane byte offsets of the fragments of tile 0 / slice 0 (as in the forward)
    int kq[KS], vt0[DT];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kq[ks] = at_off<ROWB>(c, 4 * ks + g);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vt0[dt] = at_off<ROWB>(4 * g + q, 2 * dt + (p >> 1)) + (p & 1) * 8;
    const f32x2 sc22 = {sc2, sc2}, scale2 = {scale, scale};

    // S^T and dP^T of one chunk of key tiles against the wave's query tile; masked scores -> -inf
    auto chunk = [&](int pc, int query, const bf16x8 (&qf)[KS], const bf16x8 (&gf)[KS], f32x4 (&s)[ATL_CHB], f32x4 (&e)[ATL_CHB]) {
#pragma unroll
        for (int j = 0; j < ATL_CHB; ++j) {
            const int kt = 2 * pc + j;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            if (kt < nt) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_row_frag<HD>(R0, kt, ks, g, c), qf[ks], a, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_row_frag<HD>(R1, kt, ks, g, c), gf[ks], dp, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kt + 4 * g + r;
                const bool ok = key < L && !(causal && key > query);
                a[r] = ok ? a[r] * sc2 : -INFINITY;
            }
            s[j] = a;
            e[j] = dp;
        }
    };

    // ---- phase A
    for (int qt = wave; qt < nt; qt += nwaves) {
        const int query = 16 * qt + c;
        bf16x8 qf[KS], gf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = at_global_frag<HD>(qbase, ld3, L, qt, ks, g, c);
            gf[ks] = at_global_frag<HD>(gbase, d, L, qt, ks, g, c);
        }
        float ls, dl;
        if constexpr (HAVE_LSE) {
            // the forward kept its log-sum-exp and its output: delta = sum_k P dP = rowsum(dO * O) (P dP = P (dO . V) summed over
            // the keys is dO . O), so the first of the two sweeps over the keys is not needed
            float part = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 of = at_global_frag<HD>(fwd_out + (long)b * L * d + h * HD, d, L, qt, ks, g, c);
#pragma unroll
                for (int k = 0; k < 8; ++k) part += (float)gf[ks][k] * (float)of[k];
            }
            dl = group_sum(part);
            ls = query < L ? lse_in[(long)blockIdx.x * L + query] : 1e30f;
        } else {
        // sweep 1: log-sum-exp and delta = sum_k P dP, both with the online rescaling
        float m2 = -INFINITY, l = 0.f, num = 0.f;
        for (int pc = 0; pc < np; pc += ATL_CHB / 2) {
            if (causal && 32 * pc > 16 * qt + 15) break;
            f32x4 s[ATL_CHB], e[ATL_CHB];
            chunk(pc, query, qf, gf, s, e);
            float cm = -INFINITY;
#pragma unroll
            for (int j = 0; j < ATL_CHB; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) cm = fmaxf(cm, s[j][r]);
            cm = group_max(cm);
            const float mn = fmaxf(m2, cm);
            const float alpha = __builtin_amdgcn_exp2f(m2 - mn);
            l *= alpha;
            num *= alpha;
#pragma unroll
            for (int j = 0; j < ATL_CHB; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pe = __builtin_amdgcn_exp2f(s[j][r] - mn);
                    l += pe;
                    num += pe * e[j][r];
                }
            m2 = mn;
        }
        l = group_sum(l);
        num = group_sum(num);
        ls = m2 + log2f(l);
        dl = num / l;
        }
        if (g == 0) {
            lse2[query] = FAST ? -ls : ls;
            delta[query] = FAST ? -dl * scale : dl;
        }
        // sweep 2: dS^T = P^T (dP^T - delta) scale, dQ += dS K
        f32x4 dq[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (FAST) {
            const f32x2 nls2 = {-ls, -ls}, ndl2 = {-dl * scale, -dl * scale};
            // NSL slices of 32 keys (two key tiles each) starting at slice pc; `pad`: the chunk holds rows behind L
            auto sweep = [&](auto nsl_c, int pc, bool pad) {
                constexpr int NSL = decltype(nsl_c)::value, NTL = 2 * NSL;
                const char* Kc = R0 + pc * 32 * ROWB;
                const char* Vc = R1 + pc * 32 * ROWB;
                f32x4 s[NTL];
#pragma unroll
                for (int j = 0; j < NTL; ++j) {
                    f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kc + j * 16 * ROWB + kq[0]), qf[0],
                                                                      (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Vc + j * 16 * ROWB + kq[0]), gf[0],
                                                                       (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                    for (int ks = 1; ks < KS; ++ks) {
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Kc + j * 16 * ROWB + kq[ks]), qf[ks], a, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Vc + j * 16 * ROWB + kq[ks]), gf[ks], dp, 0, 0, 0);
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x2 t = __builtin_elementwise_fma((f32x2){a[2 * h], a[2 * h + 1]}, sc22, nls2);
                        const f32x2 u = __builtin_elementwise_fma((f32x2){dp[2 * h], dp[2 * h + 1]}, scale2, ndl2);
                        const f32x2 pe = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
                        const f32x2 ds = pe * u;
                        a[2 * h] = ds[0];
                        a[2 * h + 1] = ds[1];
                    }
                    s[j] = a;
                }
                if (pad) {
#pragma unroll
                    for (int j = 0; j < NTL; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (32 * pc + 16 * j + 4 * g + r >= L) s[j][r] = 0.f;
                }
#pragma unroll
                for (int jp = 0; jp < NSL; ++jp) {
                    const bf16x8 df = pack_pair(s[2 * jp], s[2 * jp + 1]);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            lds_tr8(Kc + jp * 32 * ROWB + vt0[dt], Kc + (jp * 32 + 16) * ROWB + vt0[dt]), df, dq[dt], 0, 0, 0);
                }
            };
            int pc = 0;
            for (; pc + 2 <= np; pc += 2) sweep(std::integral_constant<int, 2>{}, pc, 32 * pc + 64 > L);
            if (pc < np) sweep(std::integral_constant<int, 1>{}, pc, 32 * pc + 32 > L);
        } else
        for (int pc = 0; pc < np; pc += ATL_CHB / 2) {
            if (causal && 32 * pc > 16 * qt + 15) break;
            f32x4 s[ATL_CHB], e[ATL_CHB];
            chunk(pc, query, qf, gf, s, e);
#pragma unroll
            for (int j = 0; j < ATL_CHB; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[j][r] = __builtin_amdgcn_exp2f(s[j][r] - ls) * (e[j][r] - dl) * scale;
#pragma unroll
            for (int jp = 0; jp < ATL_CHB / 2; ++jp) {
                const int sp = pc + jp;
                if (sp < np) {
                    const bf16x8 df = pack_pair(s[2 * jp], s[2 * jp + 1]);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_tr_frag<HD>(R0, sp, dt, g, q, p), df, dq[dt], 0, 0, 0);
                }
            }
        }
        at_store_tile<HD>(dbase, ld3, L, 16 * qt, dq, 1.0f, lane);
    }
    __syncthreads();
    at_stage2<HD, AtCfg<HD>::STAGE_U>(R0, qbase, ld3, R1, gbase, d, L, LP);     // Q, dO
    __syncthreads();

    // ---- phase B: wave = one 16-key tile, query tiles walked in pairs
    for (int kt = wave; kt < nt; kt += nwaves) {
        const int key = 16 * kt + c;
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = at_global_frag<HD>(qbase + d, ld3, L, kt, ks, g, c);
            vf[ks] = at_global_frag<HD>(qbase + 2 * d, ld3, L, kt, ks, g, c);
        }
        f32x4 dv[DT], dk[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) { dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        if constexpr (FAST) {
            const bool tail_k = 16 * kt + 16 > L;               // the one key tile with columns behind L
            for (int sp = 0; sp < np; ++sp) {
                const char* Qc = R0 + sp * 32 * ROWB;
                const char* Gc = R1 + sp * 32 * ROWB;
                f32x4 pt[2], dst[2];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Qc + hh * 16 * ROWB + kq[0]), kf[0],
                                                                      (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    f32x4 e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Gc + hh * 16 * ROWB + kq[0]), vf[0],
                                                                      (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                    for (int ks = 1; ks < KS; ++ks) {
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Qc + hh * 16 * ROWB + kq[ks]), kf[ks], a, 0, 0, 0);
                        e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_read8(Gc + hh * 16 * ROWB + kq[ks]), vf[ks], e, 0, 0, 0);
                    }
                    const f32x4 nls = *reinterpret_cast<const f32x4*>(lse2 + 32 * sp + 16 * hh + 4 * g);     // -lse (padded queries: -1e30)
                    const f32x4 ndl = *reinterpret_cast<const f32x4*>(delta + 32 * sp + 16 * hh + 4 * g);    // -delta * scale
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x2 t = __builtin_elementwise_fma((f32x2){a[2 * h], a[2 * h + 1]}, sc22, (f32x2){nls[2 * h], nls[2 * h + 1]});
                        const f32x2 u = __builtin_elementwise_fma((f32x2){e[2 * h], e[2 * h + 1]}, scale2, (f32x2){ndl[2 * h], ndl[2 * h + 1]});
                        const f32x2 pr = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
                        const f32x2 ds = pr * u;
                        a[2 * h] = pr[0];
                        a[2 * h + 1] = pr[1];
                        e[2 * h] = ds[0];
                        e[2 * h + 1] = ds[1];
                    }
                    if (tail_k && key >= L) { a = (f32x4){0.f, 0.f, 0.f, 0.f}; e = (f32x4){0.f, 0.f, 0.f, 0.f}; }
                    pt[hh] = a;
                    dst[hh] = e;
                }
                const bf16x8 pf = pack_pair(pt[0], pt[1]);
                const bf16x8 df = pack_pair(dst[0], dst[1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr8(Gc + vt0[dt], Gc + 16 * ROWB + vt0[dt]), pf, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_tr8(Qc + vt0[dt], Qc + 16 * ROWB + vt0[dt]), df, dk[dt], 0, 0, 0);
                }
            }
        } else {
        const int sp0 = causal ? (kt >> 1) : 0;               // queries before the key tile see none of its keys
        for (int sp = sp0; sp < np; ++sp) {
            f32x4 pt[2], dst[2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int qt = 2 * sp + hh;
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_row_frag<HD>(R0, qt, ks, g, c), kf[ks], a, 0, 0, 0);
                    e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_row_frag<HD>(R1, qt, ks, g, c), vf[ks], e, 0, 0, 0);
                }
                const f32x4 ls = *reinterpret_cast<const f32x4*>(lse2 + 16 * qt + 4 * g);
                const f32x4 dl = *reinterpret_cast<const f32x4*>(delta + 16 * qt + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int query = 16 * qt + 4 * g + r;
                    const bool ok = key < L && query < L && !(causal && key > query);
                    const float pr = ok ? __builtin_amdgcn_exp2f(a[r] * sc2 - ls[r]) : 0.f;
                    a[r] = pr;
                    e[r] = pr * (e[r] - dl[r]) * scale;
                }
                pt[hh] = a;
                dst[hh] = e;
            }
            const bf16x8 pf = pack_pair(pt[0], pt[1]);
            const bf16x8 df = pack_pair(dst[0], dst[1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_tr_frag<HD>(R1, sp, dt, g, q, p), pf, dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_tr_frag<HD>(R0, sp, dt, g, q, p), df, dk[dt], 0, 0, 0);
            }
        }
        }
        at_store_tile<HD>(dbase + d, ld3, L, 16 * kt, dk, 1.0f, lane);
        at_store_tile<HD>(dbase + 2 * d, ld3, L, 16 * kt, dv, 1.0f, lane);
    }
}

// ---- launches
// runtime bools -> std::bool_constant arguments of a generic lambda: one kernel instantiation per combination
template <typename F>
static void with_bools(F&& f) { f(); }
template <typename F, typename... Rest>
static void with_bools(F&& f, bool b, Rest... rest) {
    if (b) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
// experiment switches, each read once: CLIPX_ATTN_WAVES / CLIPX_ATTN_BWD4_WAVES override the waves per block of the forward and
// online-softmax kernels / of the four-image backward; CLIPX_ATTN_GENERIC=1 sends everything to the generic tiled kernels
static int env_int(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }
static int attn_waves_override() { static const int v = env_int("CLIPX_ATTN_WAVES"); return v; }
static int attn_bwd4_waves_override() { static const int v = env_int("CLIPX_ATTN_BWD4_WAVES"); return v; }
static bool attn_force_generic() {
    static const bool v = [] { const char* e = getenv("CLIPX_ATTN_GENERIC"); return e && e[0] == '1'; }();
    return v;
}

// largest L whose two operand images (+ lse / delta in the backward) fit the 160 KiB of LDS
template <int HD>
static int atl_max_l() { return HD <= 64 ? 608 : 288; }

template <int HD>
static int launch_bf16_long(bool bwd, int batch, int L, int heads, int causal, const void* qkv, const void* dout, void* out,
                            hipStream_t stream, const void* fwd_out = nullptr, float* lse = nullptr) {
    const int LP = ((L + 31) / 32) * 32;
    const size_t lds = (size_t)2 * LP * AtCfg<HD>::ROWB + (bwd ? (size_t)2 * LP * sizeof(float) : 0);
    CLIPX_CHECK(lds <= 160 * 1024, "long attention: L=%d does not fit LDS", L);
    const int nt = (L + 15) / 16;
    // One block per CU when the images take more than half the LDS: as many waves as it may have (16 measured best at L = 577).
    // When two blocks fit (L <= 320 at head dim 64) 8 waves each, so that both are resident within the 16 wave slots that 128
    // VGPRs allow and one block's staging runs beside the other's MFMA phase (L = 197: 8 waves 0.194 / 0.580 ms, 13 waves
    // 0.254 / 0.679, 7 waves 0.210 / 0.614 -- profiles/r03_attention_long.txt).
    int waves = 2 * lds <= 160 * 1024 ? (nt < 8 ? nt : 8) : nt;
    if (attn_waves_override() > 0) waves = attn_waves_override();
    const int maxw = bwd ? AtCfg<HD>::MAXW_B : AtCfg<HD>::MAXW_F;
    if (waves > maxw) waves = maxw;
    if (waves < 1) waves = 1;
    if (bwd) {
        const bool have_lse = fwd_out != nullptr && lse != nullptr;
        with_bools([&](auto lse_c, auto causal_c) {
            auto kernel = attn_bf16_long_bwd_kernel<HD, decltype(lse_c)::value, decltype(causal_c)::value>;
            (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kernel, dim3(batch * heads), dim3(64 * waves), lds, stream, L, heads, (const bf16_t*)qkv,
                               (const bf16_t*)dout, (bf16_t*)out, have_lse ? (const bf16_t*)fwd_out : nullptr,
                               have_lse ? (const float*)lse : nullptr);
        }, have_lse, causal != 0);
    } else {
        with_bools([&](auto causal_c) {
            auto kernel = attn_bf16_long_fwd_kernel<HD, decltype(causal_c)::value>;
            (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kernel, dim3(batch * heads), dim3(64 * waves), lds, stream, L, heads, (const bf16_t*)qkv,
                               (bf16_t*)out, lse);
        }, causal != 0);
    }
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// whole-sequence kernels: NT tiles of 16 rows, head dim 64
template <int NT>
static int launch_bf16(bool bwd, int batch, int L, int heads, int causal, const void* qkv, const void* dout,
                       void* out, hipStream_t stream, const int* seq_ids = nullptr, const int* cu_rows = nullptr) {
    constexpr int LP = 16 * NT;
    const int nt_used = (L + 15) / 16;
    // (a dense batch whose L does not fill its NT tiles -- L <= 16 (NT - 1) -- takes the guarded form as well)
    const bool packed = cu_rows != nullptr || nt_used != NT;
    if (bwd) {
        // four images: 4 x LP x 128 B still leaves >= 2 blocks per CU at NT = 8
        const size_t lds = (size_t)4 * LP * AT_ROWB + 2 * LP * sizeof(float);
        // one 16-row tile per wave up to 4 tiles (32.5 KiB of LDS: four blocks of four waves per CU); beyond that two tiles per
        // wave -- measured at b = 4096 (scripts/bench_attn.py, profiles/r03_attention_bwd4.txt): L = 50: 4 waves 497 us, 3: 550,
        // 2: 556 (the earlier two-image kernel 588); L = 77: 5 waves 937 us, 3: 572, 2: 687 (two-image 658)
        int waves = NT <= 4 ? nt_used : (nt_used + 1) / 2;
        const int wv = attn_bwd4_waves_override();
        if (wv > 0 && wv <= nt_used) waves = wv;
        with_bools([&](auto causal_c, auto packed_c) {
            auto kernel = attn_bf16_bwd4_kernel<NT, decltype(causal_c)::value, decltype(packed_c)::value>;
            (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kernel, dim3(batch * heads), dim3(64 * waves), lds, stream, L, heads, (const bf16_t*)qkv,
                               (const bf16_t*)dout, (bf16_t*)out, seq_ids, cu_rows);
        }, causal != 0, packed);
    } else {
        const size_t lds = (size_t)2 * LP * AT_ROWB;
        // Two 16-row tiles per wave: blocks of half as many waves, so more (sample, head) blocks are resident per CU and one
        // block's staging overlaps another's MFMA phase.  Measured at b=4096 (scripts/bench_attn.py): L=77 forward 412 -> 325 us
        // (the two-image backward of the time 966 -> 728 us) with 3 waves instead of 5; one wave per block is slower again.
        int waves = (nt_used + 1) / 2;
        const int wv = attn_waves_override();
        if (wv > 0 && wv <= nt_used && wv <= 16) waves = wv;
        with_bools([&](auto causal_c, auto packed_c) {
            auto kernel = attn_bf16_fwd_kernel<NT, decltype(causal_c)::value, decltype(packed_c)::value>;
            (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kernel, dim3(batch * heads), dim3(64 * waves), lds, stream, L, heads, (const bf16_t*)qkv,
                               (bf16_t*)out, seq_ids, cu_rows);
        }, causal != 0, packed);
    }
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// =============================================================================== generic tiled kernels
// Any sequence length and head dim in {32, 64, 80, 128}, fp32 or bf16 storage, fp32 arithmetic: one thread per query
// (key) row, the other operand streamed through LDS in tiles of AT_TK rows with an online softmax.  This is the
// coverage path for shapes the MFMA kernels do not take yet (ViT-L/14-336: 577 tokens; ViT-H/14: head dim 80) and for
// fp32 sequences whose K and V do not fit LDS whole; it is scalar-FMA bound and far from the MFMA roofline.
#define AT_TK 64
template <typename T, int HD>
__global__ __launch_bounds__(128) void attn_gen_fwd_kernel(int L, int heads, int causal, const T* __restrict__ qkv,
                                                           T* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ks = sm;
    float* Vs = sm + AT_TK * HD;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int d = heads * HD;
    const T* base = qkv + (long)b * L * 3 * d + h * HD;
    const float scale = rsqrtf((float)HD);
    for (int c0 = 0; c0 < L; c0 += 128) {
        const int i = c0 + threadIdx.x;
        const bool act = i < L;
        float q[HD], o[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) { q[k] = act ? (float)base[(long)i * 3 * d + k] : 0.f; o[k] = 0.f; }
        float m = -INFINITY, l = 0.f;
        const int kend = causal ? min(L, c0 + 128) : L;
        for (int t0 = 0; t0 < kend; t0 += AT_TK) {
            __syncthreads();
            for (int idx = threadIdx.x; idx < AT_TK * HD; idx += 128) {
                const int r = t0 + idx / HD, cc = idx % HD;
                Ks[idx] = r < L ? (float)base[(long)r * 3 * d + d + cc] : 0.f;
                Vs[idx] = r < L ? (float)base[(long)r * 3 * d + 2 * d + cc] : 0.f;
            }
            __syncthreads();
            const int jmax = min(AT_TK, (causal ? i + 1 : L) - t0);
            if (act)
                for (int j = 0; j < jmax; ++j) {
                    float sc = 0.f;
#pragma unroll
                    for (int k = 0; k < HD; ++k) sc += q[k] * Ks[j * HD + k];
                    sc *= scale;
                    const float mn = fmaxf(m, sc);
                    const float a = expf(m - mn), pp = expf(sc - mn);
                    l = l * a + pp;
#pragma unroll
                    for (int k = 0; k < HD; ++k) o[k] = o[k] * a + pp * Vs[j * HD + k];
                    m = mn;
                }
        }
        if (act) {
            const float inv = 1.0f / l;
            T* orow = out + ((long)b * L + i) * d + h * HD;
#pragma unroll
            for (int k = 0; k < HD; ++k) orow[k] = (T)(o[k] * inv);
        }
    }
}

template <typename T, int HD>
__global__ __launch_bounds__(128) void attn_gen_bwd_kernel(int L, int heads, int causal, const T* __restrict__ qkv,
                                                           const T* __restrict__ dout, T* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* A = sm;                          // phase 1: K tile   phase 2: Q tile
    float* B = sm + AT_TK * HD;             // phase 1: V tile   phase 2: dO tile
    float* lse = B + AT_TK * HD;            // [L]
    float* delta = lse + L;                 // [L]
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int d = heads * HD;
    const T* base = qkv + (long)b * L * 3 * d + h * HD;
    const T* dob = dout + (long)b * L * d + h * HD;
    T* dbase = dqkv + (long)b * L * 3 * d + h * HD;
    const float scale = rsqrtf((float)HD);
    auto load_kv = [&](int t0) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < AT_TK * HD; idx += 128) {
            const int r = t0 + idx / HD, cc = idx % HD;
            A[idx] = r < L ? (float)base[(long)r * 3 * d + d + cc] : 0.f;
            B[idx] = r < L ? (float)base[(long)r * 3 * d + 2 * d + cc] : 0.f;
        }
        __syncthreads();
    };
    auto load_qdo = [&](int t0) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < AT_TK * HD; idx += 128) {
            const int r = t0 + idx / HD, cc = idx % HD;
            A[idx] = r < L ? (float)base[(long)r * 3 * d + cc] : 0.f;
            B[idx] = r < L ? (float)dob[(long)r * d + cc] : 0.f;
        }
        __syncthreads();
    };
    // ---- phase 1: per query row -> lse, delta, dq (three passes over the key tiles: registers hold q, dO, dq)
    for (int c0 = 0; c0 < L; c0 += 128) {
        const int i = c0 + threadIdx.x;
        const bool act = i < L;
        const int kend = causal ? min(L, c0 + 128) : L;
        const int jlim = causal ? i + 1 : L;
        float q[HD], go[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) {
            q[k] = act ? (float)base[(long)i * 3 * d + k] : 0.f;
            go[k] = act ? (float)dob[(long)i * d + k] : 0.f;
        }
        float m = -INFINITY, l = 0.f;
        for (int t0 = 0; t0 < kend; t0 += AT_TK) {
            load_kv(t0);
            const int jmax = min(AT_TK, jlim - t0);
            if (act)
                for (int j = 0; j < jmax; ++j) {
                    float sc = 0.f;
#pragma unroll
                    for (int k = 0; k < HD; ++k) sc += q[k] * A[j * HD + k];
                    sc *= scale;
                    const float mn = fmaxf(m, sc);
                    l = l * expf(m - mn) + expf(sc - mn);
                    m = mn;
                }
        }
        const float ls = m + logf(l);
        float dl = 0.f;
        for (int t0 = 0; t0 < kend; t0 += AT_TK) {
            load_kv(t0);
            const int jmax = min(AT_TK, jlim - t0);
            if (act)
                for (int j = 0; j < jmax; ++j) {
                    float sc = 0.f, dp = 0.f;
#pragma unroll
                    for (int k = 0; k < HD; ++k) { sc += q[k] * A[j * HD + k]; dp += go[k] * B[j * HD + k]; }
                    dl += expf(sc * scale - ls) * dp;
                }
        }
        float dq[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) dq[k] = 0.f;
        for (int t0 = 0; t0 < kend; t0 += AT_TK) {
            load_kv(t0);
            const int jmax = min(AT_TK, jlim - t0);
            if (act)
                for (int j = 0; j < jmax; ++j) {
                    float sc = 0.f, dp = 0.f;
#pragma unroll
                    for (int k = 0; k < HD; ++k) { sc += q[k] * A[j * HD + k]; dp += go[k] * B[j * HD + k]; }
                    const float ds = expf(sc * scale - ls) * (dp - dl) * scale;
#pragma unroll
                    for (int k = 0; k < HD; ++k) dq[k] += ds * A[j * HD + k];
                }
        }
        if (act) {
            lse[i] = ls;
            delta[i] = dl;
#pragma unroll
            for (int k = 0; k < HD; ++k) dbase[(long)i * 3 * d + k] = (T)dq[k];
        }
    }
    __syncthreads();
    // ---- phase 2: per key row -> dv, then dk (two passes over the query tiles)
    for (int c0 = 0; c0 < L; c0 += 128) {
        const int j = c0 + threadIdx.x;
        const bool act = j < L;
        const int ibeg_u = causal ? (c0 / AT_TK) * AT_TK : 0;      // first query tile any row of this chunk needs
        const int ibeg = causal ? j : 0;
        float kk[HD], acc[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) { kk[k] = act ? (float)base[(long)j * 3 * d + d + k] : 0.f; acc[k] = 0.f; }
        for (int t0 = ibeg_u; t0 < L; t0 += AT_TK) {
            load_qdo(t0);
            if (act)
                for (int r = max(0, ibeg - t0); r < min(AT_TK, L - t0); ++r) {
                    float sc = 0.f;
#pragma unroll
                    for (int k = 0; k < HD; ++k) sc += A[r * HD + k] * kk[k];
                    const float pp = expf(sc * scale - lse[t0 + r]);
#pragma unroll
                    for (int k = 0; k < HD; ++k) acc[k] += pp * B[r * HD + k];
                }
        }
        float vv[HD];
#pragma unroll
        for (int k = 0; k < HD; ++k) {
            if (act) dbase[(long)j * 3 * d + 2 * d + k] = (T)acc[k];
            acc[k] = 0.f;
            vv[k] = act ? (float)base[(long)j * 3 * d + 2 * d + k] : 0.f;
        }
        for (int t0 = ibeg_u; t0 < L; t0 += AT_TK) {
            load_qdo(t0);
            if (act)
                for (int r = max(0, ibeg - t0); r < min(AT_TK, L - t0); ++r) {
                    float sc = 0.f, dp = 0.f;
#pragma unroll
                    for (int k = 0; k < HD; ++k) { sc += A[r * HD + k] * kk[k]; dp += B[r * HD + k] * vv[k]; }
                    const float ds = expf(sc * scale - lse[t0 + r]) * (dp - delta[t0 + r]) * scale;
#pragma unroll
                    for (int k = 0; k < HD; ++k) acc[k] += ds * A[r * HD + k];
                }
        }
        if (act) {
#pragma unroll
            for (int k = 0; k < HD; ++k) dbase[(long)j * 3 * d + d + k] = (T)acc[k];
        }
    }
}

template <typename T, int HD>
static int launch_gen(bool bwd, int batch, int L, int heads, int causal, const void* qkv, const void* dout, void* out,
                      hipStream_t stream) {
    const size_t lds = ((size_t)2 * AT_TK * HD + (bwd ? 2 * L : 0)) * sizeof(float);
    CLIPX_CHECK(lds <= 160 * 1024, "generic attention: L=%d does not fit LDS", L);
    if (bwd) {
        (void)hipFuncSetAttribute((const void*)attn_gen_bwd_kernel<T, HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((attn_gen_bwd_kernel<T, HD>), dim3(batch * heads), dim3(128), lds, stream, L, heads, causal,
                           (const T*)qkv, (const T*)dout, (T*)out);
    } else {
        (void)hipFuncSetAttribute((const void*)attn_gen_fwd_kernel<T, HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((attn_gen_fwd_kernel<T, HD>), dim3(batch * heads), dim3(128), lds, stream, L, heads, causal,
                           (const T*)qkv, (T*)out);
    }
    CLIPX_LAUNCH_CHECK();
    return 0;
}
template <typename T>
static int dispatch_gen(bool bwd, int batch, int L, int heads, int hd, int causal, const void* qkv, const void* dout,
                        void* out, hipStream_t stream) {
    if (hd == 32) return launch_gen<T, 32>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    if (hd == 64) return launch_gen<T, 64>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    if (hd == 80) return launch_gen<T, 80>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    if (hd == 128) return launch_gen<T, 128>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    clipx_set_error("attention: head dim %d unsupported (32, 64, 80, 128)", hd);
    return -1;
}

// =============================================================================== dispatch and C ABI
// the shapes the online-softmax kernels take: the only ones with a log-sum-exp hand-over between forward and backward.
// Head dim 64: the whole-sequence kernels up to 128 rows, these beyond.  (Until round 3 they started at 225 and a 14-tile
// whole-sequence instantiation took 129..224: at L = 197 (ViT-B/16, b = 512 x 12 heads) it ran 0.249 / 0.667 ms fwd / bwd against
// 0.194 / 0.580 ms for these kernels with two 8-wave blocks per CU and the log-sum-exp hand-over.)
static bool bf16_long_applies(int L, int hd) {
    if (attn_force_generic()) return false;
    return (hd == 64 && L > 128 && L <= atl_max_l<64>()) || (hd == 80 && L <= atl_max_l<80>());
}
static int dispatch_bf16(bool bwd, int batch, int L, int heads, int hd, int causal, const void* qkv, const void* dout,
                         void* out, hipStream_t stream) {
    if (bf16_long_applies(L, hd)) {                                      // online-softmax MFMA kernels
        if (hd == 64) return launch_bf16_long<64>(bwd, batch, L, heads, causal, qkv, dout, out, stream);   // ViT-B/16, ViT-L/14-336
        return launch_bf16_long<80>(bwd, batch, L, heads, causal, qkv, dout, out, stream);                 // ViT-H/14
    }
    if (hd != AT_HD || L > 128 || attn_force_generic())                  // whole-sequence MFMA kernels: head dim 64, L <= 128
        return dispatch_gen<bf16_t>(bwd, batch, L, heads, hd, causal, qkv, dout, out, stream);
    if (L <= 32) return launch_bf16<2>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    if (L <= 64) return launch_bf16<4>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    if (L <= 96) return launch_bf16<6>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    return launch_bf16<8>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
}

template <int HD>
static int launch_f32(bool bwd, int batch, int L, int heads, int causal, const void* qkv, const void* dout, void* out,
                      hipStream_t stream, const int* seq_ids = nullptr, const int* cu_rows = nullptr) {
    const size_t lds = ((size_t)2 * L * HD + (bwd ? 2 * L : 0)) * sizeof(float);
    CLIPX_CHECK(lds <= 160 * 1024, "fp32 attention: L=%d does not fit LDS", L);
    if (bwd) {
        (void)hipFuncSetAttribute((const void*)attn_f32_bwd_kernel<HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(attn_f32_bwd_kernel<HD>, dim3(batch * heads), dim3(128), lds, stream, L, heads, causal,
                           (const float*)qkv, (const float*)dout, (float*)out, seq_ids, cu_rows);
    } else {
        (void)hipFuncSetAttribute((const void*)attn_f32_fwd_kernel<HD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(attn_f32_fwd_kernel<HD>, dim3(batch * heads), dim3(128), lds, stream, L, heads, causal,
                           (const float*)qkv, (float*)out, seq_ids, cu_rows);
    }
    CLIPX_LAUNCH_CHECK();
    return 0;
}

static int dispatch(bool bwd, int dtype, int batch, int L, int heads, int hd, int causal, const void* qkv,
                    const void* dout, void* out, hipStream_t stream) {
    if (batch <= 0) return 0;
    if (dtype == CLIPX_BF16) return dispatch_bf16(bwd, batch, L, heads, hd, causal, qkv, dout, out, stream);
    CLIPX_CHECK(dtype == CLIPX_F32, "attention: bad dtype");
    const size_t whole = ((size_t)2 * L * hd + (bwd ? 2 * L : 0)) * sizeof(float);
    if (whole > 160 * 1024 || attn_force_generic() || (hd != 32 && hd != 64 && hd != 80))
        return dispatch_gen<float>(bwd, batch, L, heads, hd, causal, qkv, dout, out, stream);
    if (hd == 32) return launch_f32<32>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    if (hd == 64) return launch_f32<64>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    if (hd == 80) return launch_f32<80>(bwd, batch, L, heads, causal, qkv, dout, out, stream);
    clipx_set_error("fp32 attention: head dim %d unsupported", hd);
    return -1;
}

extern "C" int clipx_attention_fwd(int dtype, int batch, int L, int heads, int hd, int causal, const void* qkv,
                                   void* out, void* stream) {
    return dispatch(false, dtype, batch, L, heads, hd, causal, qkv, nullptr, out, (hipStream_t)stream);
}
extern "C" int clipx_attention_bwd(int dtype, int batch, int L, int heads, int hd, int causal, const void* qkv,
                                   const void* dout, void* dqkv, void* stream) {
    return dispatch(true, dtype, batch, L, heads, hd, causal, qkv, dout, dqkv, (hipStream_t)stream);
}
// Forward / backward with the log-sum-exp handed over (flash-attention's saved statistic): 1 when the shape runs on the
// online-softmax kernels, whose backward otherwise spends a third of its work on re-deriving it.
extern "C" int clipx_attention_lse_supported(int dtype, int L, int hd) {
    return dtype == CLIPX_BF16 && bf16_long_applies(L, hd) ? 1 : 0;
}
extern "C" int clipx_attention_fwd_lse(int dtype, int batch, int L, int heads, int hd, int causal, const void* qkv, void* out,
                                       float* lse, void* stream) {
    CLIPX_CHECK(clipx_attention_lse_supported(dtype, L, hd) && lse != nullptr, "attention_fwd_lse: shape L=%d hd=%d has no lse path", L, hd);
    if (batch <= 0) return 0;
    if (hd == 64) return launch_bf16_long<64>(false, batch, L, heads, causal, qkv, nullptr, out, (hipStream_t)stream, nullptr, lse);
    return launch_bf16_long<80>(false, batch, L, heads, causal, qkv, nullptr, out, (hipStream_t)stream, nullptr, lse);
}
extern "C" int clipx_attention_bwd_lse(int dtype, int batch, int L, int heads, int hd, int causal, const void* qkv, const void* dout,
                                       const void* out, const float* lse, void* dqkv, void* stream) {
    CLIPX_CHECK(clipx_attention_lse_supported(dtype, L, hd) && lse != nullptr && out != nullptr,
                "attention_bwd_lse: shape L=%d hd=%d has no lse path", L, hd);
    if (batch <= 0) return 0;
    if (hd == 64)
        return launch_bf16_long<64>(true, batch, L, heads, causal, qkv, dout, dqkv, (hipStream_t)stream, out, const_cast<float*>(lse));
    return launch_bf16_long<80>(true, batch, L, heads, causal, qkv, dout, dqkv, (hipStream_t)stream, out, const_cast<float*>(lse));
}

// ---- packed rows (sequences of different lengths back to back; clipx_text_layout): block i handles sequence
// seq_ids[i] (or i), rows cu_rows[s] .. cu_rows[s+1]; max_len bounds every sequence of THIS launch and picks the
// kernel's padded tile count, so callers launch once per length bucket and short captions skip the key tiles a padded
// 77-row layout would compute and mask.
static int dispatch_packed(bool bwd, int dtype, int nseq, int max_len, int heads, int hd, int causal, const int* seq_ids,
                           const int* cu_rows, const void* qkv, const void* dout, void* out, hipStream_t stream) {
    if (nseq <= 0) return 0;
    CLIPX_CHECK(cu_rows != nullptr && max_len > 0, "packed attention: cu_rows / max_len");
    if (dtype == CLIPX_BF16) {
        CLIPX_CHECK(hd == AT_HD && max_len <= 128, "packed bf16 attention: head dim 64 and sequences of <= 128 rows (got %d, %d)",
                    hd, max_len);
        if (max_len <= 32) return launch_bf16<2>(bwd, nseq, max_len, heads, causal, qkv, dout, out, stream, seq_ids, cu_rows);
        if (max_len <= 64) return launch_bf16<4>(bwd, nseq, max_len, heads, causal, qkv, dout, out, stream, seq_ids, cu_rows);
        if (max_len <= 96) return launch_bf16<6>(bwd, nseq, max_len, heads, causal, qkv, dout, out, stream, seq_ids, cu_rows);
        return launch_bf16<8>(bwd, nseq, max_len, heads, causal, qkv, dout, out, stream, seq_ids, cu_rows);
    }
    CLIPX_CHECK(dtype == CLIPX_F32, "packed attention: bad dtype");
    if (hd == 32) return launch_f32<32>(bwd, nseq, max_len, heads, causal, qkv, dout, out, stream, seq_ids, cu_rows);
    if (hd == 64) return launch_f32<64>(bwd, nseq, max_len, heads, causal, qkv, dout, out, stream, seq_ids, cu_rows);
    if (hd == 80) return launch_f32<80>(bwd, nseq, max_len, heads, causal, qkv, dout, out, stream, seq_ids, cu_rows);
    clipx_set_error("packed fp32 attention: head dim %d unsupported", hd);
    return -1;
}
extern "C" int clipx_attention_packed_fwd(int dtype, int nseq, int max_len, int heads, int hd, int causal, const int* seq_ids,
                                          const int* cu_rows, const void* qkv, void* out, void* stream) {
    return dispatch_packed(false, dtype, nseq, max_len, heads, hd, causal, seq_ids, cu_rows, qkv, nullptr, out, (hipStream_t)stream);
}
extern "C" int clipx_attention_packed_bwd(int dtype, int nseq, int max_len, int heads, int hd, int causal, const int* seq_ids,
                                          const int* cu_rows, const void* qkv, const void* dout, void* dqkv, void* stream) {
    return dispatch_packed(true, dtype, nseq, max_len, heads, hd, causal, seq_ids, cu_rows, qkv, dout, dqkv, (hipStream_t)stream);
}
