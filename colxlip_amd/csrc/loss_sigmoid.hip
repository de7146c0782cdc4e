// Fused sigmoid contrastive loss (SigLipLoss, reference loss.py:498-521) that never holds the logits matrix.
//
//   z[i,j] = s * (A[i] . B[j]) + beta           (A [r, E], B [c, E] fp32; s = logit_scale, beta = logit_bias, both on the device)
//   y[i,j] = +1 where j == i + pos_off, -1 elsewhere (pos_off < 0: no positives, the reference's negative_only)
//   loss   = 1/r * sum softplus(-y z),   dz = -1/r * y * sigmoid(-y z)
//   dA = s * dz @ B,  dB = s * dz^T @ A,  d(s) = sum dz * (A . B),  d(beta) = sum dz
//
// Every product is exact fp32 (v_mfma_f32_16x16x4_f32 == an fmaf chain) on 64x64 tiles, as in loss_fused.hip.  The
// per-element gradient needs no row statistics, so one walk does everything the A side needs:
//   forward   (gradient wanted) a block owns 64 rows of A and walks B's 64-row tiles: recompute the z tile, form dz and the
//             loss / d(s) / d(beta) partials, accumulate dz . B_tile into 64 x E registers = dA at unit upstream gradient.
//   backward  the mirrored walk: a block owns 64 rows of B, walks A, accumulates dz^T . A_tile = dB.
//   no_grad   the walk without the product: loss only.
// FLOPs: 2 (forward: recompute + product) + 2 (backward) = 4 logits-GEMM equivalents, against the CE path's 5.
// The walks are split over gridDim.y blocks; split partials and block partials are summed in a fixed order (no atomics:
// the same result every run).  Embed dims outside ops.FUSED_CE_DIMS run sig_dense_kernel on a materialised logits matrix.
// The tile engine is loss_tile.h.
#include "loss_tile.h"

// one logit's share: x = -y z;  softplus(x) = max(x, 0) + log1p(exp(-|x|)),  sigmoid(x) = (x >= 0 ? 1 : e) / (1 + e), e = exp(-|x|)
// (|z| reaches ~110 at the clamped s = 100 with beta = -10: neither form overflows)
__device__ __forceinline__ float sig_term(float z, bool pos, float inv_r, float& loss) {
    const float x = pos ? -z : z;
    const float e = expf(-fabsf(x));
    loss += fmaxf(x, 0.f) + log1pf(e);
    const float sg = (x >= 0.f ? 1.f : e) / (1.f + e);
    return pos ? -inv_r * sg : inv_r * sg;
}

// A block owns rows [p0, p0+64) of P and walks its share of Q's 64-row tiles.  The positive of own row p sits at column
// q == p + pos_off (transposed: p == q + pos_off, P being the B side).  NE = E / 16 accumulator tiles per wave; NE == 0 is the
// loss-only walk (no product, E at run time).  dP_part[blockIdx.y][p][e] = sum_q dz(p,q) Q[q,e] over this block's tiles
// (unscaled); part_{loss,ds,db}[blockIdx.y * gridDim.x + blockIdx.x] the block's sums (each optional).
template <int NE>
__global__ __launch_bounds__(256, (NE <= 32 ? 2 : 1)) void sig_walk_kernel(
        int np, int nq, int E_rt, const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ scale_dev,
        const float* __restrict__ bias_dev, int pos_off, int transposed, float inv_r, float* __restrict__ dP_part,
        float* __restrict__ part_loss, float* __restrict__ part_ds, float* __restrict__ part_db) {
    constexpr int NACC = NE > 0 ? NE : 1;
    const int E = NE > 0 ? 16 * NE : E_rt;
    __shared__ float Ps[LT_BK][LT_LD];
    __shared__ float Qs[LT_BK][LT_LD];
    __shared__ float dZs[NE > 0 ? LT_T : 1][LT_T + 2];
    __shared__ float Qe[NE > 0 ? LT_T : 1][lt_ec(NE) + 16];
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int p0 = blockIdx.x * LT_T;
    int jt0, jt1;
    lt_split_range(nq, jt0, jt1);
    const float s = scale_dev[0], beta = bias_dev[0];

    f32x4 acc[NACC];
#pragma unroll
    for (int t = 0; t < NACC; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int prow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) prow[r] = p0 + 16 * wave + 4 * g + r;
    float l_part = 0.f, ds_part = 0.f, db_part = 0.f;

    for (int jt = jt0; jt < jt1; ++jt) {
        const int q0 = jt * LT_T;
        f32x4 d[4];
        lt_slab(d, Ps, Qs, P, Q, p0, np, q0, nq, E, tid, wave, g, c);
        // ---- epilogue on this wave's 16 x 64 slice (C/D map: col = lane & 15, row = 4*(lane >> 4) + reg)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = q0 + 16 * t + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = prow[r];
                float dz = 0.f;
                if (p < np && q < nq) {
                    const float dot = d[t][r];
                    const bool pos = pos_off >= 0 && (transposed ? p == q + pos_off : q == p + pos_off);
                    dz = sig_term(fmaf(s, dot, beta), pos, inv_r, l_part);
                    ds_part = fmaf(dz, dot, ds_part);
                    db_part += dz;
                }
                if constexpr (NE > 0) dZs[16 * wave + 4 * g + r][16 * t + c] = dz;
            }
        }
        if constexpr (NE > 0) lt_product<NE>(acc, dZs, Qe, Q, q0, nq, tid, wave, g, c);
    }
    if constexpr (NE > 0) lt_store_part<NE>(dP_part, acc, prow, np, 1.f, c);
    const int bid = blockIdx.y * gridDim.x + blockIdx.x;
    if (part_loss) {
        const float v = lt_block_sum(l_part, red, wave, lane);
        if (tid == 0) part_loss[bid] = v;
    }
    if (part_ds) {
        const float v = lt_block_sum(ds_part, red, wave, lane);
        if (tid == 0) part_ds[bid] = v;
    }
    if (part_db) {
        const float v = lt_block_sum(db_part, red, wave, lane);
        if (tid == 0) part_db[bid] = v;
    }
}

// out3 (+)= [inv_r * sum part_loss, sum part_ds, sum part_db], each summed in index order by its own thread (absent: 0)
__global__ void sig_sum3_kernel(int n, const float* __restrict__ part_loss, const float* __restrict__ part_ds,
                                const float* __restrict__ part_db, float inv_r, int accumulate, float* __restrict__ out3) {
    const int k = threadIdx.x;
    if (k >= 3) return;
    const float* part = k == 0 ? part_loss : (k == 1 ? part_ds : part_db);
    float acc = 0.f;
    if (part)
        for (int i = 0; i < n; ++i) acc += part[i];
    const float v = k == 0 ? inv_r * acc : acc;
    out3[k] = accumulate ? out3[k] + v : v;
}

// blocks over the q tiles of one row tile: ~3 blocks per CU in flight for the product walks, more for the loss-only walk
static int sig_split(int np, int nq, bool grad) { return lt_split(np, nq, grad ? 768 : 2048); }

// workspace: dP split partials (grad) + three arrays of block partials
static size_t sig_ws_floats(int np, int nq, int E, bool grad) {
    const size_t split = sig_split(np, nq, grad), nb = split * (size_t)cdiv(np, LT_T);
    return (grad ? split * (size_t)np * E : 0) + 3 * nb;
}

static int sig_walk(int np, int nq, int E, const float* P, const float* Q, const float* scale_dev, const float* bias_dev,
                    int pos_off, int transposed, float inv_r, float* dP_part, float* pl, float* pds, float* pdb, bool grad,
                    hipStream_t stream) {
    const dim3 grid(cdiv(np, LT_T), sig_split(np, nq, grad));
    auto launch = [&](auto ne) {
        hipLaunchKernelGGL(sig_walk_kernel<decltype(ne)::value>, grid, dim3(256), 0, stream, np, nq, E, P, Q, scale_dev, bias_dev,
                           pos_off, transposed, inv_r, dP_part, pl, pds, pdb);
    };
    if (!grad) {
        launch(std::integral_constant<int, 0>{});
        return 0;
    }
    return fused_dim_dispatch(E, launch);
}

extern "C" size_t clipx_sigmoid_fused_ws_bytes(int r, int c, int E, int grad) {
    return sig_ws_floats(r, c, E, grad != 0) * sizeof(float);
}

extern "C" int clipx_sigmoid_fused_fwd(int r, int c, int E, const float* A, const float* B, const float* scale_dev,
                                       const float* bias_dev, int pos_off, float inv_r, float* out3, float* dA,
                                       int accumulate, void* ws, size_t ws_bytes, void* stream) {
    CLIPX_CHECK(r > 0 && c > 0 && E > 0, "sigmoid_fused_fwd: empty problem");
    CLIPX_CHECK(is_fused_dim(E), "sigmoid_fused_fwd: embed dim %d unsupported (" LT_FUSED_DIMS_STR ")", E);
    CLIPX_CHECK(pos_off < 0 || r + pos_off <= c, "sigmoid_fused_fwd: positives out of range");
    const bool grad = dA != nullptr;
    CLIPX_CHECK(ws_bytes >= clipx_sigmoid_fused_ws_bytes(r, c, E, grad), "sigmoid_fused_fwd: workspace too small");
    const int split = sig_split(r, c, grad), nb = split * cdiv(r, LT_T);
    float* dA_part = (float*)ws;
    float* pl = dA_part + (grad ? (size_t)split * r * E : 0);
    float* pds = pl + nb;
    float* pdb = pds + nb;
    hipStream_t st = (hipStream_t)stream;
    sig_walk(r, c, E, A, B, scale_dev, bias_dev, pos_off, 0, inv_r, dA_part, pl, grad ? pds : nullptr, grad ? pdb : nullptr,
             grad, st);
    if (grad) lt_split_sum(split, (long)r * E, dA_part, scale_dev, nullptr, accumulate, dA, st);
    hipLaunchKernelGGL(sig_sum3_kernel, dim3(1), dim3(64), 0, st, nb, pl, grad ? pds : nullptr, grad ? pdb : nullptr, inv_r,
                       accumulate, out3);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t clipx_sigmoid_fused_bwd_ws_bytes(int r, int c, int E) {
    const size_t split = sig_split(c, r, true);
    return split * (size_t)c * E * sizeof(float);
}

extern "C" int clipx_sigmoid_fused_bwd(int r, int c, int E, const float* A, const float* B, const float* scale_dev,
                                       const float* bias_dev, int pos_off, float inv_r, const float* gout_dev, float* dB,
                                       int accumulate, void* ws, size_t ws_bytes, void* stream) {
    CLIPX_CHECK(r > 0 && c > 0 && E > 0, "sigmoid_fused_bwd: empty problem");
    CLIPX_CHECK(is_fused_dim(E), "sigmoid_fused_bwd: embed dim %d unsupported (" LT_FUSED_DIMS_STR ")", E);
    CLIPX_CHECK(pos_off < 0 || r + pos_off <= c, "sigmoid_fused_bwd: positives out of range");
    CLIPX_CHECK(ws_bytes >= clipx_sigmoid_fused_bwd_ws_bytes(r, c, E), "sigmoid_fused_bwd: workspace too small");
    const int split = sig_split(c, r, true);
    float* dB_part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    // rows of B own the walk: the positive of B row j is A row j - pos_off
    sig_walk(c, r, E, B, A, scale_dev, bias_dev, pos_off, 1, inv_r, dB_part, nullptr, nullptr, nullptr, true, st);
    lt_split_sum(split, (long)c * E, dB_part, scale_dev, gout_dev, accumulate, dB, st);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- materialised logits
// in place dot -> dz over rows [row0 ...) of a block's stripe; block partials of the loss, d(s), d(beta)
#define LS_DENSE_BLOCKS 1024
__global__ __launch_bounds__(256) void sig_dense_kernel(int rows, int cols, float* __restrict__ z, long ldz,
                                                        const float* __restrict__ scale_dev, const float* __restrict__ bias_dev,
                                                        int pos_off, float inv_r, float* __restrict__ part_loss,
                                                        float* __restrict__ part_ds, float* __restrict__ part_db) {
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float s = scale_dev[0], beta = bias_dev[0];
    float l_part = 0.f, ds_part = 0.f, db_part = 0.f;
    for (int i = blockIdx.x; i < rows; i += gridDim.x)
        for (int j = tid; j < cols; j += 256) {
            const float dot = z[(long)i * ldz + j];
            const float dz = sig_term(fmaf(s, dot, beta), pos_off >= 0 && j == i + pos_off, inv_r, l_part);
            ds_part = fmaf(dz, dot, ds_part);
            db_part += dz;
            z[(long)i * ldz + j] = dz;
        }
    float v = lt_block_sum(l_part, red, wave, lane);
    if (tid == 0) part_loss[blockIdx.x] = v;
    v = lt_block_sum(ds_part, red, wave, lane);
    if (tid == 0) part_ds[blockIdx.x] = v;
    v = lt_block_sum(db_part, red, wave, lane);
    if (tid == 0) part_db[blockIdx.x] = v;
}

static int sig_dense_blocks(int rows) { return rows < LS_DENSE_BLOCKS ? rows : LS_DENSE_BLOCKS; }

extern "C" size_t clipx_sigmoid_dense_ws_bytes(int rows, int cols) {
    (void)cols;
    return 3 * (size_t)sig_dense_blocks(rows) * sizeof(float);
}

extern "C" int clipx_sigmoid_dense(int rows, int cols, float* z, long ldz, const float* scale_dev, const float* bias_dev,
                                   int pos_off, float inv_r, float* out3, void* ws, size_t ws_bytes, void* stream) {
    CLIPX_CHECK(rows > 0 && cols > 0 && ldz >= cols, "sigmoid_dense: bad shape");
    CLIPX_CHECK(pos_off < 0 || rows + pos_off <= cols, "sigmoid_dense: positives out of range");
    CLIPX_CHECK(ws_bytes >= clipx_sigmoid_dense_ws_bytes(rows, cols), "sigmoid_dense: workspace too small");
    const int nb = sig_dense_blocks(rows);
    float* pl = (float*)ws;
    float* pds = pl + nb;
    float* pdb = pds + nb;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sig_dense_kernel, dim3(nb), dim3(256), 0, st, rows, cols, z, ldz, scale_dev, bias_dev, pos_off, inv_r, pl,
                       pds, pdb);
    hipLaunchKernelGGL(sig_sum3_kernel, dim3(1), dim3(64), 0, st, nb, pl, pds, pdb, inv_r, 0, out3);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
