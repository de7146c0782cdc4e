// Fused contrastive + distillation cross-entropy (DistillClipLoss, reference loss.py:343-379) that never holds a logits matrix.
//
//   s[p,q] = P[p] . Q[q]     (student: P = logit_scale * own features [np, Es], Q = the other side's [nq, Es], fp32)
//   t[p,q] = TP[p] . TQ[q]   (teacher: TP = dist_logit_scale * own teacher features [np, Et], TQ [nq, Et])
//   per row p:  lse_s = logsumexp_q s,  pi = softmax_q t,  X = sum_q pi * s
//               CE_p = lse_s - s[p, p+off]           (the contrastive term, loss.py:364-367)
//               D_p  = lse_s - X                     (-(softmax(t) * log_softmax(s)).sum(), loss.py:345)
//   contrastive += w_own * sum_p CE_p,  distill += w_own * sum_p D_p   [+ the same over columns when symmetric]
//   d(loss)/ds[p,q] = w * (g_c * (sigma - delta) + g_d * (sigma - pi)),  sigma = softmax_q s   (+ the column term)
//
// Everything is exact fp32 (v_mfma_f32_16x16x4_f32 == an fmaf chain) on 64x64 tiles, as in loss_fused.hip:
//   forward   one pass over the tiles: each tile computes the student tile (depth Es) and the teacher tile (depth Et) through
//             the same staging buffers, keeps per-tile partials for every row (and column): (m_s, l_s) of the student's
//             log-sum-exp and (m_t, l_t, c = sum exp(t - m_t) * s) of the teacher; a merge kernel rescales and combines
//             them into lse_s, lse_t, X and both losses.  Scratch: 5 x (N/64) x N floats per direction.
//   backward  one walk per student operand: a block owns 64 rows of that operand, walks the other side's 64-row tiles,
//             recomputes both tiles, forms ds and accumulates ds . Q_tile into 64 x Es registers (as ce_fused_bwd).
//             d(logit_scale) = sum ds * s / scale rides along.  The walk is split over gridDim.y blocks; the split and block
//             partials are summed in a fixed order (no atomics: the same result every run).
// FLOPs at Es = Et: 2 (forward) + 2 x 3 (two backward walks: two recomputes + the product) = 8 logits-GEMM equivalents.
// Gradients of the teacher (rarely wanted: the teacher runs without a graph) and embed dims outside ops.FUSED_CE_DIMS take
// the materialised path at the end of this file (logits from gemm_f32, the statistics and ds / dt from the kernels here).
#include "kernels.h"

#define LD_T 64              // tile edge
#define LD_BK 64             // k-depth of one staged chunk
#define LD_LD (LD_T + 16)    // LDS row stride of the k-major operand images

// stage rows [r0, r0+64) x columns [k0, k0+64) of a row-major [n, E] matrix into the k-major LDS image S[k][row]
// (rows >= n and columns >= E read as zero)
__device__ __forceinline__ void ld_stage(float (&S)[LD_BK][LD_LD], const float* __restrict__ src, int r0, int n, int E, int k0,
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

// block partials -> 4 waves -> one float (fixed order)
__device__ __forceinline__ float ld_block_sum(float v, float* red, int wave, int lane) {
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------- forward
// 64x64 tile of X @ Y^T (depth E) into the LDS matrix Z (256 threads; 2x2 waves of 32x32)
__device__ __forceinline__ void ld_tile_to_lds(float (&Xs)[LD_BK][LD_LD], float (&Ys)[LD_BK][LD_LD], float (&Z)[LD_T][LD_T + 1],
                                               const float* __restrict__ X, const float* __restrict__ Y, int p0, int np, int q0,
                                               int nq, int E, int tid) {
    const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += LD_BK) {
        ld_stage(Xs, X, p0, np, E, k0, tid);
        ld_stage(Ys, Y, q0, nq, E, k0, tid);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < LD_BK / 4; ++ks) {
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

// the five partials of one row (or column) of a tile, n valid entries at stride `st` of the two LDS matrices
__device__ __forceinline__ void ld_partials(const float* zs, const float* zt, int n, int st, float& ms, float& ls, float& mt,
                                            float& lt, float& cc) {
    ms = -INFINITY;
    mt = -INFINITY;
    for (int j = 0; j < n; ++j) {
        ms = fmaxf(ms, zs[j * st]);
        mt = fmaxf(mt, zt[j * st]);
    }
    ls = 0.f;
    lt = 0.f;
    cc = 0.f;
    for (int j = 0; j < n; ++j) {
        const float s = zs[j * st];
        const float e = expf(zt[j * st] - mt);
        ls += expf(s - ms);
        lt += e;
        cc = fmaf(e, s, cc);
    }
}

// part layout of one direction: 5 arrays [ntiles][n]: m_s, l_s, m_t, l_t, c
__global__ __launch_bounds__(256) void distill_fwd_kernel(int np, int nq, int Es, int Et, const float* __restrict__ P,
                                                          const float* __restrict__ Q, const float* __restrict__ TP,
                                                          const float* __restrict__ TQ, int label_off, int symmetric,
                                                          float* __restrict__ row_part, float* __restrict__ col_part,
                                                          float* __restrict__ zdiag) {
    __shared__ float Ps[LD_BK][LD_LD];
    __shared__ float Qs[LD_BK][LD_LD];
    __shared__ float Zs[LD_T][LD_T + 1];
    __shared__ float Ts[LD_T][LD_T + 1];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.y * LD_T, q0 = blockIdx.x * LD_T;
    ld_tile_to_lds(Ps, Qs, Zs, P, Q, p0, np, q0, nq, Es, tid);        // student tile
    ld_tile_to_lds(Ps, Qs, Ts, TP, TQ, p0, np, q0, nq, Et, tid);      // teacher tile (the staging buffers are free again)
    __syncthreads();
    float ms, ls, mt, lt, cc;
    if (tid < LD_T) {                       // one thread per tile row
        const int p = p0 + tid;
        if (p < np) {
            const int nvalid = min(LD_T, nq - q0);
            ld_partials(&Zs[tid][0], &Ts[tid][0], nvalid, 1, ms, ls, mt, lt, cc);
            const long n = np, o = (long)blockIdx.x * np + p, stride = (long)gridDim.x * n;
            row_part[o] = ms;
            row_part[o + stride] = ls;
            row_part[o + 2 * stride] = mt;
            row_part[o + 3 * stride] = lt;
            row_part[o + 4 * stride] = cc;
            const int lab = p + label_off - q0;
            if (lab >= 0 && lab < nvalid) zdiag[p] = Zs[tid][lab];
        }
    } else if (symmetric && tid < 2 * LD_T) {   // one thread per tile column
        const int j = tid - LD_T, q = q0 + j;
        if (q < nq) {
            const int nvalid = min(LD_T, np - p0);
            ld_partials(&Zs[0][j], &Ts[0][j], nvalid, LD_T + 1, ms, ls, mt, lt, cc);
            const long o = (long)blockIdx.y * nq + q, stride = (long)gridDim.y * nq;
            col_part[o] = ms;
            col_part[o + stride] = ls;
            col_part[o + 2 * stride] = mt;
            col_part[o + 3 * stride] = lt;
            col_part[o + 4 * stride] = cc;
        }
    }
}

// merge the per-tile partials of one direction into stats[3][n] = (lse_s, lse_t, X) and the block's two loss partials
__global__ __launch_bounds__(256) void distill_merge_kernel(int n, int ntiles, const float* __restrict__ part,
                                                            const float* __restrict__ zdiag, float weight,
                                                            float* __restrict__ stats, float* __restrict__ loss_part) {
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = blockIdx.x * 256 + tid;
    float ce = 0.f, di = 0.f;
    if (i < n) {
        const long stride = (long)ntiles * n;
        const float* pms = part;
        const float* pls = part + stride;
        const float* pmt = part + 2 * stride;
        const float* plt = part + 3 * stride;
        const float* pcc = part + 4 * stride;
        float Ms = -INFINITY, Mt = -INFINITY;
        for (int t = 0; t < ntiles; ++t) {
            Ms = fmaxf(Ms, pms[(long)t * n + i]);
            Mt = fmaxf(Mt, pmt[(long)t * n + i]);
        }
        float Ls = 0.f, Lt = 0.f, C = 0.f;
        for (int t = 0; t < ntiles; ++t) {
            const long k = (long)t * n + i;
            Ls += pls[k] * expf(pms[k] - Ms);
            const float r = expf(pmt[k] - Mt);
            Lt += plt[k] * r;
            C += pcc[k] * r;
        }
        const float lse_s = Ms + logf(Ls);
        const float X = C / Lt;
        stats[i] = lse_s;
        stats[n + i] = Mt + logf(Lt);
        stats[2 * n + i] = X;
        ce = lse_s - zdiag[i];
        di = lse_s - X;
    }
    const float vc = ld_block_sum(ce, red, wave, lane);
    const float vd = ld_block_sum(di, red, wave, lane);
    if (tid == 0) {
        loss_part[2 * blockIdx.x] = weight * vc;
        loss_part[2 * blockIdx.x + 1] = weight * vd;
    }
}

// out2[k] += sum_i part[2*i + k] (k = 0, 1), each summed in index order by its own thread
__global__ void distill_sum2_kernel(int n, const float* __restrict__ part, float* __restrict__ out2) {
    const int k = threadIdx.x;
    if (k >= 2) return;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += part[2 * i + k];
    out2[k] += s;
}

static size_t distill_fwd_floats(int np, int nq, int symmetric) {
    const size_t tq = cdiv(nq, LD_T), tp = cdiv(np, LD_T);
    size_t f = 5 * tq * (size_t)np + (size_t)max(np, nq);
    if (symmetric) f += 5 * tp * (size_t)nq;
    f += 2 * ((size_t)cdiv(np, 256) + (symmetric ? (size_t)cdiv(nq, 256) : 0));
    return f;
}

static bool distill_dim_ok(int E) {
    return E == 16 || E == 32 || E == 64 || E == 128 || E == 256 || E == 512 || E == 640 || E == 768 || E == 1024;
}

extern "C" size_t clipx_distill_fused_ws_bytes(int np, int nq, int symmetric) {
    return distill_fwd_floats(np, nq, symmetric) * sizeof(float);
}

extern "C" int clipx_distill_fused_fwd(int np, int nq, int Es, int Et, const float* P, const float* Q, const float* TP,
                                       const float* TQ, int label_off, int symmetric, float w_own, float w_oth,
                                       float* stats_own, float* stats_oth, float* loss2, void* ws, size_t ws_bytes,
                                       void* stream) {
    CLIPX_CHECK(np > 0 && nq > 0 && Es > 0 && Et > 0, "distill_fused_fwd: empty problem");
    CLIPX_CHECK(distill_dim_ok(Es) && distill_dim_ok(Et),
                "distill_fused_fwd: embed dims %d / %d unsupported (16, 32, 64, 128, 256, 512, 640, 768, 1024)", Es, Et);
    CLIPX_CHECK(label_off >= 0 && np + label_off <= nq, "distill_fused_fwd: labels out of range");
    CLIPX_CHECK(!symmetric || (np == nq && label_off == 0), "distill_fused_fwd: the symmetric form needs a square problem");
    CLIPX_CHECK(!symmetric || stats_oth, "distill_fused_fwd: the symmetric form needs the column statistics");
    CLIPX_CHECK(ws_bytes >= clipx_distill_fused_ws_bytes(np, nq, symmetric), "distill_fused_fwd: workspace too small");
    const int tq = cdiv(nq, LD_T), tp = cdiv(np, LD_T);
    float* row_part = (float*)ws;
    float* zdiag = row_part + 5 * (size_t)tq * np;
    float* col_part = zdiag + max(np, nq);
    float* loss_part = symmetric ? col_part + 5 * (size_t)tp * nq : col_part;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(distill_fwd_kernel, dim3(tq, tp), dim3(256), 0, st, np, nq, Es, Et, P, Q, TP, TQ, label_off, symmetric,
                       row_part, symmetric ? col_part : nullptr, zdiag);
    hipLaunchKernelGGL(distill_merge_kernel, dim3(cdiv(np, 256)), dim3(256), 0, st, np, tq, row_part, zdiag, w_own, stats_own,
                       loss_part);
    if (symmetric)
        hipLaunchKernelGGL(distill_merge_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, st, nq, tp, col_part, zdiag, w_oth,
                           stats_oth, loss_part + 2 * cdiv(np, 256));
    hipLaunchKernelGGL(distill_sum2_kernel, dim3(1), dim3(64), 0, st, cdiv(np, 256) + (symmetric ? cdiv(nq, 256) : 0),
                       loss_part, loss2);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- backward
// dP_part[split][p, :] = sum_q ds(p,q) * Q[q, :] over this block's share of the q tiles,
//   ds(p,q) = w_own * (g_c * (sigma_own - [q == p+off_own]) + g_d * (sigma_own - pi_own))       (own row statistics)
//           + w_oth * (g_c * (sigma_oth - [p == q+off_oth]) + g_d * (sigma_oth - pi_oth))       (the other side's)
// sigma = exp(s - lse_s), pi = exp(t - lse_t); a NULL statistics pointer drops its term.  NE = Es / 16 accumulator tiles.
template <int NE>
__global__ __launch_bounds__(256, (NE <= 32 ? 2 : 1)) void distill_bwd_kernel(
        int np, int nq, int Et, const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ TP,
        const float* __restrict__ TQ, const float* __restrict__ st_own, float w_own, int off_own,
        const float* __restrict__ st_oth, float w_oth, int off_oth, const float* __restrict__ gc_dev,
        const float* __restrict__ gd_dev, float* __restrict__ dP_part, float* __restrict__ ds_part_out) {
    constexpr int E = 16 * NE;
    constexpr int EC = (NE >= 4) ? 64 : 16 * NE;     // columns of Q staged per chunk of the product
    constexpr int TC = EC / 16;                      // accumulator tiles per chunk
    __shared__ float Ps[LD_BK][LD_LD];
    __shared__ float Qs[LD_BK][LD_LD];
    __shared__ float dZs[LD_T][LD_T + 2];      // stride 66: the A-operand read (row = lane & 15, k = lane >> 4) is conflict-free
    __shared__ float Qe[LD_T][EC + 16];        // stride == 16 (mod 32), as the k-major operand images
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int p0 = blockIdx.x * LD_T;
    const int ntq = (nq + LD_T - 1) / LD_T;
    const int per = (ntq + gridDim.y - 1) / gridDim.y;
    const int jt0 = blockIdx.y * per, jt1 = min(ntq, jt0 + per);
    const float gc = gc_dev[0], gd = gd_dev[0];

    f32x4 acc[NE];
#pragma unroll
    for (int t = 0; t < NE; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // this lane's four rows (C/D map): own index p and its student / teacher log-sum-exps
    float ls_own[4], lt_own[4];
    int prow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        prow[r] = p0 + 16 * wave + 4 * g + r;
        const bool ok = st_own && prow[r] < np;
        ls_own[r] = ok ? st_own[prow[r]] : 0.f;
        lt_own[r] = ok ? st_own[np + prow[r]] : 0.f;
    }
    float ds_part = 0.f;

    for (int jt = jt0; jt < jt1; ++jt) {
        const int q0 = jt * LD_T;
        // ---- teacher tile first (wave w owns rows 16w..16w+15 against the tile's four 16-column groups): its share of ds,
        // -w * g_d * pi, goes straight to LDS so that only one 16 x 64 tile is live in registers next to the accumulators
        f32x4 z[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) z[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Et; k0 += LD_BK) {
            ld_stage(Ps, TP, p0, np, Et, k0, tid);
            ld_stage(Qs, TQ, q0, nq, Et, k0, tid);
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < LD_BK / 4; ++ks) {
                const float a = Ps[ks * 4 + g][16 * wave + c];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    z[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Qs[ks * 4 + g][16 * t + c], z[t], 0, 0, 0);
            }
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = q0 + 16 * t + c;
            const float lt_q = (st_oth && q < nq) ? st_oth[nq + q] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float d = 0.f;                                    // padding rows / columns are zeroed below
                if (st_own) d -= w_own * gd * expf(z[t][r] - lt_own[r]);
                if (st_oth) d -= w_oth * gd * expf(z[t][r] - lt_q);
                dZs[16 * wave + 4 * g + r][16 * t + c] = d;      // read back below by the thread that wrote it
            }
        }
        // ---- student tile, then the rest of ds for this wave's 16 x 64 slice (read back as the A operand of the product)
#pragma unroll
        for (int t = 0; t < 4; ++t) z[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < E; k0 += LD_BK) {
            ld_stage(Ps, P, p0, np, E, k0, tid);
            ld_stage(Qs, Q, q0, nq, E, k0, tid);
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < LD_BK / 4; ++ks) {
                const float a = Ps[ks * 4 + g][16 * wave + c];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    z[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Qs[ks * 4 + g][16 * t + c], z[t], 0, 0, 0);
            }
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = q0 + 16 * t + c;
            const float ls_q = (st_oth && q < nq) ? st_oth[q] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = prow[r];
                const float v = z[t][r];         // padding rows / columns: v = 0 and the statistics read as 0 (all finite)
                float d = dZs[16 * wave + 4 * g + r][16 * t + c];
                if (st_own) d += w_own * ((gc + gd) * expf(v - ls_own[r]) - (q == p + off_own ? gc : 0.f));
                if (st_oth) d += w_oth * ((gc + gd) * expf(v - ls_q) - (p == q + off_oth ? gc : 0.f));
                d = (p < np && q < nq) ? d : 0.f;
                ds_part = fmaf(d, v, ds_part);
                dZs[16 * wave + 4 * g + r][16 * t + c] = d;
            }
        }
        // ---- product: acc[16 rows x E] += dZ[16 x 64] . Q_tile[64 x E], Q staged EC columns at a time
#pragma unroll
        for (int ec = 0; ec < NE / TC; ++ec) {
            __syncthreads();                            // Qe free (previous chunk consumed); dZs rows of this wave written
            for (int i = tid; i < LD_T * (EC / 4); i += 256) {
                const int row = i / (EC / 4), c4 = (i % (EC / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q0 + row < nq) v = load4(Q + (long)(q0 + row) * E + ec * EC + c4);
                Qe[row][c4] = v.x; Qe[row][c4 + 1] = v.y; Qe[row][c4 + 2] = v.z; Qe[row][c4 + 3] = v.w;
            }
            __syncthreads();
#pragma unroll
            for (int kc = 0; kc < LD_T / 4; ++kc) {
                const float a = dZs[16 * wave + c][4 * kc + g];
#pragma unroll
                for (int t = 0; t < TC; ++t)
                    acc[ec * TC + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Qe[4 * kc + g][16 * t + c], acc[ec * TC + t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < NE; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = prow[r];
            if (p < np) dP_part[((long)blockIdx.y * np + p) * E + 16 * t + c] = acc[t][r];
        }
    if (ds_part_out) {
        const float v = ld_block_sum(ds_part, red, wave, lane);
        if (tid == 0) ds_part_out[blockIdx.y * gridDim.x + blockIdx.x] = v;
    }
}

// out[j] = (osc) * sum_k part[k*n + j], k in order; osc = *scale_dev if given, else 1
__global__ __launch_bounds__(256) void distill_split_sum_kernel(int nsplit, long n, const float* __restrict__ part,
                                                                const float* __restrict__ scale_dev, float* __restrict__ out) {
    const float osc = scale_dev ? scale_dev[0] : 1.f;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        float s = 0.f;
        for (int k = 0; k < nsplit; ++k) s += part[k * n + j];
        out[j] = osc * s;
    }
}

// *acc += (sum_i part[i] in index order) / *div_dev
__global__ void distill_sum_div_kernel(int n, const float* __restrict__ part, const float* __restrict__ div_dev,
                                       float* __restrict__ acc) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += part[i];
    *acc += s / div_dev[0];
}

// blocks over the q tiles of one row tile: ~3 blocks per CU in flight
static int distill_bwd_split(int np, int nq) {
    const int tp = cdiv(np, LD_T), tq = cdiv(nq, LD_T);
    int split = cdiv(768, tp);
    if (split > tq) split = tq;
    if (split < 1) split = 1;
    return split;
}

extern "C" size_t clipx_distill_fused_bwd_ws_bytes(int np, int nq, int Es) {
    const size_t split = distill_bwd_split(np, nq);
    return (split * (size_t)np * Es + split * (size_t)cdiv(np, LD_T)) * sizeof(float);
}

template <int NE>
static void launch_distill_bwd(int np, int nq, int Et, const float* P, const float* Q, const float* TP, const float* TQ,
                               const float* st_own, float w_own, int off_own, const float* st_oth, float w_oth, int off_oth,
                               const float* gc_dev, const float* gd_dev, float* dP_part, float* ds_part, hipStream_t stream) {
    const dim3 grid(cdiv(np, LD_T), distill_bwd_split(np, nq));
    hipLaunchKernelGGL(distill_bwd_kernel<NE>, grid, dim3(256), 0, stream, np, nq, Et, P, Q, TP, TQ, st_own, w_own, off_own,
                       st_oth, w_oth, off_oth, gc_dev, gd_dev, dP_part, ds_part);
}

extern "C" int clipx_distill_fused_bwd(int np, int nq, int Es, int Et, const float* P, const float* Q, const float* TP,
                                       const float* TQ, const float* stats_own, float w_own, int off_own,
                                       const float* stats_oth, float w_oth, int off_oth, const float* gc_dev,
                                       const float* gd_dev, const float* out_scale_dev, float* dP, float* dscale_acc,
                                       const float* scale_dev, void* ws, size_t ws_bytes, void* stream) {
    CLIPX_CHECK(np > 0 && nq > 0 && Et > 0, "distill_fused_bwd: empty problem");
    CLIPX_CHECK(distill_dim_ok(Et), "distill_fused_bwd: teacher embed dim %d unsupported", Et);
    CLIPX_CHECK(ws_bytes >= clipx_distill_fused_bwd_ws_bytes(np, nq, Es), "distill_fused_bwd: workspace too small");
    CLIPX_CHECK(stats_own || stats_oth, "distill_fused_bwd: no loss term");
    CLIPX_CHECK(gc_dev && gd_dev, "distill_fused_bwd: the two upstream gradients are required");
    CLIPX_CHECK(!stats_own || (off_own >= 0 && np + off_own <= nq), "distill_fused_bwd: own labels out of range");
    CLIPX_CHECK(!stats_oth || (off_oth >= 0 && nq + off_oth <= np), "distill_fused_bwd: other labels out of range");
    CLIPX_CHECK(!dscale_acc || scale_dev, "distill_fused_bwd: d(scale) needs the scale");
    const int tp = cdiv(np, LD_T), split = distill_bwd_split(np, nq);
    const long n = (long)np * Es;
    float* dP_part = (float*)ws;
    float* ds_part = dP_part + (size_t)split * n;
    hipStream_t st = (hipStream_t)stream;
#define LD_CASE(ne)                                                                                                     \
    else if (Es == 16 * (ne)) launch_distill_bwd<ne>(np, nq, Et, P, Q, TP, TQ, stats_own, w_own, off_own, stats_oth,    \
                                                     w_oth, off_oth, gc_dev, gd_dev, dP_part, dscale_acc ? ds_part : nullptr, st);
    if (false) {
    }
    LD_CASE(1) LD_CASE(2) LD_CASE(4) LD_CASE(8) LD_CASE(16) LD_CASE(32) LD_CASE(40) LD_CASE(48) LD_CASE(64)
    else {
        clipx_set_error("distill_fused_bwd: embed dim %d unsupported (16, 32, 64, 128, 256, 512, 640, 768, 1024)", Es);
        return -1;
    }
#undef LD_CASE
    int grid = cdiv(n, 256);
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(distill_split_sum_kernel, dim3(grid), dim3(256), 0, st, split, n, dP_part, out_scale_dev, dP);
    if (dscale_acc)
        hipLaunchKernelGGL(distill_sum_div_kernel, dim3(1), dim3(1), 0, st, tp * split, ds_part, scale_dev, dscale_acc);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- materialised logits
// s [rows, cols] (ld lds) and t (ld ldt) in memory.  Row statistics: one block per row; stats[3][rows] = (lse_s, lse_t, X);
// part[2 * row] = w * CE_row, part[2 * row + 1] = w * D_row.
__device__ __forceinline__ float ld_block_max(float v, float* red, int wave, int lane) {
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void distill_dense_rows_kernel(int rows, int cols, const float* __restrict__ s, long lds,
                                                                 const float* __restrict__ t, long ldt, int label_off, float w,
                                                                 float* __restrict__ stats, float* __restrict__ part) {
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = blockIdx.x;
    const float* sr = s + (long)i * lds;
    const float* tr = t + (long)i * ldt;
    float ms = -INFINITY, mt = -INFINITY;
    for (int j = tid; j < cols; j += 256) {
        ms = fmaxf(ms, sr[j]);
        mt = fmaxf(mt, tr[j]);
    }
    ms = ld_block_max(ms, red, wave, lane);
    mt = ld_block_max(mt, red, wave, lane);
    float ls = 0.f, lt = 0.f, cc = 0.f;
    for (int j = tid; j < cols; j += 256) {
        const float e = expf(tr[j] - mt);
        ls += expf(sr[j] - ms);
        lt += e;
        cc = fmaf(e, sr[j], cc);
    }
    ls = ld_block_sum(ls, red, wave, lane);
    lt = ld_block_sum(lt, red, wave, lane);
    cc = ld_block_sum(cc, red, wave, lane);
    if (tid == 0) {
        const float lse_s = ms + logf(ls), X = cc / lt;
        stats[i] = lse_s;
        stats[rows + i] = mt + logf(lt);
        stats[2 * rows + i] = X;
        part[2 * i] = w * (lse_s - sr[i + label_off]);
        part[2 * i + 1] = w * (lse_s - X);
    }
}

// column statistics of a square matrix (labels on the diagonal): one thread per column; part per block as above
__global__ __launch_bounds__(256) void distill_dense_cols_kernel(int rows, int cols, const float* __restrict__ s, long lds,
                                                                 const float* __restrict__ t, long ldt, float w,
                                                                 float* __restrict__ stats, float* __restrict__ part) {
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = blockIdx.x * 256 + tid;
    float ce = 0.f, di = 0.f;
    if (j < cols) {
        float ms = -INFINITY, mt = -INFINITY;
        for (int i = 0; i < rows; ++i) {
            ms = fmaxf(ms, s[(long)i * lds + j]);
            mt = fmaxf(mt, t[(long)i * ldt + j]);
        }
        float ls = 0.f, lt = 0.f, cc = 0.f;
        for (int i = 0; i < rows; ++i) {
            const float sv = s[(long)i * lds + j];
            const float e = expf(t[(long)i * ldt + j] - mt);
            ls += expf(sv - ms);
            lt += e;
            cc = fmaf(e, sv, cc);
        }
        const float lse_s = ms + logf(ls), X = cc / lt;
        stats[j] = lse_s;
        stats[cols + j] = mt + logf(lt);
        stats[2 * cols + j] = X;
        ce = lse_s - s[(long)j * lds + j];
        di = lse_s - X;
    }
    const float vc = ld_block_sum(ce, red, wave, lane);
    const float vd = ld_block_sum(di, red, wave, lane);
    if (tid == 0) {
        part[2 * blockIdx.x] = w * vc;
        part[2 * blockIdx.x + 1] = w * vd;
    }
}

// in place s -> ds and (want_dt) t -> dt:
//   ds = sum over the present directions of w * (g_c * (sigma - delta) + g_d * (sigma - pi))
//   dt = -sum over the present directions of w * g_d * pi * (s - X)
// part[2*block] = sum ds * s, part[2*block + 1] = sum dt * t (block partials in a fixed order)
#define LD_DENSE_BLOCKS 1024
__global__ __launch_bounds__(256) void distill_dense_grad_kernel(int rows, int cols, float* __restrict__ s, long lds,
                                                                 float* __restrict__ t, long ldt, int label_off,
                                                                 const float* __restrict__ st_row, float w_row,
                                                                 const float* __restrict__ st_col, float w_col,
                                                                 const float* __restrict__ gc_dev, const float* __restrict__ gd_dev,
                                                                 int want_dt, float* __restrict__ part) {
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float gc = gc_dev[0], gd = gd_dev[0];
    float ps = 0.f, pt = 0.f;
    const long n = (long)rows * cols;
    for (long k = (long)blockIdx.x * 256 + tid; k < n; k += (long)gridDim.x * 256) {
        const int i = (int)(k / cols), j = (int)(k % cols);
        const float sv = s[(long)i * lds + j], tv = t[(long)i * ldt + j];
        float d = 0.f, dt = 0.f;
        if (st_row) {
            const float sg = expf(sv - st_row[i]), pi = expf(tv - st_row[rows + i]);
            d += w_row * (gc * (sg - (j == i + label_off ? 1.f : 0.f)) + gd * (sg - pi));
            dt -= w_row * gd * pi * (sv - st_row[2 * rows + i]);
        }
        if (st_col) {
            const float sg = expf(sv - st_col[j]), pi = expf(tv - st_col[cols + j]);
            d += w_col * (gc * (sg - (i == j ? 1.f : 0.f)) + gd * (sg - pi));
            dt -= w_col * gd * pi * (sv - st_col[2 * cols + j]);
        }
        ps = fmaf(d, sv, ps);
        pt = fmaf(dt, tv, pt);
        s[(long)i * lds + j] = d;
        if (want_dt) t[(long)i * ldt + j] = dt;
    }
    const float vs = ld_block_sum(ps, red, wave, lane);
    const float vt = ld_block_sum(pt, red, wave, lane);
    if (tid == 0) {
        part[2 * blockIdx.x] = vs;
        part[2 * blockIdx.x + 1] = vt;
    }
}

// out2 (+)= [sum part[2i] / *scale_dev, sum part[2i+1] / *tscale_dev], in index order
__global__ void distill_dense_scales_kernel(int n, const float* __restrict__ part, const float* __restrict__ scale_dev,
                                            const float* __restrict__ tscale_dev, float* __restrict__ out2) {
    const int k = threadIdx.x;
    const float* div = k == 0 ? scale_dev : tscale_dev;
    if (k >= 2 || !div) return;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += part[2 * i + k];
    out2[k] += s / div[0];
}

static int distill_dense_blocks(long n) {
    const int b = cdiv(n, 256);
    return b < LD_DENSE_BLOCKS ? b : LD_DENSE_BLOCKS;
}

extern "C" size_t clipx_distill_dense_ws_bytes(int rows, int cols) {
    const size_t a = 2 * (size_t)rows + 2 * (size_t)cdiv(cols, 256);
    const size_t b = 2 * (size_t)distill_dense_blocks((long)rows * cols);
    return (a > b ? a : b) * sizeof(float);
}

extern "C" int clipx_distill_dense_fwd(int rows, int cols, const float* s, long lds, const float* t, long ldt, int label_off,
                                       int symmetric, float w_row, float w_col, float* stats_row, float* stats_col,
                                       float* loss2, void* ws, size_t ws_bytes, void* stream) {
    CLIPX_CHECK(rows > 0 && cols > 0 && lds >= cols && ldt >= cols, "distill_dense_fwd: bad shape");
    CLIPX_CHECK(label_off >= 0 && rows + label_off <= cols, "distill_dense_fwd: labels out of range");
    CLIPX_CHECK(!symmetric || (rows == cols && label_off == 0 && stats_col), "distill_dense_fwd: bad symmetric problem");
    CLIPX_CHECK(ws_bytes >= clipx_distill_dense_ws_bytes(rows, cols), "distill_dense_fwd: workspace too small");
    float* part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(distill_dense_rows_kernel, dim3(rows), dim3(256), 0, st, rows, cols, s, lds, t, ldt, label_off, w_row,
                       stats_row, part);
    int nparts = rows;
    if (symmetric) {
        hipLaunchKernelGGL(distill_dense_cols_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, st, rows, cols, s, lds, t, ldt, w_col,
                           stats_col, part + 2 * rows);
        nparts += cdiv(cols, 256);
    }
    hipLaunchKernelGGL(distill_sum2_kernel, dim3(1), dim3(64), 0, st, nparts, part, loss2);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_distill_dense_grad(int rows, int cols, float* s, long lds, float* t, long ldt, int label_off,
                                        const float* stats_row, float w_row, const float* stats_col, float w_col,
                                        const float* gc_dev, const float* gd_dev, int want_dt, const float* scale_dev,
                                        const float* tscale_dev, float* dscales2, void* ws, size_t ws_bytes, void* stream) {
    CLIPX_CHECK(rows > 0 && cols > 0 && lds >= cols && ldt >= cols, "distill_dense_grad: bad shape");
    CLIPX_CHECK(stats_row || stats_col, "distill_dense_grad: no loss term");
    CLIPX_CHECK(!stats_row || (label_off >= 0 && rows + label_off <= cols), "distill_dense_grad: labels out of range");
    CLIPX_CHECK(!stats_col || rows == cols, "distill_dense_grad: column statistics need a square problem");
    CLIPX_CHECK(ws_bytes >= clipx_distill_dense_ws_bytes(rows, cols), "distill_dense_grad: workspace too small");
    const int nb = distill_dense_blocks((long)rows * cols);
    float* part = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(distill_dense_grad_kernel, dim3(nb), dim3(256), 0, st, rows, cols, s, lds, t, ldt, label_off, stats_row,
                       w_row, stats_col, w_col, gc_dev, gd_dev, want_dt, part);
    if (dscales2)
        hipLaunchKernelGGL(distill_dense_scales_kernel, dim3(1), dim3(64), 0, st, nb, part, scale_dev, tscale_dev, dscales2);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
