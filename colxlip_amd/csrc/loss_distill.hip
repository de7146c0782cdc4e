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
// The tile engine is loss_tile.h.
#include "loss_tile.h"

// ---------------------------------------------------------------------------------------------- forward
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
    __shared__ float Ps[LT_BK][LT_LD];
    __shared__ float Qs[LT_BK][LT_LD];
    __shared__ float Zs[LT_T][LT_T + 1];
    __shared__ float Ts[LT_T][LT_T + 1];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.y * LT_T, q0 = blockIdx.x * LT_T;
    lt_tile_to_lds(Ps, Qs, Zs, P, Q, p0, np, q0, nq, Es, tid);        // student tile
    lt_tile_to_lds(Ps, Qs, Ts, TP, TQ, p0, np, q0, nq, Et, tid);      // teacher tile (the staging buffers are free again)
    __syncthreads();
    float ms, ls, mt, lt, cc;
    if (tid < LT_T) {                       // one thread per tile row
        const int p = p0 + tid;
        if (p < np) {
            const int nvalid = min(LT_T, nq - q0);
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
    } else if (symmetric && tid < 2 * LT_T) {   // one thread per tile column
        const int j = tid - LT_T, q = q0 + j;
        if (q < nq) {
            const int nvalid = min(LT_T, np - p0);
            ld_partials(&Zs[0][j], &Ts[0][j], nvalid, LT_T + 1, ms, ls, mt, lt, cc);
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
    const float vc = lt_block_sum(ce, red, wave, lane);
    const float vd = lt_block_sum(di, red, wave, lane);
    if (tid == 0) {
        loss_part[2 * blockIdx.x] = weight * vc;
        loss_part[2 * blockIdx.x + 1] = weight * vd;
    }
}

static size_t distill_fwd_floats(int np, int nq, int symmetric) {
    const size_t tq = cdiv(nq, LT_T), tp = cdiv(np, LT_T);
    size_t f = 5 * tq * (size_t)np + (size_t)max(np, nq);
    if (symmetric) f += 5 * tp * (size_t)nq;
    f += 2 * ((size_t)cdiv(np, 256) + (symmetric ? (size_t)cdiv(nq, 256) : 0));
    return f;
}

extern "C" size_t clipx_distill_fused_ws_bytes(int np, int nq, int symmetric) {
    return distill_fwd_floats(np, nq, symmetric) * sizeof(float);
}

extern "C" int clipx_distill_fused_fwd(int np, int nq, int Es, int Et, const float* P, const float* Q, const float* TP,
                                       const float* TQ, int label_off, int symmetric, float w_own, float w_oth,
                                       float* stats_own, float* stats_oth, float* loss2, void* ws, size_t ws_bytes,
                                       void* stream) {
    CLIPX_CHECK(np > 0 && nq > 0 && Es > 0 && Et > 0, "distill_fused_fwd: empty problem");
    CLIPX_CHECK(is_fused_dim(Es) && is_fused_dim(Et), "distill_fused_fwd: embed dims %d / %d unsupported (" LT_FUSED_DIMS_STR ")",
                Es, Et);
    CLIPX_CHECK(label_off >= 0 && np + label_off <= nq, "distill_fused_fwd: labels out of range");
    CLIPX_CHECK(!symmetric || (np == nq && label_off == 0), "distill_fused_fwd: the symmetric form needs a square problem");
    CLIPX_CHECK(!symmetric || stats_oth, "distill_fused_fwd: the symmetric form needs the column statistics");
    CLIPX_CHECK(ws_bytes >= clipx_distill_fused_ws_bytes(np, nq, symmetric), "distill_fused_fwd: workspace too small");
    const int tq = cdiv(nq, LT_T), tp = cdiv(np, LT_T);
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
    hipLaunchKernelGGL(lt_sum_parts_kernel, dim3(2), dim3(1), 0, st, cdiv(np, 256) + (symmetric ? cdiv(nq, 256) : 0), 2,
                       loss_part, nullptr, loss2);
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
    __shared__ float Ps[LT_BK][LT_LD];
    __shared__ float Qs[LT_BK][LT_LD];
    __shared__ float dZs[LT_T][LT_T + 2];
    __shared__ float Qe[LT_T][lt_ec(NE) + 16];
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int p0 = blockIdx.x * LT_T;
    int jt0, jt1;
    lt_split_range(nq, jt0, jt1);
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
        const int q0 = jt * LT_T;
        // ---- teacher tile first: its share of ds, -w * g_d * pi, goes straight to LDS so that only one 16 x 64 tile is live
        // in registers next to the accumulators
        f32x4 z[4];
        lt_slab(z, Ps, Qs, TP, TQ, p0, np, q0, nq, Et, tid, wave, g, c);
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
        lt_slab(z, Ps, Qs, P, Q, p0, np, q0, nq, E, tid, wave, g, c);
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
        lt_product<NE>(acc, dZs, Qe, Q, q0, nq, tid, wave, g, c);
    }
    lt_store_part<NE>(dP_part, acc, prow, np, 1.f, c);
    if (ds_part_out) {
        const float v = lt_block_sum(ds_part, red, wave, lane);
        if (tid == 0) ds_part_out[blockIdx.y * gridDim.x + blockIdx.x] = v;
    }
}

extern "C" size_t clipx_distill_fused_bwd_ws_bytes(int np, int nq, int Es) {
    const size_t split = lt_split(np, nq, 768);
    return (split * (size_t)np * Es + split * (size_t)cdiv(np, LT_T)) * sizeof(float);
}

extern "C" int clipx_distill_fused_bwd(int np, int nq, int Es, int Et, const float* P, const float* Q, const float* TP,
                                       const float* TQ, const float* stats_own, float w_own, int off_own,
                                       const float* stats_oth, float w_oth, int off_oth, const float* gc_dev,
                                       const float* gd_dev, const float* out_scale_dev, float* dP, float* dscale_acc,
                                       const float* scale_dev, void* ws, size_t ws_bytes, void* stream) {
    CLIPX_CHECK(np > 0 && nq > 0 && Et > 0, "distill_fused_bwd: empty problem");
    CLIPX_CHECK(is_fused_dim(Et), "distill_fused_bwd: teacher embed dim %d unsupported", Et);
    CLIPX_CHECK(ws_bytes >= clipx_distill_fused_bwd_ws_bytes(np, nq, Es), "distill_fused_bwd: workspace too small");
    CLIPX_CHECK(stats_own || stats_oth, "distill_fused_bwd: no loss term");
    CLIPX_CHECK(gc_dev && gd_dev, "distill_fused_bwd: the two upstream gradients are required");
    CLIPX_CHECK(!stats_own || (off_own >= 0 && np + off_own <= nq), "distill_fused_bwd: own labels out of range");
    CLIPX_CHECK(!stats_oth || (off_oth >= 0 && nq + off_oth <= np), "distill_fused_bwd: other labels out of range");
    CLIPX_CHECK(!dscale_acc || scale_dev, "distill_fused_bwd: d(scale) needs the scale");
    const int tp = cdiv(np, LT_T), split = lt_split(np, nq, 768);
    const long n = (long)np * Es;
    float* dP_part = (float*)ws;
    float* ds_part = dP_part + (size_t)split * n;
    hipStream_t st = (hipStream_t)stream;
    const int known = fused_dim_dispatch(Es, [&](auto ne) {
        hipLaunchKernelGGL(distill_bwd_kernel<decltype(ne)::value>, dim3(tp, split), dim3(256), 0, st, np, nq, Et, P, Q, TP, TQ,
                           stats_own, w_own, off_own, stats_oth, w_oth, off_oth, gc_dev, gd_dev, dP_part,
                           dscale_acc ? ds_part : nullptr);
    });
    CLIPX_CHECK(known == 0, "distill_fused_bwd: embed dim %d unsupported (" LT_FUSED_DIMS_STR ")", Es);
    // the split partials are scaled after the split sum; d(scale) is divided by the scale once, after the block sum
    lt_split_sum(split, n, dP_part, out_scale_dev, nullptr, 0, dP, st);
    if (dscale_acc) hipLaunchKernelGGL(lt_sum_parts_kernel, dim3(1), dim3(1), 0, st, tp * split, 1, ds_part, scale_dev, dscale_acc);
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
    ls = lt_block_sum(ls, red, wave, lane);
    lt = lt_block_sum(lt, red, wave, lane);
    cc = lt_block_sum(cc, red, wave, lane);
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
    const float vc = lt_block_sum(ce, red, wave, lane);
    const float vd = lt_block_sum(di, red, wave, lane);
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
    const float vs = lt_block_sum(ps, red, wave, lane);
    const float vt = lt_block_sum(pt, red, wave, lane);
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
    hipLaunchKernelGGL(lt_sum_parts_kernel, dim3(2), dim3(1), 0, st, nparts, 2, part, nullptr, loss2);
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
