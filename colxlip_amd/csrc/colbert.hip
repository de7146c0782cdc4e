// Token-level (ColBERT / MaxSim) similarity pieces of ColClipLoss (reference loss.py:20-46): the similarity tensor
// sim[m,k,n,q] is produced one text chunk at a time by the GEMM kernels as S[(m,n), (k,q)]; these kernels reduce it
// (max over an image's q tokens with the arg-max, mean over the text tokens with the reference's non-zero count) and
// build the sparse d(S) for the backward GEMMs.  HBM-bound streaming kernels.
#include "kernels.h"

// maxv[row, g] = max_qq S[row, g*q + qq] (first maximum on ties, like torch.max on the reference's CPU path).
// A sub-wave of LPG lanes (power of two, 4 elements per lane per pass) owns one (row, group): its q contiguous elements are
// read coalesced, reduced in registers and then across the sub-wave with (value, index) shuffles.  (The first version,
// one thread per (row, group) walking q strided elements, was 70 % of ColClipLoss's time.)
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(256) void maxsim_reduce_kernel(long rows, int groups, int q, int lpg, const T* __restrict__ S,
                                                            float* __restrict__ maxv, unsigned char* __restrict__ arg) {
    const int lane = threadIdx.x & 63;
    const int sub = lane / lpg, sl = lane % lpg;            // sub-wave index inside the wave, lane inside the sub-wave
    const int per_wave = 64 / lpg;
    const long total = rows * groups;
    const long wave_global = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long wave_stride = (long)gridDim.x * 4;
    for (long base = wave_global * per_wave; base < total; base += wave_stride * per_wave) {
        const long item = base + sub;
        const bool live = item < total;
        const long it = live ? item : total - 1;
        const T* p = S + (it / groups) * (long)groups * q + (it % groups) * (long)q;
        float best = -INFINITY;
        int bi = 0;
        for (int e0 = 4 * sl; e0 < q; e0 += 4 * lpg) {
            float v[4];
            if (ALIGNED && e0 + 4 <= q) {
                const float4 t = load4(p + e0);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = (e0 + k < q) ? (float)p[e0 + k] : -INFINITY;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v[k] > best) { best = v[k]; bi = e0 + k; }
        }
        for (int o = lpg >> 1; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (live && sl == 0) {
            maxv[item] = best;
            arg[item] = (unsigned char)bi;
        }
    }
}

// out[m, g] = sum_n maxv[(m*n_tok + n), g] / (#{n: maxv != 0} + 1e-8);  inv_count[m, g] = 1 / (that denominator)
__global__ __launch_bounds__(256) void masked_mean_kernel(int ct, int n_tok, int groups, const float* __restrict__ maxv,
                                                          float* __restrict__ out, float* __restrict__ inv_count) {
    const long total = (long)ct * groups;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / groups;
        const int g = (int)(i % groups);
        float s = 0.f, c = 0.f;
        for (int n = 0; n < n_tok; ++n) {
            const float v = maxv[(m * n_tok + n) * groups + g];
            s += v;
            c += (v != 0.f) ? 1.f : 0.f;
        }
        const float inv = 1.0f / (c + 1e-8f);
        out[i] = s * inv;
        inv_count[i] = inv;
    }
}

// d(S): P[(m,n), (g,qq)] = (qq == arg[(m,n), g]) ? dlogits[m,g] * inv_count[m,g] : 0, and optionally its transpose
// PT[(g,qq), (m,n)] (the reduction-major operand of the wgrad-style GEMM).  The sum in the reference's numerator runs over
// ALL text tokens, so every (m,n,g) passes a gradient to its arg-max, zeroed tokens included.
template <typename T>
__global__ __launch_bounds__(256) void maxsim_scatter_kernel(int ct, int n_tok, int groups, int q,
                                                             const float* __restrict__ dlogits,
                                                             const float* __restrict__ inv_count,
                                                             const unsigned char* __restrict__ arg, T* __restrict__ P,
                                                             T* __restrict__ PT) {
    // one block per (m,n) row; a thread writes 4 consecutive columns (32-bit index math only)
    const int row = blockIdx.x;
    const int m = row / n_tok;
    const int cols = groups * q;
    const long rows = (long)ct * n_tok;
    const float* dl = dlogits + (long)m * groups;
    const float* ic = inv_count + (long)m * groups;
    const unsigned char* ar = arg + (long)row * groups;
    T* prow = P + (long)row * cols;
    for (int c0 = threadIdx.x * 4; c0 < cols; c0 += 1024) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = c0 + k;
            float x = 0.f;
            if (col < cols) {
                const int g = col / q, qq = col - g * q;
                if ((int)ar[g] == qq) x = dl[g] * ic[g];
            }
            v[k] = x;
        }
        if (c0 + 4 <= cols && (cols & 3) == 0) {
            store4(prow + c0, make_float4(v[0], v[1], v[2], v[3]));
        } else {
            for (int k = 0; k < 4 && c0 + k < cols; ++k) prow[c0 + k] = (T)v[k];
        }
        if (PT) {
            for (int k = 0; k < 4 && c0 + k < cols; ++k) PT[(long)(c0 + k) * rows + row] = (T)v[k];
        }
    }
}

static int grid_for(long total) {
    long g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    if (g < 1) g = 1;
    return (int)g;
}

extern "C" int clipx_maxsim_reduce(int dtype, long rows, int groups, int q, const void* S, float* maxv,
                                   unsigned char* arg, void* stream) {
    CLIPX_CHECK(q >= 1 && q <= 255, "maxsim_reduce: 1 <= q <= 255 (got %d)", q);
    if (rows <= 0 || groups <= 0) return 0;
    int lpg = 4;
    while (lpg < 64 && 4 * lpg < q) lpg <<= 1;          // lanes per (row, group): one pass when q <= 256
    const int per_wave = 64 / lpg;
    long waves = (rows * groups + per_wave - 1) / per_wave;
    long grid = (waves + 3) / 4;
    if (grid > 65536) grid = 65536;
    const bool aligned = (q % 4 == 0) && ((uintptr_t)S % 16 == 0);   // every group then starts on an 8 / 16-byte boundary
#define MAXSIM_LAUNCH(TT, AL)                                                                                       \
    hipLaunchKernelGGL((maxsim_reduce_kernel<TT, AL>), dim3((int)grid), dim3(256), 0, (hipStream_t)stream, rows, groups, q, \
                       lpg, (const TT*)S, maxv, arg)
    if (dtype == CLIPX_F32) {
        if (aligned) MAXSIM_LAUNCH(float, true); else MAXSIM_LAUNCH(float, false);
    } else {
        if (aligned) MAXSIM_LAUNCH(bf16_t, true); else MAXSIM_LAUNCH(bf16_t, false);
    }
#undef MAXSIM_LAUNCH
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_masked_mean(int ct, int n_tok, int groups, const float* maxv, float* out, float* inv_count,
                                 void* stream) {
    if (ct <= 0 || groups <= 0) return 0;
    hipLaunchKernelGGL(masked_mean_kernel, dim3(grid_for((long)ct * groups)), dim3(256), 0, (hipStream_t)stream, ct, n_tok,
                       groups, maxv, out, inv_count);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_maxsim_scatter(int dtype, int ct, int n_tok, int groups, int q, const float* dlogits,
                                    const float* inv_count, const unsigned char* arg, void* P, void* PT, void* stream) {
    if (ct <= 0 || groups <= 0) return 0;
    const int grid = ct * n_tok;
    if (dtype == CLIPX_F32)
        hipLaunchKernelGGL(maxsim_scatter_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ct, n_tok, groups, q,
                           dlogits, inv_count, arg, (float*)P, (float*)PT);
    else
        hipLaunchKernelGGL(maxsim_scatter_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ct, n_tok, groups,
                           q, dlogits, inv_count, arg, (bf16_t*)P, (bf16_t*)PT);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused MaxSim (round 4; bf16 tokens, q >= 16).  Three ideas, each exact:
//  (1) DUPLICATE TEXT ROWS ARE COMPUTED ONCE.  Every text position at or behind a caption's EOT leaves ColXLIP's token head as
//      the SAME vector (reference model.py:589-603 zeroes the token BEFORE the head), so the trailing rows of a sample that are
//      bitwise equal to its last row have the same similarities, the same maximum and the same arg-max: one representative row
//      carries their count as a weight.  Found from the data (no side channel from the model: the loss sees only the tensor).
//      On the synthetic captions (EOT ~ U[8, 76]) 56 % of the 77 rows remain; real captions are shorter.
//  (2) the similarity GEMM reduces to per-(row, image) maxima in its own epilogue (gemm_nt_maxsim.h): S is never written;
//  (3) what the backward needs -- arg-max and 1 / count -- is kept; d(S) is rebuilt on the packed rows.
//
// Packed row r of sample m: position pos[r]; weight w[r] = 1, or (n_tok - pos[r]) for the representative of the equal tail.

// cnt[m] = t + 1 where rows t .. n_tok-1 of sample m are bitwise equal (t = n_tok - 1 when the last two rows differ)
__global__ __launch_bounds__(256) void maxsim_tail_kernel(int n_tok, int e, const unsigned short* __restrict__ txt, int* __restrict__ cnt) {
    const int m = blockIdx.x;
    const unsigned short* base = txt + (long)m * n_tok * e;
    const unsigned short* last = base + (long)(n_tok - 1) * e;
    __shared__ int first_diff;           // largest row index that differs from the last row (-1: none)
    if (threadIdx.x == 0) first_diff = -1;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int n = n_tok - 2 - wave; n >= 0; n -= 4) {
        if (n < first_diff) break;       // (racy read: only an early exit)
        bool diff = false;
        for (int k = lane; k < e; k += 64) diff |= base[(long)n * e + k] != last[k];
        if (__any(diff)) { if (lane == 0) atomicMax(&first_diff, n); }
    }
    __syncthreads();
    if (threadIdx.x == 0) cnt[m] = first_diff + 2;      // rows 0 .. first_diff as they are + one representative of the tail
}

// cu[0..nt] = exclusive scan of cnt (one block; nt is a batch size)
__global__ __launch_bounds__(1024) void maxsim_scan_kernel(int nt, const int* __restrict__ cnt, int* __restrict__ cu) {
    __shared__ int part[1024];
    const int per = (nt + 1023) / 1024;
    const int lo = threadIdx.x * per, hi = min(nt, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; }
        cu[nt] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { cu[i] = run; run += cnt[i]; }
}

// packed[r,:] = txt[m, pos,:];  row_m[r], row_w[r].  One wave per packed row.
__global__ __launch_bounds__(256) void maxsim_pack_kernel(int nt, int n_tok, int e, const unsigned short* __restrict__ txt,
                                                          const int* __restrict__ cu, unsigned short* __restrict__ packed,
                                                          int* __restrict__ row_m, float* __restrict__ row_w) {
    const int m = blockIdx.x;
    const int r0 = cu[m], cntm = cu[m + 1] - r0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int p = wave; p < cntm; p += 4) {
        const unsigned short* src = txt + ((long)m * n_tok + p) * e;
        unsigned short* dst = packed + (long)(r0 + p) * e;
        for (int k = lane * 8; k < e; k += 512) *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + k);
        if (lane == 0) {
            row_m[r0 + p] = m;
            row_w[r0 + p] = (p == cntm - 1) ? (float)(n_tok - p) : 1.0f;
        }
    }
}

// The partial rows that hold image k, in column order (gemm_nt_maxsim.h): from 64 tokens per image up one row per 64-column slot
// the image touches, [2 * slot + seg] with seg = 1 when the slot begins inside an earlier image; below that one row per slot
// half, [2 * k + half].  part = 0 .. maxsim_parts(q, k) - 1.
__device__ __forceinline__ int maxsim_parts(int q, int k) { return ((((k + 1) * q - 1) >> 6) - ((k * q) >> 6)) + 1; }
__device__ __forceinline__ int maxsim_part_row(int q, int k, int part) {
    if (q < 64) return 2 * k + part;
    const int s = ((k * q) >> 6) + part;
    return 2 * s + (((s << 6) / q == k) ? 0 : 1);
}

// Fold the partials of image k for packed row r: maxvT[k, r], argT[k, r] (row-contiguous, like the partials)
__global__ __launch_bounds__(256) void maxsim_finish_kernel(int R, int ldp, int r0, int ld, int ni, int q, const float* __restrict__ pmax,
                                                            const unsigned short* __restrict__ pidx, float* __restrict__ maxvT,
                                                            unsigned short* __restrict__ argT) {
    const int r = blockIdx.x * 256 + threadIdx.x;        // row inside this chunk of packed rows (partials are per chunk)
    const int k = blockIdx.y;
    if (r >= R) return;
    const int parts = maxsim_parts(q, k);
    float best = -INFINITY;
    int bi = 0;
    for (int p = 0; p < parts; ++p) {
        const long o = (long)maxsim_part_row(q, k, p) * ldp + r;
        const float v = pmax[o];
        if (v > best) { best = v; bi = pidx[o]; }
    }
    maxvT[(long)k * ld + r0 + r] = best;
    argT[(long)k * ld + r0 + r] = (unsigned short)bi;
}

// logits[m, k] = sum_r w_r maxvT[k, r] / (sum_r w_r [maxvT != 0] + 1e-8) over the packed rows of sample m (reference loss.py:36-44:
// the non-zero count runs over ALL the sample's text positions, each tail position counted)
__global__ __launch_bounds__(256) void maxsim_mean_kernel(int nt, int ni, int ld, const int* __restrict__ cu, const float* __restrict__ row_w,
                                                          const float* __restrict__ maxvT, float* __restrict__ out,
                                                          float* __restrict__ inv_count) {
    const long total = (long)nt * ni;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int m = (int)(i / ni), k = (int)(i % ni);
        float s = 0.f, c = 0.f;
        for (int r = cu[m]; r < cu[m + 1]; ++r) {
            const float v = maxvT[(long)k * ld + r], w = row_w[r];
            s += w * v;
            c += (v != 0.f) ? w : 0.f;
        }
        const float inv = 1.0f / (c + 1e-8f);
        out[i] = s * inv;
        inv_count[i] = inv;
    }
}

// Forward-only scoring (retrieval, ColXLIP.get_logits under no_grad): slot partials -> final scores in one pass, with neither
// maxvT / argT nor inv_count in memory.  For text samples m < nm (packed rows cu[m] .. cu[m+1], chunk-local row = r - rbase) and
// images k < ni of the partial arrays' image chunk:
//     tok[m, k]    = sum_r w_r v_r / (sum_r w_r [v_r != 0] + 1e-8),  v_r = max over the partials of image k (as finish)
//     scores[k, m] = scale * (alpha * G[k, m] + beta * tok[m, k]),  beta = 1 - alpha   (image-major; G == nullptr: no global term)
// The partials are row-contiguous and a sample's rows are consecutive, so a wave owns one image and walks SPW consecutive
// samples with its lanes on consecutive rows (256-byte reads per segment; > 64 rows take another pass) and reduces (sum,
// count) across the wave; lane i keeps sample i's score, and the SPW scores leave as one 64-byte store.  pmax == nullptr is
// the global-only form (alpha = 1): scale * G bit for bit, the token term is skipped, not multiplied by 0.
#define MAXSIM_FOLD_SPW 16
__global__ __launch_bounds__(256) void maxsim_score_fold_kernel(int nm, int ni, int q, int ldp, int rbase, const int* __restrict__ cu,
                                                                const float* __restrict__ row_w, const float* __restrict__ pmax,
                                                                const float* __restrict__ G, long ld_g, float* __restrict__ scores,
                                                                long ld_scores, float alpha, float beta, float scale) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (k >= ni) return;
    const int mb = blockIdx.x * MAXSIM_FOLD_SPW;
    const int mcnt = min(MAXSIM_FOLD_SPW, nm - mb);
    float tok = 0.f;
    if (pmax) {
        const int parts = maxsim_parts(q, k);
        for (int i = 0; i < mcnt; ++i) {
            const int ra = cu[mb + i] - rbase, rb = cu[mb + i + 1] - rbase;
            float s = 0.f, c = 0.f;
            for (int r = ra + lane; r < rb; r += 64) {
                float best = -INFINITY;
                for (int p = 0; p < parts; ++p) {
                    const float v = pmax[(long)maxsim_part_row(q, k, p) * ldp + r];
                    best = v > best ? v : best;
                }
                const float w = row_w[rbase + r];
                s += w * best;
                c += (best != 0.f) ? w : 0.f;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                s += __shfl_xor(s, o, 64);
                c += __shfl_xor(c, o, 64);
            }
            if (lane == i) tok = s / (c + 1e-8f);
        }
    }
    if (lane < mcnt) {
        const int m = mb + lane;
        float out;
        // every product and the sum rounded on its own (no fma contraction): the same fp32 values as the expression written out
        if (!pmax) out = __fmul_rn(scale, G[(long)k * ld_g + m]);
        else if (G) out = __fmul_rn(scale, __fadd_rn(__fmul_rn(alpha, G[(long)k * ld_g + m]), __fmul_rn(beta, tok)));
        else out = __fmul_rn(scale, __fmul_rn(beta, tok));
        scores[(long)k * ld_scores + m] = out;
    }
}

// d(S) on the packed rows: P[r, k*q + qq] = (qq == argT[k, r]) ? dlogits[m_r, k] * inv_count[m_r, k] : 0   (bf16).
// One block per packed row; 8 columns (16 B) per thread and pass.
__global__ __launch_bounds__(256) void maxsim_scatter_packed_kernel(int r0, int ld, int ni, int q, const int* __restrict__ row_m,
                                                                    const float* __restrict__ dlogits, const float* __restrict__ inv_count,
                                                                    const unsigned short* __restrict__ argT, bf16_t* __restrict__ P) {
    const int r = r0 + blockIdx.x;                       // P holds the rows of one chunk, row 0 = packed row r0
    const int m = row_m[r];
    const int cols = ni * q;
    const float* dl = dlogits + (long)m * ni;
    const float* ic = inv_count + (long)m * ni;
    bf16_t* prow = P + (long)blockIdx.x * cols;
    for (int c0 = threadIdx.x * 8; c0 < cols; c0 += 2048) {
        union { bf16_t h[8]; uint4 v; } o;
        int k = c0 / q, qq = c0 - k * q;
        int a = argT[(long)k * ld + r];
        float coef = dl[k] * ic[k];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            o.h[t] = (bf16_t)((qq == a) ? coef : 0.f);
            if (++qq == q && t < 7) {
                qq = 0;
                ++k;
                if (k < ni) { a = argT[(long)k * ld + r]; coef = dl[k] * ic[k]; }
            }
        }
        *reinterpret_cast<uint4*>(prow + c0) = o.v;
    }
}

// text rows scaled by their weights (the dImg GEMM sums over ALL original rows: a representative counts w times), and the
// expansion of the packed text gradient back to [nt, n_tok, e]: every tail position receives its representative's gradient
__global__ __launch_bounds__(256) void maxsim_scale_rows_kernel(long total, int e, const float* __restrict__ row_w,
                                                                const bf16_t* __restrict__ x, bf16_t* __restrict__ y) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256)
        y[i] = (bf16_t)((float)x[i] * row_w[i / e]);
}
template <typename T>
__global__ __launch_bounds__(256) void maxsim_expand_kernel(int n_tok, int e, const int* __restrict__ cu, const float* __restrict__ dpacked,
                                                            T* __restrict__ dtxt) {
    const int m = blockIdx.x;
    const int r0 = cu[m], cntm = cu[m + 1] - r0;
    for (int i = threadIdx.x; i < n_tok * e; i += 256) {
        const int n = i / e, k = i - n * e;
        const int p = n < cntm ? n : cntm - 1;
        dtxt[((long)m * n_tok + n) * e + k] = (T)dpacked[(long)(r0 + p) * e + k];
    }
}

extern "C" int clipx_maxsim_pack_text(int nt, int n_tok, int e, const void* txt, int* cnt, int* cu, void* stream) {
    CLIPX_CHECK(nt >= 1 && n_tok >= 1 && e % 8 == 0, "maxsim_pack_text: embed dim must be a multiple of 8 (got %d)", e);
    hipLaunchKernelGGL(maxsim_tail_kernel, dim3(nt), dim3(256), 0, (hipStream_t)stream, n_tok, e, (const unsigned short*)txt, cnt);
    hipLaunchKernelGGL(maxsim_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, nt, cnt, cu);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_maxsim_pack_rows(int nt, int n_tok, int e, const void* txt, const int* cu, void* packed, int* row_m,
                                      float* row_w, void* stream) {
    hipLaunchKernelGGL(maxsim_pack_kernel, dim3(nt), dim3(256), 0, (hipStream_t)stream, nt, n_tok, e, (const unsigned short*)txt, cu,
                       (unsigned short*)packed, row_m, row_w);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// partial maxima of S = packed . img^T: per (row, 64-column slot, segment) from 64 tokens per image up, pmax / pidx
// [2 * ceil(ni*q / 64), ld]; per (row, image, slot half) for 16 <= q < 64, [2 * ni, ld]
extern "C" int clipx_maxsim_gemm(int R, int ni, int q, int e, const void* packed, const void* img, float* pmax,
                                 unsigned short* pidx, int ld, void* stream) {
    CLIPX_CHECK(q >= 16 && q <= 65535 && e % 64 == 0 && e >= 128 && ld >= R, "maxsim_gemm: needs q >= 16, embed dim %% 64 == 0 (q=%d e=%d)", q, e);
    if (R <= 0 || ni <= 0) return 0;
    EpiB16 epi = {};
    epi.ms_max = pmax;
    epi.ms_idx = pidx;
    epi.ms_q = q;
    epi.ms_ld = ld;
    const int rc = launch_gemm_bf16_nt8p_maxsim(R, ni * q, e, (const bf16_t*)packed, (const bf16_t*)img, epi, (hipStream_t)stream);
    CLIPX_CHECK(rc == 0, "maxsim_gemm: the ping-pong NT kernel does not take this shape (R=%d ni*q=%d e=%d)", R, ni * q, e);
    return 0;
}

// the same partials from e4m3 operands on the fp8 MFMA (gemm_fp8_nt8p.hip): packed8 [R, e] / img8 [ni * q, e] bytes with one
// power-of-two exponent per row (clipx_quant_rows_e4m3).  A shape the kernel does not take is an error: the caller chooses the
// route before it calls.
extern "C" int clipx_maxsim_gemm_fp8(int R, int ni, int q, int e, const void* packed8, const int* packed_exp, const void* img8,
                                     const int* img_exp, float* pmax, unsigned short* pidx, int ld, void* stream) {
    CLIPX_CHECK(q >= 16 && q <= 65535 && e % 128 == 0 && e >= 256 && ld >= R,
                "maxsim_gemm_fp8: needs q >= 16, embed dim %% 128 == 0 and >= 256 (q=%d e=%d)", q, e);
    if (R <= 0 || ni <= 0) return 0;
    CLIPX_CHECK(packed8 && packed_exp && img8 && img_exp && pmax && pidx, "maxsim_gemm_fp8: null operand");
    EpiB16 epi = {};
    epi.ms_max = pmax;
    epi.ms_idx = pidx;
    epi.ms_q = q;
    epi.ms_ld = ld;
    const int rc = launch_gemm_fp8_nt8p_maxsim(R, ni * q, e, (const unsigned char*)packed8, packed_exp, (const unsigned char*)img8,
                                               img_exp, epi, (hipStream_t)stream);
    CLIPX_CHECK(rc == 0, "maxsim_gemm_fp8: the fp8 ping-pong NT kernel does not take this shape or alignment (R=%d ni*q=%d e=%d)", R,
                ni * q, e);
    return 0;
}

extern "C" int clipx_maxsim_finish(int R, int ldp, int r0, int ld, int ni, int q, const float* pmax, const unsigned short* pidx,
                                   float* maxvT, unsigned short* argT, void* stream) {
    if (R <= 0 || ni <= 0) return 0;
    hipLaunchKernelGGL(maxsim_finish_kernel, dim3(cdiv(R, 256), ni), dim3(256), 0, (hipStream_t)stream, R, ldp, r0, ld, ni, q, pmax,
                       pidx, maxvT, argT);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_maxsim_score_fold(int nm, int ni, int q, int ldp, int rbase, const int* cu, const float* row_w, const float* pmax,
                                       const float* G, long ld_g, float* scores, long ld_scores, float alpha, float beta, float scale,
                                       void* stream) {
    CLIPX_CHECK(pmax || G, "maxsim_score_fold: the global-only form (no partials) needs G");
    CLIPX_CHECK(!pmax || (q >= 16 && ldp >= 1 && cu && row_w), "maxsim_score_fold: partials need q >= 16, cu and row_w (q=%d)", q);
    CLIPX_CHECK(ni <= 4 * 65535, "maxsim_score_fold: at most 262140 images per call (got %d)", ni);
    if (nm <= 0 || ni <= 0) return 0;
    hipLaunchKernelGGL(maxsim_score_fold_kernel, dim3(cdiv(nm, MAXSIM_FOLD_SPW), cdiv(ni, 4)), dim3(256), 0, (hipStream_t)stream, nm, ni,
                       q, ldp, rbase, cu, row_w, pmax, G, ld_g, scores, ld_scores, alpha, beta, scale);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_maxsim_mean(int nt, int ni, int ld, const int* cu, const float* row_w, const float* maxvT, float* logits,
                                 float* inv_count, void* stream) {
    if (nt <= 0 || ni <= 0) return 0;
    hipLaunchKernelGGL(maxsim_mean_kernel, dim3(grid_for((long)nt * ni)), dim3(256), 0, (hipStream_t)stream, nt, ni, ld, cu, row_w,
                       maxvT, logits, inv_count);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_maxsim_scatter_packed(int R, int r0, int ld, int ni, int q, const int* row_m, const float* dlogits,
                                           const float* inv_count, const unsigned short* argT, void* P, void* stream) {
    CLIPX_CHECK((ni * (long)q) % 8 == 0, "maxsim_scatter_packed: ni * q must be a multiple of 8");
    if (R <= 0) return 0;
    hipLaunchKernelGGL(maxsim_scatter_packed_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, r0, ld, ni, q, row_m, dlogits,
                       inv_count, argT, (bf16_t*)P);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_maxsim_scale_rows(int R, int e, const float* row_w, const void* x, void* y, void* stream) {
    if (R <= 0) return 0;
    hipLaunchKernelGGL(maxsim_scale_rows_kernel, dim3(grid_for((long)R * e)), dim3(256), 0, (hipStream_t)stream, (long)R * e, e, row_w,
                       (const bf16_t*)x, (bf16_t*)y);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

extern "C" int clipx_maxsim_expand(int dtype, int nt, int n_tok, int e, const int* cu, const float* dpacked, void* dtxt, void* stream) {
    if (dtype == CLIPX_F32)
        hipLaunchKernelGGL(maxsim_expand_kernel<float>, dim3(nt), dim3(256), 0, (hipStream_t)stream, n_tok, e, cu, dpacked, (float*)dtxt);
    else
        hipLaunchKernelGGL(maxsim_expand_kernel<bf16_t>, dim3(nt), dim3(256), 0, (hipStream_t)stream, n_tok, e, cu, dpacked, (bf16_t*)dtxt);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Retrieval ranks (reference train.py:457-508 sorts every row on the CPU with argsort and searches the ground truth):
// rank of a target column = number of columns scoring strictly higher; a row with several targets (captions of one
// image) takes the best of them.  One wave per row, targets in CSR form.
__global__ __launch_bounds__(256) void retrieval_rank_kernel(int rows, int cols, const float* __restrict__ scores, long ld,
                                                             const int* __restrict__ tgt_off, const int* __restrict__ tgt_idx,
                                                             int* __restrict__ ranks) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float* s = scores + (long)row * ld;
    int best = cols;
    for (int t = tgt_off[row]; t < tgt_off[row + 1]; ++t) {
        const float ref = s[tgt_idx[t]];
        int cnt = 0;
        for (int c = lane; c < cols; c += 64) cnt += (s[c] > ref) ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        best = cnt < best ? cnt : best;
    }
    if (lane == 0) ranks[row] = best;
}

extern "C" int clipx_retrieval_rank(int rows, int cols, const float* scores, long ld, const int* tgt_off,
                                    const int* tgt_idx, int* ranks, void* stream) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(retrieval_rank_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, rows, cols, scores, ld,
                       tgt_off, tgt_idx, ranks);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
