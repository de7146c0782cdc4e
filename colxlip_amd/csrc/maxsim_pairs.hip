// Gathered MaxSim for late-interaction reranking (colxlip_amd/search.py: LateInteractionIndex.rerank): the scores of an irregular
// set of (query, gallery item) pairs, straight from the index's storage.
//
//     out[i, c] = scale * (alpha * Gp[i, c] + (1 - alpha) * MaxSim(image tokens, text tokens)),   p = cand[i, c] the gallery position
//
// MaxSim as clipx_maxsim_score_fold forms it (reference loss.py:20-46): per text row the maximum over the image's q tokens, then
// sum_r w_r max_r / (sum_r w_r [max_r != 0] + 1e-8) over the text's first cnt rows with w = 1 and w = n - cnt + 1 for row cnt - 1, the
// representative of the bitwise-equal tail (clipx_maxsim_pack_text).  The denominator is n unless a maximum is exactly 0.
//
// Work split.  A workgroup of eight waves owns one query and a run of its candidate slots.  The query's rows (an image's q tokens;
// a text's first cnt rows) are staged once in LDS, zero-padded to whole 16-row tiles, at most MSP_QT tiles.  Each wave then takes
// one candidate at a time and streams its rows ONCE from global memory, 16 rows x 256 elements (a unit) per step with the next
// unit's loads in flight, as operand fragments of v_mfma_f32_16x16x32_bf16: the image rows are always the A operand (rows of the
// result) and the text rows the B operand (columns), so a text row's similarities sit in one column = the registers of the four
// lanes {l, l + 16, l + 32, l + 48}: the maximum over image rows is a register maximum and two cross-lane steps, and no similarity
// ever leaves the accumulators.
//   * text gallery (query = image in LDS, candidate = text streamed): acc[t] = S[query image tile t, candidate text tile]; after a
//     candidate tile's k-loop the column maxima are weighted and summed per lane.
//   * image gallery (query = text in LDS, candidate = image streamed): acc[t] = S[candidate image tile, query text tile t]; the
//     column maxima run over the candidate's tiles in registers (rmax) and are weighted once per candidate.
// Image rows >= q are masked to -inf BEFORE the maximum (a zero padding row would win against negative similarities); text rows
// >= cnt get weight 0 by selection, never by multiplication.
//
// Every global read is guarded twice.  clipx_maxsim_pairs first runs maxsim_pairs_check_kernel, which only reads cand / cnt, and
// refuses the call (nothing is scored, `out` is not touched) when a position lies outside [0, n_items) other than -1 or a cnt
// outside 1 .. n.  The scoring kernel itself still never follows such a value: a bad position writes NaN and reads no token, a bad
// cnt is clamped into 1 .. n.
#include "common.h"
#include <math.h>

#define MSP_QT 5                          // query row tiles held in the accumulators: at most 80 staged query rows
#define MSP_WAVES 8
#define MSP_KU 8                          // fragments (32 elements) of a unit: 256 elements of 16 candidate rows in flight per wave
#define MSP_PAD 8                         // bf16 elements between staged rows: 16-byte reads of 16 rows spread over the banks
#define MSP_LDS_BYTES (128 * 1024)        // staging limit (of the 160 KiB of a CU)

struct MspArgs {
    int nq, C, q, n, e, spw;              // spw: candidate slots per workgroup
    const unsigned short* query;          // [nq, q or n, e] bf16
    const int* query_cnt;                 // image gallery: cnt [nq] of the query texts
    const void* const* gal_tok;           // device table: chunk -> [chunk_items, q or n, e] bf16
    const int* const* gal_cnt;            // text gallery, device table: chunk -> cnt [chunk_items]
    int chunk_items;
    long n_items;
    const int* cand;                      // [nq, C]
    const float* Gp;                      // [nq, C] with row stride ld_gp, or null
    long ld_gp;
    float* out;                           // [nq, C] with row stride ld_out
    long ld_out;
    float alpha, beta, scale;
};

// weight of text row r of a text with `cnt` packed rows out of n
__device__ __forceinline__ float msp_row_weight(int r, int cnt, int n) {
    return r < cnt - 1 ? 1.0f : (r == cnt - 1 ? (float)(n - cnt + 1) : 0.0f);
}

template <bool GALLERY_IS_IMAGE>
__global__ __launch_bounds__(64 * MSP_WAVES) void maxsim_pairs_kernel(const MspArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lg = lane >> 4;
    const long i = blockIdx.x;
    const int e = a.e;
    const int qrows_mem = GALLERY_IS_IMAGE ? a.n : a.q;                          // rows of a query item in memory
    int qrows = qrows_mem;
    if (GALLERY_IS_IMAGE) qrows = min(max(a.query_cnt[i], 1), a.n);             // (the entry refused a cnt outside 1 .. n)
    const int qtiles = (qrows + 15) >> 4;                                        // <= MSP_QT: the entry's shape rule
    const int ldq = e + MSP_PAD;

    {   // the query's rows -> LDS, zero rows behind them
        const unsigned short* src = a.query + i * qrows_mem * e;
        const int per_row = e >> 3;
        for (int x = threadIdx.x; x < qtiles * 16 * per_row; x += 64 * MSP_WAVES) {
            const int r = x / per_row, c = x - r * per_row;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (r < qrows) v = *reinterpret_cast<const uint4*>(src + (long)r * e + c * 8);
            *reinterpret_cast<uint4*>(smem + ((long)r * ldq + c * 8) * 2) = v;
        }
    }
    __syncthreads();

    const int crows_mem = GALLERY_IS_IMAGE ? a.q : a.n;
    const int ksteps = (e + 32 * MSP_KU - 1) / (32 * MSP_KU);
    const int s0 = blockIdx.y * a.spw, s1 = min(a.C, s0 + a.spw);
    for (int s = s0 + wave; s < s1; s += MSP_WAVES) {                            // wave-uniform: no barrier below
        const int p = __builtin_amdgcn_readfirstlane(a.cand[i * a.C + s]);
        float* dst = a.out + i * a.ld_out + s;
        if (p < 0 || (long)p >= a.n_items) {                                     // -1: an empty slot.  Anything else was refused.
            if (lane == 0) *dst = (p == -1) ? -INFINITY : NAN;
            continue;
        }
        const int ch = p / a.chunk_items, off = p - ch * a.chunk_items;
        int crows = crows_mem;
        if (!GALLERY_IS_IMAGE) crows = min(max(__builtin_amdgcn_readfirstlane(a.gal_cnt[ch][off]), 1), a.n);
        const unsigned short* base = reinterpret_cast<const unsigned short*>(a.gal_tok[ch]) + (long)off * crows_mem * e;
        const int ctiles = (crows + 15) >> 4, units = ctiles * ksteps;

        bf16x8 cur[MSP_KU], nxt[MSP_KU];
        auto load_unit = [&](int u, bf16x8(&f)[MSP_KU]) {
            const int ct = u / ksteps, k0 = (u - ct * ksteps) * (32 * MSP_KU);
            const int row = ct * 16 + lr;
            const unsigned short* src = base + (long)row * e + k0 + lg * 8;
#pragma unroll
            for (int x = 0; x < MSP_KU; ++x) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (row < crows && k0 + x * 32 < e) v = *reinterpret_cast<const uint4*>(src + x * 32);
                f[x] = __builtin_bit_cast(bf16x8, v);
            }
        };

        f32x4 acc[MSP_QT];
        float rmax[MSP_QT];
#pragma unroll
        for (int t = 0; t < MSP_QT; ++t) rmax[t] = -INFINITY;
        float wsum = 0.f, wcnt = 0.f;                                            // this lane's text rows: sum w max, sum w [max != 0]
        load_unit(0, nxt);
        for (int u = 0; u < units; ++u) {
#pragma unroll
            for (int x = 0; x < MSP_KU; ++x) cur[x] = nxt[x];
            if (u + 1 < units) load_unit(u + 1, nxt);
            const int ct = u / ksteps, ks = u - ct * ksteps, k0 = ks * (32 * MSP_KU);
            if (ks == 0) {
#pragma unroll
                for (int t = 0; t < MSP_QT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int x = 0; x < MSP_KU; ++x) {
                if (k0 + x * 32 < e) {
#pragma unroll
                    for (int t = 0; t < MSP_QT; ++t) {
                        if (t < qtiles) {
                            const bf16x8 qf = *reinterpret_cast<const bf16x8*>(smem + ((long)(t * 16 + lr) * ldq + k0 + x * 32 + lg * 8) * 2);
                            if (GALLERY_IS_IMAGE) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur[x], qf, acc[t], 0, 0, 0);
                            else acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, cur[x], acc[t], 0, 0, 0);
                        }
                    }
                }
            }
            if (ks != ksteps - 1) continue;
            // the candidate tile is complete: acc[t][j] = S[image row (lg * 4 + j of its tile), text row (lr of its tile)]
            if (GALLERY_IS_IMAGE) {
#pragma unroll
                for (int t = 0; t < MSP_QT; ++t) {
                    if (t < qtiles) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float v = (ct * 16 + lg * 4 + j < a.q) ? acc[t][j] : -INFINITY;
                            rmax[t] = fmaxf(rmax[t], v);
                        }
                    }
                }
            } else {
                float m = -INFINITY;
#pragma unroll
                for (int t = 0; t < MSP_QT; ++t) {
                    if (t < qtiles) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float v = (t * 16 + lg * 4 + j < a.q) ? acc[t][j] : -INFINITY;
                            m = fmaxf(m, v);
                        }
                    }
                }
                m = fmaxf(m, __shfl_xor(m, 16, 64));
                m = fmaxf(m, __shfl_xor(m, 32, 64));
                const float w = msp_row_weight(ct * 16 + lr, crows, a.n);
                if (w > 0.f) {
                    wsum += w * m;
                    wcnt += (m != 0.f) ? w : 0.f;
                }
            }
        }
        if (GALLERY_IS_IMAGE) {
#pragma unroll
            for (int t = 0; t < MSP_QT; ++t) {
                if (t < qtiles) {
                    float m = rmax[t];
                    m = fmaxf(m, __shfl_xor(m, 16, 64));
                    m = fmaxf(m, __shfl_xor(m, 32, 64));
                    const float w = msp_row_weight(t * 16 + lr, qrows, a.n);
                    if (w > 0.f) {
                        wsum += w * m;
                        wcnt += (m != 0.f) ? w : 0.f;
                    }
                }
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {                                        // over the 16 text rows of the lanes' tiles
            wsum += __shfl_xor(wsum, o, 64);
            wcnt += __shfl_xor(wcnt, o, 64);
        }
        if (lane == 0) {
            const float tok = wsum / (wcnt + 1e-8f);
            // every product and the sum rounded on its own, as clipx_maxsim_score_fold does
            float r = __fmul_rn(a.beta, tok);
            if (a.Gp) r = __fadd_rn(__fmul_rn(a.alpha, a.Gp[i * a.ld_gp + s]), r);
            *dst = __fmul_rn(a.scale, r);
        }
    }
}

// status |= 1: a position outside [0, n_items) other than -1; |= 2: a candidate text's cnt outside 1 .. n; |= 4: a query text's.
// Reads cand, and cnt only at positions that passed.
__global__ __launch_bounds__(256) void maxsim_pairs_check_kernel(long slots, int nq, int n, const int* __restrict__ cand,
                                                                 const int* __restrict__ query_cnt, const int* const* __restrict__ gal_cnt,
                                                                 int chunk_items, long n_items, int* __restrict__ status) {
    int bad = 0;
    for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < slots; x += (long)gridDim.x * 256) {
        const int p = cand[x];
        if (p == -1) continue;
        if (p < 0 || (long)p >= n_items) { bad |= 1; continue; }
        if (gal_cnt) {
            const int c = gal_cnt[p / chunk_items][p % chunk_items];
            if (c < 1 || c > n) bad |= 2;
        }
    }
    if (query_cnt)
        for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < nq; x += (long)gridDim.x * 256)
            if (query_cnt[x] < 1 || query_cnt[x] > n) bad |= 4;
    if (bad) atomicOr(status, bad);
}

template <bool GALLERY_IS_IMAGE>
static void maxsim_pairs_launch(const MspArgs& a, size_t lds, hipStream_t stream) {
    static bool raised = false;
    if (!raised) {
        (void)hipFuncSetAttribute((const void*)maxsim_pairs_kernel<GALLERY_IS_IMAGE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  MSP_LDS_BYTES);
        raised = true;
    }
    hipLaunchKernelGGL(maxsim_pairs_kernel<GALLERY_IS_IMAGE>, dim3(a.nq, cdiv(a.C, a.spw)), dim3(64 * MSP_WAVES), lds, stream, a);
}

extern "C" int clipx_maxsim_pairs(int gallery_is_image, int nq, int C, int q, int n, int e, const void* query, const int* query_cnt,
                                  const void* gal_tok, const void* gal_cnt, int n_chunks, int chunk_items, long n_items,
                                  const int* cand, long cand_stride, const float* Gp, long ld_gp, float* out, long ld_out, float alpha,
                                  float beta, float scale, int* status, void* stream) {
    CLIPX_CHECK(nq >= 0 && C >= 0, "maxsim_pairs: negative shape (%d queries x %d candidates)", nq, C);
    CLIPX_CHECK(q >= 16 && n >= 1 && e >= 128 && e % 64 == 0, "maxsim_pairs: needs q >= 16, e %% 64 == 0 and e >= 128 (q=%d n=%d e=%d)", q, n, e);
    const int stage_rows = ((gallery_is_image ? n : q) + 15) / 16 * 16;
    const size_t lds = (size_t)stage_rows * (e + MSP_PAD) * 2;
    CLIPX_CHECK(stage_rows <= 16 * MSP_QT && lds <= MSP_LDS_BYTES,
                "maxsim_pairs: the query side (%d rows of %d) exceeds the staging of %d rows / %d bytes", gallery_is_image ? n : q, e,
                16 * MSP_QT, MSP_LDS_BYTES);
    CLIPX_CHECK(C <= 65535 * MSP_WAVES, "maxsim_pairs: at most %d candidates per query (got %d)", 65535 * MSP_WAVES, C);
    CLIPX_CHECK(nq <= 1 || cand_stride == C, "maxsim_pairs: cand must be contiguous, row stride %d (got %ld)", C, cand_stride);
    CLIPX_CHECK(ld_out >= C && (!Gp || ld_gp >= C), "maxsim_pairs: row strides of out / Gp below C = %d (%ld, %ld)", C, ld_out, ld_gp);
    CLIPX_CHECK(chunk_items >= 1 && n_chunks >= 0 && n_items >= 0 && n_items <= 2147483647L && n_items <= (long)n_chunks * chunk_items,
                "maxsim_pairs: %ld items do not fit %d chunks of %d", n_items, n_chunks, chunk_items);
    if (nq == 0 || C == 0) return 0;
    CLIPX_CHECK(query && cand && out && status && (n_items == 0 || gal_tok), "maxsim_pairs: null pointer");
    CLIPX_CHECK(((uintptr_t)query & 15) == 0, "maxsim_pairs: query tokens must be 16-byte aligned");
    CLIPX_CHECK(gallery_is_image ? query_cnt != nullptr : (n_items == 0 || gal_cnt != nullptr),
                "maxsim_pairs: the text side comes with its cnt (%s)", gallery_is_image ? "query_cnt" : "gal_cnt");
    hipStream_t st = (hipStream_t)stream;

    // refuse what the scoring kernel would have to skip: one read-only pass over cand and the cnt it names
    const long slots = (long)nq * C;
    int bad = 0;
    CLIPX_CHECK(hipMemsetAsync(status, 0, sizeof(int), st) == hipSuccess, "maxsim_pairs: status reset failed");
    hipLaunchKernelGGL(maxsim_pairs_check_kernel, dim3(min(cdiv(slots > nq ? slots : nq, 256), 2048)), dim3(256), 0, st, slots, nq, n, cand,
                       gallery_is_image ? query_cnt : (const int*)nullptr,
                       gallery_is_image ? (const int* const*)nullptr : (const int* const*)gal_cnt, chunk_items, n_items, status);
    CLIPX_LAUNCH_CHECK();
    CLIPX_CHECK(hipMemcpyAsync(&bad, status, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess,
                "maxsim_pairs: status read-back failed");
    CLIPX_CHECK(!(bad & 1), "maxsim_pairs: a candidate position lies outside [0, %ld) and is not -1", n_items);
    CLIPX_CHECK(!(bad & 6), "maxsim_pairs: a %s text's cnt lies outside 1 .. %d", (bad & 4) ? "query" : "gallery", n);

    MspArgs a;
    a.nq = nq; a.C = C; a.q = q; a.n = n; a.e = e;
    // slots per workgroup: all of a query's candidates (the staged query is reused most), halved while the grid is short of
    // four workgroups per CU, never below one candidate per wave
    int spw = (C + MSP_WAVES - 1) / MSP_WAVES * MSP_WAVES;
    const long want = 4L * clipx_num_cu(false);
    while (spw > MSP_WAVES && (long)nq * cdiv(C, spw) < want) spw = (spw / 2 + MSP_WAVES - 1) / MSP_WAVES * MSP_WAVES;
    a.spw = spw;
    a.query = (const unsigned short*)query; a.query_cnt = query_cnt;
    a.gal_tok = (const void* const*)gal_tok; a.gal_cnt = (const int* const*)gal_cnt;
    a.chunk_items = chunk_items; a.n_items = n_items;
    a.cand = cand; a.Gp = Gp; a.ld_gp = ld_gp; a.out = out; a.ld_out = ld_out;
    a.alpha = alpha; a.beta = beta; a.scale = scale;
    if (gallery_is_image) maxsim_pairs_launch<true>(a, lds, st);
    else maxsim_pairs_launch<false>(a, lds, st);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
