// Patch dropout (FLIP, arXiv 2212.00794; reference transformer.py:48-88, applied at :712 before ln_pre): while training, each
// image keeps `keep` of its G2 patch tokens and the image tower runs on 1 + keep rows per image.  Here the dropped patches are
// never embedded: the mask is drawn on the device, the patch-embed GEMM's input is gathered from the image (patchify_keep),
// the assemble adds the positional rows of the kept patches, and its backward scatters the token gradient back to the
// positional-embedding rows in a fixed order (no float atomics: the same bits every run).
#include "common.h"

#define PK_MAX_G2 1024
#define PK_THREADS 256
#define PK_PARTS 64            // batch parts of the positional-gradient partial sums (as clipx_vision_assemble_bwd)
#define PK_POS_TILE 16         // positions per block of the backward's partial-sum kernel

void launch_reduce_partials(int nparts, int n, long stride, const float* ws, float* out, float beta, hipStream_t stream);
extern "C" int clipx_scale(size_t n, float* x, float s, void* stream);

#define DISPATCH_T(dtype, ...)                                        \
    if ((dtype) == CLIPX_F32) { typedef float T; __VA_ARGS__; }       \
    else if ((dtype) == CLIPX_BF16) { typedef bf16_t T; __VA_ARGS__; } \
    else { clipx_set_error("bad dtype %d", (int)(dtype)); return -1; }

// ------------------------------------------------------------------ mask draw
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One block per sample.  Position p gets the 64-bit key hash(key, sample, p) with its low 10 bits replaced by p, so the keys of a
// sample are distinct and ties of the hash are broken by position; the `keep` smallest keys are kept (a uniform draw without
// replacement).  Each position's rank is counted over the sample's keys in LDS; the kept positions are written in ascending order,
// their output slots from a ballot prefix count.
__global__ __launch_bounds__(PK_THREADS) void patch_keep_index_kernel(int G2, int keep, uint64_t key, int* __restrict__ keep_idx) {
    __shared__ uint64_t keys[PK_MAX_G2];
    __shared__ int wave_kept[PK_THREADS / 64];
    const long s = blockIdx.x;
    const uint64_t kmix = splitmix64(key);
    for (int p = threadIdx.x; p < G2; p += PK_THREADS) {
        const uint64_t h = splitmix64(kmix ^ (((uint64_t)s << 10) | (uint64_t)p));
        keys[p] = (h & ~1023ull) | (uint64_t)p;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int p0 = 0; p0 < G2; p0 += PK_THREADS) {
        const int p = p0 + threadIdx.x;
        bool kept = false;
        if (p < G2) {
            const uint64_t k = keys[p];
            int rank = 0;
            for (int q = 0; q < G2; ++q) rank += keys[q] < k ? 1 : 0;
            kept = rank < keep;
        }
        const uint64_t m = __ballot(kept);
        if (lane == 0) wave_kept[wave] = __popcll(m);
        __syncthreads();
        int off = base, total = 0;
        for (int w = 0; w < PK_THREADS / 64; ++w) {
            if (w < wave) off += wave_kept[w];
            total += wave_kept[w];
        }
        if (kept) keep_idx[s * keep + off + __popcll(m & ((1ull << lane) - 1ull))] = p;
        base += total;
        __syncthreads();
    }
}

extern "C" int clipx_patch_keep_index(int batch, int G2, int keep, uint64_t key, int* keep_idx, void* stream) {
    CLIPX_CHECK(G2 > 0 && G2 <= PK_MAX_G2, "patch_keep_index: G2 = %d outside 1..%d", G2, PK_MAX_G2);
    CLIPX_CHECK(keep >= 1 && keep <= G2, "patch_keep_index: keep = %d outside 1..G2", keep);
    if (batch <= 0) return 0;
    hipLaunchKernelGGL(patch_keep_index_kernel, dim3(batch), dim3(PK_THREADS), 0, (hipStream_t)stream, G2, keep, key, keep_idx);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ gathered patch-embed input
// Row (s, j) = patch keep_idx[s, j] of image s, with clipx_patchify's inner order (c, py, px) and zero K padding: the same
// values, so the same bits, as row s*G2 + keep_idx[s, j] of clipx_patchify's output.  An index outside [0, G2) gives a zero row.
template <typename TI, typename T>
__global__ void patchify_keep_kernel(int batch, int H, int W, int P, int Kp, int keep, const int* __restrict__ keep_idx,
                                     const TI* __restrict__ image, T* __restrict__ patches) {
    const int Gw = W / P, Gh = H / P, G2 = Gw * Gh;
    const int kq = Kp >> 2;
    const long total = (long)batch * keep * kq;
    const int K = 3 * P * P;
    const bool vec = (P % 4 == 0) && (W % 4 == 0);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long row = idx / kq;
        const int k = (int)(idx % kq) * 4;
        const int b = (int)(row / keep), g = keep_idx[row];
        const int gy = g / Gw, gx = g % Gw;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g >= 0 && g < G2) {
            if (vec) {
                if (k < K) {
                    const int c = k / (P * P), rem = k % (P * P), py = rem / P, px = rem % P;
                    o = load4(image + (((long)b * 3 + c) * H + gy * P + py) * W + gx * P + px);
                }
            } else {
                float t[4] = {0.f, 0.f, 0.f, 0.f};
                for (int j = 0; j < 4; ++j) {
                    const int kk = k + j;
                    if (kk < K) {
                        const int c = kk / (P * P), rem = kk % (P * P), py = rem / P, px = rem % P;
                        t[j] = to_f(image[(((long)b * 3 + c) * H + gy * P + py) * W + gx * P + px]);
                    }
                }
                o = make_float4(t[0], t[1], t[2], t[3]);
            }
        }
        store4(patches + row * Kp + k, o);
    }
}

extern "C" int clipx_patchify_keep(int img_dtype, int dtype, int batch, int H, int W, int P, int Kp, int keep,
                                   const int* keep_idx, const void* image, void* patches, void* stream) {
    CLIPX_CHECK(H % P == 0 && W % P == 0 && Kp % 4 == 0 && Kp >= 3 * P * P, "patchify_keep: bad geometry");
    CLIPX_CHECK(keep >= 1, "patchify_keep: keep = %d", keep);
    const long total = (long)batch * keep * (Kp / 4);
    if (total <= 0) return 0;
    int grid = (int)((total + 255) / 256);
    if (grid > 65536) grid = 65536;
#define PATCHIFY_KEEP(TI, T) hipLaunchKernelGGL((patchify_keep_kernel<TI, T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, \
                                                batch, H, W, P, Kp, keep, keep_idx, (const TI*)image, (T*)patches)
    if (img_dtype == CLIPX_F32 && dtype == CLIPX_F32) PATCHIFY_KEEP(float, float);
    else if (img_dtype == CLIPX_F32 && dtype == CLIPX_BF16) PATCHIFY_KEEP(float, bf16_t);
    else if (img_dtype == CLIPX_BF16 && dtype == CLIPX_BF16) PATCHIFY_KEEP(bf16_t, bf16_t);
    else if (img_dtype == CLIPX_BF16 && dtype == CLIPX_F32) PATCHIFY_KEEP(bf16_t, float);
    else { clipx_set_error("patchify_keep: bad dtypes"); return -1; }
#undef PATCHIFY_KEEP
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ assemble over the kept tokens
// x0[s, 0] = cls + pos[0]; x0[s, 1+j] = tok[s*keep + j] + pos[1 + keep_idx[s, j]]: the additions of clipx_vision_assemble, so a
// kept row has the bits of the dense assemble's row.  An index outside [0, G2) adds no positional row.
template <typename T>
__global__ void vision_assemble_keep_kernel(int batch, int keep, int G2, int width, const T* __restrict__ tok,
                                            const float* __restrict__ cls, const float* __restrict__ pos,
                                            const int* __restrict__ keep_idx, T* __restrict__ x0) {
    const int wq = width >> 2, L = keep + 1;
    const long total = (long)batch * L * wq;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % wq) * 4;
        const long row = idx / wq;
        const int l = (int)(row % L);
        const long b = row / L;
        int prow = 0;
        float4 v;
        if (l == 0) {
            v = load4(cls + c);
        } else {
            const int g = keep_idx[b * keep + (l - 1)];
            prow = (g >= 0 && g < G2) ? 1 + g : -1;
            v = load4(tok + (b * keep + (l - 1)) * width + c);
        }
        if (prow >= 0) {
            const float4 p = load4(pos + (long)prow * width + c);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        store4(x0 + row * width + c, v);
    }
}

extern "C" int clipx_vision_assemble_keep(int dtype, int batch, int keep, int G2, int width, const void* tok, const float* cls,
                                          const float* pos, const int* keep_idx, void* x0, void* stream) {
    CLIPX_CHECK(width % 4 == 0, "assemble_keep: width %% 4");
    CLIPX_CHECK(keep >= 1 && keep <= G2, "assemble_keep: keep = %d outside 1..G2", keep);
    const long total = (long)batch * (keep + 1) * (width / 4);
    if (total <= 0) return 0;
    int grid = (int)((total + 255) / 256);
    if (grid > 65536) grid = 65536;
    DISPATCH_T(dtype, hipLaunchKernelGGL(vision_assemble_keep_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                                         batch, keep, G2, width, (const T*)tok, cls, pos, keep_idx, (T*)x0));
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// dtok[s*keep + j] = dx0[s, 1+j]
template <typename T>
__global__ void vision_unassemble_keep_kernel(int batch, int keep, int width, const T* __restrict__ dx0, T* __restrict__ dtok) {
    const int wq = width >> 2;
    const long total = (long)batch * keep * wq;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % wq) * 4;
        const long row = idx / wq;
        const long b = row / keep;
        const int j = (int)(row % keep);
        store4(dtok + row * width + c, load4(dx0 + (b * (keep + 1) + 1 + j) * width + c));
    }
}

// ws[part, l, :] = sum over the samples s of the part of the dx0 row that token l (0 = class token, 1+p = patch p) became in
// sample s, or nothing when s dropped patch p.  Block (position tile, part, column tile): the tile's positions -> dx0 rows of the
// part's samples are built in LDS from keep_idx first (so the index need not be sorted), then each thread sums one column quad
// of one position over the samples in sample order, in registers.  The parts are added up afterwards in part order.
template <typename T>
__global__ __launch_bounds__(256) void assemble_keep_partial_kernel(int batch, int per, int keep, int G2, int width,
                                                                    const T* __restrict__ dx0, const int* __restrict__ keep_idx,
                                                                    float* __restrict__ ws) {
    extern __shared__ int rowof[];                                   // [per][PK_POS_TILE]: row within the sample, or -1
    const int l0 = blockIdx.x * PK_POS_TILE;
    const int s0 = blockIdx.y * per, ns = min(per, batch - s0);
    for (int i = threadIdx.x; i < per * PK_POS_TILE; i += 256) {
        const int l = l0 + i % PK_POS_TILE;
        rowof[i] = (l == 0) ? 0 : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ns * keep; i += 256) {
        const int si = i / keep, j = i % keep;
        const int l = 1 + keep_idx[(long)(s0 + si) * keep + j];
        if (l >= 1 && l <= G2 && l >= l0 && l < l0 + PK_POS_TILE) rowof[si * PK_POS_TILE + (l - l0)] = 1 + j;
    }
    __syncthreads();
    const int wq = width >> 2;
    const int q = blockIdx.z * 64 + (threadIdx.x & 63);
    if (q >= wq) return;
    const int c = q * 4;
    const long n = (long)(G2 + 1) * width;
    for (int li = threadIdx.x >> 6; li < PK_POS_TILE; li += 4) {
        const int l = l0 + li;
        if (l > G2) break;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int si = 0; si < ns; ++si) {
            const int r = rowof[si * PK_POS_TILE + li];
            if (r >= 0) {
                const float4 v = load4(dx0 + ((long)(s0 + si) * (keep + 1) + r) * width + c);
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        }
        store4(ws + blockIdx.y * n + (long)l * width + c, acc);
    }
}

extern "C" size_t clipx_vision_assemble_keep_bwd_ws_bytes(int G2, int width) {
    return (size_t)PK_PARTS * (G2 + 1) * width * sizeof(float);
}

extern "C" int clipx_vision_assemble_keep_bwd(int dtype, int batch, int keep, int G2, int width, const void* dx0,
                                              const int* keep_idx, void* dtok, float* dpos, float* dcls, float beta, float* ws,
                                              size_t ws_bytes, void* stream) {
    CLIPX_CHECK(width % 4 == 0, "assemble_keep_bwd: width %% 4");
    CLIPX_CHECK(keep >= 1 && keep <= G2, "assemble_keep_bwd: keep = %d outside 1..G2", keep);
    CLIPX_CHECK(ws_bytes >= clipx_vision_assemble_keep_bwd_ws_bytes(G2, width), "assemble_keep_bwd: workspace too small");
    const int n = (G2 + 1) * width;
    if (batch <= 0) {
        if (beta == 0.f) {
            (void)hipMemsetAsync(dpos, 0, sizeof(float) * n, (hipStream_t)stream);
            (void)hipMemsetAsync(dcls, 0, sizeof(float) * width, (hipStream_t)stream);
        } else if (beta != 1.f) {
            clipx_scale(n, dpos, beta, stream);
            clipx_scale(width, dcls, beta, stream);
        }
        return 0;
    }
    const int per = cdiv(batch, PK_PARTS), nparts = cdiv(batch, per);
    const size_t lds = (size_t)per * PK_POS_TILE * sizeof(int);
    CLIPX_CHECK(lds <= 64 * 1024, "assemble_keep_bwd: batch %d too large", batch);
    const long total = (long)batch * keep * (width / 4);
    int grid = (int)((total + 255) / 256);
    if (grid > 65536) grid = 65536;
    const dim3 pgrid(cdiv(G2 + 1, PK_POS_TILE), nparts, cdiv(width / 4, 64));
    DISPATCH_T(dtype, {
        if (dtok)
            hipLaunchKernelGGL(vision_unassemble_keep_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, batch, keep,
                               width, (const T*)dx0, (T*)dtok);
        hipLaunchKernelGGL(assemble_keep_partial_kernel<T>, pgrid, dim3(256), lds, (hipStream_t)stream, batch, per, keep, G2,
                           width, (const T*)dx0, keep_idx, ws);
    });
    // dpos = beta*dpos + sum of the parts (a position no sample kept gets beta*dpos exactly); dcls = the class token's row
    launch_reduce_partials(nparts, n, n, ws, dpos, beta, (hipStream_t)stream);
    launch_reduce_partials(nparts, width, n, ws, dcls, beta, (hipStream_t)stream);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
