// Image input transform on the device (reference factory.py:411-418 builds open_clip's image_transform_v2: torchvision
// RandomResizedCrop, or Resize + CenterCrop, then ToTensor and Normalize, all on PIL images in DataLoader workers).  Here the host
// moves raw uint8 HWC bytes and one kernel does crop, PIL's two-pass resample, normalise and cast, straight into the [b,3,H,W]
// tensor that clipx_patchify reads.
//
// Resample semantics are PIL's (src/libImaging/Resample.c: precompute_coeffs, ImagingResampleHorizontal_8bpc / Vertical_8bpc):
// the horizontal pass over the boxed region first, rounded half up and clamped to [0, 255], then the vertical pass, rounded and
// clamped again.  Per axis, scale = in / out, fs = max(scale, 1), support = (2 bicubic | 1 bilinear) * fs; output index i has
// center = (i + 0.5) * scale, lo = max(0, int(center - support + 0.5)), hi = min(in, int(center + support + 0.5)), and source j
// in [lo, hi) weighs f((j - center + 0.5) / fs), normalised to sum 1 (f: the cubic with a = -0.5, or the triangle).  The
// arithmetic is PIL's too, because exact .5 ties are common (a 2x bilinear downscale is made of them) and a sum that breaks them
// another way lands a level off, two after the second pass: coefficients evaluated in double in PIL's operation order, rounded
// half away from zero to 22-bit fixed point (normalize_coeffs_8bpc), and each pass an int32 sum of level * coefficient started
// at 2^21 and shifted right by 22.
//
// One workgroup per (image, band of IT_BAND output rows).  The band's vertical coefficients go to LDS once.  Then, per chunk of
// output columns (the whole width when its horizontal coefficients fit in LDS) and per group of the band's rows whose source rows
// fit: the horizontal pass of those source rows -> LDS as uint8 levels, planar per channel; the vertical pass from LDS, four
// columns per lane from one 32-bit LDS read per tap, 16-byte (fp32) / 8-byte (bf16) stores along x.  A product is one 24-bit
// multiply (level < 2^8, |coefficient| < 2^23).
//
// Bounds: every load address is box origin + a tap index from the clamped [lo, hi) of a box that is itself clamped to the image,
// and an image whose bytes [offset, offset + 3*h*w) do not lie inside the buffer, or whose scale exceeds IT_MAX_SCALE, is skipped
// (its output left untouched) -- the Python wrapper refuses both before any launch.
#include "common.h"

#define IT_THREADS 256
#define IT_BAND 16                 // output rows per workgroup
#define IT_MAX_SCALE 16            // per axis: support <= 32 source pixels either side
#define IT_MAX_TAPS 65             // int(c + 32.5) - int(c - 31.5)
#define IT_WX_COEFFS 2048          // horizontal coefficients of a column chunk: chunk width * taps <= this (8 KiB)
#define IT_PRECISION_BITS 22       // PIL's PRECISION_BITS for 8-bit channels (32 - 8 - 2)
#define IT_MAX_CHUNK 512           // columns per chunk (lo / count arrays)
#define IT_INTER_BYTES 32768       // horizontal-pass output of a row group: rows * 3 * chunk width <= this

struct ImageMeta {                 // 48 bytes: one int64 offset + ten int32, the wrapper's packed record
    int64_t offset;
    int h, w, top, left, bh, bw, vh, vw, oy, ox;
};

__device__ __forceinline__ double it_filter(int bicubic, double x) {
#pragma clang fp contract(off)
    x = fabs(x);
    if (bicubic) {
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

// coefficients of output index i (in the virtual output) of an axis with `in` source pixels: w[0 .. n), n <= kmax, first tap lo
// (PIL's precompute_coeffs + normalize_coeffs_8bpc, operation for operation; no fused multiply-add, PIL's build has none)
__device__ __forceinline__ void it_coeffs(int bicubic, int i, int in, double scale, double fs, double support, int kmax, int* w,
                                          int* lo_out, int* n_out) {
#pragma clang fp contract(off)
    const double center = (i + 0.5) * scale, ss = 1.0 / fs;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in) hi = in;
    int n = hi - lo;
    if (n > kmax) n = kmax;
    if (n < 1) { n = 1; if (lo > in - 1) lo = in - 1; }
    double sum = 0.0;
    for (int t = 0; t < n; ++t) sum += it_filter(bicubic, (lo + t - center + 0.5) * ss);
    for (int t = 0; t < n; ++t) {
        double k = it_filter(bicubic, (lo + t - center + 0.5) * ss);
        if (sum != 0.0) k /= sum;
        k *= (double)(1 << IT_PRECISION_BITS);
        w[t] = k < 0.0 ? (int)(-0.5 + k) : (int)(0.5 + k);
    }
    *lo_out = lo;
    *n_out = n;
}

// one pass's sum (started at 2^21) -> level: PIL's clip8
__device__ __forceinline__ int it_level(int ss) { return min(max(ss >> IT_PRECISION_BITS, 0), 255); }

template <typename T>
__global__ __launch_bounds__(IT_THREADS) void image_transform_kernel(int bands, const unsigned char* __restrict__ bytes, size_t nbytes,
                                                                     const ImageMeta* __restrict__ meta, int H, int W, float m0,
                                                                     float m1, float m2, float s0, float s1, float s2, int bicubic,
                                                                     T* __restrict__ out) {
    __shared__ int wy[IT_BAND * IT_MAX_TAPS];
    __shared__ int ylo[IT_BAND], yn[IT_BAND];
    __shared__ int wx[IT_WX_COEFFS];
    __shared__ int xlo[IT_MAX_CHUNK], xn[IT_MAX_CHUNK];
    __shared__ __attribute__((aligned(16))) unsigned char inter[IT_INTER_BYTES];

    const int b = blockIdx.x / bands, band = blockIdx.x % bands;
    const ImageMeta im = meta[b];
    const int h = im.h, w = im.w;
    if (h < 1 || w < 1 || im.vh < 1 || im.vw < 1 || im.offset < 0) return;
    if ((uint64_t)im.offset + 3ull * (uint64_t)h * (uint64_t)w > (uint64_t)nbytes) return;
    // the box, clamped to the image; the window, clipped to the virtual output (what lies beyond it is left untouched)
    const int top = min(max(im.top, 0), h - 1), left = min(max(im.left, 0), w - 1);
    const int bh = min(max(im.bh, 1), h - top), bw = min(max(im.bw, 1), w - left);
    if (im.oy < 0 || im.ox < 0 || im.oy >= im.vh || im.ox >= im.vw) return;
    const int Hc = min(H, im.vh - im.oy), Wc = min(W, im.vw - im.ox);
    const double sx = (double)bw / im.vw, sy = (double)bh / im.vh;
    if (sx > IT_MAX_SCALE || sy > IT_MAX_SCALE) return;
    const double fsx = sx > 1.0 ? sx : 1.0, fsy = sy > 1.0 ? sy : 1.0;
    const double base = bicubic ? 2.0 : 1.0;
    const double supx = base * fsx, supy = base * fsy;
    const int kx = min(2 * (int)ceil(supx) + 1, IT_MAX_TAPS), ky = min(2 * (int)ceil(supy) + 1, IT_MAX_TAPS);

    const int y0 = band * IT_BAND, y1 = min(Hc, y0 + IT_BAND);
    if (y0 >= Hc) return;
    if ((int)threadIdx.x < y1 - y0)
        it_coeffs(bicubic, im.oy + y0 + threadIdx.x, bh, sy, fsy, supy, ky, wy + threadIdx.x * IT_MAX_TAPS, &ylo[threadIdx.x],
                  &yn[threadIdx.x]);

    // chunk width: a multiple of 4 whose horizontal coefficients fit, and of which at least `ky` source rows fit
    int tw_max = min(min(IT_WX_COEFFS / kx, IT_INTER_BYTES / (3 * ky)), IT_MAX_CHUNK) & ~3;
    const unsigned char* src = bytes + im.offset + ((long)top * w + left) * 3;
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    const bool vec = (W & 3) == 0;
    const int half = 1 << (IT_PRECISION_BITS - 1);

    for (int cx = 0; cx < Wc; cx += tw_max) {
        const int tw = min(tw_max, Wc - cx), twp = (tw + 3) & ~3, tq = twp >> 2;
        __syncthreads();                                   // the previous chunk's readers are done with wx / xlo / xn / inter
        for (int xl = threadIdx.x; xl < tw; xl += IT_THREADS)
            it_coeffs(bicubic, im.ox + cx + xl, bw, sx, fsx, supx, kx, wx + xl * kx, &xlo[xl], &xn[xl]);
        __syncthreads();
        const int cap = IT_INTER_BYTES / (3 * twp);        // source rows of a group; >= ky by the choice of tw_max
        int g0 = y0;
        while (g0 < y1) {
            const int glo = ylo[g0 - y0];
            int g1 = g0 + 1;
            while (g1 < y1 && ylo[g1 - y0] + yn[g1 - y0] - glo <= cap) ++g1;
            const int rows = min(ylo[g1 - 1 - y0] + yn[g1 - 1 - y0] - glo, cap);
            // horizontal pass: source rows glo .. glo+rows of the box -> inter[row][channel][column]
            for (int idx = threadIdx.x; idx < rows * tw; idx += IT_THREADS) {
                const int r = idx / tw, xl = idx - r * tw;
                const int lo = xlo[xl], n = xn[xl];
                const unsigned char* p = src + ((long)(glo + r) * w + lo) * 3;
                const int* k = wx + xl * kx;
                int a0 = half, a1 = half, a2 = half;
                for (int t = 0; t < n; ++t) {
                    const int kk = k[t];
                    a0 += __mul24((int)p[3 * t], kk);
                    a1 += __mul24((int)p[3 * t + 1], kk);
                    a2 += __mul24((int)p[3 * t + 2], kk);
                }
                unsigned char* q = inter + (long)r * 3 * twp + xl;
                q[0] = (unsigned char)it_level(a0);
                q[twp] = (unsigned char)it_level(a1);
                q[2 * twp] = (unsigned char)it_level(a2);
            }
            __syncthreads();
            // vertical pass: output rows g0 .. g1, four columns of one channel per lane
            const int per_row = 3 * tq;
            for (int idx = threadIdx.x; idx < (g1 - g0) * per_row; idx += IT_THREADS) {
                const int yl = idx / per_row, rem = idx - yl * per_row;
                const int c = rem / tq, x4 = (rem - c * tq) * 4;
                const int yy = g0 - y0 + yl;
                const int lo = ylo[yy] - glo, n = min(yn[yy], rows - lo);
                const int* k = wy + yy * IT_MAX_TAPS;
                const unsigned char* q = inter + ((long)lo * 3 + c) * twp + x4;
                int s4[4] = {half, half, half, half};
                for (int t = 0; t < n; ++t) {
                    const unsigned int v = *reinterpret_cast<const unsigned int*>(q + (long)t * 3 * twp);
                    const int kk = k[t];
                    s4[0] += __mul24((int)(v & 255u), kk);
                    s4[1] += __mul24((int)((v >> 8) & 255u), kk);
                    s4[2] += __mul24((int)((v >> 16) & 255u), kk);
                    s4[3] += __mul24((int)(v >> 24), kk);
                }
                float a[4];
                // ToTensor (level / 255) then Normalize ((x - mean) / std), each step rounded to fp32 as torchvision does
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = __fdiv_rn(__fdiv_rn((float)it_level(s4[j]), 255.f) - mean[c], sd[c]);
                const int x = cx + x4;
                T* o = out + (((long)b * 3 + c) * H + (g0 + yl)) * W + x;
                if (vec && x + 4 <= Wc) {
                    store4(o, make_float4(a[0], a[1], a[2], a[3]));
                } else {
                    for (int j = 0; j < 4 && x + j < cx + tw; ++j) o[j] = from_f<T>(a[j]);
                }
            }
            __syncthreads();
            g0 = g1;
        }
    }
}

extern "C" int clipx_image_transform(int batch, const void* bytes, size_t nbytes, const void* meta, int H, int W, float mean0,
                                     float mean1, float mean2, float std0, float std1, float std2, int bicubic, int out_dtype,
                                     void* out, void* stream) {
    CLIPX_CHECK(H >= 1 && W >= 1, "image_transform: output %d x %d", H, W);
    CLIPX_CHECK(std0 != 0.f && std1 != 0.f && std2 != 0.f, "image_transform: zero std");
    if (batch <= 0) return 0;
    const int bands = cdiv(H, IT_BAND);
    CLIPX_CHECK((long)batch * bands < (1l << 31), "image_transform: batch %d too large", batch);
    const dim3 grid((unsigned)((long)batch * bands));
#define IMAGE_TRANSFORM(T) hipLaunchKernelGGL(image_transform_kernel<T>, grid, dim3(IT_THREADS), 0, (hipStream_t)stream, bands, \
                                              (const unsigned char*)bytes, nbytes, (const ImageMeta*)meta, H, W, mean0, mean1, mean2, \
                                              std0, std1, std2, bicubic ? 1 : 0, (T*)out)
    if (out_dtype == CLIPX_F32) IMAGE_TRANSFORM(float);
    else if (out_dtype == CLIPX_BF16) IMAGE_TRANSFORM(bf16_t);
    else { clipx_set_error("image_transform: bad dtype %d", out_dtype); return -1; }
#undef IMAGE_TRANSFORM
    CLIPX_LAUNCH_CHECK();
    return 0;
}
