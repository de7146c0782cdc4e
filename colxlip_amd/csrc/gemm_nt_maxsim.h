// MaxSim epilogue of the eight-wave ping-pong NT GEMM (gemm_bf16_nt8p.hip, flag F_MAXSIM): ColBERT similarity of ColClipLoss
// (reference loss.py:20-46) WITHOUT the similarity matrix in memory.
//
// The GEMM is S[(text row r), (image k, token qq)] = txt[r,:] . img[k*q + qq,:]; what the loss needs of it is, per (r, k), the
// maximum over the image's q tokens and the first arg-max.  A wave of the 256x256 tile owns 128 rows x 64 columns (one "slot" of
// 64 columns); with q >= 64 a slot holds at most ONE image boundary, i.e. at most two segments: A = the image col0 / q up to the
// boundary, B = the next image behind it.  The epilogue reduces the wave's accumulators to one (max, index-in-image) per row
// and segment -- in the lane, then across the four lane groups that hold a row's columns -- and stores them to
//     pmax[(2 * slot + seg) * ld + r],  pidx[...]            (row-contiguous: sixteen lanes write sixteen consecutive rows)
// An image spans at most q / 64 + 2 slots; clipx_maxsim_finish folds its partials in slot order (first maximum wins, like
// torch.max).  Nothing of S is written: for B/16 tokens at N = 512 that is 7.9 GB (3.4 GB after the duplicate text rows are
// folded) that the unfused path wrote and read back.
#pragma once
#include "gemm_epi.h"

template <int MT>
__device__ __forceinline__ void nt_maxsim_epilogue(f32x4 (&acc)[4][MT], const EpiB16& epi, int M, int N, int m0, int n0, int wm, int wn,
                                                   int lane) {
    const int g = lane >> 4, c = lane & 15;
    const int q = epi.ms_q;
    const int col0 = n0 + wn * 64;                       // wave-uniform
    if (col0 >= N) return;                               // a slot wholly behind the last image (last tile column): nothing to keep,
                                                         // and the partial arrays have no row for it
    const int slot = col0 >> 6;
    const int kA = col0 / q;
    const int bnd = (kA + 1) * q - col0;                 // first column (relative to col0) of the next image
    const bool has_bnd = bnd < 64;
    const int baseA = col0 - kA * q;                     // index inside image kA of relative column 0
    float* pa = epi.ms_max + (long)(2 * slot) * epi.ms_ld;
    float* pb = pa + epi.ms_ld;
    unsigned short* ia = epi.ms_idx + (long)(2 * slot) * epi.ms_ld;
    unsigned short* ib = ia + epi.ms_ld;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        float mA = -INFINITY, mB = -INFINITY;
        int iA = 0, iB = 0;
        if (!has_bnd) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = acc[i][j][e];
                    const int r = 16 * i + 4 * g + e;
                    if (v > mA) { mA = v; iA = r; }
                }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = acc[i][j][e];
                    const int r = 16 * i + 4 * g + e;
                    const bool b = r >= bnd;
                    const float va = b ? -INFINITY : v, vb = b ? v : -INFINITY;
                    if (va > mA) { mA = va; iA = r; }
                    if (vb > mB) { mB = vb; iB = r; }
                }
        }
        // the row's 64 columns sit in lanes c, c + 16, c + 32, c + 48 (interleaved: column 16 i + 4 g + e): larger value wins,
        // the smaller column on ties
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float om = __shfl_xor(mA, o, 64);
            const int oi = __shfl_xor(iA, o, 64);
            if (om > mA || (om == mA && oi < iA)) { mA = om; iA = oi; }
        }
        if (has_bnd) {
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float om = __shfl_xor(mB, o, 64);
                const int oi = __shfl_xor(iB, o, 64);
                if (om > mB || (om == mB && oi < iB)) { mB = om; iB = oi; }
            }
        }
        const int row = m0 + wm * 16 * MT + 16 * j + c;
        if (g == 0 && row < M) {
            pa[row] = mA;
            ia[row] = (unsigned short)(baseA + iA);
            if (has_bnd) {
                pb[row] = mB;
                ib[row] = (unsigned short)(iB - bnd);
            }
        }
    }
}

// 16 <= q < 64: the slot's images kA, kA + 1, ... one at a time.  Segment s holds the relative columns
// max(0, bnd_{s-1}) <= r < min(64, bnd_s) with bnd_s = (kA + 1 + s) * q - col0 (bnd_{-1} <= 0: image kA began in an earlier slot
// when it is negative).  Same tie rules as above: a larger value wins, the smaller column on equal values.
template <int MT>
__device__ __forceinline__ void nt_maxsim_seg_epilogue(f32x4 (&acc)[4][MT], const EpiB16& epi, int M, int N, int m0, int n0, int wm,
                                                       int wn, int lane) {
    const int g = lane >> 4, c = lane & 15;
    const int q = epi.ms_q;
    const int col0 = n0 + wn * 64;                       // wave-uniform
    if (col0 >= N) return;
    const int kA = col0 / q;
    const int row0 = m0 + wm * 16 * MT + c;
#pragma unroll 1
    for (int k = kA, start = kA * q - col0; start < 64 && col0 + start < N; ++k, start += q) {
        const int lo = start < 0 ? 0 : start;            // start: relative column of the image's token 0
        const int hi = start + q < 64 ? start + q : 64;
        const long o = (long)(2 * k + (start < 0 ? 1 : 0)) * epi.ms_ld;
        float* pm = epi.ms_max + o;
        unsigned short* pi = epi.ms_idx + o;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            float m = -INFINITY;
            int idx = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (16 * i + 16 <= lo || 16 * i >= hi) continue;       // wave-uniform: a 16-column block outside the segment
                if (16 * i >= lo && 16 * i + 16 <= hi) {               // ... wholly inside: no mask
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[i][j][e];
                        if (v > m) { m = v; idx = 16 * i + 4 * g + e; }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 16 * i + 4 * g + e;
                        const float v = (r >= lo && r < hi) ? acc[i][j][e] : -INFINITY;
                        if (v > m) { m = v; idx = r; }
                    }
                }
            }
#pragma unroll
            for (int w = 16; w <= 32; w <<= 1) {
                const float om = __shfl_xor(m, w, 64);
                const int oi = __shfl_xor(idx, w, 64);
                if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
            }
            const int row = row0 + 16 * j;
            if (g == 0 && row < M) {
                pm[row] = m;
                pi[row] = (unsigned short)(idx - start);
            }
        }
    }
}
