// Performance-mode TN GEMM (wgrad):  dw[N,K] (+)= dy[M,N]^T . x[M,K], bf16 operands, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16.  The reduction dim is the ROW index of both operands, so both MFMA fragments come
// from ds_read_b64_tr_b16 (hardware-transposed LDS reads) of row-major [m][n] / [m][k] tiles.
//
// 256(n) x 256(k) output tile, 8 waves (2x4: 128 k x 64 n each = 8x4 MFMA tiles).  Operands stream through the
// same FIVE-slot ring of 32-KiB items as the NT kernel: an item is 64 reduction rows x 256 columns of dy or of x,
// filled by 16-byte global_load_lds, three items in flight while two are computed on; counted s_waitcnt vmcnt +
// raw s_barrier, ONE barrier per 64 reduction rows (two 32-deep MFMA slices).  Within a step the fragment reads of
// the second slice are issued between the first slice's MFMAs (pinned with sched_group_barrier).
// LDS image of an item: two 128-column halves of [64 rows][256 B]; 16-B chunk c of row r stored at
// c ^ (((r&3)<<2) | ((r>>2)&3)) (swizzle applied on the per-lane SOURCE address): conflict-free tr reads.
// The reduction over M is split across blocks (fp32 slabs + a reduce pass) so that tiles x splits ~ one block per
// CU; the work list is dealt to the XCDs in contiguous runs so the tiles of one M-split share an L2 (rocprofv3
// FETCH_SIZE: 3.0x the algorithmic bytes before, 1.2x after).  Rows beyond the split / M and columns beyond N / K
// are fed from a zero page.
// Bias gradient for free: colsum_m dy[m,n] = (ones[k,m] . dy[m,n]) for any k, i.e. one more MFMA per n-tile with a
// constant all-ones A fragment on the dy fragments that are in registers anyway.  The tiles_k blocks that stage
// the same dy rows take every tiles_k-th slice each, and a wave pair (wk = 0/1) splits the four n-tiles: +2 MFMAs
// on 1/tiles_k of the slices.  Partials [split*tiles_k + tk][N] are folded by the slab-reduce kernel.
#include "kernels.h"

static __device__ __attribute__((aligned(64))) unsigned char g_zero_page[64];

#define TN_BN 256          // dy columns (n) per block
#define TN_BK 256          // x columns (k) per block
#define TN_BM 64           // reduction rows per ring item / per barrier
#define TN_SLOTS 5
#define TN_SLOT_BYTES (TN_BM * 512)          // 64 rows x 256 columns: 32 KiB
#define TN_HALF_BYTES (TN_BM * 256)          // one 128-column half of an item

#ifndef TN_FAST_LOADER
#define TN_FAST_LOADER 1   // buffer-descriptor LDS-DMA addressing when N and K are multiples of 256 (every production shape)
#endif

__device__ __forceinline__ void tn_wait_vmcnt(int n) {
    if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__device__ __forceinline__ bf16x8 tn_join(s16x4 lo, s16x4 hi) {
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo;
    u.s.b = hi;
    return u.v;
}

__global__ __launch_bounds__(512, 2) void gemm_bf16_tn_kernel(int M, int N, int K, const bf16_t* __restrict__ DY,
                                                              const bf16_t* __restrict__ X, float* __restrict__ dw,
                                                              float beta, float* __restrict__ slabs, int tiles_n,
                                                              int tiles_k, int splits, int rows_per_split,
                                                              float* __restrict__ cs_part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15, q = c >> 2, p = c & 3;
    const int wk = wave >> 2, wn = wave & 3;

    const int tiles = tiles_n * tiles_k;
    // XCD-aware work order: hardware deals blocks to the 8 XCDs round-robin (block b -> XCD b & 7); re-index so
    // that each XCD owns a CONTIGUOUS run of the (split-major, tile-minor) work list.
    const int per_xcd = gridDim.x >> 3;
    const int work = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (work >= tiles * splits) return;
    const int split = work / tiles, t = work % tiles;
    const int tn = t / tiles_k, tk = t % tiles_k;
    const int n0 = tn * TN_BN, k0 = tk * TN_BK;
    const int m_begin = split * rows_per_split;
    int m_end = m_begin + rows_per_split;
    if (m_end > M) m_end = M;
    const int nsteps = (m_end - m_begin + TN_BM - 1) / TN_BM;
    const int nitems = 2 * nsteps;      // dy(0) x(0) dy(1) x(1) ...

    // staging: an item is 32 pieces of 1 KiB (= 4 rows x 256 B of one 128-column half); wave w stages pieces
    // 4w..4w+3.  lane -> row l>>4 of the piece, 16-B slot l&15.
    const int srow = lane >> 4, sslot = lane & 15;
    int prow[4], pcol[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pc = 4 * wave + i;
        const int half = pc >> 4, r = 4 * (pc & 15) + srow;
        const int lchunk = sslot ^ (((r & 3) << 2) | ((r >> 2) & 3));
        prow[i] = r;
        pcol[i] = half * 128 + lchunk * 8;
    }
    int it_next = 0;
    // FAST LOADER (N % 256 == 0 and K % 256 == 0): one descriptor per operand covering this block's rows [m_begin, m_end) of
    // its 256-column strip, ONE per-lane byte offset per piece and operand, the 64-row step as the scalar offset; rows beyond
    // m_end fall outside the descriptor and read as zero.  The pointer form costs ~15 vector instructions per piece.
    const bool fast = TN_FAST_LOADER && (N % TN_BN) == 0 && (K % TN_BK) == 0 &&
                      (long)(m_end - m_begin) * (N > K ? N : K) * 2 < (1l << 31);      // 32-bit buffer offsets
    unsigned voff_dy[4], voff_x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        voff_dy[i] = (unsigned)(prow[i] * N + pcol[i]) * 2u;
        voff_x[i] = (unsigned)(prow[i] * K + pcol[i]) * 2u;
    }
    __amdgpu_buffer_rsrc_t rdy, rxx;
    if (fast) {
        const int rows = m_end - m_begin;
        rdy = __builtin_amdgcn_make_buffer_rsrc((void*)(DY + (long)m_begin * N + n0), 0, ((rows - 1) * N + TN_BN) * 2, 0x00020000);
        rxx = __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long)m_begin * K + k0), 0, ((rows - 1) * K + TN_BK) * 2, 0x00020000);
    }
    auto issue_item = [&](int slot) {
        char* base = smem + slot * TN_SLOT_BYTES;
        if (fast) {
            const int step = it_next >> 1;
            if (it_next & 1) {
                const int so = step * (TN_BM * 2) * K;
#pragma unroll
                for (int i = 0; i < 4; ++i) lds_dma_piece(rxx, base + (4 * wave + i) * 1024, voff_x[i], so);
            } else {
                const int so = step * (TN_BM * 2) * N;
#pragma unroll
                for (int i = 0; i < 4; ++i) lds_dma_piece(rdy, base + (4 * wave + i) * 1024, voff_dy[i], so);
            }
            ++it_next;
            return;
        }
        const bool is_x = it_next & 1;
        const bf16_t* src = is_x ? X : DY;
        const int ld = is_x ? K : N, c0 = is_x ? k0 : n0;
        const int mrow0 = m_begin + (it_next >> 1) * TN_BM;
        const bf16_t* zp = reinterpret_cast<const bf16_t*>(g_zero_page);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mrow = mrow0 + prow[i], col = c0 + pcol[i];
            glds16((mrow < m_end && col < ld) ? src + (long)mrow * ld + col : zp, base + (4 * wave + i) * 1024);
        }
        ++it_next;
    };

    f32x4 acc[8][4];   // [k-tile][n-tile]: D[k][n]; a lane owns 4 consecutive k of one n
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // transposed-read addressing (lane 4q+p of a 16-lane group: block row q, columns 4p..4p+3)
    // row(h) = 8g + 4h + q (+32 for the second slice); swizzle = (q<<2) | ((2g+h)&3); a 16-column block starts at
    // 16-B chunk 2*tile (+ p>>1).  Per-lane byte offsets inside a ring slot, fragment r of a slice:
    // r = 0..3: dy n-tile r (B operand, half wn>>1, tiles 4*(wn&1)+r);  r = 4..11: x k-tile r-4 (A operand, half wk)
    const int row0 = 8 * g + q, row1 = row0 + 4;
    const int sw0 = (q << 2) | ((2 * g) & 3), sw1 = (q << 2) | ((2 * g + 1) & 3);
    const int ro0 = row0 * 256 + (p & 1) * 8, ro1 = row1 * 256 + (p & 1) * 8;
    unsigned foff[12][2];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        const int half_base = (r < 4) ? (wn >> 1) * TN_HALF_BYTES : wk * TN_HALF_BYTES;
        const int tile = (r < 4) ? 4 * (wn & 1) + r : r - 4;
        const int ch = 2 * tile + (p >> 1);
        foff[r][0] = half_base + ro0 + ((ch ^ sw0) << 4);
        foff[r][1] = half_base + ro1 + ((ch ^ sw1) << 4);
    }
    const unsigned lds0 = (unsigned)(size_t)smem;

    f32x4 cs[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.0f;
    const bool do_cs = cs_part != nullptr;
    int cs_wait = tk;              // this block takes the 32-row slices with index % tiles_k == tk

    int inflight = 0, wslot = 0, rslot = 0;
#pragma unroll 1
    for (int i = 0; i < TN_SLOTS; ++i)
        if (it_next < nitems) { issue_item(wslot); wslot = (wslot + 1 == TN_SLOTS) ? 0 : wslot + 1; ++inflight; }

    // The fragment reads and their waits are inline asm.  Through the intrinsic the compiler puts s_waitcnt vmcnt(0)
    // in front of the first LDS read of every step (LDS-DMA may alias it), which drains the whole ring -- including
    // the items issued a moment earlier -- and left this kernel at 0.57x the NT kernel's rate per step.
    // A step's 24 fragments (slice 0: dy 0..3, x 0..7; slice 1 likewise) are read in order with at most ~7
    // fragments (14 reads, the LGKM counter holds 15) in flight; MFMA group (s,i) = x-tile i of slice s against the
    // four dy tiles waits for exactly its own fragment.
    s16x4 flo[24], fhi[24];
#define TN_ADDR(f, h) (((f) % 12 < 4 ? ybs : xbs) + foff[(f) % 12][h])
#define TN_ISSUE(f)                                                                                                 \
    {                                                                                                               \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(flo[f]) : "v"(TN_ADDR(f, 0)), "n"(((f) / 12) * 8192)); \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(fhi[f]) : "v"(TN_ADDR(f, 1)), "n"(((f) / 12) * 8192)); \
    }
#define TN_WAIT1(n, f) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(flo[f]), "+v"(fhi[f]))
#define TN_WAIT5(n, f0, f1, f2, f3, f4)                                                                             \
    asm volatile("s_waitcnt lgkmcnt(" #n ")"                                                                        \
                 : "+v"(flo[f0]), "+v"(fhi[f0]), "+v"(flo[f1]), "+v"(fhi[f1]), "+v"(flo[f2]), "+v"(fhi[f2]),        \
                   "+v"(flo[f3]), "+v"(fhi[f3]), "+v"(flo[f4]), "+v"(fhi[f4]))
#define TN_FRAG(f) tn_join(flo[f], fhi[f])
#define TN_GROUP(s, i)                                                                                              \
    {                                                                                                               \
        const bf16x8 a_ = TN_FRAG((s) * 12 + 4 + (i));                                                              \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                               \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_, TN_FRAG((s) * 12 + j), acc[i][j], 0, 0, 0);     \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
    }

#pragma unroll 1
    for (int step = 0; step < nsteps; ++step) {
        tn_wait_vmcnt(4 * (inflight - 2));     // every item is 4 pieces per wave
        __builtin_amdgcn_s_barrier();          // all pieces landed; everyone left the previous step's slots
        if (step > 0) {
#pragma unroll 1
            for (int i = 0; i < 2; ++i)
                if (it_next < nitems) { issue_item(wslot); wslot = (wslot + 1 == TN_SLOTS) ? 0 : wslot + 1; ++inflight; }
        }
        const int xsl = (rslot + 1 == TN_SLOTS) ? 0 : rslot + 1;
        const unsigned ybs = lds0 + rslot * TN_SLOT_BYTES, xbs = lds0 + xsl * TN_SLOT_BYTES;
        __builtin_amdgcn_sched_barrier(0);
        TN_ISSUE(0) TN_ISSUE(1) TN_ISSUE(2) TN_ISSUE(3) TN_ISSUE(4) TN_ISSUE(5) TN_ISSUE(6)
        TN_ISSUE(7) TN_ISSUE(8) TN_ISSUE(9) TN_ISSUE(10)
        TN_WAIT5(12, 0, 1, 2, 3, 4);   TN_GROUP(0, 0)
        TN_ISSUE(11) TN_WAIT1(12, 5);  TN_GROUP(0, 1)
        TN_ISSUE(12) TN_WAIT1(12, 6);  TN_GROUP(0, 2)
        TN_ISSUE(13) TN_WAIT1(12, 7);  TN_GROUP(0, 3)
        TN_ISSUE(14) TN_WAIT1(12, 8);  TN_GROUP(0, 4)
        TN_ISSUE(15) TN_WAIT1(12, 9);  TN_GROUP(0, 5)
        TN_ISSUE(16) TN_WAIT1(12, 10); TN_GROUP(0, 6)
        TN_ISSUE(17) TN_WAIT1(12, 11); TN_GROUP(0, 7)
        TN_ISSUE(18) TN_ISSUE(19) TN_ISSUE(20) TN_ISSUE(21) TN_ISSUE(22)
        TN_WAIT5(12, 12, 13, 14, 15, 16); TN_GROUP(1, 0)
        TN_ISSUE(23) TN_WAIT1(12, 17); TN_GROUP(1, 1)
        TN_WAIT1(10, 18); TN_GROUP(1, 2)
        TN_WAIT1(8, 19);  TN_GROUP(1, 3)
        TN_WAIT1(6, 20);  TN_GROUP(1, 4)
        TN_WAIT1(4, 21);  TN_GROUP(1, 5)
        TN_WAIT1(2, 22);  TN_GROUP(1, 6)
        TN_WAIT1(0, 23);  TN_GROUP(1, 7)
        if (do_cs) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (cs_wait == 0) {
                    cs[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, wk ? TN_FRAG(s2 * 12 + 2) : TN_FRAG(s2 * 12 + 0), cs[0], 0, 0, 0);
                    cs[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, wk ? TN_FRAG(s2 * 12 + 3) : TN_FRAG(s2 * 12 + 1), cs[1], 0, 0, 0);
                    cs_wait = tiles_k;
                }
                --cs_wait;
            }
        }
        rslot = (rslot + 2 >= TN_SLOTS) ? rslot + 2 - TN_SLOTS : rslot + 2;
        inflight -= 2;
    }

    if (do_cs && g == 0) {
        float* row = cs_part + (long)(split * tiles_k + tk) * N;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int n = n0 + wn * 64 + 16 * (2 * wk + jj) + c;
            if (n < N) row[n] = cs[jj][0];
        }
    }

    float* dst = (splits > 1) ? slabs + (long)split * N * K : dw;
    const float b = (splits > 1) ? 0.f : beta;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + 16 * j + c;
        if (n >= N) continue;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + wk * 128 + 16 * i + 4 * g;
            if (k >= K) continue;
            float* o = dst + (long)n * K + k;
            float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            if (b != 0.f) {
                const float4 old = load4(o);
                v.x += b * old.x; v.y += b * old.y; v.z += b * old.z; v.w += b * old.w;
            }
            store4(o, v);
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// PING-PONG form of the same kernel (see gemm_nt_pp.h for the scheme and its hazard analysis): a step is an L segment
// (48 transposed fragment reads + 8 LDS-DMA pieces) and a C segment (64 MFMAs) with a barrier after each, and waves 4-7 run one
// segment behind waves 0-3, so on every SIMD one wave multiplies while its partner loads.  Groups split the tile by x columns
// (wk = wave >> 2, as before): the dy rows of a step are SHARED (3 slots x 32 KiB), each group's 128-column half of the x rows
// is PRIVATE (2 slots x 16 KiB per group) and is staged by the OTHER group:
//     A in L_j issues  x_B(j+1) [4 pieces/wave], then its half of dy(j+2) [4];  waits vmcnt(4) at the end of C_j
//     B in L_j issues  x_A(j+2) [4],             then its half of dy(j+2) [4];  waits vmcnt(0) at the end of C_j
// Needs the buffer-descriptor loader (N, K multiples of 256): rows beyond the split read as zero through the descriptor.
#define TNP_DY_BYTES (TN_BM * 512)      // 32 KiB
#define TNP_X_BYTES (TN_BM * 256)       // 16 KiB: one group's 128 columns
#define TNP_X_BASE (3 * TNP_DY_BYTES)
#define TNP_LDS (3 * TNP_DY_BYTES + 4 * TNP_X_BYTES)
#define TNP_ADDR(f, h) (((f) % 12 < 4 ? (h ? yb1 : yb0) ^ (unsigned)(((f) % 12) << 5) : (h ? xb1 : xb0) ^ (unsigned)(((f) % 12 - 4) << 5)))
#define TNP_ISSUE(f)                                                                                                \
    {                                                                                                               \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(flo[f]) : "v"(TNP_ADDR(f, 0)), "n"(((f) / 12) * 8192)); \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(fhi[f]) : "v"(TNP_ADDR(f, 1)), "n"(((f) / 12) * 8192)); \
    }
#ifdef PP_PROFILE
// per wave: [0] total [1] up to the end of the step loop [2] L segment [3] read wait + barrier after L [4] C segment [5] vmcnt wait
// [6] barrier after C [7] steps
__device__ unsigned long long g_tnp_dbg[64];
extern "C" int clipx_debug_tnpp(unsigned long long* out, int reset) {
    if (reset) {
        unsigned long long z[64] = {0};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_tnp_dbg), z, sizeof(z));
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tnp_dbg), 64 * sizeof(unsigned long long));
}
#endif
#ifndef TNP_WAIT_MODE
#define TNP_WAIT_MODE 0      // 1: waits as late as the data dependences allow (some at the end of the L segment)
#endif
// The body of the ping-pong wgrad kernel for ONE work item (`work` = split * tiles + tile of one problem); shared by the
// single-problem kernel and the grouped one below (same code, inlined into both).
__device__ __forceinline__ void tn_pp_body(int M, int N, int K, const bf16_t* __restrict__ DY, const bf16_t* __restrict__ X,
                                           float* __restrict__ dw, float beta, float* __restrict__ slabs, int tiles_n, int tiles_k,
                                           int splits, int rows_per_split, float* __restrict__ cs_part, int work) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15, q = c >> 2, p = c & 3;
    const int wk = wave >> 2, wn = wave & 3;        // wk = group
    const int grp = wk, og = wk ^ 1;

    const int tiles = tiles_n * tiles_k;
    if (work >= tiles * splits) return;
    const int split = work / tiles, t = work % tiles;
    const int tn = t / tiles_k, tk = t % tiles_k;
    const int n0 = tn * TN_BN, k0 = tk * TN_BK;
    const int m_begin = split * rows_per_split;
    int m_end = m_begin + rows_per_split;
    if (m_end > M) m_end = M;
    const int rows = m_end - m_begin;
    const int nsteps = (rows + TN_BM - 1) / TN_BM;

    // staging.  dy item: 32 pieces (piece pc: half pc >> 4, rows 4*(pc&15)..+3), wave w stages 4w..4w+3.  x half of the other
    // group: 16 pieces, wave wn of this group stages 4wn..4wn+3.  lane -> row l>>4 of the piece, 16-byte slot l&15.
    const int srow = lane >> 4, sslot = lane & 15;
    // per-lane byte offset of piece 0; piece i is 4 rows further (through the scalar offset) and its chunk swizzle differs in
    // the two low bits only: row r = 4*(pc&15) + srow has r&3 = srow and (r>>2)&3 = i, so chunk = sslot ^ (srow<<2) ^ i
    unsigned voff_dy0, voff_x0;
    {
        const int pc = 4 * wave;
        const int half = pc >> 4, r = 4 * (pc & 15) + srow;
        voff_dy0 = (unsigned)(r * N + half * 128 + (sslot ^ (srow << 2)) * 8) * 2u;
        const int rx_ = 4 * (4 * wn) + srow;
        voff_x0 = (unsigned)(rx_ * K + og * 128 + (sslot ^ (srow << 2)) * 8) * 2u;
    }
    const __amdgpu_buffer_rsrc_t rdy =
        __builtin_amdgcn_make_buffer_rsrc((void*)(DY + (long)m_begin * N + n0), 0, ((rows - 1) * N + TN_BN) * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rxx =
        __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long)m_begin * K + k0), 0, ((rows - 1) * K + TN_BK) * 2, 0x00020000);
    int sy = 0, sx = 0, yls = 0, xls = 0;      // step cursors and the slots they write next
    auto issue_dy = [&]() -> bool {
        if (sy >= nsteps) return false;
        char* dst = smem + yls * TNP_DY_BYTES + (4 * wave) * 1024;
        const int so = sy * (TN_BM * 2) * N;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma_piece(rdy, dst + i * 1024, voff_dy0 ^ (unsigned)(i << 4), so + i * 8 * N);
        yls = (yls == 2) ? 0 : yls + 1;
        ++sy;
        return true;
    };
    auto issue_x = [&]() -> bool {
        if (sx >= nsteps) return false;
        char* dst = smem + TNP_X_BASE + og * (2 * TNP_X_BYTES) + xls * TNP_X_BYTES + (4 * wn) * 1024;
        const int so = sx * (TN_BM * 2) * K;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma_piece(rxx, dst + i * 1024, voff_x0 ^ (unsigned)(i << 4), so + i * 8 * K);
        xls ^= 1;
        ++sx;
        return true;
    };

    // prologue = the issues of the virtual segments L_-2, L_-1:  A: dy(0) | x_B(0), dy(1);   B: x_A(0), dy(0) | x_A(1), dy(1)
    if (grp == 0) {
        issue_dy();
        issue_x();
        issue_dy();
    } else {
        issue_x();
        issue_dy();
        issue_x();
        issue_dy();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();     // B runs one segment behind

    f32x4 acc[8][4];   // [k-tile][n-tile]: D[k][n]; a lane owns 4 consecutive k of one n
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // transposed-read addressing: as in the kernel above, but the x fragments come from the group's own 16-KiB half slot
    const int row0 = 8 * g + q, row1 = row0 + 4;
    const int sw0 = (q << 2) | ((2 * g) & 3), sw1 = (q << 2) | ((2 * g + 1) & 3);
    const int ro0 = row0 * 256 + (p & 1) * 8, ro1 = row1 * 256 + (p & 1) * 8;
    // fragment r of a slice sits at chunk (8*(wn&1) | 2*r | p>>1) ^ sw (dy) or (2*(r-4) | p>>1) ^ sw (x): the tile index only
    // flips address bits 5..7, so four base addresses and one v_xor per read replace the 24 per-lane offsets of the kernel above
    const unsigned ay0 = (wn >> 1) * TN_HALF_BYTES + ro0 + ((((8 * (wn & 1)) | (p >> 1)) ^ sw0) << 4);
    const unsigned ay1 = (wn >> 1) * TN_HALF_BYTES + ro1 + ((((8 * (wn & 1)) | (p >> 1)) ^ sw1) << 4);
    const unsigned ax0 = ro0 + (((p >> 1) ^ sw0) << 4);
    const unsigned ax1 = ro1 + (((p >> 1) ^ sw1) << 4);
    const unsigned lds0 = (unsigned)(size_t)smem;
    const unsigned xring = lds0 + TNP_X_BASE + grp * (2 * TNP_X_BYTES);

    f32x4 cs[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.0f;
    const bool do_cs = cs_part != nullptr;
    int cs_wait = tk;

    s16x4 flo[24], fhi[24];
    int yrs = 0, xrs = 0, y_prev = 0;
#ifdef PP_PROFILE
    long p_t0 = clock64(), p_l = 0, p_lw = 0, p_c = 0, p_vm = 0, p_cb = 0;
#endif
#pragma unroll 1
    for (int step = 0; step < nsteps; ++step) {
        // ---- L segment
#ifdef PP_PROFILE
        long t0 = clock64();
#endif
        const unsigned yb0 = lds0 + yrs * TNP_DY_BYTES + ay0, yb1 = lds0 + yrs * TNP_DY_BYTES + ay1;
        const unsigned xb0 = xring + xrs * TNP_X_BYTES + ax0, xb1 = xring + xrs * TNP_X_BYTES + ax1;
        __builtin_amdgcn_sched_barrier(0);
        TNP_ISSUE(0) TNP_ISSUE(1) TNP_ISSUE(2) TNP_ISSUE(3) TNP_ISSUE(4) TNP_ISSUE(5) TNP_ISSUE(6) TNP_ISSUE(7) TNP_ISSUE(8) TNP_ISSUE(9)
        TNP_ISSUE(10) TNP_ISSUE(11)
        __builtin_amdgcn_sched_barrier(0);
        const bool xi = issue_x();
        __builtin_amdgcn_sched_barrier(0);
        TNP_ISSUE(12) TNP_ISSUE(13) TNP_ISSUE(14) TNP_ISSUE(15) TNP_ISSUE(16) TNP_ISSUE(17) TNP_ISSUE(18) TNP_ISSUE(19) TNP_ISSUE(20)
        TNP_ISSUE(21) TNP_ISSUE(22) TNP_ISSUE(23)
        __builtin_amdgcn_sched_barrier(0);
        const bool yi = issue_dy();
        __builtin_amdgcn_sched_barrier(0);
#ifdef PP_PROFILE
        long t1 = clock64();
#endif
#if TNP_WAIT_MODE == 1
        // deep waits: what this wave issued in its PREVIOUS L segment for the readers right after this barrier has landed --
        // A: x_B (its dy pieces of that segment, needed one barrier later, may stay in flight), B: everything
        {
            const int now = (xi ? 4 : 0) + (yi ? 4 : 0);
            tn_wait_vmcnt(grp == 0 ? now + y_prev : now);
        }
#endif
        // all 24 fragments in registers before the barrier: the slots may be refilled right after it
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(flo[0]), "+v"(flo[1]), "+v"(flo[2]), "+v"(flo[3]), "+v"(flo[4]), "+v"(flo[5]), "+v"(flo[6]),
                       "+v"(flo[7]), "+v"(flo[8]), "+v"(flo[9]), "+v"(flo[10]), "+v"(flo[11]), "+v"(flo[12]), "+v"(flo[13]),
                       "+v"(flo[14]), "+v"(flo[15]), "+v"(flo[16]), "+v"(flo[17]), "+v"(flo[18]), "+v"(flo[19]), "+v"(flo[20]),
                       "+v"(flo[21]), "+v"(flo[22]), "+v"(flo[23]));
        asm volatile(""
                     : "+v"(fhi[0]), "+v"(fhi[1]), "+v"(fhi[2]), "+v"(fhi[3]), "+v"(fhi[4]), "+v"(fhi[5]), "+v"(fhi[6]),
                       "+v"(fhi[7]), "+v"(fhi[8]), "+v"(fhi[9]), "+v"(fhi[10]), "+v"(fhi[11]), "+v"(fhi[12]), "+v"(fhi[13]),
                       "+v"(fhi[14]), "+v"(fhi[15]), "+v"(fhi[16]), "+v"(fhi[17]), "+v"(fhi[18]), "+v"(fhi[19]), "+v"(fhi[20]),
                       "+v"(fhi[21]), "+v"(fhi[22]), "+v"(fhi[23]));
        __builtin_amdgcn_s_barrier();
#ifdef PP_PROFILE
        long t2 = clock64();
#endif
        // ---- C segment
        __builtin_amdgcn_sched_barrier(0);
        TN_GROUP(0, 0) TN_GROUP(0, 1) TN_GROUP(0, 2) TN_GROUP(0, 3) TN_GROUP(0, 4) TN_GROUP(0, 5) TN_GROUP(0, 6) TN_GROUP(0, 7)
        TN_GROUP(1, 0) TN_GROUP(1, 1) TN_GROUP(1, 2) TN_GROUP(1, 3) TN_GROUP(1, 4) TN_GROUP(1, 5) TN_GROUP(1, 6) TN_GROUP(1, 7)
        if (do_cs) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (cs_wait == 0) {
                    cs[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, wk ? TN_FRAG(s2 * 12 + 2) : TN_FRAG(s2 * 12 + 0), cs[0], 0, 0, 0);
                    cs[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, wk ? TN_FRAG(s2 * 12 + 3) : TN_FRAG(s2 * 12 + 1), cs[1], 0, 0, 0);
                    cs_wait = tiles_k;
                }
                --cs_wait;
            }
        }
#ifdef PP_PROFILE
        long t3 = clock64();
#endif
#if TNP_WAIT_MODE == 1
        if (grp == 0) tn_wait_vmcnt((xi ? 4 : 0) + (yi ? 4 : 0));      // A: its dy pieces of the previous segment
        y_prev = yi ? 4 : 0;
#else
        if (grp == 0 && yi) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
#ifdef PP_PROFILE
        long t4 = clock64();
#endif
        __builtin_amdgcn_s_barrier();
#ifdef PP_PROFILE
        long t5 = clock64();
        p_l += t1 - t0; p_lw += t2 - t1; p_c += t3 - t2; p_vm += t4 - t3; p_cb += t5 - t4;
#endif
        yrs = (yrs == 2) ? 0 : yrs + 1;
        xrs ^= 1;
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();     // the barrier that ends B's last C segment
#ifdef PP_PROFILE
    const long p_t1 = clock64();
#endif

    if (do_cs && g == 0) {
        float* row = cs_part + (long)(split * tiles_k + tk) * N;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int n = n0 + wn * 64 + 16 * (2 * wk + jj) + c;
            if (n < N) row[n] = cs[jj][0];
        }
    }
    float* dst = (splits > 1) ? slabs + (long)split * N * K : dw;
    const float b = (splits > 1) ? 0.f : beta;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + 16 * j + c;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + wk * 128 + 16 * i + 4 * g;
            float* o = dst + (long)n * K + k;
            float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            if (b != 0.f) {
                const float4 old = load4(o);
                v.x += b * old.x; v.y += b * old.y; v.z += b * old.z; v.w += b * old.w;
            }
            store4(o, v);
        }
    }
#ifdef PP_PROFILE
    if (lane == 0) {
        unsigned long long* d = g_tnp_dbg + wave * 8;
        atomicAdd(&d[0], (unsigned long long)(clock64() - p_t0));
        atomicAdd(&d[1], (unsigned long long)(p_t1 - p_t0));
        atomicAdd(&d[2], (unsigned long long)p_l);
        atomicAdd(&d[3], (unsigned long long)p_lw);
        atomicAdd(&d[4], (unsigned long long)p_c);
        atomicAdd(&d[5], (unsigned long long)p_vm);
        atomicAdd(&d[6], (unsigned long long)p_cb);
        atomicAdd(&d[7], (unsigned long long)nsteps);
    }
#endif
}

__global__ __launch_bounds__(512, 2) void gemm_bf16_tn_pp_kernel(int M, int N, int K, const bf16_t* __restrict__ DY,
                                                                 const bf16_t* __restrict__ X, float* __restrict__ dw,
                                                                 float beta, float* __restrict__ slabs, int tiles_n,
                                                                 int tiles_k, int splits, int rows_per_split,
                                                                 float* __restrict__ cs_part) {
    const int per_xcd = gridDim.x >> 3;
    const int work = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    tn_pp_body(M, N, K, DY, X, dw, beta, slabs, tiles_n, tiles_k, splits, rows_per_split, cs_part, work);
}

// GROUPED launch: up to TN_GROUP_MAX wgrads that reduce over the SAME M rows (the four of a residual block: dW of in_proj, out_proj,
// c_fc, c_proj) as one grid.  Launched one by one, a problem with few output tiles must split its rows many ways to fill the chip
// (out_proj of ViT-B/32: 9 tiles x 28 splits) and every split writes a 256-KiB fp32 slab per tile that a reduce launch reads back
// (66 MB per wgrad; at per-GPU batch 512 the slab round trip and the reduce launches are a quarter of the wgrad time); together the
// four have 108 tiles, split 2 ways.  A work item is (problem, split, tile); items are dealt to the XCDs in contiguous runs as above.
#define TN_GROUP_MAX 4
struct TnProblem {
    const bf16_t* DY;
    const bf16_t* X;
    float* dw;
    float* slabs;
    float* cs_part;
    int N, K, tiles_n, tiles_k;
    int work0;          // first work item of this problem
    float beta;
};
struct TnGroup {
    TnProblem p[TN_GROUP_MAX];
    int nprob, M, splits, rows_per_split, total;
};
__global__ __launch_bounds__(512, 2) void gemm_bf16_tn_ppg_kernel(TnGroup grp_args) {
    const int per_xcd = gridDim.x >> 3;
    const int work = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (work >= grp_args.total) return;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < TN_GROUP_MAX; ++i)
        if (i < grp_args.nprob && work >= grp_args.p[i].work0) pi = i;
    const TnProblem& pr = grp_args.p[pi];
    tn_pp_body(grp_args.M, pr.N, pr.K, pr.DY, pr.X, pr.dw, pr.beta, pr.slabs, pr.tiles_n, pr.tiles_k, grp_args.splits,
               grp_args.rows_per_split, pr.cs_part, work - pr.work0);
}
#undef TN_ADDR
#undef TN_ISSUE
#undef TNP_ADDR
#undef TNP_ISSUE
#undef TN_WAIT1
#undef TN_WAIT5
#undef TN_FRAG
#undef TN_GROUP

// dst[i] = beta * dst[i] + sum_k src[k * n + i]; blocks [0, grid1) fold the weight-gradient slabs, blocks [grid1, ...) the
// bias-gradient partials of the same wgrad (one launch for both)
__device__ __forceinline__ void slab_reduce_job(long n, int splits, const float* __restrict__ slabs, float* __restrict__ dw,
                                                float beta, long first, long stride) {
    const long n4 = n >> 2;
    for (long i = first; i < n4; i += stride) {
        float4 s = load4(slabs + 4 * i);
        for (int k = 1; k < splits; ++k) {
            const float4 v = load4(slabs + (long)k * n + 4 * i);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        if (beta != 0.f) {
            const float4 o = load4(dw + 4 * i);
            s.x += beta * o.x; s.y += beta * o.y; s.z += beta * o.z; s.w += beta * o.w;
        }
        store4(dw + 4 * i, s);
    }
}
__global__ __launch_bounds__(256) void slab_reduce_kernel(long n, int splits, const float* __restrict__ slabs,
                                                          float* __restrict__ dw, float beta, int grid1, long n2, int splits2,
                                                          const float* __restrict__ src2, float* __restrict__ dst2,
                                                          float beta2) {
    if ((int)blockIdx.x < grid1)
        slab_reduce_job(n, splits, slabs, dw, beta, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)grid1 * blockDim.x);
    else
        slab_reduce_job(n2, splits2, src2, dst2, beta2, (long)(blockIdx.x - grid1) * blockDim.x + threadIdx.x,
                        (long)(gridDim.x - grid1) * blockDim.x);
}

// the reduce jobs of a grouped wgrad (slabs -> dw and bias partials -> db of every problem) in ONE launch: job j owns the blocks
// [block0[j], block0[j + 1])
#define TN_REDUCE_JOBS 8
struct TnReduceJobs {
    const float* src[TN_REDUCE_JOBS];
    float* dst[TN_REDUCE_JOBS];
    long n[TN_REDUCE_JOBS];
    int splits[TN_REDUCE_JOBS];
    float beta[TN_REDUCE_JOBS];
    int block0[TN_REDUCE_JOBS + 1];
    int njobs;
};
__global__ __launch_bounds__(256) void slab_reduce_group_kernel(TnReduceJobs jobs) {
    int j = 0;
#pragma unroll
    for (int i = 1; i < TN_REDUCE_JOBS; ++i)
        if (i < jobs.njobs && (int)blockIdx.x >= jobs.block0[i]) j = i;
    const int nb = jobs.block0[j + 1] - jobs.block0[j];
    slab_reduce_job(jobs.n[j], jobs.splits[j], jobs.src[j], jobs.dst[j], jobs.beta[j],
                    (long)((int)blockIdx.x - jobs.block0[j]) * blockDim.x + threadIdx.x, (long)nb * blockDim.x);
}

#ifndef TN_PP_DEFAULT
#define TN_PP_DEFAULT 1
#endif
static int g_tn_pp = -1;      // -1: read CLIPX_TN_PP on first use
extern "C" int clipx_select_tn_pp(int which) {
    g_tn_pp = which < 0 ? -1 : (which ? 1 : 0);
    return 0;
}

static int tn_num_cu() { return clipx_num_cu(true); }

// workspace layout: [colsum partials: max(#CU, tiles) x N floats][split slabs]
static size_t tn_cs_reserve(int N, int K) {
    const int tiles = cdiv(N, TN_BN) * cdiv(K, TN_BK);
    const int rows = tiles > tn_num_cu() ? tiles : tn_num_cu();
    return (((size_t)rows * N * sizeof(float)) + 255) / 256 * 256;
}

static void tn_plan(int M, int N, int K, size_t ws_bytes, int* splits, int* rows_per_split) {
    const int tiles = cdiv(N, TN_BN) * cdiv(K, TN_BK);
    int s = tn_num_cu() / tiles;                // one block per CU: tiles x splits <= #CU
    if (s < 1) s = 1;
    const int max_by_rows = cdiv(M, 4 * TN_BM); // keep >= 4 ring steps (256 rows) per split
    if (s > max_by_rows) s = max_by_rows;
    const size_t slab = (size_t)N * K * sizeof(float);
    if (s > 1 && (size_t)s * slab > ws_bytes) s = (int)(ws_bytes / slab);
    if (s < 1) s = 1;
    int rps = cdiv(cdiv(M, s), TN_BM) * TN_BM;
    if (rps < TN_BM) rps = TN_BM;
    s = cdiv(M, rps);
    if (s < 1) s = 1;
    *splits = s;
    *rows_per_split = rps;
}

size_t gemm_bf16_tn_ws_bytes(int M, int N, int K) {
    int s, rps;
    tn_plan(M, N, K, (size_t)-1, &s, &rps);
    return tn_cs_reserve(N, K) + (s > 1 ? (size_t)s * N * K * sizeof(float) : 0);
}

int launch_gemm_bf16_tn(int M, int N, int K, const bf16_t* DY, const bf16_t* X, float* dw, float beta, float* db,
                        float beta_b, void* ws, size_t ws_bytes, hipStream_t stream) {
    CLIPX_CHECK(K % 8 == 0 && N % 8 == 0, "bf16 TN GEMM needs N,K %% 8 == 0 (N=%d K=%d)", N, K);
    CLIPX_CHECK(((uintptr_t)DY % 16 == 0) && ((uintptr_t)X % 16 == 0) && ((uintptr_t)dw % 16 == 0),
                "bf16 TN GEMM: operands must be 16-B aligned");
    const size_t reserve = tn_cs_reserve(N, K);
    const bool have_cs = ws != nullptr && ws_bytes >= reserve;
    CLIPX_CHECK(db == nullptr || have_cs, "bf16 TN GEMM: bias gradient needs %zu bytes of workspace", reserve);
    CLIPX_CHECK(ws == nullptr || (uintptr_t)ws % 256 == 0, "bf16 TN GEMM: workspace must be 256-B aligned");
    float* cs_part = db ? (float*)ws : nullptr;
    float* slab_ws = have_cs ? (float*)((char*)ws + reserve) : nullptr;
    int splits, rps;
    tn_plan(M, N, K, have_cs ? ws_bytes - reserve : 0, &splits, &rps);
    const int tiles_n = cdiv(N, TN_BN), tiles_k = cdiv(K, TN_BK);
    const size_t lds = TN_SLOTS * TN_SLOT_BYTES;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)gemm_bf16_tn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_done = true;
    }
    const int grid = (tiles_n * tiles_k * splits + 7) / 8 * 8;
    // ping-pong form: needs the descriptor loader (32-bit offsets) for every split
    if (g_tn_pp < 0) { const char* e = getenv("CLIPX_TN_PP"); g_tn_pp = (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : TN_PP_DEFAULT; }
    const bool pp = g_tn_pp == 1 && (N % TN_BN) == 0 && (K % TN_BK) == 0 && (long)rps * (N > K ? N : K) * 2 < (1l << 31);
    if (pp) {
        static bool attr_pp = false;
        if (!attr_pp) {
            (void)hipFuncSetAttribute((const void*)gemm_bf16_tn_pp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TNP_LDS);
            attr_pp = true;
        }
        hipLaunchKernelGGL(gemm_bf16_tn_pp_kernel, dim3(grid), dim3(512), TNP_LDS, stream, M, N, K, DY, X, dw, beta, slab_ws,
                           tiles_n, tiles_k, splits, rps, cs_part);
    } else {
        hipLaunchKernelGGL(gemm_bf16_tn_kernel, dim3(grid), dim3(512), lds, stream, M, N, K, DY, X, dw,
                           beta, slab_ws, tiles_n, tiles_k, splits, rps, cs_part);
    }
    {
        const long n = (long)N * K;
        int grid1 = 0;
        if (splits > 1) {
            grid1 = (int)((n / 4 + 255) / 256);
            if (grid1 > 2048) grid1 = 2048;
        }
        const int grid2 = db ? cdiv(N / 4, 256) : 0;
        if (grid1 + grid2 > 0)
            hipLaunchKernelGGL(slab_reduce_kernel, dim3(grid1 + grid2), dim3(256), 0, stream, n, splits, (const float*)slab_ws,
                               dw, beta, grid1, (long)N, splits * tiles_k, (const float*)cs_part, db, beta_b);
    }
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Grouped wgrad: nprob <= TN_GROUP_MAX problems over the same M rows as ONE grid (gemm_bf16_tn_ppg_kernel).
// Workspace layout: per problem [column-sum partials: splits * tiles_k rows x N floats][splits slabs of N x K floats when
// splits > 1], each piece 256-byte aligned.  Applies when every problem meets the ping-pong kernel's conditions (N, K multiples
// of 256, 32-bit row offsets); otherwise (return 1) the caller launches the problems one by one.
static bool tn_group_plan(int M, int nprob, const int* N, const int* K, int* splits, int* rps, int* total_tiles) {
    int tiles = 0;
    for (int i = 0; i < nprob; ++i) {
        if (N[i] % TN_BN != 0 || K[i] % TN_BK != 0) return false;
        tiles += (N[i] / TN_BN) * (K[i] / TN_BK);
    }
    if (tiles <= 0) return false;
    // Row split: every block reduces r rows of one 256 x 256 tile; tiles * s blocks run in ceil(tiles * s / CUs) rounds of one
    // block per CU.  One round (s = CUs / tiles) leaves CUs idle when tiles does not divide the chip (a ViT-B/32 vision block:
    // 108 tiles -> 216 blocks on 256 CUs), several rounds fill it (s = 7: 756 blocks = 2.95 rounds) at the price of s slabs per
    // tile.  The split with the smallest modelled time wins: rounds x (r rows at the kernel's measured rate + one slab store)
    // + the reduce pass over s slabs.  MEASURED (profiles/r03_ablation_wgrad_group.txt, split sweep): ViT-H/14 block (300 tiles) 1412 us
    // at s = 1 -> 1193 us at the modelled s = 5; ViT-B/32 vision block at 204 800 rows 2544 us (s = 2, 216 blocks) vs 2521 us
    // (s = 7, 756 blocks): a partly filled chip clocks higher, so filling it buys nothing there -- the model is never worse.
    const int ncu = tn_num_cu();
    const int max_by_rows = cdiv(M, 4 * TN_BM);
    double weights_bytes = 0.0;
    for (int i = 0; i < nprob; ++i) weights_bytes += 4.0 * N[i] * K[i];
    const double us_per_row = 2.0 * TN_BN * TN_BK / 5.1e6;      // 5.1 TFLOP/s per CU inside the k-loop (profiles/r03 kernel stats)
    const double us_slab = 16.0, us_reduce = weights_bytes / 4.0e6;
    int s = 1;
    double best = 1e30;
    for (int c = 1; c <= max_by_rows && c <= 64; ++c) {
        const int rc = cdiv(cdiv(M, c), TN_BM) * TN_BM;
        if (cdiv(M, rc) != c) continue;
        const int rounds = cdiv(tiles * c, ncu);
        const double t = rounds * (rc * us_per_row + (c > 1 ? us_slab : 0.0)) + (c > 1 ? c * us_reduce : 0.0);
        if (t < best) { best = t; s = c; }
    }
    int r = cdiv(cdiv(M, s), TN_BM) * TN_BM;
    if (r < TN_BM) r = TN_BM;
    s = cdiv(M, r);
    for (int i = 0; i < nprob; ++i)
        if ((long)r * (N[i] > K[i] ? N[i] : K[i]) * 2 >= (1l << 31)) return false;
    *splits = s;
    *rps = r;
    *total_tiles = tiles;
    return true;
}
static size_t tn_align256(size_t b) { return (b + 255) / 256 * 256; }

size_t gemm_bf16_tn_group_ws_bytes(int M, int nprob, const int* N, const int* K) {
    size_t single = 0;
    for (int i = 0; i < nprob; ++i) {
        const size_t b = gemm_bf16_tn_ws_bytes(M, N[i], K[i]);
        if (b > single) single = b;
    }
    int s, r, tiles;
    if (nprob < 1 || nprob > TN_GROUP_MAX || !tn_group_plan(M, nprob, N, K, &s, &r, &tiles)) return single;
    size_t total = 0;
    for (int i = 0; i < nprob; ++i) {
        total += tn_align256((size_t)s * (K[i] / TN_BK) * N[i] * sizeof(float));
        if (s > 1) total += tn_align256((size_t)s * N[i] * K[i] * sizeof(float));
    }
    return total > single ? total : single;
}

int launch_gemm_bf16_tn_group(int M, int nprob, const int* N, const int* K, const bf16_t* const* DY, const bf16_t* const* X,
                              float* const* dw, const float* beta, float* const* db, const float* beta_b, void* ws,
                              size_t ws_bytes, hipStream_t stream) {
    if (nprob < 1 || nprob > TN_GROUP_MAX) return 1;
    if (g_tn_pp < 0) { const char* e = getenv("CLIPX_TN_PP"); g_tn_pp = (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : TN_PP_DEFAULT; }
    int splits, rps, tiles;
    if (g_tn_pp != 1 || !tn_group_plan(M, nprob, N, K, &splits, &rps, &tiles)) return 1;
    if (ws == nullptr || (uintptr_t)ws % 256 != 0 || ws_bytes < gemm_bf16_tn_group_ws_bytes(M, nprob, N, K)) return 1;
    for (int i = 0; i < nprob; ++i)
        if (((uintptr_t)DY[i] % 16) || ((uintptr_t)X[i] % 16) || ((uintptr_t)dw[i] % 16)) return 1;
    TnGroup g;
    g.nprob = nprob;
    g.M = M;
    g.splits = splits;
    g.rows_per_split = rps;
    char* wp = (char*)ws;
    int work0 = 0;
    float* cs_of[TN_GROUP_MAX];
    float* slab_of[TN_GROUP_MAX];
    for (int i = 0; i < TN_GROUP_MAX; ++i) {
        const int j = i < nprob ? i : 0;
        TnProblem& p = g.p[i];
        p.DY = DY[j];
        p.X = X[j];
        p.dw = dw[j];
        p.N = N[j];
        p.K = K[j];
        p.tiles_n = N[j] / TN_BN;
        p.tiles_k = K[j] / TN_BK;
        p.beta = beta[j];
        p.slabs = nullptr;
        p.cs_part = nullptr;
        p.work0 = work0;
        if (i >= nprob) continue;
        const size_t cs_bytes = tn_align256((size_t)splits * p.tiles_k * N[i] * sizeof(float));
        cs_of[i] = (float*)wp;
        p.cs_part = db[i] ? cs_of[i] : nullptr;
        wp += cs_bytes;
        slab_of[i] = nullptr;
        if (splits > 1) {
            slab_of[i] = (float*)wp;
            p.slabs = slab_of[i];
            wp += tn_align256((size_t)splits * N[i] * K[i] * sizeof(float));
        }
        work0 += p.tiles_n * p.tiles_k * splits;
    }
    g.total = work0;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)gemm_bf16_tn_ppg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TNP_LDS);
        attr_done = true;
    }
    const int grid = (g.total + 7) / 8 * 8;
    hipLaunchKernelGGL(gemm_bf16_tn_ppg_kernel, dim3(grid), dim3(512), TNP_LDS, stream, g);
    TnReduceJobs jobs;
    int nj = 0, nblocks = 0;
    for (int i = 0; i < TN_REDUCE_JOBS; ++i) {
        jobs.src[i] = nullptr; jobs.dst[i] = nullptr; jobs.n[i] = 0; jobs.splits[i] = 1; jobs.beta[i] = 0.f; jobs.block0[i] = 0;
    }
    for (int i = 0; i < nprob; ++i) {
        const long n = (long)N[i] * K[i];
        if (splits > 1) {                       // slabs -> dw
            int gridw = (int)((n / 4 + 255) / 256);
            if (gridw > 1024) gridw = 1024;
            jobs.src[nj] = slab_of[i]; jobs.dst[nj] = dw[i]; jobs.n[nj] = n; jobs.splits[nj] = splits; jobs.beta[nj] = beta[i];
            jobs.block0[nj] = nblocks;
            nblocks += gridw;
            ++nj;
        }
        if (db[i]) {                            // bias partials -> db
            jobs.src[nj] = cs_of[i]; jobs.dst[nj] = db[i]; jobs.n[nj] = N[i]; jobs.splits[nj] = splits * (K[i] / TN_BK);
            jobs.beta[nj] = beta_b[i];
            jobs.block0[nj] = nblocks;
            nblocks += cdiv(N[i] / 4, 256);
            ++nj;
        }
    }
    for (int i = nj; i <= TN_REDUCE_JOBS; ++i) jobs.block0[i] = nblocks;
    jobs.njobs = nj;
    if (nj > 0) hipLaunchKernelGGL(slab_reduce_group_kernel, dim3(nblocks), dim3(256), 0, stream, jobs);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
