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
#include "gemm_epi.h"      // static_for
#include "pp_probe.h"

static __device__ __attribute__((aligned(64))) unsigned char g_zero_page[64];

#define TN_BN 256          // dy columns (n) per block
#define TN_BK 256          // x columns (k) per block
#define TN_BM 64           // reduction rows per ring item / per barrier
#define TN_SLOTS 5
#define TN_SLOT_BYTES (TN_BM * 512)          // 64 rows x 256 columns: 32 KiB
#define TN_HALF_BYTES (TN_BM * 256)          // one 128-column half of an item

// ---------------------------------------------------------------------------------------------------------------------
// Pieces shared by the two kernels below (one-barrier ring and ping-pong): who a lane is, which rows a block reduces, the
// transposed fragment reads and their waits, the MFMA group, the bias-gradient column sum and the output store.

// wave (wk, wn) of the 2 x 4 grid owns x columns 128 wk.. and dy columns 64 wn..; lane 4q+p of 16-lane group g
struct TnLane {
    int lane, wave, g, c, q, p, wk, wn;
    __device__ __forceinline__ TnLane() {
        lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        g = lane >> 4, c = lane & 15, q = c >> 2, p = c & 3;
        wk = wave >> 2, wn = wave & 3;
    }
};

// work item `work` = split * tiles + tile of one problem (split-major, tile-minor): the output tile and the reduction rows
struct TnWork {
    int split, tk, n0, k0, m_begin, m_end, nsteps;
    __device__ __forceinline__ TnWork(int work, int M, int tiles_n, int tiles_k, int rows_per_split) {
        const int tiles = tiles_n * tiles_k;
        split = work / tiles;
        const int t = work % tiles, tn = t / tiles_k;
        tk = t % tiles_k;
        n0 = tn * TN_BN, k0 = tk * TN_BK;
        m_begin = split * rows_per_split;
        m_end = m_begin + rows_per_split;
        if (m_end > M) m_end = M;
        nsteps = (m_end - m_begin + TN_BM - 1) / TN_BM;
    }
};
// XCD-aware work order: hardware deals blocks to the 8 XCDs round-robin (block b -> XCD b & 7); re-index so that each XCD owns a
// CONTIGUOUS run of the work list.
__device__ __forceinline__ int tn_work_of_block() { return (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3); }

// Transposed-read lane geometry inside a [64 rows][256 B] half item.  A ds_read_b64_tr_b16 of lane 4q+p covers block row q,
// columns 4p..4p+3; read h (0/1) of a fragment takes rows 8g + 4h + q (+32 for the second slice, through the offset: field), whose
// chunk swizzle is (q<<2) | ((2g+h)&3); a 16-column block starts at 16-byte chunk 2*tile (+ p>>1).
struct TnTrLane {
    int sw[2], ro[2];      // per read h: swizzle of its row; byte offset of the row + the 8-byte half of the chunk
    __device__ __forceinline__ TnTrLane(const TnLane& l) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            sw[h] = (l.q << 2) | ((2 * l.g + h) & 3);
            ro[h] = (8 * l.g + 4 * h + l.q) * 256 + (l.p & 1) * 8;
        }
    }
    __device__ __forceinline__ unsigned at(int h, int chunk) const { return ro[h] + ((chunk ^ sw[h]) << 4); }
};

// A step's 24 fragments: f = 12 s + r, slice s = 0/1 (reduction rows 32 s..); r = 0..3: dy n-tile r (B operand), r = 4..11: x k-tile
// r - 4 (A operand); each is two transposed 4-row reads (lo, hi).
struct TnFrags {
    s16x4 lo[24], hi[24];
    __device__ __forceinline__ bf16x8 operator[](int f) const {
        return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo[f], hi[f], 0, 1, 2, 3, 4, 5, 6, 7));
    }
};
// The fragment reads and their waits are inline asm.  Through the intrinsic the compiler puts s_waitcnt vmcnt(0) in front of the
// first LDS read of every step (LDS-DMA may alias it), which drains the whole ring -- including the items issued a moment earlier
// -- and left the one-barrier kernel at 0.57x the NT kernel's rate per step.
// ADDR::at<r>(h): LDS byte address of read h of fragment r of the first slice (one policy per kernel, below).
template <int f, typename ADDR>
__device__ __forceinline__ void tn_frag_read(TnFrags& F, const ADDR& a) {
    constexpr int s = f / 12, r = f % 12;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(F.lo[f]) : "v"(a.template at<r>(0)), "n"(s * 8192));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(F.hi[f]) : "v"(a.template at<r>(1)), "n"(s * 8192));
}
// one-barrier kernel: 12 x 2 per-lane offsets inside a ring slot; the dy and the x item of a step sit in different slots
struct TnRingAddr {
    unsigned foff[12][2], ybs, xbs;
    template <int r> __device__ __forceinline__ unsigned at(int h) const { return (r < 4 ? ybs : xbs) + foff[r][h]; }
};
// ping-pong kernel: the tile index only flips address bits 5..7 (see tn_pp_work), so four bases and one v_xor per read
struct TnPpAddr {
    unsigned yb[2], xb[2];
    template <int r> __device__ __forceinline__ unsigned at(int h) const {
        return r < 4 ? yb[h] ^ (unsigned)(r << 5) : xb[h] ^ (unsigned)((r - 4) << 5);
    }
};
// s_waitcnt lgkmcnt(N) that the compiler believes to redefine fragment f (wait1) / f0..f0+4 (wait5): their users stay behind it
template <int N, int f>
__device__ __forceinline__ void tn_lgkm_wait1(TnFrags& F) {
    static_assert(N >= 0 && N <= 15, "LGKM counter holds 15");
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(F.lo[f]), "+v"(F.hi[f]) : "n"(N));
}
template <int N, int f0>
__device__ __forceinline__ void tn_lgkm_wait5(TnFrags& F) {
    static_assert(N >= 0 && N <= 15, "LGKM counter holds 15");
    asm volatile("s_waitcnt lgkmcnt(%10)"
                 : "+v"(F.lo[f0]), "+v"(F.hi[f0]), "+v"(F.lo[f0 + 1]), "+v"(F.hi[f0 + 1]), "+v"(F.lo[f0 + 2]), "+v"(F.hi[f0 + 2]),
                   "+v"(F.lo[f0 + 3]), "+v"(F.hi[f0 + 3]), "+v"(F.lo[f0 + 4]), "+v"(F.hi[f0 + 4])
                 : "n"(N));
}
// every read issued so far has landed, and every fragment is redefined behind the wait (asm volatile statements keep their
// order: that alone holds the 24 redefinitions, and so every user of a fragment, behind the operand-less wait)
__device__ __forceinline__ void tn_redefine(s16x4& lo, s16x4& hi) { asm volatile("" : "+v"(lo), "+v"(hi)); }
__device__ __forceinline__ void tn_lgkm_wait_all(TnFrags& F) {
    asm volatile("s_waitcnt lgkmcnt(0)");
    static_for<0, 24>([&](auto fc) { tn_redefine(F.lo[decltype(fc)::value], F.hi[decltype(fc)::value]); });
}

// MFMA group (s, i): x k-tile i of slice s against the four dy n-tiles.  acc[k-tile][n-tile]: D[k][n]; a lane owns 4 consecutive
// k of one n.
template <int s, int i>
__device__ __forceinline__ void tn_mfma_group(f32x4 (&acc)[8][4], const TnFrags& F) {
    const bf16x8 a = F[s * 12 + 4 + i];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, F[s * 12 + j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void tn_acc_zero(f32x4 (&acc)[8][4]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// Bias gradient (see the head of the file): this block takes the 32-row slices with index % tiles_k == tk, and the wave pair
// wk = 0 / 1 takes n-tiles 0,1 / 2,3 of them.
struct TnColSum {
    f32x4 cs[2];
    bf16x8 ones;
    float* part;       // [split * tiles_k + tk][N] partials, or null: no bias gradient
    int wait, tiles_k;
    __device__ __forceinline__ TnColSum(float* cs_part, int tk, int tiles_k_) : part(cs_part), wait(tk), tiles_k(tiles_k_) {
        cs[0] = cs[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.0f;
    }
    // after the MFMAs of a step, on its dy fragments
    __device__ __forceinline__ void step(const TnFrags& F, int wk) {
        if (part == nullptr) return;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (wait == 0) {
                cs[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, wk ? F[s * 12 + 2] : F[s * 12 + 0], cs[0], 0, 0, 0);
                cs[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, wk ? F[s * 12 + 3] : F[s * 12 + 1], cs[1], 0, 0, 0);
                wait = tiles_k;
            }
            --wait;
        }
    }
    // every row of the 16 x 16 result holds the column sums: lane group 0 writes its first
    __device__ __forceinline__ void write(const TnWork& w, const TnLane& l, int N) const {
        if (part == nullptr || l.g != 0) return;
        float* row = part + (long)(w.split * tiles_k + w.tk) * N;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int n = w.n0 + l.wn * 64 + 16 * (2 * l.wk + jj) + l.c;
            if (n < N) row[n] = cs[jj][0];
        }
    }
};

// The output tile: dw = acc + beta dw without a row split, slab[split] = acc with one.  CHECK: N and K need not be multiples of
// the tile (the ping-pong kernel only runs when they are).
template <bool CHECK>
__device__ __forceinline__ void tn_store_tile(const f32x4 (&acc)[8][4], const TnWork& w, const TnLane& l, int N, int K, int splits,
                                              float* __restrict__ dw, float beta, float* __restrict__ slabs) {
    float* dst = (splits > 1) ? slabs + (long)w.split * N * K : dw;
    const float b = (splits > 1) ? 0.f : beta;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = w.n0 + l.wn * 64 + 16 * j + l.c;
        if (CHECK && n >= N) continue;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = w.k0 + l.wk * 128 + 16 * i + 4 * l.g;
            if (CHECK && k >= K) continue;
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
// ONE-BARRIER kernel: any N, K (multiples of 8), any split.
__device__ __forceinline__ void tn_wait_vmcnt(int n) {
    if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(512, 2) void gemm_bf16_tn_kernel(int M, int N, int K, const bf16_t* __restrict__ DY,
                                                              const bf16_t* __restrict__ X, float* __restrict__ dw,
                                                              float beta, float* __restrict__ slabs, int tiles_n,
                                                              int tiles_k, int splits, int rows_per_split,
                                                              float* __restrict__ cs_part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TnLane l;
    const int lane = l.lane, wave = l.wave;
    const int work = tn_work_of_block();
    if (work >= tiles_n * tiles_k * splits) return;
    const TnWork w(work, M, tiles_n, tiles_k, rows_per_split);
    const int n0 = w.n0, k0 = w.k0, m_begin = w.m_begin, m_end = w.m_end, nsteps = w.nsteps;
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
    // FAST LOADER (N % 256 == 0 and K % 256 == 0, every production shape): one descriptor per operand covering this block's rows
    // [m_begin, m_end) of its 256-column strip, ONE per-lane byte offset per piece and operand, the 64-row step as the scalar
    // offset; rows beyond m_end fall outside the descriptor and read as zero.  The pointer form costs ~15 vector instructions per piece.
    const bool fast = (N % TN_BN) == 0 && (K % TN_BK) == 0 &&
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

    f32x4 acc[8][4];
    tn_acc_zero(acc);

    // per-lane byte offsets inside a ring slot, fragment r of a slice: dy n-tile r of half wn>>1, tiles 4*(wn&1)+r; x k-tile r-4
    // of half wk
    const TnTrLane tr(l);
    TnRingAddr addr;
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        const int half_base = (r < 4) ? (l.wn >> 1) * TN_HALF_BYTES : l.wk * TN_HALF_BYTES;
        const int tile = (r < 4) ? 4 * (l.wn & 1) + r : r - 4;
#pragma unroll
        for (int h = 0; h < 2; ++h) addr.foff[r][h] = half_base + tr.at(h, 2 * tile + (l.p >> 1));
    }
    const unsigned lds0 = (unsigned)(size_t)smem;

    TnColSum colsum(cs_part, w.tk, tiles_k);

    int inflight = 0, wslot = 0, rslot = 0;
#pragma unroll 1
    for (int i = 0; i < TN_SLOTS; ++i)
        if (it_next < nitems) { issue_item(wslot); wslot = (wslot + 1 == TN_SLOTS) ? 0 : wslot + 1; ++inflight; }

    // A step's 24 fragments are read in order with at most ~7 fragments (14 reads, the LGKM counter holds 15) in flight; MFMA group
    // (s, i) waits for exactly its own x fragment (the first group of a slice also for the four dy fragments).
    TnFrags F;
    auto read = [&](auto fc) { tn_frag_read<decltype(fc)::value>(F, addr); };
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
        addr.ybs = lds0 + rslot * TN_SLOT_BYTES, addr.xbs = lds0 + xsl * TN_SLOT_BYTES;
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 11>(read);
        tn_lgkm_wait5<12, 0>(F);
        tn_mfma_group<0, 0>(acc, F);
        static_for<1, 8>([&](auto ic) {         // six fragments stay in flight behind the one waited for
            constexpr int i = decltype(ic)::value;
            tn_frag_read<10 + i>(F, addr);
            tn_lgkm_wait1<12, 4 + i>(F);
            tn_mfma_group<0, i>(acc, F);
        });
        static_for<18, 23>(read);
        tn_lgkm_wait5<12, 12>(F);
        tn_mfma_group<1, 0>(acc, F);
        tn_frag_read<23>(F, addr);
        tn_lgkm_wait1<12, 17>(F);
        tn_mfma_group<1, 1>(acc, F);
        static_for<2, 8>([&](auto ic) {         // the queue drains: 2 (7 - i) reads behind fragment 16 + i
            constexpr int i = decltype(ic)::value;
            tn_lgkm_wait1<14 - 2 * i, 16 + i>(F);
            tn_mfma_group<1, i>(acc, F);
        });
        colsum.step(F, l.wk);
        rslot = (rslot + 2 >= TN_SLOTS) ? rslot + 2 - TN_SLOTS : rslot + 2;
        inflight -= 2;
    }

    colsum.write(w, l, N);
    tn_store_tile<true>(acc, w, l, N, K, splits, dw, beta, slabs);
}


// ---------------------------------------------------------------------------------------------------------------------
// PING-PONG form of the same kernel (see gemm_nt_pp.h for the scheme and its hazard analysis): a step is an L segment
// (48 transposed fragment reads + 8 LDS-DMA pieces) and a C segment (64 MFMAs) with a barrier after each, and waves 4-7 run one
// segment behind waves 0-3, so on every SIMD one wave multiplies while its partner loads.  Groups split the tile by x columns
// (wk = wave >> 2, as before): the dy rows of a step are SHARED (3 slots x 32 KiB), each group's 128-column half of the x rows
// is PRIVATE (2 slots x 16 KiB per group) and is staged by the OTHER group:
//     A in L_j issues  x_B(j+1) [4 pieces/wave], then its half of dy(j+2) [4];  waits vmcnt(4) at the end of C_j
//     B in L_j issues  x_A(j+2) [4],             then its half of dy(j+2) [4];  waits vmcnt(0) at the end of C_j
// (at the end of the L segment instead, as late as the dependences allow, the waits were measured slower:
// profiles/r02_ablation_pingpong.txt.)
// Needs the buffer-descriptor loader (N, K multiples of 256): rows beyond the split read as zero through the descriptor.
#define TNP_DY_BYTES (TN_BM * 512)      // 32 KiB
#define TNP_X_BYTES (TN_BM * 256)       // 16 KiB: one group's 128 columns
#define TNP_X_BASE (3 * TNP_DY_BYTES)
#define TNP_LDS (3 * TNP_DY_BYTES + 4 * TNP_X_BYTES)

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
struct TnpProbe {
    long t0 = clock64(), last = 0, sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void tick() { last = clock64(); }
    template <int I>
    __device__ __forceinline__ void lap() {
        const long t = clock64();
        if constexpr (I == PP_T_LOOP) sum[I] = t - t0;
        else sum[I] += t - last;
        last = t;
        if constexpr (I == PP_T_VMCNT) ++sum[7];      // one counted wait per step
    }
    __device__ __forceinline__ void flush(int wave, int lane) {
        sum[0] = clock64() - t0;
        if (lane == 0)
            for (int i = 0; i < 8; ++i) atomicAdd(&g_tnp_dbg[wave * 8 + i], (unsigned long long)sum[i]);
    }
};
#else
typedef PpNoProbe TnpProbe;
#endif

// The ping-pong wgrad kernel for ONE work item (`work` = split * tiles + tile) of one problem.
template <typename PROBE>
__device__ __forceinline__ void tn_pp_work(int M, int N, int K, const bf16_t* __restrict__ DY, const bf16_t* __restrict__ X,
                                           float* __restrict__ dw, float beta, float* __restrict__ slabs, int tiles_n, int tiles_k,
                                           int splits, int rows_per_split, float* __restrict__ cs_part, int work) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TnLane l;
    const int lane = l.lane, wave = l.wave, wn = l.wn;
    const int grp = l.wk, og = l.wk ^ 1;        // wk = group
    if (work >= tiles_n * tiles_k * splits) return;
    const TnWork w(work, M, tiles_n, tiles_k, rows_per_split);
    const int rows = w.m_end - w.m_begin, nsteps = w.nsteps;

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
        __builtin_amdgcn_make_buffer_rsrc((void*)(DY + (long)w.m_begin * N + w.n0), 0, ((rows - 1) * N + TN_BN) * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rxx =
        __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long)w.m_begin * K + w.k0), 0, ((rows - 1) * K + TN_BK) * 2, 0x00020000);
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

    f32x4 acc[8][4];
    tn_acc_zero(acc);

    // transposed-read addressing: the x fragments come from the group's own 16-KiB half slot.  Fragment r of a slice sits at chunk
    // (8*(wn&1) | 2*r | p>>1) ^ sw (dy) or (2*(r-4) | p>>1) ^ sw (x): the tile index only flips address bits 5..7, so four base
    // addresses and one v_xor per read replace the 24 per-lane offsets of the kernel above
    const TnTrLane tr(l);
    unsigned ay[2], ax[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        ay[h] = (wn >> 1) * TN_HALF_BYTES + tr.at(h, (8 * (wn & 1)) | (l.p >> 1));
        ax[h] = tr.at(h, l.p >> 1);
    }
    const unsigned lds0 = (unsigned)(size_t)smem;
    const unsigned xring = lds0 + TNP_X_BASE + grp * (2 * TNP_X_BYTES);

    TnColSum colsum(cs_part, w.tk, tiles_k);

    TnFrags F;
    TnPpAddr addr;
    auto read = [&](auto fc) { tn_frag_read<decltype(fc)::value>(F, addr); };
    int yrs = 0, xrs = 0;
    PROBE probe;
#pragma unroll 1
    for (int step = 0; step < nsteps; ++step) {
        // ---- L segment
        probe.tick();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            addr.yb[h] = lds0 + yrs * TNP_DY_BYTES + ay[h];
            addr.xb[h] = xring + xrs * TNP_X_BYTES + ax[h];
        }
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 12>(read);
        __builtin_amdgcn_sched_barrier(0);
        issue_x();
        __builtin_amdgcn_sched_barrier(0);
        static_for<12, 24>(read);
        __builtin_amdgcn_sched_barrier(0);
        const bool yi = issue_dy();
        __builtin_amdgcn_sched_barrier(0);
        probe.template lap<PP_T_L>();
        tn_lgkm_wait_all(F);      // all 24 fragments in registers before the barrier: the slots may be refilled right after it
        __builtin_amdgcn_s_barrier();
        probe.template lap<PP_T_LWAIT>();
        // ---- C segment
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 16>([&](auto gc) { tn_mfma_group<decltype(gc)::value / 8, decltype(gc)::value % 8>(acc, F); });
        colsum.step(F, l.wk);
        probe.template lap<PP_T_C>();
        // what the readers after the coming barrier(s) need from this wave has landed: A leaves its dy pieces (needed two barriers
        // later, waited for at the end of its next C segment) in flight, B nothing
        if (grp == 0 && yi) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        probe.template lap<PP_T_VMCNT>();
        __builtin_amdgcn_s_barrier();
        probe.template lap<PP_T_CBAR>();
        yrs = (yrs == 2) ? 0 : yrs + 1;
        xrs ^= 1;
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();     // the barrier that ends B's last C segment
    probe.template lap<PP_T_LOOP>();

    colsum.write(w, l, N);
    tn_store_tile<false>(acc, w, l, N, K, splits, dw, beta, slabs);
    probe.flush(wave, lane);
}

// One problem: the work item is the block's place in the XCD-aware order.  (Launched as a group of one through the kernel below,
// a single wgrad measured 1-2 % slower at the short residual-block shapes, so the dedicated entry stays.)
__global__ __launch_bounds__(512, 2) void gemm_bf16_tn_pp_kernel(int M, int N, int K, const bf16_t* __restrict__ DY,
                                                                 const bf16_t* __restrict__ X, float* __restrict__ dw,
                                                                 float beta, float* __restrict__ slabs, int tiles_n,
                                                                 int tiles_k, int splits, int rows_per_split,
                                                                 float* __restrict__ cs_part) {
    tn_pp_work<TnpProbe>(M, N, K, DY, X, dw, beta, slabs, tiles_n, tiles_k, splits, rows_per_split, cs_part, tn_work_of_block());
}

// GROUPED launch: up to TN_MAX_PROBLEMS wgrads that reduce over the SAME M rows (the four of a residual block: dW of in_proj, out_proj,
// c_fc, c_proj) as one grid.  Launched one by one, a problem with few output tiles must split its rows many ways to fill the chip
// (out_proj of ViT-B/32: 9 tiles x 28 splits) and every split writes a 256-KiB fp32 slab per tile that a reduce launch reads back
// (66 MB per wgrad; at per-GPU batch 512 the slab round trip and the reduce launches are a quarter of the wgrad time); together the
// four have 108 tiles, split 2 ways.  A work item is (problem, split, tile); items are dealt to the XCDs in contiguous runs as above.
#define TN_MAX_PROBLEMS 4
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
    TnProblem p[TN_MAX_PROBLEMS];
    int nprob, M, splits, rows_per_split, total;
};
__global__ __launch_bounds__(512, 2) void gemm_bf16_tn_ppg_kernel(TnGroup grp_args) {
    const int work = tn_work_of_block();
    if (work >= grp_args.total) return;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < TN_MAX_PROBLEMS; ++i)
        if (i < grp_args.nprob && work >= grp_args.p[i].work0) pi = i;
    const TnProblem& pr = grp_args.p[pi];
    tn_pp_work<TnpProbe>(grp_args.M, pr.N, pr.K, pr.DY, pr.X, pr.dw, pr.beta, pr.slabs, pr.tiles_n, pr.tiles_k, grp_args.splits,
                         grp_args.rows_per_split, pr.cs_part, work - pr.work0);
}

// dst[i] = beta * dst[i] + sum_k src[k * n + i] for the four elements 4i..4i+3 that thread `first` (+ stride ...) owns
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

// the reduce jobs of a wgrad launch (slabs -> dw and bias partials -> db of every problem) in ONE launch: job j owns the blocks
// [block0[j], block0[j + 1]).  A job is 32 bytes, so a block fetches the one it selected with a single scalar load.
#define TN_REDUCE_JOBS (2 * TN_MAX_PROBLEMS)
struct TnReduceJob {
    const float* src;
    float* dst;
    long n;
    int splits;
    float beta;
};
struct TnReduceJobs {
    TnReduceJob job[TN_REDUCE_JOBS];
    int block0[TN_REDUCE_JOBS + 1];
    int njobs;
};
__global__ __launch_bounds__(256) void slab_reduce_group_kernel(TnReduceJobs jobs) {
    int j = 0;
#pragma unroll
    for (int i = 1; i < TN_REDUCE_JOBS; ++i)
        if (i < jobs.njobs && (int)blockIdx.x >= jobs.block0[i]) j = i;
    const TnReduceJob job = jobs.job[j];
    const int nb = jobs.block0[j + 1] - jobs.block0[j];
    // the whole record now: left alone, the compiler fetches n, tests the thread's range, and only then fetches the rest
    asm volatile("" ::"s"(job.src), "s"(job.dst), "s"(job.splits), "s"(job.beta));
    slab_reduce_job(job.n, job.splits, job.src, job.dst, job.beta, (long)((int)blockIdx.x - jobs.block0[j]) * blockDim.x + threadIdx.x,
                    (long)nb * blockDim.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  Both launch paths describe their reduce work as TnReduceJobs (zero-initialised: no jobs, no blocks).
// dst[n] = beta dst + the sum of `splits` consecutive [n] arrays at src, on `blocks` blocks
static void tn_reduce_add(TnReduceJobs& jobs, const float* src, float* dst, long n, int splits, float beta, int blocks) {
    const int j = jobs.njobs++;      // block0[j] is the end of job j - 1; every later entry becomes the end of job j
    jobs.job[j] = TnReduceJob{src, dst, n, splits, beta};
    for (int i = j + 1; i <= TN_REDUCE_JOBS; ++i) jobs.block0[i] = jobs.block0[j] + blocks;
}
static void tn_reduce_launch(const TnReduceJobs& jobs, hipStream_t stream) {
    const int nblocks = jobs.block0[TN_REDUCE_JOBS];
    if (nblocks > 0) hipLaunchKernelGGL(slab_reduce_group_kernel, dim3(nblocks), dim3(256), 0, stream, jobs);
}
// blocks of a slab job (n / 4 float4 elements, 256 per block, at most `cap` blocks) and of a bias job
static int tn_slab_blocks(long n, int cap) {
    const long b = (n / 4 + 255) / 256;
    return b > cap ? cap : (int)b;
}
static int tn_bias_blocks(int N) { return cdiv(N / 4, 256); }

// the kernels take more than the default 64 KiB of dynamic LDS: say so once per kernel
template <auto KERNEL>
static void tn_allow_lds(size_t bytes) {
    static bool done = false;
    if (!done) {
        (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        done = true;
    }
}
#ifndef TN_PP_DEFAULT
#define TN_PP_DEFAULT 1
#endif
static int g_tn_pp = -1;      // -1: read CLIPX_TN_PP on first use
extern "C" int clipx_select_tn_pp(int which) {
    g_tn_pp = which < 0 ? -1 : (which ? 1 : 0);
    return 0;
}
// ping-pong kernel selected (clipx_select_tn_pp, else CLIPX_TN_PP=0/1, else the default)?
static bool tn_pp_selected() {
    if (g_tn_pp < 0) {
        const char* e = getenv("CLIPX_TN_PP");
        g_tn_pp = (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : TN_PP_DEFAULT;
    }
    return g_tn_pp == 1;
}
// the ping-pong kernel's conditions on one problem: the descriptor loader with 32-bit offsets over a split's rows
static bool tn_pp_fits(int rows_per_split, int N, int K) {
    return (N % TN_BN) == 0 && (K % TN_BK) == 0 && (long)rows_per_split * (N > K ? N : K) * 2 < (1l << 31);
}

static int tn_num_cu() { return clipx_num_cu(true); }
static size_t tn_align256(size_t b) { return (b + 255) / 256 * 256; }

// workspace layout: [colsum partials: max(#CU, tiles) x N floats][split slabs]
static size_t tn_cs_reserve(int N, int K) {
    const int tiles = cdiv(N, TN_BN) * cdiv(K, TN_BK);
    const int rows = tiles > tn_num_cu() ? tiles : tn_num_cu();
    return tn_align256((size_t)rows * N * sizeof(float));
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
    const int grid = (tiles_n * tiles_k * splits + 7) / 8 * 8;
    if (tn_pp_selected() && tn_pp_fits(rps, N, K)) {
        tn_allow_lds<gemm_bf16_tn_pp_kernel>(TNP_LDS);
        hipLaunchKernelGGL(gemm_bf16_tn_pp_kernel, dim3(grid), dim3(512), TNP_LDS, stream, M, N, K, DY, X, dw, beta, slab_ws,
                           tiles_n, tiles_k, splits, rps, cs_part);
    } else {
        const size_t lds = TN_SLOTS * TN_SLOT_BYTES;
        tn_allow_lds<gemm_bf16_tn_kernel>(lds);
        hipLaunchKernelGGL(gemm_bf16_tn_kernel, dim3(grid), dim3(512), lds, stream, M, N, K, DY, X, dw,
                           beta, slab_ws, tiles_n, tiles_k, splits, rps, cs_part);
    }
    TnReduceJobs jobs = {};
    if (splits > 1) tn_reduce_add(jobs, slab_ws, dw, (long)N * K, splits, beta, tn_slab_blocks((long)N * K, 2048));
    if (db) tn_reduce_add(jobs, cs_part, db, N, splits * tiles_k, beta_b, tn_bias_blocks(N));
    tn_reduce_launch(jobs, stream);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Grouped wgrad: nprob <= TN_MAX_PROBLEMS problems over the same M rows as ONE grid (gemm_bf16_tn_ppg_kernel).
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
        if (!tn_pp_fits(r, N[i], K[i])) return false;
    *splits = s;
    *rps = r;
    *total_tiles = tiles;
    return true;
}
size_t gemm_bf16_tn_group_ws_bytes(int M, int nprob, const int* N, const int* K) {
    size_t single = 0;
    for (int i = 0; i < nprob; ++i) {
        const size_t b = gemm_bf16_tn_ws_bytes(M, N[i], K[i]);
        if (b > single) single = b;
    }
    int s, r, tiles;
    if (nprob < 1 || nprob > TN_MAX_PROBLEMS || !tn_group_plan(M, nprob, N, K, &s, &r, &tiles)) return single;
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
    if (nprob < 1 || nprob > TN_MAX_PROBLEMS) return 1;
    int splits, rps, tiles;
    if (!tn_pp_selected() || !tn_group_plan(M, nprob, N, K, &splits, &rps, &tiles)) return 1;
    if (ws == nullptr || (uintptr_t)ws % 256 != 0 || ws_bytes < gemm_bf16_tn_group_ws_bytes(M, nprob, N, K)) return 1;
    for (int i = 0; i < nprob; ++i)
        if (((uintptr_t)DY[i] % 16) || ((uintptr_t)X[i] % 16) || ((uintptr_t)dw[i] % 16)) return 1;
    TnGroup g;
    TnReduceJobs jobs = {};
    char* wp = (char*)ws;
    int work0 = 0;
    for (int i = 0; i < nprob; ++i) {
        const int tiles_n = N[i] / TN_BN, tiles_k = K[i] / TN_BK;
        float* cs = (float*)wp;
        wp += tn_align256((size_t)splits * tiles_k * N[i] * sizeof(float));
        float* slabs = nullptr;
        if (splits > 1) {
            slabs = (float*)wp;
            wp += tn_align256((size_t)splits * N[i] * K[i] * sizeof(float));
        }
        g.p[i] = TnProblem{DY[i], X[i], dw[i], slabs, db[i] ? cs : nullptr, N[i], K[i], tiles_n, tiles_k, work0, beta[i]};
        work0 += tiles_n * tiles_k * splits;
        const long n = (long)N[i] * K[i];
        if (splits > 1) tn_reduce_add(jobs, slabs, dw[i], n, splits, beta[i], tn_slab_blocks(n, 1024));
        if (db[i]) tn_reduce_add(jobs, cs, db[i], N[i], splits * tiles_k, beta_b[i], tn_bias_blocks(N[i]));
    }
    for (int i = nprob; i < TN_MAX_PROBLEMS; ++i) {      // unused entries: valid, never selected
        g.p[i] = g.p[0];
        g.p[i].slabs = nullptr;
        g.p[i].cs_part = nullptr;
        g.p[i].work0 = work0;
    }
    g.nprob = nprob;
    g.M = M;
    g.splits = splits;
    g.rows_per_split = rps;
    g.total = work0;
    tn_allow_lds<gemm_bf16_tn_ppg_kernel>(TNP_LDS);
    hipLaunchKernelGGL(gemm_bf16_tn_ppg_kernel, dim3((g.total + 7) / 8 * 8), dim3(512), TNP_LDS, stream, g);
    tn_reduce_launch(jobs, stream);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
