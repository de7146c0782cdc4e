// Performance-mode NT GEMM:  y[M,N] = epi(x[M,K] . w[N,K]^T), bf16 operands, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16.  Serves every forward linear and (with w := the [K,N] weight copy) every dgrad.
//
// Shape of the problem here: M is huge (batch x tokens: 2e5..3e5), N and K are small (512..3072).
//   * 256x256 output tile (128x256 variant for tile-count quantisation), 8 waves (2x4, each 128(m) x 64(n) =
//     8x4 MFMA tiles): 128 FLOP per staged byte.
//   * PERSISTENT blocks (one per CU) walk their tiles; operands stream through a FIVE-slot LDS ring of 32-KiB
//     items (x rows or w rows of one 64-deep k-step: 128-B rows = full cache lines per LDS-DMA request), three
//     items in flight while two are computed on.  The ring runs ACROSS tile boundaries, so a tile's epilogue
//     overlaps the next tile's first loads and there is no per-tile prologue.
//   * waits are COUNTED (s_waitcnt vmcnt(N), N = younger LDS-DMA ops [+ the epilogue's stores, which are younger
//     than the items already in flight]) and the barrier is a raw s_barrier: one barrier per 64-deep K-step.
//   * LDS image is lane-linear (what LDS-DMA writes); the bank swizzle goes on the per-lane SOURCE address:
//     128-B rows, 16-B chunk c of row r stored at c ^ (r & 7)  -> conflict-free ds_read_b128.
//   * D' = W_tile . X_tile^T, so a lane owns 4 consecutive n of one m; v_permlane16_swap pairs two n-tiles so
//     every store is 16 B per lane (64 contiguous bytes per row per instruction); act_u / residual operands are
//     read in that same store layout and un-swapped (the swap is an involution).
//   * the epilogue is SPECIALISED AT COMPILE TIME (FL = operand flags, ACT = activation kind).  With run-time
//     flags the unrolled epilogue was ~250 KB of branchy code: it missed the 64 KB instruction cache on every tile
//     and cost 11k cycles per tile (in-kernel s_memtime profile, profiles/r01_nt_inkernel_profile.txt) -- as much
//     as 2.7 k-steps -- whether or not any store was issued.
//   * tile order keeps all n-tiles of an m-panel on one XCD (shared L2): x is fetched from HBM once.
// Out-of-range rows are clamped (their outputs are discarded), K tails are fed from a zero page.
#include <stdlib.h>
#include <type_traits>
#include "kernels.h"
#include "gemm_epi.h"
#include "gemm_nt_epilogue.h"

static __device__ __attribute__((aligned(64))) unsigned char g_zero_page[64];

#ifdef NT_PROFILE
// in-kernel cycle accounting per wave (s_memtime, lane 0 of each wave): [0] total [1] epilogue [2] wait+barrier [3] compute [4] tiles
// [5] blocks [6] vmcnt part of the wait.  Read back with clipx_debug_nt (scripts/prof_nt.py).
__device__ unsigned long long g_nt_dbg[64];   // [wave][counter]
extern "C" int clipx_debug_nt(unsigned long long* out, int reset) {
    if (reset) {
        unsigned long long z[64] = {0};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_nt_dbg), z, sizeof(z));
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nt_dbg), 64 * sizeof(unsigned long long));
}
#endif

#ifndef NT_FULL_LINE
#define NT_FULL_LINE 0   // 1: epilogue stores cover whole 128-byte lines per instruction (measured: same FETCH_SIZE, same time)
#endif
#ifndef NT_FAST_LOADER
#define NT_FAST_LOADER 1   // buffer-descriptor LDS-DMA addressing when K % 64 == 0
#endif
#ifndef NT_AHEAD
#define NT_AHEAD 11    // fragment reads in flight ahead of their MFMA group (LGKM counter holds 15); 7 was 6 % slower
#endif
#ifndef NT_PP_DEFAULT
#define NT_PP_DEFAULT 1
#endif
#define NT_BN 256
#define NT_BK 64
#define NT_SLOTS 5                 // ring of operand slots: x(k0) w(k0) x(k1) w(k1) x(k2) ...
#define NT_SLOT_BYTES (256 * 128)  // one operand (256 rows) of one 64-deep k-step: 32 KiB

__device__ __forceinline__ void wait_vmcnt(int n) {
    // n is wave-uniform; s_waitcnt needs an immediate.  A smaller immediate than `n` is always safe.
    if (n >= 36) asm volatile("s_waitcnt vmcnt(36)" ::: "memory");
    else if (n >= 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else if (n >= 18) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    else if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (n >= 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n >= 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- compile-time helpers for the hand-scheduled inner loop
// fragments issued (cumulative) once MFMA group G of a k-step may start: its own fragment index + AHEAD, capped
template <int MT>
constexpr int nt_issued_before(int G, int ahead) {
    const int fs = 4 + MT, nf = 2 * fs;
    const int need = (G / MT) * fs + 4 + (G % MT);
    const int r = need + ahead;
    const int floor0 = 4 + ahead;               // the prologue's count (group 0 needs fragment 4)
    return r > nf ? nf : (r < floor0 ? floor0 : r);
}
// read fragment f of a k-step: slice s = f / FS; r = f % FS: w-tile r (r < 4) or x-tile r - 4; tiles are 2 KiB apart
template <int f, int FS>
__device__ __forceinline__ void nt_frag_read(bf16x8& dst, const unsigned (&wa)[2], const unsigned (&xa)[2]) {
    constexpr int s = f / FS, r = f % FS;
    if constexpr (r < 4)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(wa[s]), "n"(r * 2048));
    else
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(xa[s]), "n"((r - 4) * 2048));
}
#define NT_LGKM_CASE(n) else if constexpr (N == n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(a))
template <int N>
__device__ __forceinline__ void nt_lgkm_wait1(bf16x8& a) {
    static_assert(N >= 0 && N <= 15, "LGKM counter holds 15");
    if constexpr (N == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a));
    NT_LGKM_CASE(1); NT_LGKM_CASE(2); NT_LGKM_CASE(3); NT_LGKM_CASE(4); NT_LGKM_CASE(5); NT_LGKM_CASE(6); NT_LGKM_CASE(7);
    NT_LGKM_CASE(8); NT_LGKM_CASE(9); NT_LGKM_CASE(10); NT_LGKM_CASE(11); NT_LGKM_CASE(12); NT_LGKM_CASE(13);
    NT_LGKM_CASE(14); NT_LGKM_CASE(15);
}
#undef NT_LGKM_CASE
#define NT_LGKM_CASE(n) \
    else if constexpr (N == n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e))
template <int N>
__device__ __forceinline__ void nt_lgkm_wait5(bf16x8& a, bf16x8& b, bf16x8& c, bf16x8& d, bf16x8& e) {
    static_assert(N >= 0 && N <= 15, "LGKM counter holds 15");
    if constexpr (N == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e));
    NT_LGKM_CASE(1); NT_LGKM_CASE(2); NT_LGKM_CASE(3); NT_LGKM_CASE(4); NT_LGKM_CASE(5); NT_LGKM_CASE(6); NT_LGKM_CASE(7);
    NT_LGKM_CASE(8); NT_LGKM_CASE(9); NT_LGKM_CASE(10); NT_LGKM_CASE(11); NT_LGKM_CASE(12); NT_LGKM_CASE(13);
    NT_LGKM_CASE(14); NT_LGKM_CASE(15);
}
#undef NT_LGKM_CASE

template <typename OUT_T, int MT, int FL, int ACT>
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt_kernel(int M, int N, int K, const bf16_t* __restrict__ X,
                                                              const bf16_t* __restrict__ W, EpiB16 epi,
                                                              OUT_T* __restrict__ out, int tiles_m, int tiles_n,
                                                              int total_tiles, int gm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT_BM = 32 * MT;        // 2 wave rows x MT m-tiles of 16
    constexpr int XP = MT / 2;            // LDS-DMA pieces (8 rows each) per wave per x item
    constexpr bool OUT_BF16 = std::is_same<OUT_T, bf16_t>::value;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15;
    const int wm = wave >> 2, wn = wave & 3;
    const int G = gridDim.x;
    const int nk = (K + NT_BK - 1) / NT_BK;
    const int items_per_tile = 2 * nk;

    // tile index -> (tm, tn): T&7 labels the XCD (grid is a multiple of 8), whole m-panels stay on one XCD
    // tile index -> (tm, tn).  T & 7 labels the XCD (the grid is a multiple of 8; blocks are dealt round-robin over the
    // XCDs), so whole m-panels stay on one XCD and the x panel is fetched into that L2 once for all its n-tiles.  Within an
    // XCD the walk goes over blocks of `gm` m-panels: all gm panels against n-tile 0, then against n-tile 1, ...  With
    // gm = 1 the XCD's 32 CUs hold 32 / tiles_n panels against EVERY n-tile at once, i.e. the whole weight matrix is in
    // use all the time -- fine while it fits the 4-MiB L2 beside the panels, but a 4.7-MB weight (ViT-B/32 c_fc / c_proj)
    // is then re-fetched every round (rocprofv3 FETCH_SIZE: 2.3 GB per c_fc forward against 0.32 GB of x).  With gm = 8
    // the 32 CUs hold 8 panels x 4 n-tiles: 1.5 MB of weights in use, each weight tile fetched once per 8 panels.
    auto coords = [&](int T, int& tm, int& tn) {
        const int local = T >> 3;
        const int per = gm * tiles_n;
        const int blk = local / per, r = local - blk * per;
        tn = r / gm;
        tm = (blk * gm + (r - tn * gm)) * 8 + (T & 7);
    };
    auto next_valid = [&](int T) {
        while (T < total_tiles) {
            int tm, tn;
            coords(T, tm, tn);
            if (tm < tiles_m) break;
            T += G;
        }
        return T;
    };

    // ---- load side: a stream of 32-KiB items (x rows or w rows of one 64-deep k-step) through a 5-slot ring.
    // One LDS-DMA piece = 1 KiB = 8 rows x 128 B (full cache lines); lane -> row l>>3, 16-B slot l&7, holding
    // logical chunk (l&7) ^ (row&7).  Wave w stages pieces 4w..4w+3 of every item.
    const int srow = lane >> 3, sslot = lane & 7;
    const int lchunk = sslot ^ srow;
    // the zero page's address comes from the GOT (an s_load + s_waitcnt lgkmcnt(0)): fetch it ONCE -- inside the k-loop that
    // wait would also drain the fragment reads in flight
    const bf16_t* zp = reinterpret_cast<const bf16_t*>(g_zero_page);
    asm volatile("" : "+s"(zp));
    int Tl = next_valid(blockIdx.x), itl = 0, m0l = 0, n0l = 0;
    // FAST LOADER (K a multiple of 64, i.e. every production shape): buffer_load ... lds with one scalar descriptor per operand
    // and tile, ONE per-lane byte offset per piece (rows (np*wave+i)*8 + l>>3 of the item, chunk (l&7)^(row&7): the same for
    // every k-step and tile) and the k-step as the scalar offset.  Issuing a piece is then ~4 scalar instructions + the load; the
    // pointer form below costs ~15 vector instructions per piece (64-bit row * K, clamp, zero-page select), 240 per k-step and
    // SIMD -- about as many issue cycles as the MFMAs leave free.  Rows beyond M / N fall outside the descriptor and read as 0.
    const bool fastk = NT_FAST_LOADER && (K % NT_BK) == 0;
    unsigned voffw[4], voffx[XP];
#pragma unroll
    for (int i = 0; i < 4; ++i) voffw[i] = (unsigned)(((4 * wave + i) * 8 + srow) * K + lchunk * 8) * 2u;
#pragma unroll
    for (int i = 0; i < XP; ++i) voffx[i] = (unsigned)(((XP * wave + i) * 8 + srow) * K + lchunk * 8) * 2u;
    __amdgpu_buffer_rsrc_t rx, rw;
    auto set_load_tile = [&](int T) {
        int tm, tn;
        coords(T, tm, tn);
        m0l = tm * NT_BM;
        n0l = tn * NT_BN;
        if (fastk) {
            const int xr = min(NT_BM, M - m0l), wr = min(NT_BN, N - n0l);
            rx = __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long)m0l * K), 0, xr * K * 2, 0x00020000);
            rw = __builtin_amdgcn_make_buffer_rsrc((void*)(W + (long)n0l * K), 0, wr * K * 2, 0x00020000);
        }
    };
    auto fast_piece = [&](int slot, int i) {        // piece i of the item the load cursor points at
        const int kb = (itl >> 1) * (NT_BK * 2);
        if (itl & 1) {
            lds_dma_piece(rw, smem + slot * NT_SLOT_BYTES + (4 * wave + i) * 1024, voffw[i], kb);
        } else if (i < XP) {
            lds_dma_piece(rx, smem + slot * NT_SLOT_BYTES + (XP * wave + i) * 1024, voffx[i < XP ? i : 0], kb);
        }
    };
    auto issue_item = [&](int slot) {
        char* base = smem + slot * NT_SLOT_BYTES;
        const int k0 = (itl >> 1) * NT_BK + lchunk * 8;
        const bool is_w = itl & 1;
        const bf16_t* src = is_w ? W : X;
        const int r0 = is_w ? n0l : m0l, rmax = (is_w ? N : M) - 1;
        const int np = is_w ? 4 : XP;
        if (fastk) {
#pragma unroll
            for (int i = 0; i < 4; ++i) fast_piece(slot, i);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < np) {
                    int r = r0 + (np * wave + i) * 8 + srow;
                    if (r > rmax) r = rmax;
                    glds16(k0 < K ? src + (long)r * K + k0 : zp, base + (np * wave + i) * 1024);
                }
            }
        }
        if (++itl == items_per_tile) {
            itl = 0;
            Tl = next_valid(Tl + G);
            if (Tl < total_tiles) set_load_tile(Tl);
        }
    };

    int Tc = Tl;
    if (Tc >= total_tiles) return;
    set_load_tile(Tl);
    int inflight = 0, wslot = 0;      // inflight = items issued and not yet consumed
#pragma unroll 1
    for (int i = 0; i < NT_SLOTS; ++i)
        if (Tl < total_tiles) { issue_item(wslot); wslot = (wslot + 1 == NT_SLOTS) ? 0 : wslot + 1; ++inflight; }

    // ---- compute side
    f32x4 acc[4][MT];   // [n-tile][m-tile]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int sw = c & 7;
    const int xoff = (wm * 16 * MT + c) * 128;
    const int woff = (wn * 64 + c) * 128;
    constexpr int n_stores = OUT_BF16 ? ((FL & F_PRE) ? 4 * MT : 2 * MT) : 0;

#ifdef NT_PROFILE
    long p_t0 = clock64(), p_epi = 0, p_wait = 0, p_cmp = 0, p_tiles = 0, p_vm = 0, p_b = 0, p_c = 0;
#endif
    int rslot = 0, ktc = 0, post = 0;
    bool first = true;
    constexpr int FS = 4 + MT, NF = 2 * FS, AHEAD = NT_AHEAD;
    bf16x8 F[NF];
    // one k-step: wait for its two items, barrier, refill the two freed slots, multiply.  (The variants of this schedule that were
    // measured and dropped -- second slice held across the barrier, refill pieces between its MFMAs, waves 4-7 half a k-step
    // behind inside one barrier interval -- are in profiles/r02_ablation_tile_order_stores.txt (4); the half-k-step offset that
    // does pay needs its own ring layout: gemm_nt_pp.h.)
    auto kstep = [&]() {
    #ifdef NT_PROFILE
            long p_a = clock64();
    #endif
            // this k-step's two items have landed once only the younger items' pieces (4 each) [+ the previous
            // epilogue's stores] are still in flight
            {
                // younger items alternate x, w, x ... starting with an x item
                const int ny = inflight - 2;
                wait_vmcnt(((ny + 1) >> 1) * XP + (ny >> 1) * 4 + (post > 0 ? n_stores : 0));
            }
    #ifdef NT_PROFILE
            p_vm += clock64() - p_a;
    #endif
            __builtin_amdgcn_s_barrier();      // everyone's pieces landed; everyone left the previous k-step's slots
    #ifdef NT_PROFILE
            p_b = clock64();
            p_wait += p_b - p_a;
    #endif
            if (!first) {
                // the previous k-step's two slots are free: refill them
    #pragma unroll 1
                for (int i = 0; i < 2; ++i)
                    if (Tl < total_tiles) { issue_item(wslot); wslot = (wslot + 1 == NT_SLOTS) ? 0 : wslot + 1; ++inflight; }
            }
            first = false;
            {
                const int wsl = (rslot + 1 == NT_SLOTS) ? 0 : rslot + 1;
                // Fragment reads and their waits are inline asm, MFMA groups are fenced with sched_barrier: the issue order
                // below is exactly the program order.  Two reasons.  (1) Left alone the scheduler reuses ONE x-fragment
                // register (read, wait lgkmcnt(0), 4 MFMAs, read ...: an LDS round trip per 4 MFMAs).  (2) Whenever the
                // compiler can see these as LDS loads next to LDS-DMA -- or sees a VMEM load anywhere in the loop whose
                // registers it reuses -- it guards them with s_waitcnt vmcnt(0), which drains the operand ring on every
                // k-step; that cost 15-25 % and came and went with unrelated edits to the epilogue.
                // A k-step's NF = 2 x (4 + MT) fragments (slice s: w-tiles 0..3, x-tiles 0..MT-1) are read in order,
                // about 7 reads ahead of their use; MFMA group (s, j) = x-tile j against the four w-tiles.
                const unsigned lds0 = (unsigned)(size_t)smem;
                unsigned wa[2], xa[2];
    #pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const unsigned coff = ((ks * 4 + g) ^ sw) * 16;
                    wa[ks] = lds0 + wsl * NT_SLOT_BYTES + woff + coff;
                    xa[ks] = lds0 + rslot * NT_SLOT_BYTES + xoff + coff;
                }
                __builtin_amdgcn_sched_barrier(0);
                auto mfma_group = [&](auto sc, auto jc) {
                    constexpr int s_ = decltype(sc)::value, j_ = decltype(jc)::value;
    #pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[i][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[s_ * FS + i], F[s_ * FS + 4 + j_], acc[i][j_], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                };
                static_for<0, NF>([&](auto fc) {
                    constexpr int f = decltype(fc)::value;
                    if constexpr (f < 4 + AHEAD) nt_frag_read<f, FS>(F[f], wa, xa);      // prologue: group 0's fragments + look-ahead
                });
                static_for<0, 2 * MT>([&](auto gc) {
                    constexpr int G = decltype(gc)::value;
                    constexpr int s_ = G / MT, j_ = G % MT;
                    constexpr int need = s_ * FS + 4 + j_;                    // fragment this group waits for
                    constexpr int r_prev = (G == 0) ? (4 + AHEAD) : nt_issued_before<MT>(G - 1, AHEAD);
                    constexpr int r_now = nt_issued_before<MT>(G, AHEAD);
                    static_for<0, NF>([&](auto fc) {
                        constexpr int f = decltype(fc)::value;
                        if constexpr (f >= r_prev && f < r_now) nt_frag_read<f, FS>(F[f], wa, xa);
                    });
                    if constexpr (j_ == 0)
                        nt_lgkm_wait5<r_now - need - 1>(F[s_ * FS + 0], F[s_ * FS + 1], F[s_ * FS + 2], F[s_ * FS + 3], F[need]);
                    else
                        nt_lgkm_wait1<r_now - need - 1>(F[need]);
                    mfma_group(std::integral_constant<int, s_>{}, std::integral_constant<int, j_>{});
                });
                rslot = (rslot + 2 >= NT_SLOTS) ? rslot + 2 - NT_SLOTS : rslot + 2;
            }
            inflight -= 2;
            if (post > 0) --post;
    #ifdef NT_PROFILE
            p_c = clock64();
            p_cmp += p_c - p_b;
    #endif
    };
    while (true) {
        for (ktc = 0; ktc < nk; ++ktc) kstep();
        // ---------------- epilogue of tile Tc (the next tile's first stages are already in flight)
        ktc = 0;
        int tm, tn;
        coords(Tc, tm, tn);
        const int m0 = tm * NT_BM, n0 = tn * NT_BN;
        const bool widened = nt_tile_epilogue<OUT_T, MT, FL, ACT>(acc, epi, out, M, N, m0, n0, wm, wn, lane);
#ifdef NT_PROFILE
        p_epi += clock64() - p_c;
        ++p_tiles;
#endif
        Tc = next_valid(Tc + G);
        if (Tc >= total_tiles) break;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // the widened epilogue issued exactly n_stores stores, all younger than the 3 items in flight now; the
        // next k-step waits for two of those items, so it may leave the stores (and the third item) in flight
        post = (widened && inflight == 3) ? 1 : 0;
    }
#ifdef NT_PROFILE
    if (lane == 0) {
        unsigned long long* g_nt_dbg_w = g_nt_dbg + wave * 8;
        atomicAdd(&g_nt_dbg_w[0], (unsigned long long)(clock64() - p_t0));
        atomicAdd(&g_nt_dbg_w[1], (unsigned long long)p_epi);
        atomicAdd(&g_nt_dbg_w[2], (unsigned long long)p_wait);
        atomicAdd(&g_nt_dbg_w[3], (unsigned long long)p_cmp);
        atomicAdd(&g_nt_dbg_w[4], (unsigned long long)p_tiles);
        atomicAdd(&g_nt_dbg_w[5], 1ull);
        atomicAdd(&g_nt_dbg_w[6], (unsigned long long)p_vm);
    }
#endif
}

template <typename OUT_T, int MT, int FL, int ACT>
static int launch_nt(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, OUT_T* out, int n_cu,
                     hipStream_t stream) {
    constexpr int BM = 32 * MT;
    const int tiles_m = cdiv(M, BM), tiles_n = cdiv(N, NT_BN);
    const int gm = nt_pick_gm(N, K, tiles_m);
    const int total = (((tiles_m + 7) / 8 + gm - 1) / gm) * gm * 8 * tiles_n;
    const int grid = total < n_cu ? total : n_cu;     // multiple of 8 either way
    const size_t lds = NT_SLOTS * NT_SLOT_BYTES;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)gemm_bf16_nt_kernel<OUT_T, MT, FL, ACT>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_done = true;
    }
    hipLaunchKernelGGL((gemm_bf16_nt_kernel<OUT_T, MT, FL, ACT>), dim3(grid), dim3(512), lds, stream, M, N, K, X, W, epi,
                       out, tiles_m, tiles_n, total, gm);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

template <int FL, int ACT>
static int launch_epi(int mt, int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, void* out,
                      int out_dtype, int n_cu, hipStream_t stream) {
    if (out_dtype == CLIPX_BF16) {
        // the all-operands epilogue (kernel tests only) does not fit 256 VGPRs with the 256-row tile: 128-row tile always
        constexpr bool all_ops = (FL & (F_RES | F_ACT | F_PRE)) == (F_RES | F_ACT | F_PRE);
        if (mt == 4 || all_ops) return launch_nt<bf16_t, 4, FL, ACT>(M, N, K, X, W, epi, (bf16_t*)out, n_cu, stream);
        if constexpr (!all_ops) return launch_nt<bf16_t, 8, FL, ACT>(M, N, K, X, W, epi, (bf16_t*)out, n_cu, stream);
    }
    if constexpr ((FL & ~F_BIAS) == 0) {   // fp32 output: only the plain / bias epilogues are built
        if (mt == 4) return launch_nt<float, 4, FL, ACT>(M, N, K, X, W, epi, (float*)out, n_cu, stream);
        return launch_nt<float, 8, FL, ACT>(M, N, K, X, W, epi, (float*)out, n_cu, stream);
    }
    clipx_set_error("bf16 NT GEMM: fp32 output is built only for the plain and bias epilogues (flags %d)", FL);
    return -1;
}

static int g_use5 = -1;      // -1: read CLIPX_NT5 on first use
extern "C" int clipx_select_nt_kernel(int which) {
    g_use5 = which < 0 ? -1 : (which > 2 ? 1 : which);
    return 0;
}

static int g_use_pp = -1;    // -1: read CLIPX_NT_PP on first use
extern "C" int clipx_select_nt_pp(int which) {
    g_use_pp = which < 0 ? -1 : (which > 2 ? 2 : which);
    return 0;
}

int launch_gemm_bf16_nt(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, void* out,
                        int out_dtype, hipStream_t stream) {
    CLIPX_CHECK(K % 8 == 0 && N % 8 == 0, "bf16 NT GEMM needs K %% 8 == 0 and N %% 8 == 0 (K=%d N=%d)", K, N);
    CLIPX_CHECK(((uintptr_t)X % 16 == 0) && ((uintptr_t)W % 16 == 0) && ((uintptr_t)out % 16 == 0),
                "bf16 NT GEMM: operands must be 16-B aligned");
    if (M <= 0 || N <= 0) return 0;
    const int n_cu = clipx_num_cu(true);
    // Tile shape.  The 256x256 tile stages fewest bytes per FLOP (the 128x256 one runs ~0.9x as fast per FLOP).  A
    // partly filled last round of tiles is not worth a smaller tile: the two towers run on separate streams, so the
    // other tower's kernels take the idle CUs (measured at per-GPU batch 512 and 1024: 256x256 everywhere is 4-7 %
    // faster end to end than choosing by rounds).  The small tile is for problems that cannot occupy half the chip.
    const long t256 = (long)cdiv(M, 256) * cdiv(N, NT_BN);
    int mt = (2 * t256 <= n_cu) ? 4 : 8;
    {
        static int force_mt = -1;
        if (force_mt < 0) { const char* e = getenv("CLIPX_NT_MT"); force_mt = e ? atoi(e) : 0; }
        if (force_mt == 4 || force_mt == 8) mt = force_mt;
    }

    // CLIPX_NT_PP = 1: ping-pong kernel (gemm_bf16_nt8p.hip) wherever it applies; 2: only where the pipelined kernel is not
    // chosen; 0: never
    int& use_pp = g_use_pp;
    if (use_pp < 0) { const char* e = getenv("CLIPX_NT_PP"); use_pp = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : NT_PP_DEFAULT; }
    if (use_pp == 1 && mt == 8) {
        const int rc = launch_gemm_bf16_nt8p(M, N, K, X, W, epi, out, out_dtype, n_cu, stream);
        if (rc != 1) return rc;
    }
    {
        // CLIPX_NT5 = 0: eight-wave kernel only; 1: pipelined kernel wherever it applies; 2 (default): pipelined kernel only
        // where it measured faster (tiles of >= 14 k-steps, i.e. one parked tuple per k-step: +2-5 % on those shapes,
        // 706 -> 677 us average NT launch in the train step), eight-wave kernel elsewhere
        if (g_use5 < 0) { const char* e = getenv("CLIPX_NT5"); g_use5 = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 2; }
        if ((g_use5 == 1 || (g_use5 == 2 && K >= 896)) && mt == 8 && out_dtype == CLIPX_BF16) {
            const int rc = launch_gemm_bf16_nt5(M, N, K, X, W, epi, (bf16_t*)out, n_cu, stream);
            if (rc != 1) return rc;
        }
    }
    if (use_pp == 2 && mt == 8) {
        const int rc = launch_gemm_bf16_nt8p(M, N, K, X, W, epi, out, out_dtype, n_cu, stream);
        if (rc != 1) return rc;
    }
    int fl, act;
    CLIPX_CHECK(nt_epi_flags(epi, fl, act), "bf16 NT GEMM: act and act_u are mutually exclusive");
#define NT_CASE(FLV, ACTV) \
    if (fl == (FLV) && act == (ACTV)) return launch_epi<(FLV), (ACTV)>(mt, M, N, K, X, W, epi, out, out_dtype, n_cu, stream)
    NT_EPI_CASES(NT_CASE)
    NT_CASE(F_BIAS | F_ACT | F_PRE | F_RES, CLIPX_ACT_GELU);  // everything at once (kernel tests)
    NT_CASE(F_BIAS | F_ACT | F_PRE | F_RES, CLIPX_ACT_QUICKGELU);
    NT_CASE(F_BIAS | F_PRE | F_RES, CLIPX_ACT_NONE);
#undef NT_CASE
    clipx_set_error("bf16 NT GEMM: epilogue combination not built (flags %d, act %d)", fl, act);
    return -1;
}
