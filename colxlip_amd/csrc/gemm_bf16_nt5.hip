// NT GEMM, software-pipelined one-wave-per-SIMD variant (full 256x256 tiles, bf16 output):
//     y[M,N] = epi(x[M,K] . w[N,K]^T)
//
// Why a second structure.  In the 8-wave kernel (gemm_bf16_nt.hip) every k-step starts with a barrier after which all
// waves fetch their first fragments from LDS before any MFMA can issue, and a SIMD whose two waves are both stalled has
// nothing to run: the in-kernel profile shows 2048 MFMA cycles inside a ~3500-cycle k-step.  Measured on this chip
// (scripts/ubench_lds.hip): ONE wave issuing v_mfma_f32_16x16x32_bf16 back to back reaches only 65 % of the MFMA rate,
// but one wave issuing v_mfma_f32_32x32x16_bf16 reaches 99 %.  So:
//   * 4 waves (2x2), each owns 128(m) x 128(n) = 4x4 tiles of 32x32, 16 accumulator tuples = all 256 AGPRs, MFMAs as
//     tied inline asm (the register allocator otherwise shuffles accumulators through scratch);
//   * per 64-deep k-step four 16-deep slices of 8 fragment reads + 16 MFMAs; the reads of slice s+1 are issued between
//     the MFMAs of slice s (two fragment sets in registers), ACROSS k-steps as well: the one barrier per k-step sits
//     between slices 2 and 3, where "next k-step's operands have landed" (counted vmcnt) and "all of this k-step's LDS
//     reads are done" hold, so the two slots are refilled there and slice 3's MFMAs cover the next step's first reads.
//     The MFMA stream never waits for LDS after a barrier;
//   * same five-slot 32-KiB LDS-DMA ring across tiles, swizzle, XCD-aware tile order and compile-time specialised
//     epilogue as the 8-wave kernel; stores widened to 16 B with v_permlane32_swap (a lane holds 4 runs of 4 consecutive
//     n of one m; lane l and l+32 hold adjacent runs), operands read in that store layout and un-swapped.
#include <stdlib.h>
#include "gemm_epi.h"
#include "gemm_nt_epilogue.h"

static __device__ __attribute__((aligned(64))) unsigned char g_zero_page[64];
#ifdef NT_PROFILE
__device__ unsigned long long g_n5_dbg[10];
__device__ unsigned long long g_n5_step[16];
extern "C" int clipx_debug_nt5_steps(unsigned long long* out, int reset) {
    if (reset) { unsigned long long z[16] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_n5_step), z, sizeof(z)); }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_n5_step), 16 * sizeof(unsigned long long));
}
extern "C" int clipx_debug_nt5(unsigned long long* out, int reset) {
    if (reset) { unsigned long long z[10] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_n5_dbg), z, sizeof(z)); }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_n5_dbg), 10 * sizeof(unsigned long long));
}
#endif

#define N5_BM 256
#define N5_BN 256
#define N5_BK 64
#define N5_SLOTS 5
#define N5_SLOT_BYTES (256 * 128)
#ifndef N5_PARK
#define N5_PARK 14          // accumulator tuples (of 16) whose stores are deferred into the next tile's k-loop
#endif
#ifndef N5_E2_STRIDE
#define N5_E2_STRIDE 8      // parked item h of a k-step goes out after MFMA 1 + h*N5_E2_STRIDE of slice 2
#endif
#ifndef N5_RD_SPREAD
#define N5_RD_SPREAD 2      // the next slice's 8 fragment reads go out after the first N5_RD_SPREAD MFMAs of a slice
#endif

#include "gemm_nt5_acc.inc"

__device__ __forceinline__ void n5_wait_vmcnt(int n) {
    // wave-uniform n; a smaller immediate than n is always safe
    if (n >= 56) asm volatile("s_waitcnt vmcnt(56)" ::: "memory");
    else if (n >= 40) asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
    else if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// fragment t (0..3 = w tiles, 4..7 = x tiles) of one 16-deep slice; tiles are 32 rows = 4 KiB apart
template <int t>
__device__ __forceinline__ void n5_read(bf16x8& dst, unsigned wa, unsigned xa) {
#ifndef N5_NOREAD
    if constexpr (t < 4)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(wa), "n"(t * 4096));
    else
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(xa), "n"((t - 4) * 4096));
#endif
}
__device__ __forceinline__ void n5_lgkm0(bf16x8 (&f)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]));
}

// bias through the scalar cache: eight consecutive floats at a wave-uniform address into SGPRs.  (A vector load of the
// bias anywhere near the k-loop makes the compiler's waitcnt pass drain the LDS-DMA queue; scalar loads only touch lgkmcnt.)
typedef float f32x8 __attribute__((ext_vector_type(8)));
template <int BYTE_OFF>
__device__ __forceinline__ void n5_sload8(f32x8& d, const float* p) {
    asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(d) : "s"(p), "n"(BYTE_OFF));
}
__device__ __forceinline__ void n5_swait(f32x8& a, f32x8& b, f32x8& c, f32x8& d) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a), "+s"(b), "+s"(c), "+s"(d));
}
template <int N>
__device__ __forceinline__ void n5_wait_vmcnt_imm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// IPS > 0: deferred epilogue (variants without a second operand), IPS parked items stored per k-step of the next tile
template <int FL, int ACT, int IPS>
__global__ __launch_bounds__(256, 1) void gemm_bf16_nt5_kernel(int M, int N, int K, const bf16_t* __restrict__ X,
                                                               const bf16_t* __restrict__ W, EpiB16 epi,
                                                               bf16_t* __restrict__ out, int tiles_m, int tiles_n,
                                                               int total_tiles, int gm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int G = gridDim.x;
    const int nk = (K + N5_BK - 1) / N5_BK;
    const int items_per_tile = 2 * nk;

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

    // ---- load side: 32-KiB items (x rows or w rows of one 64-deep k-step), 32 pieces of 8 rows x 128 B, wave w stages
    // pieces 8w..8w+7; lane -> row l>>3, 16-B slot l&7 holding logical chunk (l&7) ^ (row&7)
    const int srow = lane >> 3;
    const int lchunk = (lane & 7) ^ srow;
    // Loader: buffer_load ... lds with a per-tile scalar descriptor per operand, ONE per-lane byte offset per piece (the
    // same 8 offsets serve x and w: rows (8w+i)*8 + l>>3 of the 256-row item, chunk (l&7)^(row&7)) and the k-step as the
    // scalar offset: issuing a piece costs no vector ALU work, so it can sit between two MFMAs of the only wave on the SIMD.
    // Items alternate x, w, x, w ...; after the 5-item prologue every refill is (w of step s, x of step s+1).
    int Tl = next_valid(blockIdx.x), itl = 0;
    unsigned voff[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) voff[i] = (unsigned)(((8 * wave + i) * 8 + srow) * K + lchunk * 8) * 2u;
    __amdgpu_buffer_rsrc_t rx, rw;
    int kx = 0, kw = 0;                   // byte offset of the next x / w item along K
    auto set_load_tile = [&](int T) {
        int tm, tn;
        coords(T, tm, tn);
        rx = __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long)tm * N5_BM * K), 0, N5_BM * K * 2, 0x00020000);
        rw = __builtin_amdgcn_make_buffer_rsrc((void*)(W + (long)tn * N5_BN * K), 0, N5_BN * K * 2, 0x00020000);
        kx = kw = 0;
    };
    auto piece_w = [&](int slot, int i) {
#ifndef N5_NODMA
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (LDS_PTR(void))(smem + slot * N5_SLOT_BYTES + (8 * wave + i) * 1024), 16,
                                                 voff[i], kw, 0, 0);
#endif
    };
    auto piece_x = [&](int slot, int i) {
#ifndef N5_NODMA
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (LDS_PTR(void))(smem + slot * N5_SLOT_BYTES + (8 * wave + i) * 1024), 16,
                                                 voff[i], kx, 0, 0);
#endif
    };
    auto finish_x = [&]() { kx += N5_BK * 2; ++itl; };
    auto finish_w = [&]() {               // a tile's last item is a w item
        kw += N5_BK * 2;
        if (++itl == items_per_tile) {
            itl = 0;
            Tl = next_valid(Tl + G);
            if (Tl < total_tiles) set_load_tile(Tl);
        }
    };

    int Tc = Tl;
    if (Tc >= total_tiles) return;
    set_load_tile(Tl);
    int inflight = 0, wslot = 0;
#pragma unroll 1
    for (int it = 0; it < N5_SLOTS; ++it)
        if (Tl < total_tiles) {
            if (itl & 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) piece_w(wslot, i);
                finish_w();
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) piece_x(wslot, i);
                finish_x();
            }
            wslot = (wslot + 1 == N5_SLOTS) ? 0 : wslot + 1;
            ++inflight;
        }

    // accumulators: tuple t = 4*i + j (w tile i, x tile j) lives in a[16t : 16t+15], addressed by name (gemm_nt5_acc.inc):
    // D' = W_tile . X_tile^T, lane: m = l&31, n = 8*(r/4) + 4*(l>>5) + r%4
    const unsigned lds0 = (unsigned)(size_t)smem;
    unsigned coff[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) coff[s] = (unsigned)(((2 * s + lh) ^ (l31 & 7)) * 16);
    const unsigned xrow = (unsigned)((wm * 128 + l31) * 128), wrow = (unsigned)((wn * 128 + l31) * 128);
    // stores issued at the end of a tile (all of it, or the tuples the deferred epilogue does not park)
    constexpr int n_stores = ((FL & F_PRE) ? 2 : 1) * (IPS > 0 ? 2 * (16 - N5_PARK) : 32);

    // ---- deferred epilogue.  Measured (scripts/ubench_store.hip, profiles/r01_ablation_gemm_nt.txt): when all 256 CUs
    // reach their epilogues together the stores are one HBM-write burst (5.5 TB/s whatever the lane -> address shape), with
    // every MFMA idle -- ~10k of a K=768 tile's ~69k cycles.  So at the end of a tile the accumulators (+ bias, from SGPRs)
    // are only rounded to bf16 and parked in 128 VGPRs (H); activation, half-wave swaps and stores of that tile then go out
    // IPS tuples per k-step during the NEXT tile's k-loop, between the MFMAs of slice 2, so the write
    // traffic is spread over the whole tile and hidden behind the matrix pipe.  The stored pre-activation is H itself and
    // GELU acts on the bf16-rounded pre-activation, as in the reference's bf16 autocast.
    constexpr bool DEFER = IPS > 0;
    static_assert(!DEFER || (FL & (F_RES | F_ACTU)) == 0, "deferred epilogue: no second operand");
    // Only N5_PARK of the 16 tuples are parked (H + two fragment sets + addresses must fit 256 VGPRs without spilling: a
    // spill reload in the k-loop is a VMEM load, and waiting for it drains the LDS-DMA queue); the rest is stored at once.
    constexpr int NITEM = N5_PARK;                                    // one item per parked tuple
    constexpr int NSTEP = DEFER ? (NITEM + IPS - 1) / IPS : 0;       // k-steps that carry parked items (launcher: nk >= NSTEP)
    constexpr int LAST_ITEMS = DEFER ? NITEM - (NSTEP - 1) * IPS : 0;
    constexpr int SP = (FL & F_PRE) ? 4 : 2;                          // stores per item
    unsigned H[DEFER ? N5_PARK : 1][8];
    bool epi_pend = false;
    long pend_base = 0;            // this lane's element offset of (tile row lane>>2, column 8*(lane&3)) of the parked tile
    // One item = one accumulator tuple (32 rows x 64 B) = two 16-row stores, TRANSPOSED across the wave (at park time, so
    // that an item in the k-loop is two plain stores and never waits for the crossbar): in the MFMA
    // layout neighbouring lanes are neighbouring rows, and such a 16-byte store runs at 13.9 B/clk per CU against 50 B/clk
    // when four neighbouring lanes cover 64 contiguous bytes (scripts/ubench_store.hip); in the k-loop the stores share
    // that address path with the LDS-DMA operand loads.  After the half-wave swap lane (r, lh) holds chunks lh (R0) and
    // 2+lh (R1) of row r; two ds_bpermute per dword (crossbar only) + a select + a quad swap put chunk c of row
    // 16*s + rho into lane 4*rho + c of store s.
    const int t_rho = lane >> 2, t_c = lane & 3;
    const int bp1 = 4 * (16 * (t_c >> 1) + t_rho + 32 * (t_c & 1)), bp2 = bp1 ^ 64;
    const bool t_low = t_c < 2;
    // transposition, issue half: swaps + the eight ds_bpermute of one tuple (results land in X1 / X2 ~100 cycles later)
    auto tr_issue = [&](const unsigned (&x)[8], unsigned (&X1)[4], unsigned (&X2)[4]) {
        const u32x2 p0 = __builtin_amdgcn_permlane32_swap(x[0], x[2], false, false);
        const u32x2 r0 = __builtin_amdgcn_permlane32_swap(x[1], x[3], false, false);
        const u32x2 p1 = __builtin_amdgcn_permlane32_swap(x[4], x[6], false, false);
        const u32x2 r1 = __builtin_amdgcn_permlane32_swap(x[5], x[7], false, false);
        const unsigned R0[4] = {p0[0], r0[0], p0[1], r0[1]}, R1[4] = {p1[0], r1[0], p1[1], r1[1]};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            X1[d] = (unsigned)__builtin_amdgcn_ds_bpermute(bp1, (int)R0[d]);
            X2[d] = (unsigned)__builtin_amdgcn_ds_bpermute(bp2, (int)R1[d]);
        }
    };
    // finish half: h[0..3] = this lane's 16 bytes of store 0 (rows 0..15 of the tuple), h[4..7] = of store 1 (rows 16..31)
    auto tr_finish = [&](const unsigned (&X1)[4], const unsigned (&X2)[4], unsigned (&h)[8]) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            h[d] = t_low ? X1[d] : X2[d];
            const unsigned y = t_low ? X2[d] : X1[d];
            h[4 + d] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)y, 0x4E, 0xF, 0xF, true);      // quad_perm [2,3,0,1]
        }
    };
    // stores of one tuple from the store layout; the activation is elementwise, so it is applied in that layout
    auto epi_emit = [&](auto tc, const unsigned (&h)[8], long base) {
        if constexpr (DEFER) {
            constexpr int t = decltype(tc)::value, i = t >> 2, j = t & 3;
            const long off = base + (long)(32 * j) * N + 32 * i;
            if constexpr ((FL & F_ACT) != 0) {
                unsigned a[8];
#pragma unroll
                for (int sr = 0; sr < 2; ++sr) {
                    float4 v0 = make_float4(bf_lo(h[4 * sr]), bf_hi(h[4 * sr]), bf_lo(h[4 * sr + 1]), bf_hi(h[4 * sr + 1]));
                    float4 v1 = make_float4(bf_lo(h[4 * sr + 2]), bf_hi(h[4 * sr + 2]), bf_lo(h[4 * sr + 3]), bf_hi(h[4 * sr + 3]));
                    act_fwd_quads(ACT, v0, v1);
                    a[4 * sr] = pack2(v0.x, v0.y); a[4 * sr + 1] = pack2(v0.z, v0.w);
                    a[4 * sr + 2] = pack2(v1.x, v1.y); a[4 * sr + 3] = pack2(v1.z, v1.w);
                }
                nt_store16(out + off, (u32x4){a[0], a[1], a[2], a[3]});
                nt_store16(out + off + 16 * (long)N, (u32x4){a[4], a[5], a[6], a[7]});
            } else {
                nt_store16(out + off, (u32x4){h[0], h[1], h[2], h[3]});
                nt_store16(out + off + 16 * (long)N, (u32x4){h[4], h[5], h[6], h[7]});
            }
            if constexpr ((FL & F_PRE) != 0) {
                nt_store16(epi.preact + off, (u32x4){h[0], h[1], h[2], h[3]});
                nt_store16(epi.preact + off + 16 * (long)N, (u32x4){h[4], h[5], h[6], h[7]});
            }
        }
    };
    auto epi_item = [&](auto itc) {
        if constexpr (DEFER) epi_emit(itc, H[decltype(itc)::value], pend_base);
    };

#ifdef NT_PROFILE
    long p_t0 = clock64(), p_vm = 0, p_bar = 0, p_epi = 0, p_steps = 0, p_tiles = 0, p_lg = 0, p_pend = 0, p_npend = 0;
#endif
    bf16x8 FA[8], FB[8];           // two fragment sets: [0..3] w tiles, [4..7] x tiles of one 16-deep slice
    int rslot = 0, ktc = 0, post = 0, slotBp = 0;
    bool pendB = false;

    // prologue: first k-step landed -> its slice-0 fragments
    n5_wait_vmcnt(8 * (inflight - 2));
    __builtin_amdgcn_s_barrier();
    inflight -= 2;
    {
        const int wsl = (rslot + 1 == N5_SLOTS) ? 0 : rslot + 1;
        const unsigned xa = lds0 + rslot * N5_SLOT_BYTES + xrow + coff[0], wa = lds0 + wsl * N5_SLOT_BYTES + wrow + coff[0];
        static_for<0, 8>([&](auto t) { n5_read<decltype(t)::value>(FA[decltype(t)::value], wa, xa); });
    }

#ifdef NT_PROFILE
#define N5_PROF_LGKM_BEGIN const long p_l0 = clock64();
#define N5_PROF_LGKM_END p_lg += clock64() - p_l0;
#else
#define N5_PROF_LGKM_BEGIN
#define N5_PROF_LGKM_END
#endif
#define N5_MFMA0(I, J, S) n5_mfma<4 * (I) + (J), true>(S[I], S[4 + J])
#define N5_MFMA(I, J, S) n5_mfma<4 * (I) + (J), false>(S[I], S[4 + J])
// one 16-deep slice: 16 MFMAs on set CUR, the 8 reads of the following slice into set NXT between the first 8 of them
#define N5_SLICE(CUR, NXT, WA, XA, MF, HOOK)                                                                             \
    {                                                                                                              \
        N5_PROF_LGKM_BEGIN                                                                                         \
        n5_lgkm0(CUR);                                                                                             \
        N5_PROF_LGKM_END                                                                                           \
        static_for<0, 16>([&](auto q_) {                                                                           \
            constexpr int q = decltype(q_)::value;                                                                 \
            constexpr int j = q >> 2, i = q & 3;                                                                   \
            MF(i, j, CUR);                                                                                         \
            if constexpr (q < N5_RD_SPREAD) {                                                                      \
                static_for<0, 8 / N5_RD_SPREAD>([&](auto r_) {                                                     \
                    constexpr int r = q * (8 / N5_RD_SPREAD) + decltype(r_)::value;                                \
                    n5_read<r>(NXT[r], WA, XA);                                                                    \
                });                                                                                                \
            }                                                                                                      \
            HOOK(q)                                                                                                \
        });                                                                                                        \
    }

    while (true) {
        const int wsl = (rslot + 1 == N5_SLOTS) ? 0 : rslot + 1;
        const unsigned xb = lds0 + rslot * N5_SLOT_BYTES + xrow, wb = lds0 + wsl * N5_SLOT_BYTES + wrow;
#ifdef NT_PROFILE
        const long p_s0 = clock64();
        const bool p_was_pend = epi_pend;
#endif
        __builtin_amdgcn_sched_barrier(0);
        // slices 0..2: MFMAs of slice s, reads of slice s+1 of the same k-step.  The x item of the refill decided at the
        // previous mid-step goes out here, one LDS-DMA piece every 4th MFMA of slices 0 and 1: the texture path takes
        // ~16 cycles per 1-KiB piece, and 16 pieces behind consecutive MFMAs backed up its queue and stalled the wave.
#define N5_NOHOOK(q)
#define N5_HOOK_B0(q) if constexpr ((q & 3) == 3) { if (pendB) piece_x(slotBp, q >> 2); }
#define N5_HOOK_B1(q) if constexpr ((q & 3) == 3) { if (pendB) piece_x(slotBp, 4 + (q >> 2)); }
// parked item h of this k-step (item ktc*IPS + h).  The four waves take turns (wave w after MFMA 4w+1 for
// item 0, after MFMA 4((w+2)&3)+3 for item 1): the CU's store path moves ~50 B/clk, and four waves storing 1 KiB each
// at the same MFMA slot queued behind each other for ~120 cycles per store (in-kernel profile).
#define N5_HOOK_E2(q)                                                                                                  \
    if constexpr (DEFER && (q & 1) == 1 && ((q & 3) == 1 || IPS == 2)) {                                               \
        constexpr int h_ = ((q & 3) == 1) ? 0 : 1;                                                                     \
        constexpr int w_ = (h_ == 0) ? (q >> 2) : (((q >> 2) + 2) & 3);                                                \
        if (epi_pend && wave == w_) {                                                                                  \
            static_for<0, NSTEP>([&](auto c_) {                                                                        \
                constexpr int it = decltype(c_)::value * IPS + h_;                                                     \
                if constexpr (it < NITEM) {                                                                            \
                    if (ktc == decltype(c_)::value) epi_item(std::integral_constant<int, it>{});                       \
                }                                                                                                      \
            });                                                                                                        \
        }                                                                                                              \
    }
        // The parked stores go out in slice 0 (N5_ITEMS_LATE: slice 2): the NEXT k-step's counted wait needs them complete
        // (they are older than its loads), and a write acknowledgement takes longer than a load under HBM write pressure --
        // issued first they have 1.75 k-steps instead of 1.25 (measured: K >= 1536 shapes +2-2.6 %, K = 512 / 768 unchanged).
        // Not for the variants with an activation: with the GELU code in slice 0 the register allocator runs out and
        // spills into the accumulator AGPRs (caught by tests/test_isa_guards.py).
#ifndef N5_ITEMS_LATE
#define N5_HOOK_B0E(q) N5_HOOK_B0(q) if constexpr ((FL & F_ACT) == 0) { N5_HOOK_E2(q) }
#define N5_HOOK_E2L(q) if constexpr ((FL & F_ACT) != 0) { N5_HOOK_E2(q) }
#else
#define N5_HOOK_B0E(q) N5_HOOK_B0(q)
#define N5_HOOK_E2L(q) N5_HOOK_E2(q)
#endif
        if (ktc == 0) {
            N5_SLICE(FA, FB, wb + coff[1], xb + coff[1], N5_MFMA0, N5_HOOK_B0E)
        } else {
            N5_SLICE(FA, FB, wb + coff[1], xb + coff[1], N5_MFMA, N5_HOOK_B0E)
        }
        N5_SLICE(FB, FA, wb + coff[2], xb + coff[2], N5_MFMA, N5_HOOK_B1)
        if (pendB) {
            finish_x();
            ++inflight;
            pendB = false;
        }
        N5_SLICE(FA, FB, wb + coff[3], xb + coff[3], N5_MFMA, N5_HOOK_E2L)
        // ---- middle of the k-step: slice 3's fragments are in registers (all of this step's LDS reads are complete), the
        // next k-step's two items have landed once only the younger item (+ the last epilogue's stores) is in flight
        {
            N5_PROF_LGKM_BEGIN
            n5_lgkm0(FB);
            N5_PROF_LGKM_END
        }
        const bool more = inflight >= 2;          // block-uniform: another k-step (this tile's or the next tile's) exists
#ifdef NT_PROFILE
        const long p_a = clock64();
#endif
        // parked-tile stores issued in slice 2 are younger than everything the wait needs
        int S = 0;
        if constexpr (DEFER) {
            if (epi_pend) S = (ktc == NSTEP - 1 ? LAST_ITEMS : IPS) * SP;
        }
        if (inflight == 3 && post == 0) {                                                      // steady state
            if constexpr (DEFER) {
                if (S == 0) n5_wait_vmcnt_imm<8>();
                else if (S == IPS * SP) n5_wait_vmcnt_imm<8 + IPS * SP>();
                else n5_wait_vmcnt_imm<8 + LAST_ITEMS * SP>();
            } else {
                n5_wait_vmcnt_imm<8>();
            }
        } else if (more) {
            n5_wait_vmcnt(8 * (inflight - 2) + S + (post > 0 ? n_stores : 0));
        }
#ifdef NT_PROFILE
        const long p_b = clock64();
#endif
        __builtin_amdgcn_s_barrier();
#ifdef NT_PROFILE
        const long p_c = clock64();
        p_vm += p_b - p_a;
        p_bar += p_c - p_b;
        ++p_steps;
#endif
        // refill: the w item goes out between slice 3's MFMAs (every second one), the x item is handed to the next
        // iteration's slices 0-1 (pendB)
        const int slotA = wslot;
        const bool doA = Tl < total_tiles;
        rslot = (rslot + 2 >= N5_SLOTS) ? rslot + 2 - N5_SLOTS : rslot + 2;
        if (more) inflight -= 2;
        if (post > 0) --post;
        {
            // slice 3 of this k-step; its reads are slice 0 of the NEXT k-step (the slots just proven landed)
            const int wsl2 = (rslot + 1 == N5_SLOTS) ? 0 : rslot + 1;
            const unsigned xn = lds0 + rslot * N5_SLOT_BYTES + xrow + coff[0], wn2 = lds0 + wsl2 * N5_SLOT_BYTES + wrow + coff[0];
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 16>([&](auto q_) {
                constexpr int q = decltype(q_)::value;
                constexpr int j = q >> 2, i = q & 3;
                N5_MFMA(i, j, FB);
                if constexpr (q < N5_RD_SPREAD) {
                    static_for<0, 8 / N5_RD_SPREAD>([&](auto r_) {
                        constexpr int r = q * (8 / N5_RD_SPREAD) + decltype(r_)::value;
                        n5_read<r>(FA[r], wn2, xn);
                    });
                }
                if constexpr ((q & 1) == 1) {
                    if (doA) piece_w(slotA, q >> 1);
                }
            });
            if (doA) {
                finish_w();
                ++inflight;
                wslot = (slotA + 1 == N5_SLOTS) ? 0 : slotA + 1;
                pendB = Tl < total_tiles;
                if (pendB) {
                    slotBp = wslot;
                    wslot = (wslot + 1 == N5_SLOTS) ? 0 : wslot + 1;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#ifdef NT_PROFILE
        if (p_was_pend) { p_pend += clock64() - p_s0; ++p_npend; }
        if (tid == 0 && blockIdx.x == 5) g_n5_step[ktc < 15 ? ktc : 15] += clock64() - p_s0;
#endif
        if constexpr (DEFER) {
            if (ktc + 1 >= NSTEP) epi_pend = false;
        }
        if (++ktc < nk) continue;

        // ---------------- epilogue of tile Tc
        ktc = 0;
#ifdef NT_PROFILE
        const long p_e0 = clock64();
#endif
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");      // inline-asm MFMAs: let the last ones retire before AGPR reads
        int tm, tn;
        coords(Tc, tm, tn);
        const int m0 = tm * N5_BM + wm * 128 + l31, n0 = tn * N5_BN + wn * 128;
        if constexpr (DEFER) {
            // park: accumulators (+ bias) -> bf16 in H.  Bias of w tile i: 32 floats at a wave-uniform address, through SGPRs.
            const long base_now = (long)(tm * N5_BM + wm * 128 + t_rho) * N + n0 + 8 * t_c;
            const float* bs = nullptr;
            if constexpr ((FL & F_BIAS) != 0) bs = epi.bias + __builtin_amdgcn_readfirstlane(n0);
            // Software-pipelined over the tuples: [read + bias + round tuple t, issue its transposition] then [finish the
            // transposition of tuple t-1 -> H (store layout) or, for the tuples not parked, its stores at once].
            unsigned X1[4], X2[4];
            float bq[4][4];
            static_for<0, 17>([&](auto tc_) {
                constexpr int t = decltype(tc_)::value, i = t >> 2;
                unsigned pk[8];
                if constexpr (t < 16) {
                    if constexpr ((FL & F_BIAS) != 0 && (t & 3) == 0) {
                        f32x8 s0, s1, s2, s3;
                        n5_sload8<128 * i + 0>(s0, bs);
                        n5_sload8<128 * i + 32>(s1, bs);
                        n5_sload8<128 * i + 64>(s2, bs);
                        n5_sload8<128 * i + 96>(s3, bs);
                        n5_swait(s0, s1, s2, s3);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            bq[0][e] = lh ? s0[4 + e] : s0[e];
                            bq[1][e] = lh ? s1[4 + e] : s1[e];
                            bq[2][e] = lh ? s2[4 + e] : s2[e];
                            bq[3][e] = lh ? s3[4 + e] : s3[e];
                        }
                    }
                    static_for<0, 4>([&](auto qc) {
                        constexpr int q = decltype(qc)::value;
                        float v0 = n5_acc_read<t, 4 * q + 0>(), v1 = n5_acc_read<t, 4 * q + 1>();
                        float v2 = n5_acc_read<t, 4 * q + 2>(), v3 = n5_acc_read<t, 4 * q + 3>();
                        if constexpr ((FL & F_BIAS) != 0) {
                            v0 += bq[q][0]; v1 += bq[q][1]; v2 += bq[q][2]; v3 += bq[q][3];
                        }
                        pk[2 * q] = pack2(v0, v1);
                        pk[2 * q + 1] = pack2(v2, v3);
                    });
                }
                if constexpr (t > 0) {
                    constexpr int tp = t - 1;
                    if constexpr (tp < N5_PARK) {
                        tr_finish(X1, X2, H[tp]);
                        // pin the parked values here: the sink pass otherwise moves their computation below the whole block
                        // (their users are in later blocks), the temporaries of every tuple stay live, and H is spilled
                        asm volatile("" : "+v"(H[tp][0]), "+v"(H[tp][1]), "+v"(H[tp][2]), "+v"(H[tp][3]), "+v"(H[tp][4]),
                                     "+v"(H[tp][5]), "+v"(H[tp][6]), "+v"(H[tp][7]));
                    } else {
                        unsigned hnow[8];
                        tr_finish(X1, X2, hnow);
                        epi_emit(std::integral_constant<int, tp>{}, hnow, base_now);
                    }
                }
                if constexpr (t < 16) tr_issue(pk, X1, X2);
                __builtin_amdgcn_sched_barrier(0);
            });
            pend_base = base_now;
            epi_pend = true;
#ifdef NT_PROFILE
            p_epi += clock64() - p_e0;
            ++p_tiles;
#endif
            Tc = next_valid(Tc + G);
            if (Tc >= total_tiles) {
                static_for<0, NITEM>([&](auto itc) { epi_item(itc); });       // nothing left to hide behind: flush
                break;
            }
            post = (N5_PARK < 16 && pendB && inflight == 2) ? 1 : 0;
            continue;
        }
        u32x4 uq[(FL & F_ACTU) ? 16 : 1][2], rq[(FL & F_RES) ? 16 : 1][2];
        if constexpr ((FL & (F_ACTU | F_RES)) != 0) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int i = t & 3, j = t >> 2;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const long so = (long)(m0 + 32 * j) * N + n0 + 32 * i + 16 * pr + 8 * lh;
                    if constexpr ((FL & F_ACTU) != 0) uq[t][pr] = *reinterpret_cast<const u32x4*>(epi.act_u + so);
                    if constexpr ((FL & F_RES) != 0) rq[t][pr] = *reinterpret_cast<const u32x4*>(epi.residual + so);
                }
            }
        }
        static_for<0, 4>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            float4 bia[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                bia[q] = (FL & F_BIAS) ? load4(epi.bias + n0 + 32 * i + 8 * q + 4 * lh) : make_float4(0.f, 0.f, 0.f, 0.f);
            static_for<0, 8>([&](auto jp) {
                constexpr int j = decltype(jp)::value >> 1, pr = decltype(jp)::value & 1;
                {
                    const long so = (long)(m0 + 32 * j) * N + n0 + 32 * i + 16 * pr + 8 * lh;
                    u32x2 ua = {0u, 0u}, ub = {0u, 0u}, ra = {0u, 0u}, rb = {0u, 0u};
                    if constexpr ((FL & F_ACTU) != 0) {
                        const u32x4 qv = uq[4 * j + i][pr];
                        ua = __builtin_amdgcn_permlane32_swap(qv[0], qv[2], false, false);
                        ub = __builtin_amdgcn_permlane32_swap(qv[1], qv[3], false, false);
                    }
                    if constexpr ((FL & F_RES) != 0) {
                        const u32x4 qv = rq[4 * j + i][pr];
                        ra = __builtin_amdgcn_permlane32_swap(qv[0], qv[2], false, false);
                        rb = __builtin_amdgcn_permlane32_swap(qv[1], qv[3], false, false);
                    }
                    float4 v[2], bb[2];
                    constexpr int T = 4 * i + j;
                    v[0] = make_float4(n5_acc_read<T, 8 * pr + 0>(), n5_acc_read<T, 8 * pr + 1>(), n5_acc_read<T, 8 * pr + 2>(),
                                       n5_acc_read<T, 8 * pr + 3>());
                    v[1] = make_float4(n5_acc_read<T, 8 * pr + 4>(), n5_acc_read<T, 8 * pr + 5>(), n5_acc_read<T, 8 * pr + 6>(),
                                       n5_acc_read<T, 8 * pr + 7>());
                    bb[0] = bia[2 * pr];
                    bb[1] = bia[2 * pr + 1];
                    unsigned plo[2], phi[2], ulo[2] = {0u, 0u}, uhi[2] = {0u, 0u};
                    const unsigned ul[2] = {ua[0], ua[1]}, uh[2] = {ub[0], ub[1]}, rl[2] = {ra[0], ra[1]}, rh[2] = {rb[0], rb[1]};
                    epi_math2<FL, ACT>(v, bb, ul, uh, rl, rh, ulo, uhi);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        plo[h] = pack2(v[h].x, v[h].y);
                        phi[h] = pack2(v[h].z, v[h].w);
                    }
                    {
                        const u32x2 a = __builtin_amdgcn_permlane32_swap(plo[0], plo[1], false, false);
                        const u32x2 b = __builtin_amdgcn_permlane32_swap(phi[0], phi[1], false, false);
                        u32x4 qv = {a[0], b[0], a[1], b[1]};
                        nt_store16(out + so, qv);
                    }
                    if constexpr ((FL & F_PRE) != 0) {
                        const u32x2 a = __builtin_amdgcn_permlane32_swap(ulo[0], ulo[1], false, false);
                        const u32x2 b = __builtin_amdgcn_permlane32_swap(uhi[0], uhi[1], false, false);
                        u32x4 qv = {a[0], b[0], a[1], b[1]};
                        nt_store16(epi.preact + so, qv);
                    }
                }
            });
        });
#ifdef NT_PROFILE
        p_epi += clock64() - p_e0;
        ++p_tiles;
#endif
        Tc = next_valid(Tc + G);
        if (Tc >= total_tiles) break;
        // the stores are younger than the two items in flight now and older than the x item that slices 0-1 of the next
        // k-step issue: the next mid-step wait (needs those two items) may leave the stores + that item outstanding
        post = (pendB && inflight == 2) ? 1 : 0;
    }
#undef N5_NOHOOK
#undef N5_HOOK_B0
#undef N5_HOOK_B1
#undef N5_HOOK_E2
#undef N5_HOOK_B0E
#undef N5_HOOK_E2L
#undef N5_MFMA0
#undef N5_MFMA
#undef N5_SLICE
#ifdef NT_PROFILE
    if (tid == 0) {
        atomicAdd(&g_n5_dbg[0], (unsigned long long)(clock64() - p_t0));
        atomicAdd(&g_n5_dbg[1], (unsigned long long)p_vm);
        atomicAdd(&g_n5_dbg[2], (unsigned long long)p_bar);
        atomicAdd(&g_n5_dbg[3], (unsigned long long)p_epi);
        atomicAdd(&g_n5_dbg[4], (unsigned long long)p_steps);
        atomicAdd(&g_n5_dbg[5], (unsigned long long)p_tiles);
        atomicAdd(&g_n5_dbg[6], (unsigned long long)p_lg);
        atomicAdd(&g_n5_dbg[7], (unsigned long long)p_pend);
        atomicAdd(&g_n5_dbg[8], (unsigned long long)p_npend);
    }
#endif
}

template <int FL, int ACT, int IPS>
static int launch_one(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, bf16_t* out, int n_cu,
                      hipStream_t stream) {
    const int tiles_m = M / N5_BM, tiles_n = N / N5_BN;
    const int gm = nt_pick_gm(N, K, tiles_m);
    const int total = (((tiles_m + 7) / 8 + gm - 1) / gm) * gm * 8 * tiles_n;
    const int grid = total < n_cu ? total : n_cu;     // multiple of 8 either way
    const size_t lds = N5_SLOTS * N5_SLOT_BYTES;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)gemm_bf16_nt5_kernel<FL, ACT, IPS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_done = true;
    }
    hipLaunchKernelGGL((gemm_bf16_nt5_kernel<FL, ACT, IPS>), dim3(grid), dim3(256), lds, stream, M, N, K, X, W, epi, out,
                       tiles_m, tiles_n, total, gm);
    CLIPX_LAUNCH_CHECK();
    return 0;
}

// returns 1 when this variant does not apply (partial tiles, epilogue combination not built): caller uses the 8-wave kernel
int launch_gemm_bf16_nt5(int M, int N, int K, const bf16_t* X, const bf16_t* W, const EpiB16& epi, bf16_t* out, int n_cu,
                         hipStream_t stream) {
    if (M % N5_BM != 0 || N % N5_BN != 0 || K % N5_BK != 0) return 1;
    if (epi.pre8 || epi.actu8 || epi.ms_max) return 1;     // epilogues this kernel does not build
    int fl, act;
    if (!nt_epi_flags(epi, fl, act)) return 1;
    const int nk = K / N5_BK;
#define N5_CASE(FLV, ACTV) \
    if (fl == (FLV) && act == (ACTV)) return launch_one<(FLV), (ACTV), 0>(M, N, K, X, W, epi, out, n_cu, stream)
    // deferred epilogue: 1 or 2 parked tuples per k-step so that a tile's N5_PARK fit in the next tile's k-steps
    static int ips0 = -1;      // experiment: CLIPX_NT5_IPS0=1 = no deferred epilogue anywhere (plain stores at the tile end)
    if (ips0 < 0) { const char* e = getenv("CLIPX_NT5_IPS0"); ips0 = (e && e[0] == '1') ? 1 : 0; }
#define N5_CASE_D(FLV, ACTV)                                                                           \
    if (fl == (FLV) && act == (ACTV)) {                                                                \
        if (ips0) return launch_one<(FLV), (ACTV), 0>(M, N, K, X, W, epi, out, n_cu, stream);                   \
        if (nk >= N5_PARK) return launch_one<(FLV), (ACTV), 1>(M, N, K, X, W, epi, out, n_cu, stream);          \
        if (2 * nk >= N5_PARK) return launch_one<(FLV), (ACTV), 2>(M, N, K, X, W, epi, out, n_cu, stream);      \
        return 1;                                                                                      \
    }
    N5_CASE_D(0, CLIPX_ACT_NONE);
    N5_CASE_D(F_BIAS, CLIPX_ACT_NONE);
    N5_CASE(F_BIAS | F_RES, CLIPX_ACT_NONE);
    N5_CASE(F_ACTU, CLIPX_ACT_GELU);
    N5_CASE(F_ACTU, CLIPX_ACT_QUICKGELU);
    N5_CASE_D(F_BIAS | F_ACT | F_PRE, CLIPX_ACT_GELU);
    N5_CASE_D(F_BIAS | F_ACT | F_PRE, CLIPX_ACT_QUICKGELU);
    N5_CASE_D(F_BIAS | F_ACT, CLIPX_ACT_GELU);
    N5_CASE_D(F_BIAS | F_ACT, CLIPX_ACT_QUICKGELU);
#undef N5_CASE
#undef N5_CASE_D
    return 1;
}
