// The eight-wave PING-PONG NT GEMM engine:  acc[256 x 256 tile] = x[M,K] . w[N,K]^T, rows of 128 bytes per k-step.
// One schedule, two kernels: gemm_bf16_nt8p.hip (64 bf16 per k-step) and gemm_fp8_nt8p.hip (128 fp8 per k-step) supply a traits
// struct (element, fragment register type, which 16-byte chunks of a row a lane reads, the C segment's MFMAs) and what happens to
// the accumulators at a tile end; the tile walk, load cursors, prologue, k-step, waits and barriers are here and nowhere else.
//
// Same tile, same LDS image, same loader instruction and the same epilogue as gemm_bf16_nt.hip; what differs is WHEN the two waves
// of a SIMD do what.  There both waves of a SIMD (w and w + 4) leave a barrier together, read their fragments together, issue
// their LDS-DMA pieces together and then compete for the one matrix pipe: a 128-byte-deep k-step costs ~3500-3900 cycles against
// 2048 cycles of MFMA issue.  Here a wave's k-step is two segments separated by barriers,
//     L: 24 fragment reads (the whole k-step: 96 VGPRs) + 8 LDS-DMA pieces        C: the k-step's MFMAs, nothing else
// and waves 4-7 run ONE SEGMENT BEHIND waves 0-3 (one extra barrier before their loop, one extra after the others'), so on
// every SIMD one wave is in C while its partner is in L: the matrix pipe sees one uninterrupted MFMA stream, and the loads /
// reads / waits of the partner happen beside it instead of before it.
//
// Interval 2j: group A (waves 0-3) in L_j, group B (waves 4-7) in C_{j-1};  interval 2j+1: A in C_j, B in L_j.
//
// Tile split between the groups: A owns tile columns 0..127, B columns 128..255 (each wave 128 rows x 64 columns), so the x
// rows of a k-step are SHARED and each group's 128 w rows are PRIVATE to it.  LDS (160 KiB):
//     X  ring: 3 slots x 32 KiB (256 rows x 128 B)     W_A ring: 2 x 16 KiB      W_B ring: 2 x 16 KiB
// A slot may be refilled only after a barrier that follows its last read, and a piece must have landed -- seen by its
// issuing wave's vmcnt wait -- before a barrier that precedes its first read.  The assignment that keeps every piece at
// least two intervals in flight, with 8 pieces per wave and k-step:
//     A in L_j issues   W_B(j+1) [4 pieces/wave]  then its half of X(j+2) [4]
//     B in L_j issues   W_A(j+2) [4]              then its half of X(j+2) [4]
// and the waits sit at the END of the C segment, in front of its barrier (at the end of L they were measured 2.5 % slower: the L
// side of an interval is the longer one):
//     A, end of C_j (interval 2j+1):  s_waitcnt vmcnt(4) -- everything but its X(j+2) pieces has landed: W_B(j+1), which B reads
//        after barrier 2j+3, and its half of X(j+1), which everyone reads after barrier 2j+2
//     B, end of C_j (interval 2j+2):  s_waitcnt vmcnt(0) -- W_A(j+2) and its half of X(j+2), both read after barrier 2j+4
// (A's X(j+2) half is covered by A's next wait, in front of barrier 2j+4.)  Freed slots: X(j-1) was last read in interval 2j-1,
// W_B(j-1) in 2j-1, W_A(j) in 2j -- all before the barrier that precedes the segment overwriting them.  Each group stages the
// OTHER group's w rows: a slot a group reads is then never written in the same interval by a wave that cannot know its
// neighbours' reads are done.
// Tile end: group A runs the epilogue after the barrier that follows its last C segment, group B before it -- both epilogues
// then fall into the same interval (A: epilogue + L_0 of the next tile; B: last C + epilogue).
#pragma once
#include <type_traits>
#include "kernels.h"
#include "gemm_epi.h"
#include "pp_probe.h"      // PpNoProbe, PP_T_*: the cycle-accounting hooks of the kernel body below

#define PP_X_BYTES (256 * 128)      // 32 KiB: 256 x rows of one k-step
#define PP_W_BYTES (128 * 128)      // 16 KiB: one group's 128 w rows
#define PP_W_BASE (3 * PP_X_BYTES)  // W_A ring at 96 KiB, W_B ring at 128 KiB
#define PP_LDS (3 * PP_X_BYTES + 4 * PP_W_BYTES)
#ifndef PP_READS_FIRST
#define PP_READS_FIRST 12     // fragment reads issued before the segment's first LDS-DMA piece (the rest follow the w pieces)
#endif

// fragment f of a k-step: slice s = f / 12; r = f % 12: w-tile r (r < 4) or x-tile r - 4; tiles are 2 KiB apart
template <int f, typename FRAG>
__device__ __forceinline__ void pp_frag_read(FRAG& dst, const unsigned (&wa)[2], const unsigned (&xa)[2]) {
    static_assert(sizeof(FRAG) == 16, "one ds_read_b128");
    constexpr int s = f / 12, r = f % 12;
    if constexpr (r < 4)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(wa[s]), "n"(r * 2048));
    else
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(xa[s]), "n"((r - 4) * 2048));
}

// The kernel body.  T: typedef elem (1 or 2 bytes; a k-step is 128 / sizeof(elem) elements) and frag (16 bytes); chunk(ks, g):
// the 16-byte chunk of a row that lane group g reads into slice ks; mfma<FIRST>(acc, F): the C segment.  tail(acc, m0, n0, wm,
// wn, lane) is called once per tile with the finished accumulators of wave (wm, wn).
//
// Tile walk.  Blocks are dealt to the 8 XCDs round-robin (block b -> XCD b & 7, its rank there b >> 3), and every XCD walks ITS
// OWN m-panels (tm = xcd, xcd + 8, ...) gm panels x all n-tiles at a time, n-tile by n-tile, so the x panel of a tile and the
// weight tiles of a walk block stay in that XCD's L2.  The XCD's tiles are dealt to its blocks round-robin; the last round may
// be partly empty.  (A split-K tail for that round -- its tiles split along K over the idle blocks, fp32 partial tiles folded
// by the last arrival -- was built in round 2 and measured SLOWER wherever it triggered, profiles/r02_ablation_pingpong.txt (8):
// NT layer-pair sum 8.55 -> 8.65 ms, per-GPU batch 512 step 24.5 -> 25.5 ms; removed in round 4.)
template <typename T, typename TAIL, typename PROBE = PpNoProbe>
__device__ __forceinline__ void pp_gemm_nt(int M, int N, int K, const typename T::elem* __restrict__ X,
                                           const typename T::elem* __restrict__ W, int tiles_m, int tiles_n, int gm, TAIL&& tail,
                                           PROBE probe = PROBE()) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MT = 8, NF = 24;
    constexpr int ES = sizeof(typename T::elem);      // bytes per element
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15;
    const int grp = wave >> 2, wq = wave & 3;       // group A / B; wave within the group
    const int wm = wq >> 1, wn = 2 * grp + (wq & 1);
    const int nk = K / (128 / ES);

    // ---- this block's tiles
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3, cpx = gridDim.x >> 3;
    const int P = (tiles_m - xcd + 7) >> 3;                 // m-panels of this XCD
    const int n_x = P * tiles_n;
    const int per = gm * tiles_n;
    auto tile_of = [&](int idx, int& tm, int& tn) {         // idx-th tile of this block = (jb + cpx * idx)-th of the XCD's walk
        const int l = jb + cpx * idx;
        const int blk = l / per, r = l - blk * per;
        const int gmb = min(gm, P - blk * gm);
        tn = r / gmb;
        tm = ((blk * gm + (r - tn * gmb)) << 3) + xcd;
    };
    const int nitems = jb < n_x ? (n_x - jb + cpx - 1) / cpx : 0;
    if (nitems == 0) return;

    // ---- load side.  One piece = 1 KiB = 8 rows x 128 B; lane -> row l>>3, 16-byte slot l&7 holding chunk (l&7)^(row&7).
    const int srow = lane >> 3, lchunk = (lane & 7) ^ srow;
    // ONE per-lane byte offset per operand (piece 0 of this wave); pieces 1..3 are 8, 16, 24 rows further, which goes into the
    // scalar offset of the load together with the k-step
    const unsigned voffx = (unsigned)(((4 * wave) * 8 + srow) * K + lchunk * (16 / ES)) * (unsigned)ES;   // x pieces 4*wave .. 4*wave+3 of 32
    const unsigned voffw = (unsigned)(((4 * wq) * 8 + srow) * K + lchunk * (16 / ES)) * (unsigned)ES;     // pieces 4*wq .. of the OTHER group's 16
    const int piece_stride = 8 * ES * K;                                                   // 8 rows, in bytes
    const int og = grp ^ 1;
    // two cursors through the same tile sequence: x (k-step j+2) and the other group's w (A: j+1, B: j+2)
    int ix = 0, kx = 0, iw = 0, kw = 0;
    __amdgpu_buffer_rsrc_t rx, rw;
    auto set_x_tile = [&](int idx) {
        int tm, tn;
        tile_of(idx, tm, tn);
        const int m0 = tm * 256;
        const int xr = min(256, M - m0);
        rx = __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long)m0 * K), 0, xr * K * ES, 0x00020000);
    };
    auto set_w_tile = [&](int idx) {
        int tm, tn;
        tile_of(idx, tm, tn);
        const int n0 = tn * 256 + og * 128;
        // (clamping both ways selects v_med3_i32, a VALU result: the descriptor then sits in VGPRs and every piece becomes a
        // readfirstlane waterfall loop)
        const int wr = __builtin_amdgcn_readfirstlane(max(0, min(128, N - n0)));
        rw = __builtin_amdgcn_make_buffer_rsrc((void*)(W + (long)min(n0, N - 1) * K), 0, wr * K * ES, 0x00020000);
    };
    int xls = 0, wls = 0;      // slots the cursors write next
    auto issue_x = [&]() -> bool {      // this wave's 4 pieces of the x item at the cursor
        if (ix >= nitems) return false;
        char* dst = smem + xls * PP_X_BYTES + (4 * wave) * 1024;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma_piece(rx, dst + i * 1024, voffx, kx * 128 + i * piece_stride);
        xls = (xls == 2) ? 0 : xls + 1;
        if (++kx == nk) {
            kx = 0;
            if (++ix < nitems) set_x_tile(ix);
        }
        return true;
    };
    auto issue_w = [&]() -> bool {      // this wave's 4 pieces of the OTHER group's w sub-item at the cursor
        if (iw >= nitems) return false;
        char* dst = smem + PP_W_BASE + og * (2 * PP_W_BYTES) + wls * PP_W_BYTES + (4 * wq) * 1024;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma_piece(rw, dst + i * 1024, voffw, kw * 128 + i * piece_stride);
        wls ^= 1;
        if (++kw == nk) {
            kw = 0;
            if (++iw < nitems) set_w_tile(iw);
        }
        return true;
    };

    set_x_tile(0);
    set_w_tile(0);
    // prologue = the issues of the "virtual" segments L_-2, L_-1:  A: X(0) | W_B(0), X(1);   B: W_A(0), X(0) | W_A(1), X(1)
    if (grp == 0) {
        issue_x();
        issue_w();
        issue_x();
    } else {
        issue_w();
        issue_x();
        issue_w();
        issue_x();
    }
    // everything of k-step 0 (and, for B, of k-step 1: its first wait inside the loop comes too late for A's L_1) has landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();     // B runs one segment behind

    f32x4 acc[4][MT];
    typename T::frag F[NF];
    const int sw = c & 7;
    const unsigned lds0 = (unsigned)(size_t)smem;
    const unsigned xoff = lds0 + (wm * 128 + c) * 128;
    const unsigned woff = lds0 + PP_W_BASE + grp * (2 * PP_W_BYTES) + ((wq & 1) * 64 + c) * 128;
    unsigned coff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) coff[ks] = (T::chunk(ks, g) ^ sw) * 16;

    int xrs = 0, wrs = 0;
    // One k-step: L segment, barrier, C segment, the counted wait.  FIRST (the first k-step of a tile) starts the accumulators
    // from zero inside the MFMAs.  Two instantiations, called from a loop that is peeled by hand: with a run-time flag selecting
    // the two MFMA forms inside ONE loop body the register allocator joins 128 accumulators from both and spills ~200 VGPRs.
    auto kstep = [&](auto first_c) {
        // ------------------------------------------------ L segment
        probe.tick();
        int issued = 0;
        {
            unsigned wa[2], xa[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                wa[ks] = woff + wrs * PP_W_BYTES + coff[ks];
                xa[ks] = xoff + xrs * PP_X_BYTES + coff[ks];
            }
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, PP_READS_FIRST>([&](auto fc) { pp_frag_read<decltype(fc)::value>(F[decltype(fc)::value], wa, xa); });
            __builtin_amdgcn_sched_barrier(0);
            if (issue_w()) issued += 4;
            __builtin_amdgcn_sched_barrier(0);
            static_for<PP_READS_FIRST, NF>([&](auto fc) { pp_frag_read<decltype(fc)::value>(F[decltype(fc)::value], wa, xa); });
            __builtin_amdgcn_sched_barrier(0);
            if (issue_x()) issued += 4;
            __builtin_amdgcn_sched_barrier(0);
        }
        probe.template lap<PP_T_L>();
        // all 24 fragments in registers before the barrier: the slots may be refilled right after it
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(F[0]), "+v"(F[1]), "+v"(F[2]), "+v"(F[3]), "+v"(F[4]), "+v"(F[5]), "+v"(F[6]), "+v"(F[7]), "+v"(F[8]),
                       "+v"(F[9]), "+v"(F[10]), "+v"(F[11]), "+v"(F[12]), "+v"(F[13]), "+v"(F[14]), "+v"(F[15]), "+v"(F[16]),
                       "+v"(F[17]), "+v"(F[18]), "+v"(F[19]), "+v"(F[20]), "+v"(F[21]), "+v"(F[22]), "+v"(F[23]));
        __builtin_amdgcn_s_barrier();
        probe.template lap<PP_T_LWAIT>();
        // ------------------------------------------------ C segment
        __builtin_amdgcn_sched_barrier(0);
        T::template mfma<decltype(first_c)::value>(acc, F);
        probe.template lap<PP_T_C>();
        // what the readers after the coming barrier(s) need from this wave has landed: A leaves its x pieces (needed two barriers
        // later, waited for at the end of its next C segment) in flight, B nothing.  (Before a tile's epilogue, so that no store
        // is waited for.)
        if (grp == 0 && issued == 8) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        probe.template lap<PP_T_VMCNT>();
        xrs = (xrs == 2) ? 0 : xrs + 1;
        wrs ^= 1;
    };
    for (int ic = 0;;) {
        kstep(std::true_type{});
        for (int kc = 1; kc != nk; ++kc) {
            probe.tick();
            __builtin_amdgcn_s_barrier();
            probe.template lap<PP_T_CBAR>();
            kstep(std::false_type{});
        }
        // ---------------- end of a tile.  Group A runs the epilogue AFTER the barrier that ends this interval, group B BEFORE it:
        // both then sit in the same interval (A: epilogue + L_0 of the next tile; B: its last C segment + epilogue) instead of
        // each group idling through the other's.  One call site, so one copy of the epilogue code.
        if (grp == 0) __builtin_amdgcn_s_barrier();
        probe.tick();
        int tm, tn;
        tile_of(ic, tm, tn);
        tail(acc, tm * 256, tn * 256, wm, wn, lane);
        probe.template lap<PP_T_EPI>();
        if (grp == 1) __builtin_amdgcn_s_barrier();
        if (++ic >= nitems) break;
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();     // the barrier that ends B's last C segment
    probe.flush(wave, lane);
}

// Launch geometry of both kernels: one block per CU; fewer when XCD 0 (which has the most m-panels) has fewer tiles than CUs.
// KERNEL(M, N, K, X, W, epi, out, tiles_m, tiles_n, gm, extra...)
template <auto KERNEL, typename ELEM, typename OUT_T, typename... EXTRA>
static int pp_launch(int M, int N, int K, const ELEM* X, const ELEM* W, const EpiB16& epi, OUT_T* out, int n_cu, hipStream_t stream,
                     EXTRA... extra) {
    const int tiles_m = cdiv(M, 256), tiles_n = cdiv(N, 256);
    const int gm = nt_pick_gm(N, K, tiles_m);
    const int per_xcd = ((tiles_m + 7) >> 3) * tiles_n;
    const int grid = per_xcd * 8 < n_cu ? per_xcd * 8 : n_cu;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PP_LDS);
        attr_done = true;
    }
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(512), PP_LDS, stream, M, N, K, X, W, epi, out, tiles_m, tiles_n, gm, extra...);
    CLIPX_LAUNCH_CHECK();
    return 0;
}
