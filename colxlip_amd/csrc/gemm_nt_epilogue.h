// Epilogue of one output tile of the eight-wave bf16 NT GEMM kernels (gemm_bf16_nt.hip, gemm_bf16_nt8p.hip): 2 x 4 waves, wave
// (wm, wn) owns rows wm*16*MT .. and columns wn*64 .. of the tile, acc[n-tile][m-tile] in the 16x16x32 accumulator layout.
// Returns true when the tile went through the widened bf16 path, which issues exactly nt_epilogue_stores<...>() stores and
// leaves them in flight (the callers' counted s_waitcnt vmcnt(N) bookkeeping needs that number).
#pragma once
#include "gemm_epi.h"

#ifndef NT_FAST_EPI
#define NT_FAST_EPI 0      // 1: phased plain / bias epilogue (see nt_tile_epilogue); measured: no gain (8.71 vs 8.69 ms layer-pair NT sum)
#endif
#ifndef NT_BIAS_UPFRONT
#define NT_BIAS_UPFRONT 1  // GELU (+ pre-activation) epilogues: all bias loads first, one wait, added into the accumulators in place
#endif
#ifndef NT_FULL_LINE
#define NT_FULL_LINE 0   // 1: epilogue stores cover whole 128-byte lines per instruction (measured: same FETCH_SIZE, same time)
#endif

// The epilogue an EpiB16 asks for, as the kernels' template arguments: fl = operand flags, act = the one activation kind in play
// (act_u's or act's).  false: act and act_u are both set, which no kernel builds.
static inline bool nt_epi_flags(const EpiB16& epi, int& fl, int& act) {
    fl = 0;
    if (epi.bias) fl |= F_BIAS;
    if (epi.residual) fl |= F_RES;
    if (epi.act_u) fl |= F_ACTU;
    if (epi.act != CLIPX_ACT_NONE) fl |= F_ACT;
    if (epi.preact) fl |= F_PRE;
    if (epi.pre8) fl |= F_PRE8;
    if (epi.actu8) fl |= F_ACTU8;
    act = (fl & F_ACTU) ? epi.act_u_kind : ((fl & F_ACT) ? epi.act : CLIPX_ACT_NONE);
    return !((fl & F_ACTU) && (fl & F_ACT));
}
// the (flags, activation) pairs that the one-barrier, the ping-pong and the fp8 kernel all build; CASE(flags, act) is the
// dispatcher's own "if it is this one, launch it"
#define NT_EPI_CASES(CASE)                                                                                       \
    CASE(0, CLIPX_ACT_NONE);                             /* dgrad, patch embedding, projections */               \
    CASE(F_BIAS, CLIPX_ACT_NONE);                        /* in_proj */                                           \
    CASE(F_BIAS | F_RES, CLIPX_ACT_NONE);                /* out_proj, c_proj (+ residual stream) */              \
    CASE(F_ACTU, CLIPX_ACT_GELU);                        /* c_proj dgrad x GELU'(u) */                           \
    CASE(F_ACTU, CLIPX_ACT_QUICKGELU);                                                                           \
    CASE(F_BIAS | F_ACT | F_PRE, CLIPX_ACT_GELU);        /* c_fc (training: keeps the pre-activation) */         \
    CASE(F_BIAS | F_ACT | F_PRE, CLIPX_ACT_QUICKGELU);                                                           \
    CASE(F_BIAS | F_ACT, CLIPX_ACT_GELU);                /* c_fc (no_grad) */                                    \
    CASE(F_BIAS | F_ACT, CLIPX_ACT_QUICKGELU);                                                                   \
    CASE(F_BIAS | F_ACT | F_PRE8, CLIPX_ACT_GELU);       /* c_fc (training): GELU' kept on eight bits (gemm_epi.h) */ \
    CASE(F_ACTU8, CLIPX_ACT_NONE);                       /* c_proj dgrad x the kept factor */

template <typename OUT_T, int MT, int FL>
constexpr int nt_epilogue_stores() {
    return std::is_same<OUT_T, bf16_t>::value ? ((FL & F_PRE) ? 4 * MT : 2 * MT) + ((FL & F_PRE8) ? MT : 0) : 0;
}

// 4 x 4 transpose between the wave's four 16-lane groups g and four registers i: afterwards register d of group g' holds what
// register g' of group d held (two v_permlane32_swap for the high bit, two v_permlane16_swap for the low one; an involution).
// The byte tiles of the 8-bit GELU' travel through it: in the accumulator layout lane (g, c) holds, per n-tile i, the four bytes
// of columns 16 i + 4 g .. + 3 of row c; transposed, group g' holds the sixteen CONTIGUOUS bytes 16 g' .. 16 g' + 15 of that row.
__device__ __forceinline__ void lanegroup_transpose4(unsigned (&r)[4]) {
    u32x2 t = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false);
    r[0] = t[0]; r[2] = t[1];
    t = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false);
    r[1] = t[0]; r[3] = t[1];
    t = __builtin_amdgcn_permlane16_swap(r[0], r[1], false, false);
    r[0] = t[0]; r[1] = t[1];
    t = __builtin_amdgcn_permlane16_swap(r[2], r[3], false, false);
    r[2] = t[0]; r[3] = t[1];
}

template <typename OUT_T, int MT, int FL, int ACT>
__device__ __forceinline__ bool nt_tile_epilogue(f32x4 (&acc)[4][MT], const EpiB16& epi, OUT_T* __restrict__ out, int M, int N,
                                                 int m0, int n0, int wm, int wn, int lane) {
    constexpr int NT_BM = 32 * MT, NT_BN_ = 256;
    constexpr bool OUT_BF16 = std::is_same<OUT_T, bf16_t>::value;
    const int g = lane >> 4, c = lane & 15;
    const bool full = (m0 + NT_BM <= M) && (n0 + NT_BN_ <= N);
    bool widened = false;
    if constexpr (OUT_BF16) {
        if (full) {
            widened = true;
            // lane (g,c), m-tile j, n-tile pair (2ip, 2ip+1).  After v_permlane16_swap the even lane groups hold
            // 8 consecutive n of tile 2ip, the odd groups 8 consecutive n of tile 2ip+1.  Both 64-byte halves of
            // a row's 128-byte line are stored back to back (ip inner) so L2 can merge them.
            const int nst = n0 + wn * 64 + ((g & 1) ? 16 : 0) + 8 * (g >> 1);   // operand column within pair 0
            // Stores go out TRANSPOSED across the wave: in the accumulator layout adjacent lanes are adjacent ROWS
            // (lane = 16*g + c: row c, 16-byte chunk ch(g) of the row's 64 bytes), and a 16-byte store whose
            // neighbouring lanes hit different cache lines runs at 13.7 B/clk per CU, against 50 B/clk when four
            // neighbouring lanes cover 64 contiguous bytes (scripts/ubench_store.hip) -- the epilogue of a tile was
            // ~10k cycles of exactly that.  ds_bpermute (crossbar only, no LDS memory) moves lane 16*g + c to lane
            // 4*c + ch(g): four per store, same source lane for all four dwords.
            const int srow = lane >> 2, sch = lane & 3;
            const int bp_src = 4 * (16 * (((sch & 1) << 1) | (sch >> 1)) + srow);
            const int nst2 = n0 + wn * 64 + 8 * sch;
            auto store_t = [&](bf16_t* dst, int j, int ip, const u32x4& q) {
                u32x4 t;
    #pragma unroll
                for (int d = 0; d < 4; ++d) t[d] = (unsigned)__builtin_amdgcn_ds_bpermute(bp_src, (int)q[d]);
                nt_store16(dst + (long)(m0 + wm * 16 * MT + 16 * j + srow) * N + nst2 + 32 * ip, t);
            };
            // FULL-LINE stores (-DNT_FULL_LINE=1; an experiment that is kept buildable).  Hypothesis: a store instruction that
            // covers only 64 of a line's 128 bytes makes L2 fill the line before merging.  Measured: FETCH_SIZE and time are the
            // same with whole-line stores (profiles/r02_ablation_tile_order_stores.txt), so the fetched excess is weight
            // re-reads, not read-for-ownership.  Form: one instruction writes whole lines: store s covers rows
            // 8s..8s+7 of the m-tile, lane L -> row L>>3, 16-byte chunk L&7 of the wave's 128-byte row.  Chunk k = 4*ip + ch
            // lives in lane (g = ginv(ch), c = row) of pair ip's quad, so first a row_ror:8 DPP move (VALU, not LDS) puts
            // pair 1's quads of rows 0..7 into lanes c >= 8 (and of rows 8..15 into lanes c < 8); then ONE ds_bpermute per
            // dword as before.
            // (variants that also hold a tile's worth of residual / act_u operand quads are at the 256-VGPR limit: they keep
            // the half-line form until their operand staging is slimmed)
            constexpr bool FULL = NT_FULL_LINE && (FL & (F_RES | F_ACTU)) == 0;
            const int frow = lane >> 3, fk = lane & 7, fch = fk & 3;
            const int fg = ((fch & 1) << 1) | (fch >> 1);
            const int bp_full0 = 4 * (16 * fg + frow + ((fk >= 4) ? 8 : 0));        // store 0: rows 0..7
            const int bp_full1 = 4 * (16 * fg + frow + ((fk >= 4) ? 0 : 8));        // store 1: rows 8..15
            const bool lo_half = c < 8;
            auto store_full = [&](bf16_t* dst, int j, const u32x4& q0, const u32x4& q1) {
                u32x4 t0, t1;
    #pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned r8 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)q1[d], 0x128, 0xf, 0xf, false);   // row_ror:8
                    const unsigned a = lo_half ? q0[d] : r8;      // rows 0..7: pair 0 in lanes c < 8, pair 1 in lanes c >= 8
                    const unsigned b = lo_half ? r8 : q0[d];      // rows 8..15: pair 1 in lanes c < 8, pair 0 in lanes c >= 8
                    t0[d] = (unsigned)__builtin_amdgcn_ds_bpermute(bp_full0, (int)a);
                    t1[d] = (unsigned)__builtin_amdgcn_ds_bpermute(bp_full1, (int)b);
                }
                bf16_t* base = dst + (long)(m0 + wm * 16 * MT + 16 * j + frow) * N + n0 + wn * 64 + 8 * fk;
                nt_store16(base, t0);
                nt_store16(base + 8 * (long)N, t1);
            };
            // NB no VMEM load into registers may sit inside the k-loop: the compiler then guards the loop's
            // LDS reads with s_waitcnt vmcnt(0) (register reuse), which drains the operand ring every k-step.
            float4 bia[4];
    #pragma unroll
            for (int i = 0; i < 4; ++i) bia[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    #if NT_BIAS_UPFRONT
            // The four bias quads of this wave's columns are loaded TOGETHER, waited for once, and added into the accumulators in
            // place before anything else.  Left to the compiler, the variants with a second store (GELU + pre-activation) loaded
            // them one at a time between the m-tiles' stores: every such wait then also waited for the stores issued before it
            // (VMEM returns in order) -- two store round trips per tile on the critical path of a VALU-bound epilogue.  Same
            // arithmetic: acc + bias is the first operation on every element either way.
            if constexpr ((FL & F_BIAS) != 0 && (FL & (F_ACT | F_PRE)) != 0) {
                f32x4 b4[4];
    #pragma unroll
                for (int i = 0; i < 4; ++i) b4[i] = *reinterpret_cast<const f32x4*>(epi.bias + n0 + wn * 64 + 4 * g + 16 * i);
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(b4[0]), "+v"(b4[1]), "+v"(b4[2]), "+v"(b4[3]));
    #pragma unroll
                for (int i = 0; i < 4; ++i)
    #pragma unroll
                    for (int j = 0; j < MT; ++j) acc[i][j] += b4[i];
            } else
    #endif
            {
    #pragma unroll
                for (int i = 0; i < 4; ++i)
                    if constexpr ((FL & F_BIAS) != 0) bia[i] = load4(epi.bias + n0 + wn * 64 + 4 * g + 16 * i);
            }
            // PHASED form for the plain / bias epilogues (NT_FAST_EPI): first every tuple is rounded, packed and widened (VALU
            // only: the accumulators die as the 64 packed registers fill -- the fragment registers are free here), then the
            // ds_bpermute transpositions go out sixteen at a time with the four stores of a group behind them.  Left to the
            // scheduler the loop below is one tuple at a time: 20 waits for 64 bpermutes, each exposing the crossbar latency.
            if constexpr (NT_FAST_EPI && (FL & ~F_BIAS) == 0 && !FULL) {
                typedef __attribute__((ext_vector_type(2))) float f32x2_;
                u32x4 qa[MT][2];
    #pragma unroll
                for (int j = 0; j < MT; ++j) {
    #pragma unroll
                    for (int ip = 0; ip < 2; ++ip) {
                        unsigned plo[2], phi[2];
    #pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int i = 2 * ip + h;
                            f32x2_ lo = {acc[i][j][0], acc[i][j][1]}, hi = {acc[i][j][2], acc[i][j][3]};
                            if constexpr ((FL & F_BIAS) != 0) {
                                lo += (f32x2_){bia[i].x, bia[i].y};
                                hi += (f32x2_){bia[i].z, bia[i].w};
                            }
                            plo[h] = pack2(lo[0], lo[1]);
                            phi[h] = pack2(hi[0], hi[1]);
                        }
                        const u32x2 a = __builtin_amdgcn_permlane16_swap(plo[0], plo[1], false, false);
                        const u32x2 b = __builtin_amdgcn_permlane16_swap(phi[0], phi[1], false, false);
                        qa[j][ip] = (u32x4){a[0], b[0], a[1], b[1]};
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                for (int j2 = 0; j2 < MT; j2 += 2) {
                    u32x4 t[2][2];
    #pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
    #pragma unroll
                        for (int ip = 0; ip < 2; ++ip)
    #pragma unroll
                            for (int d = 0; d < 4; ++d)
                                t[jj][ip][d] = (unsigned)__builtin_amdgcn_ds_bpermute(bp_src, (int)qa[j2 + jj][ip][d]);
    #pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
    #pragma unroll
                        for (int ip = 0; ip < 2; ++ip)
                            nt_store16(out + (long)(m0 + wm * 16 * MT + 16 * (j2 + jj) + srow) * N + nst2 + 32 * ip, t[jj][ip]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                return true;
            }
            // ALL of the tile's operand loads are issued up front (the fragment registers are dead here): with a
            // one-m-tile look-ahead every m-tile paid a full memory latency (20k cycles per tile, in-kernel profile)
            // Operand loads are transposed the same way, for the same reason (a 16-byte load whose neighbouring
            // lanes hit different rows: 10.8 B/clk per CU; eight neighbouring lanes on one 128-byte line: 22.9):
            // load 0 of an m-tile fetches rows 0..7, load 1 rows 8..15, lane L -> row L>>3, chunk L&7 of the wave's
            // 128 bytes; lane (g,c) then pulls chunk 4*ip + ch(g) of row c from lane 8*(c&7) + 4*ip + ch(g) of load
            // c>>3 (two ds_bpermute + a select per dword).
            u32x4 uq[(FL & F_ACTU) ? MT : 1][2], rq[(FL & F_RES) ? MT : 1][2];
            const int lrow = lane >> 3, lch = lane & 7;
            const int chg = 2 * (g & 1) + (g >> 1);
            const int bp_ld = 4 * (8 * (c & 7) + chg);            // + 16 for ip = 1
            const bool lo_rows = c < 8;
            auto fetch = [&](int j, u32x4* uqj, u32x4* rqj) {
    #pragma unroll
                for (int hr = 0; hr < 2; ++hr) {
                    const long so = (long)(m0 + wm * 16 * MT + 16 * j + 8 * hr + lrow) * N + n0 + wn * 64 + 8 * lch;
                    if constexpr ((FL & F_ACTU) != 0) uqj[hr] = *reinterpret_cast<const u32x4*>(epi.act_u + so);
                    if constexpr ((FL & F_RES) != 0) rqj[hr] = *reinterpret_cast<const u32x4*>(epi.residual + so);
                }
            };
            auto untranspose = [&](const u32x4* ld, int ip) {
                u32x4 q;
    #pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned a = (unsigned)__builtin_amdgcn_ds_bpermute(bp_ld + 16 * ip, (int)ld[0][d]);
                    const unsigned b = (unsigned)__builtin_amdgcn_ds_bpermute(bp_ld + 16 * ip, (int)ld[1][d]);
                    q[d] = lo_rows ? a : b;
                }
                return q;
            };
            if constexpr ((FL & (F_ACTU | F_RES)) != 0) {
    #pragma unroll
                for (int j = 0; j < MT; ++j) fetch(j, uq[(FL & F_ACTU) ? j : 0], rq[(FL & F_RES) ? j : 0]);
            }
            // the 8-bit GELU' tile: 64 bytes per row -- ONE 16-byte load per m-tile and lane (lane L: row L >> 2, bytes 16 (L & 3) ..),
            // four neighbouring lanes on one row; all m-tiles up front like the other operands
            u32x4 g8q[(FL & F_ACTU8) ? MT : 1];
            if constexpr ((FL & F_ACTU8) != 0) {
    #pragma unroll
                for (int j = 0; j < MT; ++j)
                    g8q[j] = *reinterpret_cast<const u32x4*>(epi.actu8 + (long)(m0 + wm * 16 * MT + 16 * j + (lane >> 2)) * N + n0 + wn * 64 +
                                                             16 * (lane & 3));
            }
    #pragma unroll
            for (int j = 0; j < MT; ++j) {
                const long rowo = (long)(m0 + wm * 16 * MT + 16 * j + c) * N;
                u32x4 qo[2], qp[2];
                unsigned g8w[4] = {0u, 0u, 0u, 0u};       // per n-tile i: the four GELU' bytes of this lane's quad
                if constexpr ((FL & F_ACTU8) != 0) {
                    // lane (g, c) <- lane 4 c + g: the sixteen bytes 16 g .. of row c; then back to the accumulator layout
    #pragma unroll
                    for (int d = 0; d < 4; ++d) g8w[d] = (unsigned)__builtin_amdgcn_ds_bpermute(4 * (4 * c + g), (int)g8q[j][d]);
                    lanegroup_transpose4(g8w);
                }
    #pragma unroll
                for (int ip = 0; ip < 2; ++ip) {
                    unsigned plo[2], phi[2], ulo[2] = {0u, 0u}, uhi[2] = {0u, 0u};
                    u32x2 ua = {0u, 0u}, ub = {0u, 0u}, ra = {0u, 0u}, rb = {0u, 0u};
                    if constexpr ((FL & F_ACTU8) != 0) ua = (u32x2){g8w[2 * ip], g8w[2 * ip + 1]};
                    if constexpr ((FL & F_ACTU) != 0) {
                        const u32x4 q = untranspose(uq[j], ip);
                        ua = __builtin_amdgcn_permlane16_swap(q[0], q[2], false, false);
                        ub = __builtin_amdgcn_permlane16_swap(q[1], q[3], false, false);
                    }
                    if constexpr ((FL & F_RES) != 0) {
                        const u32x4 q = untranspose(rq[j], ip);
                        ra = __builtin_amdgcn_permlane16_swap(q[0], q[2], false, false);
                        rb = __builtin_amdgcn_permlane16_swap(q[1], q[3], false, false);
                    }
                    float4 v[2], bb[2];
    #pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int i = 2 * ip + h;
                        v[h] = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                        bb[h] = bia[i];
                    }
                    const unsigned ul[2] = {ua[0], ua[1]}, uh[2] = {ub[0], ub[1]}, rl[2] = {ra[0], ra[1]}, rh[2] = {rb[0], rb[1]};
                    // (bias already inside the accumulators when it was added up front)
                    constexpr int FLM = (NT_BIAS_UPFRONT && (FL & F_BIAS) != 0 && (FL & (F_ACT | F_PRE)) != 0) ? (FL & ~F_BIAS) : FL;
                    epi_math2<FLM, ACT>(v, bb, ul, uh, rl, rh, ulo, uhi);
                    if constexpr ((FL & F_PRE8) != 0) { g8w[2 * ip] = ulo[0]; g8w[2 * ip + 1] = ulo[1]; }
    #pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        plo[h] = pack2(v[h].x, v[h].y);
                        phi[h] = pack2(v[h].z, v[h].w);
                    }
                    {
                        const u32x2 a = __builtin_amdgcn_permlane16_swap(plo[0], plo[1], false, false);
                        const u32x2 b = __builtin_amdgcn_permlane16_swap(phi[0], phi[1], false, false);
                        u32x4 q = {a[0], b[0], a[1], b[1]};
                        qo[ip] = q;
                        if constexpr (!FULL) {
    #ifdef NT_NOSTORE
                            if (q[0] == 0x12345678u)
    #endif
                            store_t(out, j, ip, q);
                        }
                    }
                    if constexpr ((FL & F_PRE) != 0) {
                        const u32x2 a = __builtin_amdgcn_permlane16_swap(ulo[0], ulo[1], false, false);
                        const u32x2 b = __builtin_amdgcn_permlane16_swap(uhi[0], uhi[1], false, false);
                        u32x4 q = {a[0], b[0], a[1], b[1]};
                        qp[ip] = q;
                        if constexpr (!FULL) store_t(epi.preact, j, ip, q);
                    }
                }
                if constexpr (FULL) {
    #ifdef NT_NOSTORE
                    if (qo[0][0] == 0x12345678u)
    #endif
                    store_full(out, j, qo[0], qo[1]);
                    if constexpr ((FL & F_PRE) != 0) store_full(epi.preact, j, qp[0], qp[1]);
                }
                if constexpr ((FL & F_PRE8) != 0) {
                    // group g now gets the row's sixteen contiguous bytes 16 g ..; then lane L <- lane 16 (L & 3) + (L >> 2), so that
                    // four neighbouring lanes store one row's 64 bytes (the store-pattern argument of store_t)
                    lanegroup_transpose4(g8w);
                    u32x4 t;
    #pragma unroll
                    for (int d = 0; d < 4; ++d) t[d] = (unsigned)__builtin_amdgcn_ds_bpermute(4 * (16 * (lane & 3) + (lane >> 2)), (int)g8w[d]);
                    nt_store16(epi.pre8 + (long)(m0 + wm * 16 * MT + 16 * j + (lane >> 2)) * N + n0 + wn * 64 + 16 * (lane & 3), t);
                }
            }
        }
    }
    if (!widened) {
        // partial tiles and fp32 output: per-quad path with bounds checks (8-byte operand loads)
    #pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int m = m0 + wm * 16 * MT + 16 * j + c;
    #pragma unroll
            for (int ip = 0; ip < 2; ++ip) {
                float4 v[2], bb[2];
                unsigned u_lo[2] = {0u, 0u}, u_hi[2] = {0u, 0u}, r_lo[2] = {0u, 0u}, r_hi[2] = {0u, 0u};
                unsigned pre_lo[2] = {0u, 0u}, pre_hi[2] = {0u, 0u};
                bool ok[2];
                // operand loads are unconditional at clamped addresses (no divergent control flow around VMEM
                // loads: see the note on s_waitcnt vmcnt(0) above); only the stores are predicated
    #pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = 2 * ip + h;
                    const int n = n0 + wn * 64 + 16 * i + 4 * g;
                    ok[h] = m < M && n < N;
                    const int nc = min(n, N - 4);
                    const long oc = (long)min(m, M - 1) * N + nc;
                    v[h] = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                    bb[h] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if constexpr ((FL & F_BIAS) != 0) bb[h] = load4(epi.bias + nc);
                    if constexpr ((FL & F_ACTU) != 0) {
                        const u32x2 q = *reinterpret_cast<const u32x2*>(epi.act_u + oc);
                        u_lo[h] = q[0];
                        u_hi[h] = q[1];
                    }
                    if constexpr ((FL & F_RES) != 0) {
                        const u32x2 q = *reinterpret_cast<const u32x2*>(epi.residual + oc);
                        r_lo[h] = q[0];
                        r_hi[h] = q[1];
                    }
                    if constexpr ((FL & F_ACTU8) != 0) u_lo[h] = *reinterpret_cast<const unsigned*>(epi.actu8 + oc);
                }
                epi_math2<FL, ACT>(v, bb, u_lo, u_hi, r_lo, r_hi, pre_lo, pre_hi);
    #pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (!ok[h]) continue;
                    const int i = 2 * ip + h;
                    const long o = (long)m * N + n0 + wn * 64 + 16 * i + 4 * g;
                    if constexpr ((FL & F_PRE) != 0) {
                        u32x2 q = {pre_lo[h], pre_hi[h]};
                        *reinterpret_cast<u32x2*>(epi.preact + o) = q;
                    }
                    if constexpr ((FL & F_PRE8) != 0) *reinterpret_cast<unsigned*>(epi.pre8 + o) = pre_lo[h];
                    store4(out + o, v[h]);
                }
            }
        }
        // tell the compiler's wait-count pass that nothing loaded on this (rare) path is still pending: a load whose
        // use was sunk into a predicated store block otherwise reaches the loop back-edge "in flight" and the
        // k-loop gets s_waitcnt vmcnt(0) in front of its first register write
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt/lgkmcnt untouched
    }
    return widened;
}
