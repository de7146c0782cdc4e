// In-kernel cycle accounting hooks of the ping-pong kernels (gemm_nt_pp.h, gemm_bf16_tn.hip): tick() restarts the clock,
// lap<I>() charges the time since the last hook to counter I, flush() adds the wave's counters to the kernel's debug array.  This
// one is the default build's: nothing.  (gemm_bf16_nt8p.hip and gemm_bf16_tn.hip have the counting ones behind -DPP_PROFILE.)
#pragma once
#include <hip/hip_runtime.h>      // __device__, __forceinline__

struct PpNoProbe {
    __device__ __forceinline__ void tick() {}
    template <int I> __device__ __forceinline__ void lap() {}
    __device__ __forceinline__ void flush(int, int) {}
};
// counter slots of a wave.  Slot 1 is the tile epilogues in the NT kernels and the time up to the end of the step loop in the
// wgrad kernel (which has one tile and one epilogue per block); slot 0 is the total, slot 7 the number of steps.
enum { PP_T_EPI = 1, PP_T_LOOP = 1, PP_T_L = 2, PP_T_LWAIT = 3, PP_T_C = 4, PP_T_VMCNT = 5, PP_T_CBAR = 6 };
