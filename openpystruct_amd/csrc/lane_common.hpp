// Lane-level helpers shared by the library's kernels: bf16 conversion, wave and workgroup sums, DPP moves, the late kernarg pointer.
// Device code only: beam_math.hpp and beam_adjoint.hpp, which g++ also compiles (tests/csrc), do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace opsamd {

// the bits of a finite float rounded to nearest even at bit 16: the upper half is the bfloat16
__device__ __forceinline__ uint32_t bf16_rne_bits(uint32_t u) { return u + 0x7fffu + ((u >> 16) & 1u); }
// float -> bfloat16, round to nearest even; NaN stays NaN
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// the value a float has after a store to bf16 and a load back
__device__ __forceinline__ float bf16_round(float f) { return bf16_to_f32(f32_to_bf16(f)); }

// butterfly sum over LANES lanes (64: the wave; 32: each half wave on its own): every lane gets its group's total
template <int LANES = 64, class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int s = LANES / 2; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// LDS operations of one wave execute in order; this pins the compiler and lands earlier reads (the frame kernels' hand-over between
// the lanes of one wave: frame_wave.hpp, frame_resolve.hpp, frame_groups.hip)
__device__ __forceinline__ void fw_fence() {
  __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
  __asm__ volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Sums NV doubles over a workgroup of NW waves (s_red: [NW][NV] doubles of LDS, free after the first barrier); ALL: every thread gets the
// totals, otherwise thread 0 only
template <int NW, bool ALL, int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* s_red) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) s_red[wave * NV + k] = v[k];
  __syncthreads();
  if (ALL || threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      double t = 0.0;
      for (int w = 0; w < NW; ++w) t += s_red[w * NV + k];
      v[k] = t;
    }
}

// DPP move (quad_perm, row_shr / row_shl, row_ror, row_half_mirror, ...: no LDS; lanes shifted in from outside the row read 0)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double x) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// The launch's argument block T, read AT THE POINT OF USE from the kernarg segment (constant memory: scalar loads).  A large struct held in
// scalar registers for the whole kernel spills them; the empty asm makes the pointer opaque so that the field loads stay behind it.
// ARGOFF: byte offset of the block in the segment (a kernel may carry two).
template <class T>
using kernarg_ptr = const __attribute__((opencl_constant)) T*;
template <class T, int ARGOFF = 0>
__device__ __forceinline__ kernarg_ptr<T> late_args() {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();
  __asm__ volatile("" : "+s"(p));
  return (kernarg_ptr<T>)((const __attribute__((opencl_constant)) char*)p + ARGOFF);
}

}  // namespace opsamd
